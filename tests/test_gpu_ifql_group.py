"""GPU: IFQL agent groups (fql_ifql_group_*, IFQLAgentGroup).  A member advanced by the group's fused program and sampled by the fused
calls must be bitwise where its standalone twin is (same seed, expectile, parameters, dataset and rows): fusing changes which launch a
task rides in, never its arithmetic.  The standalone agent is pinned to the fp64 restatement at these shapes by tests/test_gpu_ifql.py and
tests/test_gpu_ifql_paths.py, so the twin is a checked reference and no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import ifql_cases as IK
from tests.util import leaf_dict, randomize_params

pytestmark = pytest.mark.gpu


def _state(a):
    """Every array and counter of an agent: parameters (the target critic among them), both Adam moments, the step counters."""
    a.synchronize()
    opt = a.get_opt_state()
    out = {f'params/{k}': v for k, v in leaf_dict(a.get_params()).items()}
    for part in ('mu', 'nu'):
        out.update({f'{part}/{k}': v for k, v in leaf_dict(opt[part]).items()})
    return out, (opt['count'], opt['step'])


def _assert_same_state(a, b, what=''):
    (sa, ca), (sb, cb) = _state(a), _state(b)
    assert sa.keys() == sb.keys() and ca == cb, (what, ca, cb)
    assert any(k.startswith('params/modules_target_critic') for k in sa)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f'{what} {k}')
    assert a.read_info() == b.read_info(), what


def _setup(K, B, hidden, od=29, ad=8, expectiles=None, ds_seed=7, seeds=None, **kw):
    """A group of K members and their standalone twins on one dataset: member and twin share the create seed, the expectile and the
    randomised parameters; members differ from each other in all three unless the caller says otherwise."""
    import fql_amd
    hidden = (hidden,) * 4 if isinstance(hidden, int) else tuple(hidden)
    cfg = IK.config(hidden, hidden, B, **kw)
    ds = IK.dataset(od, ad, B, ds_seed)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
    seeds = [3 + i for i in range(K)] if seeds is None else list(seeds)
    expectiles = [float(cfg['expectile'])] * K if expectiles is None else list(expectiles)
    group = fql_amd.IFQLAgentGroup.create(seeds, ex_o, ex_a, cfg, expectiles=expectiles)
    group.upload_dataset(ds)
    twins = []
    for i in range(K):
        t = fql_amd.IFQLAgent.create(seeds[i], ex_o, ex_a, dict(cfg, expectile=expectiles[i]))
        p = randomize_params(t.get_params(), 100 + i)
        t.set_params(p)
        group.members[i].set_params(p)
        t.upload_dataset(ds)
        twins.append(t)
    assert all(type(m) is fql_amd.IFQLAgent for m in group.members)
    return cfg, ds, group, twins


def _step(group, twins, B, want_info=False, idxs=None):
    infos = group.update_from_dataset(want_info=want_info, idxs=idxs)
    want = [t.update_from_dataset(B, want_info=want_info, idxs=None if idxs is None else idxs[i])[1] for i, t in enumerate(twins)]
    return infos, want


def _assert_infos(infos, want, what):
    from fql_amd.ifql import IFQL_INFO_KEYS
    assert len(infos) == len(want)
    for i, (g, w) in enumerate(zip(infos, want)):
        g, w = g.to_dict(), w.to_dict()
        assert tuple(g) == IFQL_INFO_KEYS == tuple(w) and len(g) == 12, (what, i)
        for k in g:
            np.testing.assert_array_equal(np.asarray(g[k]), np.asarray(w[k]), err_msg=f'{what} member {i} {k}')


def _check(group, twins, what=''):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'{what} member {i}')


# ---- 1. twins on device-drawn rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, B, H, steps, expectiles', [
    (3, 64, 64, 8, [0.7, 0.8, 0.9]),
    (2, 256, 512, 6, None),
    (8, 16, 64, 6, None),
    (1, 64, 64, 6, None),
], ids=['K3-B64-H64-expectiles', 'K2-B256-H512', 'K8-B16-H64', 'K1'])
def test_ifql_group_equals_standalone_twins_device_rng(K, B, H, steps, expectiles):
    """After every step the 12 infos of every member against its twin; at the end parameters, both Adam moments, the target critic and
    the step counters."""
    cfg, ds, group, twins = _setup(K, B, H, expectiles=expectiles)
    for step in range(steps):
        infos, want = _step(group, twins, B, want_info=True)
        _assert_infos(infos, want, f'step {step}')
    _check(group, twins)
    assert group.members[0].get_opt_state()['count'] == steps
    if expectiles:
        assert [m.config['expectile'] for m in group.members] == expectiles
    group.close()


# ---- 2. the expectile is the one thing that differs --------------------------------------------------------------------------------------
def test_ifql_group_expectile_alone_moves_the_value_loss():
    """Two members in one state (create seed, parameters) on one set of rows, expectiles 0.6 and 0.9: the value losses differ; the critic
    loss (its target is value(next_obs) with the stored parameters) and the actor loss (same x_0, t) are equal on the first step."""
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, B, 64, expectiles=[0.6, 0.9], seeds=[5, 5])
    p = randomize_params(twins[0].get_params(), 77)
    for a in list(group.members) + twins:
        a.set_params(p)
    idx = np.random.default_rng(3).integers(0, len(ds['observations']), size=B)
    idxs = np.stack([idx, idx])
    infos, want = _step(group, twins, B, want_info=True, idxs=idxs)
    _assert_infos(infos, want, 'first step')
    a, b = infos[0].to_dict(), infos[1].to_dict()
    assert a['value/value_loss'] != b['value/value_loss']
    assert a['value/v_mean'] == b['value/v_mean']
    for k in ('critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min', 'actor/actor_loss'):
        assert a[k] == b[k], k
    _check(group, twins)
    group.close()


# ---- 3. kernel-path shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['b272', 'b512_mixed', 'b544_h64', 'b1040_h64', 'wide1024', 'obs600', 'no_ln_h512', 'act16', 'b16'])
def test_ifql_group_equals_standalone_twins_on_every_path(case):
    od, ad, B, actor, value, kw, seed = IK.PATHS[case]
    assert actor == value
    cfg, ds, group, twins = _setup(2, B, actor, od=od, ad=ad, ds_seed=seed, expectiles=[0.7, 0.9], **kw)
    for step in range(2):
        infos, want = _step(group, twins, B, want_info=True)
        _assert_infos(infos, want, f'{case} step {step}')
    _check(group, twins, case)
    group.close()


# ---- 4. explicit rows --------------------------------------------------------------------------------------------------------------------
def test_ifql_group_explicit_rows_host_and_device():
    """idxs [K, B] as a host array (the group's own stream) and as a CUDA tensor (torch's current stream), alternating with no
    synchronize; every member's rows include N - 1."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, 64, expectiles=[0.7, 0.8, 0.9])
    rng = np.random.default_rng(13)
    N = len(ds['observations'])
    for step in range(6):
        idxs = rng.integers(0, N, size=(K, B))
        idxs[:, step % B] = N - 1
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 3 == 0 else idxs, want_info=True)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, f'step {step}')
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), N, np.int64))
    _check(group, twins)
    group.close()


# ---- 5. info12xk through the C ABI ---------------------------------------------------------------------------------------------------------
def test_ifql_group_infos_through_the_c_abi():
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's 12 infos in
    read_info()'s key order; nothing is written behind them."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, 64, expectiles=[0.7, 0.8, 0.9])
    lib = group._lib
    for step in range(4):
        if step % 2 == 0:
            host = np.full((K * 12 + 3,), np.nan, np.float32)
            group._check(lib.fql_ifql_group_update_from_dataset(group._g, None, B, host.ctypes.data, None))
            got, tail = host[:K * 12].reshape(K, 12), host[K * 12:]
        else:
            dev = torch.full((K * 12 + 3,), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_ifql_group_update_from_dataset(group._g, None, B, dev.data_ptr(), None))
            group.synchronize()
            got, tail = dev.cpu().numpy()[:K * 12].reshape(K, 12), dev.cpu().numpy()[K * 12:]
        assert np.isnan(tail).all()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_from_dataset(B)
            assert got[i].tolist() == list(m.read_info().values()), (step, i)
            assert got[i].tolist() == list(t.read_info().values()), (step, i)
    _check(group, twins)
    group.close()


# ---- 6. the members' own work between group updates, no synchronize ------------------------------------------------------------------------
def test_ifql_group_member_work_between_group_updates(tmp_path):
    """Between group updates and with no synchronize anywhere: a member's own update_from_dataset (on the engine's queues),
    sample_actions, total_loss, network.select('value'), get_params / set_params and a checkpoint round trip.  The group update is
    ordered behind them, and they behind it; the fused sampler sees the group's last update."""
    from fql_amd import checkpoint
    K, B, od, ad = 3, 64, 29, 8
    cfg, ds, group, twins = _setup(K, B, 64, expectiles=[0.7, 0.8, 0.9])
    ms = group.members
    batch = O.sample_batch(ds, np.random.default_rng(2).integers(0, len(ds['observations']), size=B))
    nz = O.make_noise(B, ad, 5)
    noise = {'x0': nz['x0'], 't': nz['t']}
    obs = ds['observations'][:7]
    for rnd in range(2):
        _step(group, twins, B)
        ms[0].update_from_dataset(B)                    # the member's own update on its default path
        twins[0].update_from_dataset(B)
        ms[1].update(batch, noise=noise)                # a host batch with explicit noise
        twins[1].update(batch, noise=noise)
        _step(group, twins, B)
        for i, (m, t) in enumerate(zip(ms, twins)):     # straight after a group update: every read sees it
            np.testing.assert_array_equal(m.sample_actions(obs, seed=11), t.sample_actions(obs, seed=11), err_msg=f'round {rnd} member {i}')
            assert m.total_loss(batch, noise=noise) == t.total_loss(batch, noise=noise), (rnd, i)
            np.testing.assert_array_equal(m.network.select('value')(obs), t.network.select('value')(obs), err_msg=f'value round {rnd} member {i}')
            _step(group, twins, B)
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
        # the fused sampler straight after a group update
        got = group.sample_actions(obs, seed=21 + rnd)
        for i, t in enumerate(twins):
            np.testing.assert_array_equal(got[i], t.sample_actions(obs, seed=21 + rnd), err_msg=f'fused sampler round {rnd} member {i}')
        # a set_params between group updates is seen by the next one
        p = randomize_params(twins[2].get_params(), 55 + rnd)
        ms[2].set_params(p)
        twins[2].set_params(p)
        _step(group, twins, B)
        # a checkpoint of a grouped member, restored into another grouped member and into that one's twin
        d = tmp_path / f'r{rnd}'
        d.mkdir()
        checkpoint.save_agent(ms[0], str(d), 1)
        checkpoint.restore_agent(ms[1], str(d), 1)
        checkpoint.restore_agent(twins[1], str(d), 1)
        _step(group, twins, B)
    _check(group, twins)
    group.close()


# ---- 7. the fused best-of-N sampler ---------------------------------------------------------------------------------------------------------
def _sampler_setup(K, H, N, od=29, ad=8):
    cfg, ds, group, twins = _setup(K, 64, H, od=od, ad=ad, num_samples=N)
    return group, twins


def _bon_rows(K, n, N, od, ad, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n, od)).astype(np.float32), (2.0 * rng.standard_normal((K, n, N, ad))).astype(np.float32)


@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('N', [1, 7, 65])
def test_ifql_group_sample_actions_equal_the_members_own(K, N):
    """N = 65 needs a second trip of the selection loop's 64 lanes; n = 590 at N = 7 crosses the 4096-sample-row chunk edge (585
    observations per chunk), so the second chunk's row keys matter."""
    import torch
    od, ad = 29, 8
    group, twins = _sampler_setup(K, 64, N)
    ms = group.members
    before = [_state(m) for m in ms]
    side = torch.cuda.Stream()
    for n in (1, 10, 37) + ((590,) if N == 7 else ()):
        obs, z = _bon_rows(K, n, N, od, ad, 17 + n)
        got = group.sample_actions(obs, noises=z)
        assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i]), err_msg=f'n {n} noises member {i}')
            np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i]), err_msg=f'n {n} noises twin {i}')
        seeds = [50 + n + i for i in range(K)]
        got = group.sample_actions(obs, seed=seeds)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=seeds[i]), err_msg=f'n {n} seeds member {i}')
        got = group.sample_actions(obs, seed=9)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=9), err_msg=f'n {n} one seed member {i}')
        if n > 37:
            continue
        # one shared block of rows against the same rows tiled
        shared = group.sample_actions(obs[0], seed=seeds)
        np.testing.assert_array_equal(shared, group.sample_actions(np.tile(obs[:1], (K, 1, 1)), seed=seeds))
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].sample_actions(obs[0], seed=seeds[i]))
        # CUDA tensors on a side stream
        with torch.cuda.stream(side):
            to, tz = torch.from_numpy(obs).cuda(), torch.from_numpy(z).cuda()
            tg = group.sample_actions(to, noises=tz)
            assert tg.is_cuda and tuple(tg.shape) == (K, n, ad)
            want = [ms[i].sample_actions(to[i], noises=tz[i]) for i in range(K)]
            ts = group.sample_actions(to, seed=seeds)
        side.synchronize()
        for i in range(K):
            np.testing.assert_array_equal(tg[i].cpu().numpy(), want[i].cpu().numpy(), err_msg=f'n {n} cuda member {i}')
            np.testing.assert_array_equal(tg[i].cpu().numpy(), ms[i].sample_actions(obs[i], noises=z[i]))
            np.testing.assert_array_equal(ts[i].cpu().numpy(), ms[i].sample_actions(obs[i], seed=seeds[i]))
    if N == 7:   # the second chunk's first observation draws its own noise: the same observation in every row, seeded
        same = np.repeat(obs[:, :1], 590, axis=1)
        drawn = group.sample_actions(same, seed=[5, 6, 7][:K])
        for i in range(K):
            np.testing.assert_array_equal(drawn[i], ms[i].sample_actions(same[i], seed=5 + i), err_msg=f'same rows member {i}')
    # unseeded: member i's counter advances once per fused call, as by its own call; the twin (same seed, same parameters) draws the same
    o7 = _bon_rows(K, 7, N, od, ad, 4)[0]
    for r in range(3):
        calls = [m._sample_calls for m in ms]
        got = group.sample_actions(o7)
        assert [m._sample_calls for m in ms] == [c + 1 for c in calls]
        tw = []
        for i in range(K):
            tw.append(twins[i].sample_actions(o7[i]))
            assert ms[i]._sample_calls == twins[i]._sample_calls
            np.testing.assert_array_equal(got[i], tw[i], err_msg=f'unseeded round {r} member {i}')
    # no parameter or optimizer state changed
    for i, m in enumerate(ms):
        (arrays, counters), (arrays0, counters0) = _state(m), before[i]
        assert counters == counters0
        for k in arrays:
            np.testing.assert_array_equal(arrays[k], arrays0[k], err_msg=f'member {i} {k}')
    group.close()


def test_ifql_group_sample_actions_hidden_512_padded_action_width():
    """obs 69, act 21 (padded action width 32), hidden 512, num_samples 32, n = 10."""
    K, N, n = 2, 32, 10
    od, ad, actor, value = IK.SAMPLER_SHAPE
    group, twins = _sampler_setup(K, actor, N, od=od, ad=ad)
    ms = group.members
    obs, z = _bon_rows(K, n, N, od, ad, 23)
    got = group.sample_actions(obs, noises=z)
    drawn = group.sample_actions(obs, seed=[8, 9])
    for i in range(K):
        np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises member {i}')
        np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises twin {i}')
        np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=8 + i), err_msg=f'seeds twin {i}')
    zf = np.ascontiguousarray(z[:, :, 0])
    flow = group.compute_flow_actions(obs, zf)
    for i in range(K):
        np.testing.assert_array_equal(flow[i], twins[i].compute_flow_actions(obs[i], zf[i]), err_msg=f'flow twin {i}')
    group.close()


# ---- 8. the fused flow --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [2, 3])
def test_ifql_group_flow_actions_equal_the_members_own(K):
    import torch
    od, ad, N = 29, 8, 7
    group, twins = _sampler_setup(K, 64, N)
    ms = group.members
    for n in (1, 10, 37):
        obs, z = _bon_rows(K, n, 1, od, ad, 31 + n)
        z = np.ascontiguousarray(z[:, :, 0])
        got = group.compute_flow_actions(obs, z)
        assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].compute_flow_actions(obs[i], z[i]), err_msg=f'n {n} member {i}')
            np.testing.assert_array_equal(got[i], twins[i].compute_flow_actions(obs[i], z[i]), err_msg=f'n {n} twin {i}')
        shared = group.compute_flow_actions(obs[0], z)
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].compute_flow_actions(obs[0], z[i]))
        to, tz = torch.from_numpy(obs).cuda(), torch.from_numpy(z).cuda()
        tg = group.compute_flow_actions(to, tz)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(tg.cpu().numpy(), got)
        # the two calls share each member's workspace of that row count: best of N at the same padded rows in between
        bo, bz = _bon_rows(K, n, N, od, ad, 5)
        best = group.sample_actions(bo, noises=bz)
        np.testing.assert_array_equal(group.compute_flow_actions(obs, z), got)
        for i in range(K):
            np.testing.assert_array_equal(best[i], twins[i].sample_actions(bo[i], noises=bz[i]))
    with pytest.raises(ValueError):
        group.compute_flow_actions(obs, None)
    group.close()


# ---- 9. launch counts ---------------------------------------------------------------------------------------------------------------------
def test_ifql_group_launch_counts_do_not_depend_on_k():
    """The fused update has a member's launch count, whatever K.  A best-of-N chunk is repeat, the Euler flow, qin, the critic pair and
    select: 3 launches beside the two programs.  The flow is flow_steps passes of a chain of Dense layers each of which reads the one
    before (hidden layers + head: one launch per layer); the two critics read the same rows and do not depend on each other, so each
    layer of the pair is one launch.  A flow call is assemble, the flow, extract."""
    B, H = 16, 64
    counts = set()
    for K in (1, 2, 4):
        cfg, ds, group, twins = _setup(K, B, H)
        u, s, f = group.launches()
        assert u == twins[0].stats()['launches_per_update'] == group.members[0].stats()['launches_per_update'], K
        counts.add((u, s, f))
        group.close()
    layers, fs = len(cfg['actor_hidden_dims']) + 1, int(cfg['flow_steps'])
    assert len(counts) == 1
    u, s, f = counts.pop()
    assert f == 2 + fs * layers
    assert s == 3 + fs * layers + (len(cfg['value_hidden_dims']) + 1)


# ---- 10. refusals and release ---------------------------------------------------------------------------------------------------------------
def test_ifql_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    B, od, ad = 64, 29, 8
    cfg = IK.config((64,) * 4, (64,) * 4, B, num_samples=4)
    ds = IK.dataset(od, ad, B, 1)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]

    def create(members, fn=lib.fql_ifql_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def ifql(seed, **kw):
        return fql_amd.IFQLAgent.create(seed, ex_o, ex_a, dict(cfg, **kw))

    a, twin_a = ifql(0), ifql(0)
    fq_cfg = fql_amd.get_config()
    fq_cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    f0, f1 = fql_amd.FQLAgent.create(0, ex_o, ex_a, fq_cfg), fql_amd.FQLAgent.create(1, ex_o, ex_a, fq_cfg)
    rc, g = create([a, f0])
    assert rc == _cabi.FQL_E_STATE and not g.value and b'FQL' in lib.fql_last_error(None)
    more, slow, wide, steps, other_b = (ifql(1, num_samples=5), ifql(2, lr=1e-4), ifql(3, actor_hidden_dims=(128,) * 4, value_hidden_dims=(128,) * 4),
                                        ifql(4, flow_steps=5), ifql(6, batch_size=32))
    for bad in (more, slow, wide, steps, other_b):
        rc, g = create([a, bad])
        assert rc == _cabi.FQL_E_INVALID and not g.value, lib.fql_last_error(None)
        assert b'member 1' in lib.fql_last_error(None)
        if bad is not other_b:
            assert b'seed and expectile' in lib.fql_last_error(None)
    assert create([a, a])[0] == _cabi.FQL_E_INVALID
    rc, g = create([a, ifql(9)], fn=lib.fql_group_create)          # fql_group_create keeps refusing IFQL handles
    assert rc == _cabi.FQL_E_STATE and not g.value
    b, twin_b = ifql(5, expectile=0.7), ifql(5, expectile=0.7)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID and b'already belongs' in lib.fql_last_error(None)
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # every other kind's group calls on an IFQL group name the IFQL call; the IFQL calls on an FQL group name the FQL call
    o, out = np.zeros((2, 1, od), np.float32), np.zeros((2, 1, ad), np.float32)
    z, zn, seeds, v = np.zeros((2, 1, ad), np.float32), np.zeros((2, 1, 4, ad), np.float32), (C.c_uint64 * 2)(1, 2), C.c_int64(-1)
    w, la = np.ones((2, 1), np.float32), (C.c_int64 * 4)(-1, -1, -1, -1)
    for call, name in ((lambda: lib.fql_group_update_from_dataset(g, None, B, None, None), b'fql_ifql_group_update_from_dataset'),
                     (lambda: lib.fql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, out.ctypes.data, None), b'fql_ifql_group_sample_actions'),
                     (lambda: lib.fql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None), b'fql_ifql_group_flow_actions'),
                     (lambda: lib.fql_group_sample_stats(g, 0, C.byref(v)), b'fql_ifql_group_stats'),
                     (lambda: lib.fql_rebrac_group_update_from_dataset(g, None, B, 1, None, None), b'fql_ifql_group_update_from_dataset'),
                     (lambda: lib.fql_rebrac_group_sample_actions(g, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None), b'fql_ifql_group_sample_actions'),
                     (lambda: lib.fql_rebrac_group_stats(g, C.byref(v), None, None), b'fql_ifql_group_stats'),
                     (lambda: lib.fql_iqld_group_update_from_dataset(g, None, B, 1, 1, None, None), b'fql_ifql_group_update_from_dataset'),
                     (lambda: lib.fql_iqld_group_sample_actions(g, o.ctypes.data, 1, None, seeds, w.ctypes.data, out.ctypes.data, None), b'fql_ifql_group_sample_actions'),
                     (lambda: lib.fql_iqld_group_stats(g, la, C.byref(v)), b'fql_ifql_group_stats')):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None) and b'IFQL' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1 and list(la) == [-1] * 4
    rc, fg = create([f0, f1], fn=lib.fql_group_create)
    assert rc == _cabi.FQL_OK and fg.value
    for call, name in ((lambda: lib.fql_ifql_group_update_from_dataset(fg, None, B, None, None), b'fql_group_update_from_dataset'),
                     (lambda: lib.fql_ifql_group_sample_actions(fg, o.ctypes.data, 1, zn.ctypes.data, seeds, out.ctypes.data, None), b'fql_group_sample_actions'),
                     (lambda: lib.fql_ifql_group_flow_actions(fg, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None), b'fql_group_flow_actions'),
                     (lambda: lib.fql_ifql_group_stats(fg, C.byref(v), None, None), b'fql_group_sample_stats')):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1
    assert lib.fql_group_destroy(fg) == _cabi.FQL_OK
    assert lib.fql_ifql_group_update_from_dataset(g, None, 32, None, None) == _cabi.FQL_E_INVALID   # wrong batch size
    assert lib.fql_ifql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_E_INVALID    # no dataset uploaded
    assert lib.fql_ifql_group_sample_actions(g, o.ctypes.data, 1, None, None, out.ctypes.data, None) == _cabi.FQL_E_INVALID   # neither noises nor seeds
    assert lib.fql_ifql_group_flow_actions(g, o.ctypes.data, None, 1, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert lib.fql_ifql_group_sample_actions(g, o.ctypes.data, 0, None, seeds, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    # released: plain handles again, bitwise with their twins through a grouped and two standalone steps, and groupable again
    for x in (a, b, twin_a, twin_b):
        x.upload_dataset(ds)
    for _ in range(2):
        assert lib.fql_ifql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B)
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    for _ in range(2):
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B)
    _assert_same_state(a, twin_a, 'released member 0')
    _assert_same_state(b, twin_b, 'released member 1')
    rc, g = create([b, a])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert lib.fql_ifql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
    for x in (twin_a, twin_b):
        x.update_from_dataset(B)
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    _assert_same_state(a, twin_a, 'regrouped member 0')
    _assert_same_state(b, twin_b, 'regrouped member 1')
    for x in (a, b, twin_a, twin_b, more, slow, wide, steps, other_b, f0, f1):
        x.close()
