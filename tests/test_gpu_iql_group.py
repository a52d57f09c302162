"""GPU: IQL agent groups (fql_iql_group_*, IQLAgentGroup).  A member advanced by the group's fused program and sampled by the fused call
must be bitwise where its standalone twin is (same seed, expectile, alpha, parameters, dataset and rows): fusing changes which launch a
task rides in, never its arithmetic.  The standalone agent is pinned to the fp64 restatement at these shapes by tests/test_gpu_iql.py and
tests/test_kink_margins_cpu.py, so the twin is a checked reference and no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.test_gpu_iql import SHAPE_CASES, SHAPE_COMBOS
from tests.util import leaf_dict, randomize_params

pytestmark = pytest.mark.gpu
H64 = ((64,) * 4, (64,) * 4)
H512 = ((512,) * 4, (512,) * 4)


def _state(a):
    """Every array and counter of an agent: parameters (the target critic and log_stds among them), both Adam moments, the counters."""
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
    assert ('params/modules_actor/log_stds' in sa) == (not a.config['const_std'])
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f'{what} {k}')
    assert a.read_info() == b.read_info(), what


def _params(agent, seed):
    """Biases and LayerNorm leaves away from their init, the target critic away from the critic, log_stds away from 0."""
    p = randomize_params(agent.get_params(), seed)
    if 'log_stds' in p['modules_actor']:
        ls = p['modules_actor']['log_stds']
        p['modules_actor']['log_stds'] = (0.3 * np.random.default_rng(seed + 1).standard_normal(ls.shape)).astype(np.float32)
    return p


def _setup(K, B, hidden=H64, od=29, ad=8, expectiles=None, alphas=None, ds_seed=7, seeds=None, **kw):
    """A group of K members and their standalone twins on one dataset: member and twin share the create seed, the coefficients and the
    randomised parameters; members differ from each other in all of them unless the caller says otherwise."""
    import fql_amd
    cfg = fql_amd.iql.get_config()
    cfg.update(actor_hidden_dims=tuple(hidden[0]), value_hidden_dims=tuple(hidden[1]), batch_size=B)
    cfg.update(kw)
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=ds_seed)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
    seeds = [3 + i for i in range(K)] if seeds is None else list(seeds)
    expectiles = [float(cfg['expectile'])] * K if expectiles is None else list(expectiles)
    alphas = [float(cfg['alpha'])] * K if alphas is None else list(alphas)
    group = fql_amd.IQLAgentGroup.create(seeds, ex_o, ex_a, cfg, expectiles=expectiles, alphas=alphas)
    group.upload_dataset(ds)
    twins = []
    for i in range(K):
        t = fql_amd.IQLAgent.create(seeds[i], ex_o, ex_a, dict(cfg, expectile=expectiles[i], alpha=alphas[i]))
        p = _params(t, 100 + i)
        t.set_params(p)
        group.members[i].set_params(p)
        t.upload_dataset(ds)
        twins.append(t)
    assert all(type(m) is fql_amd.IQLAgent for m in group.members)
    assert [m.config['alpha'] for m in group.members] == alphas and [m.config['expectile'] for m in group.members] == expectiles
    return cfg, ds, group, twins


def _step(group, twins, B, want_info=False, idxs=None):
    infos = group.update_from_dataset(want_info=want_info, idxs=idxs)
    want = [t.update_from_dataset(B, want_info=want_info, idxs=None if idxs is None else idxs[i])[1] for i, t in enumerate(twins)]
    return infos, want


def _assert_infos(infos, want, cfg, what):
    from fql_amd.iql import IQL_INFO_KEYS
    keys = IQL_INFO_KEYS[cfg['actor_loss']]
    assert len(keys) == (19 if cfg['actor_loss'] == 'ddpgbc' else 16)
    assert len(infos) == len(want)
    for i, (g, w) in enumerate(zip(infos, want)):
        g, w = g.to_dict(), w.to_dict()
        assert tuple(g) == keys == tuple(w), (what, i)
        for k in g:
            np.testing.assert_array_equal(np.asarray(g[k]), np.asarray(w[k]), err_msg=f'{what} member {i} {k}')


def _check(group, twins, what=''):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'{what} member {i}')


# ---- 1. twins on device-drawn rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, B, H, steps, loss, const_std, alphas, expectiles', [
    (3, 64, H64, 8, 'awr', False, [0.3, 1.0, 3.0], [0.7, 0.8, 0.9]),
    (2, 256, H512, 6, 'ddpgbc', False, None, None),
    (8, 16, H64, 6, 'ddpgbc', True, None, None),
    (1, 64, H64, 6, 'awr', True, None, None),
], ids=['K3-B64-H64-awr-sweep', 'K2-B256-H512-ddpgbc', 'K8-B16-H64-ddpgbc-const', 'K1-awr-const'])
def test_iql_group_equals_standalone_twins_device_rng(K, B, H, steps, loss, const_std, alphas, expectiles):
    """After every step the 16 or 19 infos of every member against its twin; at the end parameters, both Adam moments, the target
    critic, log_stds and the counters."""
    cfg, ds, group, twins = _setup(K, B, H, alphas=alphas, expectiles=expectiles, actor_loss=loss, const_std=const_std)
    for step in range(steps):
        infos, want = _step(group, twins, B, want_info=True)
        _assert_infos(infos, want, cfg, f'step {step}')
    _check(group, twins)
    assert group.members[0].get_opt_state()['count'] == steps
    group.close()


# ---- 2. one coefficient differs ----------------------------------------------------------------------------------------------------------
VALUE_CRITIC_KEYS = ('value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
                     'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min')


def _one_state(loss, **coef):
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, B, H64, seeds=[5, 5], actor_loss=loss, const_std=False, **coef)
    p = _params(twins[0], 77)
    for a in list(group.members) + twins:
        a.set_params(p)
    idx = np.random.default_rng(3).integers(0, len(ds['observations']), size=B)
    infos, want = _step(group, twins, B, want_info=True, idxs=np.stack([idx, idx]))
    _assert_infos(infos, want, cfg, 'first step')
    _check(group, twins)
    group.close()
    return infos[0].to_dict(), infos[1].to_dict()


@pytest.mark.parametrize('loss', ['awr', 'ddpgbc'])
def test_iql_group_alpha_alone_moves_only_the_actor(loss):
    """Two members in one state (create seed, parameters) on one set of rows, alphas 0.5 and 3: the value and critic infos are equal on
    the first step, the actor loss is not."""
    a, b = _one_state(loss, alphas=[0.5, 3.0])
    for k in VALUE_CRITIC_KEYS:
        assert a[k] == b[k], k
    assert a['actor/actor_loss'] != b['actor/actor_loss']
    assert a['actor/bc_log_prob'] == b['actor/bc_log_prob'] and a['actor/mse'] == b['actor/mse']


@pytest.mark.parametrize('loss', ['awr', 'ddpgbc'])
def test_iql_group_expectile_alone_moves_only_the_value_loss(loss):
    """The same with expectiles 0.6 and 0.9: of the value and critic keys only value/value_loss differs (the critic's target is
    value(next_obs) with the stored parameters)."""
    a, b = _one_state(loss, expectiles=[0.6, 0.9])
    assert a['value/value_loss'] != b['value/value_loss']
    for k in VALUE_CRITIC_KEYS[1:]:
        assert a[k] == b[k], k


# ---- 3. kernel-path shapes ---------------------------------------------------------------------------------------------------------------
_SEEDS = {(c, loss, cs): seed for c, loss, cs, seed in SHAPE_COMBOS}
PATH_CASES = [(c, loss, 2) for c in ('default', 'act16', 'humanoidmaze', 'obs50', 'ragged_depths', 'b272', 'w50_padded') for loss in ('awr', 'ddpgbc')]
PATH_CASES += [('b1024', 'awr', 1), ('b16', 'awr', 2), ('b16', 'ddpgbc', 2)]


@pytest.mark.parametrize('case, loss, steps', PATH_CASES, ids=[f'{c}-{loss}' for c, loss, _ in PATH_CASES])
def test_iql_group_equals_standalone_twins_on_every_path(case, loss, steps):
    """K = 2, log_stds learned, at the shapes of tests/test_gpu_iql.py's SHAPE_CASES (its table, its cfg overrides, its seeds) and at
    B = 16 (one 16-row tile: obs 7, act 3, hidden 64)."""
    if case == 'b16':
        (od, ad, B, hidden), kw, seed = (7, 3, 16, H64), {}, 0
    else:
        (od, ad, B, hidden), kw, _ = SHAPE_CASES[case]
        seed = _SEEDS[(case, loss, False)]
    cfg, ds, group, twins = _setup(2, B, hidden, od=od, ad=ad, ds_seed=seed, expectiles=[0.7, 0.9], alphas=[0.5, 3.0],
                                   actor_loss=loss, const_std=False, **kw)
    for step in range(steps):
        infos, want = _step(group, twins, B, want_info=True)
        _assert_infos(infos, want, cfg, f'{case} step {step}')
    _check(group, twins, case)
    group.close()


# ---- 4. explicit rows --------------------------------------------------------------------------------------------------------------------
def test_iql_group_explicit_rows_host_and_device():
    """idxs [K, B] as a host array (the group's own stream) and as a CUDA tensor (torch's current stream), alternating with no
    synchronize; every member's rows include N - 1."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, alphas=[0.3, 1.0, 3.0], actor_loss='ddpgbc', const_std=False)
    rng = np.random.default_rng(13)
    N = len(ds['observations'])
    for step in range(6):
        idxs = rng.integers(0, N, size=(K, B))
        idxs[:, step % B] = N - 1
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 2 == 0 else idxs, want_info=True)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, cfg, f'step {step}')
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), N, np.int64))
    _check(group, twins)
    group.close()


# ---- 5. infos through the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss, n', [('awr', 16), ('ddpgbc', 19)])
def test_iql_group_infos_through_the_c_abi(loss, n):
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's 16 or 19 infos in
    read_info()'s key order; nothing is written behind them."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, alphas=[0.3, 1.0, 3.0], actor_loss=loss, const_std=False)
    lib = group._lib
    assert lib.fql_num_info(group.members[0]._h) == n
    for step in range(4):
        if step % 2 == 0:
            host = np.full((K * n + 3,), np.nan, np.float32)
            group._check(lib.fql_iql_group_update_from_dataset(group._g, None, B, host.ctypes.data, None))
            got, tail = host[:K * n].reshape(K, n), host[K * n:]
        else:
            dev = torch.full((K * n + 3,), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_iql_group_update_from_dataset(group._g, None, B, dev.data_ptr(), None))
            group.synchronize()
            got, tail = dev.cpu().numpy()[:K * n].reshape(K, n), dev.cpu().numpy()[K * n:]
        assert np.isnan(tail).all()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_from_dataset(B)
            assert got[i].tolist() == list(m.read_info().values()), (step, i)
            assert got[i].tolist() == list(t.read_info().values()), (step, i)
    _check(group, twins)
    group.close()


# ---- 6. the members' own work between group updates, no synchronize ----------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['awr', 'ddpgbc'])
def test_iql_group_member_work_between_group_updates(tmp_path, loss):
    """Between group updates and with no synchronize anywhere: a member's own total_loss, sample_actions, get_params / set_params, its
    own updates and a checkpoint round trip.  The group update is ordered behind them, and they behind it; the fused sampler sees the
    group's last update."""
    from fql_amd import checkpoint
    K, B, ad = 3, 64, 8
    cfg, ds, group, twins = _setup(K, B, alphas=[0.3, 1.0, 3.0], expectiles=[0.7, 0.8, 0.9], actor_loss=loss, const_std=False)
    ms = group.members
    batch = O.sample_batch(ds, np.random.default_rng(2).integers(0, len(ds['observations']), size=B))
    noise = {'eps': np.random.default_rng(5).standard_normal((B, ad)).astype(np.float32)}
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
            _step(group, twins, B)
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
        # the fused sampler straight after a group update
        got = group.sample_actions(obs, seed=21 + rnd)
        for i, t in enumerate(twins):
            np.testing.assert_array_equal(got[i], t.sample_actions(obs, seed=21 + rnd), err_msg=f'fused sampler round {rnd} member {i}')
        # a set_params between group updates is seen by the next one
        p = _params(twins[2], 55 + rnd)
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


# ---- 7. the fused Gaussian sampler -------------------------------------------------------------------------------------------------------
def _rows(K, n, od, ad, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n, od)).astype(np.float32), (2.0 * rng.standard_normal((K, n, ad))).astype(np.float32)


@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('const_std', [True, False], ids=['const_std', 'log_stds'])
def test_iql_group_sample_actions_equal_the_members_own(K, const_std):
    """n = 4096 + 37 crosses the 4096-row chunk edge: the second chunk's rows keep their numbers in the call, so a seeded draw does not
    depend on the chunking.  Temperature 0 is clip(mean) and takes no draw."""
    import torch
    od, ad = 29, 8
    cfg, ds, group, twins = _setup(K, 64, actor_loss='ddpgbc', const_std=const_std)
    ms = group.members
    before = [_state(m) for m in ms]
    side = torch.cuda.Stream()
    for n in (1, 10, 4096 + 37):
        obs, z = _rows(K, n, od, ad, 17 + n)
        seeds = [50 + n + i for i in range(K)]
        for temp in (0.0, 1.0):
            got = group.sample_actions(obs, noises=z, temperature=temp)
            assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0
            for i in range(K):
                np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i], temperature=temp), err_msg=f'n {n} T {temp} noises member {i}')
                np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i], temperature=temp), err_msg=f'n {n} T {temp} noises twin {i}')
            drawn = group.sample_actions(obs, seed=seeds, temperature=temp)
            for i in range(K):
                np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=seeds[i], temperature=temp), err_msg=f'n {n} T {temp} seeds twin {i}')
            if temp == 0.0:
                np.testing.assert_array_equal(drawn, got)
        got = group.sample_actions(obs, seed=9)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=9), err_msg=f'n {n} one seed member {i}')
        if n > 10:   # the second chunk's first row draws its own noise: the same observation in every row, seeded
            same = np.repeat(obs[:, :1], n, axis=1)
            drawn = group.sample_actions(same, seed=[5, 6, 7][:K])
            for i in range(K):
                np.testing.assert_array_equal(drawn[i], ms[i].sample_actions(same[i], seed=5 + i), err_msg=f'same rows member {i}')
                assert len(np.unique(drawn[i][4090:4100], axis=0)) == 10
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
            ts = group.sample_actions(to, seed=seeds, temperature=0.5)
        side.synchronize()
        for i in range(K):
            np.testing.assert_array_equal(tg[i].cpu().numpy(), want[i].cpu().numpy(), err_msg=f'n {n} cuda member {i}')
            np.testing.assert_array_equal(tg[i].cpu().numpy(), ms[i].sample_actions(obs[i], noises=z[i]))
            np.testing.assert_array_equal(ts[i].cpu().numpy(), ms[i].sample_actions(obs[i], seed=seeds[i], temperature=0.5))
    # unseeded: member i's counter advances once per fused call, as by its own call; the twin (same seed, same parameters) draws the same
    o7 = _rows(K, 7, od, ad, 4)[0]
    for r in range(3):
        calls = [m._sample_calls for m in ms]
        got = group.sample_actions(o7)
        assert [m._sample_calls for m in ms] == [c + 1 for c in calls]
        for i in range(K):
            tw = twins[i].sample_actions(o7[i])
            assert ms[i]._sample_calls == twins[i]._sample_calls
            np.testing.assert_array_equal(got[i], tw, err_msg=f'unseeded round {r} member {i}')
    # no parameter or optimizer state changed
    for i, m in enumerate(ms):
        (arrays, counters), (arrays0, counters0) = _state(m), before[i]
        assert counters == counters0
        for k in arrays:
            np.testing.assert_array_equal(arrays[k], arrays0[k], err_msg=f'member {i} {k}')
    group.close()


def test_iql_group_sample_actions_hidden_512_padded_action_width():
    """obs 69, act 21 (padded action width 32), hidden 512, n = 37, log_stds learned."""
    K, n, od, ad = 2, 37, 69, 21
    cfg, ds, group, twins = _setup(K, 64, H512, od=od, ad=ad, actor_loss='awr', const_std=False)
    obs, z = _rows(K, n, od, ad, 23)
    got = group.sample_actions(obs, noises=z)
    drawn = group.sample_actions(obs, seed=[8, 9], temperature=0.7)
    mode = group.sample_actions(obs, seed=1, temperature=0.0)
    for i in range(K):
        np.testing.assert_array_equal(got[i], group.members[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises member {i}')
        np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises twin {i}')
        np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=8 + i, temperature=0.7), err_msg=f'seeds twin {i}')
        np.testing.assert_array_equal(mode[i], twins[i].sample_actions(obs[i], seed=1, temperature=0.0), err_msg=f'mode twin {i}')
    group.close()


# ---- 8. launch counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['awr', 'ddpgbc'])
def test_iql_group_launch_counts_do_not_depend_on_k(loss):
    """The fused update has a member's launch count, whatever K.  A sampling chunk is assemble, the actor (a chain of Dense layers each
    of which reads the one before: one launch per layer) and the sampling head."""
    B = 16
    counts = set()
    for K in (1, 2, 4):
        cfg, ds, group, twins = _setup(K, B, actor_loss=loss, const_std=False)
        u, s = group.launches()
        assert u == twins[0].iql_stats()[0] == group.members[0].iql_stats()[0], K
        counts.add((u, s))
        group.close()
    assert len(counts) == 1
    u, s = counts.pop()
    assert s == 2 + len(cfg['actor_hidden_dims']) + 1


# ---- 9. refusals and release -------------------------------------------------------------------------------------------------------------
def test_iql_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    B, od, ad = 64, 29, 8
    cfg = fql_amd.iql.get_config()
    cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B, actor_loss='ddpgbc', const_std=False)
    ds = O.make_synthetic_dataset(4 * B, od, ad, seed=1)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]

    def create(members, fn=lib.fql_iql_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def iql(seed, **kw):
        return fql_amd.IQLAgent.create(seed, ex_o, ex_a, dict(cfg, **kw))

    a, twin_a = iql(0), iql(0)
    # the other kinds' creates keep refusing IQL handles
    for fn in (lib.fql_group_create, lib.fql_ifql_group_create, lib.fql_rebrac_group_create, lib.fql_iqld_group_create):
        rc, g = create([a, twin_a], fn=fn)
        assert rc == _cabi.FQL_E_STATE and not g.value and b'IQL' in lib.fql_last_error(None), lib.fql_last_error(None)
    # and the IQL create another kind's
    icfg = fql_amd.ifql.get_config()
    icfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B, num_samples=4)
    f0 = fql_amd.IFQLAgent.create(0, ex_o, ex_a, icfg)
    rc, g = create([a, f0])
    assert rc == _cabi.FQL_E_STATE and not g.value and b'IFQL' in lib.fql_last_error(None)
    other_loss, other_std, slow, wide, other_b = (iql(1, actor_loss='awr'), iql(2, const_std=True), iql(3, lr=1e-4),
                                                  iql(4, actor_hidden_dims=(128,) * 4, value_hidden_dims=(128,) * 4), iql(6, batch_size=32))
    for bad in (other_loss, other_std, slow, wide, other_b):
        rc, g = create([a, bad])
        assert rc == _cabi.FQL_E_INVALID and not g.value, lib.fql_last_error(None)
        assert b'member 1' in lib.fql_last_error(None)
        if bad is not other_b:
            assert b'seed and expectile / alpha' in lib.fql_last_error(None)
    assert create([a, a])[0] == _cabi.FQL_E_INVALID
    b, twin_b = iql(5, expectile=0.7, alpha=3.0), iql(5, expectile=0.7, alpha=3.0)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID and b'already belongs' in lib.fql_last_error(None)
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # every other kind's group calls on an IQL group name the IQL call
    o, out = np.zeros((2, 1, od), np.float32), np.zeros((2, 1, ad), np.float32)
    z, zn, seeds, v = np.zeros((2, 1, ad), np.float32), np.zeros((2, 1, 4, ad), np.float32), (C.c_uint64 * 2)(1, 2), C.c_int64(-1)
    w, la = np.ones((2, 1), np.float32), (C.c_int64 * 4)(-1, -1, -1, -1)
    for call, name in ((lambda: lib.fql_ifql_group_update_from_dataset(g, None, B, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_ifql_group_sample_actions(g, o.ctypes.data, 1, zn.ctypes.data, seeds, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_ifql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_ifql_group_stats(g, C.byref(v), None, None), b'fql_iql_group_stats'),
                       (lambda: lib.fql_group_update_from_dataset(g, None, B, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_group_sample_stats(g, 0, C.byref(v)), b'fql_iql_group_stats'),
                       (lambda: lib.fql_rebrac_group_update_from_dataset(g, None, B, 1, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_rebrac_group_sample_actions(g, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_rebrac_group_stats(g, C.byref(v), None, None), b'fql_iql_group_stats'),
                       (lambda: lib.fql_iqld_group_update_from_dataset(g, None, B, 1, 1, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_iqld_group_sample_actions(g, o.ctypes.data, 1, None, seeds, w.ctypes.data, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_iqld_group_stats(g, la, C.byref(v)), b'fql_iql_group_stats')):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None) and b'IQL agents' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1 and list(la) == [-1] * 4 and not out.any()
    # and the IQL calls on an IFQL group name the IFQL call
    f1 = fql_amd.IFQLAgent.create(1, ex_o, ex_a, icfg)
    rc, fg = create([f0, f1], fn=lib.fql_ifql_group_create)
    assert rc == _cabi.FQL_OK and fg.value
    for call, name in ((lambda: lib.fql_iql_group_update_from_dataset(fg, None, B, None, None), b'fql_ifql_group_update_from_dataset'),
                       (lambda: lib.fql_iql_group_sample_actions(fg, o.ctypes.data, 1, z.ctypes.data, seeds, 1.0, out.ctypes.data, None), b'fql_ifql_group_sample_actions'),
                       (lambda: lib.fql_iql_group_stats(fg, C.byref(v), None), b'fql_ifql_group_stats')):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1
    assert lib.fql_group_destroy(fg) == _cabi.FQL_OK
    assert lib.fql_iql_group_update_from_dataset(g, None, 32, None, None) == _cabi.FQL_E_INVALID   # wrong batch size
    assert lib.fql_iql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_E_INVALID    # no dataset uploaded
    assert lib.fql_iql_group_sample_actions(g, o.ctypes.data, 1, None, None, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID   # neither noises nor seeds
    assert lib.fql_iql_group_sample_actions(g, o.ctypes.data, 0, None, seeds, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert lib.fql_iql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, -1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    # FQLAgentGroup still refuses an IQL config
    with pytest.raises(NotImplementedError, match='IQLAgentGroup'):
        fql_amd.FQLAgentGroup.create([0, 1], ex_o, ex_a, cfg)
    # released: plain handles again, bitwise with their twins through grouped and standalone steps, and groupable again
    for x in (a, b, twin_a, twin_b):
        x.upload_dataset(ds)
    for _ in range(2):
        assert lib.fql_iql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B)
    assert lib.fql_group_synchronize(g) == _cabi.FQL_OK
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    for _ in range(2):
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B)
    _assert_same_state(a, twin_a, 'released member 0')
    _assert_same_state(b, twin_b, 'released member 1')
    rc, g = create([b, a])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert lib.fql_iql_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
    for x in (twin_a, twin_b):
        x.update_from_dataset(B)
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    _assert_same_state(a, twin_a, 'regrouped member 0')
    _assert_same_state(b, twin_b, 'regrouped member 1')
    for x in (a, b, twin_a, twin_b, other_loss, other_std, slow, wide, other_b, f0, f1):
        x.close()


def test_iql_group_close_releases_the_members_and_is_idempotent():
    """After close() the members update alone, bitwise with their twins; a second close() is a no-op."""
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, B, alphas=[0.5, 3.0], actor_loss='awr', const_std=False)
    _step(group, twins, B)
    group.close()
    group.close()
    assert group._g is None
    for m, t in zip(group.members, twins):
        m.update_from_dataset(B)
        t.update_from_dataset(B)
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'closed member {i}')
