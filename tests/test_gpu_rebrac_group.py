"""GPU: ReBRAC agent groups (fql_rebrac_group_*, ReBRACAgentGroup).  A member advanced by the group's two fused programs and sampled by the
fused call must be bitwise where its standalone twin is (same seed, alphas, parameters, dataset and rows): fusing changes which launch a
task rides in, never its arithmetic.  The standalone agent is pinned to the fp64 restatement at these shapes by
tests/test_gpu_rebrac_paths.py, so the twin is a checked reference and no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import rebrac_cases as RC
from tests import rebrac_oracle as RO
from tests.util import leaf_dict

pytestmark = pytest.mark.gpu


def _assert_same_state(a, b, what=''):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    assert pa.keys() == pb.keys()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=f'{what} {k}')
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step']), what
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{what} {part} {k}')
    assert a.read_info() == b.read_info(), what


def _alphas(K):
    """Members differ in both coefficients; member 1 (member 0 of a single-member group) has both at 0."""
    aa = [0.5 * (i + 1) for i in range(K)]
    ac = [0.3 * (K - i) for i in range(K)]
    aa[min(1, K - 1)] = ac[min(1, K - 1)] = 0.0
    return aa, ac


def _setup(K, B, hidden, od=29, ad=8, scale=0.1, ds_seed=7, **kw):
    """A group of K members and their standalone twins on one dataset: members and twins differ in seed, alpha_actor and alpha_critic
    only and start from the same randomised parameters."""
    import fql_amd
    hidden = (hidden,) * 4 if isinstance(hidden, int) else tuple(hidden)
    cfg = RC.config(hidden, hidden, B, **kw)
    ds = RC.dataset(od, ad, B, ds_seed)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
    seeds = [3 + i for i in range(K)]
    aa, ac = _alphas(K)
    group = fql_amd.ReBRACAgentGroup.create(seeds, ex_o, ex_a, cfg, alpha_actors=aa, alpha_critics=ac)
    group.upload_dataset(ds)
    twins = []
    for i in range(K):
        t = fql_amd.ReBRACAgent.create(seeds[i], ex_o, ex_a, dict(cfg, alpha_actor=aa[i], alpha_critic=ac[i]))
        p = RC.randomized(t.get_params(), 100 + i, scale=scale)
        t.set_params(p)
        group.members[i].set_params(p)
        t.upload_dataset(ds)
        twins.append(t)
    return cfg, ds, group, twins


def _step(group, twins, B, full, **kw):
    group.update_from_dataset(full_update=full, **kw)
    for t in twins:
        t.update_from_dataset(B, full_update=full)


def _check(group, twins):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')


# ---- 1. device-RNG trajectories -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, B, H, steps', [(3, 64, 128, 8), (2, 256, 512, 4), (8, 16, 64, 6), (1, 64, 128, 4)],
                         ids=['K3-B64-H128', 'K2-B256-H512', 'K8-B16-H64', 'K1'])
def test_rebrac_group_equals_standalone_twins_device_rng(K, B, H, steps):
    """Steps alternate critic-only / full, starting critic-only: the zero-gradient prep of the critic program runs before any full step."""
    cfg, ds, group, twins = _setup(K, B, H, scale=0.05 if H >= 512 else 0.1)
    aa = [m.config['alpha_actor'] for m in group.members]
    assert len(set(zip(aa, [m.config['alpha_critic'] for m in group.members]))) == K
    assert any(m.config['alpha_actor'] == 0.0 and m.config['alpha_critic'] == 0.0 for m in group.members)
    for i in range(steps):
        _step(group, twins, B, full=i % 2 == 1)
    _check(group, twins)
    assert group.members[0].get_opt_state()['count'] == steps
    group.close()


# ---- 2. kernel-path shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['b272', 'obs50', 'b1040_h64', 'wide1024', 'obs600', 'no_ln_h512_no_tanh', 'b16'])
def test_rebrac_group_equals_standalone_twins_on_every_path(case):
    od, ad, B, actor, value, kw, seed = RC.PATHS[case]
    assert actor == value
    cfg, ds, group, twins = _setup(2, B, actor, od=od, ad=ad, scale=0.05 if max(actor) >= 512 else 0.1, ds_seed=seed, **kw)
    for full in RC.STEP_KINDS:
        _step(group, twins, B, full)
    _check(group, twins)
    group.close()


# ---- 3. explicit rows ---------------------------------------------------------------------------------------------------------------
def test_rebrac_group_explicit_rows_host_and_device_and_lazy_infos():
    """idxs [K, B] as a host array (the group's own stream) and as a CUDA tensor (torch's current stream), alternating with no
    synchronize; every member's rows include N - 1, whose next_actions clamp to the row itself; lazy infos of both step kinds."""
    import torch
    from fql_amd.rebrac import REBRAC_CRITIC_INFO_KEYS, REBRAC_INFO_KEYS
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, 128)
    rng = np.random.default_rng(13)
    N = len(ds['observations'])
    for step in range(6):
        idxs = rng.integers(0, N, size=(K, B))
        idxs[:, step % B] = N - 1
        full = step % 2 == 1
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 3 == 0 else idxs, want_info=True, full_update=full)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=True, full_update=full)[1] for i, t in enumerate(twins)]
        assert len(infos) == K
        for i in range(K):
            got = infos[i].to_dict()
            assert tuple(got) == (REBRAC_INFO_KEYS if full else REBRAC_CRITIC_INFO_KEYS), (step, i)
            assert len(got) == (12 if full else 7)
            assert got == want[i].to_dict(), (step, i)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), N, np.int64))
    _check(group, twins)
    group.close()


# ---- 4. info13xk through the C ABI ----------------------------------------------------------------------------------------------------
def test_rebrac_group_infos_through_the_c_abi():
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's infos of the step's kind
    in read_info()'s key order, zeros behind them."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, 128)
    lib = group._lib
    for step in range(4):
        full = step in (1, 2)           # host: critic-only, full; device: full, critic-only
        if step % 2 == 0:
            host = np.full((K, 13), np.nan, np.float32)
            group._check(lib.fql_rebrac_group_update_from_dataset(group._g, None, B, int(full), host.ctypes.data, None))
            got = host
        else:
            dev = torch.full((K, 13), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_rebrac_group_update_from_dataset(group._g, None, B, int(full), dev.data_ptr(), None))
            group.synchronize()
            got = dev.cpu().numpy()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            m._last_full = full
            t.update_from_dataset(B, full_update=full)
            n = 12 if full else 7
            assert got[i, :n].tolist() == list(m.read_info().values()), (step, i)
            assert got[i, :n].tolist() == list(t.read_info().values()), (step, i)
            assert not got[i, n:].any(), (step, i)
    _check(group, twins)
    group.close()


# ---- 5. ordering without synchronize --------------------------------------------------------------------------------------------------
def test_rebrac_group_member_updates_between_group_updates():
    """A member's own critic-only update on the engine's queues and another member's host-batch update between group updates, with no
    synchronize anywhere: the group update is ordered behind them, and they behind it."""
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, B, 128)
    batch = RO.make_batch(ds, np.random.default_rng(2).integers(0, len(ds['observations']), size=B))
    noise = RO.make_noise(B, 8, 5)

    def sequence(update_all, agents):
        for r in range(3):
            update_all(False)
            agents[0].update_from_dataset(B, full_update=False)     # stream left to the engine: its own queues
            agents[1].update(batch, full_update=True, noise=noise)   # host batch, explicit noise
            update_all(True)

    sequence(lambda full: group.update_from_dataset(full_update=full), group.members)
    sequence(lambda full: [t.update_from_dataset(B, full_update=full) for t in twins], twins)
    _check(group, twins)
    assert group.members[0].get_opt_state()['count'] == 9 and group.members[2].get_opt_state()['count'] == 6
    group.close()


def test_rebrac_group_member_entry_points_straight_after_group_updates():
    """get_params / sample_actions / total_loss of a member straight after a group update see it; a set_params between group updates is
    seen by the next one."""
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, B, 128)
    batch = RO.make_batch(ds, np.arange(B))
    noise = RO.make_noise(B, 8, 9)
    obs = ds['observations'][:7]
    for rnd in range(2):
        for i in range(4):
            _step(group, twins, B, full=i % 2 == 1)
        for i, (m, t) in enumerate(zip(group.members, twins)):
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
            group.update_from_dataset(full_update=False)
            t.update_from_dataset(B, full_update=False)
            twins[1 - i].update_from_dataset(B, full_update=False)
            np.testing.assert_array_equal(m.sample_actions(obs, seed=11, temperature=0.7), t.sample_actions(obs, seed=11, temperature=0.7))
            group.update_from_dataset(full_update=True)
            for x in twins:
                x.update_from_dataset(B, full_update=True)
            assert m.total_loss(batch, noise=noise) == t.total_loss(batch, noise=noise)
        p = RC.randomized(twins[0].get_params(), 55 + rnd, scale=0.05)
        group.members[0].set_params(p)
        twins[0].set_params(p)
    for i in range(3):
        _step(group, twins, B, full=i % 2 == 0)
    _check(group, twins)
    group.close()


# ---- 6. sampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, H, tanh', [(2, 64, True), (3, 64, False), (2, 512, True)], ids=['K2-H64', 'K3-H64-no-tanh', 'K2-H512'])
def test_rebrac_group_sample_actions_equal_the_members_own(K, H, tanh):
    import torch
    od, ad = 29, 8
    cfg, ds, group, twins = _setup(K, 64, H, scale=0.05 if H >= 512 else 0.1, tanh_squash=tanh)
    ms = group.members
    rng = np.random.default_rng(17)
    side = torch.cuda.Stream()
    for n in (1, 5, 16, 37):
        obs = rng.standard_normal((K, n, od)).astype(np.float32)
        z = (3.0 * rng.standard_normal((K, n, ad))).astype(np.float32)   # past the noise clip for some entries
        for temp in (0.0, 0.5, 1.0):
            got = group.sample_actions(obs, noises=z, temperature=temp)
            assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0
            for i in range(K):
                np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i], temperature=temp), err_msg=f'n {n} T {temp} member {i}')
        seeds = [50 + n + i for i in range(K)]
        got = group.sample_actions(obs, seed=seeds, temperature=0.5)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=seeds[i], temperature=0.5), err_msg=f'n {n} seeds member {i}')
        got = group.sample_actions(obs, seed=9)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=9), err_msg=f'n {n} one seed member {i}')
        # one shared block of rows against the same rows tiled
        shared = group.sample_actions(obs[0], seed=seeds)
        np.testing.assert_array_equal(shared, group.sample_actions(np.tile(obs[:1], (K, 1, 1)), seed=seeds))
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].sample_actions(obs[0], seed=seeds[i]))
        # CUDA tensors on a side stream
        with torch.cuda.stream(side):
            to, tz = torch.from_numpy(obs).cuda(), torch.from_numpy(z).cuda()
            tg = group.sample_actions(to, noises=tz, temperature=0.5)
            assert tg.is_cuda and tuple(tg.shape) == (K, n, ad)
            want = [ms[i].sample_actions(to[i], noises=tz[i], temperature=0.5) for i in range(K)]
        side.synchronize()
        for i in range(K):
            np.testing.assert_array_equal(tg[i].cpu().numpy(), want[i].cpu().numpy(), err_msg=f'n {n} cuda member {i}')
            np.testing.assert_array_equal(tg[i].cpu().numpy(), ms[i].sample_actions(obs[i], noises=z[i], temperature=0.5))
    group.close()


def test_rebrac_group_sample_actions_across_the_row_chunk_counters_and_updates():
    """n = 4100 rows per member with seeds: the second chunk of every member draws as the member's own second chunk does.  Unseeded calls
    advance each member's counter as its own call does.  After group updates with no synchronize the fused call sees them."""
    K, B, od, ad, n = 2, 64, 29, 8, 4100
    cfg, ds, group, twins = _setup(K, B, 64)
    ms = group.members
    obs = np.random.default_rng(4).standard_normal((K, n, od)).astype(np.float32)
    seeds = [5, 6]
    got = group.sample_actions(obs, seed=seeds)
    for i in range(K):
        np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=seeds[i]), err_msg=f'member {i}')
    same = np.repeat(obs[:, :1], n, axis=1)
    drawn = group.sample_actions(same, seed=seeds)
    assert np.abs(drawn[:, 4096] - drawn[:, 0]).max() > 1e-3   # the second chunk's first row draws its own noise
    # unseeded: member i's counter advances once per fused call, as by its own call; the twin (same seed, same parameters so far)
    # draws the same
    o7 = obs[:, :7]
    for r in range(3):
        before = [m._sample_calls for m in ms]
        got = group.sample_actions(o7)
        assert [m._sample_calls for m in ms] == [c + 1 for c in before]
        for i in range(K):
            np.testing.assert_array_equal(got[i], twins[i].sample_actions(o7[i]), err_msg=f'unseeded round {r} member {i}')
            assert ms[i]._sample_calls == twins[i]._sample_calls
    assert np.abs(got - group.sample_actions(o7)).max() > 0
    for t in twins:
        t.sample_actions(o7[0])
    # after group updates, no synchronize
    for i in range(3):
        _step(group, twins, B, full=i % 2 == 1)
    got = group.sample_actions(o7, seed=21, temperature=0.5)
    for i in range(K):
        np.testing.assert_array_equal(got[i], twins[i].sample_actions(o7[i], seed=21, temperature=0.5), err_msg=f'after updates member {i}')
    _check(group, twins)
    group.close()


# ---- 7. launch counts -----------------------------------------------------------------------------------------------------------------
def test_rebrac_group_launch_counts_do_not_depend_on_k():
    """A fused program has a member's launch count, whatever K.  One sampling chunk: the assemble launch, the actor's forward and the
    action launch.  The actor's forward (the members' prog_os) is a chain of Dense layers each of which reads the one before, so
    no two share a launch: one launch per layer, hidden layers + mean_net."""
    B, H = 16, 64
    sample = set()
    for K in (1, 2, 4):
        cfg, ds, group, twins = _setup(K, B, H)
        full, critic, s = group.launches()
        assert full == twins[0].rebrac_stats(True)[0] and critic == twins[0].rebrac_stats(False)[0], K
        assert full == group.members[0].rebrac_stats(True)[0] and critic < full
        sample.add(s)
        group.close()
    assert sample == {2 + len(cfg['actor_hidden_dims']) + 1}


# ---- 8. refusals and release ----------------------------------------------------------------------------------------------------------
def test_rebrac_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    B, od, ad = 64, 29, 8
    cfg = RC.config((128,) * 4, (128,) * 4, B)
    ds = RC.dataset(od, ad, B, 1)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]

    def create(members, fn=lib.fql_rebrac_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def rebrac(seed, **kw):
        return fql_amd.ReBRACAgent.create(seed, ex_o, ex_a, dict(cfg, **kw))

    a, twin_a = rebrac(0), rebrac(0)
    fq_cfg = fql_amd.get_config()
    fq_cfg.update(actor_hidden_dims=(128,) * 4, value_hidden_dims=(128,) * 4, batch_size=B)
    f0, f1 = fql_amd.FQLAgent.create(0, ex_o, ex_a, fq_cfg), fql_amd.FQLAgent.create(1, ex_o, ex_a, fq_cfg)
    rc, g = create([a, f0])
    assert rc == _cabi.FQL_E_STATE and not g.value and b'FQL' in lib.fql_last_error(None)
    noisy, wide, other_b = rebrac(1, actor_noise=0.3), rebrac(2, actor_hidden_dims=(256,) * 4, value_hidden_dims=(256,) * 4), rebrac(3, batch_size=32)
    for bad in (noisy, wide, other_b):
        rc, g = create([a, bad])
        assert rc == _cabi.FQL_E_INVALID and not g.value, lib.fql_last_error(None)
        assert b'member 1' in lib.fql_last_error(None)
    assert create([a, a])[0] == _cabi.FQL_E_INVALID
    rc, g = create([a, rebrac(9)], fn=lib.fql_group_create)          # fql_group_create keeps refusing ReBRAC handles
    assert rc == _cabi.FQL_E_STATE and not g.value
    b, twin_b = rebrac(5, alpha_actor=3.0, alpha_critic=0.0), rebrac(5, alpha_actor=3.0, alpha_critic=0.0)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID                     # already grouped
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # the FQL group calls on a ReBRAC group, and the ReBRAC group calls on an FQL group
    o, out = np.zeros((2, 1, od), np.float32), np.zeros((2, 1, ad), np.float32)
    z, seeds, v = np.zeros((2, 1, ad), np.float32), (C.c_uint64 * 2)(1, 2), C.c_int64(-1)
    for rc in (lib.fql_group_update_from_dataset(g, None, B, None, None),
               lib.fql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, out.ctypes.data, None),
               lib.fql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None),
               lib.fql_group_sample_stats(g, 0, C.byref(v))):
        assert rc == _cabi.FQL_E_STATE and b'fql_rebrac_group_' in lib.fql_last_error(None), lib.fql_last_error(None)
    rc, fg = create([f0, f1], fn=lib.fql_group_create)
    assert rc == _cabi.FQL_OK and fg.value
    for rc in (lib.fql_rebrac_group_update_from_dataset(fg, None, B, 1, None, None),
               lib.fql_rebrac_group_sample_actions(fg, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None),
               lib.fql_rebrac_group_stats(fg, C.byref(v), None, None)):
        assert rc == _cabi.FQL_E_STATE, lib.fql_last_error(None)
    assert v.value == -1
    assert lib.fql_group_destroy(fg) == _cabi.FQL_OK
    assert lib.fql_rebrac_group_update_from_dataset(g, None, 32, 1, None, None) == _cabi.FQL_E_INVALID   # wrong batch size
    assert lib.fql_rebrac_group_update_from_dataset(g, None, B, 0, None, None) == _cabi.FQL_E_INVALID    # no dataset uploaded
    # released: plain handles again, bitwise with their twins through a grouped and two standalone steps
    for x in (a, b, twin_a, twin_b):
        x.upload_dataset(ds)
    for full in (False, True):
        assert lib.fql_rebrac_group_update_from_dataset(g, None, B, int(full), None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B, full_update=full)
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    a._last_full = b._last_full = True
    for full in (False, True):
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B, full_update=full)
    _assert_same_state(a, twin_a, 'released member 0')
    _assert_same_state(b, twin_b, 'released member 1')
    for x in (a, b, twin_a, twin_b, noisy, wide, other_b, f0, f1):
        x.close()
