"""GPU: IQL-diffusion agent groups (fql_iqld_group_*, IQLDiffusionAgentGroup).  A member advanced by the group's four fused programs and
sampled by the fused call must be bitwise where its standalone twin is (same seed, coefficients, parameters, dataset and rows): fusing
changes which launch a task rides in, never its arithmetic.  The standalone agent is pinned to the fp64 restatement at these shapes by
tests/test_gpu_iqld.py, so the twin is a checked reference and no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iqld_cases as IC
from tests import iqld_oracle as DO
from tests.util import leaf_dict

pytestmark = pytest.mark.gpu
KINDS = [(1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (0, 1), (1, 0)]
CRITIC_SIDE = ('critic', 'value', 'target_critic')


def _state(a):
    """Every array and counter of an agent: parameters (the target net among them), both Adam moment sets, the three counters."""
    a.synchronize()
    opt = a.get_opt_state()
    out = {f'params/{k}': v for k, v in leaf_dict(a.get_params()).items()}
    for part in ('mu', 'nu'):
        out.update({f'{part}/{k}': v for k, v in leaf_dict(opt[part]).items()})
    return out, a.get_steps()


def _assert_same_state(a, b, what=''):
    (sa, ca), (sb, cb) = _state(a), _state(b)
    assert sa.keys() == sb.keys() and ca == cb, (what, ca, cb)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f'{what} {k}')
    assert a.read_info() == b.read_info(), what


def _setup(K, c, betas=None, temps=None, ds_seed=7, rows=None):
    """A group of K members and their standalone twins on one dataset: member and twin share the create seed, the coefficients and the
    randomised parameters; members differ from each other in all three."""
    import fql_amd
    cfg = IC.config(c)
    od, ad, B = c['od'], c['ad'], c['B']
    ds = O.make_synthetic_dataset(rows or max(4 * B, 64), od, ad, seed=ds_seed)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
    seeds = [3 + i for i in range(K)]
    betas = list(betas) if betas is not None else [float(cfg['softmax_beta'])] * K
    temps = list(temps) if temps is not None else [float(cfg['awr_temperature'])] * K
    group = fql_amd.IQLDiffusionAgentGroup.create(seeds, ex_o, ex_a, cfg, awr_temperatures=temps, softmax_betas=betas)
    group.upload_dataset(ds)
    twins = []
    for i in range(K):
        t = fql_amd.IQLDiffusionAgent.create(seeds[i], ex_o, ex_a, dict(cfg, awr_temperature=temps[i], softmax_beta=betas[i]))
        p = DO.randomize(t.get_params(), 100 + i, q_spread=3.0)
        t.set_params(p)
        group.members[i].set_params(p)
        t.upload_dataset(ds)
        twins.append(t)
    return cfg, ds, group, twins


def _step(group, twins, B, uc, ua, want_info=False, idxs=None):
    infos = group.update_from_dataset(update_critic=uc, update_actor=ua, want_info=want_info, idxs=idxs)
    want = [t.update_from_dataset(B, update_critic=uc, update_actor=ua, want_info=want_info, idxs=None if idxs is None else idxs[i])[1]
            for i, t in enumerate(twins)]
    return infos, want


def _assert_infos(infos, want, uc, ua, what):
    from fql_amd.iql_diffusion import info_keys
    assert len(infos) == len(want)
    for i, (g, w) in enumerate(zip(infos, want)):
        g, w = g.to_dict(), w.to_dict()
        assert tuple(g) == info_keys(uc, ua) == tuple(w), (what, i)
        for k in g:
            np.testing.assert_array_equal(np.asarray(g[k]), np.asarray(w[k]), err_msg=f'{what} member {i} {k}')


def _check(group, twins, what=''):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'{what} member {i}')


# ---- 1. twins on device-drawn rows, every step kind ------------------------------------------------------------------------------------
@pytest.mark.parametrize('K, B, H, ov, coef', [
    (3, 64, 64, 'binary_softmax_loss', dict(betas=[1.0, 2.0, 3.0])),
    (2, 256, 512, 'binary_awr_loss', dict(temps=[0.5, 2.0])),
    (8, 16, 64, 'binary', {}),
    (1, 64, 64, 'binary_awr_loss', {}),
], ids=['K3-B64-H64-softmax', 'K2-B256-H512-awr', 'K8-B16-H64-binary', 'K1'])
def test_iqld_group_equals_standalone_twins_device_rng(K, B, H, ov, coef):
    """After every step: the infos of that kind, read_rows(0..2) and get_steps of every member against its twin.  A (0, 0) step leaves
    every array in place and moves steps[0]; a (0, 1) step leaves critic, value, target and their moments, a (1, 0) step the actor's."""
    cfg, ds, group, twins = _setup(K, IC.case(H=H, B=B, ov=ov, seed=50), **coef)
    ms = group.members
    for step, (uc, ua) in enumerate(KINDS):
        before = [_state(m) for m in ms]
        infos, want = _step(group, twins, B, uc, ua, want_info=True)
        _assert_infos(infos, want, uc, ua, f'step {step}')
        for i, (m, t) in enumerate(zip(ms, twins)):
            for which in range(3):
                np.testing.assert_array_equal(m._read_rows(which, B), t._read_rows(which, B), err_msg=f'step {step} member {i} rows {which}')
            assert m.get_steps() == t.get_steps(), (step, i)
            (arrays, steps), (arrays0, steps0) = _state(m), before[i]
            assert steps == {'updates': steps0['updates'] + 1, 'critic': steps0['critic'] + uc, 'actor': steps0['actor'] + ua}, (step, i)
            moved = set()
            for k in arrays:
                net = k.split('/')[1]
                assert net in CRITIC_SIDE + ('actor',), k
                if (not uc and net in CRITIC_SIDE) or (not ua and net == 'actor'):
                    np.testing.assert_array_equal(arrays[k], arrays0[k], err_msg=f'step {step} ({uc}, {ua}) member {i}: {k} moved')
                elif not np.array_equal(arrays[k], arrays0[k]):
                    moved.add(net)
            assert moved == set(CRITIC_SIDE if uc else ()) | set(('actor',) if ua else ()), (step, i, moved)
        if step == 0 and ov == 'binary_softmax_loss':
            # the members' own softmax_beta reached the fused weight launch: on the SAME advantages (member 0's parameters and rows
            # would do; here each member's own) weights under different betas differ, and each member's equal its twin's (above)
            w = [m._read_rows(2, B) for m in ms]
            ratio = [float((x > 0).mean()) for x in w]
            print('positive ratio', ratio)
            assert all(0.0 < r < 1.0 for r in ratio), ratio
            for i in range(K):
                for j in range(i):
                    assert not np.array_equal(w[i], w[j]), (i, j)
    _check(group, twins)
    assert ms[0].get_steps() == {'updates': 7, 'critic': 4, 'actor': 4}
    group.close()


def test_iqld_group_members_of_one_state_differ_by_their_beta_alone():
    """Three members with the SAME parameters and the same explicit rows, betas 1 / 2 / 3: a fused weight launch that read member 0's
    arguments for everyone would give three equal loss_weights arrays.  They differ, and each is its twin's."""
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, IC.case(H=64, B=B, ov='binary_softmax_loss', seed=51), betas=[1.0, 2.0, 3.0])
    p = twins[0].get_params()
    for x in group.members + twins:
        x.set_params(p)
    idxs = np.tile(np.random.default_rng(3).integers(0, len(ds['observations']), size=(1, B)), (K, 1))
    _step(group, twins, B, 0, 1, idxs=idxs)
    w = [m._read_rows(2, B) for m in group.members]
    for i in range(K):
        np.testing.assert_array_equal(w[i], twins[i]._read_rows(2, B))
        assert 0 < (w[i] > 0).sum() < B
        for j in range(i):
            assert (w[i] > 0).tolist() == (w[j] > 0).tolist() and not np.array_equal(w[i], w[j]), (i, j)
    _check(group, twins)
    group.close()


# ---- 2. kernel-path shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['b272', 'b2064-binary', 'wide1024', 'ragged', 'humanoidmaze', 'act16'])
def test_iqld_group_equals_standalone_twins_on_every_path(name):
    c = IC.PATHS[name]
    cfg, ds, group, twins = _setup(2, c, betas=[1.0, 3.0], temps=[0.3, 1.0], ds_seed=c['seed'])
    for uc, ua in [(1, 1), (1, 0), (0, 1)]:
        infos, want = _step(group, twins, c['B'], uc, ua, want_info=True)
        _assert_infos(infos, want, uc, ua, f'{name} ({uc}, {ua})')
    if name == 'b2064-binary':   # the rank tie-break of the weight kernel's global-memory branch: every positive weight is 1
        w = group.members[0]._read_rows(2, c['B'])
        assert set(np.unique(w)) == {0.0, 1.0} and (w == 1.0).sum() > int(0.1 * c['B'])
    _check(group, twins, name)
    group.close()


# ---- 3. explicit rows, infos through the C ABI -------------------------------------------------------------------------------------------
def test_iqld_group_explicit_rows_host_and_device():
    """idxs [K, B] as a host array (the group's own stream) and as a CUDA tensor (torch's current stream), alternating with no
    synchronize; every member's rows include N - 1."""
    import torch
    K, B = 3, 64
    cfg, ds, group, twins = _setup(K, IC.case(H=64, B=B, seed=52), temps=[0.3, 1.0, 3.0])
    rng = np.random.default_rng(13)
    N = len(ds['observations'])
    for step, (uc, ua) in enumerate(KINDS):
        idxs = rng.integers(0, N, size=(K, B))
        idxs[:, step % B] = N - 1
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 3 == 0 else idxs, want_info=True, update_critic=uc, update_actor=ua)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=True, update_critic=uc, update_actor=ua)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, uc, ua, f'step {step}')
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), N, np.int64))
    _check(group, twins)
    group.close()


def test_iqld_group_infos_through_the_c_abi():
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's 21 infos in
    fql_read_info_n's layout: the slots of a net that did not step are 0."""
    import torch
    from fql_amd.iql_diffusion import IQLD_INFO_KEYS
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, IC.case(H=64, B=B, seed=53))
    lib = group._lib
    for step, (uc, ua) in enumerate([(1, 0), (1, 1), (0, 1), (0, 0), (1, 1), (0, 1)]):
        if step % 2 == 0:
            host = np.full((K, 21), np.nan, np.float32)
            group._check(lib.fql_iqld_group_update_from_dataset(group._g, None, B, uc, ua, host.ctypes.data, None))
            got = host
        else:
            dev = torch.full((K, 21), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_iqld_group_update_from_dataset(group._g, None, B, uc, ua, dev.data_ptr(), None))
            group.synchronize()
            got = dev.cpu().numpy()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_from_dataset(B, update_critic=uc, update_actor=ua)
            all21 = _all21(t)
            assert got[i].tolist() == [all21[k] for k in IQLD_INFO_KEYS], (step, i)
            assert got[i].tolist() == list(_all21(m).values()), (step, i)
            if not uc:
                assert not got[i, :6].any(), (step, i)
            if not ua:
                assert not got[i, 6:18].any(), (step, i)
            if not (uc or ua):
                assert not got[i].any(), (step, i)
    _check(group, twins)
    group.close()


def _all21(a):
    """All 21 scalars of the handle in buffer order (IQLDiffusionAgent.read_info narrows them to a step kind)."""
    from fql_amd.agent import KindAgent
    return KindAgent.read_info(a)


# ---- 4. ordering without synchronize --------------------------------------------------------------------------------------------------
def test_iqld_group_member_updates_between_group_updates():
    """A member's own critic-only update on the engine's queues and another member's host-batch update between group updates, with no
    synchronize anywhere: the group update is ordered behind them, and they behind it."""
    K, B = 3, 64
    c = IC.case(H=64, B=B, seed=54)
    cfg, ds, group, twins = _setup(K, c)
    batch = O.sample_batch(ds, np.random.default_rng(2).integers(0, len(ds['observations']), size=B))
    noise = DO.make_noise(B, c['ad'], c['S'], 5)

    def sequence(update_all, agents):
        for r in range(3):
            update_all(1, 0)
            agents[0].update_from_dataset(B, update_critic=True, update_actor=False)     # stream left to the engine: its own queues
            agents[1].update(batch, update_critic=False, update_actor=True, noise=noise, want_info=False)   # host batch, explicit noise
            update_all(1, 1)
            update_all(0, 1)

    sequence(lambda uc, ua: group.update_from_dataset(update_critic=uc, update_actor=ua), group.members)
    sequence(lambda uc, ua: [t.update_from_dataset(B, update_critic=uc, update_actor=ua) for t in twins], twins)
    _check(group, twins)
    assert group.members[0].get_steps() == {'updates': 12, 'critic': 9, 'actor': 6}
    assert group.members[1].get_steps() == {'updates': 12, 'critic': 6, 'actor': 9}
    group.close()


def test_iqld_group_member_entry_points_straight_after_group_updates():
    """sample_actions / total_loss / read_rows / get_params of a member straight after a group update see it; a set_params between
    group updates is seen by the next one; network.select answers from the updated critic."""
    K, B = 2, 64
    c = IC.case(H=64, B=B, seed=55)
    cfg, ds, group, twins = _setup(K, c)
    batch = O.sample_batch(ds, np.arange(B))
    noise = DO.make_noise(B, c['ad'], c['S'], 9)
    obs, z = IC.sampler_inputs(7)
    for rnd in range(2):
        for uc, ua in KINDS[:4]:
            _step(group, twins, B, uc, ua)
        for i, (m, t) in enumerate(zip(group.members, twins)):
            _step(group, twins, B, 1, 1)
            np.testing.assert_array_equal(m.sample_actions(obs, noises=z, cfg=3.0), t.sample_actions(obs, noises=z, cfg=3.0))
            _step(group, twins, B, 0, 1)
            for which in range(3):
                np.testing.assert_array_equal(m._read_rows(which, B), t._read_rows(which, B))
            _step(group, twins, B, 1, 0)
            lm, im = m.total_loss(batch, noise=noise)
            lt, it = t.total_loss(batch, noise=noise)
            assert lm == lt and im.keys() == it.keys()
            for k in im:
                np.testing.assert_array_equal(np.asarray(im[k]), np.asarray(it[k]), err_msg=k)
            _step(group, twins, B, 1, 1)
            np.testing.assert_array_equal(m.network.select('critic')(batch['observations'], batch['actions']),
                                          t.network.select('critic')(batch['observations'], batch['actions']))
            _step(group, twins, B, 1, 1)
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
        p = DO.randomize(twins[0].get_params(), 55 + rnd, scale=0.05)
        group.members[0].set_params(p)
        twins[0].set_params(p)
    for uc, ua in KINDS:
        _step(group, twins, B, uc, ua)
    _check(group, twins)
    group.close()


def test_iqld_group_members_checkpoint_as_standalone_agents(tmp_path):
    from fql_amd import checkpoint
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, IC.case(H=64, B=B, seed=56))
    for uc, ua in KINDS[:5]:
        _step(group, twins, B, uc, ua)
    checkpoint.save_agent(group.members[1], str(tmp_path), 5)
    import fql_amd
    b = fql_amd.IQLDiffusionAgent.create(4, ds['observations'][:1], ds['actions'][:1], cfg)   # member 1's create seed
    checkpoint.restore_agent(b, str(tmp_path), 5)
    b.upload_dataset(ds)
    _step(group, twins, B, 1, 1)
    b.update_from_dataset(B)
    _assert_same_state(group.members[1], b, 'restored')
    _check(group, twins)
    group.close()


# ---- 5. sampling ----------------------------------------------------------------------------------------------------------------------
def _sampler_group(K, c):
    """A group whose members carry sampler parameters (the head scaled so that the clip is reached), each member its own."""
    import fql_amd
    cfg = IC.config(c)
    ex_o, ex_a = np.zeros((1, c['od']), np.float32), np.zeros((1, c['ad']), np.float32)
    group = fql_amd.IQLDiffusionAgentGroup.create([3 + i for i in range(K)], ex_o, ex_a, cfg)
    for i, m in enumerate(group.members):
        p = DO.randomize(m.get_params(), 80 + i)
        p['actor']['Dense_0']['kernel'] = (p['actor']['Dense_0']['kernel'] * np.float32(IC.SAMPLER_HEAD_SCALE if c['H'] < 512 else IC.SAMPLER512_HEAD_SCALE)).astype(np.float32)
        m.set_params(p)
    return group


@pytest.mark.parametrize('K, c', [(2, IC.case(H=64, B=16, seed=80)), (3, IC.case(H=64, B=16, seed=80)), (2, IC.case(od=69, ad=21, H=512, B=16, seed=81))],
                         ids=['K2-H64', 'K3-H64', 'K2-obs69-act21-H512'])
def test_iqld_group_sample_actions_equal_the_members_own(K, c):
    import torch
    od, ad = c['od'], c['ad']
    group = _sampler_group(K, c)
    ms = group.members
    before = [leaf_dict(m.get_params()) for m in ms]
    rng = np.random.default_rng(17)
    side = torch.cuda.Stream()
    for n in (1, 10, 37, 2049):
        obs = rng.standard_normal((K, n, od)).astype(np.float32)
        z = rng.standard_normal((K, n, ad)).astype(np.float32)
        for cfg_w in (0.0, 3.0):    # a scalar
            got = group.sample_actions(obs, noises=z, cfg=cfg_w)
            assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0 and (cfg_w == 0.0 or n == 1 or (np.abs(got) == 1.0).any())
            for i in range(K):
                np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i], cfg=cfg_w).reshape(n, ad), err_msg=f'n {n} cfg {cfg_w} member {i}')
        per_member = [0.0, 1.5, 3.0][:K]
        got = group.sample_actions(obs, noises=z, cfg=per_member)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i], cfg=per_member[i]).reshape(n, ad), err_msg=f'n {n} per member {i}')
        per_row = rng.uniform(0.0, 5.0, size=(K, n)).astype(np.float32)
        per_row[:, 0] = 0.0
        got = group.sample_actions(obs, noises=z, cfg=per_row)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions_rows(obs[i], per_row[i], noises=z[i]), err_msg=f'n {n} per row member {i}')
            for j in sorted({0, n // 2, n - 1}):   # row j at its own weight is the member's scalar call
                np.testing.assert_array_equal(got[i, j], ms[i].sample_actions(obs[i, j], noises=z[i, j], cfg=float(per_row[i, j])))
        if n == 2049 and c['H'] >= 512:
            continue
        seeds = [50 + n + i for i in range(K)]
        got = group.sample_actions(obs, seed=seeds, cfg=3.0)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=seeds[i], cfg=3.0).reshape(n, ad), err_msg=f'n {n} seeds member {i}')
        got = group.sample_actions(obs, seed=9, cfg=per_row)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions_rows(obs[i], per_row[i], seed=9), err_msg=f'n {n} one seed member {i}')
        # one shared block of rows against the same rows tiled
        shared = group.sample_actions(obs[0], seed=seeds, cfg=per_member)
        np.testing.assert_array_equal(shared, group.sample_actions(np.tile(obs[:1], (K, 1, 1)), seed=seeds, cfg=per_member))
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].sample_actions(obs[0], seed=seeds[i], cfg=per_member[i]).reshape(n, ad))
        # CUDA tensors on a side stream, the weights on the device too
        with torch.cuda.stream(side):
            to, tz, tw = torch.from_numpy(obs).cuda(), torch.from_numpy(z).cuda(), torch.from_numpy(per_row).cuda()
            tg = group.sample_actions(to, noises=tz, cfg=tw)
            assert tg.is_cuda and tuple(tg.shape) == (K, n, ad)
            want = [ms[i].sample_actions_rows(to[i], tw[i], noises=tz[i]) for i in range(K)]
        side.synchronize()
        for i in range(K):
            np.testing.assert_array_equal(tg[i].cpu().numpy(), want[i].cpu().numpy(), err_msg=f'n {n} cuda member {i}')
            np.testing.assert_array_equal(tg[i].cpu().numpy(), ms[i].sample_actions_rows(obs[i], per_row[i], noises=z[i]))
    # unseeded: member i's counter advances once per fused call, as by its own call
    o7 = rng.standard_normal((K, 7, od)).astype(np.float32)
    calls = [m._sample_calls for m in ms]
    a, b = group.sample_actions(o7, cfg=3.0), group.sample_actions(o7, cfg=3.0)
    assert [m._sample_calls for m in ms] == [x + 2 for x in calls] and np.abs(a - b).max() > 0
    with pytest.raises(ValueError):
        group.sample_actions(o7, cfg=float('inf'))
    w = np.ones((K, 7), np.float32)
    w[K - 1, 3] = np.nan   # past the Python check: the library refuses a non-finite host weight itself
    oa, wa, out = np.ascontiguousarray(o7), np.ascontiguousarray(w), np.zeros((K, 7, ad), np.float32)
    seeds = (C.c_uint64 * K)(*range(K))
    from fql_amd import _cabi
    assert group._lib.fql_iqld_group_sample_actions(group._g, oa.ctypes.data, 7, None, seeds, wa.ctypes.data, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'finite' in group._lib.fql_last_error(None)
    # no state change
    group.synchronize()
    for i, m in enumerate(ms):
        after = leaf_dict(m.get_params())
        for k in after:
            np.testing.assert_array_equal(after[k], before[i][k], err_msg=f'member {i} {k}')
        assert m.get_steps() == {'updates': 0, 'critic': 0, 'actor': 0}
    group.close()


def test_iqld_group_sampling_sees_group_updates_without_a_synchronize():
    K, B = 2, 64
    cfg, ds, group, twins = _setup(K, IC.case(H=64, B=B, seed=57))
    obs = np.random.default_rng(4).standard_normal((K, 10, 29)).astype(np.float32)
    for rnd in range(3):
        for uc, ua in [(1, 1), (0, 1)]:
            _step(group, twins, B, uc, ua)
        got = group.sample_actions(obs, seed=21 + rnd, cfg=3.0)
        for i in range(K):
            np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], seed=21 + rnd, cfg=3.0), err_msg=f'round {rnd} member {i}')
    _check(group, twins)
    group.close()


# ---- 6. launch counts -----------------------------------------------------------------------------------------------------------------
def test_iqld_group_launch_counts_do_not_depend_on_k():
    """A fused program has a member's launch count, whatever K: 39 / 32 / 26 / 1 at the default shape (hidden 512 x 4, B 256; DESIGN.md
    section 18); a fused sampling chunk costs what the member's sweep call does, 4 + S (hidden layers + head) + 1."""
    import fql_amd
    c = IC.case(H=512, B=256, seed=58)
    ex_o, ex_a = np.zeros((1, c['od']), np.float32), np.zeros((1, c['ad']), np.float32)
    counts = set()
    for K in (1, 2, 4):
        group = fql_amd.IQLDiffusionAgentGroup.create(list(range(K)), ex_o, ex_a, IC.config(c), softmax_betas=[1.0 + i for i in range(K)])
        la = group.launches()
        m = group.members[K - 1]
        assert la[:4] == tuple(m.iqld_stats(uc, ua)[0] for uc, ua in [(1, 1), (1, 0), (0, 1), (0, 0)]), K
        assert la[4] == m.sample_cfgs_stats(), K
        counts.add(la)
        group.close()
        for x in group.members:
            x.close()
    assert counts == {(39, 32, 26, 1, 4 + 16 * 5 + 1)}, counts


# ---- 7. refusals and release ----------------------------------------------------------------------------------------------------------
def test_iqld_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    c = IC.case(H=64, B=64, seed=59)
    B, od, ad = c['B'], c['od'], c['ad']
    cfg = IC.config(c)
    ds = O.make_synthetic_dataset(256, od, ad, seed=1)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]

    def create(members, fn=lib.fql_iqld_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def iqld(seed, **kw):
        return fql_amd.IQLDiffusionAgent.create(seed, ex_o, ex_a, dict(cfg, **kw))

    a, twin_a = iqld(0), iqld(0)
    fq_cfg = fql_amd.get_config()
    fq_cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    f0, f1 = fql_amd.FQLAgent.create(0, ex_o, ex_a, fq_cfg), fql_amd.FQLAgent.create(1, ex_o, ex_a, fq_cfg)
    rb_cfg = fql_amd.rebrac.get_config()
    rb_cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    r0 = fql_amd.ReBRACAgent.create(0, ex_o, ex_a, rb_cfg)
    for other in (f0, r0):    # another kind's handle
        rc, g = create([a, other])
        assert rc == _cabi.FQL_E_STATE and not g.value and b'IQL-diffusion' in lib.fql_last_error(None), lib.fql_last_error(None)
    bad = dict(expectile=iqld(1, expectile=0.7), optimal_var=iqld(2, optimal_var='binary'), target_extraction=iqld(3, target_extraction=0),
               actor_lr=iqld(4, actor_lr=1e-4), hidden=iqld(5, hidden_dims=(128,) * 4, actor_hidden_dims=(128,) * 4), batch=iqld(6, batch_size=32))
    for what, x in bad.items():
        rc, g = create([a, x])
        assert rc == _cabi.FQL_E_INVALID and not g.value, (what, lib.fql_last_error(None))
        assert b'member 1' in lib.fql_last_error(None), what
    assert create([a, a])[0] == _cabi.FQL_E_INVALID and b'twice' in lib.fql_last_error(None)
    for fn in (lib.fql_group_create, lib.fql_rebrac_group_create):     # the other kinds' creates keep refusing IQL-diffusion handles
        rc, g = create([a, iqld(9)], fn=fn)
        assert rc == _cabi.FQL_E_STATE and not g.value
    b, twin_b = iqld(5, awr_temperature=2.0, softmax_beta=1.0), iqld(5, awr_temperature=2.0, softmax_beta=1.0)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID and b'already' in lib.fql_last_error(None)
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # the FQL and ReBRAC group calls on an IQL-diffusion group name the call that serves it
    o, out = np.zeros((2, 1, od), np.float32), np.zeros((2, 1, ad), np.float32)
    z, w, seeds, v = np.zeros((2, 1, ad), np.float32), np.ones((2, 1), np.float32), (C.c_uint64 * 2)(1, 2), C.c_int64(-1)
    for rc in (lib.fql_group_update_from_dataset(g, None, B, None, None),
               lib.fql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, out.ctypes.data, None),
               lib.fql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None),
               lib.fql_group_sample_stats(g, 0, C.byref(v)),
               lib.fql_rebrac_group_update_from_dataset(g, None, B, 1, None, None),
               lib.fql_rebrac_group_sample_actions(g, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None),
               lib.fql_rebrac_group_stats(g, C.byref(v), None, None)):
        assert rc == _cabi.FQL_E_STATE and b'fql_iqld_group_' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1
    # and the IQL-diffusion group calls on an FQL and on a ReBRAC group
    rc, fg = create([f0, f1], fn=lib.fql_group_create)
    assert rc == _cabi.FQL_OK and fg.value
    rc, rg = create([r0], fn=lib.fql_rebrac_group_create)
    assert rc == _cabi.FQL_OK and rg.value
    la = (C.c_int64 * 4)(-1, -1, -1, -1)
    for og, name in ((fg, b'fql_group_'), (rg, b'fql_rebrac_group_')):
        for rc in (lib.fql_iqld_group_update_from_dataset(og, None, B, 1, 1, None, None),
                   lib.fql_iqld_group_sample_actions(og, o.ctypes.data, 1, None, seeds, w.ctypes.data, out.ctypes.data, None),
                   lib.fql_iqld_group_stats(og, la, C.byref(v))):
            assert rc == _cabi.FQL_E_STATE and name in lib.fql_last_error(None), lib.fql_last_error(None)
    assert list(la) == [-1] * 4 and v.value == -1
    assert lib.fql_group_destroy(fg) == _cabi.FQL_OK and lib.fql_group_destroy(rg) == _cabi.FQL_OK
    assert lib.fql_iqld_group_update_from_dataset(g, None, 32, 1, 1, None, None) == _cabi.FQL_E_INVALID   # another batch size
    assert lib.fql_iqld_group_update_from_dataset(g, None, B, 1, 0, None, None) == _cabi.FQL_E_INVALID    # no dataset uploaded
    # released: plain handles again, bitwise with their twins through grouped and standalone steps
    for x in (a, b, twin_a, twin_b):
        x.upload_dataset(ds)
    for uc, ua in [(1, 0), (1, 1), (0, 1)]:
        assert lib.fql_iqld_group_update_from_dataset(g, None, B, uc, ua, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B, update_critic=uc, update_actor=ua)
    assert lib.fql_group_synchronize(g) == _cabi.FQL_OK
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    for uc, ua in [(1, 0), (1, 1)]:
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B, update_critic=uc, update_actor=ua)
    _assert_same_state(a, twin_a, 'released member 0')
    _assert_same_state(b, twin_b, 'released member 1')
    for x in [a, b, twin_a, twin_b, f0, f1, r0] + list(bad.values()):
        x.close()
