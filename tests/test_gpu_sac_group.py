"""GPU: SAC agent groups (fql_sac_group_*, SACAgentGroup).  A member advanced by the group's fused program - offline or with RLPD's
balanced batches out of its own replay ring - and sampled by the fused call must be bitwise where its standalone twin is (same seed,
target_entropy, parameters, dataset, ring and rows): fusing changes which launch a task rides in, never its arithmetic.  The standalone
agent is held to the fp64 restatement tests/sac_oracle.py by tests/test_gpu_sac.py, so the twin is a checked reference and no tolerance
is involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import sac_oracle as SO
from tests.test_gpu_sac import _randomized
from tests.util import leaf_dict

pytestmark = pytest.mark.gpu
H32 = ((32, 32), (32, 32))
H64x2 = ((64, 64), (64, 64))
H64 = ((64,) * 4, (64,) * 4)
H512 = ((512,) * 4, (512,) * 4)


def _state(a):
    """Every array and counter of an agent: parameters (modules_alpha/log_value and the target critic among them), both Adam moments,
    the counters."""
    a.synchronize()
    opt = a.get_opt_state()
    out = {f'params/{k}': v for k, v in leaf_dict(a.get_params()).items()}
    for part in ('mu', 'nu'):
        out.update({f'{part}/{k}': v for k, v in leaf_dict(opt[part]).items()})
    return out, (opt['count'], opt['step'])


def _assert_same_state(a, b, what='', infos=True):
    (sa, ca), (sb, cb) = _state(a), _state(b)
    assert sa.keys() == sb.keys() and ca == cb, (what, ca, cb)
    assert 'params/modules_alpha/log_value' in sa and sum(k.startswith('params/modules_target_critic') for k in sa) >= 2
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f'{what} {k}')
    if infos:
        ia, ib = a.read_info(), b.read_info()
        assert len(ia) == 14 and ia == ib, what


def _setup(K, B, hidden=H64, od=29, ad=8, tes=None, seeds=None, ds_seed=7, upload=True, **kw):
    """A group of K members and their standalone twins on one dataset: member and twin share the create seed, the target entropy and the
    randomised parameters (wide head biases: the log-std clip and the tanh saturation occur; log_value != 0; target != critic); members
    differ from each other in all of them unless the caller says otherwise."""
    import fql_amd
    cfg = fql_amd.sac.get_config()
    cfg.update(actor_hidden_dims=tuple(hidden[0]), value_hidden_dims=tuple(hidden[1]), batch_size=B)
    cfg.update(kw)
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=ds_seed)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
    seeds = [3 + i for i in range(K)] if seeds is None else list(seeds)
    tes = ([None, -1.0, -3.5, -0.25, -6.0] * 2)[:K] if tes is None else list(tes)
    group = fql_amd.SACAgentGroup.create(seeds, ex_o, ex_a, cfg, target_entropies=tes)
    twins = []
    for i in range(K):
        t = fql_amd.SACAgent.create(seeds[i], ex_o, ex_a, dict(cfg, target_entropy=tes[i]))
        p = _randomized(t.get_params(), 100 + i)
        t.set_params(p)
        group.members[i].set_params(p)
        twins.append(t)
    if upload:
        group.upload_dataset(ds)
        for t in twins:
            t.upload_dataset(ds)
    assert all(type(m) is fql_amd.SACAgent for m in group.members)
    assert [m.config['target_entropy'] for m in group.members] == [t.config['target_entropy'] for t in twins]
    return cfg, ds, group, twins


def _assert_infos(infos, want, what):
    from fql_amd.sac import SAC_INFO_KEYS
    assert len(infos) == len(want)
    for i, (g, w) in enumerate(zip(infos, want)):
        g, w = g.to_dict(), w.to_dict()
        assert tuple(g) == SAC_INFO_KEYS == tuple(w), (what, i)
        for k in g:
            np.testing.assert_array_equal(np.asarray(g[k]), np.asarray(w[k]), err_msg=f'{what} member {i} {k}')


def _check(group, twins, what=''):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'{what} member {i}')


def _transition(ds, i, rew=None):
    return {'observations': ds['observations'][i], 'actions': ds['actions'][i], 'rewards': float(ds['rewards'][i]) if rew is None else rew,
            'masks': float(ds['masks'][i]), 'next_observations': ds['next_observations'][i]}


# ---- 1. twins, device RNG and explicit rows ----------------------------------------------------------------------------------------------
SHAPES = {
    'b16-act3': (7, 3, 16, H32, {}),                                                   # one row tile; a partly filled block of the act kernel
    'b48-actor-ln': (29, 8, 48, H64, dict(actor_layer_norm=True)),                     # three row tiles; B not a multiple of 32
    'act17': (11, 17, 32, H64x2, {}),                                                  # ap = 32: the head layer is 64 columns
    'act16-plain': (17, 16, 32, H64x2, dict(tanh_squash=False, backup_entropy=True, q_agg='mean')),   # a full 16-column action block
}


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('case', list(SHAPES))
def test_sac_group_equals_standalone_twins(case, K):
    """Six update_from_dataset steps, alternating each member's device draw with explicit [K, B] rows (a host array, then a CUDA tensor on
    torch's current stream), distinct target entropies.  After every step the 14 infos of every member against its twin's; at the end
    every parameter leaf, both Adam moments and the counters."""
    import torch
    od, ad, B, hidden, kw = SHAPES[case]
    cfg, ds, group, twins = _setup(K, B, hidden, od=od, ad=ad, **kw)
    N = len(ds['observations'])
    rng = np.random.default_rng(5)
    for step in range(6):
        idxs = None
        if step % 2:
            idxs = rng.integers(0, N, size=(K, B))
            idxs[:, step % B] = N - 1
        arg = torch.from_numpy(idxs).cuda() if step == 3 else idxs
        infos = group.update_from_dataset(idxs=arg, want_info=True)
        want = [t.update_from_dataset(B, idxs=None if idxs is None else idxs[i], want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, f'{case} step {step}')
    _check(group, twins, case)
    assert group.members[0].get_opt_state()['count'] == 6
    group.close()


def test_sac_group_equals_standalone_twins_b256_hidden_512():
    """K = 2 at B 256, hidden 512 x 4: 64-row tiles, and the act kernel's 2 B = 512 rows across two blocks."""
    K, B = 2, 256
    cfg, ds, group, twins = _setup(K, B, H512)
    for step in range(2):
        infos = group.update_from_dataset(want_info=True)
        want = [t.update_from_dataset(B, want_info=True)[1] for t in twins]
        _assert_infos(infos, want, f'step {step}')
    _check(group, twins)
    group.close()


# ---- 2. target_entropy alone -------------------------------------------------------------------------------------------------------------
def test_sac_group_target_entropy_alone_moves_only_the_temperature():
    """Two members in one state (create seed, parameters) on one set of rows, target entropies -200 and 200: after one step every critic
    leaf is bitwise equal; alpha_loss and modules_alpha/log_value are not.  (The targets lie on either side of any entropy eight
    Gaussians with log-std in [-5, 2] can have: from zero moments Adam moves log_value by lr sign(g), so two targets on one side of the
    entropy would leave it equal.)"""
    K, B = 2, 32
    cfg, ds, group, twins = _setup(K, B, H64x2, seeds=[5, 5], tes=[-200.0, 200.0])
    p = _randomized(twins[0].get_params(), 77)
    for a in list(group.members) + twins:
        a.set_params(p)
    idx = np.random.default_rng(3).integers(0, len(ds['observations']), size=B)
    infos = group.update_from_dataset(idxs=np.stack([idx, idx]), want_info=True)
    want = [t.update_from_dataset(B, idxs=idx, want_info=True)[1] for t in twins]
    _assert_infos(infos, want, 'first step')
    _check(group, twins)
    a, b = infos[0].to_dict(), infos[1].to_dict()
    assert a['actor/alpha_loss'] != b['actor/alpha_loss']
    for k in ('critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min', 'actor/actor_loss', 'actor/entropy', 'actor/alpha'):
        assert a[k] == b[k], k
    pa, pb = leaf_dict(group.members[0].get_params()), leaf_dict(group.members[1].get_params())
    critic = [k for k in pa if k.startswith('modules_critic') or k.startswith('modules_target_critic')]
    assert len(critic) >= 4
    for k in critic:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    assert pa['modules_alpha/log_value'] != pb['modules_alpha/log_value']
    group.close()


# ---- 3. balanced twins -------------------------------------------------------------------------------------------------------------------
def test_sac_group_update_balanced_equals_the_twins_own():
    """K = 3, B 16, every member its own dataset copy and its own ring of capacity 8 holding 3, 8 and 11 inserted rows: the second is
    full, the third has wrapped.  The ring keeps the reference's size = max(pointer, size) (utils/datasets.py:489-491), so a ring of
    capacity 8 that has wrapped reports (7, 3), not (8, 3).  Four steps alternate engine-RNG draws and explicit (dataset_idxs,
    replay_idxs) - host arrays, then CUDA tensors; after every step each member equals its twin's update_balanced."""
    import torch
    K, B, cap = 3, 16, 8
    cfg, ds, group, twins = _setup(K, B, H32, od=7, ad=3)
    group.create_replay_buffers(cap)
    N = len(ds['observations'])
    for i, (n, t) in enumerate(zip((3, 8, 11), twins)):
        t.create_replay_buffer(cap)
        for j in range(n):
            tr = _transition(ds, 10 * i + j, rew=50.0 + 10 * i + j)
            group.members[i].add_transition(tr, replay=True)
            t.add_transition(tr, replay=True)
    sizes = [m.replay_size() for m in group.members]
    assert sizes == [t.replay_size() for t in twins] == [(3, 3), (7, 0), (7, 3)]
    rng = np.random.default_rng(9)
    for step in range(4):
        if step % 2 == 0:
            infos = group.update_balanced(want_info=True)
            want = [t.update_balanced(B, want_info=True)[1] for t in twins]
        else:
            di = rng.integers(0, N, size=(K, B // 2))
            ri = np.stack([rng.integers(0, m.replay_size()[0], size=B // 2) for m in group.members])
            di[:, 0], ri[:, 0] = N - 1, [m.replay_size()[0] - 1 for m in group.members]
            arg = (torch.from_numpy(di).cuda(), torch.from_numpy(ri).cuda()) if step == 3 else (di, ri)
            infos = group.update_balanced(idxs=arg, want_info=True)
            want = [t.update_balanced(B, idxs=(di[i], ri[i]), want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, f'step {step}')
        _check(group, twins, f'step {step}')
    # the ring rows carry rewards >= 50: a batch drawn from the dataset alone could not reach this target
    assert infos[0].to_dict()['critic/critic_loss'] > 100.0
    with pytest.raises(ValueError):      # one past member 0's three rows, inside the others' eight: refused on the host
        group.update_balanced(idxs=(np.zeros((K, B // 2), np.int64), np.full((K, B // 2), 3, np.int64)))
    with pytest.raises(ValueError):      # one array without the other
        group._check(group._lib.fql_sac_group_update_balanced(group._g, np.zeros((K, B // 2), np.int64).ctypes.data, None, B, None, None))
    _check(group, twins, 'after the refusals')
    group.close()


def test_sac_group_update_balanced_refuses_an_empty_ring_before_any_member_moves():
    """K = 2, member 1's ring left empty: FQL_E_INVALID naming the member, and both members' parameters, Adam moments and counters are
    what they were.  SAC has no per-row read-back of its draws; that the RNG step did not move either shows in the next step, whose
    device draws (rows, eps_n, eps_c) are bitwise those of twins that never saw the refused call."""
    from fql_amd import _cabi
    K, B = 2, 16
    cfg, ds, group, twins = _setup(K, B, H32, od=7, ad=3)
    lib = group._lib
    # no ring at all, then member 0's filled and member 1's empty
    assert lib.fql_sac_group_update_balanced(group._g, None, None, B, None, None) == _cabi.FQL_E_INVALID
    assert b'member 0' in lib.fql_last_error(None) and b'no replay ring' in lib.fql_last_error(None), lib.fql_last_error(None)
    group.create_replay_buffers(8)
    for t in twins:
        t.create_replay_buffer(8)
    group.update_from_dataset()
    for t in twins:
        t.update_from_dataset(B)
    for a in (group.members[0], twins[0]):
        for j in range(3):
            a.add_transition(_transition(ds, j, rew=20.0 + j), replay=True)
    before = [_state(m) for m in group.members]
    assert lib.fql_sac_group_update_balanced(group._g, None, None, B, None, None) == _cabi.FQL_E_INVALID
    assert b'member 1' in lib.fql_last_error(None) and b'empty' in lib.fql_last_error(None), lib.fql_last_error(None)
    with pytest.raises(ValueError, match='member 1'):
        group.update_balanced()
    assert lib.fql_sac_group_update_balanced(group._g, None, None, B + 2, None, None) == _cabi.FQL_E_INVALID   # another batch size
    for i, m in enumerate(group.members):
        (arrays, counters), (arrays0, counters0) = _state(m), before[i]
        assert counters == counters0
        for k in arrays:
            np.testing.assert_array_equal(arrays[k], arrays0[k], err_msg=f'member {i} {k}')
    _check(group, twins, 'after the refusal')
    for a in (group.members[1], twins[1]):
        a.add_transition(_transition(ds, 5, rew=30.0), replay=True)
    infos = group.update_balanced(want_info=True)
    want = [t.update_balanced(B, want_info=True)[1] for t in twins]
    _assert_infos(infos, want, 'the step after the refusal')
    _check(group, twins, 'the step after the refusal')
    group.close()


# ---- 4. the RLPD loop --------------------------------------------------------------------------------------------------------------------
def test_sac_group_rlpd_loop_equals_two_solo_loops():
    """main.py:217-259 with --offline_steps=0 --balanced_sampling=1 for K = 2 seeds, 12 steps, B 32 (the loop of
    tests/test_gpu_sac.py::test_rlpd_loop_against_restatement, whose toy environment lives inside that test and is restated here): the
    group runs the fused sample_actions on one observation per member, K environment steps, add_transitions and update_balanced on each
    member's device RNG; two solo agents run their own loops.  Actions at every step and the final state are bitwise equal."""
    K, B, od, ad = 2, 32, 29, 8
    cfg, ds, group, twins = _setup(K, B, H64)
    group.create_replay_buffers(1000)
    for t in twins:
        t.create_replay_buffer(1000)
    rng = np.random.default_rng(14)
    W = rng.standard_normal((K, ad, od)).astype(np.float32) * 0.1     # one toy environment per member
    ob_g = rng.standard_normal((K, od)).astype(np.float32)
    ob_s = ob_g.copy()
    resets = rng.standard_normal((12, K, od)).astype(np.float32)

    def env_step(i, ob, action, step):
        nob = (0.9 * ob + action @ W[i]).astype(np.float32)
        m = 0.0 if step % 5 == 4 else 1.0
        t = {'observations': ob, 'actions': action, 'rewards': float(-np.square(action).sum()), 'masks': m, 'next_observations': nob}
        return t, (nob if m else resets[step, i])

    for step in range(12):
        actions = group.sample_actions(ob_g)
        assert actions.shape == (K, ad)
        trs = []
        for i in range(K):
            tr, ob_g[i] = env_step(i, ob_g[i].copy(), actions[i], step)
            trs.append(tr)
        group.add_transitions(trs)
        group.update_balanced()
        for i, t in enumerate(twins):
            a = t.sample_actions(ob_s[i])
            np.testing.assert_array_equal(actions[i], a, err_msg=f'step {step} member {i}')
            tr, ob_s[i] = env_step(i, ob_s[i].copy(), a, step)
            t.add_transition(tr, replay=True)
            t.update_balanced(B)
    assert [m.replay_size()[0] for m in group.members] == [12] * K
    _check(group, twins)
    assert group.members[0].get_opt_state()['count'] == 12
    group.close()


# ---- 5. the members' own work between group calls, no synchronize ------------------------------------------------------------------------
def test_sac_group_member_work_between_group_updates(tmp_path):
    """Between two group updates and with no synchronize anywhere: a member's add_transition(replay=True), total_loss, sample_actions,
    get_params / set_params and a checkpoint round trip of one member.  The group update is ordered behind them, and they behind it."""
    from fql_amd import checkpoint
    K, B, ad = 3, 32, 8
    cfg, ds, group, twins = _setup(K, B, H64x2)
    ms = group.members
    group.create_replay_buffers(16)
    for t in twins:
        t.create_replay_buffer(16)
    for a in ms + twins:
        a.add_transition(_transition(ds, 0, rew=9.0), replay=True)
    batch = O.sample_batch(ds, np.random.default_rng(2).integers(0, len(ds['observations']), size=B))
    noise = SO.make_noise(B, ad, 5)
    obs = ds['observations'][:7]
    for rnd in range(2):
        group.update_balanced()
        for t in twins:
            t.update_balanced(B)
        for i, (m, t) in enumerate(zip(ms, twins)):     # straight after a group update: every call sees it
            tr = _transition(ds, 3 + 4 * rnd + i, rew=11.0 + i)
            m.add_transition(tr, replay=True)
            t.add_transition(tr, replay=True)
            assert m.total_loss(batch, noise=noise) == t.total_loss(batch, noise=noise), (rnd, i)
            np.testing.assert_array_equal(m.sample_actions(obs, seed=11), t.sample_actions(obs, seed=11), err_msg=f'round {rnd} member {i}')
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
        p = _randomized(twins[2].get_params(), 55 + rnd)
        ms[2].set_params(p)
        twins[2].set_params(p)
        d = tmp_path / f'r{rnd}'
        d.mkdir()
        checkpoint.save_agent(ms[0], str(d), 1)
        checkpoint.restore_agent(ms[1], str(d), 1)
        checkpoint.restore_agent(twins[1], str(d), 1)
        infos = group.update_balanced(want_info=True)
        want = [t.update_balanced(B, want_info=True)[1] for t in twins]
        _assert_infos(infos, want, f'round {rnd}')
        got = group.sample_actions(obs, seed=21 + rnd)   # the fused sampler straight after a group update
        for i, t in enumerate(twins):
            np.testing.assert_array_equal(got[i], t.sample_actions(obs, seed=21 + rnd), err_msg=f'fused sampler round {rnd} member {i}')
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    _check(group, twins)
    assert [m.replay_size()[0] for m in ms] == [3] * K
    group.close()


# ---- 6. the fused Gaussian sampler -------------------------------------------------------------------------------------------------------
def _rows(K, n, od, ad, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n, od)).astype(np.float32), (2.0 * rng.standard_normal((K, n, ad))).astype(np.float32)


@pytest.mark.parametrize('K', [2, 3])
def test_sac_group_sample_actions_equal_the_members_own(K):
    """n = 1, 5 and 37 rows per member: explicit noises, K seeds, one seed, seed None; temperature 0 and 1; host arrays and CUDA tensors
    on a side stream; one shared block of rows."""
    import torch
    od, ad = 29, 8
    cfg, ds, group, twins = _setup(K, 32, H64, upload=False)
    ms = group.members
    before = [_state(m) for m in ms]
    side = torch.cuda.Stream()
    for n in (1, 5, 37):
        obs, z = _rows(K, n, od, ad, 17 + n)
        seeds = [50 + n + i for i in range(K)]
        for temp in (0.0, 1.0):
            got = group.sample_actions(obs, noises=z, temperature=temp)
            assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0
            drawn = group.sample_actions(obs, seed=seeds, temperature=temp)
            for i in range(K):
                np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], noises=z[i], temperature=temp), err_msg=f'n {n} T {temp} noises member {i}')
                np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i], temperature=temp), err_msg=f'n {n} T {temp} noises twin {i}')
                np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=seeds[i], temperature=temp), err_msg=f'n {n} T {temp} seeds twin {i}')
            if temp == 0.0:
                np.testing.assert_array_equal(drawn, got)
            else:
                assert not np.array_equal(drawn, got)
        got = group.sample_actions(obs, seed=9)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], seed=9), err_msg=f'n {n} one seed member {i}')
        shared = group.sample_actions(obs[0], seed=seeds)     # one shared block of rows against the same rows tiled
        np.testing.assert_array_equal(shared, group.sample_actions(np.tile(obs[:1], (K, 1, 1)), seed=seeds))
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].sample_actions(obs[0], seed=seeds[i]))
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
    for i, m in enumerate(ms):      # no parameter or optimizer state changed
        (arrays, counters), (arrays0, counters0) = _state(m), before[i]
        assert counters == counters0
        for k in arrays:
            np.testing.assert_array_equal(arrays[k], arrays0[k], err_msg=f'member {i} {k}')
    group.close()


def test_sac_group_sample_actions_hidden_512_act17():
    """act 17 (padded action width 32: a 64-column head layer), hidden 512 x 4, n = 37."""
    K, n, od, ad = 2, 37, 29, 17
    cfg, ds, group, twins = _setup(K, 32, H512, od=od, ad=ad, upload=False)
    obs, z = _rows(K, n, od, ad, 23)
    got = group.sample_actions(obs, noises=z)
    drawn = group.sample_actions(obs, seed=[8, 9], temperature=0.7)
    mode = group.sample_actions(obs, seed=1, temperature=0.0)
    for i in range(K):
        np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises twin {i}')
        np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=8 + i, temperature=0.7), err_msg=f'seeds twin {i}')
        np.testing.assert_array_equal(mode[i], twins[i].sample_actions(obs[i], seed=1, temperature=0.0), err_msg=f'mode twin {i}')
    group.close()


def test_sac_group_sample_actions_across_the_4096_row_chunk():
    """n = 4100 crosses the 4096-row chunk edge: the second chunk's rows keep their numbers in the call, so a seeded draw does not depend
    on the chunking, with different observations in every row and with one observation in every row."""
    K, n, od, ad = 2, 4100, 7, 3
    cfg, ds, group, twins = _setup(K, 16, H32, od=od, ad=ad, tanh_squash=False, upload=False)
    obs, z = _rows(K, n, od, ad, 31)
    got = group.sample_actions(obs, noises=z)
    drawn = group.sample_actions(obs, seed=[5, 6])
    same = np.repeat(obs[:, :1], n, axis=1)
    rep = group.sample_actions(same, seed=[5, 6])
    for i in range(K):
        np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], noises=z[i]), err_msg=f'noises twin {i}')
        np.testing.assert_array_equal(drawn[i], twins[i].sample_actions(obs[i], seed=5 + i), err_msg=f'seeds twin {i}')
        np.testing.assert_array_equal(rep[i], twins[i].sample_actions(same[i], seed=5 + i), err_msg=f'same rows twin {i}')
    group.close()


# ---- 7. launch counts --------------------------------------------------------------------------------------------------------------------
def test_sac_group_launch_counts_do_not_depend_on_k():
    """The fused update has a member's launch count, whatever K.  A sampling chunk is assemble, the actor (four hidden layers and the
    [H, 2 ap] head layer, each reading the one before: one launch per layer) and the action kernel: 7."""
    for K in (1, 2, 5):
        cfg, ds, group, twins = _setup(K, 16, H64, upload=False)
        assert group.launches() == (twins[0].sac_stats()[0], 7), K
        assert group.members[0].sac_stats()[0] == twins[0].sac_stats()[0]
        group.close()


# ---- 8. infos through the C ABI ----------------------------------------------------------------------------------------------------------
def test_sac_group_infos_through_the_c_abi():
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's 14 infos in
    fql_read_info_n's order, from the dataset update and from the balanced one; nothing is written behind them."""
    import torch
    K, B, n = 3, 16, 14
    cfg, ds, group, twins = _setup(K, B, H32, od=7, ad=3)
    lib = group._lib
    assert lib.fql_num_info(group.members[0]._h) == n
    group.create_replay_buffers(4)
    for m in group.members:
        m.add_transition(_transition(ds, 1), replay=True)
    for t in twins:
        t.create_replay_buffer(4)
        t.add_transition(_transition(ds, 1), replay=True)
    for step in range(4):
        balanced = step >= 2

        def call(ptr):
            if balanced:
                return lib.fql_sac_group_update_balanced(group._g, None, None, B, ptr, None)
            return lib.fql_sac_group_update_from_dataset(group._g, None, B, ptr, None)
        if step % 2 == 0:
            host = np.full((K * n + 3,), np.nan, np.float32)
            group._check(call(host.ctypes.data))
            got, tail = host[:K * n].reshape(K, n), host[K * n:]
        else:
            dev = torch.full((K * n + 3,), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(call(dev.data_ptr()))
            group.synchronize()
            got, tail = dev.cpu().numpy()[:K * n].reshape(K, n), dev.cpu().numpy()[K * n:]
        assert np.isnan(tail).all()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_balanced(B) if balanced else t.update_from_dataset(B)
            assert got[i].tolist() == list(m.read_info().values()), (step, i)
            assert got[i].tolist() == list(t.read_info().values()), (step, i)
    _check(group, twins)
    group.close()


# ---- 9. refusals and release -------------------------------------------------------------------------------------------------------------
def test_sac_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    B, od, ad = 32, 29, 8
    cfg = fql_amd.sac.get_config()
    cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    ds = O.make_synthetic_dataset(4 * B, od, ad, seed=1)
    ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]

    def create(members, fn=lib.fql_sac_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def sac(seed, **kw):
        return fql_amd.SACAgent.create(seed, ex_o, ex_a, dict(cfg, **kw))

    a, twin_a = sac(0), sac(0)
    # the other kinds' creates keep refusing SAC handles
    for fn in (lib.fql_group_create, lib.fql_ifql_group_create, lib.fql_rebrac_group_create, lib.fql_iqld_group_create, lib.fql_iql_group_create,
               lib.fql_cfgrl_group_create):
        rc, g = create([a, twin_a], fn=fn)
        assert rc == _cabi.FQL_E_STATE and not g.value and b'SAC' in lib.fql_last_error(None), lib.fql_last_error(None)
    # and the SAC create another kind's
    icfg = fql_amd.iql.get_config()
    icfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    q0, q1 = fql_amd.IQLAgent.create(0, ex_o, ex_a, icfg), fql_amd.IQLAgent.create(1, ex_o, ex_a, icfg)
    rc, g = create([a, q0])
    assert rc == _cabi.FQL_E_STATE and not g.value and b'IQL' in lib.fql_last_error(None) and b'SAC groups take SAC agents only' in lib.fql_last_error(None)
    plain, backup, mean_q, slow, wide, other_b = (sac(1, tanh_squash=False), sac(2, backup_entropy=True), sac(3, q_agg='mean'), sac(4, lr=1e-4),
                                                  sac(5, actor_hidden_dims=(128,) * 4, value_hidden_dims=(128,) * 4), sac(6, batch_size=16))
    for bad in (plain, backup, mean_q, slow, wide, other_b):
        rc, g = create([a, bad])
        assert rc == _cabi.FQL_E_INVALID and not g.value, lib.fql_last_error(None)
        assert b'member 1' in lib.fql_last_error(None)
        if bad is other_b:
            assert b'batch size' in lib.fql_last_error(None)
        else:
            assert b'target_entropy' in lib.fql_last_error(None)
    assert create([a, a])[0] == _cabi.FQL_E_INVALID and b'twice' in lib.fql_last_error(None)
    # target_entropy given against automatic (NaN in fql_sac_config), another multiplier: one group
    b, twin_b = sac(5, target_entropy=-2.0, target_entropy_multiplier=0.25), sac(5, target_entropy=-2.0, target_entropy_multiplier=0.25)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID and b'already belongs' in lib.fql_last_error(None)
    assert lib.fql_set_batch_size(a._h, 16) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # every other kind's group calls on a SAC group name the SAC call
    o, out = np.zeros((2, 1, od), np.float32), np.zeros((2, 1, ad), np.float32)
    z, zn, seeds, v = np.zeros((2, 1, ad), np.float32), np.zeros((2, 1, 4, ad), np.float32), (C.c_uint64 * 2)(1, 2), C.c_int64(-1)
    w, la, gl = np.ones((2, 1), np.float32), (C.c_int64 * 4)(-1, -1, -1, -1), np.zeros((2, 1, 2), np.float32)
    UPD, SMP, STA = b'fql_sac_group_update_from_dataset', b'fql_sac_group_sample_actions', b'fql_sac_group_stats'
    for call, name in ((lambda: lib.fql_group_update_from_dataset(g, None, B, None, None), UPD),
                       (lambda: lib.fql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_group_sample_stats(g, 0, C.byref(v)), STA),
                       (lambda: lib.fql_rebrac_group_update_from_dataset(g, None, B, 1, None, None), UPD),
                       (lambda: lib.fql_rebrac_group_sample_actions(g, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_rebrac_group_stats(g, C.byref(v), None, None), STA),
                       (lambda: lib.fql_iqld_group_update_from_dataset(g, None, B, 1, 1, None, None), UPD),
                       (lambda: lib.fql_iqld_group_sample_actions(g, o.ctypes.data, 1, None, seeds, w.ctypes.data, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_iqld_group_stats(g, la, C.byref(v)), STA),
                       (lambda: lib.fql_ifql_group_update_from_dataset(g, None, B, None, None), UPD),
                       (lambda: lib.fql_ifql_group_sample_actions(g, o.ctypes.data, 1, zn.ctypes.data, seeds, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_ifql_group_flow_actions(g, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_ifql_group_stats(g, C.byref(v), None, None), STA),
                       (lambda: lib.fql_iql_group_update_from_dataset(g, None, B, None, None), UPD),
                       (lambda: lib.fql_iql_group_sample_actions(g, o.ctypes.data, 1, None, seeds, 1.0, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_iql_group_stats(g, C.byref(v), None), STA),
                       (lambda: lib.fql_cfgrl_group_update_from_dataset(g, None, B, None, None, None), UPD),
                       (lambda: lib.fql_cfgrl_group_sample_actions(g, o.ctypes.data, gl.ctypes.data, 1, None, seeds, w.ctypes.data, out.ctypes.data, None), SMP),
                       (lambda: lib.fql_cfgrl_group_stats(g, C.byref(v), None), STA)):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None) and b'SAC agents' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1 and list(la) == [-1] * 4 and not out.any()
    # and the SAC calls on an IQL group name the IQL call
    rc, qg = create([q0, q1], fn=lib.fql_iql_group_create)
    assert rc == _cabi.FQL_OK and qg.value
    for call, name in ((lambda: lib.fql_sac_group_update_from_dataset(qg, None, B, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_sac_group_update_balanced(qg, None, None, B, None, None), b'fql_iql_group_update_from_dataset'),
                       (lambda: lib.fql_sac_group_sample_actions(qg, o.ctypes.data, 1, z.ctypes.data, seeds, 1.0, out.ctypes.data, None), b'fql_iql_group_sample_actions'),
                       (lambda: lib.fql_sac_group_stats(qg, C.byref(v), None), b'fql_iql_group_stats')):
        assert call() == _cabi.FQL_E_STATE and name in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1
    assert lib.fql_group_destroy(qg) == _cabi.FQL_OK
    assert lib.fql_sac_group_update_from_dataset(g, None, 16, None, None) == _cabi.FQL_E_INVALID   # wrong batch size
    assert b'batch_size' in lib.fql_last_error(None)
    assert lib.fql_sac_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_E_INVALID    # no dataset uploaded
    assert lib.fql_sac_group_sample_actions(g, o.ctypes.data, 1, None, None, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID   # neither noises nor seeds
    assert lib.fql_sac_group_sample_actions(g, o.ctypes.data, 0, None, seeds, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert lib.fql_sac_group_sample_actions(g, o.ctypes.data, 1, None, seeds, -1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    # FQLAgentGroup still refuses a SAC config
    with pytest.raises(NotImplementedError, match='SAC'):
        fql_amd.FQLAgentGroup.create([0, 1], ex_o, ex_a, cfg)
    # released: plain handles again, bitwise with their twins through grouped and standalone steps, and groupable again
    for x in (a, b, twin_a, twin_b):
        x.upload_dataset(ds)
    for _ in range(2):
        assert lib.fql_sac_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B)
    assert lib.fql_group_synchronize(g) == _cabi.FQL_OK
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 16) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    for _ in range(2):
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B)
    _assert_same_state(a, twin_a, 'released member 0')
    _assert_same_state(b, twin_b, 'released member 1')
    rc, g = create([b, a])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert lib.fql_sac_group_update_from_dataset(g, None, B, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
    for x in (twin_a, twin_b):
        x.update_from_dataset(B)
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    _assert_same_state(a, twin_a, 'regrouped member 0')
    _assert_same_state(b, twin_b, 'regrouped member 1')
    for x in (a, b, twin_a, twin_b, plain, backup, mean_q, slow, wide, other_b, q0, q1):
        x.close()


def test_sac_group_close_releases_the_members_and_is_idempotent():
    """After close() the members update alone, bitwise with twins that were never grouped; a second close() is a no-op."""
    K, B = 2, 32
    cfg, ds, group, twins = _setup(K, B, H64x2)
    group.update_from_dataset()
    for t in twins:
        t.update_from_dataset(B)
    group.close()
    group.close()
    assert group._g is None
    for m, t in zip(group.members, twins):
        m.update_from_dataset(B)
        t.update_from_dataset(B)
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'closed member {i}')
