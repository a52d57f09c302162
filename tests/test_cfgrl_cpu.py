"""CPU tests of the CFGRL agent's restatements (tests/cfgrl_oracle.py, tests/cfgrl_oracle_torch.py), of the goal rule driven by given draws,
and of the host-side CFGRLAgent surface."""
import numpy as np
import pytest

import cfgrl_oracle as CO
import cfgrl_oracle_torch as CT
import fql_amd
from fql_amd import cfgrl as cmod
from oracle import fql_oracle as O

OD, AD, GD, B = 7, 3, 5, 12
EMB = 'modules_unc_embed/Embed_0/embedding'
MIXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.2, 0.5, 0.3))   # cur / traj / random


def _masks():
    ends = np.zeros(B, bool)
    ends[0] = ends[B - 1] = True
    return {'none': np.zeros(B, bool), 'all': np.ones(B, bool), 'ends': ends}


def _problem(ln=False, hidden=(16, 16), seed=0):
    cfg = CO.get_config()
    cfg.update(actor_hidden_dims=hidden, actor_layer_norm=ln, batch_size=B, flow_steps=4)
    params = CO.init_params(seed, OD, AD, GD, cfg, np.float64)
    rng = np.random.default_rng(seed + 1)
    for _, v in O.tree_leaves_with_path(params):
        v += 0.1 * rng.standard_normal(v.shape)
    batch = {'observations': rng.standard_normal((B, OD)), 'actions': np.clip(rng.standard_normal((B, AD)), -1, 1),
             'actor_goals': rng.standard_normal((B, GD))}
    return cfg, params, batch, CO.make_noise(B, AD, seed + 2)


@pytest.mark.parametrize('ln', [False, True])
@pytest.mark.parametrize('kind', ['none', 'all', 'ends'])
def test_numpy_equals_torch(ln, kind):
    """The hand-derived backward (dU = the goal columns of the input gradient, summed over the dropped rows) against autograd through the
    reference's where(): 1e-9."""
    cfg, params, batch, noise = _problem(ln)
    mask = _masks()[kind]
    a, b = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64), CT.TorchCFGRL(params, cfg)
    la, _, ga = a.grads(batch, noise, mask)
    lb, gb = b.grads(batch, noise, mask)
    assert abs(la - lb) <= 1e-12 * max(1.0, abs(la))
    gb = CT.leaves(gb)
    for p, v in O.tree_leaves_with_path(ga):
        np.testing.assert_allclose(v, gb[p], rtol=1e-9, atol=1e-13, err_msg=p)
    dU = dict(O.tree_leaves_with_path(ga))[EMB]
    assert dU.shape == (1, GD) and (not dU.any() if kind == 'none' else dU.all())
    sn = np.random.default_rng(9).standard_normal((5, AD))
    for c in (0.0, 3.0):
        np.testing.assert_allclose(a.sample_actions(batch['observations'][:5], batch['actor_goals'][:5], sn, c),
                                   b.sample_actions(batch['observations'][:5], batch['actor_goals'][:5], sn, c), atol=1e-12)
    a.update(batch, noise, mask)
    b.update(batch, noise, mask)
    pb = CT.leaves(b.params)
    for p, v in O.tree_leaves_with_path(a.params):
        np.testing.assert_allclose(v, pb[p], rtol=1e-9, atol=1e-13, err_msg=p)


@pytest.mark.parametrize('kind', ['none', 'all', 'ends'])
def test_finite_differences_on_every_leaf(kind):
    """Central differences on three entries of every actor_flow leaf and on EVERY element of unc_embed."""
    cfg, params, batch, noise = _problem(True, hidden=(6, 5))
    mask = _masks()[kind]
    ref = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64)
    _, _, g = ref.grads(batch, noise, mask)
    rng = np.random.default_rng(4)
    gl = dict(O.tree_leaves_with_path(g))
    for p, v in O.tree_leaves_with_path(ref.params):
        where = list(np.ndindex(*v.shape)) if p == EMB else [tuple(rng.integers(0, s) for s in v.shape) for _ in range(3)]
        assert p != EMB or len(where) == GD
        for i in where:
            old, h = v[i], 1e-6
            v[i] = old + h
            lp = ref.policy_loss(batch, noise, mask)[0]
            v[i] = old - h
            lm = ref.policy_loss(batch, noise, mask)[0]
            v[i] = old
            fd = (lp - lm) / (2 * h)
            assert abs(fd - gl[p][i]) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (p, i, fd, gl[p][i])


def test_loss_of_an_all_zero_network_and_info_keys():
    cfg, params, batch, noise = _problem()
    zero = O.tree_map(np.zeros_like, params)
    ref = CO.OracleCFGRL(zero, cfg, OD, AD, GD, np.float64)
    vel = batch['actions'] - noise['x0']
    assert abs(ref.policy_loss(batch, noise, _masks()['ends'])[0] - np.mean(vel * vel)) <= 1e-14
    _, info = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64).update(batch, noise, _masks()['ends'])
    assert tuple(info) == ('actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm') == fql_amd.CFGRL_INFO_KEYS == CO.INFO_KEYS


def test_cfg_zero_ignores_the_goal_and_cfg_one_ignores_unc_embed():
    cfg, params, batch, _ = _problem()
    ref = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64)
    obs, g, sn = batch['observations'][:4], batch['actor_goals'][:4], np.random.default_rng(2).standard_normal((4, AD))
    np.testing.assert_array_equal(ref.sample_actions(obs, g, sn, 0.0), ref.sample_actions(obs, g[::-1], sn, 0.0))
    other = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64)
    other.params['modules_unc_embed']['Embed_0']['embedding'] += 1.0
    np.testing.assert_allclose(ref.sample_actions(obs, g, sn, 1.0), other.sample_actions(obs, g, sn, 1.0), atol=1e-12)
    assert ref.sample_actions(obs[0], g[0], sn[0]).shape == (AD,) and ref.sample_actions(obs[:1], g[:1], sn[:1]).shape == (AD,)
    np.testing.assert_array_equal(ref.sample_actions(obs, g[0], sn), ref.sample_actions(obs, np.tile(g[:1], (4, 1)), sn))


# ---- GCDataset.sample_goals from given draws -----------------------------------------------------------------------------------------
def _draws(n, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32) for k in ('random', 'dist', 'traj', 'cur')}


def test_goals_stay_in_their_trajectory():
    ds = CO.make_gc_dataset(OD, AD, seed=1)
    N = len(ds['terminals'])
    assert N == 224 and list(np.nonzero(ds['terminals'])[0]) == [0, 2, 5, 22, 222, 223]
    final = CO.final_indices(ds['terminals'])
    np.testing.assert_array_equal(final, cmod.final_indices(ds['terminals']))
    assert final[0] == 0 and final[1] == final[2] == 2 and final[6] == 22 and final[23] == 222 and final[223] == 223
    idx = np.tile(np.arange(N), 40)
    d = _draws(len(idx), 2)
    d['dist'][:N] = 0                     # d = 0: the far end, final
    d['dist'][N:2 * N] = 2 ** 32 - 1      # d just below 1: the near end
    g = CO.sample_goals(idx, ds['terminals'], d, 0.0, 1.0, 0.0)
    lo = np.minimum(idx + 1, final[idx])
    assert (g >= lo).all() and (g <= final[idx]).all()          # [min(idx + 1, final), final] of the row's own trajectory
    np.testing.assert_array_equal(g[:N], final)
    np.testing.assert_array_equal(g[N:2 * N], lo[:N])
    last = idx == final[idx]                                    # a length-1 trajectory and each trajectory's last row: goal = idx
    assert last.sum() == 6 * 40 and (g[last] == idx[last]).all()
    inside = g[idx == 23]                                       # the first row of the 200-row trajectory reaches both ends
    assert inside.min() == 24 and inside.max() == 222


def test_round_is_half_to_even_in_fp64():
    """idx 23 of the 200-row trajectory: min(idx + 1, final) = 24, final = 222; d = 0.75 gives 24 * 0.75 + 222 * 0.25 = 73.5 -> 74 and
    d = 0.25 gives 172.5 -> 172: np.round's half to even, which the device's rint restates."""
    ds = CO.make_gc_dataset(OD, AD, seed=1)
    d = {k: np.zeros(2, np.uint32) for k in ('random', 'dist', 'traj', 'cur')}
    d['dist'][:] = [3 << 30, 1 << 30]
    np.testing.assert_array_equal(CO.sample_goals(np.array([23, 23]), ds['terminals'], d, 0.0, 1.0, 0.0), [74, 172])


@pytest.mark.parametrize('mix', MIXES)
def test_probability_mixes_select_as_the_reference_does(mix):
    ds = CO.make_gc_dataset(OD, AD, seed=1)
    N = len(ds['terminals'])
    idx = np.random.default_rng(3).integers(0, N, size=4000)
    d = _draws(4000, 4)
    g = CO.sample_goals(idx, ds['terminals'], d, *mix)
    pc, pt, _ = mix
    if pc == 1.0:
        np.testing.assert_array_equal(g, idx)
        return
    u, uc = d['traj'] / 2.0 ** 32, d['cur'] / 2.0 ** 32
    traj = CO.sample_goals(idx, ds['terminals'], d, 0.0, 1.0, 0.0)
    rand = (d['random'].astype(np.uint64) * np.uint64(N) >> np.uint64(32)).astype(np.int64)
    np.testing.assert_array_equal(g, np.where(uc < pc, idx, np.where(u < pt / (1.0 - pc), traj, rand)))
    if mix == (0.2, 0.5, 0.3):
        cur, tr = uc < pc, (uc >= pc) & (u < 0.625)
        assert abs(cur.mean() - 0.2) < 0.04 and abs(tr.mean() - 0.5) < 0.04 and (g[cur] == idx[cur]).all()


# ---- the sampler in fp32 -------------------------------------------------------------------------------------------------------------
def test_fp32_rounding_of_the_sampler_at_hidden_512():
    """The inputs of tests/test_gpu_cfgrl.py::test_sample_actions_at_hidden_512 (obs 69, G 69, act 21, hidden 512 x 4, n = 1, 37, 2049,
    cfg 0 and 3), from that module's own builders: fp32 numpy stays within 5e-6 of fp64 at the head scale the GPU test uses, a quarter of
    the 2e-5 the GPU test allows, and at least 20 % of the coordinates end on the clip at n > 1.  Measured at head scale 2.0: worst
    |fp32 - fp64| 7.8e-7 (cfg 3, n 2049) and 4.6e-7 (cfg 0); share on the clip 33 % at cfg 0 and 37 % at cfg 3 (n 2049).  Scales 1.0 and
    3.0 give 4.8e-7 and 1.2e-6 at n 513 / cfg 3: the error grows with the head's gain and stays far inside the bound, so the scale is
    BC's 2.0, at which the velocities are O(2) and a third of the coordinates leave [-1, 1]."""
    from tests import test_gpu_cfgrl as G
    S = G.SAMPLER512
    cfg, params = G.sampler512_problem()
    assert (S['od'], S['gd'], S['ad'], tuple(cfg['actor_hidden_dims']), S['ns'], S['cfgs']) == (69, 69, 21, (512,) * 4, (1, 37, 2049), (0.0, 3.0))
    r64 = CO.OracleCFGRL(params, cfg, S['od'], S['ad'], S['gd'], np.float64)
    r32 = CO.OracleCFGRL(params, cfg, S['od'], S['ad'], S['gd'], np.float32)
    worst, share = {}, {}
    for n in S['ns']:
        obs, goals, sn = G.sampler512_inputs(n)
        for c in S['cfgs']:
            a64, a32 = r64.sample_actions(obs, goals, sn, c), r32.sample_actions(obs, goals, sn, c)
            assert a32.dtype == np.float32
            worst[n, c] = float(np.abs(a32.astype(np.float64) - a64).max())
            share[n, c] = float((np.abs(a64) == 1).mean())
            if n > 1:
                assert share[n, c] >= 0.2, (n, c, share[n, c])
    print(S['scale'], worst, share)
    assert max(worst.values()) <= 5e-6, worst


def test_registry_config_and_host_refusals():
    assert fql_amd.agents['cfgrl'] is fql_amd.CFGRLAgent
    assert set(fql_amd.agents) == {'fql', 'ifql', 'rebrac', 'sac', 'bc', 'iql', 'iql_diffusion', 'cfgrl'}   # agents/__init__.py:10-19
    cfg = cmod.get_config()
    want = dict(agent_name='cfgrl', lr=3e-4, batch_size=1024, actor_hidden_dims=(512, 512, 512, 512), actor_layer_norm=False, discount=0.99,
                flow_steps=16, cfg=3.0, encoder=None, action_dim=None, dataset_class='GCDataset', value_p_curgoal=0.0, value_p_trajgoal=1.0,
                value_p_randomgoal=0.0, value_geom_sample=False, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
                actor_geom_sample=False, gc_negative=True, p_aug=0.0, frame_stack=None, rng='engine', precision='fp32')
    assert dict(cfg) == want
    ex = {'observations': np.zeros((1, OD), np.float32), 'actions': np.zeros((1, AD), np.float32), 'value_goals': np.zeros((1, GD), np.float32)}
    for bad in (dict(encoder='impala_small'), dict(precision='bf16x3'), dict(rng='jax'), dict(actor_geom_sample=True), dict(frame_stack=3)):
        with pytest.raises(NotImplementedError):
            fql_amd.CFGRLAgent.create(0, ex, bad)
    with pytest.raises(ValueError):
        fql_amd.CFGRLAgent.create(0, ex, dict(actor_p_curgoal=0.5))
    with pytest.raises(KeyError):
        fql_amd.CFGRLAgent.create(0, {k: ex[k] for k in ('observations', 'actions')}, {})
    with pytest.raises(AssertionError):
        cmod.final_indices(np.array([0, 1, 0], np.float32))


def test_create_without_a_gpu_fails_loudly():
    """No CPU fallback: without a HIP device CFGRLAgent.create raises (FQL_E_NODEVICE), as FQLAgent.create does; with one it succeeds."""
    import torch
    ex = {'observations': np.zeros((1, OD), np.float32), 'actions': np.zeros((1, AD), np.float32), 'value_goals': np.zeros((1, GD), np.float32)}
    args = (0, ex, dict(actor_hidden_dims=(64, 64), batch_size=16))
    if torch.cuda.is_available():
        fql_amd.CFGRLAgent.create(*args).close()
        return
    with pytest.raises(RuntimeError, match='no HIP device'):
        fql_amd.CFGRLAgent.create(*args)
