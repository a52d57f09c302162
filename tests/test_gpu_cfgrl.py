"""GPU: the CFGRL agent (agents/cfgrl.py) on the engine against the fp64 restatement in tests/cfgrl_oracle.py.  Tolerances are the module
bounds of tests/test_gpu_bc.py, applied to the unc_embed leaf exactly as to any other leaf: infos rtol 5e-5 / atol 5e-6, per-leaf
gradients (Adam mu / 0.1) within 2e-5 max|g| + 1e-9, post-step parameters as _check_first_update does, sampled actions atol 2e-5.

test_paths_match_fp64_restatement runs the first-update comparison at hidden 512 x 4 unless noted, after asserting from the engine's plan
(fql_debug_plan; [M, N, K] of a GEMM task, rows per tile) the launches the case is named for:
  humanoidmaze (obs 69, G 69, act 21, B 256, with and without LayerNorm): layer 0 [256, 512, 192] (69 + 69 + 21 + 1 = 160 before
      padding), head [256, 32, 512] and its dgrad [256, 512, 32] on the 16-row kernel; the goal block [69, 138) crosses a 64-lane stride
      of the prep kernel
  act16 (obs 29, G 29, act 16): head [256, 16, 512], dgrad [256, 512, 16], no task 32 wide
  reps2 (obs 29, G 2, act 8): a goal block narrower than anything else in the row; dU with two columns
  b1024 (obs 40, G 40, act 4): every 512 x 512 task on fql_side_big_kernel's 64-row tiles at M 1024
  b272 (obs 29, G 29, act 8): every task at M 272 on fql_gemm16_kernel<false>; rows 256..271 are a second chunk of 16 in the column sum
  wide1024 (1024 x 2, B 48): every K 1024 task on fql_gemm16_kernel<true>; fql_cfgrl_embed_grad_kernel sums four columns per thread (H = 1024)
  ragged (hidden (128, 64, 96), B 32): padded widths that differ layer to layer
No plan holds an OP_DGRAD0 launch or a dgrad with N = in_p: the embedding gradient is formed from dZ0, not from an input gradient."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import cfgrl_oracle as CO
from tests.util import (K_GEMM16, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, OP_GEMM, OP_GEMM64, assert_info_close, leaf_dict, read_plan,
                        sync_restatement)

pytestmark = pytest.mark.gpu
OD, AD, GD = 29, 8, 29
OP_DGRAD0 = 24   # enum OpType (fql_amd/csrc/fql_engine.hip): the lean 16-column first-layer input gradient
EMB = 'modules_unc_embed/Embed_0/embedding'
MIXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.2, 0.5, 0.3))   # actor_p_curgoal, actor_p_trajgoal, actor_p_randomgoal
THR_MASK = int(0.1 * 2 ** 32)                                  # do_cfg = u32 < floor(p_uncond 2^32)


def _cfg(H=64, B=64, nh=4, **kw):
    import fql_amd.cfgrl
    cfg = fql_amd.cfgrl.get_config()
    cfg.update(actor_hidden_dims=(H,) * nh, batch_size=B)
    cfg.update(kw)
    return cfg


def _mask(B, seed, kind='some'):
    if kind == 'none':
        return np.zeros(B, bool)
    if kind == 'all':
        return np.ones(B, bool)
    if kind == 'ends':
        m = np.zeros(B, bool)
        m[0] = m[B - 1] = True
        return m
    m = np.random.default_rng(seed).random(B) < 0.25
    m[0], m[1] = True, False
    return m


def _data(od, ad, gd, B, seed, kind='some'):
    rng = np.random.default_rng(seed)
    batch = {'observations': rng.standard_normal((B, od)).astype(np.float32),
             'actions': np.clip(rng.standard_normal((B, ad)), -1, 1).astype(np.float32),
             'actor_goals': rng.standard_normal((B, gd)).astype(np.float32)}
    return batch, CO.make_noise(B, ad, seed + 100), _mask(B, seed + 200, kind)


def _randomized(params, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, np.float32), params)
    for p, v in O.tree_leaves_with_path(out):
        if not p.endswith('/kernel'):
            v += (scale * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def _example(od, ad, gd):
    return {'observations': np.zeros((1, od), np.float32), 'actions': np.zeros((1, ad), np.float32), 'value_goals': np.zeros((1, gd), np.float32)}


def _agent(cfg, od=OD, ad=AD, gd=GD, seed=3, params=None):
    import fql_amd
    a = fql_amd.CFGRLAgent.create(seed, _example(od, ad, gd), cfg)
    if params is not None:
        a.set_params(params)
    return a


def _same_state(a, b):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step'])
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{part} {k}')


def _check_first_update(a, cfg, od, ad, gd, batch, noise, mask, seed=5):
    params = _randomized(a.get_params(), seed)
    a.set_params(params)
    ref = CO.OracleCFGRL(params, dict(cfg), od, ad, gd, np.float64)
    _, _, g_ref = ref.grads(batch, noise, mask)
    _, info = a.update(batch, noise=noise, do_cfg=mask)
    info = info.to_dict()
    assert tuple(info) == CO.INFO_KEYS
    _, want = ref.update(batch, noise, mask)
    print('infos', info, want)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=CO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    assert opt['count'] == 1 and opt['step'] == 2
    mu, new, new_ref = leaf_dict(opt['mu']), leaf_dict(a.get_params()), leaf_dict(ref.params)
    assert EMB in leaf_dict(g_ref)
    for p, g in leaf_dict(g_ref).items():
        tol = 2e-5 * np.abs(g).max() + 1e-9
        print('grad', p, float(np.abs(mu[p] / 0.1 - g).max()), tol)
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        d = np.abs(new[p] - new_ref[p])
        stable = np.abs(g) > 50 * tol
        assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p
    rows = a.read_rows()
    np.testing.assert_array_equal(rows['do_cfg'], mask)
    assert (rows['goal_idx'] == -1).all()
    want_goals = np.where(mask[:, None], params['modules_unc_embed']['Embed_0']['embedding'], batch['actor_goals'])
    np.testing.assert_array_equal(rows['goals'], want_goals)
    return params, mu


def test_leaf_names_shapes_and_init_statistics():
    import fql_amd
    assert fql_amd.agents['cfgrl'] is fql_amd.CFGRLAgent and len(fql_amd.agents) == 8
    cfg = _cfg(512, 64, actor_layer_norm=True)
    a = _agent(cfg)
    want = [(p, v.shape) for p, v in O.tree_leaves_with_path(CO.init_params(0, OD, AD, GD, cfg))]
    assert a.leaves() == want   # jax dict order: Dense_i, LayerNorm_i, then modules_unc_embed
    assert set(a.get_params()) == {'modules_actor_flow', 'modules_unc_embed'}
    p = leaf_dict(a.get_params())
    assert p['modules_actor_flow/mlp/Dense_0/kernel'].shape == (OD + GD + AD + 1, 512)
    assert p['modules_actor_flow/mlp/Dense_4/kernel'].shape == (512, AD) and p[EMB].shape == (1, GD)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.endswith('/kernel'):   # default_init on every Dense, the head included: Glorot uniform
            lim = np.sqrt(6.0 / (v.shape[0] + v.shape[1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
    a2 = _agent(_cfg(64, 64))
    assert not any('LayerNorm' in k for k, _ in a2.leaves())   # actor_layer_norm=False is the default


def test_unc_embed_init_variance_over_4096_draws():
    """N(0, 1 / G), untruncated: over 4096 draws the sample variance times G lies within 5 sqrt(2 / 4096) of 1 (five standard deviations of
    the variance estimate), and some draw lies beyond 2 sigma (a truncated_normal has none).  The issue asks for one handle at G = 4096;
    the engine's layer widths end at 1024 and layer 0 is obs + G + act + 1 wide, so that create is refused (asserted here) and the 4096
    draws come from 8 handles at G = 512, each drawn once, each row scaled by sqrt(512): the same statistic under the same bound."""
    with pytest.raises(ValueError, match='1024'):
        _agent(_cfg(64, 16, 2), 5, 2, 4096)
    G = 512
    v = np.concatenate([leaf_dict(_agent(_cfg(64, 16, 2), 5, 2, G, seed=100 + s).get_params())[EMB].ravel() for s in range(8)]) * np.sqrt(G)
    assert v.size == 4096
    print('var G', float(v.var()), 'mean', float(v.mean()), 'max', float(np.abs(v).max()))
    assert abs(v.var() - 1.0) < 5 * np.sqrt(2.0 / 4096) and abs(v.mean()) < 5 / np.sqrt(4096)
    assert (np.abs(v) > 2.0).any()


@pytest.mark.parametrize('H,B', [(64, 64), (512, 256)])
@pytest.mark.parametrize('ln', [True, False])
def test_one_update_matches_fp64_restatement(H, B, ln):
    cfg = _cfg(H, B, actor_layer_norm=ln)
    batch, noise, mask = _data(OD, AD, GD, B, seed=1)
    assert mask[0] and not mask[1] and noise['t'][0] == 0
    _check_first_update(_agent(cfg), cfg, OD, AD, GD, batch, noise, mask)


@pytest.mark.parametrize('kind', ['none', 'all', 'ends'])
def test_mask_extremes(kind):
    """No row dropped: dU is exactly zero (Adam's moments of the leaf stay 0 and the leaf does not move).  Every row dropped, and rows 0 and
    B - 1 only: against the restatement at the module bounds."""
    cfg = _cfg(64, 64)
    batch, noise, mask = _data(OD, AD, GD, 64, seed=2, kind=kind)
    a = _agent(cfg)
    params, mu = _check_first_update(a, cfg, OD, AD, GD, batch, noise, mask)
    if kind == 'none':
        opt = a.get_opt_state()
        assert not leaf_dict(opt['mu'])[EMB].any() and not leaf_dict(opt['nu'])[EMB].any()
        np.testing.assert_array_equal(leaf_dict(a.get_params())[EMB], params['modules_unc_embed']['Embed_0']['embedding'])
    else:
        assert mu[EMB].any()


def test_policy_loss_matches_and_changes_no_state():
    cfg = _cfg()
    batch, noise, mask = _data(OD, AD, GD, 64, seed=2)
    a = _agent(cfg)
    a.update(batch, noise=noise, do_cfg=mask)
    a.synchronize()
    before, info_before, opt_before, rows_before = leaf_dict(a.get_params()), a.read_info(), a.get_opt_state(), a.read_rows()
    b2, n2, m2 = _data(OD, AD, GD, 64, seed=12)
    loss, info = a.policy_loss(b2, noise=n2, do_cfg=m2)
    ref = CO.OracleCFGRL(a.get_params(), dict(cfg), OD, AD, GD, np.float64)
    want = ref.policy_loss(b2, n2, m2)[0]
    assert abs(loss - want) <= 5e-5 * abs(want) + 5e-6 and info == {'actor_loss': loss}
    a.synchronize()
    for k, v in leaf_dict(a.get_params()).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
    opt = a.get_opt_state()
    assert (opt['count'], opt['step']) == (opt_before['count'], opt_before['step']) == (1, 2)
    for part in ('mu', 'nu'):
        for k, v in leaf_dict(opt[part]).items():
            np.testing.assert_array_equal(v, leaf_dict(opt_before[part])[k])
    assert a.read_info() == info_before
    np.testing.assert_array_equal(a.read_rows()['do_cfg'], rows_before['do_cfg'])   # the probe writes its own half
    np.testing.assert_array_equal(a.read_rows(probe=True)['do_cfg'], m2)


# ---- hidden 512 at the shapes and batches that switch kernels: what the update program's plan holds --------------------------------
def _gemm(plan, kernels=None):
    return [dict(t, kernel=L['kernel'], type=L['type']) for L in plan if kernels is None or L['kernel'] in kernels for t in L['gemm']]


def _wgrad(plan):
    return {(t['M'], t['Kin'], t['N']) for L in plan for t in L['wgrad']}


def _has(tasks, M, N, K, **kw):
    return [t for t in tasks if (t['M'], t['N'], t['K']) == (M, N, K) and all(t[k] == v for k, v in kw.items())]


def _no_input_gradient(plan, in_p, H0=512):
    """No OP_DGRAD0 launch and no dgrad with N = in_p (a first-layer input gradient is [B, in_p, H0]; where in_p == H0 the one task of
    that shape is layer 0's forward)."""
    assert not [L for L in plan if L['type'] == OP_DGRAD0]
    assert len([t for t in _gemm(plan) if (t['N'], t['K']) == (in_p, H0)]) == (1 if in_p == H0 else 0)


def _p_humanoidmaze(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 192)
    assert _has(g, B, 512, 192)                                  # layer 0 at in_p 192 (69 + 69 + 21 + 1 = 160)
    assert _has(g, B, 32, 512, rows=16, kernel=K_GEMM16)         # the head at the padded action width 32
    assert _has(g, B, 512, 32)                                   # ... and its dgrad: K = 32
    assert {(B, 192, 512), (B, 512, 32)} <= _wgrad(plan)


def _p_act16(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 128)                                # 29 + 29 + 16 + 1 = 75
    assert _has(g, B, 16, 512, rows=16, kernel=K_GEMM16) and _has(g, B, 512, 16)   # act == padded width 16: no padding column
    assert not [t for t in g if t['N'] == 32 or t['K'] == 32] and (B, 512, 16) in _wgrad(plan)


def _p_reps2(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 64)                                 # 29 + 2 + 8 + 1 = 40
    assert _has(g, B, 512, 64) and (B, 64, 512) in _wgrad(plan)


def _p_b1024(plan, B):
    _no_input_gradient(plan, 128)                                # 40 + 40 + 4 + 1 = 85
    hid = [t for t in _gemm(plan) if (t['N'], t['K']) == (512, 512)]
    assert hid and all(t['M'] == B and t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in hid)   # fql_side_big_kernel's 64-row tiles
    assert (B, 512, 512) in _wgrad(plan)


def _p_b272(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 128)
    assert g and all(t['M'] == B and t['rows'] == 16 and t['kernel'] == K_GEMM16 and t['type'] == OP_GEMM for t in g)   # M % 64 != 0
    assert _has(g, B, 512, 512) and (B, 512, 512) in _wgrad(plan)


def _p_wide1024(plan, B):
    _no_input_gradient(plan, 128, 1024)
    kbig = [t for t in _gemm(plan) if t['K'] > 512]
    assert kbig and all(t['kernel'] == K_GEMM16_KBIG and t['rows'] == 16 for t in kbig)
    assert _has(kbig, B, 1024, 1024) and _has(kbig, B, 16, 1024) and (B, 1024, 1024) in _wgrad(plan)


def _p_ragged(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 128, 128)
    assert _has(g, B, 128, 128) and _has(g, B, 64, 128) and _has(g, B, 96, 64) and _has(g, B, 16, 96)
    assert {(B, 128, 128), (B, 128, 64), (B, 64, 96), (B, 96, 16)} <= _wgrad(plan)


def _p_w50_padded(plan, B):
    g = _gemm(plan)
    _no_input_gradient(plan, 128, 64)                            # 29 + 29 + 8 + 1 = 67
    assert g and all(t['M'] == B and t['rows'] == 16 and t['kernel'] == K_GEMM16 and t['type'] == OP_GEMM for t in g)
    assert _has(g, B, 64, 64) and (B, 64, 64) in _wgrad(plan) and B in {m for L in plan for m in L['ln']}   # out 50 of out_p 64


H512_CASES = {   # id -> (od, gd, ad, hidden, B, actor_layer_norm, plan assertion)
    'humanoidmaze': (69, 69, 21, (512,) * 4, 256, True, _p_humanoidmaze),
    'humanoidmaze-no-ln': (69, 69, 21, (512,) * 4, 256, False, _p_humanoidmaze),
    'act16': (29, 29, 16, (512,) * 4, 256, False, _p_act16),
    'reps2': (29, 2, 8, (512,) * 4, 256, False, _p_reps2),
    'b1024': (40, 40, 4, (512,) * 4, 1024, False, _p_b1024),
    'b272': (29, 29, 8, (512,) * 4, 272, False, _p_b272),
    'wide1024': (29, 29, 8, (1024,) * 2, 48, False, _p_wide1024),
    'ragged': (29, 29, 8, (128, 64, 96), 32, True, _p_ragged),
    'w50-padded': (29, 29, 8, (50, 50, 50), 32, True, _p_w50_padded),   # hidden widths that are no multiple of 16: LayerNorm over 50 of 64 columns
}


@pytest.mark.parametrize('cid', list(H512_CASES))
def test_paths_match_fp64_restatement(cid):
    """Each case first asserts, from the engine's own plan (fql_debug_plan), the path its id names, then runs _check_first_update at its
    bounds.  The mask of b272 drops rows in the last 16 (the tail of the column sum)."""
    od, gd, ad, hidden, B, ln, check = H512_CASES[cid]
    cfg = _cfg(B=B, actor_hidden_dims=hidden, actor_layer_norm=ln)
    batch, noise, mask = _data(od, ad, gd, B, seed=40 + od + ad)
    mask[B - 1] = mask[B - 16] = True
    a = _agent(cfg, od, ad, gd)
    plan = read_plan(a)
    print(cid, 'gemm (kernel, type, M, N, K, rows):', sorted({(t['kernel'], t['type'], t['M'], t['N'], t['K'], t['rows']) for t in _gemm(plan)}))
    print(cid, 'wgrad (M, Kin, N):', sorted(_wgrad(plan)), 'ln M:', sorted({m for L in plan for m in L['ln']}),
          'other launch types:', sorted({L['type'] for L in plan if L['type'] not in (OP_GEMM, OP_GEMM64)}))
    check(plan, B)
    _check_first_update(a, cfg, od, ad, gd, batch, noise, mask)
    check(read_plan(a), B)   # reading the plan changed no launch


def _check_step(a, ref, cfg, batch, noise, mask):
    """One more update, moments carried from earlier steps, from the engine's own pre-step state: the 4 infos at the first step's bounds,
    every leaf's gradient as (mu - 0.9 mu0) / 0.1 (tests/test_gpu_bc.py::_check_step's bounds), nu and the parameter step."""
    sync_restatement(ref, a)
    _, _, g_ref = ref.grads(batch, noise, mask)
    mu0, pre = leaf_dict(a.get_opt_state()['mu']), leaf_dict(a.get_params())
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, noise=noise, do_cfg=mask)
    info = info.to_dict()
    _, want = ref.update(batch, noise, mask)
    print('infos', info, want)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=CO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for p, g in leaf_dict(g_ref).items():
        tol = 2e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9
        np.testing.assert_allclose((mu[p] - np.float32(0.9) * mu0[p]) / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
        d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))
        stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
        assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p


def test_batch_size_walk_at_hidden_512():
    """B = 256, 1024, 272, 256 on one hidden-512 handle: 32-row tiles, fql_side_big_kernel's 64-row tiles, the 16-row kernel, and back.
    The rebuilt plan holds the new row count only; every step is compared from the engine's own pre-step state."""
    cfg = _cfg(512, 256)
    a = _agent(cfg)
    params = _randomized(a.get_params(), 16)
    a.set_params(params)
    ref = CO.OracleCFGRL(params, dict(cfg), OD, AD, GD, np.float64)
    tiles = {256: (32, K_SIDE), 1024: (64, K_SIDE_BIG), 272: (16, K_GEMM16)}
    for i, B in enumerate((256, 1024, 272, 256)):
        batch, noise, mask = _data(OD, AD, GD, B, seed=50 + i)
        assert a.get_opt_state()['count'] == i
        _check_step(a, ref, cfg, batch, noise, mask)
        plan = read_plan(a)
        assert {t['M'] for t in _gemm(plan)} == {B} == {M for M, _, _ in _wgrad(plan)}
        hid = _has(_gemm(plan), B, 512, 512)
        assert hid and {(t['rows'], t['kernel']) for t in hid} == {tiles[B]}
    assert a.get_opt_state()['count'] == 4


# ---- the goal draw on the device -----------------------------------------------------------------------------------------------------
def _gc_agent(mix, reps, B=256, seed=3):
    ds = CO.make_gc_dataset(OD, AD, seed=70, reps_dim=2 if reps else None)
    cfg = _cfg(64, B, actor_p_curgoal=mix[0], actor_p_trajgoal=mix[1], actor_p_randomgoal=mix[2])
    a = _agent(cfg, OD, AD, 2 if reps else OD, seed=seed)
    a.upload_dataset(ds)
    return a, ds, (ds['oracle_reps'] if reps else ds['observations'])


@pytest.mark.parametrize('reps', [False, True])
@pytest.mark.parametrize('mix', MIXES)
def test_goal_draw_equals_host_restatement_for_every_row(mix, reps):
    """8 update_from_dataset steps at B 256 on the six-trajectory dataset (lengths 1, 2, 3, 17, 200, 1).  From the raw draws read_rows()
    returns, tests/cfgrl_oracle.py::sample_goals gives the same goal index for EVERY row, the index draw and the mask are the stated
    functions of their draws, and the goal columns of the assembled rows are reps[goal_idx], or the pre-step unc_embed row where do_cfg,
    bitwise."""
    a, ds, table = _gc_agent(mix, reps)
    N = len(ds['terminals'])
    assert N == sum(CO.TRAJ_LENGTHS)
    seen = set()
    for _ in range(8):
        unc = leaf_dict(a.get_params())[EMB]
        a.update_from_dataset()
        r = a.read_rows()
        d = r['draws']
        idx = ((d['idx'].astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
        np.testing.assert_array_equal(r['idx'], idx)
        want = CO.sample_goals(idx, ds['terminals'], d, *mix)
        np.testing.assert_array_equal(r['goal_idx'], want)
        np.testing.assert_array_equal(r['do_cfg'], d['mask'] < THR_MASK)
        np.testing.assert_array_equal(r['goals'], np.where(r['do_cfg'][:, None], unc, table[r['goal_idx']]))
        seen |= set(zip(idx.tolist(), r['goal_idx'].tolist()))
    final = CO.final_indices(ds['terminals'])
    if mix == (0.0, 1.0, 0.0):   # every goal lies in [min(idx + 1, final), final] of its own trajectory
        assert all(min(i + 1, final[i]) <= g <= final[i] for i, g in seen)
        assert len({g for i, g in seen if final[i] - i > 100}) > 20
    if mix == (1.0, 0.0, 0.0):
        assert all(i == g for i, g in seen)
    if mix == (0.2, 0.5, 0.3):   # all three sources occur
        assert any(g == i and i < final[i] for i, g in seen) and any(g < i or g > final[i] for i, g in seen)
    assert a.get_opt_state()['count'] == 8


def test_drop_count_over_64_steps():
    """16,384 draws at p = 0.1: the count lies within 1638 +- 192 (five standard deviations of 38.4)."""
    a, _, _ = _gc_agent(MIXES[1], False)
    count = 0
    for _ in range(64):
        a.update_from_dataset()
        count += int(a.read_rows()['do_cfg'].sum())
    print('dropped', count)
    assert abs(count - 1638) <= 192


def test_goal_draw_refusals():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    with pytest.raises(NotImplementedError, match='actor_geom_sample'):
        _agent(_cfg(actor_geom_sample=True))
    c = _cabi.FqlConfig(); lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim, c.batch_size = OD, AD, 64
    gc = _cabi.FqlCfgrlConfig(); lib.fql_cfgrl_default_config(C.byref(gc))
    assert (gc.flow_steps, gc.cfg, gc.p_uncond, gc.actor_p_curgoal, gc.actor_p_trajgoal, gc.actor_p_randomgoal) == (16, 3.0, 0.1, 0.0, 1.0, 0.0)
    gc.goal_dim, gc.actor_geom_sample = GD, 1
    out = C.c_void_p()
    assert lib.fql_cfgrl_create(C.byref(c), C.byref(gc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    assert b'actor_geom_sample' in lib.fql_last_error(None)
    gc.actor_geom_sample = 0
    for field in ('encoder', 'precision'):
        c2 = _cabi.FqlConfig.from_buffer_copy(c)
        setattr(c2, field, 2 if field == 'precision' else 1)
        assert lib.fql_cfgrl_create(C.byref(c2), C.byref(gc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    a = _agent(_cfg())
    with pytest.raises(ValueError, match='goal table'):
        a.update_from_dataset()            # before upload_dataset
    assert a.get_opt_state()['count'] == 0
    ds = CO.make_gc_dataset(OD, AD, seed=71)
    bad = dict(ds, terminals=np.zeros_like(ds['terminals']))
    with pytest.raises(AssertionError):
        a.upload_dataset(bad)              # the last row must be terminal (utils/datasets.py:153)
    b = _agent(_cfg(), OD, AD, 2)
    with pytest.raises(ValueError, match='goal_dim'):
        b.upload_dataset(ds)               # G != obs_dim needs oracle_reps
    with pytest.raises(ValueError):
        a.sample_actions(np.zeros(OD, np.float32))   # goals=None
    # admission: the table refuses the other kinds' calls on this handle and this kind's calls on another
    h, E = a._h, _cabi.FQL_E_STATE
    f = lambda arr: arr.ctypes.data_as(C.c_void_p)   # noqa: E731
    ob, ac, r = np.zeros((64, OD), np.float32), np.zeros((64, AD), np.float32), np.zeros(64, np.float32)
    buf = (C.c_float * 16)()
    assert lib.fql_num_info(h) == 4 and [lib.fql_handle_info_name(h, i).decode() for i in range(4)] == list(CO.INFO_KEYS)
    assert lib.fql_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None) == E
    assert lib.fql_update_from_dataset(h, None, 64, 0, 0, None, None, None) == E and b'CFGRL handle' in lib.fql_last_error(h)
    assert lib.fql_sample_actions(h, f(ob), 1, None, 0, buf, None) == E
    assert lib.fql_bc_update(h, f(ob), f(ac), 64, None, None, None) == E
    assert lib.fql_replay_create(h, 128) == E and lib.fql_read_info(h, buf) == E
    assert lib.fql_update_begin(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None) == E
    grp = C.c_void_p()
    assert lib.fql_group_create((C.c_void_p * 1)(h), 1, C.byref(grp)) == E
    bc = fql_amd.BCAgent.create(1, ob[:1], ac[:1], dict(hidden_dims=(64, 64), batch_size=64))
    assert lib.fql_cfgrl_update(bc._h, f(ob), f(ac), f(ob), 64, None, None, None, None) == E
    assert lib.fql_cfgrl_dataset_goals(bc._h, None, None) == E
    la, ma, ls = a.cfgrl_stats()
    assert la > 0 and ma > 0 and ls == 3 + 16 * 6
    assert a.stats()['param_count'] == sum(int(np.prod(s)) for _, s in a.leaves())


def test_aql_and_graph_updates_bitwise_over_20_steps():
    """AQL packets on the engine's own queues against the captured graph on a caller's stream: torch's default stream (the legacy
    stream), which adds no stream to torch's pool for the rest of the process."""
    import torch
    from fql_amd import _cabi
    a, _, _ = _gc_agent(MIXES[2], False, B=64)
    b, _, _ = _gc_agent(MIXES[2], False, B=64)
    assert torch.cuda.current_stream().cuda_stream == 0
    for _ in range(20):
        a.update_from_dataset()
        b.update_from_dataset(stream=_cabi.FQL_STREAM_LEGACY)
    assert a.synchronize() == 'aql'
    torch.cuda.synchronize(); assert b.synchronize() == 'graph'
    _same_state(a, b)
    assert a.get_opt_state()['count'] == 20
    ra, rb = a.read_rows(), b.read_rows()
    np.testing.assert_array_equal(ra['goal_idx'], rb['goal_idx'])
    np.testing.assert_array_equal(ra['goals'], rb['goals'])


# ---- sampler ------------------------------------------------------------------------------------------------------------------------
SAMPLER512 = dict(od=69, gd=69, ad=21, hidden=(512,) * 4, scale=2.0, ns=(1, 37, 2049), cfgs=(0.0, 3.0))


def sampler512_problem(scale=SAMPLER512['scale']):
    """(cfg, params) of the sampler at the humanoidmaze shape, hidden 512, no LayerNorm (the default), biases and unc_embed randomized and
    the head kernel scaled by `scale`.  tests/test_cfgrl_cpu.py::test_fp32_rounding_of_the_sampler_at_hidden_512 chooses the scale: fp32
    numpy within 5e-6 of fp64 on these inputs at cfg 0 and 3."""
    S = SAMPLER512
    cfg = _cfg(actor_hidden_dims=S['hidden'], batch_size=256)
    params = _randomized(CO.init_params(8, S['od'], S['ad'], S['gd'], cfg), 8)
    params['modules_actor_flow']['mlp']['Dense_4']['kernel'] *= np.float32(scale)
    return cfg, params


def sampler512_inputs(n):
    rng = np.random.default_rng(n)
    S = SAMPLER512
    return (rng.standard_normal((n, S['od'])).astype(np.float32), rng.standard_normal((n, S['gd'])).astype(np.float32),
            rng.standard_normal((n, S['ad'])).astype(np.float32))


@pytest.fixture(scope='module')
def sampler512():
    cfg, params = sampler512_problem()
    S = SAMPLER512
    return _agent(cfg, S['od'], S['ad'], S['gd'], params=params), CO.OracleCFGRL(params, dict(cfg), S['od'], S['ad'], S['gd'], np.float64)


@pytest.mark.parametrize('n', SAMPLER512['ns'])
@pytest.mark.parametrize('cfg_scale', SAMPLER512['cfgs'])
def test_sample_actions_at_hidden_512(sampler512, n, cfg_scale):
    """n = 1, 37 and 2049 (one row past the 2048-observation chunk) against the restatement at 2e-5, cfg 0 (the unconditional half alone
    decides) and 3; the clip is reached; rows 0, n // 2 and n - 1 are bitwise the single-observation calls."""
    a, ref = sampler512
    ad = SAMPLER512['ad']
    obs, goals, sn = sampler512_inputs(n)
    got = a.sample_actions(obs, goals, noises=sn, cfg=cfg_scale, temperature=0.3)   # temperature: accepted and ignored
    want = ref.sample_actions(obs, goals, sn, cfg_scale)
    assert got.shape == ((ad,) if n == 1 else (n, ad)) == want.shape
    print('n', n, 'cfg', cfg_scale, 'max err', float(np.abs(got - want).max()), 'saturated', float((np.abs(want) == 1).mean()))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    assert (np.abs(got) <= 1).all()
    if n > 1:
        assert (np.abs(want) == 1).any() and (np.abs(got) == 1).any()
    for j in sorted({0, n // 2, n - 1}):
        one = a.sample_actions(obs[j], goals[j], noises=sn[j], cfg=cfg_scale)
        assert one.shape == (ad,)
        np.testing.assert_array_equal(one, got.reshape(n, ad)[j])


def test_sample_actions_goal_broadcast_seed_and_default_cfg(sampler512):
    a, ref = sampler512
    obs, goals, sn = sampler512_inputs(37)
    tiled = a.sample_actions(obs, np.tile(goals[:1], (37, 1)), noises=sn)
    np.testing.assert_array_equal(a.sample_actions(obs, goals[0], noises=sn), tiled)       # one [G] for every row
    np.testing.assert_array_equal(a.sample_actions(obs, goals[:1], noises=sn), tiled)
    np.testing.assert_array_equal(tiled, a.sample_actions(obs, np.tile(goals[:1], (37, 1)), noises=sn, cfg=3.0))   # cfg=None: the config's 3.0
    np.testing.assert_array_equal(a.sample_actions(obs, goals, seed=7), a.sample_actions(obs, goals, seed=7))
    assert np.abs(a.sample_actions(obs, goals, seed=7) - a.sample_actions(obs, goals, seed=8)).max() > 0
    with pytest.raises(ValueError):
        a.sample_actions(obs, goals[:5], noises=sn)


def test_trajectory_100_updates_tracks_restatement():
    """Bounds as tests/test_gpu_bc.py fits its trajectory: every info within 2e-3 relative, every parameter within 5e-3 after 100 steps."""
    cfg = _cfg()
    rng = np.random.default_rng(9)
    ds = CO.make_gc_dataset(OD, AD, seed=3, lengths=(400, 300, 324))
    a = _agent(cfg)
    ref = CO.OracleCFGRL(a.get_params(), dict(cfg), OD, AD, GD, np.float64)
    for _ in range(100):
        idx, gi = rng.integers(0, 1024, size=64), rng.integers(0, 1024, size=64)
        batch = {'observations': ds['observations'][idx], 'actions': ds['actions'][idx], 'actor_goals': ds['observations'][gi]}
        noise = {'x0': rng.standard_normal((64, AD)).astype(np.float32), 't': rng.random(64).astype(np.float32)}
        mask = rng.random(64) < 0.1
        _, info = a.update(batch, noise=noise, do_cfg=mask)
        _, want = ref.update(batch, noise, mask)
    info = info.to_dict()
    print('trajectory', info, want)
    for k in CO.INFO_KEYS:
        assert abs(info[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, info[k], want[k])
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg = _cfg()
    batch, noise, mask = _data(OD, AD, GD, 64, seed=6)
    a = _agent(cfg)
    for _ in range(3):
        a.update(batch, noise=noise, do_cfg=mask)
    a.synchronize()
    sd = checkpoint.to_state_dict(a)
    assert set(sd) == {'rng', 'network'} and set(sd['network']) == {'step', 'params', 'opt_state'}
    assert set(sd['network']['params']) == {'modules_actor_flow', 'modules_unc_embed'}
    checkpoint.save_agent(a, str(tmp_path), 3)
    b = _agent(cfg, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 3)
    _same_state(a, b)
    a.update(batch, noise=noise, do_cfg=mask); b.update(batch, noise=noise, do_cfg=mask)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
