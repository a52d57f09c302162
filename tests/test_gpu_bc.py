"""GPU: the BC agent (agents/bc.py) on the engine against the fp64 restatement in tests/bc_oracle.py.  Tolerances are the ones
tests/test_gpu_ifql.py holds its agent to: infos rtol 5e-5 / atol 5e-6, per-leaf gradients (Adam mu / 0.1) within 2e-5 max|g| + 1e-9,
sampled actions atol 2e-5.

test_paths_match_fp64_restatement runs the first-update comparison at hidden 512 x 4 (wide1024: 1024 x 2) after asserting from the
engine's plan (fql_debug_plan; [M, N, K] of a GEMM task, rows per tile) the launches the case is named for:
  humanoidmaze (obs 69, act 21, B 256, with and without LayerNorm): layer 0 [256, 512, 128], head [256, 32, 512] and its dgrad
      [256, 512, 32] on the 16-row kernel (padded action width 32), weight gradients (M, Kin, N) = (256, 128, 512) and (256, 512, 32)
  act16 (obs 29, act 16, B 256): head [256, 16, 512], dgrad [256, 512, 16], no task 32 wide
  b1024 (obs 40, act 4): every 512 x 512 task on fql_side_big_kernel's 64-row tiles at M 1024
  b272 (obs 29, act 8): every task at M 272 on fql_gemm16_kernel<false> (16 rows)
  wide1024 (B 48): every K 1024 task on fql_gemm16_kernel<true>: [48, 1024, 1024] and the head [48, 16, 1024]
No plan holds an OP_DGRAD0 launch or a dgrad with N = in_p: BC takes no input gradient of layer 0, at any action width.  Measured on an
MI355X, worst |g_gpu - g_ref| / max|g_ref| over the leaves (figures, not bounds): humanoidmaze 1.1e-06, act16 1.1e-06, b1024 9.1e-07,
b272 7.4e-07, wide1024 4.7e-07, humanoidmaze without LayerNorm 4.5e-07; the sampler at obs 69 / act 21 / hidden 512: 3.0e-06 at n 4097."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import bc_oracle as BO
from tests.util import (K_GEMM16, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, OP_GEMM, OP_GEMM64, assert_info_close, leaf_dict, read_plan,
                        sync_restatement)

pytestmark = pytest.mark.gpu
OD, AD = 29, 8
OP_DGRAD0 = 24   # enum OpType (fql_amd/csrc/fql_engine.hip): the lean 16-column first-layer input gradient


def _cfg(H=64, B=64, nh=4, **kw):
    import fql_amd
    cfg = fql_amd.bc.get_config()
    cfg.update(hidden_dims=(H,) * nh, batch_size=B)
    cfg.update(kw)
    return cfg


def _data(od, ad, B, S, seed):
    rng = np.random.default_rng(seed)
    batch = {'observations': rng.standard_normal((B, od)).astype(np.float32),
             'actions': np.clip(rng.standard_normal((B, ad)), -1, 1).astype(np.float32)}
    return batch, BO.make_noise(B, ad, S, seed + 100)


def _randomized(params, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, np.float32), params)
    for p, v in O.tree_leaves_with_path(out):
        if not p.endswith('/kernel'):
            v += (scale * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def _agent(cfg, od=OD, ad=AD, seed=3, params=None):
    import fql_amd
    a = fql_amd.BCAgent.create(seed, np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32), cfg)
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


def _check_first_update(a, cfg, od, ad, batch, noise, seed=5):
    params = _randomized(a.get_params(), seed)
    a.set_params(params)
    ref = BO.OracleBC(params, dict(cfg), od, ad, np.float64)
    _, _, g_ref = ref.grads(batch, noise)
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == BO.INFO_KEYS
    _, want = ref.update(batch, noise)
    print('infos', info, want)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=BO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    assert opt['count'] == 1 and opt['step'] == 2
    mu, new, new_ref = leaf_dict(opt['mu']), leaf_dict(a.get_params()), leaf_dict(ref.params)
    for p, g in leaf_dict(g_ref).items():
        tol = 2e-5 * np.abs(g).max() + 1e-9
        print('grad', p, float(np.abs(mu[p] / 0.1 - g).max()), tol)
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        d = np.abs(new[p] - new_ref[p])
        stable = np.abs(g) > 50 * tol
        assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
        assert d.max() <= 2 * cfg['bc_lr'] + 1e-6, p


def test_leaf_names_shapes_and_init_statistics():
    cfg = _cfg(512, 64)
    a = _agent(cfg)
    want = {p: v.shape for p, v in O.tree_leaves_with_path(BO.init_params(0, OD, AD, cfg))}
    assert dict(a.leaves()) == want
    assert set(a.get_params()) == {'MLP_0', 'Dense_0'}
    p = leaf_dict(a.get_params())
    assert p['MLP_0/Dense_0/kernel'].shape == (OD + AD + 16, 512) and p['Dense_0/kernel'].shape == (512, AD)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.startswith('MLP_0/') and k.endswith('/kernel'):   # default_init: Glorot uniform
            lim = np.sqrt(6.0 / (v.shape[0] + v.shape[1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
    hk = p['Dense_0/kernel']   # lecun_normal: variance 1 / fan_in, truncated at 2 sigma of the untruncated normal; 4096 samples
    assert abs(hk.var() * 512 - 1.0) < 0.1 and abs(hk.mean()) < 4.0 / np.sqrt(512 * hk.size)
    assert np.abs(hk).max() <= 2.0 * np.sqrt(1.0 / 512) / 0.87962566103423978 * (1 + 1e-6)
    a2 = _agent(_cfg(64, 64, use_layer_norm=0))
    assert not any('LayerNorm' in k for k, _ in a2.leaves())


@pytest.mark.parametrize('H,B', [(64, 64), (512, 256)])
@pytest.mark.parametrize('ln', [1, 0])
def test_one_update_matches_fp64_restatement(H, B, ln):
    cfg = _cfg(H, B, use_layer_norm=ln)
    batch, noise = _data(OD, AD, B, 16, seed=1)
    k = np.rint(noise['t'] * 16)
    assert k[0] == 0 and k[1] == 16
    _check_first_update(_agent(cfg), cfg, OD, AD, batch, noise)


def test_policy_loss_matches_and_changes_no_state():
    cfg = _cfg()
    batch, noise = _data(OD, AD, 64, 16, seed=2)
    a = _agent(cfg)
    a.update(batch, noise=noise)
    a.synchronize()
    before, info_before = leaf_dict(a.get_params()), a.read_info()
    opt_before = a.get_opt_state()
    b2, n2 = _data(OD, AD, 64, 16, seed=12)
    loss, info = a.policy_loss(b2, noise=n2)
    ref = BO.OracleBC(a.get_params(), dict(cfg), OD, AD, np.float64)
    want = ref.policy_loss(b2, n2)[0]
    assert abs(loss - want) <= 5e-5 * abs(want) + 5e-6 and info == {'bc_loss': loss}
    a.synchronize()
    for k, v in leaf_dict(a.get_params()).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
    opt = a.get_opt_state()
    assert (opt['count'], opt['step']) == (opt_before['count'], opt_before['step']) == (1, 2)
    for part in ('mu', 'nu'):
        for k, v in leaf_dict(opt[part]).items():
            np.testing.assert_array_equal(v, leaf_dict(opt_before[part])[k])
    assert a.read_info() == info_before


def test_trajectory_100_updates_tracks_restatement():
    """Bounds as tests/test_gpu_ifql.py fits its trajectory: every info within 2e-3 relative, every parameter within 5e-3 after 100 steps."""
    cfg = _cfg()
    rng = np.random.default_rng(9)
    ds = O.make_synthetic_dataset(1024, OD, AD, seed=3)
    a = _agent(cfg)
    ref = BO.OracleBC(a.get_params(), dict(cfg), OD, AD, np.float64)
    for _ in range(100):
        idx = rng.integers(0, 1024, size=64)
        batch = {'observations': ds['observations'][idx], 'actions': ds['actions'][idx]}
        noise = {'x0': rng.standard_normal((64, AD)).astype(np.float32),
                 't': (rng.integers(0, 17, size=64).astype(np.float32) / np.float32(16))}
        _, info = a.update(batch, noise=noise)
        _, want = ref.update(batch, noise)
    info = info.to_dict()
    print('trajectory', info, want)
    for k in BO.INFO_KEYS:
        assert abs(info[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, info[k], want[k])
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


def test_update_from_dataset_explicit_rows_equals_update():
    cfg = _cfg()
    ds = O.make_synthetic_dataset(512, OD, AD, seed=4)
    _, noise = _data(OD, AD, 64, 16, seed=4)
    idx = np.random.default_rng(4).integers(0, 512, size=64)
    a, b = _agent(cfg), _agent(cfg)
    a.upload_dataset(ds)
    for _ in range(3):
        a.update_from_dataset(idxs=idx, noise=noise)
        b.update({'observations': ds['observations'][idx], 'actions': ds['actions'][idx]}, noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def test_aql_and_graph_updates_bitwise_over_20_steps():
    import torch
    cfg = _cfg()
    ds = O.make_synthetic_dataset(512, OD, AD, seed=5)
    a, b = _agent(cfg), _agent(cfg)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for _ in range(20):
        a.update_from_dataset()
        b.update_from_dataset(stream=s.cuda_stream)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.get_opt_state()['count'] == 20


def _check_step(a, ref, cfg, batch, noise):
    """One more update, moments carried from earlier steps, from the engine's own pre-step state: the 4 infos at the first step's bounds,
    every leaf's gradient as (mu - 0.9 mu0) / 0.1 (tests/test_gpu_ifql.py::_check_step's bounds), nu and the parameter step."""
    sync_restatement(ref, a)
    _, _, g_ref = ref.grads(batch, noise)
    mu0, pre = leaf_dict(a.get_opt_state()['mu']), leaf_dict(a.get_params())
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == BO.INFO_KEYS
    _, want = ref.update(batch, noise)
    print('infos', info, want)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=BO.INFO_KEYS)
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
        assert d.max() <= 2 * cfg['bc_lr'] + 1e-6, p


def test_batch_size_switches_track_restatement():
    """B = 64, 16, 256, 64: each switch rebuilds the workspace and programs; every step is compared after the rebuild, from the engine's
    own pre-step state.  Then update_from_dataset after a switch equals update on the same rows, bitwise."""
    cfg = _cfg()
    a = _agent(cfg)
    params = _randomized(a.get_params(), 15)
    a.set_params(params)
    ref = BO.OracleBC(params, dict(cfg), OD, AD, np.float64)
    for i, B in enumerate((64, 16, 256, 64)):
        batch, noise = _data(OD, AD, B, 16, seed=20 + i)
        assert a.get_opt_state()['count'] == i
        _check_step(a, ref, cfg, batch, noise)
    opt = a.get_opt_state()
    assert opt['count'] == 4 and opt['step'] == 5
    ds = O.make_synthetic_dataset(512, OD, AD, seed=21)
    x, y = _agent(cfg, params=params), _agent(cfg, params=params)
    x.upload_dataset(ds)
    for B in (64, 32):
        idx = np.random.default_rng(B).integers(0, 512, size=B)
        _, noise = _data(OD, AD, B, 16, seed=30 + B)
        x.update_from_dataset(batch_size=B, idxs=idx, noise=noise)
        y.update({'observations': ds['observations'][idx], 'actions': ds['actions'][idx]}, noise=noise)
    x.synchronize(); y.synchronize()
    _same_state(x, y)


@pytest.mark.parametrize('od,ad,nh,S', [(5, 1, 4, 16), (29, 8, 2, 4), (70, 17, 4, 1), (29, 17, 2, 16), (5, 8, 4, 4)])
def test_update_and_sampling_across_shapes(od, ad, nh, S):
    cfg = _cfg(64, 32, nh, denoise_steps=S)
    batch, noise = _data(od, ad, 32, S, seed=od + ad)
    a = _agent(cfg, od, ad)
    _check_first_update(a, cfg, od, ad, batch, noise)
    ref = BO.OracleBC(a.get_params(), dict(cfg), od, ad, np.float64)
    sn = np.random.default_rng(1).standard_normal((5, ad)).astype(np.float32)
    np.testing.assert_allclose(a.sample_actions(batch['observations'][:5], noises=sn), ref.sample_actions(batch['observations'][:5], sn),
                               rtol=0, atol=2e-5)


@pytest.mark.parametrize('n', [1, 5, 16, 37, 256, 4097])
def test_sample_actions_match_oracle_and_single_calls(n):
    cfg = _cfg()
    params = _randomized(BO.init_params(8, OD, AD, cfg), 8)
    # The head is scaled by 2 so that the velocities are O(2) and a large share of the coordinates leaves [-1, 1]: the clip is reached.
    # The scale stays where fp32 itself holds the 2e-5 bound: tests/test_bc_cpu.py::test_fp32_rounding_of_the_sampler_grows_with_the_head_scale
    # shows the fp32 numpy restatement of these very inputs within 3e-6 of fp64 at this scale and beyond 2e-5 at a scale of 6.
    params['Dense_0']['kernel'] *= 2.0
    a = _agent(cfg, params=params)
    ref = BO.OracleBC(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(n)
    obs = rng.standard_normal((n, OD)).astype(np.float32)
    sn = rng.standard_normal((n, AD)).astype(np.float32)
    got = a.sample_actions(obs, noises=sn, temperature=0.3)   # temperature: accepted and ignored
    want = ref.sample_actions(obs, sn)
    assert got.shape == ((AD,) if n == 1 else (n, AD)) == want.shape
    print('n', n, 'max err', float(np.abs(got - want).max()), 'saturated', int((np.abs(want) == 1).sum()))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    assert (np.abs(want) == 1).any() and (np.abs(got) <= 1).all()
    assert (got.reshape(n, AD)[np.abs(want.reshape(n, AD)) == 1] == want.reshape(n, AD)[np.abs(want.reshape(n, AD)) == 1]).mean() > 0.99
    for j in sorted({0, n // 2, n - 1}):   # row j of the batched call is the single-observation call on the same noise
        one = a.sample_actions(obs[j], noises=sn[j])
        assert one.shape == (AD,)
        np.testing.assert_array_equal(one, got.reshape(n, AD)[j])
    assert a.sample_actions(obs[:1], noises=sn[:1]).shape == (AD,)   # [1, od] -> [act]: the reference's squeeze
    if n == 5:   # engine RNG: a seed fixes the draw, chunking does not change it
        np.testing.assert_array_equal(a.sample_actions(obs, seed=7), a.sample_actions(obs, seed=7))


@pytest.mark.parametrize('S', [1, 3])
def test_sampler_program_at_two_hidden_layers_and_act_1(S):
    """The sampler's program away from S = 16, nl = 5: hidden 64 x 2 (nl = 3), obs 5, act 1 (the narrowest padded width).  bc_stats counts
    the launches of the built program: assemble, step-bias table, C0, S (layer 0 + 2 GEMMs), extract.  At S = 1 the first Euler step is
    also the last one (the head's epilogue adds v / S and writes the clipped actions in one launch)."""
    od, ad = 5, 1
    cfg = _cfg(64, 32, 2, denoise_steps=S)
    params = _randomized(BO.init_params(8, od, ad, cfg), 8)
    a = _agent(cfg, od, ad, params=params)
    assert a.bc_stats()[2] == 4 + S * 3
    ref = BO.OracleBC(params, dict(cfg), od, ad, np.float64)
    rng = np.random.default_rng(S)
    obs = rng.standard_normal((17, od)).astype(np.float32)
    sn = rng.standard_normal((17, ad)).astype(np.float32)
    for n in (5, 17):
        got = a.sample_actions(obs[:n], noises=sn[:n])
        want = ref.sample_actions(obs[:n], sn[:n])
        assert got.shape == (n, ad) == want.shape
        print('S', S, 'n', n, 'max err', float(np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    for j in range(17):   # row j of the n = 17 call is the single-row call on row j
        np.testing.assert_array_equal(a.sample_actions(obs[j], noises=sn[j]), got[j])


# ---- hidden 512 at the shapes and batches that switch kernels: what the update program's plan holds --------------------------------
def _gemm(plan, kernels=None):
    return [dict(t, kernel=L['kernel'], type=L['type']) for L in plan if kernels is None or L['kernel'] in kernels for t in L['gemm']]


def _wgrad(plan):
    return {(t['M'], t['Kin'], t['N']) for L in plan for t in L['wgrad']}


def _has(tasks, M, N, K, **kw):
    return [t for t in tasks if (t['M'], t['N'], t['K']) == (M, N, K) and all(t[k] == v for k, v in kw.items())]


def _p_humanoidmaze(plan, B):
    g = _gemm(plan)
    assert not [L for L in plan if L['type'] == OP_DGRAD0]       # BC takes no first-layer input gradient, at any action width
    assert _has(g, B, 512, 128)                                  # layer 0 at in_p 128 (69 + 21 + 16 = 106)
    assert _has(g, B, 32, 512, rows=16, kernel=K_GEMM16)         # the head at the padded action width 32
    assert _has(g, B, 512, 32)                                   # ... and its dgrad: K = 32
    assert not [t for t in g if t['N'] == 128]                   # no first-layer dgrad
    assert {(B, 128, 512), (B, 512, 32)} <= _wgrad(plan)


def _p_act16(plan, B):
    g = _gemm(plan)
    assert not [L for L in plan if L['type'] == OP_DGRAD0]
    assert _has(g, B, 16, 512, rows=16, kernel=K_GEMM16) and _has(g, B, 512, 16)   # act == padded width 16: no padding column
    assert not [t for t in g if t['N'] == 32 or t['K'] == 32] and (B, 512, 16) in _wgrad(plan)


def _p_b1024(plan, B):
    hid = [t for t in _gemm(plan) if (t['N'], t['K']) == (512, 512)]
    assert hid and all(t['M'] == B and t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in hid)   # fql_side_big_kernel's 64-row tiles
    assert (B, 512, 512) in _wgrad(plan) and B in {m for L in plan for m in L['ln']}


def _p_b272(plan, B):
    g = _gemm(plan)
    assert g and all(t['M'] == B and t['rows'] == 16 and t['kernel'] == K_GEMM16 and t['type'] == OP_GEMM for t in g)   # M % 64 != 0
    assert _has(g, B, 512, 512) and (B, 512, 512) in _wgrad(plan) and B in {m for L in plan for m in L['ln']}


def _p_wide1024(plan, B):
    kbig = [t for t in _gemm(plan) if t['K'] > 512]
    assert kbig and all(t['kernel'] == K_GEMM16_KBIG and t['rows'] == 16 for t in kbig)
    assert _has(kbig, B, 1024, 1024) and _has(kbig, B, 16, 1024) and (B, 1024, 1024) in _wgrad(plan)


def _p_w50_padded(plan, B):
    g = _gemm(plan)
    assert not [L for L in plan if L['type'] == OP_DGRAD0]
    assert g and all(t['M'] == B and t['rows'] == 16 and t['kernel'] == K_GEMM16 and t['type'] == OP_GEMM for t in g)
    assert _has(g, B, 64, 64) and (B, 64, 64) in _wgrad(plan) and B in {m for L in plan for m in L['ln']}   # out 50 of out_p 64


H512_CASES = {   # id -> (od, ad, hidden, B, S, use_layer_norm, plan assertion)
    'humanoidmaze': (69, 21, (512,) * 4, 256, 16, 1, _p_humanoidmaze),
    'act16': (29, 16, (512,) * 4, 256, 16, 1, _p_act16),
    'b1024': (40, 4, (512,) * 4, 1024, 16, 1, _p_b1024),
    'b272': (29, 8, (512,) * 4, 272, 16, 1, _p_b272),
    'wide1024': (29, 8, (1024,) * 2, 48, 16, 1, _p_wide1024),
    'humanoidmaze-no-ln': (69, 21, (512,) * 4, 256, 16, 0, _p_humanoidmaze),
    'w50-padded': (29, 8, (50, 50, 50), 32, 16, 1, _p_w50_padded),   # hidden widths that are no multiple of 16: LayerNorm over 50 of 64 columns
}


@pytest.mark.parametrize('cid', list(H512_CASES))
def test_paths_match_fp64_restatement(cid):
    """Each case first asserts, from the engine's own plan (fql_debug_plan), the path its id names, then runs _check_first_update at its
    bounds.  fql_bc_prep_kernel is one entry in the plan; it writes vel at the padded action stride (32 at humanoidmaze)."""
    od, ad, hidden, B, S, ln, check = H512_CASES[cid]
    cfg = _cfg(B=B, hidden_dims=hidden, denoise_steps=S, use_layer_norm=ln)
    batch, noise = _data(od, ad, B, S, seed=40 + od + ad)
    a = _agent(cfg, od, ad)
    plan = read_plan(a)
    print(cid, 'gemm (kernel, type, M, N, K, rows):', sorted({(t['kernel'], t['type'], t['M'], t['N'], t['K'], t['rows']) for t in _gemm(plan)}))
    print(cid, 'wgrad (M, Kin, N):', sorted(_wgrad(plan)), 'ln M:', sorted({m for L in plan for m in L['ln']}),
          'other launch types:', sorted({L['type'] for L in plan if L['type'] not in (OP_GEMM, OP_GEMM64)}))
    check(plan, B)
    _check_first_update(a, cfg, od, ad, batch, noise)
    check(read_plan(a), B)   # reading the plan changed no launch


def test_batch_size_walk_at_hidden_512():
    """B = 256, 1024, 272, 256 on one hidden-512 handle: 32-row tiles, fql_side_big_kernel's 64-row tiles, the 16-row kernel, and back.
    The rebuilt plan holds the new row count only; every step is compared from the engine's own pre-step state."""
    cfg = _cfg(512, 256)
    a = _agent(cfg)
    params = _randomized(a.get_params(), 16)
    a.set_params(params)
    ref = BO.OracleBC(params, dict(cfg), OD, AD, np.float64)
    tiles = {256: (32, K_SIDE), 1024: (64, K_SIDE_BIG), 272: (16, K_GEMM16)}
    for i, B in enumerate((256, 1024, 272, 256)):
        batch, noise = _data(OD, AD, B, 16, seed=50 + i)
        assert a.get_opt_state()['count'] == i
        _check_step(a, ref, cfg, batch, noise)
        plan = read_plan(a)
        assert {t['M'] for t in _gemm(plan)} == {B} == {M for M, _, _ in _wgrad(plan)}
        hid = _has(_gemm(plan), B, 512, 512)
        assert hid and {(t['rows'], t['kernel']) for t in hid} == {tiles[B]}
    assert a.get_opt_state()['count'] == 4


SAMPLER512 = dict(od=69, ad=21, hidden=(512,) * 4, scale=2.0, ns=(1, 37, 4097))


def sampler512_problem(scale=SAMPLER512['scale']):
    """(cfg, params) of the sampler at the humanoidmaze shape (act 21: fql_bc_layer0_kernel strides the action rows by the padded width
    32, and the head's GF_EULER | GF_EULER_BARE epilogue adds into rows of that stride), hidden 512, the head scaled by 2 as above.
    tests/test_bc_cpu.py::test_fp32_rounding_of_the_sampler_at_hidden_512 holds fp32 numpy to 5e-6 of fp64 on these inputs."""
    cfg = _cfg(hidden_dims=SAMPLER512['hidden'], batch_size=256)
    params = _randomized(BO.init_params(8, SAMPLER512['od'], SAMPLER512['ad'], cfg), 8)
    params['Dense_0']['kernel'] *= np.float32(scale)
    return cfg, params


def sampler512_inputs(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal((n, SAMPLER512['od'])).astype(np.float32), rng.standard_normal((n, SAMPLER512['ad'])).astype(np.float32)


@pytest.fixture(scope='module')
def sampler512():
    cfg, params = sampler512_problem()
    od, ad = SAMPLER512['od'], SAMPLER512['ad']
    return _agent(cfg, od, ad, params=params), BO.OracleBC(params, dict(cfg), od, ad, np.float64)


@pytest.mark.parametrize('n', SAMPLER512['ns'])
def test_sample_actions_at_hidden_512_and_padded_action_width_32(sampler512, n):
    """n = 1, 37 and 4097 (one row past the 4096-row chunk) against the restatement at 2e-5; the clip is reached; rows 0, n // 2 and n - 1
    are bitwise the single-observation calls."""
    a, ref = sampler512
    ad = SAMPLER512['ad']
    obs, sn = sampler512_inputs(n)
    got = a.sample_actions(obs, noises=sn)
    want = ref.sample_actions(obs, sn)
    assert got.shape == ((ad,) if n == 1 else (n, ad)) == want.shape
    print('n', n, 'max err', float(np.abs(got - want).max()), 'saturated', int((np.abs(want) == 1).sum()))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    assert (np.abs(want) == 1).any() and (np.abs(got) == 1).any() and (np.abs(got) <= 1).all()
    for j in sorted({0, n // 2, n - 1}):
        one = a.sample_actions(obs[j], noises=sn[j])
        assert one.shape == (ad,)
        np.testing.assert_array_equal(one, got.reshape(n, ad)[j])


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg = _cfg()
    batch, noise = _data(OD, AD, 64, 16, seed=6)
    a = _agent(cfg)
    for _ in range(3):
        a.update(batch, noise=noise)
    a.synchronize()
    sd = checkpoint.to_state_dict(a)
    assert set(sd) == {'rng', 'policy'} and set(sd['policy']) == {'step', 'params', 'opt_state'}
    assert set(sd['policy']['params']) == {'Dense_0', 'MLP_0'}
    checkpoint.save_agent(a, str(tmp_path), 3)
    b = _agent(cfg, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 3)
    _same_state(a, b)
    a.update(batch, noise=noise); b.update(batch, noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)


def test_fql_and_bc_interleaved_end_where_they_end_alone():
    import fql_amd
    from tests.util import make_problem
    fcfg, ds, fbatch, fnoise = make_problem(OD, AD, 64, (64,) * 4, seed=7)
    cfg = _cfg()
    batch, noise = _data(OD, AD, 64, 16, seed=7)

    def fql():
        return fql_amd.FQLAgent.create(1, fbatch['observations'][:1], fbatch['actions'][:1], fcfg)
    f_alone, b_alone, f_mix, b_mix = fql(), _agent(cfg), fql(), _agent(cfg)
    for _ in range(5):
        f_alone.update(fbatch, noise=fnoise)
    for _ in range(5):
        b_alone.update(batch, noise=noise)
    for _ in range(5):
        f_mix.update(fbatch, noise=fnoise)
        b_mix.update(batch, noise=noise)
    for x in (f_alone, b_alone, f_mix, b_mix):
        x.synchronize()
    _same_state(f_alone, f_mix)
    _same_state(b_alone, b_mix)


def test_refusals_and_info_width():
    import fql_amd
    from fql_amd import _cabi
    from tests.util import make_problem
    lib = _cabi.load()
    cfg = _cfg()
    batch, noise = _data(OD, AD, 64, 16, seed=8)
    a = _agent(cfg)
    h = a._h
    E = _cabi.FQL_E_STATE
    f = lambda arr: arr.ctypes.data_as(C.c_void_p)
    ob, ac = batch['observations'], batch['actions']
    r = np.zeros(64, np.float32)
    buf = (C.c_float * 16)()
    i64 = (C.c_int64 * 2)()
    sz = (C.c_size_t * 2)()
    assert lib.fql_num_info(h) == 4
    assert [lib.fql_handle_info_name(h, i).decode() for i in range(4)] == list(BO.INFO_KEYS)
    assert lib.fql_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None) == E
    assert lib.fql_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None) == E
    assert lib.fql_update_from_dataset(h, None, 64, 0, 0, None, None, None) == E
    assert lib.fql_sample_actions(h, f(ob), 1, None, 0, buf, None) == E
    assert lib.fql_flow_actions(h, f(ob), f(ac), 1, buf, None) == E
    assert lib.fql_update_begin(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None) == E
    assert lib.fql_update_end(h, None, None) == E
    st = C.c_void_p(1)
    st2 = C.c_void_p(2)
    assert lib.fql_update_begin_split(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, st, st2) == E
    assert lib.fql_update_end_split(h, None, st, st2) == E
    assert lib.fql_update_from_dataset_begin(h, None, 64, 0, 0, None, None) == E
    assert lib.fql_update_from_dataset_begin_split(h, None, 64, 0, 0, None, st, st2) == E
    u8 = np.zeros(64, np.uint8)
    assert lib.fql_dataset_add_frames(h, f(u8), f(u8), f(ac), 0.0, 1.0) == E
    assert lib.fql_replay_add_frames(h, f(u8), f(u8), f(ac), 0.0, 1.0) == E
    assert lib.fql_dataset_upload_frames(h, 1, f(u8), f(u8), f(ac), f(r), f(r), f(r), 1, 0.0) == E
    assert lib.fql_update_from_frames(h, None, None, 64, 0, 0, None, None, None) == E
    assert lib.fql_replay_add(h, f(ob), f(ac), 0.0, 1.0, f(ob)) == E
    assert lib.fql_info_wait(h, 0, buf) == E
    assert lib.fql_grad_buckets(h, sz, sz) == E
    assert lib.fql_replay_create(h, 128) == E
    assert lib.fql_replay_size(h, i64, i64) == E
    assert lib.fql_update_balanced(h, None, None, None, 64, None, None, None) == E
    assert lib.fql_read_info(h, buf) == E
    assert lib.fql_rebrac_update(h, f(ob), f(ac), f(r), f(r), f(ob), f(ac), 64, None, 1, None, None) == E
    assert lib.fql_sac_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None) == E
    assert lib.fql_sac_sample_actions(h, f(ob), 1, None, 0, 1.0, buf, None) == E
    assert lib.fql_rebrac_update_from_dataset(h, None, 64, 0, 0, None, 1, None, None) == E
    assert lib.fql_rebrac_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), f(ac), 64, None, 1, None, None, None) == E
    assert lib.fql_rebrac_sample_actions(h, f(ob), 1, None, 0, 1.0, buf, None) == E
    assert lib.fql_sac_update_from_dataset(h, None, 64, 0, 0, None, None, None) == E
    assert lib.fql_sac_update_balanced(h, None, None, 64, None, None, None) == E
    assert lib.fql_sac_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None) == E
    assert lib.fql_read_info(h, buf) == E and b'4 infos' in lib.fql_last_error(h) and b'BC handle' in lib.fql_last_error(h)
    keys = (C.c_uint32 * 20)()
    nz = _cabi.FqlNoise()
    assert lib.fql_noise_from_jax_keys(h, keys, 0, 64, C.byref(nz), None) == E
    grp = C.c_void_p()
    hs = (C.c_void_p * 1)(h)
    assert lib.fql_group_create(hs, 1, C.byref(grp)) == E
    # fql_bc_* on another handle
    fcfg, _, fbatch, _ = make_problem(OD, AD, 64, (64,) * 4, seed=7)
    fa = fql_amd.FQLAgent.create(1, fbatch['observations'][:1], fbatch['actions'][:1], fcfg)
    assert lib.fql_bc_update(fa._h, f(ob), f(ac), 64, None, None, None) == E
    assert lib.fql_bc_sample_actions(fa._h, f(ob), 1, None, 0, buf, None) == E
    assert lib.fql_bc_policy_loss(fa._h, f(ob), f(ac), 64, None, None, None) == E
    assert lib.fql_bc_update_from_dataset(fa._h, None, 64, 0, 0, None, None, None) == E
    assert lib.fql_bc_stats(fa._h, i64, i64, i64) == E
    import fql_amd.ifql
    ia = fql_amd.IFQLAgent.create(1, fbatch['observations'][:1], fbatch['actions'][:1], fql_amd.ifql.get_config())   # (IFQL has no calls of its
    assert lib.fql_bc_update(ia._h, f(ob), f(ac), 64, None, None, None) == E                                         # own besides create)
    # create-time refusals
    c = _cabi.FqlConfig(); lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim = OD, AD
    bc = _cabi.FqlBcConfig(); lib.fql_bc_default_config(C.byref(bc))
    assert bc.denoise_steps == 16
    out = C.c_void_p()
    for field in ('encoder', 'precision'):
        c2 = _cabi.FqlConfig.from_buffer_copy(c)
        setattr(c2, field, 2 if field == 'precision' else 1)
        assert lib.fql_bc_create(C.byref(c2), C.byref(bc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    # noise: any pointer but x0 / t is FQL_E_INVALID; an off-grid t too (ValueError on the host before the call)
    bad = _cabi.FqlNoise(f(noise['x0']), None, None, None, None)
    assert lib.fql_bc_update(h, f(ob), f(ac), 64, C.byref(bad), None, None) == _cabi.FQL_E_INVALID
    off = np.full(64, 0.3, np.float32)
    bad = _cabi.FqlNoise(None, f(noise['x0']), f(off), None, None)
    assert lib.fql_bc_update(h, f(ob), f(ac), 64, C.byref(bad), None, None) == _cabi.FQL_E_INVALID
    with pytest.raises(ValueError):
        a.update(batch, noise={'x0': noise['x0'], 't': off})
    with pytest.raises(ValueError):
        a.update(batch, noise={'x0': noise['x0'], 'eps1': noise['x0']})
    assert a.get_opt_state()['count'] == 0
    # exactly 4 floats: the guard values after them stay
    a.update(batch, noise=noise)
    for i in range(16):
        buf[i] = -7.0
    assert lib.fql_read_info_n(h, buf, 16) == 0
    assert all(buf[i] == -7.0 for i in range(4, 16)) and all(buf[i] != -7.0 for i in range(4))
    assert lib.fql_read_info_n(h, buf, 3) == _cabi.FQL_E_INVALID
    t = C.c_uint64()
    assert lib.fql_info_enqueue(h, None, C.byref(t)) == 0
    for i in range(16):
        buf[i] = -7.0
    assert lib.fql_info_wait(h, t.value, buf) == E
    assert lib.fql_info_wait_n(h, t.value, buf, 16) == 0
    assert all(buf[i] == -7.0 for i in range(4, 16)) and buf[0] == pytest.approx(a.read_info()['bc_loss'])
    # working on a BC handle
    la, ma, ls = a.bc_stats()
    assert la > 0 and ma > 0 and ls == 4 + 16 * 5
    assert a.stats()['param_count'] == sum(int(np.prod(s)) for _, s in a.leaves())


def test_train_bc_loop():
    import fql_amd
    ds = fql_amd.Dataset.create(**O.make_synthetic_dataset(512, OD, AD, seed=11))
    val = fql_amd.Dataset.create(**O.make_synthetic_dataset(128, OD, AD, seed=12))
    a = _agent(_cfg())
    rows = fql_amd.train_bc(a, ds, steps=60, log_every=20, val_dataset=val)
    assert [r['step'] for r in rows] == [20, 40, 60]
    assert all(set(r) == {'step', 'validation/bc_loss'} | {f'training/{k}' for k in BO.INFO_KEYS} for r in rows)
    assert a.get_opt_state()['count'] == 60
    assert rows[-1]['training/bc_loss'] < rows[0]['training/bc_loss'] * 1.5 and np.isfinite(rows[-1]['validation/bc_loss'])
