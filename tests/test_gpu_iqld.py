"""GPU: the IQL-diffusion agent (agents/iql_diffusion.py, binary optimality family) on the engine against the fp64 restatement in
tests/iqld_oracle.py, on the problems of tests/iqld_cases.py.  Tolerances are the ones tests/test_gpu_ifql.py and tests/test_gpu_bc.py
hold their agents to: infos rtol 5e-5 / atol 5e-6, per-leaf gradients (from Adam's mu) within 2e-5 max|g| + 1e-9, sampled actions atol
2e-5, a 100-update trajectory within 2e-3 relative (infos) and 5e-3 (parameters).

The loss weights are discontinuous at adv = 0 and kinked at adv awr_temperature = ln 100: every compared step first asserts, on the
fp64 values, that every row keeps 1e-3 from both (iqld_cases.check_margins); no row is masked out of a comparison.

iqld_cases.PATHS run one update each at the shapes and batches where the kernels change, after asserting from the engine's plan
(fql_debug_plan, tests/util.py read_plan; [M, N, K] of a GEMM task, rows per tile) the launches the case is named for:
  humanoidmaze  obs 69, act 21, 512 x 4, B 256: actor layer 0 [512, 512, 192] (in_p 192), head [512, 32, 512] and its dgrad [512, 512, 32]
                on the 16-row kernel (padded action width 32), weight gradients (M, Kin, N) = (512, 192, 512) and (512, 512, 32)
  act16         obs 29, act 16, 512 x 4, B 256: head [512, 16, 512], dgrad [512, 512, 16], no task 32 wide (no padding column)
  b1024         obs 40, act 4, 512 x 4, B 1024: every 512 x 512 task on fql_side_big_kernel's 64-row tiles, at M 2048 and M 1024
  b272          512 x 4, B 272: M 544 and 272 only, every task on fql_gemm16_kernel<false> (16 rows, K <= 512)
  b2064-*       64 x 4, B 2064: M 4128 and 2064 only, every task on fql_gemm16_kernel<false>
  wide1024      1024 x 2, B 48: every K 1024 task on fql_gemm16_kernel<true>, [M, 1024, 1024] and the heads [M, 16, 1024] at M 48 and 96
  ragged        critic / value (48, 80, 64), actor (128, 64, 96), B 32: [M, 80, 48], [M, 64, 80], [M, 16, 64] at M 32 and 64; [64, 64, 128],
                [64, 96, 64], [64, 16, 96]
No plan holds an OP_DGRAD0 launch or a first-layer dgrad (N = in_p): this agent takes no input gradient of a layer 0, so the act_dim <= 16
admission of OP_DGRAD0 is out of its reach at act 16 and at act 21 alike, and the cases assert that absence.  Every case landed where
reading the selection code had placed it.  Measured on an MI355X, worst |g_gpu - g_ref| / max|g_ref| over the leaves of the first update
(figures, not bounds): humanoidmaze 3.6e-06, act16 1.0e-06, b1024 1.1e-06, b272 2.1e-06, b2064-awr 1.8e-06, b2064-binary 5.1e-07,
wide1024 3.9e-06, ragged 2.3e-06; the sampler at obs 69 / act 21 / hidden 512: 6.1e-07 (cfg 0) and 1.3e-06 (cfg 3) at n 2049."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iqld_cases as K
from tests import iqld_oracle as DO
from tests.util import K_GEMM16, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, OP_GEMM, OP_GEMM64, leaf_dict, read_plan
from fql_amd.iql_diffusion import info_keys, IQLD_INFO_KEYS, IQLD_ROW_KEYS

pytestmark = pytest.mark.gpu
OD, AD = K.OD, K.AD
NETS = ('actor', 'critic', 'value')
KINDS = [(True, True), (True, False), (False, True)]
OP_DGRAD0 = 24   # enum OpType (fql_amd/csrc/fql_engine.hip): the lean 16-column first-layer input gradient


def _agent(cfg, od=OD, ad=AD, seed=3, params=None):
    import fql_amd
    a = fql_amd.agents['iql_diffusion'].create(seed, np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32), cfg)
    if params is not None:
        a.set_params(params)
    return a


def _built(c):
    cfg, params, batch, noise, ref = K.build(c)
    return cfg, params, batch, noise, ref, _agent(cfg, c['od'], c['ad'], params=params)


def _same_state(a, b):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert [oa[k] for k in ('count', 'step', 'actor_count', 'updates')] == [ob[k] for k in ('count', 'step', 'actor_count', 'updates')]
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{part} {k}')


def _assert_infos(info, want, uc, ua):
    assert tuple(info) == info_keys(uc, ua) == tuple(want)
    for k, w in want.items():
        g = info[k]
        if k in IQLD_ROW_KEYS:
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape
            print('rows', k, float(np.abs(g - w).max()))
            np.testing.assert_allclose(g, w, rtol=5e-5, atol=5e-6, err_msg=k)
        else:
            print('info', k, float(g), float(w))
            assert abs(float(g) - float(w)) <= 5e-6 + 5e-5 * abs(float(w)), (k, float(g), float(w))


def _check_step(a, ref, cfg, batch, noise, uc=True, ua=True):
    """One update of the given step kind from the engine's own pre-step state against the fp64 restatement on that state: the infos of
    that step kind (scalars and per-row arrays), every stepped leaf's gradient as (mu - 0.9 mu0) / 0.1 within 2e-5 max|g| + 1e-5 max|mu0|
    + 1e-9 (mu0 = 0 on a first update: the bound of tests/test_gpu_ifql.py), nu, the parameter step, the Polyak target, the per-TrainState
    counters; the nets that do not step keep parameters and moments bitwise."""
    a.synchronize()
    DO.sync(ref, a)
    K.check_margins(ref, batch)
    g_ref, _ = ref.grads(batch, noise, uc, ua)
    opt0 = a.get_opt_state()
    mu0, nu0, pre = leaf_dict(opt0['mu']), leaf_dict(opt0['nu']), leaf_dict(a.get_params())
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, update_critic=uc, update_actor=ua, noise=noise)
    want = ref.update(batch, noise, uc, ua)
    _assert_infos(info, want, uc, ua)
    a.synchronize()
    opt = a.get_opt_state()
    assert opt['count'] == opt0['count'] + int(uc) == ref.counts['critic'] and opt['step'] == opt['count'] + 1
    assert opt['actor_count'] == opt0['actor_count'] + int(ua) == ref.counts['actor']
    assert opt['updates'] == opt0['updates'] + 1 == ref.updates
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    stepped = [n for n in NETS if (ua if n == 'actor' else uc)]
    for p in pre:
        net = p.split('/')[0]
        if net in stepped:
            continue
        if net == 'target_critic' and uc:   # Polyak from the PRE-step critic
            assert np.abs(new[p] - new_ref[p]).max() <= 1e-6, p
            continue
        np.testing.assert_array_equal(new[p], pre[p], err_msg=f'param {p}')
        np.testing.assert_array_equal(mu[p], mu0[p], err_msg=f'mu {p}')
        np.testing.assert_array_equal(nu[p], nu0[p], err_msg=f'nu {p}')
    for net in stepped:
        lr = cfg[DO.LR_KEY[net]]
        for q, g in leaf_dict(g_ref[net]).items():
            p = f'{net}/{q}'
            tol = 2e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9
            err = float(np.abs((mu[p] - np.float32(0.9) * mu0[p]) / 0.1 - g).max())
            print('grad', p, err, tol)
            assert err <= tol, (p, err, tol)
            np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
            d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))
            stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
            assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
            assert d.max() <= 2 * lr + 1e-6, p
    return info


def test_leaf_names_shapes_and_init():
    cfg = K.config(K.case(H=512))
    a = _agent(cfg)
    want = {p: v.shape for p, v in O.tree_leaves_with_path(DO.init_params(0, OD, AD, cfg))}
    assert dict(a.leaves()) == want
    assert [p for p, _ in a.leaves()] == sorted(want)   # jax dict order
    p = leaf_dict(a.get_params())
    assert set(a.get_params()) == {'actor', 'critic', 'target_critic', 'value'}
    assert p['actor/MLP_0/Dense_0/kernel'].shape == (OD + AD + 16 + 32, 512) and p['actor/Embed_0/embedding'].shape == (2, 32)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if 'target_critic' in k:
            np.testing.assert_array_equal(v, p[k.replace('target_critic', 'critic')])
    em = p['actor/Embed_0/embedding']   # N(0, 1 / 32), 64 samples: the variance estimate has a relative sd of 0.18
    assert 0.4 < em.var() * 32 < 1.8 and np.abs(em).max() < 5 / np.sqrt(32) and np.abs(em).max() > 0
    hk = p['actor/Dense_0/kernel']
    assert abs(hk.var() * 512 - 1.0) < 0.1 and np.abs(hk).max() <= 2.0 * np.sqrt(1.0 / 512) / 0.87962566103423978 * (1 + 1e-6)
    a2 = _agent(K.config(K.case(ln=0)))
    assert not any('LayerNorm' in k for k, _ in a2.leaves())


@pytest.mark.parametrize('name', sorted(K.FIRST))
def test_one_update_matches_fp64_restatement(name):
    c = K.FIRST[name]
    cfg, params, batch, noise, ref, a = _built(c)
    info = _check_step(a, ref, cfg, batch, noise)
    w = np.asarray(info['loss_weights'])
    assert (w > 0).any() and (w == 0).any()
    if c['ov'] == 'binary_awr_loss':
        assert (w == 100.0).any()
    if name == 'b16':
        assert int(0.1 * c['B']) == 1


@pytest.mark.parametrize('name', sorted(K.SHAPES))
def test_update_and_sampling_across_shapes(name):
    c = K.SHAPES[name]
    cfg, params, batch, noise, ref, a = _built(c)
    _check_step(a, ref, cfg, batch, noise)
    DO.sync(ref, a)
    sn = np.random.default_rng(1).standard_normal((5, c['ad'])).astype(np.float32)
    for cfg_scale in (0.0, 3.0):
        got = a.sample_actions(batch['observations'][:5], noises=sn, cfg=cfg_scale)
        np.testing.assert_allclose(got, ref.sample_actions(batch['observations'][:5], sn, cfg_scale), rtol=0, atol=2e-5)


def test_batch_size_switches_track_restatement():
    """B = 64, 16, 256: each switch rebuilds the workspace and the four programs; every step is compared after the rebuild, from the
    engine's own pre-step state."""
    cfg, params, _, _, ref, a = _built(K.SWITCH[0])
    for i, c in enumerate(K.SWITCH):
        batch, noise = K.data(c)
        assert a.get_opt_state()['updates'] == i
        _check_step(a, ref, cfg, batch, noise)


# ---- the shapes and batches that switch kernels (iqld_cases.PATHS): what the update program's plan holds ----------------------------
def _gemm(plan, kernels=None):
    return [dict(t, kernel=L['kernel'], type=L['type']) for L in plan if kernels is None or L['kernel'] in kernels for t in L['gemm']]


def _wgrad(plan):
    return [t for L in plan for t in L['wgrad']]


def _has(tasks, M, N, K, **kw):
    return [t for t in tasks if (t['M'], t['N'], t['K']) == (M, N, K) and all(t[k] == v for k, v in kw.items())]


def _print_plan(name, plan):
    seen = sorted({(t['kernel'], t['type'], t['M'], t['N'], t['K'], t['rows']) for t in _gemm(plan)})
    print(name, 'gemm (kernel, type, M, N, K, rows):', seen)
    print(name, 'wgrad (M, Kin, N):', sorted({(t['M'], t['Kin'], t['N']) for t in _wgrad(plan)}), 'ln M:', sorted({m for L in plan for m in L['ln']}),
          'other launch types:', sorted({L['type'] for L in plan if L['type'] not in (OP_GEMM, OP_GEMM64)}))


def _assert_no_dgrad0(plan):
    """This agent takes no first-layer input gradient: the embedding gradient is formed from dZ0 (fql_iqld_embed_grad_kernel) and the
    critic's dQ/da is not read, so neither OP_DGRAD0 nor a generic first-layer dgrad (N = in_p) is in the plan at any action width."""
    assert not [L for L in plan if L['type'] == OP_DGRAD0]


def _assert_rows16_only(plan, kernel=K_GEMM16):
    g = _gemm(plan)
    assert g and all(t['rows'] == 16 and t['kernel'] == kernel and t['type'] == OP_GEMM for t in g), sorted({(t['kernel'], t['rows']) for t in g})


def _p_humanoidmaze(plan, c):
    B = c['B']
    _assert_no_dgrad0(plan)
    g = _gemm(plan)
    assert _has(g, 2 * B, 512, 192)                              # the actor's layer 0 at in_p 192 (69 + 21 + 16 + 32 = 138)
    assert _has(g, 2 * B, 32, 512, rows=16, kernel=K_GEMM16)     # its head at the padded action width 32
    assert _has(g, 2 * B, 512, 32)                               # the head's dgrad: K = 32
    assert not [t for t in g if t['N'] == 192 or (t['N'] == 128 and t['K'] == 512)]   # no first-layer dgrad of any net
    w = {(t['M'], t['Kin'], t['N']) for t in _wgrad(plan)}
    assert (2 * B, 192, 512) in w and (2 * B, 512, 32) in w, sorted(w)


def _p_act16(plan, c):
    B = c['B']
    _assert_no_dgrad0(plan)
    g = _gemm(plan)
    assert _has(g, 2 * B, 16, 512, rows=16, kernel=K_GEMM16)     # the head at act == padded width 16: no padding column
    assert _has(g, 2 * B, 512, 16) and not [t for t in g if t['N'] == 32 or t['K'] == 32]
    assert _has(g, 2 * B, 512, 128)                              # layer 0 at in_p 128 (29 + 16 + 48 = 93)
    assert (2 * B, 512, 16) in {(t['M'], t['Kin'], t['N']) for t in _wgrad(plan)}


def _p_b1024(plan, c):
    B = c['B']
    big = _gemm(plan, (K_SIDE_BIG,))
    assert _has(big, 2 * B, 512, 512, rows=64) and _has(big, B, 512, 512, rows=64)   # fql_side_big_kernel's 64-row tiles at M 2048 and 1024
    hid = [t for t in _gemm(plan) if (t['N'], t['K']) == (512, 512)]
    assert hid and all(t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in hid)
    assert {t['M'] for t in _wgrad(plan)} == {B, 2 * B} and 2 * B in {m for L in plan for m in L['ln']}


def _p_b272(plan, c):
    B = c['B']
    _assert_rows16_only(plan)                                    # M 544 and 272: no multiple of 64, every GEMM on the 16-row kernel at K <= 512
    g = _gemm(plan)
    assert _has(g, 2 * B, 512, 512) and _has(g, B, 512, 512) and {t['M'] for t in g} == {B, 2 * B}
    assert {t['M'] for t in _wgrad(plan)} == {B, 2 * B} and 2 * B in {m for L in plan for m in L['ln']}
    assert (2 * B) // 16 == 34 and B % 256 == 16


def _p_b2064(plan, c):
    B = c['B']
    _assert_rows16_only(plan)                                    # M 4128 and 2064 (no multiple of 64): the 16-row fallback above 1024 rows
    g = _gemm(plan)
    assert _has(g, 2 * B, 64, 64) and _has(g, B, 64, 64) and {t['M'] for t in g} == {B, 2 * B}
    assert {t['M'] for t in _wgrad(plan)} == {B, 2 * B}
    assert B > 2048 and B % 256 == 16


def _p_wide1024(plan, c):
    B = c['B']
    g = _gemm(plan)
    kbig = [t for t in g if t['K'] > 512]
    assert kbig and all(t['kernel'] == K_GEMM16_KBIG and t['rows'] == 16 for t in kbig)
    for M in (B, 2 * B):                                         # critic (B rows), value and actor (2B rows): hidden layer and head
        assert _has(kbig, M, 1024, 1024)
    assert _has(kbig, 2 * B, 16, 1024) and _has(kbig, B, 16, 1024)
    assert {(2 * B, 1024, 1024), (B, 1024, 1024)} <= {(t['M'], t['Kin'], t['N']) for t in _wgrad(plan)}


def _p_ragged(plan, c):
    B = c['B']
    g = _gemm(plan)
    for M in (B, 2 * B):                                         # critic on B rows, value on 2B: 48 -> 80 -> 64
        assert _has(g, M, 80, 48) and _has(g, M, 64, 80) and _has(g, M, 16, 64)
    assert _has(g, 2 * B, 64, 128) and _has(g, 2 * B, 96, 64) and _has(g, 2 * B, 16, 96)   # the actor: 128 -> 64 -> 96 -> act
    assert {(2 * B, 64, 96), (2 * B, 128, 64), (B, 48, 80), (B, 80, 64)} <= {(t['M'], t['Kin'], t['N']) for t in _wgrad(plan)}


PATH_PLAN = {'humanoidmaze': _p_humanoidmaze, 'act16': _p_act16, 'b1024': _p_b1024, 'b272': _p_b272, 'b2064-awr': _p_b2064,
             'b2064-binary': _p_b2064, 'wide1024': _p_wide1024, 'ragged': _p_ragged}
PATH_TOPK = {'humanoidmaze': 25, 'act16': 25, 'b1024': 102, 'b272': 27, 'b2064-awr': 206, 'b2064-binary': 206, 'wide1024': 4, 'ragged': 3}


@pytest.mark.parametrize('name', list(K.PATHS))
def test_paths_match_fp64_restatement(name):
    """Each case first asserts, from the engine's own plan (fql_debug_plan), the path its id names, then runs one full update through
    _check_step at its bounds.  The agent's own kernels are one entry in the plan (K_OTHER); their branches follow from B and the code:
    fql_iqld_weight_kernel reads the weights from global memory when B > 2048 (b2064-*), its loops and those of the two loss kernels
    run B / 256 rows per thread with a strided tail of 16 rows at B 272 and 2064 and four rows per thread at B 1024, and
    fql_iqld_embed_grad_kernel fills cs[H] in H / 256 strides (four at wide1024).  humanoidmaze and b1024 go on with a critic-only and an
    actor-only step on fresh rows: the other two programs at those sizes."""
    c = K.PATHS[name]
    cfg, params, batch, noise, ref, a = _built(c)
    plan = read_plan(a)
    _print_plan(name, plan)
    PATH_PLAN[name](plan, c)
    info = _check_step(a, ref, cfg, batch, noise)
    w = np.asarray(info['loss_weights'])
    assert w.shape == (c['B'],) and (w > 0).any() and (w == 0).any()
    assert int(0.1 * c['B']) == PATH_TOPK[name]
    if c['ov'] == 'binary_awr_loss':
        assert (w == 100.0).any()
    if name == 'b2064-binary':   # every positive weight is 1: the mass is 206 / (positive rows) only if exactly 206 tied rows are taken
        pos = int((w == 1.0).sum())
        assert pos > 206 and pos == int((w > 0).sum())
        got = float(info['loss_weights_top_10_mass'])
        print('top-10 mass', got, 206 / pos)
        assert abs(got - 206 / pos) <= 5e-6 + 5e-5 * 206 / pos
    for s, (uc, ua) in zip(K.PATH_STEPS.get(name, ()), ((True, False), (False, True))):
        b, nz = K.data(c, seed=s)
        _check_step(a, ref, cfg, b, nz, uc, ua)
    PATH_PLAN[name](read_plan(a), c)   # reading the plan changed no launch


@pytest.mark.parametrize('walk', ['walk512', 'walk64'])
def test_batch_size_walks_across_kernel_switches(walk):
    """One hidden-512 handle through B = 256, 1024, 272, 256 (the 2B-row passes on 32-row tiles, fql_side_big_kernel's 64-row tiles, the
    16-row kernel, and back) and one hidden-64 handle through 64, 2064, 64 (across the weight kernel's 2048-row stage and back): each
    switch rebuilds the workspace and the four programs; the rebuilt plan holds the new row counts only, and every step is compared from
    the engine's own pre-step state."""
    cases = K.WALK512 if walk == 'walk512' else K.WALK64
    cfg, params, _, _, ref, a = _built(cases[0])
    for i, c in enumerate(cases):
        batch, noise = K.data(c)
        assert a.get_opt_state()['updates'] == i
        _check_step(a, ref, cfg, batch, noise)
        plan = read_plan(a)
        assert {t['M'] for t in _gemm(plan)} == {c['B'], 2 * c['B']} == {t['M'] for t in _wgrad(plan)}
        if walk == 'walk512':
            hid = [t for t in _gemm(plan) if (t['M'], t['N'], t['K']) == (2 * c['B'], 512, 512)]
            assert hid and {(t['rows'], t['kernel']) for t in hid} == {{256: (32, K_SIDE), 1024: (64, K_SIDE_BIG), 272: (16, K_GEMM16)}[c['B']]}
    assert a.get_steps() == {'updates': len(cases), 'critic': len(cases), 'actor': len(cases)}


def test_step_kinds_against_restatement():
    """Critic-only, actor-only, (False, False) and full steps in a mixed sequence: each against the restatement, the per-TrainState
    counts, the nets that do not step bitwise untouched (in _check_step), grad/* the value net's on a critic-only step."""
    cfg, params, batch, noise, ref, a = _built(K.STEP_KINDS)
    seq = [(True, False), (False, True), (False, False), (True, True), (False, True), (True, False)]
    for i, (uc, ua) in enumerate(seq):
        b, nz = K.data(K.STEP_KINDS, seed=500 + i)
        before = leaf_dict(a.get_params())
        info = _check_step(a, ref, cfg, b, nz, uc, ua)
        if (uc, ua) == (True, False):
            assert 'actor_loss' not in info and 'grad/norm' in info
        if (uc, ua) == (False, False):
            assert len(info) == 0
            for k, v in leaf_dict(a.get_params()).items():
                np.testing.assert_array_equal(v, before[k], err_msg=k)
    s = a.get_steps()
    assert s == {'updates': 6, 'critic': 3, 'actor': 3}
    # a critic-only step reports the VALUE net's gradient statistics, never the critic's
    b, nz = K.data(K.STEP_KINDS, seed=520)
    a.synchronize()
    DO.sync(ref, a)
    K.check_margins(ref, b)
    g, _ = ref.grads(b, nz, True, False)
    vs, cs = O.OracleFQL.grad_stats(g['value']), O.OracleFQL.grad_stats(g['critic'])
    _, info = a.update(b, update_critic=True, update_actor=False, noise=nz)
    for k in ('grad/max', 'grad/min', 'grad/norm'):
        assert abs(float(info[k]) - vs[k]) <= 5e-6 + 5e-5 * abs(vs[k]), (k, float(info[k]), vs[k])
        assert abs(vs[k] - cs[k]) > 1e-3 * abs(vs[k])   # (the two differ, so the check tells them apart)


def test_trajectory_100_updates_of_mixed_step_kinds_tracks_restatement():
    c = K.TRAJECTORY
    cfg, params, _, _, ref, a = _built(c)
    compared = {}
    for i in range(100):
        b, nz = K.data(c, seed=7000 + i)
        uc, ua = K.trajectory_kind(i)
        K.check_margins(ref, b, i)
        _, info = a.update(b, update_critic=uc, update_actor=ua, noise=nz, want_info=(i >= 96))
        want = ref.update(b, nz, uc, ua)
        if i < 96:
            continue
        # the last step of each kind: 96 updates both nets (all 21 scalars and the three row arrays), 97 critic and value, 98 the actor, 99 none
        info = info.to_dict()
        assert tuple(info) == info_keys(uc, ua) == tuple(want)
        compared[uc, ua] = len(want)
        for k, w in want.items():
            if k in IQLD_ROW_KEYS:
                assert np.abs(info[k] - w).max() <= 2e-3 * max(1.0, np.abs(w).max()), (i, k)
            else:
                print('trajectory', i, k, info[k], w)
                assert abs(info[k] - w) <= 2e-3 * max(1.0, abs(w)), (i, k, info[k], w)
    assert compared == {(True, True): 24, (True, False): 9, (False, True): 18, (False, False): 0}
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k
    assert a.get_steps() == {'updates': 100, 'critic': ref.counts['critic'], 'actor': ref.counts['actor']}


def test_total_loss_matches_and_changes_no_state():
    cfg, params, batch, noise, ref, a = _built(K.STEP_KINDS)
    a.update(batch, noise=noise)
    a.synchronize()
    before, opt_before, info_before = leaf_dict(a.get_params()), a.get_opt_state(), a.read_info()
    rows_before = [a._read_rows(i, 64) for i in range(3)]
    DO.sync(ref, a)
    b2, n2 = K.data(K.STEP_KINDS, seed=530)
    K.check_margins(ref, b2)
    loss, info = a.total_loss(b2, grad_params=None, noise=n2)
    want_loss, want = ref.total_loss(b2, n2)
    assert abs(loss - want_loss) <= 5e-6 + 5e-5 * abs(want_loss)
    assert tuple(info) == info_keys(True, True, grads=False) == tuple(want)
    for k, w in want.items():
        np.testing.assert_allclose(np.asarray(info[k]), np.asarray(w), rtol=5e-5, atol=5e-6, err_msg=k)
    a.synchronize()
    for k, v in leaf_dict(a.get_params()).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)
    opt = a.get_opt_state()
    assert [opt[k] for k in ('count', 'step', 'actor_count', 'updates')] == [opt_before[k] for k in ('count', 'step', 'actor_count', 'updates')]
    for part in ('mu', 'nu'):
        for k, v in leaf_dict(opt[part]).items():
            np.testing.assert_array_equal(v, leaf_dict(opt_before[part])[k])
    assert a.read_info() == info_before
    for i in range(3):
        np.testing.assert_array_equal(a._read_rows(i, 64), rows_before[i])


@pytest.mark.parametrize('uc,ua', KINDS)
def test_aql_and_graph_updates_bitwise_over_20_steps(uc, ua):
    import torch
    cfg, params, _, _, _, a = _built(K.STEP_KINDS)
    b = _agent(cfg, params=params)
    ds = O.make_synthetic_dataset(512, OD, AD, seed=5)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for _ in range(20):
        a.update_from_dataset(update_critic=uc, update_actor=ua)
        b.update_from_dataset(stream=s.cuda_stream, update_critic=uc, update_actor=ua)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.get_steps() == {'updates': 20, 'critic': 20 * uc, 'actor': 20 * ua}
    assert a.read_info() == b.read_info()


def test_update_from_dataset_explicit_rows_equals_update():
    cfg, params, _, noise, _, a = _built(K.STEP_KINDS)
    b = _agent(cfg, params=params)
    ds = O.make_synthetic_dataset(512, OD, AD, seed=4)
    idx = np.random.default_rng(4).integers(0, 512, size=64)
    a.upload_dataset(ds)
    for uc, ua in KINDS:
        a.update_from_dataset(idxs=idx, noise=noise, update_critic=uc, update_actor=ua)
        b.update({k: ds[k][idx] for k in ds}, update_critic=uc, update_actor=ua, noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg, params, batch, noise, _, a = _built(K.STEP_KINDS)
    for uc, ua in [(True, False), (True, True), (False, False), (False, True), (True, False)]:
        a.update(batch, update_critic=uc, update_actor=ua, noise=noise)
    a.synchronize()
    sd = checkpoint.to_state_dict(a)
    assert set(sd) == {'rng', 'critic', 'target_critic', 'value', 'actor'}
    assert all(set(sd[f]) == {'step', 'params', 'opt_state'} for f in ('critic', 'target_critic', 'value', 'actor'))
    assert sd['target_critic']['opt_state'] is None and int(sd['target_critic']['step']) == 1
    assert int(sd['critic']['opt_state']['0']['count']) == 3 == int(sd['value']['opt_state']['0']['count']) and int(sd['critic']['step']) == 4
    assert int(sd['actor']['opt_state']['0']['count']) == 2 and set(sd['actor']['params']) == {'Dense_0', 'Embed_0', 'MLP_0'}
    checkpoint.save_agent(a, str(tmp_path), 5)
    b = _agent(cfg)   # (the same create seed keys the device RNG: the engine's own draws continue below)
    checkpoint.restore_agent(b, str(tmp_path), 5)
    _same_state(a, b)
    ds = O.make_synthetic_dataset(512, OD, AD, seed=6)
    for x in (a, b):   # the engine's own draws continue where the saved agent's would (same seed, same update counter)
        x.upload_dataset(ds)
        x.update_from_dataset()
        x.synchronize()
    _same_state(a, b)


def test_fql_and_iqld_interleaved_end_where_they_end_alone():
    import fql_amd
    from tests.util import make_problem
    fcfg, ds, fbatch, fnoise = make_problem(OD, AD, 64, (64,) * 4, seed=7)
    cfg, params, batch, noise, _, d_alone = _built(K.STEP_KINDS)
    d_mix = _agent(cfg, params=params)

    def fql():
        return fql_amd.FQLAgent.create(1, fbatch['observations'][:1], fbatch['actions'][:1], fcfg)
    f_alone, f_mix = fql(), fql()
    kinds = [(True, True), (True, False), (False, True), (True, True), (False, False)]
    for _ in range(5):
        f_alone.update(fbatch, noise=fnoise)
    for uc, ua in kinds:
        d_alone.update(batch, update_critic=uc, update_actor=ua, noise=noise)
    for uc, ua in kinds:
        f_mix.update(fbatch, noise=fnoise)
        d_mix.update(batch, update_critic=uc, update_actor=ua, noise=noise)
    for x in (f_alone, d_alone, f_mix, d_mix):
        x.synchronize()
    from tests.util import assert_same_state
    assert_same_state(f_alone, f_mix)
    _same_state(d_alone, d_mix)


@pytest.fixture(scope='module')
def sampler():
    """One agent and restatement for the sampler tests.  The head is scaled by 2 so that the velocities are O(2) and many coordinates
    leave [-1, 1]; tests/test_iqld_cpu.py::test_fp32_rounding_of_the_cfg_sampler shows fp32 numpy within 1.2e-5 of fp64 (8.8e-6 measured at
    cfg 3, 1.9e-6 at cfg 0) on these very inputs at this scale: inside the 2e-5 bound, by a factor of about 2 at cfg 3."""
    cfg, params, _ = K.sampler_problem()
    return _agent(cfg, params=params), DO.OracleIQLD(params, cfg, OD, AD, np.float64)


@pytest.mark.parametrize('n', [1, 5, 16, 37, 256, 2049])
def test_sample_actions_match_oracle_and_single_calls(sampler, n):
    a, ref = sampler
    obs, sn = K.sampler_inputs(n)
    for cfg_scale in (0.0, 1.0, 3.0):
        got = a.sample_actions(obs, noises=sn, temperature=0.3, cfg=cfg_scale, o=0.5)   # temperature and o: accepted and not read
        want = ref.sample_actions(obs, sn, cfg_scale)
        assert got.shape == ((AD,) if n == 1 else (n, AD)) == want.shape
        print('n', n, 'cfg', cfg_scale, 'max err', float(np.abs(got - want).max()), 'saturated', int((np.abs(want) == 1).sum()))
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
        assert (np.abs(want) == 1).any() and (np.abs(got) <= 1).all()
        for j in sorted({0, n // 2, n - 1}):   # row j of the batched call is the single-observation call on the same noise
            one = a.sample_actions(obs[j], noises=sn[j], cfg=cfg_scale)
            assert one.shape == (AD,)
            np.testing.assert_array_equal(one, got.reshape(n, AD)[j])
    assert a.sample_actions(obs[:1], noises=sn[:1]).shape == (AD,)   # [1, od] -> [act]: the reference's squeeze
    if n == 5:   # engine RNG: a seed fixes the draw
        np.testing.assert_array_equal(a.sample_actions(obs, seed=7, cfg=1.5), a.sample_actions(obs, seed=7, cfg=1.5))


@pytest.fixture(scope='module')
def sampler512():
    """The sampler at the humanoidmaze shape: obs 69, act 21 (fql_iqld_layer0_kernel and fql_iqld_cfg_step_kernel stride the action rows
    by the padded width 32), hidden 512.  The head is scaled by K.SAMPLER512_HEAD_SCALE, where
    tests/test_iqld_cpu.py::test_fp32_rounding_of_the_cfg_sampler_at_hidden_512 shows fp32 numpy within 5e-6 of fp64 on these inputs."""
    c = K.SAMPLER512
    cfg, params, _ = K.sampler_problem(K.SAMPLER512_HEAD_SCALE, c)
    return _agent(cfg, c['od'], c['ad'], params=params), DO.OracleIQLD(params, cfg, c['od'], c['ad'], np.float64)


@pytest.mark.parametrize('n', K.SAMPLER512_N)
def test_sample_actions_at_hidden_512_and_padded_action_width_32(sampler512, n):
    """n = 1, 37 and 2049 (one row past the 2048-observation chunk), cfg 0 and 3, against the restatement at 2e-5; the clip is reached;
    rows 0, n // 2 and n - 1 are bitwise the single-observation calls."""
    a, ref = sampler512
    od, ad = K.SAMPLER512['od'], K.SAMPLER512['ad']
    obs, sn = K.sampler_inputs(n, od, ad)
    for cfg_scale in (0.0, 3.0):
        got = a.sample_actions(obs, noises=sn, cfg=cfg_scale)
        want = ref.sample_actions(obs, sn, cfg_scale)
        assert got.shape == ((ad,) if n == 1 else (n, ad)) == want.shape
        print('n', n, 'cfg', cfg_scale, 'max err', float(np.abs(got - want).max()), 'saturated', int((np.abs(want) == 1).sum()))
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
        assert (np.abs(want) == 1).any() and (np.abs(got) == 1).any() and (np.abs(got) <= 1).all()
        for j in sorted({0, n // 2, n - 1}):
            one = a.sample_actions(obs[j], noises=sn[j], cfg=cfg_scale)
            assert one.shape == (ad,)
            np.testing.assert_array_equal(one, got.reshape(n, ad)[j])


def test_cfg_zero_ignores_the_positive_embedding_row(sampler):
    a, _ = sampler
    obs, sn = K.sampler_inputs(16)
    base0, base1 = a.sample_actions(obs, noises=sn, cfg=0.0), a.sample_actions(obs, noises=sn, cfg=1.0)
    p = a.get_params()
    keep = p['actor']['Embed_0']['embedding'].copy()
    emb = keep.copy()
    emb[1] += 1.0
    a.set_params({'actor': {'Embed_0': {'embedding': emb}}})
    try:
        np.testing.assert_array_equal(a.sample_actions(obs, noises=sn, cfg=0.0), base0)
        assert np.abs(a.sample_actions(obs, noises=sn, cfg=1.0) - base1).max() > 1e-3
    finally:
        a.set_params({'actor': {'Embed_0': {'embedding': keep}}})


def test_refusals_and_info_width():
    import fql_amd
    import fql_amd.bc
    import fql_amd.iql
    from fql_amd import _cabi
    from tests.util import make_problem
    lib = _cabi.load()
    cfg, params, batch, noise, _, a = _built(K.STEP_KINDS)
    h = a._h
    E = _cabi.FQL_E_STATE
    f = lambda arr: arr.ctypes.data_as(C.c_void_p)   # noqa: E731
    ob, ac = batch['observations'], batch['actions']
    r = np.zeros(64, np.float32)
    buf = (C.c_float * 32)()
    i64 = (C.c_int64 * 3)()
    sz = (C.c_size_t * 2)()
    assert lib.fql_num_info(h) == 21
    assert [lib.fql_handle_info_name(h, i).decode() for i in range(21)] == list(IQLD_INFO_KEYS)
    st, st2 = C.c_void_p(1), C.c_void_p(2)
    u8 = np.zeros(64, np.uint8)
    keys = (C.c_uint32 * 20)()
    nz = _cabi.FqlNoise()
    # every foreign entry point on an IQL-diffusion handle
    foreign = [
        lambda: lib.fql_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None),
        lambda: lib.fql_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None),
        lambda: lib.fql_update_from_dataset(h, None, 64, 0, 0, None, None, None),
        lambda: lib.fql_sample_actions(h, f(ob), 1, None, 0, buf, None),
        lambda: lib.fql_flow_actions(h, f(ob), f(ac), 1, buf, None),
        lambda: lib.fql_update_begin(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None),
        lambda: lib.fql_update_end(h, None, None),
        lambda: lib.fql_update_begin_split(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, st, st2),
        lambda: lib.fql_update_end_split(h, None, st, st2),
        lambda: lib.fql_update_from_dataset_begin(h, None, 64, 0, 0, None, None),
        lambda: lib.fql_update_from_dataset_begin_split(h, None, 64, 0, 0, None, st, st2),
        lambda: lib.fql_dataset_add_frames(h, f(u8), f(u8), f(ac), 0.0, 1.0),
        lambda: lib.fql_replay_add_frames(h, f(u8), f(u8), f(ac), 0.0, 1.0),
        lambda: lib.fql_dataset_upload_frames(h, 1, f(u8), f(u8), f(ac), f(r), f(r), f(r), 1, 0.0),
        lambda: lib.fql_update_from_frames(h, None, None, 64, 0, 0, None, None, None),
        lambda: lib.fql_replay_add(h, f(ob), f(ac), 0.0, 1.0, f(ob)),
        lambda: lib.fql_replay_create(h, 128),
        lambda: lib.fql_replay_size(h, i64, i64),
        lambda: lib.fql_update_balanced(h, None, None, None, 64, None, None, None),
        lambda: lib.fql_info_wait(h, 0, buf),
        lambda: lib.fql_read_info(h, buf),
        lambda: lib.fql_grad_buckets(h, sz, sz),
        lambda: lib.fql_noise_from_jax_keys(h, keys, 0, 64, C.byref(nz), None),
        lambda: lib.fql_set_step(h, 3, 4),   # (one count per TrainState: fql_iqld_set_steps)
        lambda: lib.fql_set_grad_scale(h, 0.5),
        lambda: lib.fql_rebrac_update(h, f(ob), f(ac), f(r), f(r), f(ob), f(ac), 64, None, 1, None, None),
        lambda: lib.fql_rebrac_update_from_dataset(h, None, 64, 0, 0, None, 1, None, None),
        lambda: lib.fql_rebrac_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), f(ac), 64, None, 1, None, None, None),
        lambda: lib.fql_rebrac_sample_actions(h, f(ob), 1, None, 0, 1.0, buf, None),
        lambda: lib.fql_rebrac_stats(h, 1, i64, i64),
        lambda: lib.fql_sac_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None),
        lambda: lib.fql_sac_update_from_dataset(h, None, 64, 0, 0, None, None, None),
        lambda: lib.fql_sac_update_balanced(h, None, None, 64, None, None, None),
        lambda: lib.fql_sac_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None),
        lambda: lib.fql_sac_sample_actions(h, f(ob), 1, None, 0, 1.0, buf, None),
        lambda: lib.fql_sac_stats(h, i64, i64),
        lambda: lib.fql_iql_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None),
        lambda: lib.fql_iql_update_from_dataset(h, None, 64, 0, 0, None, None, None),
        lambda: lib.fql_iql_total_loss(h, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None),
        lambda: lib.fql_iql_sample_actions(h, f(ob), 1, None, 0, 1.0, buf, None),
        lambda: lib.fql_iql_stats(h, i64, i64),
        lambda: lib.fql_bc_update(h, f(ob), f(ac), 64, None, None, None),
        lambda: lib.fql_bc_update_from_dataset(h, None, 64, 0, 0, None, None, None),
        lambda: lib.fql_bc_policy_loss(h, f(ob), f(ac), 64, None, None, None),
        lambda: lib.fql_bc_sample_actions(h, f(ob), 1, None, 0, buf, None),
        lambda: lib.fql_bc_stats(h, i64, i64, i64),
    ]
    for i, call in enumerate(foreign):
        assert call() == E, i
    assert lib.fql_read_info(h, buf) == E and b'21 infos' in lib.fql_last_error(h) and b'IQL-diffusion handle' in lib.fql_last_error(h)
    grp = C.c_void_p()
    hs = (C.c_void_p * 1)(h)
    assert lib.fql_group_create(hs, 1, C.byref(grp)) == E
    # every fql_iqld_* entry point on an FQL, an IQL and a BC handle
    fcfg, _, fbatch, _ = make_problem(OD, AD, 64, (64,) * 4, seed=7)
    ex = (fbatch['observations'][:1], fbatch['actions'][:1])
    others = [fql_amd.FQLAgent.create(1, *ex, fcfg), fql_amd.IQLAgent.create(1, *ex, dict(fql_amd.iql.get_config(), batch_size=64)),
              fql_amd.BCAgent.create(1, *ex, dict(fql_amd.bc.get_config(), batch_size=64))]
    for x in others:
        g = x._h
        assert lib.fql_iqld_update(g, f(ob), f(ac), f(r), f(r), f(ob), 64, None, 1, 1, None, None) == E
        assert lib.fql_iqld_update_from_dataset(g, None, 64, 0, 0, None, 1, 1, None, None) == E
        assert lib.fql_iqld_total_loss(g, f(ob), f(ac), f(r), f(r), f(ob), 64, None, None, None, None) == E
        assert lib.fql_iqld_sample_actions(g, f(ob), 1, None, 0, 1.0, buf, None) == E
        assert lib.fql_iqld_read_rows(g, 0, buf, 64) == E
        assert lib.fql_iqld_get_steps(g, i64) == E and lib.fql_iqld_set_steps(g, i64) == E
        assert lib.fql_iqld_stats(g, 1, 1, i64, i64, i64) == E
        assert b'needs an IQL-diffusion handle' in lib.fql_last_error(g)
    # create-time refusals: FQL_E_INVALID with a message naming the field
    c = _cabi.FqlConfig(); lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim = OD, AD
    dc = _cabi.FqlIqldConfig(); lib.fql_iqld_default_config(C.byref(dc))
    assert (dc.optimal_var, dc.target_extraction, dc.denoise_steps, dc.opt_decay_schedule) == (1, 1, 16, 0)
    assert abs(dc.awr_temperature - 0.1) < 1e-8 and abs(dc.softmax_beta - 3.0) < 1e-7 and abs(dc.expectile - 0.9) < 1e-7
    out = C.c_void_p()
    for field in ('encoder', 'precision'):
        c2 = _cabi.FqlConfig.from_buffer_copy(c)
        setattr(c2, field, 2 if field == 'precision' else 1)
        assert lib.fql_iqld_create(C.byref(c2), C.byref(dc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
        assert field.encode() in lib.fql_last_error(None)
    for field, val in (('optimal_var', 3), ('optimal_var', 4), ('opt_decay_schedule', 1)):
        d2 = _cabi.FqlIqldConfig.from_buffer_copy(dc)
        setattr(d2, field, val)
        assert lib.fql_iqld_create(C.byref(c), C.byref(d2), 0, C.byref(out)) == _cabi.FQL_E_INVALID
        assert field.encode() in lib.fql_last_error(None)
    ex0 = (np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32))
    for kw in (dict(optimal_var='softmax'), dict(optimal_var='sampled_adv_softmax'), dict(opt_decay_schedule='cosine'),
               dict(encoder='impala_small'), dict(precision='bf16x3'), dict(activation='relu')):
        with pytest.raises(NotImplementedError):
            fql_amd.agents['iql_diffusion'].create(0, *ex0, dict(cfg, **kw))
    for method in ('update_begin', 'update_end', 'grad_buckets', 'create_replay_buffer', 'update_balanced', 'compute_flow_actions'):
        with pytest.raises(NotImplementedError):
            getattr(a, method)()
    # noise: any pointer but x0 / t is FQL_E_INVALID; an off-grid t too
    bad = _cabi.FqlNoise(f(noise['x0']), None, None, None, None)
    assert lib.fql_iqld_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, C.byref(bad), 1, 1, None, None) == _cabi.FQL_E_INVALID
    off = np.full(64, 0.3, np.float32)
    bad = _cabi.FqlNoise(None, f(noise['x0']), f(off), None, None)
    assert lib.fql_iqld_update(h, f(ob), f(ac), f(r), f(r), f(ob), 64, C.byref(bad), 1, 1, None, None) == _cabi.FQL_E_INVALID
    with pytest.raises(ValueError):
        a.update(batch, noise={'x0': noise['x0'], 'eps1': noise['x0']})
    assert a.get_steps() == {'updates': 0, 'critic': 0, 'actor': 0}
    # exactly 21 floats: the guard values after them stay
    a.update(batch, noise=noise)
    for i in range(32):
        buf[i] = -7.0
    assert lib.fql_read_info_n(h, buf, 32) == 0
    assert all(buf[i] == -7.0 for i in range(21, 32)) and all(buf[i] != -7.0 for i in range(21))
    assert lib.fql_read_info_n(h, buf, 20) == _cabi.FQL_E_INVALID
    t = C.c_uint64()
    assert lib.fql_info_enqueue(h, None, C.byref(t)) == 0
    for i in range(32):
        buf[i] = -7.0
    assert lib.fql_info_wait_n(h, t.value, buf, 32) == 0
    assert all(buf[i] == -7.0 for i in range(21, 32)) and buf[7] == pytest.approx(a.read_info()['actor_loss'])
    assert lib.fql_iqld_read_rows(h, 6, buf, 64) == _cabi.FQL_E_INVALID and lib.fql_iqld_read_rows(h, 0, buf, 32) == _cabi.FQL_E_INVALID
    # working on the handle
    S, nl = 16, 5
    for uc, ua in [(1, 1), (1, 0), (0, 1), (0, 0)]:
        la, ma, ls = a.iqld_stats(uc, ua)
        assert la > 0 and ls == 4 + S * (nl + 1) and (ma > 0) == bool(uc or ua)
    assert a.iqld_stats(0, 0)[0] == 1 and a.iqld_stats(1, 1)[0] > a.iqld_stats(1, 0)[0]
    assert a.stats()['param_count'] == sum(int(np.prod(s)) for _, s in a.leaves())
