"""GPU: FQL at hidden widths that are no multiple of 16, against the fp64 oracle on identical params, batch and noise.

The engine pads every hidden width to a multiple of 16 and many kernels carry code that runs only when out < out_p: the LayerNorm
prologue of the 16-row Dense kernel and the LayerNorm statistics of the 32- and 64-row tile bodies (`ln_width`, clamped indices, masked
terms), LayerNorm-backward's masked sums and zeroed dgamma / dbeta, the strided Segment copies behind get_params / set_params /
checkpoints, the Glorot initialiser, and every path choice made on the padded size.  tests/padded_cases.py holds the cases; each asserts
from the engine's plan (fql_debug_plan, tests/util.py read_plan) where it runs before and after it compares numbers with bounds that are
those of the unpadded cases, unchanged (a padded width does no more arithmetic than its out_p-wide neighbour).

Where the cases run, read from want64 / side_ri / build_chain_weights in fql_amd/csrc/fql_engine.hip and confirmed by the plans:
  * every case: the 16-row Dense kernel with a padded N and K (and, with LayerNorm, its ln_width prologue); LayerNorm-backward and the
    weight gradients as riders of fql_side_kernel launches.
  * w250, w500 (B 64, out_p 256 / 512): no Euler chain although out_p is a chain width (out != out_p); hidden layers of the side lanes on
    fql_side_kernel's 32-row tiles with LayerNorm partial sums over 250 / 500 valid columns; w500 the lean OP_DGRAD0 at K 512.
  * w1000: fql_gemm16_kernel<true> at K 1008.
  * w300_b256 and w300_b1024 do NOT reach the 32- and 64-row tile bodies they were proposed for: those bodies take N % 64 == 0 and
    K % 64 == 0 only (want64), and out_p = 304 = 4 x 64 + 48.  At hidden 300 every GEMM runs on the 16-row kernel, at M 256 and at M 1024,
    and the side launches carry the weight gradients (N 304) and LayerNorm-backward (width 300 of 304) alone; the two cases are kept for
    exactly that and assert it.  The tile bodies are reached with width < out_p at out_p 256 and 512: the 32-row body by w250 and w500,
    fql_side_big_kernel's 64-row body by w250_b1024 ((250, 250) at B 1024), the one case added to those asked for.
  * bf16x3: the split weight-gradient body in every case, fql_side_split_kernel's 32-row tiles at w500.

The Euler chain kernels (fql_chain_kernel<256 / 512>) have no width operand and cannot run at a padded width: build_chain_weights admits
them for out == out_p only, which w250 and w500 pin.

Measured against the fp64 oracle (worst |g_gpu - g_ref| / max|g_ref| over the leaves and the four updates; worst info delta / max(1, |ref|));
figures of one run, not bounds:
  case          fp32 gradient  fp32 info  bf16x3 gradient  bf16x3 info
  w50           6.3e-07        2.0e-07    7.0e-06          9.7e-07
  w33_100_17    9.4e-07        2.6e-07
  w50_actor_ln  8.9e-07        3.5e-07
  w100_no_ln    4.2e-07        2.0e-07
  w250          1.7e-06        4.1e-07
  w500          1.9e-06        5.2e-07    2.1e-05          9.5e-06
  w300_b256     1.5e-06        6.0e-07    3.8e-06          3.0e-07
  w300_b1024    6.9e-07        3.2e-07
  w1000         1.2e-06        8.7e-07
  w250_b1024    7.1e-07        2.2e-07
(bf16x3 is one update; the fp32 bounds are 2e-5 and 5e-5, the bf16x3 bounds 1e-4: the padded paths sit where their unpadded neighbours do.)
No case failed and no kernel changed.

A kernel that stops masking is caught.  In a scratch build whose LayerNorm-backward row pass stored dZ's padding columns unmasked (the same
stores, other values; lnbwd_body's `k4 + e < T.width ? ... : 0`), every case with a LayerNorm failed: the four-update test at the first
step on grad/norm (0.07 % to 0.7 % off at bounds of 5e-5) or, where that held, at a later step on critic_loss or a leaf's gradient; the
restore test of all three cases at the first common update; bf16x3 at w50 with 7e-4 against 1e-4.  w100_no_ln, which has no LayerNorm, passed.
"""
import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import padded_cases as PC
from tests.util import (BF16X3_BOUND, K_GEMM16, K_GEMM16_EULER, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, K_SIDE_SPLIT, OP_CHAIN, OP_DGRAD0,
                        OP_GEMM64, assert_info_close, assert_initialised_like_the_reference, assert_same_state, assert_step_matches,
                        assert_total_loss_matches, bf16x3_update_errors, leaf_dict, make_problem, plan_gemm, plan_ln, plan_wgrad,
                        print_plan, read_plan, sync_restatement)

pytestmark = pytest.mark.gpu

_FROZEN = {}    # id -> tests.padded_cases.FrozenRef of the first update: computed once, shared by both precisions, never written


def _agent(cid, seed=0, **cfgkw):
    import fql_amd
    cfg, ds, batch, noise, params = PC.fql_problem(cid, **cfgkw)
    agent = fql_amd.FQLAgent.create(seed, batch['observations'][:1], batch['actions'][:1], cfg)
    agent.set_params(params)
    return cfg, ds, batch, noise, params, agent


def _frozen(cid, cfg, params, batch, noise):
    if cid not in _FROZEN:
        od, ad = PC.FQL_CASES[cid][:2]
        _FROZEN[cid] = PC.FrozenRef(params, _oracle_cfg(cfg), od, ad, batch, noise)
    return _FROZEN[cid]


def _oracle_cfg(cfg):
    ocfg = dict(cfg)
    ocfg['precision'] = 'fp32'     # (the oracle is fp64 whatever the engine's mode)
    return ocfg


# ---- where a case runs ----------------------------------------------------------------------------------------------------------------
def _padded(cid):
    return {PC.pad16(w) for w in PC.FQL_CASES[cid][3] if w % 16}


def _families(cid, plan):
    """The kernel families with a width / ln_width operand that this plan runs on a padded width of the case."""
    pw = _padded(cid)
    on = lambda t: t['N'] in pw or t['K'] in pw   # noqa: E731
    fam = set()
    if [t for t in plan_gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if on(t) and t['rows'] == 16]:
        fam.add('gemm16')
    if [t for t in plan_gemm(plan, (K_GEMM16_KBIG,)) if on(t) and t['K'] > 512]:
        fam.add('kbig')
    if [t for t in plan_gemm(plan, (K_SIDE,)) if on(t) and t['rows'] == 32]:
        fam.add('side32')
    if [t for t in plan_gemm(plan, (K_SIDE_BIG,)) if on(t) and t['rows'] == 64]:
        fam.add('side64')
    if [t for t in plan_gemm(plan, (K_SIDE_SPLIT,)) if on(t) and t['rows'] == 32]:
        fam.add('side32_split')
    if plan_ln(plan) and PC.FQL_CASES[cid][4].get('layer_norm', True):
        fam.add('lnbwd')
    return fam


def _no_chain(plan):
    assert all(L['chain'] is None and L['type'] != OP_CHAIN for L in plan)


def _riders_on_side_launches(plan, cid, split=False):
    """The weight gradients (every padded N among them) and LayerNorm-backward ride in side-lane launches, on the body of the mode."""
    B = PC.FQL_CASES[cid][2]
    w = plan_wgrad(plan)
    assert w and _padded(cid) <= {t['N'] for t in w} and {t['split'] for t in w} == {1 if split else 0}
    assert B in {t['M'] for t in w}
    kernels = (K_SIDE_SPLIT,) if split else (K_SIDE, K_SIDE_BIG)
    assert all(L['kernel'] in kernels and L['type'] == OP_GEMM64 for L in plan if L['wgrad'] or L['ln'])


def _only_16_row_tiles(plan):
    assert not [t for t in plan_gemm(plan) if t['rows'] != 16]
    assert all(L['kernel'] != K_SIDE_BIG for L in plan)


def _p_small(cid, plan, fam):
    assert 'gemm16' in fam
    _no_chain(plan)


def _p_w250(cid, plan, fam):
    _no_chain(plan)                                       # out_p 256 is a chain width; out 250 is not
    assert {'gemm16', 'side32', 'lnbwd'} <= fam


def _p_w500(cid, plan, fam):
    _no_chain(plan)
    assert {'gemm16', 'side32', 'lnbwd'} <= fam
    assert [L for L in plan if L['type'] == OP_DGRAD0]    # K = out_p = 512 with 500 valid
    assert 500 in PC.FQL_CASES[cid][3]


def _p_w300_b256(cid, plan, fam):
    """K_SIDE launches at M 256 with LayerNorm-backward over 300 of 304 columns and the N 304 weight gradients; no 32-row GEMM tile:
    304 % 64 != 0 (see the module's docstring)."""
    assert [L for L in plan if L['kernel'] == K_SIDE and L['ln'] and 256 in L['ln']]
    assert [L for L in plan if L['kernel'] == K_SIDE and [t for t in L['wgrad'] if t['N'] == 304]]
    _only_16_row_tiles(plan)
    assert {'gemm16', 'lnbwd'} <= fam


def _p_w300_b1024(cid, plan, fam):
    """The 16-row kernel at M 1024 and N 304; no 64-row tile: 304 % 64 != 0 (see the module's docstring)."""
    assert [t for t in plan_gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if t['M'] == 1024 and t['N'] == 304 and t['K'] == 304]
    _only_16_row_tiles(plan)
    assert {'gemm16', 'lnbwd'} <= fam


def _p_w250_b1024(cid, plan, fam):
    big = [t for t in plan_gemm(plan, (K_SIDE_BIG,)) if t['rows'] == 64 and t['M'] % 1024 == 0 and (t['N'] == 256 or t['K'] == 256)]
    assert big and 'side64' in fam


def _p_w1000(cid, plan, fam):
    assert [t for t in plan_gemm(plan, (K_GEMM16_KBIG,)) if t['K'] == 1008]
    assert [t for t in plan_gemm(plan, (K_GEMM16_KBIG,)) if t['K'] == 1008 and t['N'] == 1008]
    assert 'kbig' in fam


PROPERTY = {'w50': _p_small, 'w33_100_17': _p_small, 'w50_actor_ln': _p_small, 'w100_no_ln': _p_small, 'w250': _p_w250, 'w500': _p_w500,
            'w300_b256': _p_w300_b256, 'w300_b1024': _p_w300_b1024, 'w1000': _p_w1000, 'w250_b1024': _p_w250_b1024}


def _assert_on_path(cid, agent, split=False):
    plan = read_plan(agent)
    fam = _families(cid, plan)
    print_plan(cid, plan)
    print(cid, 'families on a padded width:', sorted(fam))
    _riders_on_side_launches(plan, cid, split)
    if not split:
        PROPERTY[cid](cid, plan, fam)
    return fam


# ---- 1. one update and then three more ------------------------------------------------------------------------------------------------
def _later_step_matches(agent, ref, batch, noise):
    """One update past the first, on both sides from the engine's state: the 13 infos at assert_step_matches' bound, and every leaf's
    gradient, recovered from Adam's first moment (mu' = 0.9 mu + 0.1 g), within 2e-5 of the leaf's largest entry.  The recovery costs two
    fp32 roundings of mu scaled by 1 / 0.1: 2 x 6e-8 x 10 of the moment's largest entry is allowed for it."""
    pre = leaf_dict(agent.get_opt_state()['mu'])
    sync_restatement(ref, agent)
    count = ref.count
    _, _, g_ref = ref.grads(batch, noise)
    _, info = agent.update(batch, noise=noise)
    _, info_r = ref.update(batch, noise)
    assert_info_close(info, info_r, rtol=5e-5, atol=5e-6)
    opt = agent.get_opt_state()
    assert opt['count'] == count + 1 and opt['step'] == count + 2
    post = leaf_dict(opt['mu'])
    worst = (0.0, None)
    for p, g in leaf_dict(g_ref).items():
        scale = np.abs(g).max()
        got = (post[p].astype(np.float64) - 0.9 * pre[p].astype(np.float64)) / 0.1
        err = np.abs(got - g).max()
        worst = max(worst, (err / max(scale, 1e-30), p))
        assert err <= 2e-5 * scale + 1e-9 + 1.2e-6 * np.abs(post[p]).max(), (p, err, scale)
    delta = max(abs(float(info[k]) - float(info_r[k])) / max(1.0, abs(float(info_r[k]))) for k in O.INFO_KEYS)
    return worst, delta


@pytest.mark.parametrize('cid', list(PC.FQL_CASES))
def test_four_updates_match_oracle_on_the_named_path(cid):
    od, ad = PC.FQL_CASES[cid][:2]
    cfg, ds, batch, noise, params, agent = _agent(cid)
    fam = _assert_on_path(cid, agent)
    ref = _frozen(cid, cfg, params, batch, noise)
    if cid in ('w50', 'w500'):
        assert_total_loss_matches(agent, ref, params, batch, noise)
    worst = assert_step_matches(agent, ref, cfg, batch, noise)
    info, info_r = agent.read_info(), ref.update(batch, noise)[1]
    delta = max(abs(float(info[k]) - float(info_r[k])) / max(1.0, abs(float(info_r[k]))) for k in O.INFO_KEYS)
    live = O.OracleFQL(params, _oracle_cfg(cfg), od, ad, np.float64)
    for step in (1, 2, 3):
        b, nz = PC.later_step(cid, ds, step)
        w, d = _later_step_matches(agent, live, b, nz)
        worst, delta = max(worst, w), max(delta, d)
    print(f'{cid} fp32: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info delta {delta:.3e}')
    assert _families(cid, read_plan(agent)) == fam       # reading the plan changed no launch: the same plan after the updates
    agent.close()


def test_every_family_with_a_width_operand_runs_at_a_padded_width():
    """Over the whole table: the 16-row Dense kernel, fql_side_kernel's 32-row tiles, fql_side_big_kernel's 64-row tiles, the K > 512
    kernels and LayerNorm-backward each appear at least once with width < out_p."""
    seen = {}
    for cid in PC.FQL_CASES:
        agent = _agent(cid)[-1]
        seen[cid] = _families(cid, read_plan(agent))
        agent.close()
    print({c: sorted(f) for c, f in seen.items()})
    assert {'gemm16', 'side32', 'side64', 'kbig', 'lnbwd'} <= set().union(*seen.values())
    assert 'side64' in seen['w250_b1024'] and 'side64' not in seen['w300_b1024'] and 'side32' not in seen['w300_b256']


# ---- 2. padding stays zero ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ['w50', 'w500', 'w50_actor_ln'])
def test_restore_into_a_fresh_engine_continues_bitwise(cid, tmp_path):
    """`a` takes 6 updates on device-drawn rows; its parameters, Adam moments and counters move through a checkpoint into a fresh agent
    `b` of another seed, whose padding columns are the initial zero while a's are whatever six updates left (get_params copies the real
    region only).  Three updates on identical explicit rows and noise: equal infos and bitwise equal state after each, which any drift
    in a's padding (a gradient kernel that writes a non-zero there, moved on by Adam) breaks."""
    import fql_amd
    from fql_amd import checkpoint
    cfg, ds, batch, noise, params, a = _agent(cid)
    a.upload_dataset(ds)
    for _ in range(6):
        a.update_from_dataset()
    a.synchronize()
    assert a.get_opt_state()['count'] == 6
    checkpoint.save_agent(a, str(tmp_path), 6)
    b = fql_amd.FQLAgent.create(99, batch['observations'][:1], batch['actions'][:1], cfg)
    b = checkpoint.restore_agent(b, str(tmp_path), 6)
    assert_same_state(a, b)
    for step in (1, 2, 3):
        rows, nz = PC.later_step(cid, ds, step)
        _, ia = a.update(rows, noise=nz)
        _, ib = b.update(rows, noise=nz)
        assert {k: float(v) for k, v in ia.items()} == {k: float(v) for k, v in ib.items()}, step
        assert_same_state(a, b)
    assert a.get_opt_state()['count'] == 9
    a.close(); b.close()


# ---- 3. bf16x3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ['w50', 'w500', 'w300_b256'])
def test_bf16x3_update_within_the_split_bound(cid):
    cfg, ds, batch, noise, params, agent = _agent(cid, precision='bf16x3')
    fam = _assert_on_path(cid, agent, split=True)
    assert all(L['kernel'] == K_SIDE_SPLIT for L in read_plan(agent) if L['type'] == OP_GEMM64)
    if cid == 'w500':
        assert 'side32_split' in fam
    worst, deltas = bf16x3_update_errors(agent, _frozen(cid, cfg, params, batch, noise), batch, noise)
    print(f'{cid} bf16x3: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info delta {max(deltas.values()):.3e}')
    assert max(deltas.values()) <= BF16X3_BOUND, deltas
    assert worst[0] <= BF16X3_BOUND, worst
    agent.close()


# ---- 4. forward-only paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ['w50', 'w500'])
def test_sample_and_flow_actions_across_the_row_chunk(cid):
    """tests/test_gpu_shapes.py's check and tolerances at n = 1, 37 and 4097; row j of a call is bitwise the single-row call."""
    od, ad = PC.FQL_CASES[cid][:2]
    cfg, ds, batch, noise, params, agent = _agent(cid)
    ref = O.OracleFQL(params, _oracle_cfg(cfg), od, ad, np.float64)
    rng = np.random.default_rng(11)
    obs = rng.standard_normal((4097, od)).astype(np.float32)
    z = rng.standard_normal((4097, ad)).astype(np.float32)
    for n in (1, 37, 4097):
        got_s, got_f = agent.sample_actions(obs[:n], noises=z[:n]), agent.compute_flow_actions(obs[:n], z[:n])
        np.testing.assert_allclose(got_s, ref.sample_actions(obs[:n], z[:n]), atol=2e-6, err_msg=str(n))
        np.testing.assert_allclose(got_f, ref.compute_flow_actions(obs[:n], z[:n]), atol=5e-6, err_msg=str(n))
        for j in sorted({0, n // 2, min(n - 1, 4095), n - 1}):
            np.testing.assert_array_equal(agent.sample_actions(obs[j:j + 1], noises=z[j:j + 1])[0], got_s[j], err_msg=f'n {n} row {j}')
            np.testing.assert_array_equal(agent.compute_flow_actions(obs[j:j + 1], z[j:j + 1])[0], got_f[j], err_msg=f'n {n} row {j}')
    agent.close()


@pytest.mark.parametrize('cid', ['w50', 'w500'])
def test_module_queries_match_the_fp64_oracle(cid):
    """network.select(name) of the four FQL modules at n = 5 and 37, at tests/test_gpu_module_forward.py's fp32 bound."""
    from tests.test_gpu_module_forward import _bound_fp32, _check_all_modules
    od, ad = PC.FQL_CASES[cid][:2]
    cfg, ds, batch, noise, params, agent = _agent(cid)
    assert list(agent._modules) == ['critic', 'target_critic', 'actor_bc_flow', 'actor_onestep_flow']
    _check_all_modules(agent, agent.get_params(), od, ad, _bound_fp32, f'fql/{cid}', ns=(5, 37))
    agent.close()


# ---- 5. create-time layout ------------------------------------------------------------------------------------------------------------
def test_create_initialises_like_the_reference_at_hidden_500():
    """tests/test_gpu_hardening.py::test_create_initialises_like_the_reference's checks at (500,) * 4: the Glorot limit from the real
    fan-in and fan-out (500, not 512), attained; biases 0, LayerNorm (1, 0).  get_params gives the real shapes, and set_params then
    get_params is bitwise the tree set, random on every leaf."""
    import fql_amd
    od, ad, hidden = 29, 8, (500,) * 4
    cfg = make_problem(od, ad, 64, hidden, seed=1)[0]
    ex = np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32)
    a0, a1 = (fql_amd.FQLAgent.create(s, *ex, cfg) for s in (0, 1))
    p0 = a0.get_params()
    assert_initialised_like_the_reference(p0, a1.get_params(), a0.get_opt_state(), n_kernel=20)
    want = leaf_dict(O.init_params(0, od, ad, cfg))
    got = leaf_dict(p0)
    assert list(got) == list(want)
    for path, w in want.items():
        assert got[path].shape == w.shape and got[path].dtype == np.float32, (path, got[path].shape, w.shape)
    assert got['modules_critic/value_net/Dense_1/kernel'].shape == (2, 500, 500)
    assert got['modules_critic/value_net/LayerNorm_3/scale'].shape == (2, 500)
    assert got['modules_actor_bc_flow/mlp/Dense_0/kernel'].shape == (od + ad + 1, 500)
    assert got['modules_actor_onestep_flow/mlp/Dense_4/kernel'].shape == (500, ad)
    rng = np.random.default_rng(17)
    p = O.tree_map(lambda x: rng.standard_normal(x.shape).astype(np.float32), p0)
    a0.set_params(p)
    back = leaf_dict(a0.get_params())
    for path, x in leaf_dict(p).items():
        np.testing.assert_array_equal(back[path], x, err_msg=path)
    a0.close(); a1.close()
