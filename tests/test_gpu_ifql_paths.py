"""GPU: the IFQL update at the shapes and batches that switch kernels (tests/ifql_cases.py), against the fp64 restatement at the bounds of
tests/test_gpu_ifql.py (its _check_total_loss, _check_first_update and _check_step, unchanged: infos 5e-5 rel + 5e-6, per-leaf gradients
2e-5 max|g|, nu 1e-4, the parameter and Polyak bounds).

Every path case reads the update program back through fql_debug_plan (tests/util.py read_plan), prints its summary and asserts the path
its id names BEFORE any number is compared, and again after the two steps.  A task is (M, N, K) with the rows of its tile; the value net
runs at 2B rows, its backward and every other pass at B:
  b512_mixed   one fql_side_big_kernel launch holds the value pass [1024, 512, K] on 64-row tiles AND the target critics' and the flow
               net's [512, 512, K] on 32-row tiles (tile0 of the later tasks and their XCD order follow the big task's 128 tiles)
  b272         M 544 and 272: the 16-row kernel everywhere; weight gradients and LayerNorm backward at M 272 (17 steps of 16; a partial
               second trip of 256)
  b544_h64     [1088, 64, 64] on 64-row tiles beside M 544 on the 16-row kernel
  b1040_h64    M 2080 and 1040: the 16-row fallback above 1024 rows
  b2048_h64    M 4096 and 2048 on 64-row tiles
  wide1024     every K 1024 task on fql_gemm16_kernel<true>, [M, 1024, 1024] at M 96 and 48
  obs600       the three nets' first layers [M, 64, 640] on fql_gemm16_kernel<true> (B 48: at B 64 they are 64-aligned and take
               fql_side_kernel's 32-row tiles instead)
  no_ln_h512   no LayerNorm-backward task; the heads' dgrads [256, 512, 16] of the value net and both critics are GEMM tasks (with
               LayerNorm they are synthesised inside its backward) and the hidden dgrads are among the [256, 512, 512] tasks
  act16        heads [M, 16, 512]; no task 32 wide
  b16          M 32 and 16 only
Every case landed where the selection code in fql_engine.hip places it except obs600, which was moved from B 64 to B 48.
"""
import time

import numpy as np
import pytest

from tests import ifql_cases as K
from tests import ifql_oracle as IO
from tests.test_gpu_ifql import _agent, _check_first_update, _check_step, _check_total_loss
from tests.util import (K_GEMM16, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, OP_DGRAD0, OP_GEMM, OP_GEMM64, assert_same_state, leaf_dict, plan_gemm,
                        plan_has, plan_ln, plan_wgrad, print_plan, read_plan, sync_restatement)

pytestmark = pytest.mark.gpu


def _ms(tasks):
    return {t['M'] for t in tasks}


def _rows16_only(plan, kernels=(K_GEMM16,)):
    g = plan_gemm(plan)
    assert g and all(t['rows'] == 16 and t['kernel'] in kernels and t['type'] == OP_GEMM for t in g), sorted({(t['kernel'], t['rows']) for t in g})
    return g


def _common(plan, B):
    """What every IFQL plan holds: passes at 2B and B rows only, weight gradients and LayerNorm backward at B only (the value net's
    backward is rows [0, B) of its pass), and no first-layer input gradient of any kind."""
    g = plan_gemm(plan)
    assert _ms(g) == {B, 2 * B} and _ms(plan_wgrad(plan)) == {B} and set(plan_ln(plan)) <= {B}
    assert not [L for L in plan if L['type'] == OP_DGRAD0]
    return g


def _p_b512_mixed(plan, B):
    _common(plan, B)
    mixed = [L for L in plan if L['kernel'] == K_SIDE_BIG and any((t['M'], t['rows']) == (2 * B, 64) for t in L['gemm'])
             and any((t['M'], t['rows']) == (B, 32) for t in L['gemm'])]
    assert 2 * B == 1024 and mixed
    for L in mixed:   # the big task first: the 32-row tasks start at tile 128, a multiple of 8, and keep their XCD order
        assert L['type'] == OP_GEMM64 and L['gemm'][0]['rows'] == 64 and all(t['xg'] > 0 for t in L['gemm'] if t['rows'] == 32), L
        assert L['grid'] >= sum((t['M'] // t['rows']) * (t['N'] // (32 * t['wk'])) for t in L['gemm'])
    assert any(plan_has(L['gemm'], 2 * B, 512, 512, rows=64) and len(plan_has(L['gemm'], B, 512, 512, rows=32)) == 3 for L in mixed)
    assert plan_has(plan_gemm(plan, (K_SIDE,)), B, 512, 512, rows=32)   # and plain 32-row launches beside them (the critic's lane)


def _p_b272(plan, B):
    g = _common(plan, B)
    _rows16_only(plan)
    assert plan_has(g, 2 * B, 512, 512) and plan_has(g, B, 512, 512)
    assert {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)} == {(B, 64, 512), (B, 512, 512), (B, 512, 16)}
    assert B in plan_ln(plan) and B // 16 == 17 and B % 256 == 16


def _p_b544_h64(plan, B):
    g = _common(plan, B)
    big = [t for t in g if t['M'] == 2 * B and t['N'] % 64 == 0 and t['K'] % 64 == 0]
    assert 2 * B == 17 * 64 and len(big) == 4 and all(t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in big)
    small = [t for t in g if t['M'] == B]
    assert plan_has(small, B, 64, 64) and all(t['rows'] == 16 and t['kernel'] == K_GEMM16 for t in small)


def _p_b1040_h64(plan, B):
    g = _common(plan, B)
    _rows16_only(plan)
    assert B > 1024 and plan_has(g, 2 * B, 64, 64) and plan_has(g, B, 64, 64)
    assert (B, 64, 64) in {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}


def _p_b2048_h64(plan, B):
    g = _common(plan, B)
    hid = [t for t in g if t['N'] % 64 == 0 and t['K'] % 64 == 0]
    assert plan_has(hid, 2 * B, 64, 64) and plan_has(hid, B, 64, 64)
    assert all(t['rows'] == 64 and t['kernel'] == K_SIDE_BIG and t['type'] == OP_GEMM64 for t in hid)


def _p_wide1024(plan, B):
    g = _common(plan, B)
    _rows16_only(plan, (K_GEMM16, K_GEMM16_KBIG))
    kbig = [t for t in g if t['K'] > 512]
    assert kbig and all(t['kernel'] == K_GEMM16_KBIG for t in kbig)
    assert plan_has(kbig, 2 * B, 1024, 1024) and plan_has(kbig, B, 1024, 1024) and plan_has(kbig, 2 * B, 16, 1024)
    assert (B, 1024, 1024) in {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}


def _p_obs600(plan, B):
    g = _common(plan, B)
    _rows16_only(plan, (K_GEMM16, K_GEMM16_KBIG))
    first = [t for t in g if t['K'] >= 640]
    assert all(t['kernel'] == K_GEMM16_KBIG and (t['N'], t['K']) == (64, 640) for t in first)
    # the value net at 2B rows; both critics, both target critics and the flow net at B
    assert len(plan_has(first, 2 * B, 64, 640)) == 1 and len(plan_has(first, B, 64, 640)) == 5
    assert len([t for t in plan_wgrad(plan) if (t['Kin'], t['N']) == (640, 64)]) == 4   # value, two critics, flow


def _p_no_ln_h512(plan, B):
    g = _common(plan, B)
    assert not plan_ln(plan)
    # the heads' dgrads: value, both critics, flow (with LayerNorm only the flow net's is a GEMM task: test act16)
    assert len(plan_has(g, B, 512, 16)) == 4
    # forward: 2 critics + 2 targets + flow, 3 hidden layers each; hidden dgrads: value (rows [0, B)), 2 critics, flow, 3 each
    assert len(plan_has(g, B, 512, 512)) == 15 + 12 and len(plan_has(g, 2 * B, 512, 512)) == 3


def _p_act16(plan, B):
    g = _common(plan, B)
    assert len(plan_has(g, B, 16, 512, rows=16, kernel=K_GEMM16)) == 5 and plan_has(g, 2 * B, 16, 512)
    assert len(plan_has(g, B, 512, 16)) == 1 and not [t for t in g if t['N'] == 32 or t['K'] == 32]
    assert (B, 512, 16) in {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}


def _p_b16(plan, B):
    _common(plan, B)
    _rows16_only(plan)
    assert B == 16


def _p_w50_padded(plan, B):
    g = _common(plan, B)
    # out 50 of out_p 64: the value net's 2B = 64 rows on fql_side_kernel's 32-row tiles (LayerNorm partial sums over 50 of 64 columns),
    # every B-row task on the 16-row kernel
    assert plan_has(plan_gemm(plan, (K_SIDE,)), 2 * B, 64, 64, rows=32) and B in plan_ln(plan)
    assert plan_has(g, B, 64, 64) and all(t['rows'] == 16 and t['kernel'] == K_GEMM16 for t in g if t['M'] == B)
    assert (B, 64, 64) in {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}


def _p_w500_padded(plan, B):
    g = _common(plan, B)
    assert plan_has(g, 2 * B, 512, 512) and plan_has(g, B, 512, 512) and B in plan_ln(plan)   # out 500 of out_p 512
    assert plan_has(plan_gemm(plan, (K_SIDE,)), 2 * B, 512, 512, rows=32)                 # LayerNorm partial sums over 500 valid columns
    assert (B, 512, 512) in {(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}


PROPERTY = {'b512_mixed': _p_b512_mixed, 'b272': _p_b272, 'b544_h64': _p_b544_h64, 'b1040_h64': _p_b1040_h64, 'b2048_h64': _p_b2048_h64,
            'wide1024': _p_wide1024, 'obs600': _p_obs600, 'no_ln_h512': _p_no_ln_h512, 'act16': _p_act16, 'b16': _p_b16,
            'w50_padded': _p_w50_padded, 'w500_padded': _p_w500_padded}


def _recorded(ref):
    """The infos every later ref.update returns, in order (the checks keep them to themselves)."""
    rec, update = [], ref.update

    def recording(*a, **kw):
        out = update(*a, **kw)
        rec.append(out[1])
        return out
    ref.update = recording
    return rec


def _info_deviation(a, want):
    got = a.read_info()
    return max((abs(float(got[k]) - w) / max(1.0, abs(w)), k) for k, w in want.items())


@pytest.mark.parametrize('case', list(K.PATHS))
def test_paths_match_fp64_restatement(case):
    """The plan's property, total_loss (no state change), the first update from zero moments, a second one from the engine's own state
    and moments (sync_restatement), the property again.  Nothing is masked out of any comparison."""
    t0 = time.perf_counter()
    od, ad, B = K.PATHS[case][:3]
    cfg, batch, params, noises = K.problem(case)
    a = _agent(cfg, batch, params=params)
    plan = read_plan(a)
    print_plan(case, plan)
    PROPERTY[case](plan, B)
    ref = IO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    wants = _recorded(ref)
    _check_total_loss(a, ref, params, batch, noises[0])
    worst = _check_first_update(a, ref, cfg, params, batch, noises[0])
    dev = _info_deviation(a, wants[-1])
    sync_restatement(ref, a)
    _check_step(a, ref, cfg, batch, noises[1], leaf_dict(a.get_params()))
    dev = max(dev, _info_deviation(a, wants[-1]))
    opt = a.get_opt_state()
    assert opt['count'] == 2 and opt['step'] == 3
    PROPERTY[case](read_plan(a), B)   # reading the plan changed no launch
    print(f'{case}: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info deviation {dev[0]:.3e} ({dev[1]}), '
          f'{time.perf_counter() - t0:.2f} s')


def test_batch_size_walk_at_hidden_512(tmp_path):
    """One hidden-512 handle through B = 256, 512, 272, 16, 256: 32-row tiles, the mixed 64- and 32-row launches, the 16-row kernel, one
    tile per task, and back.  Every step is compared with the restatement from the engine's own pre-step state; the rebuilt plan holds the
    new row counts only; and a fresh handle created at that batch size, loaded from a checkpoint taken before the step and given the same
    rows and noise, ends bitwise where the walking handle ends, infos included."""
    from fql_amd import checkpoint
    od, ad, sizes, seed = K.WALK
    cfg = K.config(K.H512, K.H512, sizes[0])
    params = K.parameters(od, ad, cfg, seed)
    batch0, _ = K.data(od, ad, sizes[0], seed, steps=1)
    a = _agent(cfg, batch0, params=params)
    ref = IO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    # (rows, kernel) of the hidden layers' [B, 512, 512] and [2B, 512, 512] tasks.  B 512: the B-row tasks of the value net's lane ride
    # in fql_side_big_kernel launches beside the 2B-row task, those of the critic's lane in fql_side_kernel launches
    small = {256: {(32, K_SIDE)}, 512: {(32, K_SIDE), (32, K_SIDE_BIG)}, 272: {(16, K_GEMM16)}, 16: {(16, K_GEMM16)}}
    large = {256: {(32, K_SIDE)}, 512: {(64, K_SIDE_BIG)}, 272: {(16, K_GEMM16)}, 16: {(16, K_GEMM16)}}
    for i, B in enumerate(sizes):
        batch, (noise,) = K.data(od, ad, B, seed + 10 * i, steps=1)
        a.synchronize()
        assert a.get_opt_state()['count'] == i
        checkpoint.save_agent(a, str(tmp_path), i)
        fresh = _agent(K.config(K.H512, K.H512, B), batch, seed=99)
        checkpoint.restore_agent(fresh, str(tmp_path), i)
        assert_same_state(a, fresh)
        sync_restatement(ref, a)
        print('step at B', B)
        _check_step(a, ref, cfg, batch, noise, leaf_dict(a.get_params()))
        plan = read_plan(a)
        g = _common(plan, B)
        hid = plan_has(g, B, 512, 512)
        assert {(t['rows'], t['kernel']) for t in hid} == small[B]
        assert {(t['rows'], t['kernel']) for t in plan_has(g, 2 * B, 512, 512)} == large[B]
        fresh.update(batch, noise=noise)
        fresh.synchronize()
        assert_same_state(a, fresh)
        assert a.read_info() == fresh.read_info()
        assert [L['type'] for L in read_plan(fresh)] == [L['type'] for L in plan]
    opt = a.get_opt_state()
    assert opt['count'] == len(sizes) and opt['step'] == len(sizes) + 1


@pytest.mark.parametrize('case', K.AQL_CASES)
def test_aql_and_graph_updates_bitwise_over_8_steps(case):
    """tests/test_gpu_ifql.py::test_aql_and_graph_updates_bitwise_over_20_steps at the mixed-tile and the 16-row shapes."""
    import torch
    od, ad, B, actor, value, kw, seed = K.PATHS[case]
    cfg = K.config(actor, value, B, **kw)
    ds = K.dataset(od, ad, B, seed)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    PROPERTY[case](read_plan(a), B)
    s = torch.cuda.Stream()
    for _ in range(8):
        a.update_from_dataset()
        b.update_from_dataset(stream=s.cuda_stream)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    assert_same_state(a, b)
    assert a.read_info() == b.read_info()
    a2 = _agent(cfg, ds)   # determinism: same seed, same device-drawn rows and noise
    a2.upload_dataset(ds)
    for _ in range(8):
        a2.update_from_dataset()
    a2.synchronize()
    assert_same_state(a, a2)


@pytest.mark.parametrize('N,n', list(K.SAMPLER_CASES))
def test_sample_actions_at_hidden_512(N, n):
    """Best-of-N at obs 69, act 21 (padded action width 32) and hidden 512 for both nets: the flow program, the repeat / qin / select
    kernels and the scoring program at the width every other kind samples at.  Rows with a clear winner (top two scores more than 1e-2
    apart in fp64) must pick the restatement's action to 2e-5, the others a candidate within 1e-2 of the best score; row n - 1 equals its
    single-observation call bitwise; flow_actions on the same rows within 2e-5.  tests/test_kink_margins_cpu.py proves on the CPU that at
    least half the rows of these inputs have a clear winner."""
    od, ad = K.SAMPLER_SHAPE[:2]
    cfg, params, obs, noises = K.sampler_problem(N, n)
    a = _agent(cfg, {'observations': obs, 'actions': noises[:, 0]}, params=params)
    ref = IO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    want, cand, q = K.best_of_n(ref, obs, noises)
    for i in (0, n - 1):   # the batched restatement is OracleIFQL.sample_actions row by row
        w, qi = ref.sample_actions(obs[i], noises[i])
        np.testing.assert_allclose(want[i], w, rtol=0, atol=1e-12)
        np.testing.assert_allclose(q[i], qi, rtol=0, atol=1e-12)
    got = a.sample_actions(obs, noises=noises)
    assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
    clear = K.clear_winners(q)
    print(f'N {N} n {n}: clear-winner share {clear.mean():.3f}, worst |action - restatement| on them {np.abs(got[clear] - want[clear]).max():.3e}')
    assert clear.mean() >= 0.5, clear.mean()
    np.testing.assert_allclose(got[clear], want[clear], rtol=0, atol=2e-5)
    for i in np.nonzero(~clear)[0]:
        near = q[i] >= q[i].max() - K.SAMPLER_GAP
        assert np.abs(cand[i][near] - got[i]).max(axis=1).min() <= 2e-5, i
    np.testing.assert_array_equal(got[n - 1], a.sample_actions(obs[n - 1], noises=noises[n - 1]))
    z = noises[:, 0]
    np.testing.assert_allclose(a.compute_flow_actions(obs, z), cand[:, 0], rtol=0, atol=2e-5)
