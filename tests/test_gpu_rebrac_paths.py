"""GPU: the ReBRAC update at the shapes and batches that switch kernels (tests/rebrac_cases.py), against the fp64 restatement at the
bounds of tests/test_gpu_rebrac.py (its _check_total_loss and _check_step, unchanged: infos 5e-5 rel + 5e-6, per-leaf gradients 2e-5
max|g|, nu 1e-4, the parameter and Polyak bounds).

Every path case reads the full step's program back through fql_debug_plan (tests/util.py read_plan; the critic-only program is not
exported and is covered by numbers only), prints its summary and asserts the path its id names BEFORE any number is compared, and again
after the three steps: a full step from zero moments, a critic-only step and another full step, each from the engine's own state
(sync_restatement), so the target actor's Polyak and the actor's moments decayed by a zero gradient are compared too.  Before each full
step the restatement asserts q_tie >= MARGIN at the state it steps from (tests/rebrac_cases.py).  Every pass runs at B rows.  The
critic's first-layer input gradient is the lean OP_DGRAD0 launch (both members in one launch, 16 rows per workgroup; no task records,
its K is the critic's first hidden width) when K % 512 == 0, M % 16 == 0, act <= 16 and obs + 16 <= in_p = round64(obs + act);
otherwise a generic dgrad task [B, in_p, K] on the 16-row kernel:
  b272                 the 16-row kernel everywhere; OP_DGRAD0 (in_p 64, 29 + 16 <= 64)
  obs50                no OP_DGRAD0 (50 + 16 > 64): the generic dgrads [256, 64, 512] of both members
  b1040_h64            rows 16 above 1024; no OP_DGRAD0 (K 64)
  b2048_h64            every 64-aligned task on fql_side_big_kernel's 64-row tiles; the two generic first-layer dgrads stay on the 16-row kernel
  wide1024             every K 1024 task on fql_gemm16_kernel<true>; OP_DGRAD0 at K 1024
  obs600               first layers [48, 64, 640] on fql_gemm16_kernel<true>; the generic dgrads [48, 640, 64], action block at column 600
                       (B 48: at B 64 the first layers are 64-aligned and take fql_side_kernel's 32-row tiles instead)
  no_ln_h512_no_tanh   no LayerNorm-backward task; OP_DGRAD0 with all 16 columns live
  b16                  M 16 only
Every case landed where the selection code in fql_engine.hip places it except obs600, which was moved from B 64 to B 48.
"""
import time

import numpy as np
import pytest

from tests import rebrac_cases as K
from tests import rebrac_oracle as RO
from tests import test_gpu_rebrac as TR
from tests.test_gpu_rebrac import _agent, _check_step, _check_total_loss
from tests.util import (K_GEMM16, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, OP_DGRAD0, OP_GEMM, OP_GEMM64, assert_same_state, leaf_dict, plan_gemm,
                        plan_has, plan_ln, plan_wgrad, print_plan, read_plan, sync_restatement)

pytestmark = pytest.mark.gpu


def _rows16_only(plan, kernels=(K_GEMM16,)):
    g = plan_gemm(plan)
    assert g and all(t['rows'] == 16 and t['kernel'] in kernels and t['type'] == OP_GEMM for t in g), sorted({(t['kernel'], t['rows']) for t in g})


def _common(plan, B):
    g = plan_gemm(plan)
    assert {t['M'] for t in g} == {B} == {t['M'] for t in plan_wgrad(plan)} and set(plan_ln(plan)) <= {B}
    return g


def _dgrad0(plan, B, present):
    """The lean first-layer input gradient: one launch for both members, B / 16 workgroups each; or none."""
    lean = [L for L in plan if L['type'] == OP_DGRAD0]
    assert [L['grid'] for L in lean] == ([2 * (B // 16)] if present else []), [(L['type'], L['grid']) for L in lean]


def _p_b272(plan, B):
    g = _common(plan, B)
    _rows16_only(plan)
    _dgrad0(plan, B, True)
    assert plan_has(g, B, 512, 512) and not plan_has(g, B, 64, 512) and B // 16 == 17


def _p_obs50(plan, B):
    g = _common(plan, B)
    _dgrad0(plan, B, False)
    # beyond layer 0's forward [256, 512, 64]: its input gradient [256, in_p 64, 512] for both members, on the 16-row kernel
    assert len(plan_has(g, B, 64, 512, rows=16, kernel=K_GEMM16)) == 2 and plan_has(g, B, 512, 64)


def _p_b1040_h64(plan, B):
    g = _common(plan, B)
    _rows16_only(plan)
    _dgrad0(plan, B, False)
    assert B > 1024 and plan_has(g, B, 64, 64)


def _p_b2048_h64(plan, B):
    g = _common(plan, B)
    _dgrad0(plan, B, False)
    big = [t for t in g if t['type'] == OP_GEMM64]
    assert plan_has(big, B, 64, 64) and all(t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in big)
    # the generic first-layer dgrads [2048, in_p 64, 64] are never offered to the tiled kernels
    assert len(plan_has(g, B, 64, 64, rows=16)) == 2 and len(plan_has(big, B, 64, 64)) == len(plan_has(g, B, 64, 64)) - 2


def _p_wide1024(plan, B):
    g = _common(plan, B)
    _rows16_only(plan, (K_GEMM16, K_GEMM16_KBIG))
    _dgrad0(plan, B, True)   # K = the critic's first hidden width, 1024
    kbig = [t for t in g if t['K'] > 512]
    assert kbig and all(t['kernel'] == K_GEMM16_KBIG for t in kbig) and plan_has(kbig, B, 1024, 1024) and plan_has(kbig, B, 16, 1024)
    assert not plan_has(g, B, 64, 1024)   # no generic first-layer dgrad beside the lean one


def _p_obs600(plan, B):
    g = _common(plan, B)
    _rows16_only(plan, (K_GEMM16, K_GEMM16_KBIG))
    _dgrad0(plan, B, False)
    first = [t for t in g if t['K'] >= 640]
    # actor, target actor, and the critic pair on (obs, actions), (next_obs, a') and (obs, a)
    assert len(first) == 8 and all(t['kernel'] == K_GEMM16_KBIG and (t['N'], t['K']) == (64, 640) for t in first)
    assert len(plan_has(g, B, 640, 64)) == 2   # the generic dgrad with N = the critic's in_p


def _p_no_ln(plan, B):
    g = _common(plan, B)
    assert not plan_ln(plan)
    _dgrad0(plan, B, True)
    assert len(plan_has(g, B, 512, 16)) == 5   # the heads' dgrads as GEMM tasks: actor, critic(obs, a) pair, critic(obs, actions) pair


def _p_b16(plan, B):
    _common(plan, B)
    _rows16_only(plan)
    assert B == 16


def _p_w50_padded(plan, B):
    g = _common(plan, B)
    _rows16_only(plan)
    _dgrad0(plan, B, False)
    assert plan_has(g, B, 64, 64) and B in plan_ln(plan)   # out 50 of out_p 64


PROPERTY = {'b272': _p_b272, 'obs50': _p_obs50, 'b1040_h64': _p_b1040_h64, 'b2048_h64': _p_b2048_h64, 'wide1024': _p_wide1024,
            'obs600': _p_obs600, 'no_ln_h512_no_tanh': _p_no_ln, 'b16': _p_b16, 'w50_padded': _p_w50_padded}


def _recorded(ref):
    """The infos every later ref.update returns, in order (_check_step keeps them to itself)."""
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
    """The plan's property, total_loss of both step kinds (no state change), a full step from zero moments, a critic-only step and a full
    step from the engine's own state and moments, the property again.  Nothing is masked out of any comparison."""
    t0 = time.perf_counter()
    od, ad, B = K.PATHS[case][:3]
    cfg, batch, params, noises = K.problem(case)
    a = _agent(cfg, batch, params=params)
    plan = read_plan(a)
    print_plan(case, plan)
    PROPERTY[case](plan, B)
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    wants = _recorded(ref)
    _check_total_loss(a, ref, params, batch, noises[0])
    worst, dev = (0.0, ''), (0.0, '')
    for i, (noise, full) in enumerate(zip(noises, K.STEP_KINDS)):
        assert a.get_opt_state()['count'] == i
        sync_restatement(ref, a)
        if full:
            print(case, 'step', i, 'q_tie', K.check_margin(ref, batch, what=(case, i)), 'q1 the smaller on', K.first_member_share(ref, batch))
        worst = max(worst, _check_step(a, ref, batch, noise, full, cfg, leaf_dict(a.get_params())))
        dev = max(dev, _info_deviation(a, wants[-1]))
    opt = a.get_opt_state()
    assert opt['count'] == 3 and opt['step'] == 4
    PROPERTY[case](read_plan(a), B)   # reading the plan changed no launch
    print(f'{case}: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info deviation {dev[0]:.3e} ({dev[1]}), '
          f'{time.perf_counter() - t0:.2f} s')


def test_the_b1024_shape_case_takes_the_lean_first_layer_dgrad():
    """tests/test_gpu_rebrac.py's b1024 case (obs 40, act 4): in_p = round64(44) = 64 and 40 + 16 <= 64, so dQ/da is the OP_DGRAD0 launch
    with 4 live columns, as in IQL's table; no generic first-layer dgrad [1024, 64, 512] is in the plan.  The hidden layers run on
    fql_side_big_kernel's 64-row tiles."""
    case = [p for p in TR.SHAPE_CASES if p.id == 'b1024']
    assert len(case) == 1
    od, ad, B, actor, value, kw = case[0].values
    cfg, _, batch, _ = TR._problem_at(od, ad, B, actor, value, seed=21, **kw)
    plan = read_plan(_agent(cfg, batch))
    print_plan('b1024', plan)
    g = _common(plan, B)
    _dgrad0(plan, B, True)
    assert (od, ad, B) == (40, 4, 1024) and not plan_has(g, B, 64, 512) and len(plan_has(g, B, 512, 64)) == 8
    hid = plan_has(g, B, 512, 512)
    assert hid and all(t['rows'] == 64 and t['kernel'] == K_SIDE_BIG for t in hid)


def test_batch_size_walk_at_hidden_512(tmp_path):
    """One hidden-512 handle through B = 256, 512, 272, 16, 256, full and critic-only steps in turn: each switch rebuilds the workspace and
    all three programs.  Every step is compared with the restatement from the engine's own pre-step state; the rebuilt plan holds the new
    row count only; and a fresh handle created at that batch size, loaded from a checkpoint taken before the step and given the same rows
    and noise, ends bitwise where the walking handle ends, infos included."""
    from fql_amd import checkpoint
    od, ad, sizes, _ = K.WALK
    cfg, params, steps = K.walk_problem()
    a = _agent(cfg, steps[0][0], params=params)
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    paths = {256: (32, K_SIDE), 512: (32, K_SIDE), 272: (16, K_GEMM16), 16: (16, K_GEMM16)}
    for i, (batch, noise, full) in enumerate(steps):
        B = sizes[i]
        a.synchronize()
        assert a.get_opt_state()['count'] == i
        checkpoint.save_agent(a, str(tmp_path), i)
        fresh = _agent(K.config(K.H512, K.H512, B), batch, seed=99)
        checkpoint.restore_agent(fresh, str(tmp_path), i)
        assert_same_state(a, fresh)
        sync_restatement(ref, a)
        if full:
            K.check_margin(ref, batch, what=('walk', i))
        print('step at B', B, 'full' if full else 'critic-only')
        _check_step(a, ref, batch, noise, full, cfg, leaf_dict(a.get_params()))
        plan = read_plan(a)
        g = _common(plan, B)
        _dgrad0(plan, B, True)
        assert {(t['rows'], t['kernel']) for t in plan_has(g, B, 512, 512)} == {paths[B]}
        fresh.update(batch, full_update=full, noise=noise)
        fresh.synchronize()
        assert_same_state(a, fresh)
        assert a.read_info() == fresh.read_info()
        assert [L['type'] for L in read_plan(fresh)] == [L['type'] for L in plan]
    opt = a.get_opt_state()
    assert opt['count'] == len(sizes) and opt['step'] == len(sizes) + 1


@pytest.mark.parametrize('case', K.AQL_CASES)
def test_aql_and_graph_updates_bitwise_over_8_mixed_steps(case):
    """tests/test_gpu_rebrac.py::test_aql_and_graph_updates_bitwise_over_20_mixed_steps on the 16-row kernel below and above 1024 rows."""
    import torch
    od, ad, B, actor, value, kw, seed = K.PATHS[case]
    cfg = K.config(actor, value, B, **kw)
    ds = K.dataset(od, ad, B, seed)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    PROPERTY[case](read_plan(a), B)
    s = torch.cuda.Stream()
    for i in range(8):
        a.update_from_dataset(full_update=i % 2 == 0)
        b.update_from_dataset(stream=s.cuda_stream, full_update=i % 2 == 0)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    assert_same_state(a, b)
    a2 = _agent(cfg, ds)   # determinism: same seed, same device-drawn rows and noise
    a2.upload_dataset(ds)
    for i in range(8):
        a2.update_from_dataset(full_update=i % 2 == 0)
    a2.synchronize()
    assert_same_state(a, a2)
