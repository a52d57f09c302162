"""GPU: FQL (obs 29, act 8) at the batch sizes where the update kernels change their loops and tiles, one update from zero moments
against the fp64 oracle on identical params, batch and noise, in fp32 (tests/util.py's bounds, unchanged) and in precision 'bf16x3' (the
two 1e-4 bounds of test_gpu_precision.py).  Every case first asserts, from the engine's own plan (the diagnostic export fql_debug_plan,
tests/util.py read_plan), that it runs the path it is named for, then compares numbers.

The edges and the case that covers each (M = batch rows of a task; fql_amd/csrc/fql_kernels.h, fql_engine.hip):
  * weight gradient (wgrad_body, wgrad_split_body): steps = M / 16 MFMA steps per wave in 8-step chunks, two register buffers, 16 steps
    per loop trip.  steps 9 (full a0, partial a1): b144.  steps 17 (full a0, full a1, partial a0, no a1): b272.  A partial chunk on a
    later trip: steps 25 b400, steps 65 b1040_h64.  Whole chunks at 48 and 128: b768, b2048.
  * LayerNorm-backward column pass (lnbwd_body: rows in strides of 256, 16 clamped rows in flight): a partial second trip at M 272 and
    400: b272, b400.
  * XCD-aware tile order (xcd_tile) of the 32-row side tiles: fp32 xg 8: b256_h64 (N 64 is one column tile: no other grouping divides it).  fp32
    xg 4 below M 1024: b768.  Split tiles xg 8: b2048 (and b256_h64).  Split tiles at M 1088, where no grouping divides the 34 row
    tiles (xg 0, row-major): b1088_h64.
  * the chain's 16-row tiles, chain<256>: xg 1 at 9 row tiles: b144.  xg 2: b256.  xg 4: b768.  xg 8: b2048.
  * fql_side_big_kernel (fp32, M >= 1024, M % 64 == 0) at an odd tile count, 17 row tiles of M 1088: b1088_h64; at M 2048: b2048.
  * the 16-row fallback above 1024, M 1040 (not a multiple of 64, 65 row tiles): b1040_h64.  No 32- or 64-row task below it: b144.
The cases were placed by reading the selection code, and the plan put each where it was placed: none had to move.

A wrong tail in the weight gradient fails these tests: in a copy of the numpy oracle at B 144, dropping the last 16 batch rows from one
layer's dW (critic, BC flow or one-step actor, Dense_1) moves that leaf by 0.23 to 0.32 of its largest entry, 1.1e4 to 1.6e4 times
assert_step_matches' gradient bound of 2e-5 and over 2e3 times the bf16x3 bound.

Measured against the fp64 oracle (worst |g_gpu - g_ref| / max|g_ref| over the leaves; worst info delta / max(1, |ref|)); figures, not bounds:
  case        fp32 gradient  fp32 info  bf16x3 gradient  bf16x3 info
  b144        4.3e-07        2.8e-07    5.3e-06          2.8e-07
  b256        3.5e-07        2.1e-07    9.7e-06          2.7e-06
  b272        3.8e-07        1.2e-07    5.2e-06          1.2e-07
  b400        4.4e-07        2.2e-07    4.6e-06          4.4e-07
  b256_h64    5.5e-07        1.0e-07    1.6e-05          3.5e-06
  b768        4.0e-07        1.7e-07    8.4e-06          1.1e-06
  b1040_h64   3.4e-07        6.5e-08    2.5e-06          1.9e-07
  b1088_h64   4.6e-07        2.1e-07    1.1e-05          4.6e-06
  b2048       4.9e-07        1.3e-07    9.7e-06          1.4e-06

test_batch_size_switches_equal_fresh_agents and test_aql_equals_graph_at_b400_and_b1088 pin the rebuilt task tables and AQL packets of a
batch-size switch, and both dispatch forms, at these sizes (bitwise).
"""
import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import (BF16X3_BOUND, K_CHAIN, K_CHAIN_SPLIT, K_GEMM16, K_GEMM16_EULER, K_SIDE, K_SIDE_BIG, K_SIDE_SPLIT, OP_GEMM64,
                        assert_same_state, assert_step_matches, assert_total_loss_matches, bf16x3_update_errors, make_problem, plan_lib,
                        randomize_params, read_plan)

pytestmark = pytest.mark.gpu

OD, AD = 29, 8
CASES = {   # id -> (B, hidden)
    'b144': (144, (256,) * 3),
    'b256': (256, (256,) * 3),
    'b272': (272, (256,) * 3),
    'b400': (400, (256,) * 3),
    'b256_h64': (256, (64,) * 3),
    'b768': (768, (256,) * 3),
    'b1040_h64': (1040, (64,) * 3),
    'b1088_h64': (1088, (64,) * 3),
    'b2048': (2048, (256,) * 3),
}
_PROBLEM = {}    # id -> (batch, noise, params, frozen fp64 reference): computed once, shared by both precisions, never written


class _FrozenRef:
    """The fp64 oracle's answers for one (params, batch, noise), computed once: total_loss, grads, then update, with the interface the
    assert helpers use (after update(), .params are the post-step parameters).  The arrays are read-only."""

    def __init__(self, params, cfg, batch, noise):
        ref = O.OracleFQL(params, dict(cfg), OD, AD, np.float64)
        self._loss = ref.total_loss(batch, noise)
        self._grads = ref.grads(batch, noise)
        self._update = ref.update(batch, noise)
        self.params = ref.params
        for tree in (self._grads[2], self.params):
            for _, leaf in O.tree_leaves_with_path(tree):
                leaf.flags.writeable = False

    def total_loss(self, batch, noise): return self._loss
    def grads(self, batch, noise): return self._grads
    def update(self, batch, noise): return self._update


def _agent(cid, precision):
    import fql_amd
    B, hidden = CASES[cid]
    cfg, ds, batch, noise = make_problem(OD, AD, B, hidden, seed=3, precision=precision)
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    if cid not in _PROBLEM:
        params = randomize_params(agent.get_params(), seed=5, scale=0.05 if max(hidden) >= 256 else 0.1)
        ocfg = dict(cfg)
        ocfg['precision'] = 'fp32'     # (the oracle is fp64 whatever the engine's mode)
        _PROBLEM[cid] = (batch, noise, params, _FrozenRef(params, ocfg, batch, noise))
    batch, noise, params, ref = _PROBLEM[cid]
    agent.set_params(params)
    return cfg, batch, noise, params, ref, agent


# ---- what a plan holds -------------------------------------------------------------------------------------------------------------
def _gemm(plan, kernels=None):
    return [dict(t, kernel=L['kernel']) for L in plan if kernels is None or L['kernel'] in kernels for t in L['gemm']]


def _chains(plan, H=256):
    return [dict(L['chain'], grid=L['grid'], kernel=L['kernel']) for L in plan if L['chain'] is not None and L['chain']['H'] == H]


def _assert_wgrad_steps(plan, B, precision):
    tasks = [t for L in plan for t in L['wgrad']]
    assert tasks and all(t['M'] % 16 == 0 for t in tasks)
    assert B // 16 in {t['M'] // 16 for t in tasks}, sorted({t['M'] for t in tasks})
    assert {t['split'] for t in tasks} == {1 if precision == 'bf16x3' else 0}      # the body that runs: wgrad_split_body / wgrad_body
    assert all(L['kernel'] in (K_SIDE, K_SIDE_SPLIT, K_SIDE_BIG) and L['type'] == OP_GEMM64 for L in plan if L['wgrad'] or L['ln'])


def _assert_chain256(plan, B, xg, precision):
    ch = _chains(plan)
    assert ch, 'no chain<256> launch'
    for c in ch:
        assert (c['M'], c['xg'], c['grid']) == (B, xg, (B // 16) * (256 // 32)), c
        assert (c['kernel'] == K_CHAIN_SPLIT) == bool(c['split']) and c['kernel'] in (K_CHAIN, K_CHAIN_SPLIT)
    assert any(c['split'] for c in ch) == (precision == 'bf16x3')


def _assert_no_tile_rows(plan, rows):
    assert not [t for t in _gemm(plan) if t['rows'] in rows]
    assert all(L['kernel'] != K_SIDE_BIG for L in plan)


def _side(precision):
    return (K_SIDE_SPLIT,) if precision == 'bf16x3' else (K_SIDE, K_SIDE_BIG)


def _p_b144(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    _assert_no_tile_rows(plan, (32, 64))                                             # M % 64 != 0
    hid = [t for t in _gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if (t['N'], t['K']) == (256, 256)]
    assert hid and all(t['rows'] == 16 and t['M'] % 144 == 0 for t in hid)          # hidden layers on the 16-row kernel
    _assert_chain256(plan, B, 1, precision)                                          # 9 row tiles: grid 9 x 8 (checked there)
    assert B // 16 == 9


def _p_b256(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    _assert_chain256(plan, B, 2, precision)


def _p_ln(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    assert B in [m for L in plan for m in L['ln']]                                   # a partial second trip of the column pass
    assert 256 < B < 512


def _p_b256_h64(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    assert [t for t in _gemm(plan, _side(precision)) if t['rows'] == 32 and t['xg'] == 8 and t['N'] == 64]


def _p_b768(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    if precision == 'fp32':
        assert [t for t in _gemm(plan, _side(precision)) if t['rows'] == 32 and t['xg'] == 4 and t['M'] < 1024]
    _assert_chain256(plan, B, 4, precision)


def _p_b1040_h64(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    _assert_no_tile_rows(plan, (32, 64))                                             # M >= 1024, M % 64 != 0: the 16-row kernels
    assert [t for t in _gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if t['M'] == B and t['rows'] == 16]


def _p_b1088_h64(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    if precision == 'fp32':
        big = [t for t in _gemm(plan, (K_SIDE_BIG,)) if t['M'] == B and t['rows'] == 64]
        assert big and B // 64 == 17
    else:
        sp = [t for t in _gemm(plan, (K_SIDE_SPLIT,)) if t['M'] == B]
        assert sp and all(t['rows'] == 32 and t['xg'] == 0 for t in sp)               # 34 row tiles: no grouping, row-major
        _assert_no_tile_rows(plan, (64,))


def _p_b2048(plan, B, precision):
    _assert_wgrad_steps(plan, B, precision)
    _assert_chain256(plan, B, 8, precision)
    if precision == 'fp32':
        assert [t for t in _gemm(plan, (K_SIDE_BIG,)) if t['M'] == B and t['rows'] == 64]
    else:
        assert [t for t in _gemm(plan, (K_SIDE_SPLIT,)) if t['rows'] == 32 and t['xg'] == 8]
        _assert_no_tile_rows(plan, (64,))


PROPERTY = {'b144': _p_b144, 'b256': _p_b256, 'b272': _p_ln, 'b400': _p_ln, 'b256_h64': _p_b256_h64, 'b768': _p_b768,
            'b1040_h64': _p_b1040_h64, 'b1088_h64': _p_b1088_h64, 'b2048': _p_b2048}


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('cid', list(CASES))
def test_update_matches_oracle_on_the_named_path(cid, precision):
    B, hidden = CASES[cid]
    cfg, batch, noise, params, ref, agent = _agent(cid, precision)
    PROPERTY[cid](read_plan(agent), B, precision)
    if precision == 'fp32':
        assert_total_loss_matches(agent, ref, params, batch, noise)
        worst = assert_step_matches(agent, ref, cfg, batch, noise)
        info, info_r = agent.read_info(), ref.update(batch, noise)[1]
        delta = max(abs(float(info[k]) - float(info_r[k])) / max(1.0, abs(float(info_r[k]))) for k in O.INFO_KEYS)
        print(f'{cid} fp32: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info delta {delta:.3e}')
    else:
        worst, deltas = bf16x3_update_errors(agent, ref, batch, noise)
        print(f'{cid} bf16x3: worst relative gradient error {worst[0]:.3e} ({worst[1]}), worst info delta {max(deltas.values()):.3e}')
        assert max(deltas.values()) <= BF16X3_BOUND, deltas
        assert worst[0] <= BF16X3_BOUND, worst
    PROPERTY[cid](read_plan(agent), B, precision)       # reading the plan changed no launch: the same plan after the update


def test_plan_refusals():
    """fql_debug_plan's bounds follow fql_debug_enc's: any prefix of the plan is served, one word more than the plan is FQL_E_INVALID
    (-1), as are a null handle and a byte count that is no multiple of 4.  A visual handle is refused with FQL_E_STATE (-4).  Every
    agent kind builds a prog_full, so none is refused for its kind: an IFQL handle answers."""
    import fql_amd
    from tests.test_gpu_visual import make_visual
    lib = plan_lib()
    cfg, ds, batch, noise = make_problem(OD, AD, 32, (64,) * 3, seed=3)
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    head = np.zeros(1, np.int32)
    assert lib.fql_debug_plan(agent._h, head.ctypes.data, 4) == 0
    n = int(head[0])
    buf = np.zeros(n + 1, np.int32)
    assert lib.fql_debug_plan(agent._h, buf.ctypes.data, 4 * n) == 0 and buf[0] == n and buf[1] == len(read_plan(agent))
    assert lib.fql_debug_plan(agent._h, buf.ctypes.data, 4 * n + 4) == -1
    assert lib.fql_debug_plan(agent._h, buf.ctypes.data, 6) == -1
    assert lib.fql_debug_plan(agent._h, None, 4) == -1
    assert lib.fql_debug_plan(None, buf.ctypes.data, 4) == -1
    assert lib.fql_debug_plan(agent._h, None, 0) == 0
    vcfg, vbatch, _ = make_visual()
    visual = fql_amd.FQLAgent.create(0, vbatch['observations'][:1], vbatch['actions'][:1], vcfg)
    assert lib.fql_debug_plan(visual._h, head.ctypes.data, 4) == -4
    icfg = fql_amd.ifql.get_config()
    icfg.update(actor_hidden_dims=(64,) * 3, value_hidden_dims=(64,) * 3, batch_size=32)
    ifql = fql_amd.IFQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], icfg)
    assert lib.fql_debug_plan(ifql._h, head.ctypes.data, 4) == 0 and head[0] > 2


def _twin_inputs(ds, B, step):
    return np.random.default_rng(100 + step).integers(0, len(ds['observations']), size=B), O.make_noise(B, AD, 40 + step)


def test_batch_size_switches_equal_fresh_agents():
    """One agent walks B = 256 -> 144 -> 1088 -> 400 -> 2048 -> 16 (every step resizes: programs, task tables and AQL packets are
    rebuilt); at each size an agent freshly created at that size, given the walker's parameters and optimizer state, does the same
    update: equal infos and bitwise equal state."""
    import fql_amd
    hidden, sizes = (256,) * 3, (256, 144, 1088, 400, 2048, 16)
    cfg, ds, batch, noise = make_problem(OD, AD, 2048, hidden, seed=3)      # (the dataset holds 4 x 2048 rows)
    ex = batch['observations'][:1], batch['actions'][:1]
    cfg['batch_size'] = sizes[0]
    walker = fql_amd.FQLAgent.create(0, *ex, cfg)
    walker.set_params(randomize_params(walker.get_params(), seed=5, scale=0.05))
    walker.upload_dataset(ds)
    for step, B in enumerate(sizes):
        fcfg = dict(cfg)
        fcfg['batch_size'] = B
        fresh = fql_amd.FQLAgent.create(0, *ex, fcfg)
        fresh.set_params(walker.get_params())
        fresh.set_opt_state(walker.get_opt_state())
        fresh.upload_dataset(ds)
        idxs, nz = _twin_inputs(ds, B, step)
        walker.update_from_dataset(B, idxs=idxs, noise=nz)
        fresh.update_from_dataset(B, idxs=idxs, noise=nz)
        assert walker.config['batch_size'] == B
        assert walker.read_info() == fresh.read_info(), B
        assert_same_state(walker, fresh)
        assert walker.get_opt_state()['count'] == step + 1
        fresh.close()


@pytest.mark.parametrize('B,hidden', [(400, (256,) * 3), (1088, (64,) * 3)], ids=['b400', 'b1088_h64'])
def test_aql_equals_graph_at_b400_and_b1088(B, hidden):
    """Both dispatch forms at a weight-gradient tail and LayerNorm-backward partial trip (B 400) and at fql_side_big_kernel's 17 row
    tiles (B 1088): the engine's own queues against the captured graph on a caller's stream, three updates from the same rows and noise."""
    import torch
    import fql_amd
    cfg, ds, batch, noise = make_problem(OD, AD, B, hidden, seed=3)
    agents = []
    for _ in range(2):
        a = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed=5, scale=0.05 if max(hidden) >= 256 else 0.1))
        a.upload_dataset(ds)
        agents.append(a)
    a, b = agents
    st = torch.cuda.Stream()
    for step in range(3):
        idxs, nz = _twin_inputs(ds, B, step)
        a.update_from_dataset(B, idxs=idxs, noise=nz)                          # stream left to the engine -> its own queues
        b.update_from_dataset(B, idxs=idxs, noise=nz, stream=st.cuda_stream)    # a caller's stream -> the captured graph
        assert a.synchronize() == 'aql'
        assert b.synchronize() == 'graph'
        st.synchronize()
        assert a.read_info() == b.read_info()
    assert_same_state(a, b)
