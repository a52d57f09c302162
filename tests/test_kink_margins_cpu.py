"""CPU: the inputs of the IQL and SAC shape cases (tests/test_gpu_iql.py, tests/test_gpu_sac.py) and of the ReBRAC path cases
(tests/rebrac_cases.py) are clear of the losses' kinks, and IFQL's hidden-512 sampler problems (tests/ifql_cases.py) are inside their cap.

The GPU tests compare every element of every gradient with the fp64 restatement and mask nothing out, which is sound only where the
restatement itself is a margin away from each point where a loss is not smooth: an element that sits on a kink may fall on the other
side in fp32 and take the other branch's gradient.  Each case's seeds were chosen for that; this file builds every problem exactly as
the GPU test does (the same functions, no engine) and asserts the margins in every step, so the choice can be checked on any machine.

A step after the first runs, on the GPU, from the engine's own state (tests/util.py sync_restatement), which parts from the
restatement's trajectory by up to 2 lr per element; there the restatement's own trajectory must keep 3 times the margin.
"""
import numpy as np
import pytest

from tests import ifql_cases as FC
from tests import ifql_oracle as FO
from tests import iql_oracle as IO
from tests import rebrac_cases as RC
from tests import rebrac_oracle as RO
from tests import sac_oracle as SO
from tests import test_gpu_iql as TI
from tests import test_gpu_sac as TS


def _iql_steps(ref, cfg, problems):
    """The restatement through the steps of `problems` ((batch, noise) each), as _check_step takes it: the |x| = 1 move (which asserts
    its own two conditions), then every margin, then the update.  The moved kink is cleared at the state of each step on the GPU too, so
    it alone needs no room in the later steps."""
    for i, (batch, noise) in enumerate(problems):
        cleared = TI._cleared(ref, batch, noise, cfg)
        moved, noise = cleared is not noise, cleared
        f = ref._forward(batch, noise)
        margins = ref.kink_margins(batch, noise, f)
        assert min(margins.values()) >= TI.MARGIN, (i, margins)
        if i:
            assert min(v for k, v in margins.items() if not (moved and k == 'unit_clip')) >= 3 * TI.MARGIN, (i, margins)
        if cfg['actor_loss'] == 'ddpgbc':   # both branches of the clip mask are live
            assert 0.2 <= np.mean(np.abs(f['x']) > 1.0) <= 0.8
        if i + 1 < len(problems):
            ref.update(batch, noise)


@pytest.mark.parametrize('case,actor_loss,const_std,seed', TI.SHAPE_COMBOS)
def test_iql_shape_cases_keep_their_margins(case, actor_loss, const_std, seed):
    shape, steps, cfg, batch, params, noises = TI.shape_problem(case, actor_loss, const_std, seed)
    assert len(noises) == steps
    _iql_steps(TI._ref(params, cfg, shape), cfg, [(batch, nz) for nz in noises])


def test_iql_shape_cases_are_the_combinations_asked_for():
    combos = {c[:3] for c in TI.SHAPE_COMBOS}
    assert len(combos) == len(TI.SHAPE_COMBOS)
    for case in TI.SHAPE_CASES:
        assert {(case, 'awr', False), (case, 'ddpgbc', False)} <= combos
    assert {('act16', 'ddpgbc', True), ('humanoidmaze', 'ddpgbc', True)} <= combos
    assert any(kw.get('actor_layer_norm') for _, kw, _ in TI.SHAPE_CASES.values())


def test_iql_batch_size_switch_keeps_its_margins():
    cfg, _, _, _, params = TI._problem(TI.SWITCH_SHAPE, TI.SWITCH_SEED, actor_loss='ddpgbc', const_std=False)
    _iql_steps(TI._ref(params, cfg, TI.SWITCH_SHAPE), cfg, [TI.switch_problem(cfg, i, B) for i, B in enumerate(TI.SWITCH_BATCHES)])


def test_clear_of_unit_clip_moves_only_the_near_elements_and_keeps_their_side():
    shape, _, cfg, batch, params, noises = TI.shape_problem('b272', 'ddpgbc', False, 2)
    ref = TI._ref(params, cfg, shape)
    before = ref._forward(batch, noises[0])['x']
    moved = IO.clear_of_unit_clip(ref, batch, noises[0], TI.MARGIN)
    assert moved['eps'].dtype == np.float32 and moved['eps'] is not noises[0]['eps']
    after = ref._forward(batch, moved)['x']
    near = np.abs(np.abs(before) - 1.0) < 2 * TI.MARGIN
    assert 0 < near.sum() <= 0.01 * near.size
    np.testing.assert_array_equal(moved['eps'][~near], noises[0]['eps'][~near])
    np.testing.assert_array_equal(after[~near], before[~near])
    assert ((np.abs(after) > 1.0) == (np.abs(before) > 1.0)).all() and (np.sign(after) == np.sign(before)).all()
    np.testing.assert_allclose(np.abs(np.abs(after[near]) - 1.0), 2 * TI.MARGIN, rtol=0, atol=1e-6)
    # nothing near the kink: the noise comes back unchanged
    np.testing.assert_array_equal(IO.clear_of_unit_clip(ref, batch, moved, TI.MARGIN)['eps'], moved['eps'])


@pytest.mark.parametrize('case', list(TS.SHAPE_CASES))
def test_sac_shape_cases_keep_their_margins(case):
    od, ad, cfg, batch, params, noises = TS.shape_problem(case)
    assert cfg['q_agg'] == 'min' and len(noises) == TS.SHAPE_CASES[case][6]
    ref = SO.OracleSAC(params, dict(cfg), od, ad, np.float64)
    raw = ref.actor_heads(batch['observations'])[1]
    assert (raw < SO.LOG_STD_MIN).any() and (raw > SO.LOG_STD_MAX).any()   # the clip bites on both sides
    for i, nz in enumerate(noises):
        margins = ref.kink_margins(batch, nz)
        assert set(margins) == {'log_std_clip', 'q_tie'} and min(margins.values()) >= (3 if i else 1) * TS.MARGIN, (i, margins)
        if i + 1 < len(noises):
            ref.update(batch, nz)


def test_sac_shape_cases_cover_the_configurations_asked_for():
    kws = [c[5] for c in TS.SHAPE_CASES.values()]
    assert sum(kw.get('backup_entropy', False) for kw in kws) == 1 and sum(not kw.get('tanh_squash', True) for kw in kws) == 1
    assert set(TS.SHAPE_CASES) == {'act16', 'humanoidmaze', 'b1024', 'ragged_depths', 'b272', 'w50_padded'}


# ---- ReBRAC: q1 = q2 at (obs, actor action) --------------------------------------------------------------------------------------------
def _rebrac_seed_holds(od, ad, cfg, params, steps):
    """The admission rule of tests/rebrac_cases.py on the restatement's own trajectory through `steps` ((batch, noise, full_update)
    each): q_tie >= MARGIN in the first step, >= 3 MARGIN in every later full step.  Returns (holds, [q_tie of each full step])."""
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    ties = []
    for i, (batch, noise, full) in enumerate(steps):
        if full:
            m = ref.kink_margins(batch, noise)
            assert set(m) == {'q_tie'}
            ties.append(m['q_tie'])
            if m['q_tie'] < (3 if i else 1) * RC.MARGIN:
                return False, ties
        if i + 1 < len(steps):
            ref.update(batch, noise, full_update=full)
    return True, ties


@pytest.mark.parametrize('case', list(RC.PATHS))
def test_rebrac_path_cases_keep_their_margin_at_the_smallest_seed(case):
    """The recorded data seed keeps the margin through the case's full, critic-only and full step, and no smaller seed does."""
    od, ad = RC.PATHS[case][:2]
    recorded = RC.PATHS[case][6]
    assert 0 <= recorded <= 7 and RC.STEP_KINDS == (True, False, True)
    for seed in range(recorded + 1):
        cfg, batch, params, noises = RC.problem(case, seed)
        assert len(noises) == len(RC.STEP_KINDS)
        holds, ties = _rebrac_seed_holds(od, ad, cfg, params, [(batch, nz, full) for nz, full in zip(noises, RC.STEP_KINDS)])
        print(case, 'seed', seed, 'q_tie of the full steps', ties)
        assert holds == (seed == recorded), (case, seed, ties)


def test_rebrac_batch_size_walk_keeps_its_margin_at_the_smallest_seed():
    od, ad, sizes, recorded = RC.WALK
    for seed in range(recorded + 1):
        cfg, params, steps = RC.walk_problem(seed)
        assert [len(b['observations']) for b, _, _ in steps] == list(sizes) and [f for _, _, f in steps] == [True, False] * 2 + [True]
        holds, ties = _rebrac_seed_holds(od, ad, cfg, params, steps)
        print('walk seed', seed, 'q_tie of the full steps', ties)
        assert holds == (seed == recorded), (seed, ties)


def test_rebrac_kink_margin_is_the_smallest_q_gap_at_the_actor_action():
    """kink_margins against the values the loss itself reads: moving the critic pair apart by d moves q_tie by d."""
    cfg, batch, params, noises = RC.problem('b16')
    od, ad = RC.PATHS['b16'][:2]
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    a = ref._mode(ref.actor_mean('modules_actor', batch['observations']))
    qs = ref._critic('modules_critic', ref._c(batch['observations']), a, stored=True)
    assert ref.kink_margins(batch, noises[0]) == {'q_tie': float(np.abs(qs[0] - qs[1]).min())}
    assert RC.MARGIN == TS.MARGIN == TI.MARGIN


# ---- IFQL: no margins (C1 losses, see tests/ifql_cases.py); the sampler problems are inside the clear-winner cap ---------------------------
@pytest.mark.parametrize('N,n', list(FC.SAMPLER_CASES))
def test_ifql_sampler_problems_at_hidden_512_have_clear_winners(N, n):
    """At least half the rows of each best-of-N problem have a top-two gap above 1e-2 in fp64, so the GPU test's strict branch (pick the
    restatement's action to 2e-5) covers them."""
    cfg, params, obs, noises = FC.sampler_problem(N, n)
    od, ad = FC.SAMPLER_SHAPE[:2]
    assert obs.shape == (n, od) and noises.shape == (n, N, ad) and cfg['num_samples'] == N and cfg['value_hidden_dims'] == (512,) * 4
    ref = FO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    _, _, q = FC.best_of_n(ref, obs, noises)
    clear = FC.clear_winners(q)
    print(f'N {N} n {n}: clear-winner share {clear.mean():.3f}, score spread {q.std():.3f}')
    assert FC.SAMPLER_GAP == 1e-2 and clear.mean() >= 0.5, clear.mean()


def test_ifql_and_rebrac_case_tables_hold_the_cases_asked_for():
    assert list(FC.PATHS) == ['b512_mixed', 'b272', 'b544_h64', 'b1040_h64', 'b2048_h64', 'wide1024', 'obs600', 'no_ln_h512', 'act16', 'b16',
                              'w50_padded', 'w500_padded']
    assert list(RC.PATHS) == ['b272', 'obs50', 'b1040_h64', 'b2048_h64', 'wide1024', 'obs600', 'no_ln_h512_no_tanh', 'b16', 'w50_padded']
    assert list(FC.SAMPLER_CASES) == [(1, 37), (7, 590), (65, 64)] and FC.SAMPLER_SHAPE[:2] == (69, 21)
    big = 1024 * 512 ** 2   # no new case costs more than the existing b1024 cases: B x H^2
    for table in (FC.PATHS, RC.PATHS):
        for name, (od, ad, B, actor, value, kw, seed) in table.items():
            assert B * max(actor + value) ** 2 <= big, name
    for case in FC.PATHS:
        cfg, batch, params, noises = FC.problem(case)
        od, ad, B = FC.PATHS[case][:3]
        assert batch['observations'].shape == (B, od) and noises[0]['x0'].shape == (B, ad) and len(noises) == 2
        assert not np.array_equal(noises[0]['x0'], noises[1]['x0'])
