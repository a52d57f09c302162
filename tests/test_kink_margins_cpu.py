"""CPU: the inputs of the IQL and SAC shape cases (tests/test_gpu_iql.py, tests/test_gpu_sac.py) are clear of the losses' kinks.

The GPU tests compare every element of every gradient with the fp64 restatement and mask nothing out, which is sound only where the
restatement itself is a margin away from each point where a loss is not smooth: an element that sits on a kink may fall on the other
side in fp32 and take the other branch's gradient.  Each case's seeds were chosen for that; this file builds every problem exactly as
the GPU test does (the same functions, no engine) and asserts the margins in every step, so the choice can be checked on any machine.

A step after the first runs, on the GPU, from the engine's own state (tests/util.py sync_restatement), which parts from the
restatement's trajectory by up to 2 lr per element; there the restatement's own trajectory must keep 3 times the margin.
"""
import numpy as np
import pytest

from tests import iql_oracle as IO
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
    assert set(TS.SHAPE_CASES) == {'act16', 'humanoidmaze', 'b1024', 'ragged_depths', 'b272'}
