"""CPU: the conditions under which tests/test_gpu_conditioning.py says anything, checked on the problems exactly as the GPU test builds
them (tests/conditioning_cases.py: the same functions, no engine).

  cap          for every offset and Q-offset case, every leaf and info: 2 x yardstick <= 1e-3 of the leaf's largest gradient, or of
               max(1, |info|).  Above that a comparison says nothing and the case has to be rebuilt; this is a condition on the inputs.
  regime       at every LayerNorm input of a c = 10 case's fp64 pass, |row mean| / row std >= 5 (the combined case: all but LayerNorm_0,
               whose input is the 5 obs + 30 layer), so the one-pass variance loses a factor 25 and more on every such row; and the
               pairwise figure of the worst critic leaf is at least twice that of the same problem without the offset (the twin
               `<base>/plain`), that is, the offset adds at least as much fp32 error as every other source together: otherwise the case
               would test nothing new.  Measured 2.3 (side64, B 1088) to 31 (kbig).  Printed, not asserted: the quantities whose
               tolerance is the measured one (none at side64: there the plain bounds hold on ill-conditioned rows).
               The scaled-observation cases: every tolerance, leaf and info, is the plain one.
               For the Q-offset cases |mean q| >= 150 and |mean q| / median|q - target| >= 50 in fp64: the residual the critic's
               gradient starts from is a difference of two numbers 50 and more times its size.
  dead layer   in fp64 the rstd of the dead LayerNorm_1 is 1 / sqrt(1e-6) within 1e-6 relative, in every case.  At c = 30 and width
               250 both sequential fp32 variants give an unclamped variance below -1e-6, so var + eps < 0 (-6.1e-5 and -7.2e-5: 7500 x
               fp32(1 / 250) rounds to 30.000002; the row sums 7500 and 225000 are exact in every order, so a kernel has the same).
               The four CLAMP_CASES, width 250 on the 16-row kernel, the 32-row tiles, the 64-row tiles and the split 32-row tiles,
               each exercise their site's clamp.  At widths 256 and 64 both forms are exactly 0, since 30 w / w and 900 w / w are
               exact there: rows16 / side32 / side64 at c = 30 pin rstd = 1000 and the bounded upstream gradients, not a clamp.
  kinks        every FQL case keeps MARGIN = 1e-3 from |a| = 1 of the one-step actor's output and, under q_agg='min', from q1 = q2 of
               the target pair; the IQL cases keep it from every kink of tests/iql_oracle.py's kink_margins.

Departure from the figures the cases were proposed with.  Those (gradient error 1.3e-5 to 5.5e-5 pairwise at c = 10, 1.0e-5 at a
head bias of -200) were measured at B 32; the error of a leaf's gradient is an average over the batch rows and falls with B.  At the
batch sizes that reach the LayerNorm sites (144 to 1088) the pairwise figure of the worst critic leaf is 2.3e-6 to 9.6e-6 at c = 10
(3.1e-5 at kbig, B 32) and 0.9e-6 to 1.6e-6 at q0 = -200 / -1000, so "pairwise above 2e-5" and "above 5e-6" cannot hold with c, q0 and
the shapes as they are set; the regime is asserted in the forms above instead, and the figures are printed.

What the comparisons catch, each mistake made in a copy of the oracle's layer_norm (mistaken_layer_norm, sequential_layer_norm(clamp=
False)) and measured against the case's own tolerance by test_a_mistake_in_the_statistics_is_far_outside_the_tolerance:
  one zero pad column counted into both sums, width 50 (padded/c10)        worst leaf 2.3e4 x its tolerance
  the last 32-column partial dropped, width 256 (side32/c10)                worst leaf 4.9e4 x its tolerance
  no max(0, .) at the dead layer, c = 30, width 250 (each CLAMP_CASES entry)  NaN in every downstream leaf
"""
import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import conditioning_cases as CC
from tests.util import leaf_dict

C10 = [n for n in CC.OFFSET_CASES if n in CC.GPU_CASES] + ['iql/c10', 'bc/c10']
QOFF = [n for n in CC.Q_CASES if n in CC.GPU_CASES] + ['iql/q200']
CAPPED = sorted(set(C10 + QOFF))


def _is_critic(path):
    return path.startswith('modules_critic') or path.startswith('MLP_0') or path.startswith('Dense_0')   # (BC's one net)


def _plain_twin(name):
    return name.split('/')[0] + '/plain'


def test_the_case_table_holds_the_cases_asked_for():
    K = CC.FQL_CASES
    assert {n for n in CC.GPU_CASES if K[n]['c'] is not None and K[n]['q0'] is None} == {
        f'{b}/c10' for b in ('rows16', 'side32', 'side32_h64', 'side64', 'split', 'kbig', 'padded', 'chain_ln')}
    assert all(K[n]['c'] == 10.0 for n in CC.OFFSET_CASES)
    q = {(K[n]['base'].split('_')[0], K[n]['q0']) for n in CC.GPU_CASES if K[n]['q0'] is not None and K[n]['c'] is None}
    assert q == {('rows16', -200.0), ('rows16', -1000.0), ('side32', -200.0), ('side32', -1000.0)}
    assert all(K[n]['cfg']['discount'] == 0.995 for n in CC.Q_CASES)
    assert any(K[n]['cfg'].get('normalize_q_loss') and K[n]['cfg'].get('q_agg') == 'min' for n in CC.Q_CASES)
    assert {K[n]['base'] for n in CC.SCALED_ONLY} == {'rows16', 'side32'}
    assert K['side32/c10_q200_scaled'] == dict(base='side32', c=10.0, q0=-200.0, scaled=True, dead=None, cfg=CC.Q_CFG, seed=5)
    assert {(K[n]['base'], K[n]['dead']) for n in CC.DEAD_CASES} == {(b, c) for b in ('rows16', 'side32', 'side64', 'padded250')
                                                                    for c in (0.0, 30.0)} | {
        (b, 30.0) for b in ('side32_w250', 'side64_w250', 'split_w250')}
    assert CC.CLAMP_CASES == ['padded250/dead30', 'side32_w250/dead30', 'side64_w250/dead30', 'split_w250/dead30']
    assert [CC.BASES[b][0] for b in ('side32_w250', 'side64_w250', 'split_w250')] == [256, 1088, 256]
    assert CC.BASES['rows16'][:2] == (144, (256,) * 3) and CC.BASES['side64'][:2] == (1088, (64,) * 3)
    assert CC.BASES['split'][2] == dict(precision='bf16x3') and CC.BASES['chain_ln'][2] == dict(actor_layer_norm=True)
    assert all(w % 16 for w in CC.BASES['padded'][1] + CC.BASES['padded250'][1]) and max(CC.BASES['kbig'][1]) > 512
    assert all(B <= 1088 for B, _, _ in CC.BASES.values())
    assert (CC.FACTOR, CC.CAP, CC.GRAD_BOUND, CC.INFO_RTOL, CC.INFO_ATOL) == (2.0, 1e-3, 2e-5, 5e-5, 5e-6)


def test_the_builders_move_what_they_name_and_nothing_else():
    cfg, batch, noise, plain = CC.fql_problem('chain_ln/plain')
    moved = leaf_dict(CC.offset_params(plain, 10.0, ('modules_critic',) + CC.ACTORS))
    for p, v in leaf_dict(plain).items():
        hidden_bias = p.endswith('/bias') and 'Dense_' in p and not p.endswith('Dense_3/bias')
        np.testing.assert_array_equal(moved[p], v + np.float32(10.0) if hidden_bias else v, err_msg=p)
    moved = leaf_dict(CC.q_offset(plain, -200.0))
    for p, v in leaf_dict(plain).items():
        head = p in ('modules_critic/value_net/Dense_3/bias', 'modules_target_critic/value_net/Dense_3/bias')
        np.testing.assert_array_equal(moved[p], v + np.float32(-200.0) if head else v, err_msg=p)
    dead = CC.dead_layer(plain, 30.0)
    for m in CC.CRITICS:
        d = dead[m]['value_net']['Dense_1']
        assert d['kernel'].shape == (2, 256, 256) and not d['kernel'].any() and (d['bias'] == np.float32(30.0)).all()
    sb = CC.scaled_obs(batch)
    np.testing.assert_array_equal(sb['observations'], np.float32(5) * batch['observations'] + np.float32(30))
    np.testing.assert_array_equal(sb['next_observations'], np.float32(5) * batch['next_observations'] + np.float32(30))
    np.testing.assert_array_equal(sb['actions'], batch['actions'])


def test_the_swapped_layer_norm_is_restored_and_touches_fp32_only():
    orig = O.layer_norm
    with pytest.raises(RuntimeError):
        with CC.variant_context('sequential'):
            assert O.layer_norm is not orig
            raise RuntimeError
    assert O.layer_norm is orig
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 80)) + 10.0
    g, b = rng.standard_normal(80), rng.standard_normal(80)
    for fused in (False, True):
        f = CC.sequential_layer_norm(fused)
        for got, want in zip(f(x, g, b), orig(x, g, b)):
            np.testing.assert_array_equal(got, want)                              # fp64 goes to the oracle's own
        x32, g32, b32 = x.astype(np.float32), g.astype(np.float32), b.astype(np.float32)
        y, xhat, rstd = f(x32, g32, b32)
        assert y.dtype == xhat.dtype == rstd.dtype == np.float32
        np.testing.assert_allclose(y, orig(x, g, b)[0], rtol=0, atol=2e-3)       # (mean / std)^2 = 100 times fp32's rounding, scaled
        assert np.abs(y - orig(x32, g32, b32)[0]).max() > 0                      # and not the pairwise sums
    CC.yardstick('padded/c10')
    assert O.layer_norm is orig


@pytest.mark.parametrize('name', CAPPED)
def test_cap_twice_the_yardstick_stays_below_1e_3(name):
    y = CC.yardstick(name)
    i64 = y.truth.update()[1]
    worst_g = max(y.grads.values())
    worst_i = max(y.infos[k] / max(1.0, abs(i64[k])) for k in i64)
    print(f'{name}: pairwise {y.worst("pairwise")[0]:.2e} sequential {y.worst("sequential")[0]:.2e} fused {y.worst("fused")[0]:.2e}'
          f' worst leaf {worst_g:.2e}, worst info / max(1, |info|) {worst_i:.2e}')
    for p, e in y.grads.items():
        assert CC.FACTOR * e <= CC.CAP, (p, e)
    for k, e in y.infos.items():
        assert CC.FACTOR * e <= CC.CAP * max(1.0, abs(i64[k])), (k, e, i64[k])


@pytest.mark.parametrize('name', C10)
def test_offset_cases_reach_the_ill_conditioned_regime(name):
    ratios = [r for r, _ in CC.layer_norm_inputs(name)]
    y, y0 = CC.yardstick(name), CC.yardstick(_plain_twin(name))
    g64, i64 = leaf_dict(y.truth.grads()[2]), y.truth.update()[1]
    critic = [p for p in y.grads if _is_critic(p) and np.abs(g64[p]).max() > 0]
    worst, worst0 = max(y.grad['pairwise'][p] for p in critic), max(y0.grad['pairwise'][p] for p in critic)
    print(f'{name}: |mean| / std {min(ratios):.2f} .. {max(ratios):.2f}; pairwise worst critic leaf {worst:.2e}, without the offset '
          f'{worst0:.2e} (x {worst / worst0:.1f})')
    if 'scaled' in name:   # the first layer's input is 5 obs + 30: its LayerNorm is not an offset one (one call in three per net and pass)
        assert sum(r >= 5.0 for r in ratios) >= 2 * len(ratios) // 3, ratios
    else:
        assert min(ratios) >= 5.0, ratios
    assert worst >= 2.0 * worst0, (worst, worst0)
    floor = CC.grad_floor(name)
    measured = [p for p in critic if CC.FACTOR * y.grads[p] > floor]
    measured += [k for k in i64 if (k.startswith('critic/') or k == 'bc_loss') and CC.FACTOR * y.infos[k] > CC.info_floor(name, i64[k])]
    print(f'{name}: tolerance above the plain bound for {len(measured)} critic quantities', measured[:4])


@pytest.mark.parametrize('name', CC.SCALED_ONLY + ['bc/scaled'])
def test_scaled_observation_cases_keep_the_plain_tolerances(name):
    y = CC.yardstick(name)
    i64 = y.truth.update()[1]
    assert all(y.grad_tol(p, CC.grad_floor(name)) == CC.grad_floor(name) for p in y.grads)
    assert all(y.info_tol(k, CC.info_floor(name, w)) == CC.info_floor(name, w) for k, w in i64.items())


@pytest.mark.parametrize('name', QOFF)
def test_q_offset_cases_subtract_two_large_numbers(name):
    y = CC.yardstick(name)
    i64 = y.truth.update()[1]
    q, rms = CC.q_cancellation(name)
    print(f'{name}: |mean q| {q:.1f}, median |q - target| {rms:.3f}; pairwise worst leaf {y.worst("pairwise")[0]:.2e}, '
          f'critic_loss error {y.infos["critic/critic_loss"]:.2e}')
    assert q >= 150.0 and q / rms >= 50.0, (q, rms)


@pytest.mark.parametrize('name', CC.DEAD_CASES)
def test_dead_layer_has_rstd_1000_and_the_clamp_cases_need_the_clamp(name):
    c = CC.FQL_CASES[name]['dead']
    rstds = [r for ratio, r in CC.layer_norm_inputs(name) if np.allclose(r, r.flat[0]) and r.flat[0] > 900.0]
    assert len(rstds) == 6       # two members in the target pass, the critic pass and the actor's Q pass
    for r in rstds:
        np.testing.assert_allclose(r, 1.0 / np.sqrt(1e-6), rtol=1e-6)
    for fused in (False, True):
        raws = CC.dead_layer_raw_variance(name, fused)
        assert len(raws) == 6
        lo, hi = min(float(r.min()) for r in raws), max(float(r.max()) for r in raws)
        print(f'{name} {"fused" if fused else "two roundings"}: unclamped variance {lo:.3e} .. {hi:.3e}')
        if name in CC.CLAMP_CASES:
            assert hi < -CC.O.LN_EPS, 'var + eps >= 0 on some row: the case does not need the clamp'
        else:
            assert lo == hi == 0.0


@pytest.mark.parametrize('name', CC.CLAMP_CASES)
def test_dead_layer_without_the_clamp_is_nan(name):
    with CC.swapped_layer_norm(CC.sequential_layer_norm(False, clamp=False)):
        ref, batch, noise = CC.fql_oracle(name, np.float32)
        with np.errstate(invalid='ignore'):
            g = leaf_dict(ref.grads(batch, noise)[2])
    assert all(np.isnan(g[f'modules_critic/value_net/{leaf}']).all() for leaf in ('Dense_2/kernel', 'Dense_3/kernel', 'LayerNorm_1/bias'))
    assert all(np.isfinite(v).all() for v in leaf_dict(CC.yardstick(name).truth.grads()[2]).values())


@pytest.mark.parametrize('name,kind,least', [('padded/c10', 'pad_column', 1e3), ('side32/c10', 'drop_partial', 1e4)])
def test_a_mistake_in_the_statistics_is_far_outside_the_tolerance(name, kind, least):
    y = CC.yardstick(name)
    g64 = leaf_dict(y.truth.grads()[2])
    with CC.swapped_layer_norm(CC.mistaken_layer_norm(kind)):
        ref, batch, noise = CC.fql_oracle(name, np.float64)
        g = leaf_dict(ref.grads(batch, noise)[2])
    factor = max(np.abs(g[p] - g64[p]).max() / (y.grad_tol(p) * np.abs(g64[p]).max()) for p in g64 if p.startswith('modules_critic'))
    print(f'{name} {kind}: worst critic leaf at {factor:.3g} times its tolerance')
    assert factor >= least


@pytest.mark.parametrize('name', CC.GPU_CASES)
def test_fql_cases_keep_their_kink_margins(name):
    m = CC.fql_kink_margins(name)
    assert ('q_tie' in m) == (CC.FQL_CASES[name]['cfg'].get('q_agg') == 'min')
    assert min(m.values()) >= CC.MARGIN, m


@pytest.mark.parametrize('name', ['iql/c10', 'iql/q200'])
def test_iql_cases_keep_their_kink_margins(name):
    ref, batch, noise = CC.iql_oracle(name, np.float64)
    m = ref.kink_margins(batch, noise)
    assert set(m) == {'expectile', 'log_stds', 'q_tie', 'unit_clip'} and min(m.values()) >= CC.MARGIN, m
    assert 0.2 <= np.mean(np.abs(ref._forward(batch, noise)['x']) > 1.0) <= 0.8      # both branches of the clip mask are live


def test_forward_yardstick_is_inside_the_cap():
    want, err = CC.forward_yardstick()
    print('forward yardstick', err)
    assert set(err) == {'sample_actions', 'compute_flow_actions', 'critic'}
    for q, e in err.items():
        assert CC.FACTOR * e <= CC.CAP * max(1.0, float(np.abs(want[q]).max())), (q, e)
