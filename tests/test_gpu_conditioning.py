"""GPU: the update and forward kernels on ill-conditioned rows (tests/conditioning_cases.py): LayerNorm inputs with |mean| / std of 7 to 16
(c = 10 on every hidden Dense bias), Q near -200 and -1000, observations 5 obs + 30, and a dead layer whose LayerNorm input has true variance
0.  One update from zero moments against the fp64 oracle on identical parameters, batch and noise: the infos, every leaf's gradient as
mu / 0.1, nu, and (FQL, fp32) the post-step parameters, as tests/util.py's assert_step_matches does, with per-quantity tolerances
tol = max(existing bound, 2 x yardstick), the yardstick being the error of plain fp32 numpy on the same inputs in three summation orders
(conditioning_cases.Yardstick; tests/test_conditioning_cpu.py holds the conditions under which that says anything).  Each case first
asserts from the engine's plan (fql_debug_plan, tests/util.py read_plan) that the launches it is named for are there, and prints it.

  rows16      B 144, hidden 256 x 3       the 16-row Dense kernel's LDS statistics only, no 32- or 64-row task
  side32      B 256, hidden 256 x 3       32-row tiles folding 8 partials per row; side32_h64 (hidden 64 x 3): 2 partials
  side64      B 1088, hidden 64 x 3       fql_side_big_kernel, 17 row tiles
  split       side32 in bf16x3            split tiles and split chain; floor BF16X3_BOUND
  kbig        B 32, hidden 1024 x 3       the K > 512 kernels
  padded      B 32, hidden 50 x 3         ln_width 50 of 64 columns; padded250 (250 x 3): ln_width 250 of 256, the dead layer's clamp
  chain_ln    rows16 with actor LayerNorm the actor nets' LayerNorm, actors offset too.  Proposed for "the chain's LayerNorm forward and
                                          fused backward"; the engine has neither: the Euler chain is refused under actor_layer_norm
                                          (build_chain_weights) and fql_chain.h's variant 4, the one chain variant that reads (mean, rstd),
                                          is launched by no program.  The case asserts that there is no chain and runs where the plan puts it:
                                          the 16-row Dense kernel and the LayerNorm-backward riders, for all five LayerNorm'd nets at once.

Dead layer (critic Dense_1 kernel 0, bias c): at c = 0 the plain tolerances; at c = 30 everything finite, infos and the leaves
downstream of LayerNorm_1 within tolerance, and the leaves upstream of it bounded by twice the fp64 gradient (with the clamp rstd <=
1 / sqrt(eps), fp64's value).  At widths 256 and 64 the fp32 variance of a row of 30s is exactly 0 in every order, so rows16, side32
and side64 at c = 30 reach no clamp.  The clamp cases are the four at width 250, where 7500 x fp32(1 / 250) = 30.000002 makes
E[x^2] - E[x]^2 = -6e-5 and a site without max(0, .) gives NaN, one per site that computes a variance:
  padded250    B 32                       the 16-row Dense kernel (gemm16_body)
  side32_w250  B 256                      the 32-row tiles (gemm32_body)
  side64_w250  B 1088                     fql_side_big_kernel's 64-row tiles (gemm64_body)
  split_w250   B 256, bf16x3              the split 32-row tiles (gemm32s_body)
What these four pin is finiteness and the upstream bound.  Their comparison of infos and downstream leaves follows the same formula,
but plain fp32 itself is off by 2.7e-2 there (xhat = (30 - 30.000002) x 1000 where fp64 has 0), 50 times the 1e-3 cap above which a
comparison says nothing: that part has no discriminating power and is kept only for uniformity.

IQL (ddpgbc with log_stds, actor LayerNorm) and BC get one offset case each, IQL a large-return case (q0 = -200 on critic, target critic
and value net), BC a scaled-observation case; BC has no critic and therefore no large-return case.  Both oracles
run in fp32, so both have a yardstick.

Measured on an MI355X (worst over the leaves of max|g - g64| / max|g64|; worst info error / max(1, |info|); `of tol` the worst
error / tolerance over every compared quantity; GPU / envelope the ratio of the two worst gradient figures); figures, not bounds:
  case                     pairwise  sequential  GPU gradient  GPU info  GPU / envelope  of tol
  rows16/c10               7.4e-06   3.4e-05     6.8e-06       1.4e-05   0.20            0.26
  side32/c10               5.5e-06   3.0e-05     4.2e-06       1.2e-05   0.14            0.23
  side32_h64/c10           4.7e-06   1.4e-05     5.1e-06       3.6e-06   0.37            0.23
  side64/c10               2.3e-06   7.4e-06     2.8e-06       1.0e-05   0.37            0.20
  split/c10                5.5e-06   3.0e-05     8.6e-06       6.5e-06   0.28            0.09
  kbig/c10                 3.1e-05   1.1e-04     1.5e-05       8.0e-06   0.13            0.28
  padded/c10               9.6e-06   4.4e-05     9.0e-06       1.4e-05   0.20            0.28
  chain_ln/c10             9.6e-06   6.3e-05     1.1e-05       1.3e-06   0.18            0.17
  rows16/q200              1.3e-06   1.5e-06     8.5e-07       1.6e-07   0.57            0.04
  rows16/q1000_norm_min    1.2e-06   1.0e-06     6.0e-07       1.1e-07   0.51            0.03
  side32/q200_norm_min     1.5e-06   1.5e-06     8.0e-07       3.0e-07   0.52            0.04
  side32_h64/q1000         9.4e-07   1.0e-06     7.3e-07       3.2e-07   0.70            0.04
  rows16/scaled            5.8e-07   6.9e-07     3.0e-07       2.2e-07   0.44            0.02
  side32/scaled            6.9e-07   7.1e-07     2.6e-07       2.2e-07   0.36            0.01
  side32/c10_q200_scaled   5.7e-06   5.0e-05     3.8e-06       1.6e-07   0.08            0.19
  rows16/dead0             2.1e-06   2.0e-06     1.1e-06       1.0e-06   0.54            0.06
  rows16/dead30            2.1e-06   2.0e-06     1.1e-06       1.0e-06   0.54            0.06
  side32/dead0             3.8e-06   3.5e-06     8.7e-07       4.4e-07   0.23            0.04
  side32/dead30            3.8e-06   3.5e-06     8.7e-07       4.4e-07   0.23            0.04
  side64/dead0             1.4e-05   1.4e-05     2.4e-06       5.5e-07   0.17            0.12
  side64/dead30            1.4e-05   1.4e-05     2.4e-06       3.3e-07   0.17            0.12
  padded250/dead0          8.1e-07   6.5e-07     6.4e-07       5.9e-07   0.79            0.03
  padded250/dead30         8.1e-07   2.7e-02     2.7e-02       2.3e-02   1.00            0.50
  side32_w250/dead30       3.2e-06   2.7e-02     2.7e-02       2.3e-02   1.00            0.50
  side64_w250/dead30       1.4e-05   2.7e-02     2.7e-02       2.3e-02   1.00            0.50
  split_w250/dead30        3.2e-06   2.7e-02     2.7e-02       2.3e-02   1.00            0.50
  iql/c10                  6.8e-06   3.1e-05     8.8e-06       6.9e-06   0.28            0.18
  iql/q200                 4.4e-06   4.0e-06     4.7e-06       5.3e-07   1.07            0.09
  bc/c10                   1.4e-05   3.0e-05     8.1e-06       5.6e-07   0.27            0.20
  bc/scaled                4.2e-07   4.0e-07     2.6e-07       7.2e-08   0.63            0.01

  forward sample_actions n=1           yardstick 6.3e-05  GPU 4.1e-06  of tol 0.03
  forward sample_actions n=5           yardstick 6.3e-05  GPU 8.0e-06  of tol 0.06
  forward sample_actions n=33          yardstick 6.3e-05  GPU 1.3e-05  of tol 0.10
  forward compute_flow_actions n=1     yardstick 4.2e-05  GPU 0.0e+00  of tol 0.00
  forward compute_flow_actions n=5     yardstick 4.2e-05  GPU 3.1e-06  of tol 0.04
  forward compute_flow_actions n=33    yardstick 4.2e-05  GPU 5.8e-06  of tol 0.07
  forward critic n=1                   yardstick 1.8e-04  GPU 2.7e-06  of tol 0.01
  forward critic n=5                   yardstick 1.8e-04  GPU 1.6e-05  of tol 0.04
  forward critic n=33                  yardstick 1.8e-04  GPU 4.2e-05  of tol 0.12
  bc/c10 sampler                       yardstick 1.8e-05  GPU 5.2e-06  of tol 0.15
  bc/scaled sampler                    yardstick 6.2e-07  GPU 5.5e-07  of tol 0.03
(the forward rows and the BC sampler: yardstick, the GPU's worst element error, its share of the tolerance.  The four clamp
cases: the sequential orders and the GPU both have mean = 30.000002 at the dead layer, so xhat = -1.9e-3 where fp64 has 0; the GPU
lands on the sequential figure itself at every site.  Upstream of that layer the GPU's largest gradients (Dense_1 bias, kernel) are
2.508e3, 2.705e3 at padded250, 2.527e3, 1.905e3 at side32_w250 and split_w250, 2.491e3, 1.664e3 at side64_w250, each 1.02 times
fp64's, at a bound of twice; at widths 256 and 64 they equal fp64's to four digits.  iql/q200: GPU / envelope
1.07 is 4.7e-6 against 4.4e-6, a tenth of the 5e-5 floor.)  No case failed on a kernel and no kernel changed.
"""
import numpy as np
import pytest

from tests import conditioning_cases as CC
from tests.util import (K_CHAIN_SPLIT, K_GEMM16, K_GEMM16_EULER, K_GEMM16_KBIG, K_SIDE, K_SIDE_BIG, K_SIDE_SPLIT, leaf_dict,
                        plan_gemm, plan_ln, print_plan, read_plan)

pytestmark = pytest.mark.gpu

UPDATE_CASES = [n for n in CC.GPU_CASES if CC.FQL_CASES[n]['dead'] is None]
UPSTREAM = ('Dense_0/', 'LayerNorm_0/', 'Dense_1/')                     # of the dead layer's LayerNorm_1, in the critic


# ---- where a case runs -----------------------------------------------------------------------------------------------------------------
def _chains(plan):
    return [dict(L['chain'], kernel=L['kernel']) for L in plan if L['chain'] is not None]


def _p_rows16(plan, B):
    assert not [t for t in plan_gemm(plan) if t['rows'] in (32, 64)] and all(L['kernel'] != K_SIDE_BIG for L in plan)
    hid = [t for t in plan_gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if (t['N'], t['K']) == (256, 256)]
    assert hid and all(t['rows'] == 16 and t['M'] % B == 0 for t in hid)


def _p_side32(plan, B, H=256, kernel=K_SIDE):
    assert [t for t in plan_gemm(plan, (kernel,)) if t['rows'] == 32 and (t['N'], t['K']) == (H, H) and t['M'] % B == 0]


def _p_side64(plan, B, H=64):
    assert [t for t in plan_gemm(plan, (K_SIDE_BIG,)) if t['rows'] == 64 and t['M'] == B and (t['N'], t['K']) == (H, H)] and B // 64 == 17


def _p_split(plan, B):
    _p_side32(plan, B, kernel=K_SIDE_SPLIT)
    ch = _chains(plan)
    assert ch and any(c['split'] for c in ch) and all((c['kernel'] == K_CHAIN_SPLIT) == bool(c['split']) for c in ch)


def _p_kbig(plan, B):
    assert [t for t in plan_gemm(plan, (K_GEMM16_KBIG,)) if (t['N'], t['K']) == (1024, 1024) and t['rows'] == 16]


def _p_padded(plan, B, wp=64):
    assert [t for t in plan_gemm(plan, (K_GEMM16, K_GEMM16_EULER)) if (t['N'], t['K']) == (wp, wp) and t['rows'] == 16]
    assert B in plan_ln(plan) and not _chains(plan)                    # LayerNorm-backward over `width` of wp columns; no chain


def _p_chain_ln(plan, B):
    """build_chain_weights admits the Euler chain without actor LayerNorm only, and no program launches the chain kernel's variant with
    a LayerNorm backward in its prologue (fql_chain.h, variant 4), so there is no chain here: the three actor nets' LayerNorm runs in the
    16-row Dense kernel's prologue and their backward as riders of the side launches, next to the critic's."""
    _p_rows16(plan, B)
    assert not _chains(plan) and B in plan_ln(plan)


PROPERTY = {'rows16': _p_rows16, 'side32': _p_side32, 'side32_h64': lambda p, B: _p_side32(p, B, 64), 'side64': _p_side64,
            'split': _p_split, 'kbig': _p_kbig, 'padded': _p_padded, 'padded250': lambda p, B: _p_padded(p, B, 256), 'chain_ln': _p_chain_ln,
            # width 250 of 256 columns on the tiles: the GEMMs that normalise their input (Dense_1, Dense_2) are the [*, 256, 256] tasks
            'side32_w250': _p_side32, 'side64_w250': lambda p, B: _p_side64(p, B, 256),
            'split_w250': lambda p, B: _p_side32(p, B, kernel=K_SIDE_SPLIT)}


def _fql_agent(name):
    import fql_amd
    cfg, batch, noise, params = CC.fql_problem(name)
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    agent.set_params(params)
    base = CC.FQL_CASES[name]['base']
    plan = read_plan(agent)
    print_plan(name, plan)
    PROPERTY[base](plan, CC.BASES[base][0])
    return cfg, batch, noise, params, agent


# ---- one update against the fp64 oracle, tolerances passed in -------------------------------------------------------------------------
def _step(name, agent, batch, noise, lr=None, only=None, finite_only=()):
    """assert_step_matches' structure with the case's tolerances.  only: a predicate on the leaf path (default: every leaf is compared);
    finite_only: info keys that are only required to be finite.  Returns the measured figures."""
    y = CC.yardstick(name)
    g_ref, info_ref = leaf_dict(y.truth.grads()[2]), y.truth.update()[1]
    info = agent.update(batch, noise=noise)[1]
    info = agent.read_info() if info is None else info
    info = info.to_dict() if hasattr(info, 'to_dict') else info
    agent.synchronize()
    opt = agent.get_opt_state()
    assert opt['count'] == 1 and opt['step'] == 2
    fig = dict(grad=(0.0, None), info=(0.0, None), of_tol=(0.0, None))
    for k, want in info_ref.items():
        got = float(info[k])
        assert np.isfinite(got), (k, got)
        if k in finite_only:
            continue
        tol, err = y.info_tol(k, CC.info_floor(name, want)), abs(got - want)
        fig['info'] = max(fig['info'], (err / max(1.0, abs(want)), k))
        fig['of_tol'] = max(fig['of_tol'], (err / tol, k))
    mu, nu = leaf_dict(opt['mu']), leaf_dict(opt['nu'])
    new, new_ref = leaf_dict(agent.get_params()), leaf_dict(y.truth.params)
    for p, g in g_ref.items():
        assert np.isfinite(mu[p]).all() and np.isfinite(nu[p]).all() and np.isfinite(new[p]).all(), p
        if only is not None and not only(p):
            continue
        scale = float(np.abs(g).max())
        rel = y.grad_tol(p, CC.grad_floor(name))
        tol = rel * scale + 1e-9
        err = float(np.abs(mu[p] / 0.1 - g).max())
        if scale > 0:
            fig['grad'] = max(fig['grad'], (err / scale, p))
        fig['of_tol'] = max(fig['of_tol'], (err / tol, p))
        if lr is None:
            continue
        # nu = 0.001 g^2: an error d <= tol of g moves it by 2 |g| d + d^2 <= tol scale + 2 rel g^2 (assert_step_matches' form; its rtol
        # 1e-4 is 2 rel at the plain bound and beyond)
        assert (np.abs(nu[p] / 0.001 - g * g) <= tol * scale + 1e-12 + max(1e-4, 2.0 * rel) * g * g).all(), f'nu {p}'
        # assert_step_matches' parameter bounds plus one fp32 spacing of the parameter: a head bias of -200 or -1000 is stored to 1.5e-5 or
        # 6.1e-5, more than the bounds themselves
        d = np.abs(new[p] - new_ref[p])
        d = d - np.where(np.abs(new_ref[p]) > 1.0, np.spacing(np.abs(new_ref[p]).astype(np.float32)), 0.0)    # (other leaves: unchanged)
        if 'target' in p:
            assert d.max() <= 1e-6, p
        else:
            assert d[np.abs(g) > 50 * tol].max(initial=0) <= 2e-6, p
            assert d.max() <= 2 * lr + 1e-6, p
    return y, fig


def _report(name, y, fig):
    pw, sq = y.worst('pairwise')[0], max(y.worst('sequential')[0], y.worst('fused')[0])
    print(f'{name}: yardstick pairwise {pw:.1e} sequential {sq:.1e} | GPU gradient {fig["grad"][0]:.1e} ({fig["grad"][1]}) info '
          f'{fig["info"][0]:.1e} ({fig["info"][1]}) | of tol {fig["of_tol"][0]:.2f} ({fig["of_tol"][1]}) | GPU / envelope '
          f'{fig["grad"][0] / max(pw, sq):.2f}')
    assert fig['of_tol'][0] <= 1.0, fig['of_tol']


@pytest.mark.parametrize('name', UPDATE_CASES)
def test_update_matches_fp64_within_twice_plain_fp32(name):
    cfg, batch, noise, params, agent = _fql_agent(name)
    y, fig = _step(name, agent, batch, noise, lr=None if CC.is_split(name) else cfg['lr'])
    if name in CC.SCALED_ONLY:      # scaled observations do not hurt fp32: every tolerance, leaf and info, is the plain one
        assert all(y.grad_tol(p) == CC.GRAD_BOUND for p in y.grads)
        assert all(y.info_tol(k, CC.info_floor(name, w)) == CC.INFO_ATOL + CC.INFO_RTOL * abs(w) for k, w in y.truth.update()[1].items())
    _report(name, y, fig)
    agent.close()


@pytest.mark.parametrize('name', CC.DEAD_CASES)
def test_dead_layer_stays_finite_and_bounded(name):
    cfg, batch, noise, params, agent = _fql_agent(name)
    if CC.FQL_CASES[name]['dead'] == 0.0:   # everything is exact and the gradient well defined: the full comparison
        y, fig = _step(name, agent, batch, noise, lr=cfg['lr'])
        _report(name, y, fig)
        agent.close()
        return
    upstream = lambda p: p.startswith('modules_critic/') and any(u in p for u in UPSTREAM)      # noqa: E731
    # LayerNorm_1/scale is neither side: its fp64 gradient sum dy xhat is 0 (xhat = 0), in fp32 xhat is (30 - mean) rstd: finite only
    skipped = lambda p: upstream(p) or p == 'modules_critic/value_net/LayerNorm_1/scale'        # noqa: E731
    # the three gradient statistics take in the upstream leaves, which are bounded from above only
    y, fig = _step(name, agent, batch, noise, only=lambda p: not skipped(p), finite_only=('grad/max', 'grad/min', 'grad/norm'))
    g64, mu = leaf_dict(y.truth.grads()[2]), leaf_dict(agent.get_opt_state()['mu'])
    for p in g64:
        if upstream(p):
            got, cap = float(np.abs(mu[p] / 0.1).max()), 2.0 * float(np.abs(g64[p]).max())
            print(f'{name} {p}: max|g| {got:.3e}, fp64 {cap / 2:.3e}')
            assert np.isfinite(got) and got <= cap + 1e-9, (p, got, cap)
    _report(name, y, fig)
    agent.close()


# ---- forward paths on the offset parameters ------------------------------------------------------------------------------------------
def test_forward_queries_on_offset_rows():
    """sample_actions, compute_flow_actions and the critic query at n = 1, 5 and 33 against the fp64 oracle, on chain_ln/c10's parameters
    (every net offset); row j of the n = 33 call is bitwise the single-row call."""
    cfg, batch, noise, params, agent = _fql_agent(CC.FORWARD_CASE)
    want, yard = CC.forward_yardstick()
    obs, z, act = CC.forward_rows(33)
    query = {'sample_actions': lambda n: agent.sample_actions(obs[:n], noises=z[:n]),
             'compute_flow_actions': lambda n: agent.compute_flow_actions(obs[:n], z[:n]),
             'critic': lambda n: agent.network.select('critic')(obs[:n], actions=act[:n])}
    floor = {'sample_actions': lambda w: CC.SAMPLE_ATOL + 0 * w, 'compute_flow_actions': lambda w: CC.FLOW_ATOL + 0 * w,
             'critic': lambda w: CC.QUERY_ATOL + CC.QUERY_RTOL * np.abs(w)}
    for q, f in query.items():
        rows = (lambda a, n: a[..., :n]) if q == 'critic' else (lambda a, n: a[:n])
        big = None
        for n in CC.FORWARD_NS:
            got = f(n)
            w = rows(want[q], n)
            assert got.shape == w.shape and got.dtype == np.float32, (q, n, got.shape)
            tol = np.maximum(floor[q](w), CC.FACTOR * yard[q])
            ratio = float((np.abs(got - w) / tol).max())
            print(f'forward {q} n={n}: yardstick {yard[q]:.1e}, GPU worst error {np.abs(got - w).max():.1e}, of tol {ratio:.2f}')
            assert ratio <= 1.0, (q, n, ratio)
            big = got
        for j in range(33):
            single = {'sample_actions': lambda: agent.sample_actions(obs[j:j + 1], noises=z[j:j + 1]),
                      'compute_flow_actions': lambda: agent.compute_flow_actions(obs[j:j + 1], z[j:j + 1]),
                      'critic': lambda: agent.network.select('critic')(obs[j:j + 1], actions=act[j:j + 1])}[q]()
            np.testing.assert_array_equal(big[..., j:j + 1] if q == 'critic' else big[j:j + 1], single, err_msg=f'{q} row {j}')
    agent.close()


# ---- IQL and BC ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in CC.OTHER_GPU_CASES if n.startswith('iql')])
def test_iql_update_matches_fp64_within_twice_plain_fp32(name):
    import fql_amd
    cfg, batch, noise, params = CC.iql_problem(name)
    agent = fql_amd.IQLAgent.create(3, batch['observations'][:1], batch['actions'][:1], dict(fql_amd.iql.get_config(), **cfg))
    agent.set_params(params)
    print_plan(name, read_plan(agent))
    _report(name, *_step(name, agent, batch, noise))
    agent.close()


@pytest.mark.parametrize('name', [n for n in CC.OTHER_GPU_CASES if n.startswith('bc')])
def test_bc_update_and_sampler_match_fp64_within_twice_plain_fp32(name):
    import fql_amd
    od, ad = CC.BC_SHAPE[:2]
    cfg, batch, noise, params = CC.bc_problem(name)
    agent = fql_amd.BCAgent.create(3, np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32), dict(fql_amd.bc.get_config(), **cfg))
    agent.set_params(params)
    print_plan(name, read_plan(agent))
    # the sampler first (stored parameters): its first layer's obs W0 + b0 is loop-invariant, computed once for the 16 Euler steps
    want, yard = CC.bc_sampler_yardstick(name)
    obs, z = CC.bc_sampler_rows(name)
    got = agent.sample_actions(obs, noises=z)
    tol = max(CC.BC_SAMPLE_ATOL, CC.FACTOR * yard)
    err = float(np.abs(got - want).max())
    print(f'{name} sampler: yardstick {yard:.1e}, GPU worst error {err:.1e}, of tol {err / tol:.2f}')
    assert got.shape == want.shape and err <= tol, (err, tol)
    _report(name, *_step(name, agent, batch, noise))
    agent.close()
