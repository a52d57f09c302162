"""CPU: the optimizer-stage restatement against the existing oracle, the layout decode on a stand-in agent, and the measurement that
fixes the bounds of tests/test_gpu_optimizer.py (fp32 numpy against fp64 numpy on every injected case), with the proof that those
bounds tell three one-line mistakes from the truth."""
import numpy as np
import pytest
import torch

from oracle import fql_oracle as O
from tests import optimizer_cases as C

LR, TAU = 3e-4, 0.005


def _state(case, count, scale, seed=11):
    """(params {path: leaf}, grads, mu0, nu0) of an injected case."""
    params = dict(O.tree_leaves_with_path(C.case_params(case)))
    grads = C.crafted_gradient({p: a.shape for p, a in params.items() if 'target' not in p}, seed)
    mu0, nu0 = C.crafted_moments(seed + 1, grads, scale)
    return params, grads, mu0, nu0


@pytest.mark.parametrize('count', [0, 1, 999])
def test_restatement_equals_the_oracles_apply_gradients(count):
    """adam_polyak_step in fp64 against OracleFQL.apply_gradients on the same inputs.  The two write 1 - b as `1 - 0.9` and as `0.1`
    (one ulp of a double apart), hence a few ulps and not bitwise."""
    cfg, _, _, od, ad = C.case_problem('ragged')
    tree = C.case_params('ragged')
    params = dict(O.tree_leaves_with_path(tree))
    grads = C.crafted_gradient({p: a.shape for p, a in params.items() if 'target' not in p}, 5)
    mu0, nu0 = C.crafted_moments(6, grads)
    ref = O.OracleFQL(tree, dict(cfg), od, ad, np.float64)
    zeros = lambda a: np.zeros(a.shape, np.float64)   # noqa: E731
    full = {p: (grads[p].astype(np.float64) if p in grads else zeros(a)) for p, a in params.items()}
    ref.mu = C.unflatten({p: (mu0[p].astype(np.float64) if p in mu0 else zeros(a)) for p, a in params.items()})
    ref.nu = C.unflatten({p: (nu0[p].astype(np.float64) if p in nu0 else zeros(a)) for p, a in params.items()})
    ref.count, ref.step = count, count + 1
    ref.apply_gradients(C.unflatten(full))
    assert ref.count == count + 1 and ref.step == count + 2
    got = C.reference_step(params, mu0, nu0, grads, count, cfg['lr'], cfg['tau'], 1.0)
    want_p, want_mu, want_nu = (dict(O.tree_leaves_with_path(t)) for t in (ref.params, ref.mu, ref.nu))
    assert cfg['lr'] == LR and cfg['tau'] == TAU
    for p, s in got.items():
        t = C.target_path(p)
        theirs = C.Step(want_p[p], want_mu[p], want_nu[p], want_p[t] if t else None, None)
        e = C.step_errors(theirs, s, params[p], mu0[p], nu0[p], params[t] if t else None, grads[p], LR, TAU, 1.0)
        # a few ulps of a double in units of the terms; the step inherits mu's error divided by how far 0.9 mu0 + 0.1 g cancels (down
        # to 1e-6 of its terms in the crafted moments)
        assert e['mu'].max() <= 2e-15 and e['nu'].max() <= 2e-15 and e['p'].max() <= 1e-9, (p, {k: v.max() for k, v in e.items()})
        assert t is None or e['target'].max() <= 2e-15, t


def test_grad_stats_follow_the_reference():
    grads = C.crafted_gradient({'a/bias': (7,), 'a/kernel': (5, 7), 'b/bias': (3,)}, 2, extremes=False)
    st = C.grad_stats(grads, 0.5)
    flat = np.concatenate([g.reshape(-1).astype(np.float64) for g in grads.values()]) * 0.5
    assert st['grad/max'] == max(flat.max(), 0) and st['grad/min'] == min(flat.min(), 0)
    assert abs(st['grad/norm'] - sum(np.linalg.norm(g.astype(np.float64)) * 0.5 for g in grads.values())) <= 1e-12 * st['grad/norm']
    only_neg = {'a/bias': -np.ones(3, np.float32), 'b/bias': np.zeros(2, np.float32)}
    assert C.grad_stats(only_neg, 1.0)['grad/max'] == 0.0           # the target leaves' zeros bound the extrema


class _FakeAgent:
    """What `layout` calls, over a padded arena on the host: leaves laid out row by row with padded rows and a gap between leaves;
    update_end takes Adam's first step from zero moments (mu = 0.1 g) and records what it was handed."""

    def __init__(self, shapes, pad_to=16):
        self.shapes, self.offsets, at = shapes, {}, 0
        for p, shp in shapes.items():
            rows, cols = (int(np.prod(shp[:-1])), shp[-1])
            cp = -(-cols // pad_to) * pad_to
            self.offsets[p] = (at + np.arange(rows)[:, None] * cp + np.arange(cols)[None, :]).reshape(shp)
            at += rows * cp + 4
        self.buf = torch.zeros(at)
        self.mu = {p: np.zeros(s, np.float32) for p, s in shapes.items()}
        self.count, self.handed, self.calls = 0, None, []

    def grad_tensor(self): return self.buf
    def synchronize(self): return 'graph'
    def get_params(self): return C.unflatten({**{p: np.zeros(s, np.float32) for p, s in self.shapes.items()}, 'modules_target_critic/x': np.zeros(2, np.float32)})
    def get_opt_state(self): return {'count': self.count, 'step': self.count + 1, 'mu': C.unflatten(dict(self.mu)), 'nu': C.unflatten(dict(self.mu))}

    def update_begin(self, batch=None, noise=None):
        self.calls.append('begin')
        self.buf.zero_()
        for o in self.offsets.values():
            self.buf[torch.as_tensor(o.reshape(-1))] = 0.25

    def update_end(self):
        self.calls.append('end')
        self.handed = self.buf.numpy().copy()
        for p, o in self.offsets.items():
            self.mu[p] = np.float32(0.1) * self.handed[o]
        self.count += 1


def test_layout_decodes_a_padded_arena():
    shapes = {'m/Dense_0/bias': (5,), 'm/Dense_0/kernel': (7, 5), 'n/Dense_0/kernel': (2, 3, 21), 'n/Dense_0/bias': (2, 21)}
    fake = _FakeAgent(shapes)
    lay = C.layout(fake, None, None)
    assert fake.calls == ['begin', 'end']
    np.testing.assert_array_equal(fake.handed, np.arange(1, fake.buf.numel() + 1, dtype=np.float32))   # the whole buffer, offset + 1
    assert lay.n == fake.buf.numel() and set(lay.offsets) == set(shapes)
    for p in shapes:
        np.testing.assert_array_equal(lay.offsets[p], fake.offsets[p])
    real = np.concatenate([o.reshape(-1) for o in fake.offsets.values()])
    np.testing.assert_array_equal(np.sort(np.concatenate([real, lay.padding])), np.arange(lay.n))
    assert lay.padding.size == lay.n - sum(int(np.prod(s)) for s in shapes.values()) > 0
    # scatter / gather are inverse on the real offsets and leave the padding alone
    grads = C.crafted_gradient(shapes, 1)
    idx, val = lay.scatter(grads)
    buf = np.zeros(lay.n, np.float32)
    buf[idx] = val
    assert not buf[lay.padding].any()
    for p, g in lay.gather(buf).items():
        np.testing.assert_array_equal(g, grads[p])
    assert lay.longest_run_chunks('m/Dense_0/kernel') == 1


def test_layout_refuses_two_elements_on_one_offset():
    fake = _FakeAgent({'m/Dense_0/bias': (5,), 'm/Dense_0/kernel': (7, 5)})
    fake.offsets['m/Dense_0/bias'] = fake.offsets['m/Dense_0/kernel'][0].copy()
    with pytest.raises(AssertionError):
        C.layout(fake, None, None)


def test_crafted_inputs_hold_every_population():
    params, grads, mu0, nu0 = _state('ragged', 0, 1.0)
    assert sum(1 for p, g in grads.items() if p.endswith('/bias') and not g.any()) >= 1
    allg = np.concatenate([g.reshape(-1) for g in grads.values()]).astype(np.float64)
    allm = np.concatenate([mu0[p].reshape(-1) for p in grads]).astype(np.float64)
    allv = np.concatenate([nu0[p].reshape(-1) for p in grads]).astype(np.float64)
    for p, g in grads.items():
        assert (g == 0).sum() >= 0.1 * g.size or g.size == 1, p
    a = np.abs(allg)
    assert ((a >= 1e-9) & (a <= 1e-7)).sum() > 100 and (a > 0.9e12).sum() > 10 and ((a > 0) & (a < 1.1e-12)).sum() > 10
    assert a[a > 0].min() >= 0.99e-12 and a.max() <= 1.01e12
    sq = (allg.astype(np.float32) * np.float32(0.5)) ** 2
    assert np.isfinite(sq).all() and sq[allg != 0].min() >= np.finfo(np.float32).tiny     # every square a normal fp32 number
    cancel = np.abs(0.9 * allm + 0.1 * allg) < 1e-2 * np.abs(0.1 * allg)
    assert (cancel & (allg != 0)).sum() > 100
    assert ((allv == 0) & (allg != 0)).sum() > 100 and ((allv > 0) & (allv < 1e-15)).sum() > 100
    assert not ((allv == 0) & (allm != 0) & (allg == 0)).any()
    assert (allm > 0).any() and (allm < 0).any()
    # sqrt(v_hat) on both sides of eps, at the first count and at a large one
    for count in (0, 999):
        vh = (0.999 * allv + 0.001 * allg ** 2) / (1 - 0.999 ** (count + 1))
        r = np.sqrt(vh[vh > 0])
        assert ((r > 1e-9) & (r < 1e-8)).sum() > 50 and ((r > 1e-8) & (r < 1e-7)).sum() > 50


def _measure():
    """Worst fp32-against-fp64 error per unit over every injected case, its second step included, and of grad/norm."""
    worst = {k: (0.0, '') for k in C.MEASURED}
    stats = 0.0
    for case in C.INJECTED_IDS:
        for count, scale in C.injected_runs(case):
            params, grads, mu0, nu0 = _state(case, count, scale)
            shapes = {p: g.shape for p, g in grads.items()}
            for second in (False, True):
                ref = C.reference_step(params, mu0, nu0, grads, count, LR, TAU, scale)
                got = C.reference_step(params, mu0, nu0, grads, count, LR, TAU, scale, dtype=np.float32)
                for p, s in got.items():
                    assert all(np.isfinite(a).all() for a in (s.p, s.mu, s.nu)), (case, count, scale, p)
                w, _ = C.worst_errors(got, ref, params, mu0, nu0, grads, LR, TAU, scale)
                for k, (e, p) in w.items():
                    worst[k] = max(worst[k], (e, f'{case} count {count} scale {scale} {p}'))
                s64, s32 = C.grad_stats(grads, scale), C.grad_stats(grads, scale, np.float32)
                assert s64['grad/max'] == s32['grad/max'] and s64['grad/min'] == s32['grad/min']
                stats = max(stats, abs(s32['grad/norm'] - s64['grad/norm']) / s64['grad/norm'])
                if second:
                    break
                # the second step starts from the fp32 state the first one reached, with a fresh gradient, at count + 1
                params = dict(params)
                for p, s in got.items():
                    params[p], mu0[p], nu0[p] = s.p, s.mu, s.nu
                    if s.target is not None:
                        params[C.target_path(p)] = s.target
                grads, count = C.crafted_gradient(shapes, 77, extremes=False), count + 1
    return worst, stats


def test_measured_errors_fix_the_gpu_bounds():
    """The figures in optimizer_cases.MEASURED are what this measurement gives, rounded up to two digits; the GPU bounds are 4 x them."""
    worst, stats = _measure()
    print('optimizer stage, fp32 numpy against fp64:', {k: f'{e:.3e} ({p})' for k, (e, p) in worst.items()}, f'grad/norm {stats:.3e}')
    for k, (e, p) in worst.items():
        assert 0.9 * C.MEASURED[k] <= e <= C.MEASURED[k], (k, e, p)
        assert C.BOUNDS[k] == 4 * C.MEASURED[k]
    assert 0.9 * C.MEASURED_STATS <= stats <= C.MEASURED_STATS and C.STATS_RTOL == min(2e-6, 4 * C.MEASURED_STATS)


@pytest.mark.parametrize('variant', ['eps_in_root', 'count_bias', 'polyak_post'])
def test_bounds_tell_one_line_mistakes_from_the_truth(variant):
    """The fp64 restatement with one deliberate mistake misses the GPU bounds on at least 1 % of the elements of at least one case."""
    best = 0.0
    for count, scale in C.injected_runs('act21'):
        params, grads, mu0, nu0 = _state('act21', count, scale)
        ref = C.reference_step(params, mu0, nu0, grads, count, LR, TAU, scale)
        bad = C.reference_step(params, mu0, nu0, grads, count, LR, TAU, scale, variant=variant)
        _, every = C.worst_errors(bad, ref, params, mu0, nu0, grads, LR, TAU, scale)
        unit = 'target' if variant == 'polyak_post' else 'p'
        best = max(best, float((every[unit] > C.BOUNDS[unit]).mean()))
    assert best >= 0.01, (variant, best)


def _fused_case(case, count, scale, dtype):
    """The fused case on the CPU: (pre state, oracle after one update in `dtype`, gmax, infos)."""
    cfg, batch, noise, od, ad = C.case_problem(case)
    tree = C.case_params(case)
    g64 = C.trainable(O.OracleFQL(tree, dict(cfg), od, ad, np.float64).grads(batch, noise)[2])
    mu0, nu0 = C.carried_moments(21, g64, count, scale)
    ref = O.OracleFQL(tree, dict(cfg), od, ad, dtype)
    C.set_oracle_moments(ref, mu0, nu0, count)
    pre = dict(params=dict(O.tree_leaves_with_path(tree)), mu=mu0, nu=nu0)
    info, _ = C.oracle_update(ref, batch, noise, scale)
    post = dict(params=dict(O.tree_leaves_with_path(ref.params)), mu=dict(O.tree_leaves_with_path(ref.mu)), nu=dict(O.tree_leaves_with_path(ref.nu)))
    gmax = {p: max(float(np.abs(g).max()) * scale, 1e-6 * scale) for p, g in g64.items()}
    return pre, post, gmax, info, cfg


def test_measured_errors_fix_the_fused_bounds():
    """OracleFQL in fp32 against fp64 on every fused case of test_gpu_optimizer.py: optimizer_cases.MEASURED_FUSED."""
    worst = {k: (0.0, '') for k in C.MEASURED_FUSED}
    for case in ('ragged', 'h512'):
        for count in C.FUSED_COUNTS:
            for scale in C.SCALES:
                pre, p32, gmax, _, cfg = _fused_case(case, count, scale, np.float32)
                _, p64, _, _, _ = _fused_case(case, count, scale, np.float64)
                w = C.fused_step_errors(pre, p32, pre, p64, gmax, cfg['lr'], cfg['tau'])
                for k, (e, p) in w.items():
                    worst[k] = max(worst[k], (e, f'{case} count {count} scale {scale} {p}'))
    print('fused update, OracleFQL fp32 against fp64:', {k: f'{e:.3e} ({p})' for k, (e, p) in worst.items()})
    for k, (e, p) in worst.items():
        assert 0.5 * C.MEASURED_FUSED[k] <= e <= C.MEASURED_FUSED[k], (k, e, p)
        assert C.BOUNDS_FUSED[k] == 4 * C.MEASURED_FUSED[k]
