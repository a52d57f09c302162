"""Cases, restatement and bounds of the optimizer-stage tests (tests/test_optimizer_cpu.py, tests/test_gpu_optimizer.py).

The optimizer stage is fql_adam_body + fql_finalize_body (fql_amd/csrc/fql_kernels.h): gradient statistics, Adam, the Polyak target
update and the counters.  `adam_polyak_step` restates optax Adam and the reference's target update in plain numpy (fp64: the reference;
fp32: the measurement that fixes the bounds).  Two routes reach the kernels past the first update.  The fused update from carried
moments (`carried_moments`, `oracle_update`, `fused_step_errors`) is what the GPU tests run.  Between update_begin and update_end the
engine also exposes the flat gradient buffer, so a test can hand the kernels any gradient: `layout` finds which buffer offset belongs to
which leaf element through public calls only, `crafted_gradient` / `crafted_moments` build the inputs at which the arithmetic can go
wrong, and BOUNDS holds that route's measured bounds; these are tested on the CPU, and their GPU tests are not in the suite yet
(MEASUREMENTS.md "Optimizer stage" says why).

Nothing here needs a GPU at import time.
"""
import math

import numpy as np

from oracle import fql_oracle as O

B1, B2, EPS = 0.9, 0.999, 1e-8

# ------------------------------------------------------------------------------------------------
# the measured errors of the fp32 restatement against the fp64 one, and the GPU bounds = 4 x measured
# (tests/test_optimizer_cpu.py::test_measured_errors_fix_the_gpu_bounds re-measures them; MEASUREMENTS.md "Optimizer stage").
# The kernel evaluates the same expression in the same order as the fp32 restatement; the factor 4 covers its fused multiply-adds
# and the device's rounding of `/` and sqrtf.  Units: see step_errors.
# ------------------------------------------------------------------------------------------------
MEASURED = {'mu': 1.5e-7, 'nu': 2.2e-7, 'p': 6.8e-6, 'target': 1.3e-7}
BOUNDS = {k: 4.0 * v for k, v in MEASURED.items()}
# grad/norm is an fp32 sum of exactly known terms: fp32 numpy against fp64 on the crafted gradients measures MEASURED_STATS.  4 x that
# is 2.6e-6; the GPU test asserts the tighter 2e-6 (grad/max and grad/min are exact: g * grad_scale with grad_scale a power of two)
MEASURED_STATS = 6.5e-7
STATS_RTOL = min(2e-6, 4 * MEASURED_STATS)
# the fused update (no injection): OracleFQL in fp32 against fp64 on the same case, in the units of fused_errors.  Measured: mu 9.2e-7,
# nu 1.13e-6, p 6.03e-5 (an element with |p| ~ 1e-6 whose 0.9 mu0 + 0.1 g cancels), target 1.22e-7; recorded 15 % up, since the oracle's
# fp32 matrix products depend on the BLAS underneath numpy (the CPU test accepts [0.5, 1] of the recorded figure)
MEASURED_FUSED = {'mu': 1.1e-6, 'nu': 1.3e-6, 'p': 7.0e-5, 'target': 1.4e-7}
BOUNDS_FUSED = {k: 4.0 * v for k, v in MEASURED_FUSED.items()}

COUNTS = (0, 1, 9, 999, 1_000_000)
SCALES = (1.0, 0.5)

# id -> (od, ad, B, hidden); `visual` is tests.test_gpu_visual.make_visual() as built there
STATE_CASES = {
    'ragged': (17, 6, 16, (80, 48, 64)),
    'h512': (29, 8, 16, (512, 512, 512, 512)),
    'act21': (69, 21, 16, (64, 64, 64)),
}
CASE_IDS = ('ragged', 'h512', 'act21', 'visual')
INJECTED_IDS = ('h512', 'act21', 'visual')


def injected_runs(case):
    """(count, grad_scale) pairs of an injected case: the full cross product on `act21`, counts 9 and 1 000 000 at scale 0.5 elsewhere."""
    if case == 'act21':
        return [(c, s) for c in COUNTS for s in SCALES]
    return [(9, 0.5), (1_000_000, 0.5)]


def case_problem(case, seed=0):
    """(cfg, batch, noise, obs_shape, act_dim) of a case."""
    if case == 'visual':
        from tests.test_gpu_visual import make_visual
        cfg, batch, noise = make_visual()
        return cfg, batch, noise, tuple(batch['observations'].shape[1:]), int(batch['actions'].shape[1])
    from tests.util import make_problem
    od, ad, B, hidden = STATE_CASES[case]
    cfg, _, batch, noise = make_problem(od, ad, B, hidden, seed=seed)
    return cfg, batch, noise, od, ad


def case_params(case, seed=3):
    """A parameter tree of the case's shapes without a GPU: the oracle's init, biases / LN off their init, target != critic."""
    from tests.util import randomize_params
    cfg, _, _, obs, ad = case_problem(case)
    return randomize_params(O.init_params(0, obs, ad, cfg), seed=seed)


def trainable(tree):
    """{path: leaf} of the leaves Adam updates (every leaf but the target networks')."""
    return {p: a for p, a in O.tree_leaves_with_path(tree) if 'target' not in p}


def target_path(path):
    """The target leaf a critic leaf is averaged into, or None."""
    return path.replace('modules_critic/', 'modules_target_critic/', 1) if path.startswith('modules_critic/') else None


def unflatten(leaves):
    tree = {}
    for path, v in leaves.items():
        node = tree
        keys = path.split('/')
        for k in keys[:-1]:
            node = node.setdefault(k, {})
        node[keys[-1]] = v
    return tree


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
class Step:
    __slots__ = ('p', 'mu', 'nu', 'target', 'step')

    def __init__(self, p, mu, nu, target, step):
        self.p, self.mu, self.nu, self.target, self.step = p, mu, nu, target, step


def adam_polyak_step(p, mu, nu, target, g, count, lr, tau, grad_scale, dtype, variant=None):
    """optax.adam(lr) (b1 0.9, b2 0.999, eps 1e-8 OUTSIDE the root, eps_root 0, bias correction with count + 1) on one leaf, and the
    reference's target update from the PRE-step parameter, target = tau p_old + (1 - tau) target (oracle/fql_oracle.py
    apply_gradients).  `count` is the optimizer's count BEFORE the step.  Every operand is cast to `dtype` and every operation rounds
    in it; the bias corrections are formed in double and cast, as the engine does.  `target` may be None (no target leaf).
    `variant` names one deliberate mistake (the CPU test shows that the bounds tell each from the truth): 'eps_in_root',
    'count_bias' (bias correction with count), 'polyak_post' (target from the post-step parameter).  Returns a Step; `.step` is
    mhat / (sqrt(vhat) + eps), the update in units of lr."""
    dt = np.dtype(dtype).type
    p, mu, nu, g = (np.asarray(a, dtype=dt) for a in (p, mu, nu, g))
    k = count if variant == 'count_bias' else count + 1
    with np.errstate(divide='ignore', invalid='ignore'):
        c1, c2 = dt(1.0 - B1 ** k), dt(1.0 - B2 ** k)
        ge = g * dt(grad_scale)
        m = dt(0.9) * mu + dt(0.1) * ge
        v = dt(0.999) * nu + dt(0.001) * ge * ge
        mh, vh = m / c1, v / c2
        step = mh / (np.sqrt(vh + dt(EPS)) if variant == 'eps_in_root' else np.sqrt(vh) + dt(EPS))
        pn = p - dt(lr) * step
    tn = None
    if target is not None:
        src = pn if variant == 'polyak_post' else p
        tn = src * dt(tau) + np.asarray(target, dtype=dt) * (dt(1.0) - dt(tau))
    return Step(pn, m, v, tn, step)


def grad_stats(g_by_leaf, grad_scale, dtype=np.float64):
    """utils/flax_utils.py:139-157 over the gradient tree, whose target leaves are zeros: grad/max = max(max g, 0), grad/min =
    min(min g, 0), grad/norm = sum over leaves of ||g_leaf||_2, of the scaled gradient.  fp64 by default."""
    dt = np.dtype(dtype).type
    mx, mn, nrm = 0.0, 0.0, dt(0.0)
    for g in g_by_leaf.values():
        ge = np.asarray(g, dtype=dt) * dt(grad_scale)
        mx, mn = max(mx, float(ge.max())), min(mn, float(ge.min()))
        nrm = nrm + np.sqrt(np.sum(ge * ge, dtype=dt))
    return {'grad/max': mx, 'grad/min': mn, 'grad/norm': float(nrm)}


def step_errors(got, ref, p0, mu0, nu0, t0, g, lr, tau, grad_scale):
    """Per-element errors of one leaf's step `got` against the fp64 Step `ref`, each in units of the magnitudes that entered it, so that
    a cancelling sum is not asked for relative accuracy of its result:
        mu      |d| / (|0.9 mu0| + |0.1 g s|)
        nu      |d| / (0.999 nu0 + 0.001 (g s)^2)
        p       |d| / (|p| + lr |step_ref|)
        target  |d| / (tau |p| + (1 - tau) |target|)
    Where a denominator is 0 every term is 0 and the result must be exactly 0: such an element reports 0 or inf."""
    f = lambda a: np.asarray(a, dtype=np.float64)   # noqa: E731
    p0, mu0, nu0, g = f(p0), f(mu0), f(nu0), f(g) * grad_scale
    den = {'mu': np.abs(0.9 * mu0) + np.abs(0.1 * g), 'nu': 0.999 * nu0 + 0.001 * g * g, 'p': np.abs(p0) + lr * np.abs(f(ref.step))}
    d = {'mu': f(got.mu) - f(ref.mu), 'nu': f(got.nu) - f(ref.nu), 'p': f(got.p) - f(ref.p)}
    if ref.target is not None:
        den['target'] = tau * np.abs(p0) + (1 - tau) * np.abs(f(t0))
        d['target'] = f(got.target) - f(ref.target)
    out = {}
    for k in d:
        a = np.abs(d[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            e = np.where(den[k] > 0, a / den[k], np.where(a == 0, 0.0, np.inf))
        out[k] = np.where(np.isnan(a), np.inf, e)
    return out


def fused_errors(got, ref, p0, mu0, nu0, t0, gmax, lr, tau, grad_scale):
    """step_errors for a step whose gradient the engine computed itself.  That gradient carries an error relative to its leaf's largest
    element (2e-5 of it is what the parity tests allow), so the leaf's max |g| `gmax` stands where step_errors has the element's own g."""
    g = np.full(np.shape(p0), float(gmax))
    return step_errors(got, ref, p0, mu0, nu0, t0, g, lr, tau, grad_scale)


# ------------------------------------------------------------------------------------------------
# the layout map
# ------------------------------------------------------------------------------------------------
def grad_view(agent):
    """The flat gradient buffer as a torch tensor without a copy (a CPU stand-in hands its own over, as for fql_amd.parallel)."""
    if hasattr(agent, 'grad_tensor'):
        return agent.grad_tensor()
    import torch
    from fql_amd.parallel import _DevView
    ptr, n = agent.grad_buffer()
    t = torch.as_tensor(_DevView(ptr, n), device='cuda')
    assert t.data_ptr() == ptr and t.numel() == n
    return t


def device_wait(agent):
    """Everything enqueued so far has run: the engine's own stream and queues, and every stream torch knows."""
    agent.synchronize()
    if not hasattr(agent, 'grad_tensor'):
        import torch
        torch.cuda.synchronize()


class Layout:
    """offsets[path]: the flat gradient-buffer offset of every element of the trainable leaf `path` (the leaf's shape); `n` floats in
    the buffer; `padding`: the offsets that belong to no element."""

    def __init__(self, offsets, n):
        self.offsets, self.n = offsets, n
        real = np.zeros(n, bool)
        for o in offsets.values():
            real[o.reshape(-1)] = True
        self.padding = np.flatnonzero(~real)

    def scatter(self, g_by_leaf):
        """(offsets, values) of a per-leaf gradient in buffer order."""
        idx = np.concatenate([self.offsets[p].reshape(-1) for p in g_by_leaf])
        val = np.concatenate([np.asarray(g_by_leaf[p], np.float32).reshape(-1) for p in g_by_leaf])
        order = np.argsort(idx, kind='stable')
        return idx[order], val[order]

    def gather(self, buf):
        return {p: np.asarray(buf)[o] for p, o in self.offsets.items()}

    def longest_run_chunks(self, path):
        """Adam chunks (4096 floats) of the longest contiguous run of the leaf's offsets: a lower bound of its chunk count."""
        o = np.sort(self.offsets[path].reshape(-1))
        cuts = np.flatnonzero(np.diff(o) != 1)
        runs = np.diff(np.concatenate([[-1], cuts, [o.size - 1]]))
        return int(math.ceil(runs.max() / 4096))


def layout(agent, batch, noise):
    """The map from gradient-buffer offset to (leaf, element), through public calls only: on a SCRATCH agent with zero moments at count
    0 (it is stepped, and its padding is overwritten: do not train it afterwards) run update_begin, overwrite the whole buffer with
    float(offset + 1), run update_end and read mu = 0.1 (offset + 1).  Asserts that the map is injective and covers every element of
    every trainable leaf; every other offset is padding."""
    import torch
    opt = agent.get_opt_state()
    assert opt['count'] == 0 and all(not a.any() for a in trainable(opt['mu']).values())
    agent.update_begin(batch=batch, noise=noise)
    device_wait(agent)
    g = grad_view(agent)
    n = g.numel()
    assert n < 6_000_000   # offset + 1 and 0.1f (offset + 1) are exact / decodable in fp32 (2^24; the product's ulp stays below 0.05)
    g.copy_(torch.arange(1, n + 1, dtype=torch.float32).to(g.device))
    device_wait(agent)
    agent.update_end()
    device_wait(agent)
    offsets, seen = {}, np.zeros(n, np.int64)
    for path, mu in trainable(agent.get_opt_state()['mu']).items():
        off = np.rint(mu.astype(np.float64) / 0.1).astype(np.int64) - 1
        assert off.min() >= 0 and off.max() < n, path
        np.testing.assert_array_equal((np.float32(0.1) * (off + 1).astype(np.float32)), mu, err_msg=path)   # decoded, not guessed
        np.add.at(seen, off.reshape(-1), 1)
        offsets[path] = off
    assert seen.max() == 1, 'two leaf elements share a gradient-buffer offset'
    assert set(offsets) == set(trainable(agent.get_params())) and all(offsets[p].shape == a.shape for p, a in trainable(agent.get_params()).items())
    return Layout(offsets, n)


# ------------------------------------------------------------------------------------------------
# crafted inputs
# ------------------------------------------------------------------------------------------------
def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def crafted_gradient(shapes, seed, extremes=True):
    """{path: fp32 gradient} for the trainable leaves `shapes` ({path: shape}).  Per leaf: exact zeros (at least a tenth, and one whole
    bias leaf); +-|N(0, 1)| times the leaf's scale (10^U(-4, 0)); a band with |g| in [1e-9, 1e-7], where sqrt(v_hat) straddles 1e-8; a few
    elements at +-1e12 and at +-1e-12.  |g| stays inside [1e-12, 1e12] or is exactly 0: every square is a normal fp32 number.
    extremes=False: zeros and +-|N(0, 1)| times U(0.5, 2) only - every chunk of every leaf then weighs in grad/norm."""
    rng = np.random.default_rng(seed)
    paths = sorted(shapes)
    biases = [p for p in paths if p.endswith('/bias')]
    zero_leaf = biases[seed % len(biases)]
    out = {}
    for p in paths:
        n = int(np.prod(shapes[p]))
        scale = 10.0 ** rng.uniform(-4, 0) if extremes else rng.uniform(0.5, 2.0)
        g = _sign(rng, n) * np.maximum(np.abs(rng.standard_normal(n)), 1e-6) * scale
        perm = rng.permutation(n)
        nz = min(n - 1, max(1, math.ceil(0.1 * n))) if n > 1 else 0
        g[perm[:nz]] = 0.0
        at = nz
        if extremes:
            nb = n // 10
            g[perm[at:at + nb]] = _sign(rng, nb) * 10.0 ** rng.uniform(-9, -7, nb)
            at += nb
            for mag in (1e12, 1e-12):
                k = min(3, max(0, (n - at) // 8))
                g[perm[at:at + k]] = _sign(rng, k) * mag
                at += k
        if p == zero_leaf:
            g[:] = 0.0
        g = g.astype(np.float32)
        a = np.abs(g[g != 0])
        assert a.size == 0 or (a.min() >= np.float32(1e-12) * (1 - 1e-6) and a.max() <= np.float32(1e12) * (1 + 1e-6))
        out[p] = g.reshape(shapes[p])
    return out


def crafted_moments(seed, grads, grad_scale=1.0):
    """({path: mu0}, {path: nu0}) in fp32 beside the gradient `grads`.  Per element one of: both 0 (a fresh element); mu0 = -(0.1 g s) /
    0.9 (1 + d), |d| in [1e-6, 1e-3], so that 0.9 mu0 and 0.1 g s nearly cancel, with nu0 on the gradient's scale; nu0 around 1e-16 and
    |mu0| around 1e-8, where sqrt(v_hat) sits at eps; nu0 = 0 beside a mu0 of its element's own |g| (only where g != 0); mu0 and nu0 on
    the leaf's gradient scale, mixed sign.  Every |m_hat| / (sqrt(v_hat) + eps) stays below about 50, so a step moves no parameter by more
    than 50 lr and the network's next forward pass stays finite (an overflowing one would put inf x 0 = NaN into the gradient padding)."""
    rng = np.random.default_rng(seed)
    mu0, nu0 = {}, {}
    for p in sorted(grads):
        g = np.asarray(grads[p], np.float64).reshape(-1) * grad_scale
        n = g.size
        nzg = np.abs(g[g != 0])
        s = float(np.median(nzg)) if nzg.size else 1e-3
        kind = rng.integers(0, 5, n)
        m, v = np.zeros(n), np.zeros(n)
        k = kind == 1
        m[k] = -(0.1 * g[k]) / 0.9 * (1 + _sign(rng, k.sum()) * 10.0 ** rng.uniform(-6, -3, k.sum()))
        v[k] = g[k] ** 2 * rng.uniform(0.25, 4, k.sum())
        k = kind == 2
        m[k] = _sign(rng, k.sum()) * 1e-8 * rng.uniform(0.1, 3, k.sum())
        v[k] = 1e-16 * rng.uniform(0.25, 4, k.sum())
        k = (kind == 3) & (g != 0)
        m[k] = rng.standard_normal(k.sum()) * 0.3 * np.abs(g[k])
        k = kind == 4
        m[k] = rng.standard_normal(k.sum()) * s
        v[k] = (np.maximum(np.abs(rng.standard_normal(k.sum())), 0.1) * s) ** 2
        m, v = m.astype(np.float32), v.astype(np.float32)
        assert not ((v == 0) & (m != 0) & (g == 0)).any()
        mu0[p], nu0[p] = m.reshape(np.shape(grads[p])), v.reshape(np.shape(grads[p]))
    return mu0, nu0


def reference_step(params, mu0, nu0, grads, count, lr, tau, grad_scale, dtype=np.float64, variant=None):
    """adam_polyak_step over every trainable leaf of `params` (a {path: leaf} dict with the target leaves in it): {path: Step}."""
    out = {}
    for p, g in grads.items():
        t = target_path(p)
        out[p] = adam_polyak_step(params[p], mu0[p], nu0[p], params[t] if t else None, g, count, lr, tau, grad_scale, dtype, variant)
    return out


def worst_errors(got, ref, params, mu0, nu0, grads, lr, tau, grad_scale):
    """({unit: (worst error, its leaf)}, {unit: every element's error, all leaves}) of steps `got` against `ref` ({path: Step})."""
    worst, every = {}, {}
    for p in grads:
        t = target_path(p)
        e = step_errors(got[p], ref[p], params[p], mu0[p], nu0[p], params[t] if t else None, grads[p], lr, tau, grad_scale)
        for k, a in e.items():
            worst[k] = max(worst.get(k, (0.0, '')), (float(a.max()), p))
            every.setdefault(k, []).append(a.reshape(-1))
    return worst, {k: np.concatenate(v) for k, v in every.items()}


# ------------------------------------------------------------------------------------------------
# the fused update past the first step (no injection)
# ------------------------------------------------------------------------------------------------
FUSED_COUNTS = (9, 999, 1_000_000)


def carried_moments(seed, grads, count, grad_scale=1.0):
    """({path: mu0}, {path: nu0}) for a step whose gradient the engine computes itself; `grads` is the reference's gradient at the same
    parameters.  nu0 = c2 (max |g_leaf| s)^2 U(1, 4), so that sqrt(nu0 / c2) >= max |g_leaf|: the 2e-5 max |g_leaf| by which the engine's
    gradient may differ then moves the step by less than 2e-5 lr.  mu0: every other element -(0.1 g s) / 0.9 (1 + d), |d| in [1e-3, 1e-1]
    (0.9 mu0 and 0.1 g s nearly cancel), the rest N(0, 1) 0.3 max |g_leaf| s: mixed sign, and |step| stays below about 10."""
    rng = np.random.default_rng(seed)
    c2 = 1.0 - B2 ** (count + 1)
    mu0, nu0 = {}, {}
    for p in sorted(grads):
        g = np.asarray(grads[p], np.float64).reshape(-1) * grad_scale
        gmax = max(float(np.abs(g).max()), 1e-6)
        m = rng.standard_normal(g.size) * 0.3 * gmax
        k = rng.random(g.size) < 0.5
        m[k] = -(0.1 * g[k]) / 0.9 * (1 + _sign(rng, k.sum()) * 10.0 ** rng.uniform(-3, -1, k.sum()))
        v = c2 * gmax ** 2 * rng.uniform(1.0, 4.0, g.size)
        mu0[p], nu0[p] = m.astype(np.float32).reshape(np.shape(grads[p])), v.astype(np.float32).reshape(np.shape(grads[p]))
    return mu0, nu0


def set_oracle_moments(ref, mu0, nu0, count):
    """Hand an oracle (params / mu / nu trees, count, step) the carried moments; leaves without one (the targets) keep zeros."""
    def put(tree, leaves):
        for p, a in O.tree_leaves_with_path(tree):
            a[...] = leaves[p] if p in leaves else 0
    put(ref.mu, mu0)
    put(ref.nu, nu0)
    ref.count, ref.step = count, count + 1


def oracle_update(ref, batch, noise, grad_scale=1.0):
    """OracleFQL.update with the data-parallel gradient scale applied where the engine applies it: to the gradient that enters the
    statistics and the moments.  Returns (infos, the scaled gradient's leaves)."""
    _, info, grads = ref._losses(batch, noise, want_grads=True)
    grads = O.tree_map(lambda g: g * ref.dtype.type(grad_scale), grads)
    info.update(ref.grad_stats(grads))
    ref.apply_gradients(grads)
    return {k: float(info[k]) for k in O.INFO_KEYS}, trainable(grads)


def fused_step_errors(pre, post, ref_pre, ref_post, gmax, lr, tau, target_of=target_path):
    """{unit: (worst error, leaf)} of a fused step `pre` -> `post` against the reference's `ref_pre` -> `ref_post` (each a dict of
    {'params', 'mu', 'nu'} leaf dicts; ref in fp64) in the units of fused_errors, over the leaves of `gmax`: {path: max |g_leaf| s}.
    `lr`: a float or {path: lr}; `target_of(path)`: the target leaf averaged from `path`, or None."""
    worst = {}
    for p in gmax:
        t = target_of(p)
        lr_p = lr[p] if isinstance(lr, dict) else lr
        f = lambda d, q: np.asarray(d[q], np.float64)   # noqa: E731
        step = (f(ref_pre['params'], p) - f(ref_post['params'], p)) / lr_p
        got = Step(post['params'][p], post['mu'][p], post['nu'][p], post['params'][t] if t else None, None)
        ref = Step(ref_post['params'][p], ref_post['mu'][p], ref_post['nu'][p], ref_post['params'][t] if t else None, step)
        e = fused_errors(got, ref, pre['params'][p], pre['mu'][p], pre['nu'][p], pre['params'][t] if t else None, gmax[p], lr_p, tau, 1.0)
        for k, a in e.items():
            worst[k] = max(worst.get(k, (0.0, '')), (float(a.max()), p))
    return worst
