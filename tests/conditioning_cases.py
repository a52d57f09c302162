"""Ill-conditioned problems for the parity tests (tests/test_gpu_conditioning.py, tests/test_conditioning_cpu.py) and the fp32
yardstick that sets their tolerances, built on the CPU from numpy and the oracles alone.

Every other parity test runs on N(0, 1) observations and parameters 0.05 to 0.1 away from their init, where a LayerNorm row has a mean of
about its standard deviation and Q is of order 1.  The one-pass variance var = max(0, E[x^2] - E[x]^2) (flax's, and the kernels') loses
(mean / std)^2 of its precision, so a mistake in a LayerNorm sum that costs 1e-6 there costs 100 to 1000 times as much on rows with an
offset; and q - target is a difference of two large numbers once Q is near -200 or -1000.  The builders here reach both regimes:

  offset_params(params, c, nets)   c added to every hidden Dense bias of the named nets: GELU(z + c) ~ z + c, a LayerNorm input with
                                   |mean| / std of 5 and more
  q_offset(params, q0)             q0 added to the last Dense bias of the critic and the target critic
  scaled_obs(batch)                5 obs + 30
  dead_layer(params, c)            the critic's Dense_1 kernel 0 and bias exactly c: the input of LayerNorm_1 is one value in every column,
                                   true variance 0, rstd = 1 / sqrt(eps)

On such inputs plain fp32 arithmetic itself leaves the suite's fixed tolerances, by an amount that depends on the order of the sums, so
the comparisons use a measured yardstick, never a figure from the engine: yardstick(case) runs the numpy oracle in fp64 (the truth) and
in fp32 in three variants,
  pairwise    the oracle as it is (numpy's pairwise row sums, division by the width)
  sequential  O.layer_norm swapped, for fp32 arrays, for one whose two row sums are sequential fp32 sums (np.cumsum) multiplied by an fp32
              1 / width (what the kernels do: 1 / 50 and 1 / 250 are inexact), var = s2 inv - mean mean in two roundings
  fused       the sequential one with var = fma(s2, inv, -(mean mean)): one rounding, the contraction a compiler may apply
and returns, per gradient leaf, max over the variants of max|g32 - g64| / max|g64|, per info the same maximum of |i32 - i64|, and per
forward query the maximum element error.  tol = max(existing bound, 2 x yardstick): a kernel's reduction (32 sequential terms per lane and
a butterfly; 16 sequential partials of 32 columns) is one more fp32 order between the pairwise and the sequential one, rounding errors are
random so it may land a factor 2 off the worse end, and anything beyond that is not an fp32 sum of the right columns.
"""
import contextlib

import numpy as np

from oracle import fql_oracle as O
from tests import bc_oracle as BO
from tests import iql_oracle as IO
from tests.util import BF16X3_BOUND, leaf_dict, make_problem, randomize_params

OD, AD = 29, 8
C_OFFSET, C_DEAD, Q0S = 10.0, (0.0, 30.0), (-200.0, -1000.0)
FACTOR, CAP = 2.0, 1e-3
GRAD_BOUND, INFO_RTOL, INFO_ATOL = 2e-5, 5e-5, 5e-6          # assert_step_matches' bounds (tests/util.py)
SAMPLE_ATOL, FLOW_ATOL, QUERY_ATOL, QUERY_RTOL = 2e-6, 5e-6, 2e-6, 2e-5   # tests/test_gpu_shapes.py, tests/test_gpu_module_forward.py
MARGIN = 1e-3                                                # kink margin (tests/test_kink_margins_cpu.py)
DATA_SEED, INIT_SEED, RANDOMIZE_SEED = 3, 7, 5
CRITICS = ('modules_critic', 'modules_target_critic')
ACTORS = ('modules_actor_bc_flow', 'modules_actor_onestep_flow')
VARIANTS = ('pairwise', 'sequential', 'fused')

# the LayerNorm sites (tests/test_gpu_batch_edges.py, tests/padded_cases.py, tests/test_gpu_shapes.py): id -> (B, hidden, config)
BASES = {
    'rows16': (144, (256,) * 3, {}),                                   # the 16-row Dense kernel only, no 32-row task
    'side32': (256, (256,) * 3, {}),                                   # 32-row tiles folding 8 partials
    'side32_h64': (256, (64,) * 3, {}),                                # 32 x 64 tiles folding 2 partials
    'side64': (1088, (64,) * 3, {}),                                   # fql_side_big_kernel, 17 row tiles
    'split': (256, (256,) * 3, dict(precision='bf16x3')),              # split tiles and split chain
    'kbig': (32, (1024,) * 3, {}),                                     # the K > 512 kernels (wide1024's width)
    'padded': (32, (50, 50, 50), {}),                                  # ln_width 50 of 64 columns (padded_cases' w50)
    'padded250': (32, (250,) * 3, {}),                                 # ln_width 250 of 256: 1 / 250 inexact, the dead layer's clamp
    'side32_w250': (256, (250,) * 3, {}),                              # the same on the 32-row tiles (gemm32_body's clamp)
    'side64_w250': (1088, (250,) * 3, {}),                             # on fql_side_big_kernel's 64-row tiles (gemm64_body's clamp)
    'split_w250': (256, (250,) * 3, dict(precision='bf16x3')),         # on the split 32-row tiles (gemm32s_body's clamp)
    'chain_ln': (144, (256,) * 3, dict(actor_layer_norm=True)),        # the chain's LayerNorm forward and fused backward
}
Q_CFG = dict(discount=0.995)
Q_CFG_NORM = dict(discount=0.995, normalize_q_loss=True, q_agg='min')

#   id -> dict(base, c, q0, scaled, dead, cfg)
FQL_CASES = {}


def _case(name, base, c=None, q0=None, scaled=False, dead=None, cfg=None, seed=DATA_SEED):
    FQL_CASES[name] = dict(base=base, c=c, q0=q0, scaled=scaled, dead=dead, cfg=dict(cfg or {}), seed=seed)


for _b in ('rows16', 'side32', 'side32_h64', 'side64', 'split', 'kbig', 'padded', 'chain_ln'):
    _case(f'{_b}/c10', _b, c=C_OFFSET)
_case('rows16/q200', 'rows16', q0=-200.0, cfg=Q_CFG)
_case('rows16/q1000_norm_min', 'rows16', q0=-1000.0, cfg=Q_CFG_NORM)
_case('side32/q200_norm_min', 'side32', q0=-200.0, cfg=Q_CFG_NORM)
_case('side32_h64/q1000', 'side32_h64', q0=-1000.0, cfg=Q_CFG)
# scaled observations move the one-step actor's outputs: the data seeds are the smallest from DATA_SEED on that keep MARGIN from |a| = 1
_case('rows16/scaled', 'rows16', scaled=True, seed=4)
_case('side32/scaled', 'side32', scaled=True, seed=5)
_case('side32/c10_q200_scaled', 'side32', c=C_OFFSET, q0=-200.0, scaled=True, cfg=Q_CFG, seed=5)
for _b in ('rows16', 'side32', 'side64', 'padded250'):
    for _c in C_DEAD:
        _case(f'{_b}/dead{int(_c)}', _b, dead=_c)
# 30 w / w is exact at widths 256 and 64, so the three c = 30 cases above never reach a clamp; these do, one per site that computes a variance
CLAMP_CASES = ['padded250/dead30']
for _b in ('side32_w250', 'side64_w250', 'split_w250'):
    _case(f'{_b}/dead30', _b, dead=30.0)
    CLAMP_CASES.append(f'{_b}/dead30')

GPU_CASES = list(FQL_CASES)          # what tests/test_gpu_conditioning.py runs; the twins below are CPU-only baselines of the regime checks
for _b in ('rows16', 'side32', 'side32_h64', 'side64', 'split', 'kbig', 'padded', 'chain_ln'):
    _case(f'{_b}/plain', _b)

OFFSET_CASES = [n for n, k in FQL_CASES.items() if k['c'] is not None]
Q_CASES = [n for n, k in FQL_CASES.items() if k['q0'] is not None]
SCALED_ONLY = [n for n, k in FQL_CASES.items() if k['scaled'] and k['c'] is None and k['q0'] is None]
DEAD_CASES = [n for n, k in FQL_CASES.items() if k['dead'] is not None]
FORWARD_CASE, FORWARD_NS = 'chain_ln/c10', (1, 5, 33)


# ---- problem builders ----------------------------------------------------------------------------------------------------------------
def _f32(tree):
    return O.tree_map(lambda a: np.array(a, dtype=np.float32), tree)


def _offset_net(net, c, keep_last):
    n = O._n_layers(net)
    for i in range(n - 1 if keep_last else n):
        b = net[f'Dense_{i}']['bias']
        b += np.asarray(c, b.dtype)


def offset_params(params, c, nets):
    """A copy with c added to every hidden Dense bias (every Dense but the last) of the named nets, both ensemble members; the critic and
    the target critic move together."""
    nets = set(nets)
    if nets & set(CRITICS):
        nets |= set(CRITICS)
    out = _f32(params)
    for m in nets:
        _offset_net(out[m]['value_net' if 'value_net' in out[m] else 'mlp'], c, keep_last=True)
    return out


def q_offset(params, q0, nets=CRITICS):
    """A copy with q0 added to the last Dense bias of the critic and of the target critic."""
    out = _f32(params)
    for m in nets:
        net = out[m]['value_net']
        b = net[f'Dense_{O._n_layers(net) - 1}']['bias']
        b += np.float32(q0)
    return out


def scaled_obs(batch):
    out = dict(batch)
    for k in ('observations', 'next_observations'):
        if k in out:
            out[k] = (np.float32(5.0) * out[k] + np.float32(30.0)).astype(np.float32)
    return out


def dead_layer(params, c):
    """A copy with the critic's Dense_1 kernel 0 and bias exactly c, both members, and the same in the target critic."""
    out = _f32(params)
    for m in CRITICS:
        d = out[m]['value_net']['Dense_1']
        d['kernel'][...] = 0.0
        d['bias'][...] = np.float32(c)
    return out


def fql_problem(name, **cfgkw):
    """(cfg, batch, noise, params) of an FQL_CASES entry, fp32 leaves; cfgkw: further config."""
    k = FQL_CASES[name]
    B, hidden, base_cfg = BASES[k['base']]
    cfg, ds, batch, noise = make_problem(OD, AD, B, hidden, seed=k['seed'], **dict(base_cfg, **dict(k['cfg'], **cfgkw)))
    params = randomize_params(O.init_params(INIT_SEED, OD, AD, cfg), seed=RANDOMIZE_SEED, scale=0.05 if max(hidden) >= 256 else 0.1)
    if k['c'] is not None:
        params = offset_params(params, k['c'], CRITICS + (ACTORS if cfg['actor_layer_norm'] else ()))
    if k['q0'] is not None:
        params = q_offset(params, k['q0'])
    if k['dead'] is not None:
        params = dead_layer(params, k['dead'])
    if k['scaled']:
        batch = scaled_obs(batch)
    return cfg, batch, noise, params


def oracle_cfg(cfg):
    ocfg = dict(cfg)
    ocfg['precision'] = 'fp32'     # (the oracle's precision is its dtype, whatever the engine's mode)
    return ocfg


def fql_oracle(name, dtype):
    cfg, batch, noise, params = fql_problem(name)
    return O.OracleFQL(params, oracle_cfg(cfg), OD, AD, dtype), batch, noise


# IQL (ddpgbc, log_stds) and BC: (obs, act, B, hidden); tests/test_gpu_iql.py's and tests/test_gpu_bc.py's recipes, then the offsets
IQL_SHAPE, IQL_SEED = (29, 8, 64, 128), 4
IQL_NETS = ('modules_critic', 'modules_target_critic', 'modules_value')
IQL_CASES = {'iql/c10': dict(c=C_OFFSET, q0=None), 'iql/q200': dict(c=None, q0=-200.0), 'iql/plain': dict(c=None, q0=None)}
BC_SHAPE, BC_SEED = (29, 8, 64, 64), 1
BC_CASES = {'bc/c10': dict(c=C_OFFSET, scaled=False), 'bc/scaled': dict(c=None, scaled=True), 'bc/plain': dict(c=None, scaled=False)}
OTHER_GPU_CASES = [n for n in list(IQL_CASES) + list(BC_CASES) if not n.endswith('/plain')]


def iql_problem(name):
    """(cfg, batch, noise, params): ddpgbc with log_stds and actor LayerNorm; c on every net (all have LayerNorm), q0 on the critic, the
    target critic and the value net (all three estimate the same return).  The noise is cleared of the |x| = 1 kink at these parameters."""
    k = IQL_CASES[name]
    od, ad, B, H = IQL_SHAPE
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=B, actor_loss='ddpgbc', const_std=False,
               actor_layer_norm=True)
    if k['q0'] is not None:
        cfg['discount'] = 0.995
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=IQL_SEED)
    batch = O.sample_batch(ds, np.random.default_rng(IQL_SEED + 1).integers(0, len(ds['observations']), size=B))
    noise = IO.make_noise(B, ad, IQL_SEED + 2)
    params = _f32(IO.randomize(IO.init_params(IQL_SEED + 3, od, ad, cfg), IQL_SEED + 4))
    if k['c'] is not None:
        for m in IQL_NETS:
            _offset_net(params[m]['value_net'], k['c'], keep_last=True)
        _offset_net(params['modules_actor']['actor_net'], k['c'], keep_last=False)     # activate_final: every Dense is hidden
    if k['q0'] is not None:
        params = q_offset(params, k['q0'], IQL_NETS)
    ref = IO.OracleIQL(params, dict(cfg), IQL_SHAPE[0], IQL_SHAPE[1], np.float64)
    return cfg, batch, IO.clear_of_unit_clip(ref, batch, noise, MARGIN), params


def iql_oracle(name, dtype):
    cfg, batch, noise, params = iql_problem(name)
    return IO.OracleIQL(params, dict(cfg), IQL_SHAPE[0], IQL_SHAPE[1], dtype), batch, noise


def bc_problem(name):
    """(cfg, batch, noise, params): BC has LayerNorm in its one net (MLP_0, activate_final) and no critic, so no large-return case."""
    k = BC_CASES[name]
    od, ad, B, H = BC_SHAPE
    cfg = BO.get_config()
    cfg.update(hidden_dims=(H,) * 4, batch_size=B)
    rng = np.random.default_rng(BC_SEED)
    batch = {'observations': rng.standard_normal((B, od)).astype(np.float32),
             'actions': np.clip(rng.standard_normal((B, ad)), -1, 1).astype(np.float32)}
    noise = BO.make_noise(B, ad, cfg['denoise_steps'], BC_SEED + 100)
    params = _f32(BO.init_params(INIT_SEED, od, ad, cfg))
    rng = np.random.default_rng(RANDOMIZE_SEED)
    for p, v in O.tree_leaves_with_path(params):
        if not p.endswith('/kernel'):
            v += (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    if k['c'] is not None:
        _offset_net(params['MLP_0'], k['c'], keep_last=False)
    if k['scaled']:
        batch = scaled_obs(batch)
    return cfg, batch, noise, params


def bc_oracle(name, dtype):
    cfg, batch, noise, params = bc_problem(name)
    return BO.OracleBC(params, dict(cfg), BC_SHAPE[0], BC_SHAPE[1], dtype), batch, noise


BC_SAMPLE_ATOL = 2e-5       # tests/test_gpu_bc.py's bound on sampled actions
_BC_FWD = {}


def bc_sampler_rows(name, n=33):
    """(observations, noises) of the BC sampler check: fresh rows, scaled where the case's batch is."""
    rng = np.random.default_rng(BC_SEED + 7)
    obs = rng.standard_normal((n, BC_SHAPE[0])).astype(np.float32)
    z = rng.standard_normal((n, BC_SHAPE[1])).astype(np.float32)
    return (scaled_obs({'observations': obs})['observations'] if BC_CASES[name]['scaled'] else obs), z


def bc_sampler_yardstick(name):
    """(fp64 sample_actions on bc_sampler_rows, max over the variants of the largest element error in fp32)."""
    if name not in _BC_FWD:
        obs, z = bc_sampler_rows(name)
        want = bc_oracle(name, np.float64)[0].sample_actions(obs, z)
        err = 0.0
        for v in VARIANTS:
            with variant_context(v):
                got = bc_oracle(name, np.float32)[0].sample_actions(obs, z)
            err = max(err, float(np.abs(got.astype(np.float64) - want).max()))
        _BC_FWD[name] = (want, err)
    return _BC_FWD[name]


def oracle_of(name, dtype):
    return (iql_oracle if name in IQL_CASES else bc_oracle if name in BC_CASES else fql_oracle)(name, dtype)


# ---- fp32 LayerNorm variants -----------------------------------------------------------------------------------------------------------
_ORIG_LAYER_NORM = O.layer_norm


def sequential_layer_norm(fused, raw_log=None, clamp=True):
    """O.layer_norm for fp32 arrays with sequential fp32 row sums times an fp32 1 / width; other dtypes go to the oracle's own.  raw_log:
    a list that receives (largest spread max - min of a row of x, the unclamped s2 inv - mean^2 [rows, 1]) of every call."""
    def layer_norm(x, scale, bias):
        if x.dtype != np.float32:
            return _ORIG_LAYER_NORM(x, scale, bias)
        inv = np.float32(1.0) / np.float32(x.shape[-1])
        s = np.cumsum(x, axis=-1, dtype=np.float32)[..., -1:]
        s2 = np.cumsum(x * x, axis=-1, dtype=np.float32)[..., -1:]
        mean = s * inv
        if fused:   # (a product of two fp32 numbers is exact in fp64: one rounding, as an fma)
            raw = (s2.astype(np.float64) * np.float64(inv) - mean.astype(np.float64) * mean.astype(np.float64)).astype(np.float32)
        else:
            raw = s2 * inv - mean * mean
        if raw_log is not None:
            raw_log.append((float((x.max(axis=-1) - x.min(axis=-1)).max()), raw))
        with np.errstate(invalid='ignore'):
            rstd = np.float32(1.0) / np.sqrt((np.maximum(np.float32(0.0), raw) if clamp else raw) + np.float32(O.LN_EPS))
        xhat = (x - mean) * rstd
        return xhat * scale + bias, xhat, rstd
    return layer_norm


def mistaken_layer_norm(kind):
    """The oracle's layer_norm with a kernel's mistake in its statistics, any dtype: 'pad_column' one zero pad column counted into both
    sums (width + 1 terms), 'drop_partial' the last 32 columns missing from both sums."""
    def layer_norm(x, scale, bias):
        n = x.shape[-1]
        if kind == 'pad_column':
            mean, mean2 = x.sum(axis=-1, keepdims=True) / (n + 1), (x * x).sum(axis=-1, keepdims=True) / (n + 1)
        else:
            mean, mean2 = x[..., :n - 32].sum(axis=-1, keepdims=True) / n, (x * x)[..., :n - 32].sum(axis=-1, keepdims=True) / n
        rstd = 1.0 / np.sqrt(np.maximum(0.0, mean2 - mean * mean) + x.dtype.type(O.LN_EPS))
        xhat = (x - mean) * rstd
        return xhat * scale + bias, xhat, rstd
    return layer_norm


@contextlib.contextmanager
def swapped_layer_norm(fn):
    """O.layer_norm replaced by fn inside the block (the oracle's own code is untouched), restored whatever happens."""
    try:
        O.layer_norm = fn
        yield
    finally:
        O.layer_norm = _ORIG_LAYER_NORM


def variant_context(variant, raw_log=None):
    if variant == 'pairwise':
        return contextlib.nullcontext()
    return swapped_layer_norm(sequential_layer_norm(variant == 'fused', raw_log))


def recording_layer_norm(log):
    """The oracle's layer_norm, recording per call (min over the rows of |mean| / std, rstd) of its input."""
    def layer_norm(x, scale, bias):
        out = _ORIG_LAYER_NORM(x, scale, bias)
        std = x.std(axis=-1)
        log.append((float((np.abs(x.mean(axis=-1)) / np.maximum(std, 1e-300)).min()), out[2]))
        return out
    return layer_norm


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
class Frozen:
    """One oracle's answers for one problem, computed once and read-only: grads, then update, with the interface tests/util.py's helpers
    use (after update(), .params are the post-step parameters)."""

    def __init__(self, ref, batch, noise):
        self._grads = ref.grads(batch, noise)
        self._update = ref.update(batch, noise)
        self.params = ref.params
        for tree in (self._grads[2], self.params):
            for _, leaf in O.tree_leaves_with_path(tree):
                leaf.flags.writeable = False

    def grads(self, batch=None, noise=None): return self._grads
    def update(self, batch=None, noise=None): return self._update


class Yardstick:
    """truth: the fp64 Frozen.  grad[variant][leaf] = max|g32 - g64| / max|g64|, info[variant][key] = |i32 - i64|; grads / infos: the
    maximum over the variants."""

    def __init__(self, name):
        ref, batch, noise = oracle_of(name, np.float64)
        self.truth = Frozen(ref, batch, noise)
        g64, i64 = leaf_dict(self.truth.grads()[2]), self.truth.update()[1]
        self.grad, self.info = {}, {}
        for v in VARIANTS:
            with variant_context(v):
                ref32, batch, noise = oracle_of(name, np.float32)
                f = Frozen(ref32, batch, noise)
            g32, i32 = leaf_dict(f.grads()[2]), f.update()[1]
            self.grad[v] = {p: float(np.abs(g32[p].astype(np.float64) - g).max() / max(np.abs(g).max(), 1e-30)) for p, g in g64.items()}
            self.info[v] = {k: abs(float(i32[k]) - float(i64[k])) for k in i64}
        self.grads = {p: max(self.grad[v][p] for v in VARIANTS) for p in g64}
        self.infos = {k: max(self.info[v][k] for v in VARIANTS) for k in i64}

    def worst(self, variant):
        """(worst gradient figure of a variant over the leaves that have a gradient, its leaf)."""
        g64 = leaf_dict(self.truth.grads()[2])
        return max((e, p) for p, e in self.grad[variant].items() if np.abs(g64[p]).max() > 0)

    def grad_tol(self, leaf, floor=GRAD_BOUND):
        """Relative to the leaf's largest fp64 gradient."""
        return max(floor, FACTOR * self.grads[leaf])

    def info_tol(self, key, floor):
        return max(floor, FACTOR * self.infos[key])


_YARD = {}


def yardstick(name):
    """The Yardstick of a case, computed once per process and shared."""
    if name not in _YARD:
        _YARD[name] = Yardstick(name)
    return _YARD[name]


def forward_rows(n, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((33, OD)).astype(np.float32)[:n], rng.standard_normal((33, AD)).astype(np.float32)[:n],
            rng.uniform(-1, 1, (33, AD)).astype(np.float32)[:n])


def _forward(ref, obs, z, act):
    return {'sample_actions': ref.sample_actions(obs, z), 'compute_flow_actions': ref.compute_flow_actions(obs, z),
            'critic': ref._critic('modules_critic', ref._c(obs), ref._c(act))}


_FWD = {}


def forward_yardstick(name=FORWARD_CASE):
    """(fp64 answers on the 33 forward rows, {query: max over the variants of the largest element error})."""
    if name not in _FWD:
        obs, z, act = forward_rows(33)
        want = _forward(fql_oracle(name, np.float64)[0], obs, z, act)
        err = dict.fromkeys(want, 0.0)
        for v in VARIANTS:
            with variant_context(v):
                got = _forward(fql_oracle(name, np.float32)[0], obs, z, act)
            for q in want:
                err[q] = max(err[q], float(np.abs(got[q].astype(np.float64) - want[q]).max()))
        _FWD[name] = (want, err)
    return _FWD[name]


# ---- conditions ------------------------------------------------------------------------------------------------------------------------
def layer_norm_inputs(name):
    """[(min |row mean| / row std, rstd)] of every LayerNorm call of the case's fp64 gradient pass."""
    log = []
    ref, batch, noise = oracle_of(name, np.float64)
    with swapped_layer_norm(recording_layer_norm(log)):
        ref.grads(batch, noise)
    return log


def dead_layer_raw_variance(name, fused):
    """The unclamped variances of the sequential fp32 variant at the critic's LayerNorm_1 over one gradient pass: [array [rows, 1]]."""
    raw = []
    ref, batch, noise = oracle_of(name, np.float32)
    with variant_context('fused' if fused else 'sequential', raw):
        ref.grads(batch, noise)
    return [r for spread, r in raw if spread == 0.0]      # the dead layer's calls: one value in every column of every row


def fql_kink_margins(name):
    """Distance of the fp64 pass from the points where FQL's loss is not smooth: |a| = 1 of the one-step actor's clipped output (the
    inside mask of the Q term), and, under q_agg='min', q1 = q2 of the target critic pair at the next actions."""
    ref, batch, noise = fql_oracle(name, np.float64)
    obs, nobs = ref._c(batch['observations']), ref._c(batch['next_observations'])
    a_raw = ref._actor('modules_actor_onestep_flow', obs, ref._c(noise['z']))
    m = {'unit_clip': float(np.abs(np.abs(a_raw) - 1.0).min())}
    if ref.config['q_agg'] == 'min':
        nq = ref._critic('modules_target_critic', nobs, ref.sample_actions(nobs, noise['eps1']))
        m['q_tie'] = float(np.abs(nq[0] - nq[1]).min())
    return m


def q_cancellation(name):
    """(|mean q|, median |q - target| over both members and the rows) of the critic loss in fp64."""
    ref, batch, noise = oracle_of(name, np.float64)
    if name in IQL_CASES:
        f = ref._forward(batch, noise)
        q, target = f['cq'], f['y']
    else:
        obs, nobs = ref._c(batch['observations']), ref._c(batch['next_observations'])
        nq = ref._critic('modules_target_critic', nobs, ref.sample_actions(nobs, noise['eps1']))
        nq = nq.min(axis=0) if ref.config['q_agg'] == 'min' else nq.mean(axis=0)
        target = ref._c(batch['rewards']).reshape(-1) + ref.config['discount'] * ref._c(batch['masks']).reshape(-1) * nq
        q = ref._critic('modules_critic', obs, ref._c(batch['actions']))
    return float(np.abs(q.mean())), float(np.median(np.abs(q - target)))


def is_split(name):
    return name in FQL_CASES and BASES[FQL_CASES[name]['base']][2].get('precision') == 'bf16x3'


def grad_floor(name):
    """The existing per-leaf gradient bound of the case's precision, relative to the leaf's largest gradient."""
    if name in IQL_CASES:
        return 5e-5                                    # tests/test_gpu_iql.py's bound
    return BF16X3_BOUND if is_split(name) else GRAD_BOUND


def info_floor(name, want):
    """The existing bound on an info of value `want`: assert_step_matches' in fp32, test_gpu_precision.py's in bf16x3."""
    return BF16X3_BOUND * max(1.0, abs(want)) if is_split(name) else INFO_ATOL + INFO_RTOL * abs(want)
