"""The problems the ReBRAC path tests run (tests/test_gpu_rebrac_paths.py), built on the CPU from numpy and the oracles alone:
configuration, randomized parameters (set into the engine with set_params), batch and the noise of each step.

fql_rebrac_loss_actor_kernel hands a row's whole actor gradient to the smaller of q1, q2 at (obs, actor action): a row whose two values
agree to fp32 rounding flips sides against fp64 and moves every actor leaf by O(1 / B), which no tolerance may absorb.  So every case
carries a data seed, the smallest of 0..7 for which the fp64 restatement on its own trajectory keeps q_tie = min over rows |q1 - q2| >=
MARGIN in the first step and >= 3 MARGIN in every later full step (a later step runs, on the GPU, from the engine's own state, which
parts from the restatement's by up to 2 lr per element); tests/test_kink_margins_cpu.py checks that without a GPU, and the GPU tests
assert MARGIN at the state they actually step from.  The steps of a case are full, critic-only, full.

Every case found a seed, so none is dropped.  no_ln_h512_no_tanh is one-sided at its seed (without LayerNorm the second member is the
smaller on every row); in the other cases each member is the smaller on at least 20 % of the rows.
"""
import numpy as np

from oracle import fql_oracle as O
from tests import rebrac_oracle as RO
from tests.test_gpu_rebrac import _randomized as randomized   # (numpy only: biases / LN parameters off init, mean_net x 30, targets != online)
from tests.test_gpu_sac import MARGIN   # noqa: F401  (the margin of SAC's q_tie; the IQL and SAC cases use the same)

H512, H64 = (512,) * 4, (64,) * 4
STEP_KINDS = (True, False, True)   # full_update of the three steps of a case

#   id: (obs, act, B, actor hidden, value hidden, cfg overrides, data seed)
PATHS = {
    # M 272: the 16-row kernel everywhere; OP_DGRAD0 (K 512, M % 16 == 0, in_p 64, 29 + 16 <= 64)
    'b272': (29, 8, 272, H512, H512, {}, 0),
    # obs + 16 > in_p = 64 with act <= 16: the generic first-layer dgrad (M 256, N 64, K 512) at hidden 512
    'obs50': (50, 4, 256, H512, H512, {}, 0),
    # M 1040: the 16-row fallback above 1024 rows; the generic dgrad (K 64)
    'b1040_h64': (11, 5, 1040, H64, H64, {}, 1),
    # M 2048 on 64-row tiles
    'b2048_h64': (11, 5, 2048, H64, H64, {}, 6),
    # K 1024: fql_gemm16_kernel<true> inside the three-lane program, OP_DGRAD0 at K 1024
    'wide1024': (29, 8, 48, (1024,) * 3, (1024,) * 3, {}, 0),
    # first layers with K 640 on fql_gemm16_kernel<true>; the generic dgrad with N = in_p = 640, the action block at column 600.  B 48,
    # not 64: at M 64 the 64-aligned [64, 64, 640] tasks go to fql_side_kernel's 32-row tiles and never reach the 16-row kernel
    'obs600': (600, 8, 48, (64,) * 3, (64,) * 3, {}, 0),
    # no LayerNorm anywhere, no tanh; OP_DGRAD0 with all 16 columns live
    'no_ln_h512_no_tanh': (29, 16, 256, H512, H512, dict(layer_norm=False, actor_layer_norm=False, tanh_squash=False), 7),
    'b16': (7, 3, 16, H64, H64, {}, 0),
    # hidden widths that are no multiple of 16: out 50 of out_p 64, the 16-row kernel everywhere, the generic dgrad (K 64)
    'w50_padded': (29, 8, 32, (50,) * 3, (50,) * 3, {}, 0),
}
# one hidden-512 handle through these batch sizes, full and critic-only steps in turn; the data seed of the walk
WALK = (29, 8, (256, 512, 272, 16, 256), 1)
# AQL queues against the captured graph, bitwise, at these PATHS
AQL_CASES = ('b272', 'b1040_h64')


def config(actor, value, B, **kw):
    """tests/test_gpu_rebrac.py's _cfg: both BC penalties on."""
    cfg = RO.get_config()
    cfg.update(actor_hidden_dims=tuple(actor), value_hidden_dims=tuple(value), batch_size=B, alpha_actor=0.5, alpha_critic=0.3)
    cfg.update(kw)
    return cfg


def dataset(od, ad, B, seed):
    return O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)


def data(od, ad, B, seed, steps=len(STEP_KINDS)):
    """(batch, [noise of each step]) of one data seed."""
    ds = dataset(od, ad, B, seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    return RO.make_batch(ds, idx), [RO.make_noise(B, ad, seed + 2 + 75 * i) for i in range(steps)]


def parameters(od, ad, cfg, seed):
    return randomized(RO.init_params(seed + 3, od, ad, cfg), seed + 4)


def problem(case, seed=None):
    """(cfg, batch, params, noises) of a PATHS case at its recorded data seed (or `seed`): noises[i] is the draw of step i."""
    od, ad, B, actor, value, kw, case_seed = PATHS[case]
    seed = case_seed if seed is None else seed
    cfg = config(actor, value, B, **kw)
    batch, noises = data(od, ad, B, seed)
    return cfg, batch, parameters(od, ad, cfg, seed), noises


def walk_problem(seed=None):
    """(cfg, params, [(batch, noise, full_update) of each step]) of the batch-size walk: step i draws its rows and noise from seed + 10 i."""
    od, ad, sizes, walk_seed = WALK
    seed = walk_seed if seed is None else seed
    cfg = config(H512, H512, sizes[0])
    steps = []
    for i, B in enumerate(sizes):
        batch, noises = data(od, ad, B, seed + 10 * i, steps=1)
        steps.append((batch, noises[0], i % 2 == 0))
    return cfg, parameters(od, ad, cfg, seed), steps


def check_margin(ref, batch, factor=1, what=''):
    """The admission rule above on ref's current (fp64) parameters; returns the margin."""
    m = ref.kink_margins(batch)
    assert set(m) == {'q_tie'} and m['q_tie'] >= factor * MARGIN, (what, factor, m)
    return m['q_tie']


def first_member_share(ref, batch):
    a = ref._mode(ref.actor_mean('modules_actor', batch['observations']))
    qs = ref._critic('modules_critic', ref._c(batch['observations']), a, stored=True)
    return float(np.mean(qs[0] < qs[1]))
