"""The problems the IFQL path tests run (tests/test_gpu_ifql_paths.py), built on the CPU from numpy and the oracles alone: configuration,
randomized parameters (set into the engine with set_params), batch and the noise of each step.

IFQL's losses are C1 in everything they differentiate: the expectile weight switches at q = v but multiplies (q - v)^2, so the value
gradient is continuous there; min(q1, q2) of the target pair and the critic's target carry no gradient; the flow loss is a plain square.
No row can take "the other branch's gradient" in fp32, so these cases need no kink margins and no chosen seeds (ReBRAC's do:
tests/rebrac_cases.py).

PATHS are the shapes and batches at which the update's kernels change; tests/test_gpu_ifql_paths.py asserts each path from the engine's
plan before and after it compares numbers.  Every pass of the value net runs at 2B rows (obs and next_obs), every other pass at B, and
the value net's backward covers rows [0, B) of its 2B-row pass.
"""
import numpy as np

from oracle import fql_oracle as O
from tests import ifql_oracle as IO
from tests.util import randomize_params

H512, H64 = (512,) * 4, (64,) * 4

#   id: (obs, act, B, actor hidden, value hidden, cfg overrides, seed)
PATHS = {
    # one side launch holds the value pass at M 1024 on 64-row tiles and the target critics at M 512 on 32-row tiles
    'b512_mixed': (29, 8, 512, H512, H512, {}, 100),
    # M 544 and 272, no multiple of 64: the 16-row kernel everywhere, a weight-gradient tail of 17 steps of 16, LayerNorm backward's
    # partial second trip of 256
    'b272': (29, 8, 272, H512, H512, {}, 110),
    # M 1088 = 17 x 64 on big tiles beside M 544 on the 16-row kernel
    'b544_h64': (11, 5, 544, H64, H64, {}, 120),
    # M 2080 and 1040: the 16-row fallback above 1024 rows
    'b1040_h64': (11, 5, 1040, H64, H64, {}, 130),
    # M 4096 and 2048, both on 64-row tiles
    'b2048_h64': (11, 5, 2048, H64, H64, {}, 140),
    # K 1024: fql_gemm16_kernel<true> inside the three-lane program
    'wide1024': (29, 8, 48, (1024,) * 3, (1024,) * 3, {}, 150),
    # first layers with K 640 (value, critic and flow nets alike) on fql_gemm16_kernel<true>.  B 48, not 64: at M 64 and 128 the
    # 64-aligned [M, 64, 640] tasks go to fql_side_kernel's 32-row tiles, whose K loop has no 512 limit, and never reach the 16-row kernel
    'obs600': (600, 8, 48, (64,) * 3, (64,) * 3, {}, 160),
    'no_ln_h512': (29, 8, 256, H512, H512, dict(layer_norm=False), 170),
    # act == the padded width 16: no padding column, no task 32 wide
    'act16': (29, 16, 256, H512, H512, {}, 180),
    'b16': (7, 3, 16, H64, H64, {}, 190),
    # hidden widths that are no multiple of 16: out 50 of out_p 64, the value pass (M 64) on 32-row tiles and the B-row passes on the
    # 16-row kernel; out 500 of out_p 512 (the width class of the best-of-N sampler's nets), LayerNorm over 500 of 512 columns
    'w50_padded': (29, 8, 32, (50,) * 3, (50,) * 3, {}, 210),
    'w500_padded': (29, 8, 64, (500,) * 4, (500,) * 4, {}, 220),
}
# one hidden-512 handle through these batch sizes: 32-row tiles, the mixed 64 / 32-row launch, the 16-row kernel, one tile, and back
WALK = (29, 8, (256, 512, 272, 16, 256), 200)
# AQL queues against the captured graph, bitwise, at these PATHS
AQL_CASES = ('b512_mixed', 'b272')
# best-of-N sampling at hidden 512 with the padded action width 32: obs 69, act 21; (N, n) -> seed of the observations and noises
SAMPLER_SHAPE = (69, 21, H512, H512)
SAMPLER_CASES = {(1, 37): 1, (7, 590): 7, (65, 64): 65}
SAMPLER_GAP = 1e-2   # a clear winner: the top two scores further apart than this (tests/test_gpu_ifql.py)


def config(actor, value, B, **kw):
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=tuple(actor), value_hidden_dims=tuple(value), batch_size=B)
    cfg.update(kw)
    return cfg


def dataset(od, ad, B, seed):
    return O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)


def data(od, ad, B, seed, steps=2):
    """(batch, [noise of each step]) of one data seed."""
    ds = dataset(od, ad, B, seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    noises = []
    for i in range(steps):
        nz = O.make_noise(B, ad, seed + 2 + 75 * i)
        noises.append({'x0': nz['x0'], 't': nz['t']})
    return O.sample_batch(ds, idx), noises


def parameters(od, ad, cfg, seed):
    return randomize_params(IO.init_params(seed + 3, od, ad, cfg), seed + 4)


def problem(case):
    """(cfg, batch, params, noises) of a PATHS case: noises[i] is the draw of step i."""
    od, ad, B, actor, value, kw, seed = PATHS[case]
    cfg = config(actor, value, B, **kw)
    batch, noises = data(od, ad, B, seed)
    return cfg, batch, parameters(od, ad, cfg, seed), noises


def sampler_problem(N, n):
    """(cfg, params, obs [n, od], noises [n, N, act]) of a SAMPLER_CASES entry."""
    od, ad, actor, value = SAMPLER_SHAPE
    cfg = config(actor, value, 64, num_samples=N)
    params = randomize_params(IO.init_params(8, od, ad, cfg), 8)
    rng = np.random.default_rng(SAMPLER_CASES[(N, n)])
    obs = rng.standard_normal((n, od)).astype(np.float32)
    noises = (2.0 * rng.standard_normal((n, N, ad))).astype(np.float32)
    return cfg, params, obs, noises


def best_of_n(ref, obs, noises):
    """OracleIFQL.sample_actions for every row of obs [n, od] at once: the flow of each of the N noises, min(q1, q2), the first argmax.
    Returns the chosen actions [n, act], every candidate [n, N, act] and their scores [n, N]."""
    n, N, ad = noises.shape
    rep = np.repeat(obs, N, axis=0)
    acts = ref.compute_flow_actions(rep, noises.reshape(n * N, ad))
    q = ref._critic('modules_critic', rep, acts, stored=True).min(axis=0).reshape(n, N)
    acts = acts.reshape(n, N, ad)
    return acts[np.arange(n), np.argmax(q, axis=1)], acts, q


def clear_winners(q):
    """Rows of scores [n, N] whose top two are more than SAMPLER_GAP apart (every row at N = 1)."""
    if q.shape[1] == 1:
        return np.ones(len(q), bool)
    qs = np.sort(q, axis=1)
    return qs[:, -1] - qs[:, -2] > SAMPLER_GAP
