"""The FQL problems of the padded-width tests (tests/test_gpu_padded_widths.py, tests/test_padded_widths_cpu.py), built on the CPU from
numpy and the oracle alone: configuration, dataset, batch, noise and randomized parameters (set into the engine with set_params).

The engine pads every hidden width to a multiple of 16 (fql_amd/csrc/fql_engine.hip: out_p = pad16(out), in_p = pad16(in) above the
first layer).  Every tuple here holds a width that is no multiple of 16, so every case runs the code that exists only for out < out_p:
LayerNorm over `width` of `out_p` columns, its backward's masked sums, the zeroed padding of every gradient, the strided copies behind
get_params / set_params, and the path choices made on the padded size.
"""
import numpy as np

from oracle import fql_oracle as O
from tests.util import make_problem, randomize_params

#   id: (obs, act, B, hidden, cfg overrides)
FQL_CASES = {
    'w50': (29, 8, 32, (50, 50, 50), {}),                                    # pad 14, width % 4 = 2, one 64-column tile
    'w33_100_17': (29, 8, 32, (33, 100, 17), dict(q_agg='min')),           # pads 15 / 12 / 15; 17: one real column in its second 16-block
    'w50_actor_ln': (29, 8, 32, (50, 50, 50), dict(actor_layer_norm=True)),  # LayerNorm and its backward in the actor nets
    'w100_no_ln': (29, 8, 16, (100, 100), dict(layer_norm=False)),         # padding kept zero by zero weights alone, minimum batch
    'w250': (29, 8, 64, (250,) * 4, {}),                                     # out_p 256: chain<256> must not be taken
    'w500': (29, 8, 64, (500,) * 4, {}),                                     # out_p 512: no chain; OP_DGRAD0 at K 512 with 500 valid
    'w300_b256': (29, 8, 256, (300, 300, 300), {}),                          # out_p 304 at M 256
    'w300_b1024': (40, 4, 1024, (300, 300), dict(alpha=300.0)),            # out_p 304 at M 1024
    'w1000': (29, 8, 32, (1000,) * 3, {}),                                   # K > 512 kernels at K = 1008
    # added to the cases asked for: fql_side_big_kernel's 64-row tiles take N % 64 == 0 and K % 64 == 0 only, which out_p 304 is not, so
    # w300_b1024 cannot reach them (tests/test_gpu_padded_widths.py); out_p 256 at M 1024 does, with 250 valid columns
    'w250_b1024': (40, 4, 1024, (250, 250), dict(alpha=300.0)),
}
DATA_SEED, INIT_SEED, RANDOMIZE_SEED = 3, 7, 5


def pad16(w):
    return (w + 15) & ~15


def fql_problem(cid, **cfgkw):
    """(cfg, ds, batch, noise, params) of an FQL_CASES entry; cfgkw: further config (precision)."""
    od, ad, B, hidden, kw = FQL_CASES[cid]
    cfg, ds, batch, noise = make_problem(od, ad, B, hidden, seed=DATA_SEED, **dict(kw, **cfgkw))
    params = randomize_params(O.init_params(INIT_SEED, od, ad, cfg), seed=RANDOMIZE_SEED, scale=0.05 if max(hidden) >= 256 else 0.1)
    return cfg, ds, batch, noise, params


class FrozenRef:
    """The fp64 oracle's answers for one (params, batch, noise), computed once: total_loss, grads, then update, with the interface the
    assert helpers of tests/util.py use (after update(), .params are the post-step parameters).  The arrays are read-only."""

    def __init__(self, params, cfg, od, ad, batch, noise):
        ref = O.OracleFQL(params, dict(cfg), od, ad, np.float64)
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


def later_step(cid, ds, step):
    """(batch, noise) of update `step` >= 1 after the first: fresh rows and fresh noise."""
    od, ad, B = FQL_CASES[cid][:3]
    idx = np.random.default_rng(100 + step).integers(0, len(ds['observations']), size=B)
    return O.sample_batch(ds, idx), O.make_noise(B, ad, 40 + step)
