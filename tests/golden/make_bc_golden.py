"""Writes tests/golden/bc/bc_small.npz: a small BC problem (parameters, batch, noise) with the fp64 numpy oracle's loss, gradients,
post-update parameters and sampled actions.  Run from the repository root: python tests/golden/make_bc_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import bc_oracle as BO  # noqa: E402
from oracle import fql_oracle as O  # noqa: E402

OD, AD, B, S = 11, 3, 16, 4


def main():
    cfg = BO.get_config()
    cfg.update(hidden_dims=(32, 32), denoise_steps=S, batch_size=B)
    params = BO.init_params(7, OD, AD, cfg, np.float32)
    rng = np.random.default_rng(3)
    for _, v in O.tree_leaves_with_path(params):   # biases and LayerNorm leaves off their initial values
        v += (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    batch = {'observations': rng.standard_normal((B, OD)).astype(np.float32),
             'actions': np.clip(rng.standard_normal((B, AD)), -1, 1).astype(np.float32)}
    noise = BO.make_noise(B, AD, S, seed=5)
    sn = rng.standard_normal((5, AD)).astype(np.float32)
    ref = BO.OracleBC(params, cfg, OD, AD, np.float64)
    out = {}
    for p, v in O.tree_leaves_with_path(params):
        out['param/' + p] = v
    for k, v in {**batch, **noise}.items():
        out['in/' + k] = v
    out['in/sample_noise'] = sn
    out['out/actions'] = ref.sample_actions(batch['observations'][:5], sn)
    loss, _, grads = ref.grads(batch, noise)
    for p, v in O.tree_leaves_with_path(grads):
        out['grad/' + p] = v
    _, info = ref.update(batch, noise)
    out['out/info'] = np.array([info[k] for k in BO.INFO_KEYS], np.float64)
    for p, v in O.tree_leaves_with_path(ref.params):
        out['new/' + p] = v
    path = os.path.join(ROOT, 'tests', 'golden', 'bc', 'bc_small.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; loss', loss)


if __name__ == '__main__':
    main()
