#!/usr/bin/env python3
"""Generates tests/golden/ifql/ifql_small.npz from the IFQL CPU restatement (tests/ifql_oracle.py, float64).  Run from the repo root:

    python tests/golden/make_ifql_golden.py

Like the FQL fixtures (make_golden.py) these vectors pin the restatement of agents/ifql.py, not JAX.  The file holds the inputs (params,
batch, x0 / t noise, a small dataset with the rows and noise of a short trajectory, one observation with N sample noises) and the
expected outputs: the 9 infos of total_loss, the 12 of update, per-leaf gradients, post-step parameters, the 12 infos of every
trajectory step with per-leaf checksums after it, and the best-of-N action with its N scores.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import fql_oracle as O  # noqa: E402
from tests import ifql_oracle as IO  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OD, AD, B, HIDDEN, STEPS, SEED = 7, 3, 16, (32, 32, 32, 32), 5, 1234


def build():
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=HIDDEN, value_hidden_dims=HIDDEN, batch_size=B, num_samples=8)
    params = IO.init_params(SEED, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(SEED + 1)
    for path, leaf in O.tree_leaves_with_path(params):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += 0.1 * rng.standard_normal(leaf.shape)
    params['modules_target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), params['modules_critic'])
    params = O.tree_map(lambda a: a.astype(np.float32), params)
    ds = O.make_synthetic_dataset(4 * B, OD, AD, seed=SEED)
    batch = O.sample_batch(ds, rng.integers(0, 4 * B, size=B))
    noise = {'x0': rng.standard_normal((B, AD)).astype(np.float32), 't': rng.random(B).astype(np.float32)}
    traj_idx = rng.integers(0, 4 * B, size=(STEPS, B))
    traj_x0 = rng.standard_normal((STEPS, B, AD)).astype(np.float32)
    traj_t = rng.random((STEPS, B)).astype(np.float32)
    sample_noise = (2.0 * rng.standard_normal((cfg['num_samples'], AD))).astype(np.float32)

    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    loss, info_tl = ref.total_loss(batch, noise)
    _, _, grads = ref.grads(batch, noise)
    action, scores = ref.sample_actions(batch['observations'][0], sample_noise)
    _, info_up = ref.update(batch, noise)
    new_params = O.tree_map(np.copy, ref.params)
    traj_info, traj_sums = [], []
    for s in range(STEPS):
        _, inf = ref.update(O.sample_batch(ds, traj_idx[s]), {'x0': traj_x0[s], 't': traj_t[s]})
        traj_info.append([inf[k] for k in IO.INFO_KEYS])
        traj_sums.append([float(np.sum(v)) for _, v in O.tree_leaves_with_path(ref.params)])

    out = {'meta': json.dumps(dict(obs_dim=OD, act_dim=AD, B=B, hidden=list(HIDDEN), steps=STEPS, num_samples=cfg['num_samples'],
                                   leaves=[p for p, _ in O.tree_leaves_with_path(params)]))}
    for k, v in batch.items():
        out[f'batch/{k}'] = v
    for k, v in noise.items():
        out[f'noise/{k}'] = v
    for k, v in ds.items():
        out[f'dataset/{k}'] = v
    for p, v in O.tree_leaves_with_path(params):
        out[f'params/{p}'] = v
    for p, v in O.tree_leaves_with_path(grads):
        out[f'grads/{p}'] = v.astype(np.float32)
    for p, v in O.tree_leaves_with_path(new_params):
        out[f'new_params/{p}'] = v.astype(np.float32)
    out['total_loss'] = np.float64(loss)
    out['info_total_loss'] = np.array([float(info_tl[k]) for k in IO.INFO_KEYS[:9]])
    out['info_update'] = np.array([float(info_up[k]) for k in IO.INFO_KEYS])
    out['traj/idx'] = traj_idx
    out['traj/x0'] = traj_x0
    out['traj/t'] = traj_t
    out['traj/info'] = np.array(traj_info)
    out['traj/leaf_sums'] = np.array(traj_sums)
    out['sample/noise'] = sample_noise
    out['sample/action'] = action.astype(np.float32)
    out['sample/scores'] = scores
    return out


def main():
    path = os.path.join(HERE, 'ifql', 'ifql_small.npz')   # (a directory of its own: the FQL fixture tests take every golden/*.npz)
    np.savez_compressed(path, **build())
    print('ifql_small', 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
