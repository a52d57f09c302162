#!/usr/bin/env python3
"""Generates tests/golden/iql/iql_small.npz from the IQL CPU restatement (tests/iql_oracle.py, float64).  Run from the repo root:

    python tests/golden/make_iql_golden.py

Like the other agents' fixtures these vectors pin the restatement of agents/iql.py, not JAX.  The file holds the inputs (parameters moved
away from init with const_std=False, a batch, the eps noise, a small dataset with the rows and noise of a short trajectory, sample
observations and noise) and, for each actor loss ('awr', 'ddpgbc') from the same inputs: the loss and infos of total_loss, the infos of
one update, its per-leaf gradients (and, for ddpgbc, the parameters after it), the infos of every trajectory step with per-leaf
checksums after it; and sample_actions at temperature 0.7.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import fql_oracle as O  # noqa: E402
from tests import iql_oracle as IO  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OD, AD, B, HIDDEN, STEPS, SEED = 7, 3, 16, (32, 32, 32), 6, 1358
BATCH = ('observations', 'actions', 'rewards', 'masks', 'next_observations')
LOSSES = ('awr', 'ddpgbc')


def build():
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=HIDDEN, value_hidden_dims=HIDDEN, batch_size=B, const_std=False, actor_layer_norm=True)
    rng = np.random.default_rng(SEED + 1)
    params = IO.randomize(IO.init_params(SEED, OD, AD, cfg), SEED + 3)
    params['modules_actor']['log_stds'] = np.array([-0.7, 0.4, -6.0], np.float32)   # inside, inside, past -5 (no gradient)
    ds = O.make_synthetic_dataset(4 * B, OD, AD, seed=SEED)
    idx = rng.integers(0, 4 * B, size=B)
    batch = {k: v for k, v in O.sample_batch(ds, idx).items() if k in BATCH}
    noise = IO.make_noise(B, AD, SEED + 2)
    traj_idx = rng.integers(0, 4 * B, size=(STEPS, B))
    traj_eps = rng.standard_normal((STEPS, B, AD)).astype(np.float32)
    sample_obs = ds['observations'][:5]
    sample_noise = rng.standard_normal((5, AD)).astype(np.float32)

    out = {'meta': json.dumps(dict(obs_dim=OD, act_dim=AD, B=B, hidden=list(HIDDEN), steps=STEPS, const_std=False, actor_layer_norm=True,
                                   leaves=[p for p, _ in O.tree_leaves_with_path(params)]))}
    for k, v in batch.items():
        out[f'batch/{k}'] = v
    out['noise/eps'] = noise['eps']
    for k in BATCH:
        out[f'dataset/{k}'] = ds[k]
    for p, v in O.tree_leaves_with_path(params):
        out[f'params/{p}'] = np.asarray(v, np.float32)
    out['traj/idx'] = traj_idx
    out['traj/eps'] = traj_eps
    out['sample/observations'] = sample_obs
    out['sample/noise'] = sample_noise
    for al in LOSSES:
        ref = IO.OracleIQL(params, dict(cfg, actor_loss=al), OD, AD, np.float64)
        assert min(ref.kink_margins(batch, noise).values()) >= 1e-3
        loss, info_tl = ref.total_loss(batch, noise)
        _, _, grads = ref._losses(batch, noise, want_grads=True)
        if al == 'awr':
            out['sample/action'] = ref.sample_actions(sample_obs, sample_noise, temperature=0.7).astype(np.float32)
        _, info_up = ref.update(batch, noise)
        new_params = O.tree_map(np.copy, ref.params)
        traj_info, traj_sums = [], []
        for s in range(STEPS):
            bt = {k: ds[k][traj_idx[s]] for k in BATCH}
            _, inf = ref.update(bt, {'eps': traj_eps[s]})
            traj_info.append([inf[k] for k in IO.INFO_KEYS[al]])
            traj_sums.append([float(np.sum(v)) for _, v in O.tree_leaves_with_path(ref.params)])
        for name, tree in (('grads', grads), ('new_params', new_params)):
            if name == 'new_params' and al == 'awr':
                continue   # (one post-step tree keeps the file small; the trajectory checksums cover awr's steps)
            for p, v in O.tree_leaves_with_path(tree):
                out[f'{al}/{name}/{p}'] = np.asarray(v, np.float32)
        out[f'{al}/total_loss'] = np.float64(loss)
        out[f'{al}/info_total_loss'] = np.array([float(info_tl[k]) for k in IO.INFO_KEYS[al][:-3]])
        out[f'{al}/info_update'] = np.array([float(info_up[k]) for k in IO.INFO_KEYS[al]])
        out[f'{al}/traj_info'] = np.array(traj_info)
        out[f'{al}/traj_leaf_sums'] = np.array(traj_sums)
    return out


def main():
    path = os.path.join(HERE, 'iql', 'iql_small.npz')   # (a directory of its own: the FQL fixture tests take every golden/*.npz)
    np.savez_compressed(path, **build())
    print('iql_small', 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
