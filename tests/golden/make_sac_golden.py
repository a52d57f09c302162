#!/usr/bin/env python3
"""Generates tests/golden/sac/sac_small.npz from the SAC CPU restatement (tests/sac_oracle.py, float64).  Run from the repo root:

    python tests/golden/make_sac_golden.py

Like the FQL, IFQL and ReBRAC fixtures these vectors pin the restatement of agents/sac.py, not JAX.  The file holds the inputs (parameters
moved away from init so that the log-std clip and tanh saturation occur, a batch, eps1 / eps2 noise, a small dataset and a replay ring
with the balanced rows and noise of a short trajectory, sample observations and noise) and the expected outputs: the 11 infos and the
loss of total_loss, the 14 infos of one update, its per-leaf gradients, the parameters and Adam moments after it, the infos of every
trajectory step with per-leaf checksums after it, and sample_actions at temperature 0.7.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import fql_oracle as O  # noqa: E402
from tests import sac_oracle as SO  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OD, AD, B, HIDDEN, STEPS, RING, SEED = 7, 3, 16, (32, 32, 32, 32), 6, 24, 2468
BATCH = ('observations', 'actions', 'rewards', 'masks', 'next_observations')


def build():
    cfg = SO.get_config()
    cfg.update(actor_hidden_dims=HIDDEN, value_hidden_dims=HIDDEN, batch_size=B, backup_entropy=True)
    rng = np.random.default_rng(SEED + 1)
    params = SO.init_params(SEED, OD, AD, cfg, np.float64)
    for path, leaf in O.tree_leaves_with_path(params):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += 0.1 * rng.standard_normal(leaf.shape)
        if path.endswith('mean_net/kernel') or path.endswith('log_std_net/kernel'):
            leaf *= 20.0
    params['modules_actor']['log_std_net']['bias'] += np.array([-9.0, 0.0, 6.0])   # past -5, inside, past 2
    params['modules_actor']['mean_net']['bias'] += np.array([3.0, -0.5, 0.5])        # tanh saturation on column 0
    params['modules_alpha']['log_value'] = np.asarray(-0.4)
    params['modules_target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), params['modules_critic'])
    params = O.tree_map(lambda a: np.asarray(a, np.float32), params)
    ds = O.make_synthetic_dataset(4 * B, OD, AD, seed=SEED)
    ring = {k: v[:RING].copy() for k, v in O.make_synthetic_dataset(RING, OD, AD, seed=SEED + 7).items() if k in BATCH}
    ring['rewards'] = (10.0 + np.arange(RING)).astype(np.float32)
    idx = rng.integers(0, 4 * B, size=B)
    batch = {k: v for k, v in O.sample_batch(ds, idx).items() if k in BATCH}
    noise = SO.make_noise(B, AD, SEED + 2)
    traj_ia = rng.integers(0, 4 * B, size=(STEPS, B // 2))
    traj_ib = rng.integers(0, RING, size=(STEPS, B // 2))
    traj_e1 = rng.standard_normal((STEPS, B, AD)).astype(np.float32)
    traj_e2 = rng.standard_normal((STEPS, B, AD)).astype(np.float32)
    sample_obs = ds['observations'][:5]
    sample_noise = rng.standard_normal((5, AD)).astype(np.float32)

    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    raw = ref.actor_heads(batch['observations'])[1]
    assert (raw < SO.LOG_STD_MIN).any() and (raw > SO.LOG_STD_MAX).any()
    loss, info_tl = ref.total_loss(batch, noise)
    _, _, grads = ref._losses(batch, noise, want_grads=True)
    action = ref.sample_actions(sample_obs, sample_noise, temperature=0.7)
    _, info_up = ref.update(batch, noise)
    new_params, new_mu, new_nu = (O.tree_map(np.copy, t) for t in (ref.params, ref.mu, ref.nu))
    traj_info, traj_sums = [], []
    for s in range(STEPS):
        bt = {k: np.concatenate([ds[k][traj_ia[s]], ring[k][traj_ib[s]]]) for k in BATCH}
        _, inf = ref.update(bt, {'eps1': traj_e1[s], 'eps2': traj_e2[s]})
        traj_info.append([inf[k] for k in SO.INFO_KEYS])
        traj_sums.append([float(np.sum(v)) for _, v in O.tree_leaves_with_path(ref.params)])

    out = {'meta': json.dumps(dict(obs_dim=OD, act_dim=AD, B=B, hidden=list(HIDDEN), steps=STEPS, ring=RING, backup_entropy=True,
                                   leaves=[p for p, _ in O.tree_leaves_with_path(params)]))}
    for k, v in batch.items():
        out[f'batch/{k}'] = v
    for k, v in noise.items():
        out[f'noise/{k}'] = v
    for k in BATCH:
        out[f'dataset/{k}'] = ds[k]
        out[f'ring/{k}'] = ring[k]
    for name, tree in (('params', params), ('grads', grads), ('new_params', new_params), ('new_mu', new_mu), ('new_nu', new_nu)):
        for p, v in O.tree_leaves_with_path(tree):
            out[f'{name}/{p}'] = np.asarray(v, np.float32)
    out['total_loss'] = np.float64(loss)
    out['info_total_loss'] = np.array([float(info_tl[k]) for k in SO.INFO_KEYS[:11]])
    out['info_update'] = np.array([float(info_up[k]) for k in SO.INFO_KEYS])
    out['traj/idx_dataset'] = traj_ia
    out['traj/idx_replay'] = traj_ib
    out['traj/eps1'] = traj_e1
    out['traj/eps2'] = traj_e2
    out['traj/info'] = np.array(traj_info)
    out['traj/leaf_sums'] = np.array(traj_sums)
    out['sample/observations'] = sample_obs
    out['sample/noise'] = sample_noise
    out['sample/action'] = action.astype(np.float32)
    return out


def main():
    path = os.path.join(HERE, 'sac', 'sac_small.npz')   # (a directory of its own: the FQL fixture tests take every golden/*.npz)
    np.savez_compressed(path, **build())
    print('sac_small', 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
