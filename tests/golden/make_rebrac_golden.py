#!/usr/bin/env python3
"""Generates tests/golden/rebrac/rebrac_small.npz from the ReBRAC CPU restatement (tests/rebrac_oracle.py, float64).  Run from the repo root:

    python tests/golden/make_rebrac_golden.py

Like the FQL and IFQL fixtures these vectors pin the restatement of agents/rebrac.py, not JAX.  The file holds the inputs (params, a batch
with next_actions, eps1 noise, a small dataset with the rows and noise of a short trajectory on the actor_freq = 2 schedule, sample
observations and noise) and the expected outputs: the 9 infos of total_loss, the 12 of a full update and the 7 of the critic-only update
after it, per-leaf gradients of the full step, parameters after both steps, the infos of every trajectory step with per-leaf checksums
after it, and sample_actions at temperature 0.5.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import fql_oracle as O  # noqa: E402
from tests import rebrac_oracle as RO  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OD, AD, B, HIDDEN, STEPS, SEED = 7, 3, 16, (32, 32, 32, 32), 6, 4321


def build():
    cfg = RO.get_config()
    cfg.update(actor_hidden_dims=HIDDEN, value_hidden_dims=HIDDEN, batch_size=B, alpha_actor=0.5, alpha_critic=0.2)
    params = RO.init_params(SEED, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(SEED + 1)
    for path, leaf in O.tree_leaves_with_path(params):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += 0.1 * rng.standard_normal(leaf.shape)
        if path.endswith('mean_net/kernel'):
            leaf *= 30.0
    for m in ('actor', 'critic'):
        params[f'modules_target_{m}'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), params[f'modules_{m}'])
    params = O.tree_map(lambda a: a.astype(np.float32), params)
    ds = O.make_synthetic_dataset(4 * B, OD, AD, seed=SEED)
    idx = rng.integers(0, 4 * B, size=B)
    idx[0] = 4 * B - 1
    batch = RO.make_batch(ds, idx)
    noise = {'eps1': rng.standard_normal((B, AD)).astype(np.float32)}
    noise2 = {'eps1': rng.standard_normal((B, AD)).astype(np.float32)}
    traj_idx = rng.integers(0, 4 * B, size=(STEPS, B))
    traj_eps = rng.standard_normal((STEPS, B, AD)).astype(np.float32)
    sample_obs = ds['observations'][:5]
    sample_noise = (3.0 * rng.standard_normal((5, AD))).astype(np.float32)

    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    loss, info_tl = ref.total_loss(batch, noise)
    _, _, grads = ref._losses(batch, noise, want_grads=True)
    action = ref.sample_actions(sample_obs, sample_noise, temperature=0.5)
    _, info_up = ref.update(batch, noise, full_update=True)
    _, info_cr = ref.update(batch, noise2, full_update=False)
    new_params = O.tree_map(np.copy, ref.params)
    traj_info, traj_sums = [], []
    for s in range(STEPS):
        full = s % cfg['actor_freq'] == 0
        _, inf = ref.update(RO.make_batch(ds, traj_idx[s]), {'eps1': traj_eps[s]}, full_update=full)
        traj_info.append([inf[k] for k in RO.CRITIC_INFO_KEYS])
        traj_sums.append([float(np.sum(v)) for _, v in O.tree_leaves_with_path(ref.params)])

    out = {'meta': json.dumps(dict(obs_dim=OD, act_dim=AD, B=B, hidden=list(HIDDEN), steps=STEPS, alpha_actor=cfg['alpha_actor'],
                                   alpha_critic=cfg['alpha_critic'], leaves=[p for p, _ in O.tree_leaves_with_path(params)]))}
    for k, v in batch.items():
        out[f'batch/{k}'] = v
    out['noise/eps1'] = noise['eps1']
    out['noise2/eps1'] = noise2['eps1']
    for k, v in ds.items():
        out[f'dataset/{k}'] = v
    for p, v in O.tree_leaves_with_path(params):
        out[f'params/{p}'] = v
    for p, v in O.tree_leaves_with_path(grads):
        out[f'grads/{p}'] = v.astype(np.float32)
    for p, v in O.tree_leaves_with_path(new_params):
        out[f'new_params/{p}'] = v.astype(np.float32)
    out['total_loss'] = np.float64(loss)
    out['info_total_loss'] = np.array([float(info_tl[k]) for k in RO.INFO_KEYS[:9]])
    out['info_update'] = np.array([float(info_up[k]) for k in RO.INFO_KEYS])
    out['info_critic_update'] = np.array([float(info_cr[k]) for k in RO.CRITIC_INFO_KEYS])
    out['traj/idx'] = traj_idx
    out['traj/eps1'] = traj_eps
    out['traj/info'] = np.array(traj_info)
    out['traj/leaf_sums'] = np.array(traj_sums)
    out['sample/observations'] = sample_obs
    out['sample/noise'] = sample_noise
    out['sample/action'] = action.astype(np.float32)
    return out


def main():
    path = os.path.join(HERE, 'rebrac', 'rebrac_small.npz')   # (a directory of its own: the FQL fixture tests take every golden/*.npz)
    np.savez_compressed(path, **build())
    print('rebrac_small', 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
