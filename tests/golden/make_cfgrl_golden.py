"""Writes tests/golden/cfgrl/cfgrl_small.npz: a small CFGRL problem (parameters, batch, noise, dropout mask) with the fp64 numpy oracle's
loss, gradients (the masked unc_embed gradient among them), post-update parameters and sampled actions at cfg 0, 1 and 3, and the goal
indices tests/cfgrl_oracle.py::sample_goals gives on the six-trajectory dataset for recorded draws under the three probability mixes.
Run from the repository root: python tests/golden/make_cfgrl_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cfgrl_oracle as CO  # noqa: E402
from oracle import fql_oracle as O  # noqa: E402

OD, AD, GD, B, S = 11, 3, 5, 16, 4
HIDDEN = (32, 32)
CFGS = (0.0, 1.0, 3.0)
MIXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.2, 0.5, 0.3))
PATH = os.path.join(ROOT, 'tests', 'golden', 'cfgrl', 'cfgrl_small.npz')


def config():
    cfg = CO.get_config()
    cfg.update(actor_hidden_dims=HIDDEN, actor_layer_norm=True, flow_steps=S, batch_size=B)
    return cfg


def build():
    cfg = config()
    params = CO.init_params(7, OD, AD, GD, cfg, np.float32)
    rng = np.random.default_rng(3)
    for _, v in O.tree_leaves_with_path(params):   # biases and LayerNorm leaves off their initial values
        v += (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    batch = {'observations': rng.standard_normal((B, OD)).astype(np.float32),
             'actions': np.clip(rng.standard_normal((B, AD)), -1, 1).astype(np.float32),
             'actor_goals': rng.standard_normal((B, GD)).astype(np.float32)}
    noise = CO.make_noise(B, AD, seed=5)
    mask = np.zeros(B, bool)
    mask[[0, 6, B - 1]] = True
    sn = rng.standard_normal((5, AD)).astype(np.float32)
    ref = CO.OracleCFGRL(params, cfg, OD, AD, GD, np.float64)
    out = {}
    for p, v in O.tree_leaves_with_path(params):
        out['param/' + p] = v
    for k, v in {**batch, **noise}.items():
        out['in/' + k] = v
    out['in/do_cfg'] = mask
    out['in/sample_noise'] = sn
    for c in CFGS:
        out[f'out/actions_cfg{c:g}'] = ref.sample_actions(batch['observations'][:5], batch['actor_goals'][:5], sn, c)
    _, _, grads = ref.grads(batch, noise, mask)
    for p, v in O.tree_leaves_with_path(grads):
        out['grad/' + p] = v
    _, info = ref.update(batch, noise, mask)
    out['out/info'] = np.array([info[k] for k in CO.INFO_KEYS], np.float64)
    for p, v in O.tree_leaves_with_path(ref.params):
        out['new/' + p] = v
    ds = CO.make_gc_dataset(OD, AD, seed=11)
    out['goal/terminals'] = ds['terminals']
    n = len(ds['terminals'])
    out['goal/idx'] = np.tile(np.arange(n), 2)
    for k in ('random', 'dist', 'traj', 'cur'):
        out['goal/draw_' + k] = rng.integers(0, 2 ** 32, size=2 * n, dtype=np.uint64).astype(np.uint32)
    draws = {k: out['goal/draw_' + k] for k in ('random', 'dist', 'traj', 'cur')}
    for i, mix in enumerate(MIXES):
        out[f'goal/mix{i}'] = CO.sample_goals(out['goal/idx'], ds['terminals'], draws, *mix).astype(np.int64)
    return out


if __name__ == '__main__':
    np.savez_compressed(PATH, **build())
    print(PATH, os.path.getsize(PATH), 'bytes')
