"""Writes tests/golden/iqld/iqld_small.npz: a small IQL-diffusion problem and what the fp64 restatement (tests/iqld_oracle.py) computes
on it, for the three optimal_var variants: total_loss with its infos, one full update (infos, per-row arrays, every leaf's gradient), and
sample_actions at cfg 0, 1 and 3.  The problem is tests/iqld_cases.py's, so every row keeps 1e-3 from the points where the weights branch.

    python -m tests.golden.make_iqld_golden
"""
import json
import os

import numpy as np

from oracle import fql_oracle as O
from tests import iqld_cases as K
from tests import iqld_oracle as DO
from fql_amd.iql_diffusion import info_keys, IQLD_ROW_KEYS, OPTIMAL_VARS

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'iqld', 'iqld_small.npz')
CASE = K.case(od=11, ad=3, H=32, nh=2, B=32, S=4, seed=90)
CFGS = (0.0, 1.0, 3.0)


def build():
    out = {}
    cfg0, params, batch, noise, _ = K.build(CASE)
    for p, v in O.tree_leaves_with_path(params):
        out[f'params/{p}'] = v
    for k, v in batch.items():
        out[f'batch/{k}'] = v
    for k, v in noise.items():
        out[f'noise/{k}'] = v
    rng = np.random.default_rng(91)
    out['sample/observations'] = rng.standard_normal((5, CASE['od'])).astype(np.float32)
    out['sample/noise'] = rng.standard_normal((5, CASE['ad'])).astype(np.float32)
    for ov in OPTIMAL_VARS:
        cfg = dict(cfg0, optimal_var=ov)
        ref = DO.OracleIQLD(params, cfg, CASE['od'], CASE['ad'], np.float64)
        K.check_margins(ref, batch, ov)
        loss, info = ref.total_loss(batch, noise)
        out[f'{ov}/total_loss'] = np.float64(loss)
        out[f'{ov}/info_total_loss'] = np.array([info[k] for k in info_keys(True, True, grads=False) if k not in IQLD_ROW_KEYS], np.float64)
        if ov == OPTIMAL_VARS[0]:
            for c in CFGS:
                out[f'sample/action_cfg{c:g}'] = ref.sample_actions(out['sample/observations'], out['sample/noise'], c)
        g, _ = ref.grads(batch, noise)
        for net in g:
            for p, v in O.tree_leaves_with_path(g[net]):
                out[f'{ov}/grads/{net}/{p}'] = v
        info = ref.update(batch, noise)
        out[f'{ov}/info_update'] = np.array([info[k] for k in info_keys(True, True) if k not in IQLD_ROW_KEYS], np.float64)
        for k in IQLD_ROW_KEYS:
            out[f'{ov}/rows/{k}'] = np.asarray(info[k], np.float64)
    out['meta'] = np.array(json.dumps(dict(case=CASE, awr_temperature=cfg0['awr_temperature'], cfgs=list(CFGS),
                                           leaves=[p for p, _ in O.tree_leaves_with_path(params)])))
    return out


if __name__ == '__main__':
    np.savez_compressed(PATH, **build())
    print(PATH, os.path.getsize(PATH), 'bytes')
