"""The committed IQL-diffusion fixture (tests/golden/iqld/iqld_small.npz, written by tests/golden/make_iqld_golden.py): the CPU
restatement reproduces it, and the engine matches it for the three optimal_var variants (total_loss, one update with its infos, per-row
arrays and gradients, sample_actions at cfg 0, 1 and 3)."""
import json
import os

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iqld_cases as K
from fql_amd.iql_diffusion import info_keys, IQLD_ROW_KEYS, OPTIMAL_VARS

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'iqld', 'iqld_small.npz')


def _load():
    d = np.load(PATH)
    return d, json.loads(str(d['meta']))


def _tree(d, prefix):
    out = {}
    for k in d.files:
        if k.startswith(prefix + '/'):
            node = out
            parts = k[len(prefix) + 1:].split('/')
            for p in parts[:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = d[k]
    return out


def test_restatement_reproduces_fixture():
    from tests.golden import make_iqld_golden as M
    d, _ = _load()
    new = M.build()
    assert sorted(new) == sorted(d.files)
    for k in d.files:
        if k == 'meta':
            assert json.loads(str(new[k])) == json.loads(str(d[k]))
            continue
        np.testing.assert_allclose(np.asarray(new[k], dtype=np.float64), d[k].astype(np.float64), rtol=1e-9, atol=1e-12, err_msg=k)


def test_fixture_holds_both_embedding_rows_and_both_sides_of_the_weights():
    d, meta = _load()
    assert os.path.getsize(PATH) <= 1 << 20
    assert 'actor/Embed_0/embedding' in meta['leaves'] and d['params/actor/Embed_0/embedding'].shape == (2, 32)
    for ov in OPTIMAL_VARS:
        g = d[f'{ov}/grads/actor/Embed_0/embedding']
        assert g[0].any() and g[1].any()
        w = d[f'{ov}/rows/loss_weights']
        assert (w > 0).any() and (w == 0).any()
        assert len(d[f'{ov}/info_update']) == 21 and len(d[f'{ov}/info_total_loss']) == 18
    assert (d['binary_awr_loss/rows/loss_weights'] == 100.0).any()
    assert any((np.abs(d[f'sample/action_cfg{c:g}']) == 1).any() for c in meta['cfgs'])


@pytest.mark.gpu
@pytest.mark.parametrize('ov', OPTIMAL_VARS)
def test_engine_matches_fixture(ov):
    import fql_amd
    d, meta = _load()
    c = meta['case']
    cfg = K.config(c)
    cfg.update(optimal_var=ov, awr_temperature=meta['awr_temperature'])
    batch = {k[len('batch/'):]: d[k] for k in d.files if k.startswith('batch/')}
    noise = {k[len('noise/'):]: d[k] for k in d.files if k.startswith('noise/')}
    a = fql_amd.agents['iql_diffusion'].create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(_tree(d, 'params'))
    assert [p for p, _ in a.leaves()] == meta['leaves']
    scal = [k for k in info_keys(True, True, grads=False) if k not in IQLD_ROW_KEYS]
    loss, info = a.total_loss(batch, noise=noise)
    want_loss = float(d[f'{ov}/total_loss'])
    assert abs(loss - want_loss) <= 5e-6 + 5e-5 * abs(want_loss)
    for k, w in zip(scal, d[f'{ov}/info_total_loss']):
        assert abs(info[k] - w) <= 5e-6 + 5e-5 * abs(w), (k, info[k], w)
    for cs in meta['cfgs']:
        np.testing.assert_allclose(a.sample_actions(d['sample/observations'], noises=d['sample/noise'], cfg=cs), d[f'sample/action_cfg{cs:g}'],
                                   rtol=0, atol=2e-5)
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    for k, w in zip([k for k in info_keys(True, True) if k not in IQLD_ROW_KEYS], d[f'{ov}/info_update']):
        assert abs(info[k] - w) <= 5e-6 + 5e-5 * abs(w), (k, info[k], w)
    for k in IQLD_ROW_KEYS:
        np.testing.assert_allclose(info[k], d[f'{ov}/rows/{k}'], rtol=5e-5, atol=5e-6, err_msg=k)
    a.synchronize()
    mu = dict(O.tree_leaves_with_path(a.get_opt_state()['mu']))
    for p, g in O.tree_leaves_with_path(_tree(d, f'{ov}/grads')):
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=2e-5 * np.abs(g).max() + 1e-9, err_msg=f'grad {p}')
