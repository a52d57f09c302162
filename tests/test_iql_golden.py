"""The committed IQL fixture (tests/golden/iql/iql_small.npz, written by tests/golden/make_iql_golden.py): the CPU restatement reproduces
it, and the engine matches it for both actor losses (total_loss, one update with its gradients and - for ddpgbc - parameters, a 6-update
trajectory from the device dataset, sample_actions)."""
import json
import os

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iql_oracle as IO
from tests.util import assert_info_close

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'iql', 'iql_small.npz')
BATCH = ('observations', 'actions', 'rewards', 'masks', 'next_observations')


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
    from tests.golden import make_iql_golden as M
    d, _ = _load()
    new = M.build()
    assert sorted(new) == sorted(d.files)
    for k in d.files:
        if k == 'meta':
            assert json.loads(str(new[k])) == json.loads(str(d[k]))
            continue
        np.testing.assert_allclose(np.asarray(new[k], dtype=np.float64), d[k].astype(np.float64), rtol=1e-9, atol=1e-12, err_msg=k)


def test_fixture_holds_the_log_stds_leaf_and_its_clip():
    d, meta = _load()
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(HERE, 'golden', 'sac', 'sac_small.npz'))
    assert 'modules_actor/log_stds' in meta['leaves'] and d['params/modules_actor/log_stds'].shape == (meta['act_dim'],)
    assert d['params/modules_actor/log_stds'][2] < IO.LOG_STD_MIN
    for al in ('awr', 'ddpgbc'):
        g = d[f'{al}/grads/modules_actor/log_stds']
        assert g[2] == 0.0 and g[0] != 0.0 and g[1] != 0.0   # the column past -5 gets no gradient
        assert not any(d[k].any() for k in d.files if k.startswith(f'{al}/grads/modules_target_'))
        assert len(d[f'{al}/info_update']) == len(IO.INFO_KEYS[al])


@pytest.mark.gpu
@pytest.mark.parametrize('actor_loss', ['awr', 'ddpgbc'])
def test_engine_matches_fixture(actor_loss):
    import fql_amd
    d, meta = _load()
    B, keys = meta['B'], IO.INFO_KEYS[actor_loss]
    cfg = fql_amd.iql.get_config()
    cfg.update(actor_hidden_dims=tuple(meta['hidden']), value_hidden_dims=tuple(meta['hidden']), batch_size=B, actor_loss=actor_loss,
               const_std=meta['const_std'], actor_layer_norm=meta['actor_layer_norm'])
    batch = {k: d[f'batch/{k}'] for k in BATCH}
    noise = {'eps': d['noise/eps']}
    a = fql_amd.IQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(_tree(d, 'params'))
    assert sorted(p for p, _ in a.leaves()) == sorted(meta['leaves'])

    loss, info = a.total_loss(batch, noise=noise)
    assert_info_close(info, dict(zip(keys, d[f'{actor_loss}/info_total_loss'])), rtol=5e-5, atol=5e-6, keys=keys[:-3])
    want_loss = float(d[f'{actor_loss}/total_loss'])
    assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    np.testing.assert_allclose(a.sample_actions(d['sample/observations'], noises=d['sample/noise'], temperature=0.7), d['sample/action'],
                               atol=2e-5)

    _, info = a.update(batch, noise=noise)
    assert_info_close(info.to_dict(), dict(zip(keys, d[f'{actor_loss}/info_update'])), rtol=5e-5, atol=5e-6, keys=keys)
    a.synchronize()
    mu = dict(O.tree_leaves_with_path(a.get_opt_state()['mu']))
    for p, g in O.tree_leaves_with_path(_tree(d, f'{actor_loss}/grads')):
        if p.startswith('modules_target_'):
            continue
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=5e-5 * np.abs(g).max() + 1e-9, err_msg=f'grad {p}')
    if actor_loss == 'ddpgbc':
        got = dict(O.tree_leaves_with_path(a.get_params()))
        for p, v in O.tree_leaves_with_path(_tree(d, 'ddpgbc/new_params')):
            assert np.abs(got[p] - v).max() <= 2 * cfg['lr'] + 1e-6, p

    a.upload_dataset({k: d[f'dataset/{k}'] for k in BATCH})
    for s in range(meta['steps']):
        _, info = a.update_from_dataset(idxs=d['traj/idx'][s], noise={'eps': d['traj/eps'][s]}, want_info=True)
        want = dict(zip(keys, d[f'{actor_loss}/traj_info'][s]))
        for k in keys:
            assert abs(float(info[k]) - want[k]) <= 1e-3 * max(1.0, abs(want[k])), (s, k, float(info[k]), want[k])
    a.synchronize()
    sums = [float(np.sum(v)) for _, v in O.tree_leaves_with_path(a.get_params())]
    np.testing.assert_allclose(sums, d[f'{actor_loss}/traj_leaf_sums'][-1], rtol=1e-3, atol=1e-3)
