"""The committed ReBRAC fixture (tests/golden/rebrac/rebrac_small.npz, written by tests/golden/make_rebrac_golden.py): the CPU restatement
reproduces it, and the engine matches it (total_loss, a full and a critic-only update, a 6-update trajectory on the actor_freq = 2
schedule from the device dataset, sample_actions)."""
import json
import os

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import assert_info_close

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'rebrac', 'rebrac_small.npz')
KEYS = ('critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min', 'actor/total_loss', 'actor/actor_loss', 'actor/bc_loss',
        'actor/std', 'actor/mse', 'grad/max', 'grad/min', 'grad/norm')
CKEYS = KEYS[:4] + KEYS[9:]
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
    from tests.golden import make_rebrac_golden as M
    d, _ = _load()
    new = M.build()
    assert sorted(new) == sorted(d.files)
    for k in d.files:
        if k == 'meta':
            assert json.loads(str(new[k])) == json.loads(str(d[k]))
            continue
        np.testing.assert_allclose(np.asarray(new[k], dtype=np.float64), d[k].astype(np.float64), rtol=1e-9, atol=1e-12, err_msg=k)


@pytest.mark.gpu
def test_engine_matches_fixture():
    import fql_amd
    d, meta = _load()
    B = meta['B']
    cfg = fql_amd.rebrac.get_config()
    cfg.update(actor_hidden_dims=tuple(meta['hidden']), value_hidden_dims=tuple(meta['hidden']), batch_size=B,
               alpha_actor=meta['alpha_actor'], alpha_critic=meta['alpha_critic'])
    batch = {k: d[f'batch/{k}'] for k in BATCH + ('next_actions',)}
    a = fql_amd.ReBRACAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(_tree(d, 'params'))
    assert sorted(p for p, _ in a.leaves()) == sorted(meta['leaves'])

    loss, info = a.total_loss(batch, noise={'eps1': d['noise/eps1']})
    assert_info_close(info, dict(zip(KEYS, d['info_total_loss'])), keys=KEYS[:9])
    assert abs(loss - float(d['total_loss'])) <= 1e-5 * max(1.0, abs(float(d['total_loss'])))
    np.testing.assert_allclose(a.sample_actions(d['sample/observations'], noises=d['sample/noise'], temperature=0.5), d['sample/action'],
                               atol=2e-5)

    _, info = a.update(batch, noise={'eps1': d['noise/eps1']})
    assert_info_close(info.to_dict(), dict(zip(KEYS, d['info_update'])), rtol=5e-5, atol=5e-6, keys=KEYS)
    a.synchronize()
    mu = dict(O.tree_leaves_with_path(a.get_opt_state()['mu']))
    for p, g in O.tree_leaves_with_path(_tree(d, 'grads')):
        if p.startswith('modules_target_'):
            continue
        tol = 2e-5 * np.abs(g).max() + 1e-9
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
    _, info = a.update(batch, full_update=False, noise={'eps1': d['noise2/eps1']})
    assert tuple(info) == CKEYS
    assert_info_close(info.to_dict(), dict(zip(CKEYS, d['info_critic_update'])), rtol=5e-5, atol=5e-6, keys=CKEYS)
    a.synchronize()
    got = dict(O.tree_leaves_with_path(a.get_params()))
    for p, v in O.tree_leaves_with_path(_tree(d, 'new_params')):
        assert np.abs(got[p] - v).max() <= 4 * cfg['lr'] + 1e-6, p
        np.testing.assert_allclose(float(np.sum(got[p])), float(np.sum(v)), rtol=1e-3, atol=1e-3 * v.size ** 0.5 * cfg['lr'], err_msg=p)

    a.upload_dataset({k: d[f'dataset/{k}'] for k in BATCH})
    for s in range(meta['steps']):
        _, info = a.update_from_dataset(idxs=d['traj/idx'][s], noise={'eps1': d['traj/eps1'][s]}, want_info=True,
                                        full_update=s % 2 == 0)
        want = dict(zip(CKEYS, d['traj/info'][s]))
        for k in CKEYS:
            assert abs(float(info[k]) - want[k]) <= 1e-3 * max(1.0, abs(want[k])), (s, k, float(info[k]), want[k])
    a.synchronize()
    sums = [float(np.sum(v)) for _, v in O.tree_leaves_with_path(a.get_params())]
    np.testing.assert_allclose(sums, d['traj/leaf_sums'][-1], rtol=1e-3, atol=1e-3)
