"""The committed IFQL fixture (tests/golden/ifql/ifql_small.npz, written by tests/golden/make_ifql_golden.py): the CPU restatement reproduces
it, and the engine matches it (one update, total_loss, a 5-update trajectory, best-of-N sampling)."""
import json
import os

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import assert_info_close

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'ifql', 'ifql_small.npz')
KEYS = ('value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min', 'critic/critic_loss', 'critic/q_mean', 'critic/q_max',
        'critic/q_min', 'actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm')


def _load():
    d = np.load(PATH)
    meta = json.loads(str(d['meta']))
    return d, meta


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
    from tests.golden import make_ifql_golden as M
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
    od, ad, B = meta['obs_dim'], meta['act_dim'], meta['B']
    cfg = fql_amd.ifql.get_config()
    cfg.update(actor_hidden_dims=tuple(meta['hidden']), value_hidden_dims=tuple(meta['hidden']), batch_size=B,
               num_samples=meta['num_samples'])
    batch = {k: d[f'batch/{k}'] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')}
    noise = {'x0': d['noise/x0'], 't': d['noise/t']}
    a = fql_amd.IFQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(_tree(d, 'params'))
    assert sorted(p for p, _ in a.leaves()) == sorted(meta['leaves'])

    loss, info = a.total_loss(batch, noise=noise)
    assert_info_close(info, dict(zip(KEYS, d['info_total_loss'])), keys=KEYS[:9])
    assert abs(loss - float(d['total_loss'])) <= 1e-5 * max(1.0, abs(float(d['total_loss'])))

    scores = np.sort(d['sample/scores'])
    assert scores[-1] - scores[-2] > 1e-3 * max(1.0, abs(scores[-1]))   # a clear winner: the engine must pick the same sample
    np.testing.assert_allclose(a.sample_actions(batch['observations'][0], noises=d['sample/noise']), d['sample/action'], atol=2e-5)

    _, info = a.update(batch, noise=noise)
    assert_info_close(info.to_dict(), dict(zip(KEYS, d['info_update'])), rtol=5e-5, atol=5e-6, keys=KEYS)
    a.synchronize()
    got = dict(O.tree_leaves_with_path(a.get_params()))
    mu = dict(O.tree_leaves_with_path(a.get_opt_state()['mu']))
    for p, g in O.tree_leaves_with_path(_tree(d, 'grads')):
        tol = 2e-5 * np.abs(g).max() + 1e-9
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        dlt = np.abs(got[p] - d[f'new_params/{p}'])
        assert dlt[np.abs(g) > 50 * tol].max(initial=0) <= 2e-6, p
        assert dlt.max() <= 2 * cfg['lr'] + 1e-6, p

    a.upload_dataset({k: d[f'dataset/{k}'] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')})
    for s in range(meta['steps']):
        _, info = a.update_from_dataset(idxs=d['traj/idx'][s], noise={'x0': d['traj/x0'][s], 't': d['traj/t'][s]}, want_info=True)
        want = dict(zip(KEYS, d['traj/info'][s]))
        for k in KEYS:
            assert abs(float(info[k]) - want[k]) <= 1e-3 * max(1.0, abs(want[k])), (s, k, float(info[k]), want[k])
    a.synchronize()
    sums = [float(np.sum(v)) for _, v in O.tree_leaves_with_path(a.get_params())]
    np.testing.assert_allclose(sums, d['traj/leaf_sums'][-1], rtol=1e-3, atol=1e-3)
