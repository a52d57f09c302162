"""The committed SAC fixture (tests/golden/sac/sac_small.npz, written by tests/golden/make_sac_golden.py): the CPU restatement reproduces
it, and the engine matches it (total_loss, one update with its gradients, parameters and moments, a 6-update balanced trajectory from the
device dataset and replay ring, sample_actions)."""
import json
import os

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import assert_info_close

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'sac', 'sac_small.npz')
KEYS = ('critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min', 'actor/total_loss', 'actor/actor_loss', 'actor/alpha_loss',
        'actor/alpha', 'actor/entropy', 'actor/std', 'actor/q', 'grad/max', 'grad/min', 'grad/norm')
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
    from tests.golden import make_sac_golden as M
    d, _ = _load()
    new = M.build()
    assert sorted(new) == sorted(d.files)
    for k in d.files:
        if k == 'meta':
            assert json.loads(str(new[k])) == json.loads(str(d[k]))
            continue
        np.testing.assert_allclose(np.asarray(new[k], dtype=np.float64), d[k].astype(np.float64), rtol=1e-9, atol=1e-12, err_msg=k)


def test_fixture_holds_a_zero_d_leaf_and_the_clip():
    d, meta = _load()
    assert d['params/modules_alpha/log_value'].shape == () and 'modules_alpha/log_value' in meta['leaves']
    g = d['grads/modules_actor/log_std_net/bias']
    assert g[0] == 0.0 and g[2] == 0.0 and g[1] != 0.0   # columns past -5 and past 2 get no gradient


@pytest.mark.gpu
def test_engine_matches_fixture():
    import fql_amd
    d, meta = _load()
    B = meta['B']
    cfg = fql_amd.sac.get_config()
    cfg.update(actor_hidden_dims=tuple(meta['hidden']), value_hidden_dims=tuple(meta['hidden']), batch_size=B,
               backup_entropy=meta['backup_entropy'])
    batch = {k: d[f'batch/{k}'] for k in BATCH}
    noise = {k: d[f'noise/{k}'] for k in ('eps1', 'eps2')}
    a = fql_amd.SACAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(_tree(d, 'params'))
    assert sorted(p for p, _ in a.leaves()) == sorted(meta['leaves'])

    loss, info = a.total_loss(batch, noise=noise)
    assert_info_close(info, dict(zip(KEYS, d['info_total_loss'])), keys=KEYS[:11])
    assert abs(loss - float(d['total_loss'])) <= 1e-5 * max(1.0, abs(float(d['total_loss'])))
    np.testing.assert_allclose(a.sample_actions(d['sample/observations'], noises=d['sample/noise'], temperature=0.7), d['sample/action'],
                               atol=2e-5)

    _, info = a.update(batch, noise=noise)
    assert_info_close(info.to_dict(), dict(zip(KEYS, d['info_update'])), rtol=5e-5, atol=5e-6, keys=KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu = dict(O.tree_leaves_with_path(opt['mu'])), dict(O.tree_leaves_with_path(opt['nu']))
    for p, g in O.tree_leaves_with_path(_tree(d, 'grads')):
        if p.startswith('modules_target_'):
            continue
        tol = 2e-5 * np.abs(g).max() + 1e-9
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], d[f'new_nu/{p}'], rtol=1e-4, atol=1e-4 * np.abs(d[f'new_nu/{p}']).max() + 1e-20, err_msg=p)
    got = dict(O.tree_leaves_with_path(a.get_params()))
    for p, v in O.tree_leaves_with_path(_tree(d, 'new_params')):
        assert np.abs(got[p] - v).max() <= 2 * cfg['lr'] + 1e-6, p

    a.upload_dataset({k: d[f'dataset/{k}'] for k in BATCH})
    a.create_replay_buffer(4 * meta['ring'])
    for i in range(meta['ring']):
        a.add_transition({k: d[f'ring/{k}'][i] for k in BATCH}, replay=True)
    for s in range(meta['steps']):
        _, info = a.update_balanced(B, idxs=(d['traj/idx_dataset'][s], d['traj/idx_replay'][s]),
                                    noise={'eps1': d['traj/eps1'][s], 'eps2': d['traj/eps2'][s]}, want_info=True)
        want = dict(zip(KEYS, d['traj/info'][s]))
        for k in KEYS:
            assert abs(float(info[k]) - want[k]) <= 1e-3 * max(1.0, abs(want[k])), (s, k, float(info[k]), want[k])
    a.synchronize()
    sums = [float(np.sum(v)) for _, v in O.tree_leaves_with_path(a.get_params())]
    np.testing.assert_allclose(sums, d['traj/leaf_sums'][-1], rtol=1e-3, atol=1e-3)
