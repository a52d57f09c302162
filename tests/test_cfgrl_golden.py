"""Replays tests/golden/cfgrl/cfgrl_small.npz (tests/golden/make_cfgrl_golden.py) on both CFGRL oracles and on the goal rule."""
import os

import numpy as np

import cfgrl_oracle as CO
import cfgrl_oracle_torch as CT
from oracle.fql_oracle import tree_leaves_with_path
from tests.golden import make_cfgrl_golden as M

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cfgrl', 'cfgrl_small.npz')
EMB = 'modules_unc_embed/Embed_0/embedding'


def _load():
    z = np.load(PATH)
    tree = {}
    for k in z.files:
        if not k.startswith('param/'):
            continue
        node, ks = tree, k[len('param/'):].split('/')
        for s in ks[:-1]:
            node = node.setdefault(s, {})
        node[ks[-1]] = z[k]
    batch = {k: z['in/' + k] for k in ('observations', 'actions', 'actor_goals')}
    noise = {'x0': z['in/x0'], 't': z['in/t']}
    return z, tree, M.config(), batch, noise, z['in/do_cfg']


def test_fixture_is_small_and_holds_the_masked_gradient():
    z = np.load(PATH)
    assert os.path.getsize(PATH) <= 64 << 10
    assert z['param/' + EMB].shape == (1, M.GD) and z['grad/' + EMB].shape == (1, M.GD) and z['grad/' + EMB].all()
    assert z['in/do_cfg'].sum() == 3 and z['in/do_cfg'][0] and z['in/do_cfg'][-1]
    assert any((np.abs(z[f'out/actions_cfg{c:g}']) == 1).any() for c in M.CFGS)


def test_maker_reproduces_the_fixture():
    z, new = np.load(PATH), M.build()
    assert sorted(new) == sorted(z.files)
    for k in z.files:
        np.testing.assert_allclose(np.asarray(new[k], np.float64), z[k].astype(np.float64), rtol=1e-9, atol=1e-12, err_msg=k)


def test_numpy_oracle_replays_the_fixture():
    z, tree, cfg, batch, noise, mask = _load()
    ref = CO.OracleCFGRL(tree, cfg, M.OD, M.AD, M.GD, np.float64)
    for c in M.CFGS:
        got = ref.sample_actions(batch['observations'][:5], batch['actor_goals'][:5], z['in/sample_noise'], c)
        np.testing.assert_allclose(got, z[f'out/actions_cfg{c:g}'], rtol=0, atol=1e-12)
    _, _, g = ref.grads(batch, noise, mask)
    for p, v in tree_leaves_with_path(g):
        np.testing.assert_allclose(v, z['grad/' + p], rtol=1e-12, atol=1e-15)
    _, info = ref.update(batch, noise, mask)
    np.testing.assert_allclose([info[k] for k in CO.INFO_KEYS], z['out/info'], rtol=1e-12)
    for p, v in tree_leaves_with_path(ref.params):
        np.testing.assert_allclose(v, z['new/' + p], rtol=1e-12, atol=1e-15)


def test_torch_oracle_replays_the_fixture():
    z, tree, cfg, batch, noise, mask = _load()
    ref = CT.TorchCFGRL(tree, cfg)
    for c in M.CFGS:
        got = ref.sample_actions(batch['observations'][:5], batch['actor_goals'][:5], z['in/sample_noise'], c)
        np.testing.assert_allclose(got, z[f'out/actions_cfg{c:g}'], rtol=0, atol=1e-10)
    loss, g = ref.update(batch, noise, mask)
    assert abs(loss - z['out/info'][0]) <= 1e-10 * max(1.0, abs(loss))
    for p, v in CT.leaves(g).items():
        np.testing.assert_allclose(v, z['grad/' + p], rtol=1e-8, atol=1e-12)
    for p, v in CT.leaves(ref.params).items():
        np.testing.assert_allclose(v, z['new/' + p], rtol=1e-8, atol=1e-12)


def test_goal_rule_replays_the_fixture():
    z = np.load(PATH)
    draws = {k: z['goal/draw_' + k] for k in ('random', 'dist', 'traj', 'cur')}
    final = CO.final_indices(z['goal/terminals'])
    for i, mix in enumerate(M.MIXES):
        g = CO.sample_goals(z['goal/idx'], z['goal/terminals'], draws, *mix)
        np.testing.assert_array_equal(g, z[f'goal/mix{i}'])
    traj = z['goal/mix1']
    idx = z['goal/idx']
    assert (traj >= np.minimum(idx + 1, final[idx])).all() and (traj <= final[idx]).all()
    np.testing.assert_array_equal(z['goal/mix0'], idx)
