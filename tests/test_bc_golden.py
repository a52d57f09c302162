"""Replays tests/golden/bc/bc_small.npz (tests/golden/make_bc_golden.py) on both BC oracles."""
import os

import numpy as np

import bc_oracle as BO
import bc_oracle_torch as BT

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bc', 'bc_small.npz')
OD, AD, S = 11, 3, 4


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
    cfg = BO.get_config()
    cfg.update(hidden_dims=(32, 32), denoise_steps=S, batch_size=16)
    batch = {'observations': z['in/observations'], 'actions': z['in/actions']}
    noise = {'x0': z['in/x0'], 't': z['in/t']}
    return z, tree, cfg, batch, noise


def test_fixture_is_small():
    sac = os.path.join(os.path.dirname(PATH), '..', 'sac', 'sac_small.npz')
    assert os.path.getsize(PATH) <= os.path.getsize(sac)


def test_numpy_oracle_replays_the_fixture():
    z, tree, cfg, batch, noise = _load()
    ref = BO.OracleBC(tree, cfg, OD, AD, np.float64)
    np.testing.assert_allclose(ref.sample_actions(batch['observations'][:5], z['in/sample_noise']), z['out/actions'], rtol=0, atol=1e-12)
    _, _, g = ref.grads(batch, noise)
    from oracle.fql_oracle import tree_leaves_with_path
    for p, v in tree_leaves_with_path(g):
        np.testing.assert_allclose(v, z['grad/' + p], rtol=1e-12, atol=1e-15)
    _, info = ref.update(batch, noise)
    np.testing.assert_allclose([info[k] for k in BO.INFO_KEYS], z['out/info'], rtol=1e-12)
    for p, v in tree_leaves_with_path(ref.params):
        np.testing.assert_allclose(v, z['new/' + p], rtol=1e-12, atol=1e-15)


def test_torch_oracle_replays_the_fixture():
    z, tree, cfg, batch, noise = _load()
    ref = BT.TorchBC(tree, cfg)
    np.testing.assert_allclose(ref.sample_actions(batch['observations'][:5], z['in/sample_noise']), z['out/actions'], rtol=0, atol=1e-10)
    loss, g = ref.update(batch, noise)
    assert abs(loss - z['out/info'][0]) <= 1e-10 * max(1.0, abs(loss))
    for p, v in BT.leaves(g).items():
        np.testing.assert_allclose(v, z['grad/' + p], rtol=1e-8, atol=1e-12)
    for p, v in BT.leaves(ref.params).items():
        np.testing.assert_allclose(v, z['new/' + p], rtol=1e-8, atol=1e-12)
