"""CPU: the IFQL restatement (tests/ifql_oracle.py) against finite differences and the reference's quirks; the IFQL config, registry,
C-ABI defaults and the Python-side refusals.  Nothing here launches GPU work."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import ifql_oracle as IO

OD, AD, B, H = 5, 3, 8, (8, 8)


# the configurations of the GPU matrix (tests/test_gpu_ifql.py SHAPE_CASES) beside the default one
CONFIGS = {
    'no_layer_norm': dict(layer_norm=False),
    'actor_ln': dict(actor_layer_norm=True),
    'ragged_depths': dict(actor_hidden_dims=(9, 7), value_hidden_dims=(6, 10, 8)),
    'expectile': dict(expectile=0.7, discount=0.995),
}


def _setup(seed=0, **kw):
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=H, value_hidden_dims=H)
    cfg.update(kw)
    params = IO.init_params(seed, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(seed + 1)
    for _, leaf in O.tree_leaves_with_path(params):
        leaf += 0.1 * rng.standard_normal(leaf.shape)   # every leaf matters; target != critic
    batch = {'observations': rng.standard_normal((B, OD)), 'actions': rng.uniform(-1, 1, (B, AD)), 'rewards': rng.standard_normal(B),
             'masks': (rng.random(B) > 0.2).astype(np.float64), 'next_observations': rng.standard_normal((B, OD))}
    noise = {'x0': rng.standard_normal((B, AD)), 't': rng.random(B)}
    return cfg, params, batch, noise


FD_PATHS = {
    None: ['modules_value/value_net/Dense_0/kernel', 'modules_value/value_net/LayerNorm_1/scale', 'modules_critic/value_net/Dense_1/kernel',
           'modules_critic/value_net/Dense_2/bias', 'modules_actor_flow/mlp/Dense_0/kernel', 'modules_actor_flow/mlp/Dense_2/bias'],
    'no_layer_norm': ['modules_value/value_net/Dense_1/kernel', 'modules_value/value_net/Dense_2/bias',
                      'modules_critic/value_net/Dense_0/kernel', 'modules_critic/value_net/Dense_1/bias'],
    'actor_ln': ['modules_actor_flow/mlp/LayerNorm_0/scale', 'modules_actor_flow/mlp/LayerNorm_1/bias', 'modules_actor_flow/mlp/Dense_1/kernel',
                 'modules_actor_flow/mlp/Dense_2/kernel'],
    'ragged_depths': ['modules_value/value_net/Dense_3/kernel', 'modules_value/value_net/LayerNorm_2/scale',
                      'modules_critic/value_net/Dense_2/kernel', 'modules_critic/value_net/LayerNorm_0/bias',
                      'modules_actor_flow/mlp/Dense_1/kernel', 'modules_actor_flow/mlp/Dense_2/bias'],
    'expectile': ['modules_value/value_net/Dense_0/kernel', 'modules_value/value_net/Dense_2/bias', 'modules_value/value_net/LayerNorm_0/scale',
                  'modules_critic/value_net/Dense_2/kernel'],
}


@pytest.mark.parametrize('conf,path', [pytest.param(c, p, id=p if c is None else f'{c}-{p}') for c, ps in FD_PATHS.items() for p in ps])
def test_gradients_match_finite_differences(conf, path):
    """jax.grad of total_loss: value(next_obs) and the target critic are stored parameters (no gradient flows through them)."""
    cfg, params, batch, noise = _setup(**CONFIGS.get(conf, {}))
    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    ref.frozen = O.tree_map(np.copy, ref.params)
    _, _, g = ref.grads(batch, noise)
    leaf = dict(O.tree_leaves_with_path(ref.params))[path]
    want = dict(O.tree_leaves_with_path(g))[path]
    rng = np.random.default_rng(3)
    for flat in rng.choice(leaf.size, size=min(4, leaf.size), replace=False):
        i = np.unravel_index(flat, leaf.shape)
        old = leaf[i]
        leaf[i] = old + 1e-6
        lp = ref.total_loss(batch, noise)[0]
        leaf[i] = old - 1e-6
        lm = ref.total_loss(batch, noise)[0]
        leaf[i] = old
        assert abs((lp - lm) / 2e-6 - want[i]) <= 1e-6 * max(1.0, abs(want[i])), (path, i)
    for p, gg in O.tree_leaves_with_path(g):
        if p.startswith('modules_target_critic/'):
            assert not gg.any()


def test_value_loss_expectile_weights_and_gradient():
    """w = expectile where q - v >= 0, else 1 - expectile (agents/ifql.py:28-29).  At q - v == 0 exactly the loss term and its gradient are
    0 whatever w is, so the `>=` tie rule is not observable; the row shifted to a zero advantage only checks that it contributes nothing."""
    cfg, params, batch, noise = _setup()
    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    obs, act = batch['observations'], batch['actions']
    q = ref._critic('modules_target_critic', obs, act).min(axis=0)
    v = ref._value(obs)
    # shift the value head's bias so that v == q on row 0: that row's advantage is exactly 0, the others keep their sign
    d = q - v
    _, info = ref.total_loss(batch, noise)[0], ref.total_loss(batch, noise)[1]
    w = np.where(d >= 0, 0.9, 0.1)
    assert abs(info['value/value_loss'] - np.mean(w * d * d)) <= 1e-12
    ref.params['modules_value']['value_net']['Dense_2']['bias'] += d[0]
    v2 = ref._value(obs)
    d2 = q - v2
    assert abs(d2[0]) < 1e-12
    dv = (-2.0 / B) * np.where(d2 >= 0, 0.9, 0.1) * d2
    _, _, g = ref.grads(batch, noise)
    np.testing.assert_allclose(g['modules_value']['value_net']['Dense_2']['bias'], dv.sum(keepdims=True), atol=1e-12)
    assert info['value/v_mean'] == pytest.approx(v.mean()) and info['value/v_max'] == pytest.approx(v.max())


def test_critic_loss_sums_members_and_reports_statistics_of_the_target():
    cfg, params, batch, noise = _setup()
    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    _, info = ref.total_loss(batch, noise)
    y = batch['rewards'] + 0.99 * batch['masks'] * ref._value(batch['next_observations'])
    q = ref._critic('modules_critic', batch['observations'], batch['actions'])
    assert info['critic/critic_loss'] == pytest.approx(((q[0] - y) ** 2 + (q[1] - y) ** 2).sum() / B, rel=1e-12)
    assert (info['critic/q_mean'], info['critic/q_max'], info['critic/q_min']) == pytest.approx((y.mean(), y.max(), y.min()), rel=1e-12)


def test_update_info_order_totals_and_polyak_from_pre_step_critic():
    cfg, params, batch, noise = _setup()
    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    loss, info0 = ref.total_loss(batch, noise)
    pre = O.tree_map(np.copy, ref.params)
    _, info = ref.update(batch, noise)
    assert tuple(info) == IO.INFO_KEYS and len(info) == 12
    assert loss == pytest.approx(info0['value/value_loss'] + info0['critic/critic_loss'] + info0['actor/actor_loss'])
    assert info['grad/max'] >= 0 >= info['grad/min']   # target leaves contribute zero gradients
    for (p, new), (_, c_old), (_, t_old) in zip(O.tree_leaves_with_path(ref.params['modules_target_critic']),
                                                O.tree_leaves_with_path(pre['modules_critic']),
                                                O.tree_leaves_with_path(pre['modules_target_critic'])):
        np.testing.assert_allclose(new, 0.005 * c_old + 0.995 * t_old, rtol=1e-12, err_msg=p)
    assert ref.count == 1 and ref.step == 2


def test_leaf_layout_value_unstacked_critic_stacked():
    cfg = IO.get_config()
    p = dict(O.tree_leaves_with_path(IO.init_params(0, 29, 8, cfg)))
    assert p['modules_value/value_net/Dense_0/kernel'].shape == (29, 512)
    assert p['modules_value/value_net/Dense_4/kernel'].shape == (512, 1)
    assert p['modules_critic/value_net/Dense_0/kernel'].shape == (2, 37, 512)
    assert p['modules_actor_flow/mlp/Dense_0/kernel'].shape == (38, 512)
    assert not any(k.startswith('modules_actor_flow/mlp/LayerNorm') for k in p)
    assert 'modules_value/value_net/LayerNorm_3/scale' in p


@pytest.mark.parametrize('dtype,rtol,conf', [pytest.param('float64', 1e-10, None, id='float64-1e-10'),
                                              pytest.param('float32', 1e-6, None, id='float32-1e-06')] +
                         [pytest.param('float64', 1e-10, c, id=f'float64-1e-10-{c}') for c in CONFIGS])
def test_numpy_and_torch_restatements_agree(dtype, rtol, conf):
    """tests/ifql_oracle.py (hand-derived backward) == tests/ifql_oracle_torch.py (autograd): infos, gradients, two updates."""
    import torch
    from tests import ifql_oracle_torch as IT
    cfg, params, batch, noise = _setup(4, **CONFIGS.get(conf, {}))
    npd, tdt = np.dtype(dtype), getattr(torch, dtype)
    params = O.tree_map(lambda a: a.astype(npd), params)
    batch = {k: v.astype(npd) for k, v in batch.items()}
    noise = {k: v.astype(npd) for k, v in noise.items()}
    ref, tor = IO.OracleIFQL(params, cfg, OD, AD, npd), IT.TorchIFQL(params, cfg, tdt)

    def close(a, b, scale=1.0):
        assert abs(a - b) <= rtol * max(abs(b), scale), (a, b)

    l1, i1 = ref.total_loss(batch, noise)
    l2, i2 = tor.total_loss(batch, noise)
    close(float(l1), float(l2))
    for k in IO.INFO_KEYS[:9]:
        close(float(i1[k]), float(i2[k]))
    _, _, g1 = ref.grads(batch, noise)
    _, _, g2 = tor.grads(batch, noise)
    g2 = dict(O.tree_leaves_with_path(O.tree_map(lambda t: t.numpy(), g2)))
    for p, g in O.tree_leaves_with_path(g1):
        np.testing.assert_allclose(g, g2[p], rtol=0, atol=10 * rtol * max(np.abs(g2[p]).max(), 1e-3), err_msg=p)
    for _ in range(2):
        _, u1 = ref.update(batch, noise)
        _, u2 = tor.update(batch, noise)
        for k in IO.INFO_KEYS:
            close(u1[k], u2[k], scale=1e-3 if k.startswith('grad/m') else 1.0)
    p2 = dict(O.tree_leaves_with_path(O.tree_map(lambda t: t.numpy(), tor.params)))
    for p, v in O.tree_leaves_with_path(ref.params):
        np.testing.assert_allclose(v, p2[p], rtol=0, atol=100 * rtol * max(1.0, np.abs(v).max()), err_msg=p)
    z = np.random.default_rng(5).standard_normal((6, AD)).astype(npd)
    a1, q1 = ref.sample_actions(batch['observations'][0], z)
    a2, q2 = tor.sample_actions(batch['observations'][0], z)
    np.testing.assert_allclose(q1, q2.numpy(), rtol=0, atol=10 * rtol * max(1.0, np.abs(q1).max()))
    np.testing.assert_allclose(a1, a2.numpy(), rtol=0, atol=10 * rtol)


def test_sample_actions_restatement_takes_first_argmax():
    cfg, params, batch, _ = _setup()
    ref = IO.OracleIFQL(params, cfg, OD, AD, np.float64)
    z = np.random.default_rng(2).standard_normal((4, AD))
    z = np.concatenate([z, z])   # every action twice: ties, the first index wins
    a, q = ref.sample_actions(batch['observations'][0], z)
    assert int(np.argmax(q)) < 4
    acts = ref.compute_flow_actions(np.repeat(batch['observations'][:1], 8, axis=0), z)
    np.testing.assert_array_equal(a, acts[int(np.argmax(q))])
    assert np.abs(acts).max() <= 1.0


def test_config_defaults_registry_and_cabi_defaults():
    import __graft_entry__ as g
    g.build()
    import fql_amd
    from fql_amd import _cabi
    cfg = fql_amd.ifql.get_config()
    want = IO.get_config()
    for k, v in want.items():
        assert cfg[k] == v, k
    assert fql_amd.agents['ifql'] is fql_amd.IFQLAgent and fql_amd.agents['fql'] is fql_amd.FQLAgent
    assert fql_amd.IFQL_INFO_KEYS == IO.INFO_KEYS
    lib = _cabi.load()
    ic = _cabi.FqlIfqlConfig()
    lib.fql_ifql_default_config(C.byref(ic))
    assert abs(ic.expectile - 0.9) < 1e-7 and ic.num_samples == 32 and list(ic.reserved) == [0] * 6
    assert C.sizeof(_cabi.FqlIfqlConfig) == 32
    assert lib.fql_num_info(None) == _cabi.FQL_E_INVALID and lib.fql_handle_info_name(None, 0) is None


@pytest.mark.parametrize('kw,err', [({'encoder': 'impala_small'}, 'encoder'), ({'precision': 'bf16x3'}, 'fp32'), ({'rng': 'jax'}, 'rng')])
def test_python_refusals_come_before_the_library(kw, err):
    import fql_amd
    cfg = fql_amd.ifql.get_config()
    cfg.update(kw)
    with pytest.raises(NotImplementedError, match=err):
        fql_amd.IFQLAgent.create(0, np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), cfg)
