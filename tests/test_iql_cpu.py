"""CPU: the IQL restatements (tests/iql_oracle.py against finite differences and the torch-autograd restatement), known answers of the
expectile weight, AWR's exp cap and the Gaussian log-probability, the log_stds clip's gradient, the info layout, the IQL config, registry
and C-ABI defaults, and the Python-side refusals.  Nothing here launches GPU compute."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iql_oracle as IO

OD, AD, B, SEED = 5, 3, 8, 11
CASES = [pytest.param(al, cs, id=f'{al}-const_std{int(cs)}') for al in ('awr', 'ddpgbc') for cs in (True, False)]


def _setup(**kw):
    cfg = IO.get_config()
    cfg.update(actor_hidden_dims=(16, 16), value_hidden_dims=(16, 16), batch_size=B)
    cfg.update(kw)
    params = IO.randomize(IO.init_params(SEED, OD, AD, cfg, np.float64), SEED + 1)
    ds = O.make_synthetic_dataset(64, OD, AD, seed=SEED)
    batch = O.sample_batch(ds, np.random.default_rng(SEED).integers(0, 64, size=B))
    return cfg, params, batch, IO.make_noise(B, AD, SEED + 2)


@pytest.mark.parametrize('actor_loss,const_std', CASES)
def test_gradients_match_finite_differences_on_every_leaf(actor_loss, const_std):
    """jax.grad of total_loss: the target critic, value(next_obs), the AWR weight's critic and value and the ddpgbc loss's critic are
    stored parameters (held in `frozen`); the normaliser mean|q| is a stop_gradient (held fixed).  The fixture stays 1e-4 away from every
    kink, so central differences of step 1e-6 cross none."""
    cfg, params, batch, noise = _setup(actor_loss=actor_loss, const_std=const_std, actor_layer_norm=not const_std)
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    assert min(ref.kink_margins(batch, noise).values()) >= 1e-4
    ref.frozen = O.tree_map(np.copy, ref.params)
    _, info, g = ref._losses(batch, noise, want_grads=True)
    if actor_loss == 'ddpgbc':
        ref.q_abs_override = info['actor/q_abs_mean']
    leaves, grads = dict(O.tree_leaves_with_path(ref.params)), dict(O.tree_leaves_with_path(g))
    assert sorted(leaves) == sorted(grads) and ('modules_actor/log_stds' in leaves) == (not const_std)
    rng = np.random.default_rng(3)
    for path, leaf in leaves.items():
        want = grads[path]
        assert want.shape == leaf.shape, path
        if path.startswith('modules_target_'):
            assert not want.any(), path
            continue
        for flat in rng.choice(leaf.size, size=min(3, leaf.size), replace=False):
            i = np.unravel_index(flat, leaf.shape)
            old = leaf[i]
            leaf[i] = old + 1e-6
            lp = ref.total_loss(batch, noise)[0]
            leaf[i] = old - 1e-6
            lm = ref.total_loss(batch, noise)[0]
            leaf[i] = old
            assert abs((lp - lm) / 2e-6 - want[i]) <= 1e-6 * max(1.0, abs(want[i])), (path, i, (lp - lm) / 2e-6, want[i])


@pytest.mark.parametrize('actor_loss,const_std', CASES)
def test_numpy_and_torch_restatements_agree(actor_loss, const_std):
    from tests import iql_oracle_torch as IT
    cfg, params, batch, noise = _setup(actor_loss=actor_loss, const_std=const_std, actor_layer_norm=const_std)
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    loss, info, g = ref._losses(batch, noise, want_grads=True)
    lt, it, gt = IT.losses(params, cfg, batch, noise)
    assert abs(loss - lt) <= 1e-9 * max(1.0, abs(lt))
    assert set(it) == set(IO.INFO_KEYS[actor_loss][:-3])
    for k, v in it.items():
        assert abs(float(info[k]) - v) <= 1e-9 * max(1.0, abs(v)), k
    ga, gb = dict(O.tree_leaves_with_path(g)), dict(O.tree_leaves_with_path(gt))
    assert sorted(ga) == sorted(gb)
    for p in ga:
        np.testing.assert_allclose(ga[p], gb[p], rtol=1e-8, atol=1e-10 * max(1.0, np.abs(gb[p]).max()), err_msg=p)


def test_expectile_weights_known_answers():
    """agents/iql.py:23-26: weight = expectile where adv >= 0 (zero included), else 1 - expectile."""
    np.testing.assert_array_equal(IO.expectile_weight(np.array([-2.0, -1e-30, 0.0, 1e-30, 3.0]), 0.9), [1 - 0.9, 1 - 0.9, 0.9, 0.9, 0.9])
    d = np.array([-2.0, 0.5])
    assert abs(np.mean(IO.expectile_weight(d, 0.7) * d ** 2) - ((1 - 0.7) * 4.0 + 0.7 * 0.25) / 2) < 1e-15


def test_awr_weight_is_capped_at_100():
    """agents/iql.py:66-67: exp(alpha adv) up to 100: the cap bites from alpha adv = log 100 on."""
    adv = np.array([-1.0, 0.0, 1.0, math.log(100.0) / 3.0 - 1e-9, math.log(100.0) / 3.0 + 1e-9, 50.0])
    w = IO.awr_weight(adv, 3.0)
    np.testing.assert_allclose(w[:3], [math.exp(-3.0), 1.0, math.exp(3.0)], rtol=1e-15)
    assert w[3] < 100.0 and w[4] == 100.0 and w[5] == 100.0
    # a capped row's weight is a constant: it scales the row's log-prob gradient by exactly 100 / B
    cfg, params, batch, noise = _setup(actor_loss='awr', const_std=True, alpha=1e3)
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    f = ref._forward(batch, noise)
    assert (f['w'] == 100.0).any() and f['w'].max() == 100.0
    assert abs(f['actor_loss'] + np.mean(f['w'] * f['lp'])) < 1e-12


def test_log_prob_of_a_hand_computed_2d_case():
    """mean (0.5, -1), log_std (0, log 2), a = (1.5, 1): u = (1, 1); log_prob = -1/2 - 1/2 - log 2 - log(2 pi)."""
    lp = IO.gaussian_log_prob(np.array([[1.5, 1.0]]), np.array([[0.5, -1.0]]), np.array([0.0, math.log(2.0)]))
    assert abs(lp[0] - (-1.0 - math.log(2.0) - math.log(2.0 * math.pi))) < 1e-15
    # at the mean with unit std: -log(2 pi)
    assert abs(IO.gaussian_log_prob(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros(2))[0] + math.log(2.0 * math.pi)) < 1e-15


@pytest.mark.parametrize('actor_loss', ['awr', 'ddpgbc'])
def test_log_stds_past_both_bounds_get_exactly_zero_gradient(actor_loss):
    cfg, params, batch, noise = _setup(actor_loss=actor_loss, const_std=False)
    params['modules_actor']['log_stds'][...] = [-6.0, 3.0, -1.0]
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    _, info, g = ref._losses(batch, noise, want_grads=True)
    gl = g['modules_actor']['log_stds']
    assert gl[0] == 0.0 and gl[1] == 0.0 and gl[2] != 0.0
    assert abs(info['actor/std'] - (math.exp(-5.0) + math.exp(2.0) + math.exp(-1.0)) / 3) < 1e-12
    from tests import iql_oracle_torch as IT
    _, _, gt = IT.losses(params, cfg, batch, noise)
    np.testing.assert_allclose(gt['modules_actor']['log_stds'], gl, rtol=1e-8, atol=1e-12)
    np.testing.assert_array_equal(IO.clip_mask(np.array([-6.0, -5.0, 0.0, 2.0, 3.0])), [0.0, 0.5, 1.0, 0.5, 0.0])
    np.testing.assert_array_equal(IO.unit_clip_mask(np.array([-2.0, -1.0, 0.3, 1.0, 1.5])), [0.0, 0.5, 1.0, 0.5, 0.0])


def test_const_std_has_no_log_stds_leaf_and_unit_std():
    cfg, params, batch, noise = _setup(actor_loss='ddpgbc', const_std=True)
    assert 'log_stds' not in params['modules_actor']
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    _, info, g = ref._losses(batch, noise, want_grads=True)
    assert info['actor/std'] == 1.0 and 'log_stds' not in g['modules_actor']
    # q_actions = clip(mode): the noise is not read
    assert ref.total_loss(batch, None)[0] == ref.total_loss(batch, noise)[0]
    assert abs(info['actor/actor_loss'] - info['actor/q_loss'] - info['actor/bc_loss']) < 1e-12
    assert abs(info['actor/q_loss'] + info['actor/q_mean'] / info['actor/q_abs_mean']) < 1e-12


@pytest.mark.parametrize('actor_loss,n', [('awr', 16), ('ddpgbc', 19)])
def test_update_info_order_and_polyak_of_the_critic_only(actor_loss, n):
    cfg, params, batch, noise = _setup(actor_loss=actor_loss, const_std=False)
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    pre = O.tree_map(np.copy, ref.params)
    _, info = ref.update(batch, noise)
    assert tuple(info) == IO.INFO_KEYS[actor_loss] and len(info) == n
    for (p, a), (_, b), (_, c) in zip(O.tree_leaves_with_path(ref.params['modules_target_critic']),
                                      O.tree_leaves_with_path(pre['modules_target_critic']),
                                      O.tree_leaves_with_path(pre['modules_critic'])):
        np.testing.assert_allclose(a, 0.005 * c + 0.995 * b, rtol=1e-12, err_msg=p)
    assert info['grad/max'] >= 0.0 >= info['grad/min']
    assert not np.array_equal(ref.params['modules_actor']['log_stds'], pre['modules_actor']['log_stds'])


def test_sample_actions_restatement_clips_and_scales():
    cfg, params, batch, _ = _setup(const_std=False)
    ref = IO.OracleIQL(params, cfg, OD, AD, np.float64)
    z = np.random.default_rng(1).standard_normal((B, AD))
    mean = ref.actor_mean(batch['observations'])
    np.testing.assert_array_equal(ref.sample_actions(batch['observations'], z, temperature=0.0), np.clip(mean, -1, 1))
    s = np.exp(params['modules_actor']['log_stds'])
    np.testing.assert_allclose(ref.sample_actions(batch['observations'], z, 0.5), np.clip(mean + 0.5 * s * z, -1, 1), rtol=1e-12)
    assert np.abs(ref.sample_actions(batch['observations'], 10 * z)).max() <= 1.0


def test_config_defaults_registry_and_cabi_defaults():
    import __graft_entry__ as g
    g.build()
    import fql_amd
    from fql_amd import _cabi
    cfg = fql_amd.iql.get_config()
    # the reference's agents/iql.py get_config, key for key
    want = dict(agent_name='iql', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                expectile=0.9, actor_loss='ddpgbc', alpha=1.0, const_std=True, encoder=None)
    assert IO.get_config() == want
    for k, v in want.items():
        assert cfg[k] == v, k
    assert set(cfg) - set(want) == {'ob_dims', 'action_dim', 'rng', 'precision'}
    assert fql_amd.agents['iql'] is fql_amd.IQLAgent and fql_amd.agents['fql'] is fql_amd.FQLAgent
    assert fql_amd.IQL_INFO_KEYS == IO.INFO_KEYS and [len(v) for v in fql_amd.IQL_INFO_KEYS.values()] == [16, 19]
    lib = _cabi.load()
    qc = _cabi.FqlIqlConfig()
    lib.fql_iql_default_config(C.byref(qc))
    assert abs(qc.expectile - 0.9) < 1e-7 and qc.alpha == 1.0 and (qc.actor_loss, qc.const_std) == (1, 1)
    assert list(qc.reserved) == [0] * 8 and C.sizeof(_cabi.FqlIqlConfig) == 48
    assert C.sizeof(_cabi.FqlConfig) == 152   # fql_config keeps its size
    assert lib.fql_abi_version() == 1 and (_cabi.FQL_IQL_AWR_NUM_INFO, _cabi.FQL_IQL_DDPGBC_NUM_INFO) == (16, 19)
    for name in ('fql_iql_default_config', 'fql_iql_create', 'fql_iql_update', 'fql_iql_update_from_dataset', 'fql_iql_total_loss',
                 'fql_iql_sample_actions', 'fql_iql_stats'):
        assert name in _cabi.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize('kw,exc,err', [({'encoder': 'impala_small'}, NotImplementedError, 'encoder'),
                                        ({'precision': 'bf16x3'}, NotImplementedError, 'fp32'),
                                        ({'rng': 'jax'}, NotImplementedError, 'rng'),
                                        ({'actor_loss': 'sac'}, ValueError, 'Unsupported actor loss')])
def test_python_refusals_come_before_the_library(kw, exc, err, monkeypatch):
    import fql_amd
    from fql_amd import _cabi

    def no_lib():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_cabi, 'load', no_lib)
    cfg = fql_amd.iql.get_config()
    cfg.update(kw)
    with pytest.raises(exc, match=err):
        fql_amd.IQLAgent.create(0, np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), cfg)


def test_python_refusals_of_fql_only_paths():
    import fql_amd
    a = object.__new__(fql_amd.IQLAgent)   # no handle: every refusal below must come before the library
    a.config = {'action_dim': AD, 'ob_dims': (OD,), 'batch_size': B}
    for call in (lambda: a.compute_flow_actions(None, None), lambda: a.update_begin(), lambda: a.update_end(),
                 lambda: a.update_end_split(None, None), lambda: a.update_begin_split(None, None), lambda: a.grad_buckets(),
                 lambda: a.update_balanced(B)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match='eps'):
        a._noise_args({'x0': np.zeros((B, AD))}, B)
    with pytest.raises(NotImplementedError, match='JAX'):
        a.total_loss({}, rng=np.zeros(2, np.uint32))
    nz, keep = a._noise_args({'eps': np.zeros((B, AD), np.float32)}, B)
    assert nz.eps1 and not (nz.x0 or nz.t or nz.z or nz.eps2)


def test_agent_groups_refuse_iql_configs(monkeypatch):
    import fql_amd
    from fql_amd import _cabi

    def no_lib():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_cabi, 'load', no_lib)
    with pytest.raises(NotImplementedError, match='IQL'):
        fql_amd.FQLAgentGroup.create([0, 1], np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), fql_amd.iql.get_config())
