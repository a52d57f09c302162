"""CPU: the SAC restatements (tests/sac_oracle.py against finite differences and the torch-autograd restatement), the log-std clip's
gradient, the temperature's gradient, the info layout, the SAC config, registry and C-ABI defaults, and the Python-side refusals.  Nothing
here launches GPU compute."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import sac_oracle as SO

OD, AD, B, SEED = 5, 3, 8, 11


def _setup(**kw):
    cfg = SO.get_config()
    cfg.update(actor_hidden_dims=(16, 16), value_hidden_dims=(16, 16), batch_size=B)
    cfg.update(kw)
    params = SO.randomize(SO.init_params(SEED, OD, AD, cfg, np.float64), SEED + 1)
    ds = O.make_synthetic_dataset(64, OD, AD, seed=SEED)
    batch = O.sample_batch(ds, np.random.default_rng(SEED).integers(0, 64, size=B))
    return cfg, params, batch, SO.make_noise(B, AD, SEED + 2)


CASES = [pytest.param(t, q, be, id=f'tanh{int(t)}-{q}-backup{int(be)}') for t in (True, False) for q in ('min', 'mean')
         for be in (False, True)]
PATHS = ['modules_actor/actor_net/Dense_0/kernel', 'modules_actor/actor_net/Dense_1/bias', 'modules_actor/mean_net/kernel',
         'modules_actor/mean_net/bias', 'modules_actor/log_std_net/kernel', 'modules_actor/log_std_net/bias',
         'modules_alpha/log_value', 'modules_critic/value_net/Dense_0/kernel', 'modules_critic/value_net/Dense_2/bias',
         'modules_critic/value_net/LayerNorm_1/scale']


@pytest.mark.parametrize('tanh_squash,q_agg,backup_entropy', CASES)
def test_gradients_match_finite_differences(tanh_squash, q_agg, backup_entropy):
    """jax.grad of total_loss: the target critic, the actor loss's critic and the alpha of the actor loss and the backup are stored
    parameters (held in `frozen`); the entropy inside alpha_loss is a stop_gradient (held fixed)."""
    cfg, params, batch, noise = _setup(tanh_squash=tanh_squash, q_agg=q_agg, backup_entropy=backup_entropy)
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    ref.frozen = O.tree_map(np.copy, ref.params)
    _, info, g = ref._losses(batch, noise, want_grads=True)
    ref.entropy_override = info['actor/entropy']
    leaves, grads = dict(O.tree_leaves_with_path(ref.params)), dict(O.tree_leaves_with_path(g))
    rng = np.random.default_rng(3)
    for path in PATHS:
        leaf, want = leaves[path], grads[path]
        assert want.shape == leaf.shape, path
        for flat in rng.choice(leaf.size, size=min(3, leaf.size), replace=False):
            i = np.unravel_index(flat, leaf.shape)
            old = leaf[i]
            leaf[i] = old + 1e-6
            lp = ref.total_loss(batch, noise)[0]
            leaf[i] = old - 1e-6
            lm = ref.total_loss(batch, noise)[0]
            leaf[i] = old
            assert abs((lp - lm) / 2e-6 - want[i]) <= 1e-6 * max(1.0, abs(want[i])), (path, i, (lp - lm) / 2e-6, want[i])
    for p, gg in O.tree_leaves_with_path(g):
        if p.startswith('modules_target_'):
            assert not gg.any()


@pytest.mark.parametrize('tanh_squash,q_agg,backup_entropy', CASES)
def test_numpy_and_torch_restatements_agree(tanh_squash, q_agg, backup_entropy):
    from tests import sac_oracle_torch as ST
    cfg, params, batch, noise = _setup(tanh_squash=tanh_squash, q_agg=q_agg, backup_entropy=backup_entropy)
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    loss, info, g = ref._losses(batch, noise, want_grads=True)
    lt, it, gt = ST.losses(params, cfg, batch, noise, AD)
    assert abs(loss - lt) <= 1e-9 * max(1.0, abs(lt))
    for k, v in it.items():
        assert abs(float(info[k]) - v) <= 1e-9 * max(1.0, abs(v)), k
    ga, gb = dict(O.tree_leaves_with_path(g)), dict(O.tree_leaves_with_path(gt))
    assert sorted(ga) == sorted(gb)
    for p in ga:
        np.testing.assert_allclose(ga[p], gb[p], rtol=1e-8, atol=1e-10 * max(1.0, np.abs(gb[p]).max()), err_msg=p)


def test_log_std_past_both_bounds_gets_exactly_zero_gradient():
    """A constructed case: log_std_net's bias pushes column 0 far below -5 and column 1 far above 2 for every row; column 2 stays inside."""
    cfg, params, batch, noise = _setup()
    ls = params['modules_actor']['log_std_net']
    ls['kernel'][...] = 0.0
    ls['bias'][...] = [-40.0, 40.0, -1.0]
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    raw = ref.actor_heads(batch['observations'])[1]
    assert (raw[:, 0] < SO.LOG_STD_MIN).all() and (raw[:, 1] > SO.LOG_STD_MAX).all()
    _, _, g = ref._losses(batch, noise, want_grads=True)
    gl = g['modules_actor']['log_std_net']
    assert gl['bias'][0] == 0.0 and gl['bias'][1] == 0.0 and gl['bias'][2] != 0.0
    assert not gl['kernel'][:, :2].any() and gl['kernel'][:, 2].any()
    from tests import sac_oracle_torch as ST
    _, _, gt = ST.losses(params, cfg, batch, noise, AD)
    np.testing.assert_allclose(gt['modules_actor']['log_std_net']['bias'], gl['bias'], rtol=1e-8, atol=1e-12)
    # the clip's own derivative: 1 inside, 0 outside, 1/2 at a bound (jnp.clip)
    np.testing.assert_array_equal(SO.clip_mask(np.array([-6.0, -5.0, 0.0, 2.0, 3.0])), [0.0, 0.5, 1.0, 0.5, 0.0])


def test_log_value_gradient_and_temperature_infos():
    cfg, params, batch, noise = _setup(target_entropy=0.3)
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    _, info, g = ref._losses(batch, noise, want_grads=True)
    alpha = math.exp(float(params['modules_alpha']['log_value']))
    assert abs(info['actor/alpha'] - alpha) < 1e-12
    assert abs(info['actor/alpha_loss'] - alpha * (info['actor/entropy'] - 0.3)) < 1e-12
    assert g['modules_alpha']['log_value'].shape == ()
    assert abs(float(g['modules_alpha']['log_value']) - alpha * (info['actor/entropy'] - 0.3)) < 1e-12
    assert abs(info['actor/total_loss'] - info['actor/actor_loss'] - info['actor/alpha_loss']) < 1e-12
    # the automatic target entropy: -multiplier * act_dim
    cfg2 = dict(cfg, target_entropy=None)
    assert SO.OracleSAC(params, cfg2, OD, AD, np.float64).target_entropy() == -0.5 * AD


def test_update_moves_log_value_and_polyaks_only_the_critic():
    cfg, params, batch, noise = _setup()
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    pre = O.tree_map(np.copy, ref.params)
    _, info = ref.update(batch, noise)
    assert tuple(info) == SO.INFO_KEYS and len(info) == 14
    assert float(ref.params['modules_alpha']['log_value']) != float(pre['modules_alpha']['log_value'])
    for (p, a), (_, b), (_, c) in zip(O.tree_leaves_with_path(ref.params['modules_target_critic']),
                                      O.tree_leaves_with_path(pre['modules_target_critic']),
                                      O.tree_leaves_with_path(pre['modules_critic'])):
        np.testing.assert_allclose(a, 0.005 * c + 0.995 * b, rtol=1e-12, err_msg=p)
    assert info['grad/max'] >= 0.0 >= info['grad/min']


def test_sample_actions_restatement_clips_and_scales():
    cfg, params, batch, _ = _setup()
    ref = SO.OracleSAC(params, cfg, OD, AD, np.float64)
    z = np.random.default_rng(1).standard_normal((B, AD))
    a = ref.sample_actions(batch['observations'], z)
    assert np.abs(a).max() <= 1.0
    m, _ = ref.actor_heads(batch['observations'])
    np.testing.assert_allclose(ref.sample_actions(batch['observations'], z, temperature=0.0), np.tanh(m), rtol=1e-12)
    ref2 = SO.OracleSAC(params, dict(cfg, tanh_squash=False), OD, AD, np.float64)
    np.testing.assert_allclose(ref2.sample_actions(batch['observations'], z, temperature=0.0), np.clip(m, -1, 1), rtol=1e-12)


def test_config_defaults_registry_and_cabi_defaults():
    import __graft_entry__ as g
    g.build()
    import fql_amd
    from fql_amd import _cabi
    cfg = fql_amd.sac.get_config()
    # the reference's agents/sac.py get_config, key for key
    want = dict(agent_name='sac', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                target_entropy=None, target_entropy_multiplier=0.5, tanh_squash=True, state_dependent_std=True, actor_fc_scale=0.01,
                q_agg='min', backup_entropy=False, encoder=None)
    assert SO.get_config() == want
    for k, v in want.items():
        assert cfg[k] == v, k
    assert set(cfg) - set(want) == {'ob_dims', 'action_dim', 'rng', 'precision'}
    assert cfg['rng'] == 'engine' and cfg['precision'] == 'fp32'
    assert fql_amd.agents['sac'] is fql_amd.SACAgent and fql_amd.agents['fql'] is fql_amd.FQLAgent
    assert fql_amd.SAC_INFO_KEYS == SO.INFO_KEYS and len(fql_amd.SAC_INFO_KEYS) == 14
    lib = _cabi.load()
    sc = _cabi.FqlSacConfig()
    lib.fql_sac_default_config(C.byref(sc))
    assert math.isnan(sc.target_entropy) and abs(sc.target_entropy_multiplier - 0.5) < 1e-9
    assert (sc.tanh_squash, sc.state_dependent_std, sc.backup_entropy) == (1, 1, 0)
    assert abs(sc.actor_fc_scale - 0.01) < 1e-9 and list(sc.reserved) == [0] * 6
    assert C.sizeof(_cabi.FqlSacConfig) == 48
    assert C.sizeof(_cabi.FqlConfig) == 152   # fql_config keeps its size
    assert lib.fql_abi_version() == 1 and _cabi.FQL_SAC_NUM_INFO == 14 and _cabi.FQL_NUM_INFO == 13
    for name in ('fql_sac_create', 'fql_sac_update', 'fql_sac_update_from_dataset', 'fql_sac_update_balanced', 'fql_sac_total_loss',
                 'fql_sac_sample_actions', 'fql_sac_stats', 'fql_sac_default_config', 'fql_read_info_n', 'fql_info_wait_n'):
        assert name in _cabi.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize('kw,err', [({'encoder': 'impala_small'}, 'encoder'), ({'precision': 'bf16x3'}, 'fp32'), ({'rng': 'jax'}, 'rng'),
                                    ({'state_dependent_std': False}, 'state_dependent_std')])
def test_python_refusals_come_before_the_library(kw, err, monkeypatch):
    import fql_amd
    from fql_amd import _cabi

    def no_lib():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_cabi, 'load', no_lib)
    cfg = fql_amd.sac.get_config()
    cfg.update(kw)
    with pytest.raises(NotImplementedError, match=err):
        fql_amd.SACAgent.create(0, np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), cfg)


def test_python_refusals_of_fql_only_paths():
    import fql_amd
    a = object.__new__(fql_amd.SACAgent)   # no handle: every refusal below must come before the library
    a.config = {'action_dim': AD, 'ob_dims': (OD,), 'batch_size': B}
    for call in (lambda: a.compute_flow_actions(None, None), lambda: a.update_begin(), lambda: a.update_end(),
                 lambda: a.update_end_split(None, None), lambda: a.update_begin_split(None, None), lambda: a.grad_buckets()):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match='eps1'):
        a._noise_args({'x0': np.zeros((B, AD))}, B)
    with pytest.raises(NotImplementedError, match='JAX'):
        a.total_loss({}, rng=np.zeros(2, np.uint32))
    nz, keep = a._noise_args({'eps1': np.zeros((B, AD), np.float32), 'eps2': np.ones((B, AD), np.float32)}, B)
    assert nz.eps1 and nz.eps2 and not (nz.x0 or nz.t or nz.z)


def test_agent_groups_refuse_sac_configs(monkeypatch):
    import fql_amd
    from fql_amd import _cabi

    def no_lib():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_cabi, 'load', no_lib)
    with pytest.raises(NotImplementedError, match='SAC'):
        fql_amd.FQLAgentGroup.create([0, 1], np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), fql_amd.sac.get_config())
