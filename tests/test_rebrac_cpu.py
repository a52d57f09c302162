"""CPU: the ReBRAC restatements (tests/rebrac_oracle.py, tests/rebrac_oracle_torch.py) against each other, finite differences and the
reference's quirks; the ReBRAC config, registry, C-ABI defaults, Dataset.return_next_actions and the Python-side refusals.  Nothing here
launches GPU work."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import rebrac_oracle as RO

OD, AD, B, H = 5, 3, 8, (8, 8)


def _setup(seed=0, **kw):
    cfg = RO.get_config()
    cfg.update(actor_hidden_dims=H, value_hidden_dims=H, alpha_actor=0.7, alpha_critic=0.4, actor_layer_norm=True)
    cfg.update(kw)
    params = RO.init_params(seed, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(seed + 1)
    for p, leaf in O.tree_leaves_with_path(params):
        leaf += (0.5 if p.endswith('mean_net/kernel') else 0.1) * rng.standard_normal(leaf.shape)   # every leaf matters; targets differ
    batch = {'observations': rng.standard_normal((B, OD)), 'actions': rng.uniform(-1, 1, (B, AD)), 'rewards': rng.standard_normal(B),
             'masks': (rng.random(B) > 0.2).astype(np.float64), 'next_observations': rng.standard_normal((B, OD)),
             'next_actions': rng.uniform(-1, 1, (B, AD))}
    noise = {'eps1': 3.0 * rng.standard_normal((B, AD))}   # some entries past actor_noise_clip
    return cfg, params, batch, noise


PATHS = ['modules_critic/value_net/Dense_0/kernel', 'modules_critic/value_net/LayerNorm_1/scale', 'modules_critic/value_net/Dense_2/bias',
         'modules_actor/actor_net/Dense_0/kernel', 'modules_actor/actor_net/LayerNorm_1/bias', 'modules_actor/mean_net/kernel',
         'modules_actor/mean_net/bias']
# the configurations of the GPU matrix (tests/test_gpu_rebrac.py SHAPE_CASES) beside the default one, with the leaves they add
CONFIGS = {
    'no_layer_norm': (dict(layer_norm=False), ['modules_critic/value_net/Dense_1/kernel']),
    'ragged_depths': (dict(actor_hidden_dims=(9, 7), value_hidden_dims=(6, 10, 8)),
                      ['modules_critic/value_net/Dense_3/kernel', 'modules_critic/value_net/LayerNorm_2/bias',
                       'modules_actor/actor_net/Dense_1/kernel']),
}
CASES = [pytest.param(full, tanh, conf, id=f'{full}-{tanh}' if conf is None else f'{conf}-{full}-{tanh}')
         for conf in [None] + list(CONFIGS) for tanh in (True, False) for full in (True, False)]


@pytest.mark.parametrize('full,tanh_squash,conf', CASES)
def test_gradients_match_finite_differences(full, tanh_squash, conf):
    """jax.grad of total_loss: targets and the actor loss's critic are stored parameters; lam is a stop_gradient (held fixed here)."""
    kw, extra = CONFIGS.get(conf, ({}, []))
    cfg, params, batch, noise = _setup(tanh_squash=tanh_squash, **kw)
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    ref.frozen = O.tree_map(np.copy, ref.params)
    _, info, g = ref._losses(batch, noise, want_grads=True, full_update=full)
    if full:
        ref.lam_override = info['_lam']
    leaves, grads = dict(O.tree_leaves_with_path(ref.params)), dict(O.tree_leaves_with_path(g))
    rng = np.random.default_rng(3)
    for path in [p for p in PATHS + extra if p in leaves]:
        leaf, want = leaves[path], grads[path]
        if not full and path.startswith('modules_actor/'):
            assert not want.any(), path   # critic-only step: the actor's gradient is zero
        for flat in rng.choice(leaf.size, size=min(3, leaf.size), replace=False):
            i = np.unravel_index(flat, leaf.shape)
            old = leaf[i]
            leaf[i] = old + 1e-6
            lp = ref.total_loss(batch, noise, full_update=full)[0]
            leaf[i] = old - 1e-6
            lm = ref.total_loss(batch, noise, full_update=full)[0]
            leaf[i] = old
            assert abs((lp - lm) / 2e-6 - want[i]) <= 1e-6 * max(1.0, abs(want[i])), (path, i)
    for p, gg in O.tree_leaves_with_path(g):
        if p.startswith('modules_target_'):
            assert not gg.any()


@pytest.mark.parametrize('full,tanh_squash,conf', CASES)
def test_numpy_and_torch_restatements_agree(full, tanh_squash, conf):
    from tests import rebrac_oracle_torch as RT
    cfg, params, batch, noise = _setup(tanh_squash=tanh_squash, **CONFIGS.get(conf, ({}, []))[0])
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    l1, i1, g1 = ref._losses(batch, noise, want_grads=True, full_update=full)
    l2, i2, g2 = RT.losses(params, cfg, batch, noise, full_update=full)
    assert abs(l1 - l2) <= 1e-10 * max(1.0, abs(l2))
    for k in i2:
        assert abs(float(i1[k]) - i2[k]) <= 1e-10 * max(1.0, abs(i2[k])), k
    g2 = dict(O.tree_leaves_with_path(g2))
    for p, g in O.tree_leaves_with_path(g1):
        np.testing.assert_allclose(g, g2[p], rtol=0, atol=1e-9 * max(np.abs(g2[p]).max(), 1.0), err_msg=p)


def test_tie_splits_the_gradient_equally():
    """Identical critic members: every q1 == q2, jnp.min's gradient splits 1/2 : 1/2 (torch.amin does the same)."""
    from tests import rebrac_oracle_torch as RT
    cfg, params, batch, noise = _setup()
    vn = params['modules_critic']['value_net']
    for sub in vn.values():
        for v in sub.values():
            v[1] = v[0]
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    a = ref._mode(ref.actor_mean('modules_actor', batch['observations']))
    qs = ref._critic('modules_critic', batch['observations'], a)
    assert (qs[0] == qs[1]).all()
    _, _, g1 = ref._losses(batch, noise, want_grads=True)
    _, _, g2 = RT.losses(params, cfg, batch, noise)
    g2 = dict(O.tree_leaves_with_path(g2))
    for p, g in O.tree_leaves_with_path(g1):
        if p.startswith('modules_actor/'):
            assert np.abs(g).max() > 0
            np.testing.assert_allclose(g, g2[p], rtol=0, atol=1e-9 * max(np.abs(g2[p]).max(), 1.0), err_msg=p)


def test_critic_only_step_moves_actor_by_momentum_and_leaves_targets():
    cfg, params, batch, noise = _setup()
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    ref.update(batch, noise, full_update=True)
    before = O.tree_map(np.copy, ref.params)
    mu_before = O.tree_map(np.copy, ref.mu)
    _, info = ref.update(batch, noise, full_update=False)
    assert tuple(info) == RO.CRITIC_INFO_KEYS
    assert info['grad/max'] >= 0 >= info['grad/min']
    for p, v in O.tree_leaves_with_path(ref.params):
        old = dict(O.tree_leaves_with_path(before))[p]
        if p.startswith('modules_target_'):
            np.testing.assert_array_equal(v, old, err_msg=p)
        elif p.startswith('modules_actor/'):
            m0 = dict(O.tree_leaves_with_path(mu_before))[p]
            assert (v[m0 != 0] != old[m0 != 0]).all(), p   # Adam with a zero gradient still steps where mu != 0
            np.testing.assert_allclose(dict(O.tree_leaves_with_path(ref.mu))[p], 0.9 * m0, err_msg=p)
    assert ref.count == 2 and ref.step == 3


def test_info_keys_and_order_per_step_kind():
    cfg, params, batch, noise = _setup()
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    _, full = ref.update(batch, noise, full_update=True)
    assert tuple(full) == RO.INFO_KEYS and full['actor/std'] == 1.0
    assert full['actor/total_loss'] == pytest.approx(full['actor/actor_loss'] + full['actor/bc_loss'])
    assert full['actor/bc_loss'] == pytest.approx(cfg['alpha_actor'] * full['actor/mse'])
    _, crit = ref.update(batch, noise, full_update=False)
    assert tuple(crit) == RO.CRITIC_INFO_KEYS == RO.INFO_KEYS[:4] + RO.INFO_KEYS[9:]
    loss, info = ref.total_loss(batch, noise, full_update=False)
    assert tuple(info) == RO.INFO_KEYS[:4] and loss == info['critic/critic_loss']


def test_next_actions_clamp_at_the_last_row():
    from fql_amd.datasets import Dataset
    ds = O.make_synthetic_dataset(16, OD, AD, seed=0)
    d = Dataset.create(**ds)
    idx = np.array([0, 7, 15, 15])
    assert 'next_actions' not in d.sample(4, idxs=idx)   # the default changes nothing
    d.return_next_actions = True
    got = d.sample(4, idxs=idx)
    np.testing.assert_array_equal(got['next_actions'], ds['actions'][[1, 8, 15, 15]])
    np.testing.assert_array_equal(got['next_actions'], RO.next_actions(ds['actions'], idx, 16))
    ends = np.nonzero(ds['terminals'] > 0)[0]
    ends = ends[ends < 15]
    if len(ends):   # the reference's end-of-trajectory quirk: the next episode's first action
        np.testing.assert_array_equal(d.get_subset(ends[:1])['next_actions'], ds['actions'][ends[:1] + 1])


def test_sample_actions_restatement_clips():
    cfg, params, batch, noise = _setup()
    ref = RO.OracleReBRAC(params, cfg, OD, AD, np.float64)
    obs = batch['observations']
    z = 10.0 * noise['eps1']
    a = ref.sample_actions(obs, z)
    mode = ref._mode(ref.actor_mean('modules_actor', obs))
    assert np.abs(a).max() <= 1.0 and np.abs(a - np.clip(a, -1, 1)).max() == 0
    assert np.abs(np.clip(mode + np.clip(z * 0.2, -0.5, 0.5), -1, 1) - a).max() < 1e-12
    np.testing.assert_array_equal(ref.sample_actions(obs, z, temperature=0.0), np.clip(mode, -1, 1))


def test_config_defaults_registry_and_cabi_defaults():
    import __graft_entry__ as g
    g.build()
    import fql_amd
    from fql_amd import _cabi
    cfg = fql_amd.rebrac.get_config()
    for k, v in RO.get_config().items():
        assert cfg[k] == v, k
    assert cfg['rng'] == 'engine' and cfg['precision'] == 'fp32'
    assert fql_amd.agents['rebrac'] is fql_amd.ReBRACAgent and fql_amd.agents['fql'] is fql_amd.FQLAgent
    assert fql_amd.REBRAC_INFO_KEYS == RO.INFO_KEYS and fql_amd.REBRAC_CRITIC_INFO_KEYS == RO.CRITIC_INFO_KEYS
    lib = _cabi.load()
    rc = _cabi.FqlRebracConfig()
    lib.fql_rebrac_default_config(C.byref(rc))
    assert (rc.alpha_actor, rc.alpha_critic, rc.tanh_squash) == (0.0, 0.0, 1)
    assert abs(rc.actor_noise - 0.2) < 1e-7 and abs(rc.actor_noise_clip - 0.5) < 1e-7 and abs(rc.actor_fc_scale - 0.01) < 1e-9
    assert list(rc.reserved) == [0] * 6
    assert C.sizeof(_cabi.FqlRebracConfig) == 48
    assert C.sizeof(_cabi.FqlConfig) == 152   # fql_config keeps its size
    assert _cabi.FQL_REBRAC_NUM_INFO == 12 and _cabi.FQL_REBRAC_CRITIC_NUM_INFO == 7
    for name in ('fql_rebrac_create', 'fql_rebrac_update', 'fql_rebrac_update_from_dataset', 'fql_rebrac_total_loss',
                 'fql_rebrac_sample_actions', 'fql_rebrac_stats', 'fql_rebrac_default_config'):
        assert name in _cabi.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize('kw,err', [({'encoder': 'impala_small'}, 'encoder'), ({'precision': 'bf16x3'}, 'fp32'), ({'rng': 'jax'}, 'rng')])
def test_python_refusals_come_before_the_library(kw, err, monkeypatch):
    import fql_amd
    from fql_amd import _cabi

    def no_lib():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_cabi, 'load', no_lib)
    cfg = fql_amd.rebrac.get_config()
    cfg.update(kw)
    with pytest.raises(NotImplementedError, match=err):
        fql_amd.ReBRACAgent.create(0, np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32), cfg)


def test_python_refusals_of_fql_only_paths_and_missing_next_actions():
    import fql_amd
    a = object.__new__(fql_amd.ReBRACAgent)   # no handle: every refusal below must come before the library
    a.config = {'action_dim': AD, 'ob_dims': (OD,), 'batch_size': B}
    for call in (lambda: a.compute_flow_actions(None, None), lambda: a.update_balanced(), lambda: a.update_begin(),
                 lambda: a.update_end(), lambda: a.update_end_split(None, None), lambda: a.update_begin_split(None, None),
                 lambda: a.grad_buckets(), lambda: a.create_replay_buffer(4)):
        with pytest.raises(NotImplementedError):
            call()
    _, _, batch, _ = _setup()
    batch.pop('next_actions')
    with pytest.raises(KeyError, match='next_actions'):
        a.update(batch)
    with pytest.raises(ValueError, match='eps1'):
        a._noise_args({'x0': np.zeros((B, AD))}, B)
