"""GPU: the SAC agent (agents/sac.py; RLPD's learner) on the engine against the fp64 restatement in tests/sac_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import sac_oracle as SO
from tests.util import assert_info_close, leaf_dict, sync_restatement

pytestmark = pytest.mark.gpu
OD, AD = 29, 8
MARGIN = 1e-3


def _cfg(H, B, actor=None, value=None, **kw):
    """`actor` / `value`: the hidden tuples where they are not 4 layers of H."""
    import fql_amd
    cfg = fql_amd.sac.get_config()
    cfg.update(actor_hidden_dims=tuple(actor or (H,) * 4), value_hidden_dims=tuple(value or (H,) * 4), batch_size=B)
    cfg.update(kw)
    return cfg


def _problem(H=64, B=64, seed=0, od=OD, ad=AD, actor=None, value=None, **kw):
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    return _cfg(H, B, actor, value, **kw), ds, O.sample_batch(ds, idx), SO.make_noise(B, ad, seed + 2)


def _randomized(params, seed, scale=0.1):
    """Biases / LN parameters away from init, wide head biases (so the log-std clip and tanh saturation occur), log_value != 0,
    target != online."""
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, dtype=np.float64), params)
    for path, leaf in O.tree_leaves_with_path(out):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += scale * rng.standard_normal(leaf.shape)
        if path.endswith('log_std_net/bias'):   # columns from far below -5 to far above 2
            leaf += rng.permutation(np.linspace(-10.0, 7.0, leaf.shape[-1]))
        if path.endswith('mean_net/bias'):
            leaf += rng.uniform(-3.0, 3.0, size=leaf.shape)
        if path.endswith('_net/kernel') and 'actor_net' not in path:
            leaf *= 20.0
    out['modules_alpha']['log_value'] = np.asarray(-0.7)
    out['modules_target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), out['modules_critic'])
    return O.tree_map(lambda a: np.asarray(a, dtype=np.float32), out)


def _agent(cfg, batch, seed=3, params=None):
    import fql_amd
    a = fql_amd.SACAgent.create(seed, batch['observations'][:1], batch['actions'][:1], cfg)
    if params is not None:
        a.set_params(params)
    return a


def _same_state(a, b):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step'])
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{part} {k}')


def test_leaves_match_reference_layout_and_init():
    cfg, _, batch, _ = _problem()
    a = _agent(cfg, batch)
    want = {p: v.shape for p, v in O.tree_leaves_with_path(SO.init_params(0, OD, AD, cfg))}
    assert dict(a.leaves()) == want
    assert dict(a.leaves())['modules_alpha/log_value'] == ()
    p = leaf_dict(a.get_params())
    assert p['modules_alpha/log_value'].shape == () and float(p['modules_alpha/log_value']) == 0.0
    assert p['modules_actor/mean_net/kernel'].shape == (64, AD) and p['modules_actor/log_std_net/bias'].shape == (AD,)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.endswith('/kernel'):
            s = cfg['actor_fc_scale'] if ('mean_net' in k or 'log_std_net' in k) else 1.0
            lim = np.sqrt(6.0 * s / (v.shape[-2] + v.shape[-1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
        if k.startswith('modules_target_'):
            np.testing.assert_array_equal(v, p[k.replace('modules_target_', 'modules_')])
    assert not np.array_equal(p['modules_actor/mean_net/kernel'], p['modules_actor/log_std_net/kernel'])


def _check_step(a, ref, batch, noise, cfg, pre):
    """One update of both sides on (batch, noise) from their current state.  Returns the worst gradient error relative to its leaf's
    largest gradient, with the leaf's name, and the restatement's infos."""
    _, want, g_ref = ref._losses(batch, noise, want_grads=True)
    mu0 = leaf_dict(a.get_opt_state()['mu'])
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == SO.INFO_KEYS
    want.update(ref.grad_stats(g_ref))   # OracleSAC.update, on the gradients computed above
    ref.apply_gradients(g_ref)
    want = {k: float(want[k]) for k in SO.INFO_KEYS}
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=SO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    worst = (0.0, '')
    for p, g in leaf_dict(g_ref).items():
        if p.startswith('modules_target_'):   # Polyak from the PRE-step critic
            np.testing.assert_allclose(new[p], 0.005 * pre[p.replace('target_', '')] + 0.995 * pre[p], atol=1e-6, err_msg=p)
            continue
        # (5e-5: the critic's bias gradients at B = 256 sum 256 fp32 rows of LayerNorm backward)
        tol = 5e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9
        got = (mu[p] - np.float32(0.9) * mu0[p]) / 0.1
        worst = max(worst, (float(np.abs(got - g).max() / max(np.abs(g).max(), 1e-30)), p))
        np.testing.assert_allclose(got, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
        d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))
        stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
        assert np.max(d[stable], initial=0) <= 2e-6, (p, np.max(d[stable], initial=0))
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p
    return worst, want


@pytest.mark.parametrize('H,B,tanh_squash,backup_entropy,q_agg', [(64, 64, True, False, 'min'), (64, 64, False, False, 'min'),
                                                                   (64, 64, True, True, 'mean'), (512, 256, True, False, 'min'),
                                                                   (512, 256, False, True, 'min')])
def test_update_matches_fp64_restatement(H, B, tanh_squash, backup_entropy, q_agg):
    """Two steps: the second from non-zero moments."""
    cfg, _, batch, noise = _problem(H, B, seed=1, tanh_squash=tanh_squash, backup_entropy=backup_entropy, q_agg=q_agg)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 5)
    a.set_params(params)
    ref = SO.OracleSAC(params, dict(cfg), OD, AD, np.float64)
    raw = ref.actor_heads(batch['observations'])[1]
    assert (raw < SO.LOG_STD_MIN).any() and (raw > SO.LOG_STD_MAX).any()   # the clip bites on both sides
    _check_step(a, ref, batch, noise, cfg, leaf_dict(params))
    _check_step(a, ref, batch, SO.make_noise(B, AD, 77), cfg, leaf_dict(a.get_params()))
    opt = a.get_opt_state()
    assert opt['count'] == 2 and opt['step'] == 3


# ---- the shapes that switch kernel paths -----------------------------------------------------------------------------------------------
#
# What each case reaches, from the conditions in fql_amd/csrc/fql_engine.hip.  The actor's last layer is [H, 2 ap] with ap =
# pad16(act): the mean in columns [0, act), the raw log-std in [ap, ap + act); fql_sac_act_kernel reads both and writes the action
# block of the critic's input at column obs with row stride in_p = round64(obs + act).  The critic's input gradient under the actor
# loss is the lean 16-column OP_DGRAD0 when H is a multiple of 512, act <= 16 and obs + 16 <= in_p; otherwise the generic dgrad.
#   name: (obs, act, B, actor hidden, value hidden, cfg overrides, steps, data seed, parameter seed)
# tanh_squash=True and q_agg='min' unless overridden.  The seeds are the first (data, parameter) pair of a CPU search (parameter seeds
# from 5, data seeds 1..4 for each) for which the fp64 restatement keeps every raw log-std MARGIN away from -5 and 2 and every target
# pair MARGIN apart in the first step and, on its own trajectory, 3 MARGIN in the second (tests/test_kink_margins_cpu.py checks that
# on the CPU).  The second step runs from the engine's own state (sync_restatement), which the CPU cannot know: the room is for that,
# and the test asserts MARGIN at the state it actually runs from.
SHAPE_CASES = {
    # OP_DGRAD0 with all 16 columns live; head layer 32 wide with no padding column
    'act16': (29, 16, 256, (512,) * 4, (512,) * 4, {}, 2, 4, 5),
    # generic dgrad (act > 16, in_p 128); head layer 64 wide: raw log-std in columns [32, 53)
    'humanoidmaze': (69, 21, 256, (512,) * 4, (512,) * 4, {}, 2, 1, 10),
    # the actor on 2048 rows, the critics at M = 1024; OP_DGRAD0 with 4 live columns (in_p 64, 40 + 16 <= 64).  One step: the fp64
    # restatement costs most here.
    'b1024': (40, 4, 1024, (512,) * 4, (512,) * 4, {}, 1, 1, 5),
    # ragged widths and different depths; head layer 64 wide with 8 padding columns per half; generic dgrad (K = 80)
    'ragged_depths': (45, 24, 48, (64, 64), (80, 48, 64), dict(backup_entropy=True), 2, 1, 5),
    # 256 + 16 rows, 544 actor rows: M no multiple of 64; no tanh
    'b272': (11, 5, 272, (64,) * 4, (64,) * 4, dict(tanh_squash=False), 2, 1, 5),
    # hidden widths that are no multiple of 16: out 50 of out_p 64 in the actor and the critics (LayerNorm over 50 of 64 columns)
    'w50_padded': (29, 8, 32, (50,) * 3, (50,) * 3, {}, 2, 1, 5),
}


def shape_problem(case):
    """(od, ad, cfg, batch, params, noises): the problem of one SHAPE_CASES entry, built without an engine (SO.init_params moved by
    _randomized on both sides).  noises[i] is the draw of step i."""
    od, ad, B, actor, value, kw, steps, seed, pseed = SHAPE_CASES[case]
    cfg, _, batch, noise = _problem(0, B, seed, od, ad, actor, value, **kw)
    params = _randomized(SO.init_params(pseed, od, ad, cfg), pseed)
    return od, ad, cfg, batch, params, [noise, SO.make_noise(B, ad, 77)][:steps]


@pytest.mark.parametrize('case', list(SHAPE_CASES))
def test_shape_cases_match_fp64_restatement(case):
    """total_loss (no state change), then the update steps of test_update_matches_fp64_restatement, at the shapes above, the second
    one from the engine's own state and moments."""
    od, ad, cfg, batch, params, noises = shape_problem(case)
    a = _agent(cfg, batch, params=params)
    ref = SO.OracleSAC(params, dict(cfg), od, ad, np.float64)
    raw = ref.actor_heads(batch['observations'])[1]
    assert (raw < SO.LOG_STD_MIN).any() and (raw > SO.LOG_STD_MAX).any()   # the clip bites on both sides
    loss, info = a.total_loss(batch, noise=noises[0])
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0
    worst = (0.0, '')
    for i, nz in enumerate(noises):
        if i:
            sync_restatement(ref, a)
        margins = ref.kink_margins(batch, nz)
        assert min(margins.values()) >= MARGIN, margins
        w, want = _check_step(a, ref, batch, nz, cfg, leaf_dict(a.get_params()))
        worst = max(worst, w)
        if i == 0:   # the first step's infos are total_loss's: the restatement computes them once
            assert tuple(info) == SO.INFO_KEYS[:11]
            assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=SO.INFO_KEYS[:11])
            want_loss = want['critic/critic_loss'] + want['actor/total_loss']
            assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    opt = a.get_opt_state()
    assert opt['count'] == len(noises) and opt['step'] == len(noises) + 1
    print(f'worst relative gradient error {worst[0]:.3e} ({worst[1]})')


def test_sample_actions_at_act21_hidden_512():
    """The 64-wide head layer in the sampling program: n = 1, 37 and 4097 (one row past the first 4096-row chunk), explicit noise."""
    od, ad, cfg, batch, params, _ = shape_problem('humanoidmaze')
    a = _agent(cfg, batch, params=params)
    ref = SO.OracleSAC(params, dict(cfg), od, ad, np.float64)
    rng = np.random.default_rng(21)
    obs = rng.standard_normal((4097, od)).astype(np.float32)
    z = rng.standard_normal((4097, ad)).astype(np.float32)
    want = ref.sample_actions(obs, z)   # row-wise: the first n rows are the n-row call's
    for n in (1, 37, 4097):
        got = a.sample_actions(obs[:n], noises=z[:n])
        assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
        np.testing.assert_allclose(got, want[:n], atol=2e-5, err_msg=str(n))
        np.testing.assert_array_equal(got[n - 1], a.sample_actions(obs[n - 1], noises=z[n - 1]))


def test_total_loss_matches_and_changes_no_state():
    cfg, _, batch, noise = _problem(seed=2)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 6)
    a.set_params(params)
    ref = SO.OracleSAC(params, dict(cfg), OD, AD, np.float64)
    loss, info = a.total_loss(batch, noise=noise)
    want_loss, want = ref.total_loss(batch, noise)
    assert tuple(info) == SO.INFO_KEYS[:11]
    assert_info_close(info, want, keys=SO.INFO_KEYS[:11])
    assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0


def test_trajectory_100_updates_from_device_dataset():
    cfg, ds, _, _ = _problem(seed=3)
    rng = np.random.default_rng(9)
    a = _agent(cfg, {'observations': ds['observations'][:1], 'actions': ds['actions'][:1]})
    a.upload_dataset(ds)
    ref = SO.OracleSAC(a.get_params(), dict(cfg), OD, AD, np.float64)
    B = cfg['batch_size']
    for i in range(100):
        idx = rng.integers(0, len(ds['observations']), size=B)
        noise = SO.make_noise(B, AD, 1000 + i)
        a.update_from_dataset(idxs=idx, noise=noise)
        ref.update(O.sample_batch(ds, idx), noise)
    _, info = a.update(O.sample_batch(ds, idx), noise=noise)
    _, want = ref.update(O.sample_batch(ds, idx), noise)
    info = info.to_dict()
    for k in ('critic/critic_loss', 'critic/q_mean', 'actor/actor_loss', 'actor/alpha', 'actor/entropy', 'actor/std'):
        assert abs(info[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, info[k], want[k])
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


def test_update_from_dataset_explicit_rows_equals_update():
    cfg, ds, _, noise = _problem(seed=4)
    B, n = cfg['batch_size'], len(ds['observations'])
    idx = np.random.default_rng(4).integers(0, n, size=B)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    a.upload_dataset(ds)
    for _ in range(3):
        a.update_from_dataset(idxs=idx, noise=noise)
        b.update(O.sample_batch(ds, idx), noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def _ring(a, ds, n, rew):
    """n transitions of `ds` into the replay ring, rewards marked `rew` (the dataset's are -1 or 0)."""
    a.create_replay_buffer(4 * n)
    for i in range(n):
        a.add_transition({'observations': ds['observations'][i], 'actions': ds['actions'][i], 'rewards': rew,
                          'masks': ds['masks'][i], 'next_observations': ds['next_observations'][i]}, replay=True)


def test_update_balanced_explicit_rows_equals_update_on_concatenated_batch():
    from fql_amd import _cabi
    cfg, ds, _, noise = _problem(seed=10)
    B = cfg['batch_size']
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    a.upload_dataset(ds)
    a.create_replay_buffer(64)
    with pytest.raises(ValueError):   # FQL_E_INVALID while the ring is empty
        a.update_balanced(B)
    assert a._lib.fql_sac_update_balanced(a._h, None, None, B, None, None, None) == _cabi.FQL_E_INVALID
    n = 40
    for i in range(n):
        a.add_transition({'observations': ds['observations'][i], 'actions': ds['actions'][i], 'rewards': 5.0 + i,
                          'masks': ds['masks'][i], 'next_observations': ds['next_observations'][i]}, replay=True)
    rng = np.random.default_rng(10)
    ia, ib = rng.integers(0, len(ds['observations']), size=B // 2), rng.integers(0, n, size=B // 2)
    rb = {'observations': ds['observations'][:n], 'actions': ds['actions'][:n], 'rewards': (5.0 + np.arange(n)).astype(np.float32),
          'masks': ds['masks'][:n], 'next_observations': ds['next_observations'][:n]}
    batch = {k: np.concatenate([ds[k][ia], rb[k][ib]]) for k in rb}
    for _ in range(2):
        a.update_balanced(B, idxs=(ia, ib), noise=noise)
        b.update(batch, noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def test_update_balanced_engine_draws_take_rows_from_both_sources():
    """Replay rows carry reward 100: the critic's targets see them only if the replay half is drawn from the ring."""
    cfg, ds, _, _ = _problem(seed=11)
    B = cfg['batch_size']
    a = _agent(cfg, ds)
    a.upload_dataset(ds)
    _ring(a, ds, 16, 100.0)
    _, info = a.update_balanced(B, want_info=True)
    info = info.to_dict()
    # q ~ 0 at init: the loss is about the mean squared target, half the rows near 100^2, half near <= 1
    assert 0.3 * 100.0 ** 2 / 2 < info['critic/critic_loss'] < 0.7 * 100.0 ** 2, info['critic/critic_loss']
    assert a.replay_size()[0] == 16


def test_aql_and_graph_updates_bitwise_over_20_steps():
    import torch
    cfg, ds, _, _ = _problem(seed=5)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for i in range(20):
        a.update_from_dataset()
        b.update_from_dataset(stream=s.cuda_stream)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    a2 = _agent(cfg, ds)   # determinism: same seed, same device-drawn rows and noise
    a2.upload_dataset(ds)
    for i in range(20):
        a2.update_from_dataset()
    a2.synchronize()
    _same_state(a, a2)


@pytest.mark.parametrize('tanh_squash', [True, False])
def test_sample_actions_matches_restatement(tanh_squash):
    cfg, _, batch, _ = _problem(seed=6, tanh_squash=tanh_squash)
    params = _randomized(SO.init_params(8, OD, AD, cfg), 8)
    a = _agent(cfg, batch, params=params)
    ref = SO.OracleSAC(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(6)
    n = 7
    obs = batch['observations'][:n]
    z = rng.standard_normal((n, AD)).astype(np.float32)
    for temp in (1.0, 0.3, 0.0):
        many = a.sample_actions(obs, noises=z, temperature=temp)
        assert many.shape == (n, AD) and np.abs(many).max() <= 1.0
        np.testing.assert_allclose(many, ref.sample_actions(obs, z, temp), atol=2e-5, err_msg=str(temp))
        for i in range(n):
            np.testing.assert_array_equal(many[i], a.sample_actions(obs[i], noises=z[i], temperature=temp))
    drawn = a.sample_actions(obs, seed=123)
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=123))
    assert np.abs(drawn).max() <= 1.0
    # fql_sample_actions == fql_sac_sample_actions at temperature 1
    out = np.empty((n, AD), np.float32)
    obs32, z32 = np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(z)
    assert a._lib.fql_sample_actions(a._h, obs32.ctypes.data, n, z32.ctypes.data, 0, out.ctypes.data, None) == 0
    np.testing.assert_array_equal(out, a.sample_actions(obs, noises=z, temperature=1.0))


def test_sample_actions_across_the_4096_row_chunk_boundary():
    cfg, _, batch, _ = _problem(seed=12)
    params = _randomized(SO.init_params(8, OD, AD, cfg), 12)
    a = _agent(cfg, batch, params=params)
    ref = SO.OracleSAC(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(12)
    n = 4096 + 37
    obs = rng.standard_normal((n, OD)).astype(np.float32)
    z = rng.standard_normal((n, AD)).astype(np.float32)
    got = a.sample_actions(obs, noises=z)
    np.testing.assert_allclose(got, ref.sample_actions(obs, z), atol=2e-5)
    for i in (4095, 4096, n - 1):
        np.testing.assert_array_equal(got[i], a.sample_actions(obs[i], noises=z[i]))
    drawn = a.sample_actions(obs, seed=5)
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=5))
    assert np.abs(drawn).max() <= 1.0


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg, ds, batch, noise = _problem(seed=7)
    a = _agent(cfg, batch)
    a.update(batch, noise=noise)
    a.update(batch, noise=SO.make_noise(cfg['batch_size'], AD, 70))
    a.synchronize()
    assert float(leaf_dict(a.get_params())['modules_alpha/log_value']) != 0.0
    assert float(leaf_dict(a.get_opt_state()['nu'])['modules_alpha/log_value']) > 0.0
    checkpoint.save_agent(a, str(tmp_path), 2)
    b = _agent(cfg, batch, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 2)
    _same_state(a, b)
    sd = checkpoint.to_state_dict(a)
    assert set(sd['network']['params']) == {'modules_actor', 'modules_alpha', 'modules_critic', 'modules_target_critic'}
    assert np.shape(sd['network']['params']['modules_alpha']['log_value']) == ()


def test_fql_ifql_rebrac_sac_interleaved_end_where_they_end_alone():
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, _ = _problem(seed=8)
    B = cfg['batch_size']
    fcfg = make_cfg((64,) * 4, batch_size=B)
    icfg = fql_amd.ifql.get_config()
    icfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    rcfg = fql_amd.rebrac.get_config()
    rcfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)

    def make():
        f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], fcfg)
        i = fql_amd.IFQLAgent.create(2, batch['observations'][:1], batch['actions'][:1], icfg)
        r = fql_amd.ReBRACAgent.create(4, batch['observations'][:1], batch['actions'][:1], rcfg)
        s = _agent(cfg, batch)
        for x in (f, i, r, s):
            x.upload_dataset(ds)
        return f, i, r, s

    def step(x, k):
        if isinstance(x, fql_amd.ReBRACAgent):
            x.update_from_dataset(full_update=k % 2 == 0)
        else:
            x.update_from_dataset()

    alone = make()
    for x in alone:
        for k in range(6):
            step(x, k)
    mixed = make()
    for k in range(6):
        for x in (mixed[3], mixed[0], mixed[2], mixed[1]):
            step(x, k)
    for x in alone + mixed:
        x.synchronize()
    for x, y in zip(alone, mixed):
        _same_state(x, y)


def test_stats_agree():
    cfg, _, batch, _ = _problem()
    a = _agent(cfg, batch)
    la, ma = a.sac_stats()
    assert la > 0 and ma > 0
    assert a.stats()['launches_per_update'] == la and a.stats()['macs_per_update'] == ma
    # by the accounting of fql_rebrac_stats: actor on 2B rows, target pair, critic pair fwd + bwd, the pair on [obs | a] fwd + input
    # gradient, the actor's backward on B rows
    cr = (OD + AD) * 64 + 3 * 64 * 64 + 64
    ac = OD * 64 + 3 * 64 * 64 + 64 * 2 * AD
    fc, fa = (OD + AD) * 64, OD * 64
    want = 2 * ac + 2 * cr + 2 * cr + 2 * (2 * cr - fc) + 2 * cr + 2 * cr + (2 * ac - fa)
    assert ma == want * cfg['batch_size']


def test_fourteen_infos():
    from fql_amd import _cabi
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, noise = _problem(seed=13)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    assert lib.fql_num_info(h) == 14 and lib.fql_handle_info_name(h, 14) is None
    assert [lib.fql_handle_info_name(h, i).decode() for i in range(14)] == list(SO.INFO_KEYS)
    _, lazy = a.update(batch, noise=noise)
    assert tuple(lazy) == SO.INFO_KEYS and len(lazy) == 14
    vals = lazy.to_dict()
    buf = (C.c_float * 14)()
    assert lib.fql_read_info_n(h, buf, 14) == 0
    assert [float(x) for x in buf] == [vals[k] for k in SO.INFO_KEYS]
    assert lib.fql_read_info_n(h, buf, 13) == _cabi.FQL_E_INVALID
    t = C.c_uint64()
    assert lib.fql_info_enqueue(h, None, C.byref(t)) == 0
    b15 = (C.c_float * 15)(*([-7.0] * 15))
    assert lib.fql_info_wait_n(h, t.value, b15, 15) == 0
    assert [float(x) for x in b15[:14]] == [vals[k] for k in SO.INFO_KEYS] and b15[14] == -7.0
    assert lib.fql_info_wait_n(h, t.value, buf, 13) == _cabi.FQL_E_INVALID
    b13 = (C.c_float * 13)()
    assert lib.fql_read_info(h, b13) == _cabi.FQL_E_STATE
    assert lib.fql_info_wait(h, t.value, b13) == _cabi.FQL_E_STATE
    assert a.read_info() == vals
    info14 = (C.c_float * 14)()
    obs, act, rew, mask, nobs = (np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                                 ('observations', 'actions', 'rewards', 'masks', 'next_observations'))
    assert lib.fql_sac_update(h, obs.ctypes.data, act.ctypes.data, rew.ctypes.data, mask.ctypes.data, nobs.ctypes.data,
                              cfg['batch_size'], None, info14, None) == 0
    assert list(info14) == list(a.read_info().values())
    # an FQL handle: the _n calls are the 13-float ones, the 13-float calls unchanged
    f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], make_cfg((64,) * 4, batch_size=cfg['batch_size']))
    f.update(batch, want_info=False)
    assert lib.fql_num_info(f._h) == 13
    assert lib.fql_read_info(f._h, b13) == 0
    bn = (C.c_float * 14)(*([-7.0] * 14))
    assert lib.fql_read_info_n(f._h, bn, 14) == 0
    assert list(bn[:13]) == list(b13) and bn[13] == -7.0
    assert lib.fql_read_info_n(f._h, bn, 12) == _cabi.FQL_E_INVALID
    assert lib.fql_info_enqueue(f._h, None, C.byref(t)) == 0
    assert lib.fql_info_wait_n(f._h, t.value, bn, 13) == 0 and list(bn[:13]) == list(b13)
    assert lib.fql_info_wait(f._h, t.value, b13) == 0


def test_refusals_return_documented_codes():
    from fql_amd import _cabi
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, noise = _problem(seed=9)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    B = cfg['batch_size']
    nz = _cabi.FqlNoise()
    st = C.c_size_t * 2
    assert lib.fql_grad_buckets(h, st(), st()) == _cabi.FQL_E_STATE
    obs, act, rew, mask, nobs = (np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                                 ('observations', 'actions', 'rewards', 'masks', 'next_observations'))
    bp = [x.ctypes.data for x in (obs, act, rew, mask, nobs)]
    loss, info = C.c_float(), (C.c_float * 11)()
    assert lib.fql_update(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_total_loss(h, *bp, B, None, C.byref(loss), info, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin(h, *bp, B, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin_split(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_end(h, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_end_split(h, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin(h, None, B, 0, 0, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin_split(h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    a.upload_dataset(ds)
    assert lib.fql_update_from_dataset(h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    a.create_replay_buffer(8)   # the replay ring is available on a SAC handle ...
    a.add_transition({k: ds[k][0] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')}, replay=True)
    assert a.replay_size() == (1, 1)
    assert lib.fql_update_balanced(h, None, None, None, B, None, None, None) == _cabi.FQL_E_STATE   # ... FQL's balanced step is not
    frames = np.zeros((64, 32, 32, 3), np.uint8)
    assert lib.fql_dataset_upload_frames(h, 64, frames.ctypes.data, frames.ctypes.data, ds['actions'][:64].ctypes.data,
                                         ds['rewards'][:64].ctypes.data, ds['masks'][:64].ctypes.data, ds['masks'][:64].ctypes.data,
                                         1, 0.0) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_frames(h, None, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_flow_actions(h, obs.ctypes.data, act.ctypes.data, 4, act.ctypes.data, None) == _cabi.FQL_E_STATE
    for bad in ('x0', 't', 'z'):   # the C ABI reads only eps1 and eps2 of fql_noise
        other = np.zeros((B, AD), np.float32)
        fields = {'eps1': noise['eps1'].ctypes.data, 'x0': None, 't': None, 'z': None, 'eps2': noise['eps2'].ctypes.data}
        fields[bad] = other.ctypes.data
        nzb = _cabi.FqlNoise(*[fields[k] for k in ('eps1', 'x0', 't', 'z', 'eps2')])
        assert lib.fql_sac_update(h, *bp, B, C.byref(nzb), None, None) == _cabi.FQL_E_INVALID, bad
    keys = np.zeros(10, dtype=np.uint32)
    assert lib.fql_noise_from_jax_keys(h, keys.ctypes.data, 0, B, C.byref(nz), None) == _cabi.FQL_E_STATE
    grp = C.c_void_p()
    assert lib.fql_group_create((C.c_void_p * 1)(h), 1, C.byref(grp)) == _cabi.FQL_E_STATE
    # the fql_sac_* calls on an FQL handle
    f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], make_cfg((64,) * 4, batch_size=B))
    assert lib.fql_sac_update(f._h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_sac_update_from_dataset(f._h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_sac_update_balanced(f._h, None, None, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_sac_total_loss(f._h, *bp, B, None, C.byref(loss), info, None) == _cabi.FQL_E_STATE
    out = np.empty((1, AD), np.float32)
    assert lib.fql_sac_sample_actions(f._h, obs.ctypes.data, 1, None, 0, 1.0, out.ctypes.data, None) == _cabi.FQL_E_STATE
    la = C.c_int64()
    assert lib.fql_sac_stats(f._h, C.byref(la), None) == _cabi.FQL_E_STATE
    # create-time refusals
    c = _cabi.FqlConfig()
    lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim = OD, AD
    sc = _cabi.FqlSacConfig()
    lib.fql_sac_default_config(C.byref(sc))
    hh = C.c_void_p()
    c.precision = 2
    assert lib.fql_sac_create(C.byref(c), C.byref(sc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    c.precision = 0
    sc.state_dependent_std = 0
    assert lib.fql_sac_create(C.byref(c), C.byref(sc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    sc.state_dependent_std = 1
    c.encoder, c.img_h, c.img_w, c.img_c = 1, 32, 32, 3
    assert lib.fql_sac_create(C.byref(c), C.byref(sc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID


def test_rlpd_loop_against_restatement():
    """main.py:217-259 with --offline_steps=0 --balanced_sampling=1: an empty ring; per step sample_actions on one observation, a toy
    environment step, add_transition(replay=True) and update_balanced with explicit rows and noise.  The restatement replays the
    recorded transitions, rows and noise."""
    cfg, ds, _, _ = _problem(B=32, seed=14)
    B = cfg['batch_size']
    a = _agent(cfg, ds)
    a.upload_dataset(ds)
    a.create_replay_buffer(1000)
    ref = SO.OracleSAC(a.get_params(), dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(14)
    W = rng.standard_normal((AD, OD)).astype(np.float32) * 0.1
    ob = rng.standard_normal(OD).astype(np.float32)
    ring = {k: [] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')}
    for step in range(50):
        z = rng.standard_normal(AD).astype(np.float32)
        action = a.sample_actions(ob, noises=z)
        np.testing.assert_allclose(action, ref.sample_actions(ob[None], z[None])[0], atol=1e-3)
        nob = (0.9 * ob + action @ W).astype(np.float32)                  # toy dynamics
        r = float(-np.square(action).sum())
        m = 0.0 if step % 17 == 16 else 1.0
        t = {'observations': ob, 'actions': action, 'rewards': r, 'masks': m, 'next_observations': nob}
        a.add_transition(t, replay=True)
        for k in ring:
            ring[k].append(np.asarray(t[k], np.float32))
        n = len(ring['rewards'])
        ia, ib = rng.integers(0, len(ds['observations']), size=B // 2), rng.integers(0, n, size=B // 2)
        noise = SO.make_noise(B, AD, 500 + step)
        a.update_balanced(B, idxs=(ia, ib), noise=noise)
        rb = {k: np.stack(v) for k, v in ring.items()}
        ref.update({k: np.concatenate([ds[k][ia], rb[k][ib]]) for k in rb}, noise)
        ob = nob if m else rng.standard_normal(OD).astype(np.float32)
    a.synchronize()
    assert a.replay_size()[0] == 50
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


@pytest.mark.parametrize('kind', ['ifql', 'rebrac'])
def test_info_n_calls_write_exactly_the_handles_count(kind):
    """fql_read_info_n / fql_info_wait_n write fql_num_info(h) floats and nothing past them: 12 on IFQL and ReBRAC handles."""
    import fql_amd
    from fql_amd import _cabi
    cfg, ds, batch, _ = _problem(seed=15)
    mcfg = getattr(fql_amd, kind).get_config()
    mcfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=cfg['batch_size'])
    cls = fql_amd.IFQLAgent if kind == 'ifql' else fql_amd.ReBRACAgent
    a = cls.create(1, batch['observations'][:1], batch['actions'][:1], mcfg)
    a.upload_dataset(ds)
    a.update_from_dataset()
    lib, h = a._lib, a._h
    assert lib.fql_num_info(h) == 12
    buf = (C.c_float * 13)(*([-7.0] * 13))   # 12 floats + a guard
    assert lib.fql_read_info_n(h, buf, 12) == 0
    assert buf[12] == -7.0 and all(np.isfinite(buf[:12]))
    want = list(buf[:12])
    assert lib.fql_read_info_n(h, buf, 11) == _cabi.FQL_E_INVALID
    t = C.c_uint64()
    assert lib.fql_info_enqueue(h, None, C.byref(t)) == 0
    buf2 = (C.c_float * 13)(*([-7.0] * 13))
    assert lib.fql_info_wait_n(h, t.value, buf2, 12) == 0
    assert list(buf2[:12]) == want and buf2[12] == -7.0
    assert lib.fql_info_wait_n(h, t.value, buf2, 11) == _cabi.FQL_E_INVALID


def test_total_loss_leaves_the_last_updates_infos():
    cfg, _, batch, noise = _problem(seed=16)
    a = _agent(cfg, batch)
    a.update(batch, noise=noise, want_info=False)
    before = a.read_info()
    a.total_loss(batch, noise=SO.make_noise(cfg['batch_size'], AD, 160))
    assert a.read_info() == before
