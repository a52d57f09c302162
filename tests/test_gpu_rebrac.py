"""GPU: the ReBRAC agent (agents/rebrac.py) on the engine against the fp64 restatement in tests/rebrac_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import rebrac_oracle as RO
from tests.util import assert_info_close, leaf_dict, sync_restatement

pytestmark = pytest.mark.gpu
OD, AD = 29, 8


def _cfg(H, B, **kw):
    import fql_amd
    cfg = fql_amd.rebrac.get_config()
    cfg.update(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=B, alpha_actor=0.5, alpha_critic=0.3)
    cfg.update(kw)
    return cfg


def _problem(H=64, B=64, seed=0, **kw):
    ds = O.make_synthetic_dataset(max(4 * B, 64), OD, AD, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    return _cfg(H, B, **kw), ds, RO.make_batch(ds, idx), RO.make_noise(B, AD, seed + 2)


def _randomized(params, seed, scale=0.1):
    """Biases / LN parameters away from init, a larger mean_net (so tanh and the clips bite), targets != online."""
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, dtype=np.float64), params)
    for path, leaf in O.tree_leaves_with_path(out):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += scale * rng.standard_normal(leaf.shape)
        if path.endswith('mean_net/kernel'):
            leaf *= 30.0
    for m in ('actor', 'critic'):
        out[f'modules_target_{m}'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), out[f'modules_{m}'])
    return O.tree_map(lambda a: a.astype(np.float32), out)


def _agent(cfg, batch, seed=3, params=None):
    import fql_amd
    a = fql_amd.ReBRACAgent.create(seed, batch['observations'][:1], batch['actions'][:1], cfg)
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
    want = {p: v.shape for p, v in O.tree_leaves_with_path(RO.init_params(0, OD, AD, cfg))}
    assert dict(a.leaves()) == want
    p = leaf_dict(a.get_params())
    assert p['modules_actor/mean_net/kernel'].shape == (64, AD)
    assert 'modules_actor/actor_net/Dense_3/kernel' in p and 'modules_actor/actor_net/Dense_4/kernel' not in p
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.endswith('/kernel'):
            s = cfg['actor_fc_scale'] if 'mean_net' in k else 1.0
            lim = np.sqrt(6.0 * s / (v.shape[-2] + v.shape[-1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
        if k.startswith('modules_target_'):
            np.testing.assert_array_equal(v, p[k.replace('modules_target_', 'modules_')])


def _check_step(a, ref, batch, noise, full, cfg, pre):
    _, _, g_ref = ref._losses(batch, noise, want_grads=True, full_update=full)
    mu0 = leaf_dict(a.get_opt_state()['mu'])
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, full_update=full, noise=noise)
    info = info.to_dict()
    keys = RO.INFO_KEYS if full else RO.CRITIC_INFO_KEYS
    assert tuple(info) == keys
    _, want = ref.update(batch, noise, full_update=full)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=keys)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    worst = (0.0, None)
    for p, g in leaf_dict(g_ref).items():
        if p.startswith('modules_target_'):
            if full:   # Polyak from the PRE-step online module
                np.testing.assert_allclose(new[p], 0.005 * pre[p.replace('target_', '')] + 0.995 * pre[p], atol=1e-6, err_msg=p)
            else:
                np.testing.assert_array_equal(new[p], pre[p], err_msg=p)
            continue
        tol = 2e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9   # (mu0's fp32 decay rounds at ~1e-7 relative)
        if np.abs(g).max() > 0:
            worst = max(worst, (float(np.abs((mu[p] - np.float32(0.9) * mu0[p]) / 0.1 - g).max() / np.abs(g).max()), p))
        np.testing.assert_allclose((mu[p] - np.float32(0.9) * mu0[p]) / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
        d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))   # this step's increment (an earlier ill-conditioned step's difference stays)
        # a parameter's step is well conditioned where this step's gradient AND the first moment stand clear of the fp32 error
        # (after two steps mu can cancel: then lr mu / sqrt(nu) amplifies it)
        stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
        assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p
    return worst


@pytest.mark.parametrize('H,B', [(64, 64), (512, 256)])
def test_full_then_critic_only_update_match_fp64_restatement(H, B):
    """One full step, then a critic-only step right after it: the second catches stale actor gradients and an unwanted Polyak step."""
    cfg, _, batch, noise = _problem(H, B, seed=1)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 5)
    a.set_params(params)
    ref = RO.OracleReBRAC(params, dict(cfg), OD, AD, np.float64)
    _check_step(a, ref, batch, noise, True, cfg, leaf_dict(params))
    pre = leaf_dict(a.get_params())
    noise2 = RO.make_noise(B, AD, 77)
    _check_step(a, ref, batch, noise2, False, cfg, pre)
    opt = a.get_opt_state()
    assert opt['count'] == 2 and opt['step'] == 3
    after = leaf_dict(a.get_params())
    moved = [k for k in after if k.startswith('modules_actor/') and np.any(after[k] != pre[k])]
    assert moved, 'a critic-only step moves the actor through Adam momentum'


def _check_total_loss(a, ref, params, batch, noise):
    """total_loss of both step kinds on both sides (infos, the loss); no parameter or optimizer state changes."""
    for full in (True, False):
        loss, info = a.total_loss(batch, noise=noise, full_update=full)
        want_loss, want = ref.total_loss(batch, noise, full_update=full)
        keys = RO.INFO_KEYS[:9] if full else RO.INFO_KEYS[:4]
        assert tuple(info) == keys
        assert_info_close(info, want, keys=keys)
        assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0


def test_total_loss_matches_and_changes_no_state():
    cfg, _, batch, noise = _problem(seed=2)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 6)
    a.set_params(params)
    ref = RO.OracleReBRAC(params, dict(cfg), OD, AD, np.float64)
    _check_total_loss(a, ref, params, batch, noise)


def test_trajectory_100_updates_on_actor_freq_schedule():
    cfg, ds, _, _ = _problem(seed=3)
    rng = np.random.default_rng(9)
    a = _agent(cfg, {'observations': ds['observations'][:1], 'actions': ds['actions'][:1]})
    ref = RO.OracleReBRAC(a.get_params(), dict(cfg), OD, AD, np.float64)
    B = cfg['batch_size']
    for i in range(100):
        full = i % cfg['actor_freq'] == 0
        batch = RO.make_batch(ds, rng.integers(0, len(ds['observations']), size=B))
        noise = {'eps1': rng.standard_normal((B, AD)).astype(np.float32)}
        a.update(batch, full_update=full, noise=noise, want_info=False)
        ref.update(batch, noise, full_update=full)
    _, info = a.update(batch, full_update=True, noise=noise)
    _, want = ref.update(batch, noise, full_update=True)
    info = info.to_dict()
    for k in ('critic/critic_loss', 'critic/q_mean', 'actor/actor_loss', 'actor/bc_loss', 'actor/mse'):
        assert abs(info[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, info[k], want[k])
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


def test_update_from_dataset_explicit_rows_equals_update():
    """Rows include size - 1 (its next_actions clamp to itself) and an episode's last row (the next episode's first action)."""
    cfg, ds, _, noise = _problem(seed=4)
    B, n = cfg['batch_size'], len(ds['observations'])
    idx = np.random.default_rng(4).integers(0, n, size=B)
    ends = np.nonzero(ds['terminals'] > 0)[0]
    idx[0], idx[1] = n - 1, ends[0] if len(ends) else n - 2
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    a.upload_dataset(ds)
    for full in (True, False, True):
        a.update_from_dataset(idxs=idx, noise=noise, full_update=full)
        b.update(RO.make_batch(ds, idx), full_update=full, noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def test_aql_and_graph_updates_bitwise_over_20_mixed_steps():
    import torch
    cfg, ds, _, _ = _problem(seed=5)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for i in range(20):
        a.update_from_dataset(full_update=i % 2 == 0)
        b.update_from_dataset(stream=s.cuda_stream, full_update=i % 2 == 0)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    a2 = _agent(cfg, ds)   # determinism: same seed, same device-drawn rows and noise
    a2.upload_dataset(ds)
    for i in range(20):
        a2.update_from_dataset(full_update=i % 2 == 0)
    a2.synchronize()
    _same_state(a, a2)


@pytest.mark.parametrize('tanh_squash', [True, False])
def test_sample_actions_matches_restatement(tanh_squash):
    cfg, _, batch, _ = _problem(seed=6, tanh_squash=tanh_squash)
    params = _randomized(RO.init_params(8, OD, AD, cfg), 8)
    a = _agent(cfg, batch, params=params)
    ref = RO.OracleReBRAC(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(6)
    n = 7
    obs = batch['observations'][:n]
    z = (3.0 * rng.standard_normal((n, AD))).astype(np.float32)   # past the noise clip for some entries
    for temp in (1.0, 0.3, 0.0):
        many = a.sample_actions(obs, noises=z, temperature=temp)
        assert many.shape == (n, AD) and np.abs(many).max() <= 1.0
        np.testing.assert_allclose(many, ref.sample_actions(obs, z, temp), atol=2e-5, err_msg=str(temp))
        for i in range(n):
            np.testing.assert_array_equal(many[i], a.sample_actions(obs[i], noises=z[i], temperature=temp))
    drawn = a.sample_actions(obs, seed=123)
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=123))
    assert np.abs(drawn).max() <= 1.0


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg, ds, batch, noise = _problem(seed=7)
    a = _agent(cfg, batch)
    a.update(batch, noise=noise)
    a.update(batch, full_update=False, noise=noise)
    a.synchronize()
    checkpoint.save_agent(a, str(tmp_path), 2)
    b = _agent(cfg, batch, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 2)
    _same_state(a, b)
    sd = checkpoint.to_state_dict(a)
    assert set(sd['network']['params']) == {'modules_actor', 'modules_critic', 'modules_target_actor', 'modules_target_critic'}


def test_fql_ifql_rebrac_interleaved_end_where_they_end_alone():
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, _ = _problem(seed=8)
    fcfg = make_cfg((64,) * 4, batch_size=cfg['batch_size'])
    icfg = fql_amd.ifql.get_config()
    icfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=cfg['batch_size'])

    def make():
        f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], fcfg)
        i = fql_amd.IFQLAgent.create(2, batch['observations'][:1], batch['actions'][:1], icfg)
        r = _agent(cfg, batch)
        for x in (f, i, r):
            x.upload_dataset(ds)
        return f, i, r

    alone = make()
    for k in range(6):
        alone[0].update_from_dataset()
    for k in range(6):
        alone[1].update_from_dataset()
    for k in range(6):
        alone[2].update_from_dataset(full_update=k % 2 == 0)
    mixed = make()
    for k in range(6):
        mixed[0].update_from_dataset()
        mixed[2].update_from_dataset(full_update=k % 2 == 0)
        mixed[1].update_from_dataset()
    for x in alone + mixed:
        x.synchronize()
    for x, y in zip(alone, mixed):
        _same_state(x, y)


def test_stats_count_both_programs():
    cfg, _, batch, _ = _problem()
    a = _agent(cfg, batch)
    lf, mf = a.rebrac_stats(True)
    lc, mc = a.rebrac_stats(False)
    assert lf > lc > 0 and mf > mc > 0
    assert a.stats()['launches_per_update'] == lf and a.stats()['macs_per_update'] == mf


def test_refusals_return_documented_codes():
    from fql_amd import _cabi
    cfg, ds, batch, noise = _problem(seed=9)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    B = cfg['batch_size']
    nz = _cabi.FqlNoise()
    assert lib.fql_num_info(h) == 12 and lib.fql_handle_info_name(h, 12) is None
    assert [lib.fql_handle_info_name(h, i).decode() for i in range(12)] == list(RO.INFO_KEYS)
    st = C.c_size_t * 2
    assert lib.fql_grad_buckets(h, st(), st()) == _cabi.FQL_E_STATE
    obs, act, rew, mask, nobs, nact = (np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                                       ('observations', 'actions', 'rewards', 'masks', 'next_observations', 'next_actions'))
    bp = [x.ctypes.data for x in (obs, act, rew, mask, nobs)]
    loss, info = C.c_float(), (C.c_float * 10)()
    assert lib.fql_update(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_total_loss(h, *bp, B, None, C.byref(loss), info, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin(h, *bp, B, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin_split(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_end(h, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin(h, None, B, 0, 0, None, None) == _cabi.FQL_E_STATE
    a.upload_dataset(ds)
    assert lib.fql_update_from_dataset(h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_balanced(h, None, None, None, B, None, None, None) == _cabi.FQL_E_STATE
    frames = np.zeros((64, 32, 32, 3), np.uint8)
    assert lib.fql_dataset_upload_frames(h, 64, frames.ctypes.data, frames.ctypes.data, ds['actions'][:64].ctypes.data,
                                         ds['rewards'][:64].ctypes.data, ds['masks'][:64].ctypes.data, ds['masks'][:64].ctypes.data,
                                         1, 0.0) == _cabi.FQL_E_STATE
    assert lib.fql_flow_actions(h, obs.ctypes.data, act.ctypes.data, 4, act.ctypes.data, None) == _cabi.FQL_E_STATE
    for bad in ('x0', 't', 'z', 'eps2'):   # the C ABI reads only eps1 of fql_noise
        other = np.zeros((B, AD), np.float32)
        fields = {'eps1': noise['eps1'].ctypes.data, 'x0': None, 't': None, 'z': None, 'eps2': None}
        fields[bad] = other.ctypes.data
        nzb = _cabi.FqlNoise(*[fields[k] for k in ('eps1', 'x0', 't', 'z', 'eps2')])
        assert lib.fql_rebrac_update(h, *bp, nact.ctypes.data, B, C.byref(nzb), 1, None, None) == _cabi.FQL_E_INVALID, bad
    assert lib.fql_rebrac_update(h, *bp, None, B, None, 1, None, None) == _cabi.FQL_E_INVALID   # next_actions missing
    assert lib.fql_replay_create(h, 16) == _cabi.FQL_E_STATE
    keys = np.zeros(10, dtype=np.uint32)
    assert lib.fql_noise_from_jax_keys(h, keys.ctypes.data, 0, B, C.byref(nz), None) == _cabi.FQL_E_STATE
    grp = C.c_void_p()
    assert lib.fql_group_create((C.c_void_p * 1)(h), 1, C.byref(grp)) == _cabi.FQL_E_STATE
    # the fql_rebrac_* calls on an FQL handle
    import fql_amd
    from tests.util import make_cfg
    f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], make_cfg((64,) * 4, batch_size=B))
    assert lib.fql_rebrac_update(f._h, *bp, nact.ctypes.data, B, None, 1, None, None) == _cabi.FQL_E_STATE
    la = C.c_int64()
    assert lib.fql_rebrac_stats(f._h, 1, C.byref(la), None) == _cabi.FQL_E_STATE
    c = _cabi.FqlConfig()
    lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim, c.precision = OD, AD, 2
    rc = _cabi.FqlRebracConfig()
    lib.fql_rebrac_default_config(C.byref(rc))
    out = C.c_void_p()
    assert lib.fql_rebrac_create(C.byref(c), C.byref(rc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    c.precision, c.encoder, c.img_h, c.img_w, c.img_c = 0, 1, 64, 64, 3
    assert lib.fql_rebrac_create(C.byref(c), C.byref(rc), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    a.update(batch, noise=noise)   # the handle still works after the refusals
    a.update(batch, full_update=False, noise=noise)
    a.synchronize()


# ---- shapes, configs, chunked sampling and batch-size switches -------------------------------------------------------------------------

SHAPE_CASES = [
    # od, ad, B, actor hidden, value hidden, cfg overrides (on top of _cfg's alpha_actor 0.5, alpha_critic 0.3)
    pytest.param(7, 3, 16, (32,) * 4, (32,) * 4, {}, id='small'),
    pytest.param(29, 8, 32, (64, 64), (48, 80, 64), {}, id='ragged_depths'),
    pytest.param(11, 5, 48, (64,) * 4, (64,) * 4, dict(tanh_squash=False), id='no_tanh'),
    pytest.param(17, 6, 64, (64,) * 4, (64,) * 4, dict(actor_layer_norm=True, layer_norm=False), id='actor_ln_no_critic_ln'),
    pytest.param(69, 21, 256, (512,) * 4, (512,) * 4, dict(alpha_actor=0.01, alpha_critic=0.01, discount=0.995), id='humanoidmaze'),
    pytest.param(29, 16, 256, (512,) * 4, (512,) * 4, {}, id='act16'),               # OP_DGRAD0 with a full 16-column action block
    # the reference's default alphas; the hidden layers on fql_side_big_kernel's 64-row tiles.  in_p = round64(40 + 4) = 64 and 40 + 16 <= 64:
    # OP_DGRAD0 with 4 live columns, as in IQL's table (tests/test_gpu_rebrac_paths.py asserts it from the plan; the generic first-layer dgrad
    # at H 512 with act <= 16 is that file's obs50)
    pytest.param(40, 4, 1024, (512,) * 4, (512,) * 4, dict(alpha_actor=0.0, alpha_critic=0.0), id='b1024'),
]


def _problem_at(od, ad, B, actor, value, seed, **kw):
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    cfg = _cfg(64, B, actor_hidden_dims=tuple(actor), value_hidden_dims=tuple(value), **kw)
    return cfg, ds, RO.make_batch(ds, idx), RO.make_noise(B, ad, seed + 2)


@pytest.mark.parametrize('od,ad,B,actor,value,kw', SHAPE_CASES)
def test_total_loss_and_both_step_kinds_across_shapes_and_configs(od, ad, B, actor, value, kw):
    """total_loss, a full step, then a critic-only step from the engine's post-step state (sync_restatement)."""
    cfg, _, batch, noise = _problem_at(od, ad, B, actor, value, seed=21, **kw)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 22)
    a.set_params(params)
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    _check_total_loss(a, ref, params, batch, noise)
    w_full = _check_step(a, ref, batch, noise, True, cfg, leaf_dict(params))
    assert a.get_opt_state()['count'] == 1
    sync_restatement(ref, a)
    w_crit = _check_step(a, ref, batch, RO.make_noise(B, ad, 23), False, cfg, leaf_dict(a.get_params()))
    print(f'worst relative gradient error: full step {w_full[0]:.3e} ({w_full[1]}), critic-only step {w_crit[0]:.3e} ({w_crit[1]})')


def test_sample_actions_across_the_row_chunk():
    """n = 4097 rows (one past the 4096-row chunk) with explicit noises at temperatures 1 and 0.3, then the seeded draw's chunk keying."""
    od, ad, n = 69, 21, 4097
    cfg, _, batch, _ = _problem_at(od, ad, 64, (512,) * 4, (512,) * 4, seed=24)
    params = _randomized(RO.init_params(9, od, ad, cfg), 9, scale=0.05)
    a = _agent(cfg, batch, params=params)
    ref = RO.OracleReBRAC(params, dict(cfg), od, ad, np.float64)
    rng = np.random.default_rng(24)
    obs = rng.standard_normal((n, od)).astype(np.float32)
    z = (3.0 * rng.standard_normal((n, ad))).astype(np.float32)
    for temp in (1.0, 0.3):
        got = a.sample_actions(obs, noises=z, temperature=temp)
        assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
        np.testing.assert_allclose(got, ref.sample_actions(obs, z, temp), atol=2e-5, err_msg=str(temp))
    same = np.repeat(obs[:1], n, axis=0)
    drawn = a.sample_actions(same, seed=5)
    assert np.abs(drawn).max() <= 1.0
    assert np.abs(drawn[4096] - drawn[0]).max() > 1e-3   # the second chunk's first row draws its own noise
    np.testing.assert_array_equal(drawn[:4096], a.sample_actions(same[:4096], seed=5))


def test_batch_size_switches_track_restatement():
    """B = 64, 32, 64: each switch rebuilds the workspace and both programs; every step is compared after the rebuild, from the engine's
    own pre-step state (sync_restatement).  Then update_from_dataset after a switch equals update on the same rows, bitwise."""
    cfg, ds, batch, _ = _problem(seed=25)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 26)
    a.set_params(params)
    ref = RO.OracleReBRAC(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(25)
    steps = []
    for i, (B, full) in enumerate(((64, True), (32, False), (64, True))):
        idx = rng.integers(0, len(ds['observations']), size=B)
        noise = {'eps1': rng.standard_normal((B, AD)).astype(np.float32)}
        steps.append((idx, noise, full))
        print('step at B', B)
        assert a.get_opt_state()['count'] == i
        sync_restatement(ref, a)
        _check_step(a, ref, RO.make_batch(ds, idx), noise, full, cfg, leaf_dict(a.get_params()))
    opt = a.get_opt_state()
    assert opt['count'] == 3 and opt['step'] == 4
    x, y = _agent(cfg, ds, params=params), _agent(cfg, ds, params=params)
    x.upload_dataset(ds)
    for idx, noise, full in steps:
        x.update_from_dataset(batch_size=len(idx), idxs=idx, noise=noise, full_update=full)
        y.update(RO.make_batch(ds, idx), full_update=full, noise=noise)
    x.synchronize(); y.synchronize()
    _same_state(x, y)
    assert x.read_info() == y.read_info()
