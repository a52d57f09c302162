"""GPU: the IFQL agent (agents/ifql.py) on the engine against the fp64 restatement in tests/ifql_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import ifql_oracle as IO
from tests.ifql_cases import best_of_n as _best_of_n
from tests.util import assert_info_close, leaf_dict, make_problem, randomize_params, sync_restatement

pytestmark = pytest.mark.gpu
OD, AD = 29, 8


def _cfg(H, B, **kw):
    import fql_amd
    cfg = fql_amd.ifql.get_config()
    cfg.update(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=B)
    cfg.update(kw)
    return cfg


def _problem(H=64, B=64, seed=0):
    _, ds, batch, noise = make_problem(OD, AD, B, (H,) * 4, seed=seed)
    return _cfg(H, B), ds, batch, {'x0': noise['x0'], 't': noise['t']}


def _randomized(params, seed):   # biases / LN parameters of every module (value included) away from init; target != critic
    return randomize_params(params, seed)


def _agent(cfg, batch, seed=3, params=None):
    import fql_amd
    a = fql_amd.IFQLAgent.create(seed, batch['observations'][:1], batch['actions'][:1], cfg)
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
    ref = IO.init_params(0, OD, AD, cfg)
    want = {p: v.shape for p, v in O.tree_leaves_with_path(ref)}
    assert dict(a.leaves()) == want
    p = leaf_dict(a.get_params())
    assert p['modules_value/value_net/Dense_0/kernel'].shape == (OD, 64)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.endswith('/kernel'):
            lim = np.sqrt(6.0 / (v.shape[-2] + v.shape[-1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
        if k.startswith('modules_target_critic/'):
            np.testing.assert_array_equal(v, p[k.replace('modules_target_critic/', 'modules_critic/')])


def _check_first_update(a, ref, cfg, params, batch, noise):
    """One update from zero moments on both sides: the 12 infos, every leaf's gradient (Adam mu / 0.1), nu, post-step params, and Polyak
    from the pre-step critic.  Returns the worst max|g_gpu - g_ref| / max|g_ref| over the leaves."""
    _, _, g_ref = ref.grads(batch, noise)
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == IO.INFO_KEYS
    _, want = ref.update(batch, noise)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=IO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    assert opt['count'] == 1 and opt['step'] == 2
    mu, nu = leaf_dict(opt['mu']), leaf_dict(opt['nu'])
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    worst = (0.0, None)
    for p, g in leaf_dict(g_ref).items():
        tol = 2e-5 * np.abs(g).max() + 1e-9
        worst = max(worst, (float(np.abs(mu[p] / 0.1 - g).max() / max(np.abs(g).max(), 1e-30)), p))
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p] / 0.001, g * g, rtol=1e-4, atol=tol * np.abs(g).max() + 1e-12, err_msg=f'nu {p}')
        d = np.abs(new[p] - new_ref[p])
        if p.startswith('modules_target_critic/'):   # Polyak from the PRE-step critic
            assert d.max() <= 1e-6, p
            pre = leaf_dict(params)
            np.testing.assert_allclose(new[p], 0.005 * pre[p.replace('target_critic', 'critic')] + 0.995 * pre[p], atol=1e-6)
        else:
            stable = np.abs(g) > 50 * tol
            assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
            assert d.max() <= 2 * cfg['lr'] + 1e-6, p
    return worst


def _check_total_loss(a, ref, params, batch, noise):
    """total_loss on both sides (9 infos, the loss); no parameter or optimizer state changes."""
    loss, info = a.total_loss(batch, noise=noise)
    want_loss, want = ref.total_loss(batch, noise)
    assert tuple(info) == IO.INFO_KEYS[:9]
    assert_info_close(info, want, keys=IO.INFO_KEYS[:9])
    assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0


@pytest.mark.parametrize('H,B', [(64, 64), (512, 256)])
def test_one_update_matches_fp64_restatement(H, B):
    cfg, _, batch, noise = _problem(H, B, seed=1)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 5)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
    _check_first_update(a, ref, cfg, params, batch, noise)


def test_total_loss_matches_and_changes_no_state():
    cfg, _, batch, noise = _problem(seed=2)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 6)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
    _check_total_loss(a, ref, params, batch, noise)


def test_trajectory_100_updates_tracks_restatement():
    cfg, ds, _, _ = _problem(seed=3)
    rng = np.random.default_rng(9)
    a = _agent(cfg, {'observations': ds['observations'][:1], 'actions': ds['actions'][:1]})
    ref = IO.OracleIFQL(a.get_params(), dict(cfg), OD, AD, np.float64)
    B = cfg['batch_size']
    for _ in range(100):
        batch = O.sample_batch(ds, rng.integers(0, len(ds['observations']), size=B))
        noise = {'x0': rng.standard_normal((B, AD)).astype(np.float32), 't': rng.random(B).astype(np.float32)}
        _, info = a.update(batch, noise=noise)
        _, want = ref.update(batch, noise)
    info = info.to_dict()
    for k in ('value/value_loss', 'critic/critic_loss', 'actor/actor_loss', 'value/v_mean', 'critic/q_mean'):
        assert abs(info[k] - want[k]) <= 2e-3 * max(1.0, abs(want[k])), (k, info[k], want[k])
    a.synchronize()
    got, exp = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for k in got:
        assert np.abs(got[k] - exp[k]).max() <= 5e-3, k


def test_update_from_dataset_explicit_rows_equals_update():
    cfg, ds, _, noise = _problem(seed=4)
    B = cfg['batch_size']
    idx = np.random.default_rng(4).integers(0, len(ds['observations']), size=B)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    a.upload_dataset(ds)
    for _ in range(3):
        a.update_from_dataset(idxs=idx, noise=noise)
        b.update(O.sample_batch(ds, idx), noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


def test_aql_and_graph_updates_bitwise_over_20_steps():
    import torch
    cfg, ds, _, _ = _problem(seed=5)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for _ in range(20):
        a.update_from_dataset()
        b.update_from_dataset(stream=s.cuda_stream)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    a2 = _agent(cfg, ds)   # determinism: same seed, same device-drawn rows and noise
    a2.upload_dataset(ds)
    for _ in range(20):
        a2.update_from_dataset()
    a2.synchronize()
    _same_state(a, a2)


def test_profile_pass_is_one_update():
    """fql_profile_update issues the update's launches eagerly, each dispatch carrying its event pair: the launch mode no other test
    runs for IFQL's kernels.  It reports every launch of the plan, in order, with a device time, and leaves the state one
    update_from_dataset on the same engine-drawn rows leaves."""
    from tests.util import read_plan
    cfg, ds, _, _ = _problem(seed=5)
    B = cfg['batch_size']
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    f = a._lib.fql_profile_update
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    cap = 1024
    typ, lane, grid = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * cap)()
    us, macs, null_us = (C.c_float * cap)(), (C.c_double * cap)(), C.c_float()
    n = f(a._h, B, cap, typ, lane, grid, us, macs, C.byref(null_us))
    assert n == a.stats()['launches_per_update']
    assert list(typ[:n]) == [L['type'] for L in read_plan(a)]
    assert all(np.isfinite(us[i]) and us[i] > 0 for i in range(n)), list(us[:n])
    b.update_from_dataset(batch_size=B)
    a.synchronize(); b.synchronize()
    _same_state(a, b)


def test_sample_actions_best_of_n_and_flow_actions():
    cfg, _, batch, _ = _problem(seed=6)
    params = _randomized(IO.init_params(8, OD, AD, cfg), 8)   # known on the host: the margins below hold for these params and noises
    a = _agent(cfg, batch, params=params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(6)
    N, n = cfg['num_samples'], 5
    obs = batch['observations'][:n]
    noises = (2.0 * rng.standard_normal((n, N, AD))).astype(np.float32)
    one = a.sample_actions(obs[0], noises=noises[0])
    assert one.shape == (AD,)
    many = a.sample_actions(obs, noises=noises)
    assert many.shape == (n, AD) and np.abs(many).max() <= 1.0
    for i in range(n):
        want, q = ref.sample_actions(obs[i], noises[i])
        qs = np.sort(q)
        assert qs[-1] - qs[-2] > 1e-2, (i, qs[-1] - qs[-2])   # a clear winner, so fp32 scoring must choose the same sample
        np.testing.assert_allclose(many[i], want, atol=2e-5, err_msg=str(i))
        np.testing.assert_array_equal(many[i], a.sample_actions(obs[i], noises=noises[i]))
    np.testing.assert_array_equal(one, many[0])
    drawn = a.sample_actions(obs, seed=123)
    assert drawn.shape == (n, AD) and np.abs(drawn).max() <= 1.0
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=123))
    z = rng.standard_normal((n, AD)).astype(np.float32)
    np.testing.assert_allclose(a.compute_flow_actions(obs, z), ref.compute_flow_actions(obs, z), atol=2e-5)


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg, ds, batch, noise = _problem(seed=7)
    a = _agent(cfg, batch)
    for _ in range(2):
        a.update(batch, noise=noise)
    a.synchronize()
    checkpoint.save_agent(a, str(tmp_path), 2)
    b = _agent(cfg, batch, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 2)
    _same_state(a, b)
    sd = checkpoint.to_state_dict(a)
    assert set(sd['network']['params']) == {'modules_actor_flow', 'modules_critic', 'modules_target_critic', 'modules_value'}


def test_fql_and_ifql_interleaved_end_where_they_end_alone():
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, noise = _problem(seed=8)
    fcfg = make_cfg((64,) * 4, batch_size=cfg['batch_size'])

    def fql():
        f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], fcfg)
        f.upload_dataset(ds)
        return f

    def ifql():
        i = _agent(cfg, batch)
        i.upload_dataset(ds)
        return i

    f_alone, i_alone = fql(), ifql()
    for _ in range(5):
        f_alone.update_from_dataset()
    for _ in range(5):
        i_alone.update_from_dataset()
    f, i = fql(), ifql()
    for _ in range(5):
        f.update_from_dataset()
        i.update_from_dataset()
    for x in (f_alone, i_alone, f, i):
        x.synchronize()
    _same_state(f, f_alone)
    _same_state(i, i_alone)


def test_refusals_return_documented_codes():
    import fql_amd
    from fql_amd import _cabi
    cfg, ds, batch, noise = _problem(seed=9)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    B = cfg['batch_size']
    nz = _cabi.FqlNoise()
    assert lib.fql_num_info(h) == 12 and lib.fql_handle_info_name(h, 12) is None
    assert lib.fql_handle_info_name(h, 0).decode() == 'value/value_loss'
    st = C.c_size_t * 2
    assert lib.fql_grad_buckets(h, st(), st()) == _cabi.FQL_E_STATE
    obs, act, rew, mask, nobs = (np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                                 ('observations', 'actions', 'rewards', 'masks', 'next_observations'))
    bp = [x.ctypes.data for x in (obs, act, rew, mask, nobs)]
    assert lib.fql_update_begin(h, *bp, B, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin_split(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin(h, None, B, 0, 0, None, None) == _cabi.FQL_E_STATE
    a.upload_dataset(ds)
    assert lib.fql_update_balanced(h, None, None, None, B, None, None, None) == _cabi.FQL_E_STATE
    frames = np.zeros((64, 32, 32, 3), np.uint8)
    assert lib.fql_dataset_upload_frames(h, 64, frames.ctypes.data, frames.ctypes.data, ds['actions'][:64].ctypes.data,
                                         ds['rewards'][:64].ctypes.data, ds['masks'][:64].ctypes.data, ds['masks'][:64].ctypes.data,
                                         1, 0.0) == _cabi.FQL_E_STATE
    for bad in ('eps1', 'z', 'eps2'):   # the C ABI reads only x0 / t of fql_noise
        x0, t, other = noise['x0'], noise['t'], np.zeros((B, AD), np.float32)
        fields = {'eps1': None, 'x0': x0.ctypes.data, 't': t.ctypes.data, 'z': None, 'eps2': None}
        fields[bad] = other.ctypes.data
        nzb = _cabi.FqlNoise(*[fields[k] for k in ('eps1', 'x0', 't', 'z', 'eps2')])
        assert lib.fql_update(h, *bp, B, C.byref(nzb), None, None) == _cabi.FQL_E_INVALID, bad
    assert lib.fql_replay_create(h, 16) == _cabi.FQL_E_STATE
    keys = np.zeros(10, dtype=np.uint32)
    assert lib.fql_noise_from_jax_keys(h, keys.ctypes.data, 0, B, C.byref(nz), None) == _cabi.FQL_E_STATE
    grp = C.c_void_p()
    assert lib.fql_group_create((C.c_void_p * 1)(h), 1, C.byref(grp)) == _cabi.FQL_E_STATE
    with pytest.raises(ValueError):   # only x0 / t are read
        a.update(batch, noise={'x0': noise['x0'], 't': noise['t'], 'z': noise['x0']})
    c = _cabi.FqlConfig()
    lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim, c.precision = OD, AD, 2
    ic = _cabi.FqlIfqlConfig()
    lib.fql_ifql_default_config(C.byref(ic))
    out = C.c_void_p()
    assert lib.fql_ifql_create(C.byref(c), C.byref(ic), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    c.precision, c.encoder, c.img_h, c.img_w, c.img_c = 0, 1, 64, 64, 3
    assert lib.fql_ifql_create(C.byref(c), C.byref(ic), 0, C.byref(out)) == _cabi.FQL_E_INVALID
    a.update(batch, noise=noise)   # the handle still works after the refusals
    a.synchronize()


# ---- shapes, configs, chunked sampling and batch-size switches -------------------------------------------------------------------------

SHAPE_CASES = [
    # od, ad, B, actor hidden, value hidden, cfg overrides
    pytest.param(7, 3, 16, (32,) * 4, (32,) * 4, {}, id='small'),
    pytest.param(29, 8, 32, (64, 64), (48, 80, 64), {}, id='ragged_depths'),
    pytest.param(11, 5, 48, (64,) * 4, (64,) * 4, dict(layer_norm=False), id='no_layer_norm'),
    pytest.param(17, 6, 64, (64,) * 4, (64,) * 4, dict(actor_layer_norm=True, expectile=0.7, discount=0.995), id='actor_ln_expectile'),
    pytest.param(69, 21, 256, (512,) * 4, (512,) * 4, dict(discount=0.995), id='humanoidmaze'),
    pytest.param(40, 4, 1024, (512,) * 4, (512,) * 4, {}, id='b1024'),   # the value pass runs at M = 2048
]


def _problem_at(od, ad, B, actor, value, seed, **kw):
    import fql_amd
    _, ds, batch, noise = make_problem(od, ad, B, value, seed=seed)
    cfg = fql_amd.ifql.get_config()
    cfg.update(actor_hidden_dims=tuple(actor), value_hidden_dims=tuple(value), batch_size=B)
    cfg.update(kw)
    return cfg, ds, batch, {'x0': noise['x0'], 't': noise['t']}


@pytest.mark.parametrize('od,ad,B,actor,value,kw', SHAPE_CASES)
def test_total_loss_and_update_across_shapes_and_configs(od, ad, B, actor, value, kw):
    cfg, _, batch, noise = _problem_at(od, ad, B, actor, value, seed=11, **kw)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 12)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    _check_total_loss(a, ref, params, batch, noise)
    worst = _check_first_update(a, ref, cfg, params, batch, noise)
    print(f'worst relative gradient error {worst[0]:.3e} ({worst[1]})')


@pytest.mark.parametrize('N,n', [(1, 4097), (7, 590), (65, 64), (100, 42)])
def test_sample_actions_across_the_row_chunk(N, n):
    """n x N sample rows cross the 4096-row chunk (4096 // N observations per chunk; at N = 65 the select kernel's lanes loop).  Rows with a
    clear winner (top two scores more than 1e-2 apart, the margin of test_sample_actions_best_of_n_and_flow_actions) must pick the
    restatement's action; the others one of the candidates within 1e-2 of the best score.  Then the seeded draw's chunk keying."""
    od, ad = 69, 21
    cfg, _, batch, _ = _problem_at(od, ad, 64, (64,) * 4, (64,) * 4, seed=13, num_samples=N)
    params = _randomized(IO.init_params(8, od, ad, cfg), 8)
    a = _agent(cfg, batch, params=params)
    ref = IO.OracleIFQL(params, dict(cfg), od, ad, np.float64)
    rng = np.random.default_rng(N)
    obs = rng.standard_normal((n, od)).astype(np.float32)
    noises = (2.0 * rng.standard_normal((n, N, ad))).astype(np.float32)
    want, cand, q = _best_of_n(ref, obs, noises)
    for i in (0, n - 1):   # the batched restatement is OracleIFQL.sample_actions row by row
        w, qi = ref.sample_actions(obs[i], noises[i])
        np.testing.assert_allclose(want[i], w, rtol=0, atol=1e-12)
        np.testing.assert_allclose(q[i], qi, rtol=0, atol=1e-12)
    got = a.sample_actions(obs, noises=noises)
    assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
    qs = np.sort(q, axis=1)
    clear = qs[:, -1] - qs[:, -2] > 1e-2 if N > 1 else np.ones(n, bool)
    assert clear.mean() >= 0.5, clear.mean()
    np.testing.assert_allclose(got[clear], want[clear], atol=2e-5)
    for i in np.nonzero(~clear)[0]:
        near = q[i] >= q[i].max() - 1e-2
        assert np.abs(cand[i][near] - got[i]).max(axis=1).min() <= 2e-5, i
    np.testing.assert_array_equal(got[n - 1], a.sample_actions(obs[n - 1], noises=noises[n - 1]))   # the second chunk's last row
    per = 4096 // N
    same = np.repeat(obs[:1], per + 1, axis=0)
    drawn = a.sample_actions(same, seed=5)
    assert np.abs(drawn).max() <= 1.0
    assert np.abs(drawn[per] - drawn[0]).max() > 1e-3   # the second chunk's first observation draws its own noises
    np.testing.assert_array_equal(drawn[:per], a.sample_actions(same[:per], seed=5))


def _check_step(a, ref, cfg, batch, noise, pre):
    """One more update, moments carried from earlier steps: test_gpu_rebrac._check_step's bounds.  The gradient is (mu - 0.9 mu0) / 0.1;
    the targets are Polyak of the engine's own pre-step critic and target."""
    _, _, g_ref = ref.grads(batch, noise)
    mu0 = leaf_dict(a.get_opt_state()['mu'])
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == IO.INFO_KEYS
    _, want = ref.update(batch, noise)
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=IO.INFO_KEYS)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    for p, g in leaf_dict(g_ref).items():
        if p.startswith('modules_target_critic/'):
            np.testing.assert_allclose(new[p], 0.005 * pre[p.replace('target_critic', 'critic')] + 0.995 * pre[p], atol=1e-6, err_msg=p)
            continue
        tol = 2e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9
        np.testing.assert_allclose((mu[p] - np.float32(0.9) * mu0[p]) / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
        d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))
        stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
        assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p


def test_batch_size_switches_track_restatement():
    """B = 64, 32, 64: each switch rebuilds the workspace and programs; every step is compared after the rebuild, from the engine's own
    pre-step state (sync_restatement).  Then update_from_dataset after a switch equals update on the same rows, bitwise."""
    cfg, ds, batch, _ = _problem_at(OD, AD, 64, (64,) * 4, (64,) * 4, seed=14)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 15)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
    rng = np.random.default_rng(14)
    steps = []
    for i, B in enumerate((64, 32, 64)):
        idx = rng.integers(0, len(ds['observations']), size=B)
        noise = {'x0': rng.standard_normal((B, AD)).astype(np.float32), 't': rng.random(B).astype(np.float32)}
        steps.append((idx, noise))
        print('step at B', B)
        assert a.get_opt_state()['count'] == i
        sync_restatement(ref, a)
        _check_step(a, ref, cfg, O.sample_batch(ds, idx), noise, leaf_dict(a.get_params()))
    opt = a.get_opt_state()
    assert opt['count'] == 3 and opt['step'] == 4
    x, y = _agent(cfg, ds, params=params), _agent(cfg, ds, params=params)
    x.upload_dataset(ds)
    for idx, noise in steps:
        x.update_from_dataset(batch_size=len(idx), idxs=idx, noise=noise)
        y.update(O.sample_batch(ds, idx), noise=noise)
    x.synchronize(); y.synchronize()
    _same_state(x, y)
    assert x.read_info() == y.read_info()
