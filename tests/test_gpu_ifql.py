"""GPU: the IFQL agent (agents/ifql.py) on the engine against the fp64 restatement in tests/ifql_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import ifql_oracle as IO
from tests.util import assert_info_close, leaf_dict, make_problem, randomize_params

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


@pytest.mark.parametrize('H,B', [(64, 64), (512, 256)])
def test_one_update_matches_fp64_restatement(H, B):
    cfg, _, batch, noise = _problem(H, B, seed=1)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 5)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
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
    for p, g in leaf_dict(g_ref).items():
        tol = 2e-5 * np.abs(g).max() + 1e-9
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


def test_total_loss_matches_and_changes_no_state():
    cfg, _, batch, noise = _problem(seed=2)
    a = _agent(cfg, batch)
    params = _randomized(a.get_params(), 6)
    a.set_params(params)
    ref = IO.OracleIFQL(params, dict(cfg), OD, AD, np.float64)
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
