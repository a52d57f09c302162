"""CPU tests of the BC agent's restatements (tests/bc_oracle.py, tests/bc_oracle_torch.py) and of the host-side BCAgent surface."""
import numpy as np
import pytest

import bc_oracle as BO
import bc_oracle_torch as BT
import fql_amd
from fql_amd import bc as bcmod
from oracle import fql_oracle as O

OD, AD, B, S = 7, 3, 12, 4


def _problem(ln=1, hidden=(16, 16), seed=0, S=S):
    cfg = BO.get_config()
    cfg.update(hidden_dims=hidden, denoise_steps=S, use_layer_norm=ln, batch_size=B)
    params = BO.init_params(seed, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(seed + 1)
    for _, v in O.tree_leaves_with_path(params):
        v += 0.1 * rng.standard_normal(v.shape)
    batch = {'observations': rng.standard_normal((B, OD)), 'actions': np.clip(rng.standard_normal((B, AD)), -1, 1)}
    return cfg, params, batch, BO.make_noise(B, AD, S, seed + 2)


@pytest.mark.parametrize('ln', [0, 1])
def test_numpy_equals_torch(ln):
    cfg, params, batch, noise = _problem(ln)
    a, b = BO.OracleBC(params, cfg, OD, AD, np.float64), BT.TorchBC(params, cfg)
    la, _, ga = a.grads(batch, noise)
    lb, gb = b.grads(batch, noise)
    assert abs(la - lb) <= 1e-12 * max(1.0, abs(la))
    gb = BT.leaves(gb)
    for p, v in O.tree_leaves_with_path(ga):
        np.testing.assert_allclose(v, gb[p], rtol=1e-9, atol=1e-13, err_msg=p)
    sn = np.random.default_rng(9).standard_normal((5, AD))
    np.testing.assert_allclose(a.sample_actions(batch['observations'][:5], sn), b.sample_actions(batch['observations'][:5], sn), atol=1e-12)
    a.update(batch, noise)
    b.update(batch, noise)
    pb = BT.leaves(b.params)
    for p, v in O.tree_leaves_with_path(a.params):
        np.testing.assert_allclose(v, pb[p], rtol=1e-9, atol=1e-13, err_msg=p)


def test_finite_differences_on_a_tiny_net():
    cfg, params, batch, noise = _problem(1, hidden=(6, 5))
    ref = BO.OracleBC(params, cfg, OD, AD, np.float64)
    _, _, g = ref.grads(batch, noise)
    rng = np.random.default_rng(4)
    gl = dict(O.tree_leaves_with_path(g))
    for p, v in O.tree_leaves_with_path(ref.params):
        for _ in range(3):
            i = tuple(rng.integers(0, s) for s in v.shape)
            old, h = v[i], 1e-6
            v[i] = old + h
            lp = ref.policy_loss(batch, noise)[0]
            v[i] = old - h
            lm = ref.policy_loss(batch, noise)[0]
            v[i] = old
            fd = (lp - lm) / (2 * h)
            assert abs(fd - gl[p][i]) <= 1e-6 * max(1.0, abs(fd)) + 1e-9, (p, i, fd, gl[p][i])


def test_embedding_known_answers():
    e0 = bcmod.timestep_embedding(np.array([0]), 16)[0]
    np.testing.assert_array_equal(e0[:8], np.ones(8, np.float32))    # t = 0: cos = 1
    np.testing.assert_array_equal(e0[8:], np.zeros(8, np.float32))   # ... and sin = 0
    e1 = bcmod.timestep_embedding(np.array([16]), 16)[0]              # t = 1, i = 0: the argument is exactly 10000
    assert e1[0] == np.float32(np.cos(10000.0)) and e1[8] == np.float32(np.sin(10000.0))
    assert e1.dtype == np.float32 and e1.shape == (16,)
    # freq_i = float32(exp_f64(-ln(10000) i / 8)); i = 4 is exactly 1e-2 rounded to fp32
    assert bcmod.timestep_embedding(np.array([16]), 16)[0][4] == np.float32(np.cos(np.float64(np.float32(10000.0) * np.float32(0.01))))


def test_loss_of_an_all_zero_network_is_mean_vel_squared():
    cfg, params, batch, noise = _problem(1)
    params = O.tree_map(np.zeros_like, params)
    ref = BO.OracleBC(params, cfg, OD, AD, np.float64)
    vel = batch['actions'] - noise['x0']
    assert abs(ref.policy_loss(batch, noise)[0] - np.mean(vel * vel)) <= 1e-14


def test_squeeze_and_info_keys():
    cfg, params, batch, noise = _problem(1)
    ref = BO.OracleBC(params, cfg, OD, AD, np.float64)
    sn = np.random.default_rng(1).standard_normal((1, AD))
    a1 = ref.sample_actions(batch['observations'][:1], sn)
    a0 = ref.sample_actions(batch['observations'][0], sn[0])
    assert a1.shape == (AD,) and a0.shape == (AD,)
    np.testing.assert_array_equal(a0, a1)
    assert ref.sample_actions(batch['observations'][:3], np.zeros((3, AD))).shape == (3, AD)
    assert np.all(np.abs(a1) <= 1.0)
    _, info = ref.update(batch, noise)
    assert tuple(info) == ('bc_loss', 'grad/max', 'grad/min', 'grad/norm') == fql_amd.BC_INFO_KEYS == BO.INFO_KEYS


def test_fp32_rounding_of_the_sampler_grows_with_the_head_scale():
    """The inputs of tests/test_gpu_bc.py::test_sample_actions_match_oracle_and_single_calls at n = 4097, restated in fp32 numpy against
    fp64: with the head scaled by 2 (the GPU test's scale) fp32 arithmetic alone stays within 5e-6 of fp64; scaled by 6, |x| runs to ~10
    inside the flow, every Euler step's rounding passes through the head's gain, and fp32 numpy itself leaves the 2e-5 bound the GPU
    test holds the engine to.  So that bound is tested where the number format can meet it."""
    od, ad, n = 29, 8, 4097
    cfg = BO.get_config()
    cfg.update(hidden_dims=(64,) * 4, batch_size=64)
    worst = {}
    for scale in (2.0, 6.0):
        params = O.tree_map(lambda a: np.array(a, np.float32), BO.init_params(8, od, ad, cfg))
        rng = np.random.default_rng(8)
        for p, v in O.tree_leaves_with_path(params):
            if not p.endswith('/kernel'):
                v += (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
        params['Dense_0']['kernel'] *= scale
        rng = np.random.default_rng(n)
        obs = rng.standard_normal((n, od)).astype(np.float32)
        sn = rng.standard_normal((n, ad)).astype(np.float32)
        a64 = BO.OracleBC(params, cfg, od, ad, np.float64).sample_actions(obs, sn)
        a32 = BO.OracleBC(params, cfg, od, ad, np.float32).sample_actions(obs, sn)
        assert a32.dtype == np.float32
        worst[scale] = float(np.abs(a32.astype(np.float64) - a64).max())
    assert worst[2.0] <= 5e-6 and worst[6.0] > 2e-5, worst


def test_fp32_rounding_of_the_sampler_at_hidden_512():
    """The inputs of tests/test_gpu_bc.py::test_sample_actions_at_hidden_512_and_padded_action_width_32 (obs 69, act 21, hidden 512 x 4,
    head scaled by 2, n = 1, 37, 4097), from that module's own builders: fp32 numpy stays within 5e-6 of fp64 (measured 3.2e-6 at
    n 4097), a quarter of the 2e-5 the GPU test allows, and the clip is reached (62 % of the coordinates)."""
    from tests import test_gpu_bc as G
    cfg, params = G.sampler512_problem()
    od, ad = G.SAMPLER512['od'], G.SAMPLER512['ad']
    assert (od, ad, tuple(cfg['hidden_dims']), G.SAMPLER512['ns']) == (69, 21, (512,) * 4, (1, 37, 4097))
    r64, r32 = BO.OracleBC(params, cfg, od, ad, np.float64), BO.OracleBC(params, cfg, od, ad, np.float32)
    worst = {}
    for n in G.SAMPLER512['ns']:
        obs, sn = G.sampler512_inputs(n)
        a64, a32 = r64.sample_actions(obs, sn), r32.sample_actions(obs, sn)
        assert a32.dtype == np.float32
        worst[n] = float(np.abs(a32.astype(np.float64) - a64).max())
        assert (np.abs(a64) == 1).any(), n
        if n > 1:
            assert 0.2 < (np.abs(a64) == 1).mean() < 0.9
    print(worst)
    assert max(worst.values()) <= 5e-6, worst


def test_lecun_normal_statistics():
    k = BO.lecun_normal(np.random.default_rng(0), 512, (512, 64), np.float64)
    assert abs(k.var() * 512 - 1.0) < 0.03 and abs(k.mean()) < 1e-3
    assert np.abs(k).max() <= 2.0 * np.sqrt(1.0 / 512) / 0.87962566103423978 + 1e-12


def test_registry_config_and_host_refusals():
    assert fql_amd.agents['bc'] is fql_amd.BCAgent
    cfg = bcmod.get_config()
    want = dict(agent_name='bc', batch_size=256, hidden_dims=(512, 512, 512, 512), bc_lr=3e-4, use_layer_norm=1, activation='gelu',
                denoise_steps=16, rng='engine', precision='fp32')
    assert dict(cfg) == want
    ob, ac = np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32)
    for bad in (dict(activation='relu'), dict(encoder='impala_small'), dict(precision='bf16x3'), dict(rng='jax')):
        c = bcmod.get_config()
        c.update(bad)
        with pytest.raises(NotImplementedError):
            fql_amd.BCAgent.create(0, ob, ac, c)
    with pytest.raises(ValueError):
        bcmod.grid_index(np.array([0.0, 0.3]), 4)
    np.testing.assert_array_equal(bcmod.grid_index(np.array([0.0, 0.25, 1.0], np.float32), 4), [0, 1, 4])


def test_create_without_a_gpu_fails_loudly():
    """No CPU fallback: without a HIP device BCAgent.create raises (FQL_E_NODEVICE), as FQLAgent.create does; with one it succeeds."""
    import torch
    args = (0, np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32), dict(hidden_dims=(64, 64), batch_size=16))
    if torch.cuda.is_available():
        fql_amd.BCAgent.create(*args).close()
        return
    with pytest.raises(RuntimeError, match='no HIP device'):
        fql_amd.BCAgent.create(*args)
