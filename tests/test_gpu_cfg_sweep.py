"""GPU: the guidance sweeps of IQL-diffusion and CFGRL (sample_actions_rows / sample_actions_sweep: one guidance weight per row, one
call, a program S - 1 launches shorter).

The primary check has NO tolerance: for every distinct weight c of a call, the rows that carry c are bitwise sample_actions(obs[rows],
cfg=c, noises=z[rows]) of the same agent, whose results tests/test_gpu_iqld.py and tests/test_gpu_cfgrl.py hold to the fp64 restatement.
The secondary check is that restatement at the project's atol = 2e-5, on the rows with weight 0 or 3 only and on the inputs and n that
tests/test_iqld_cpu.py::test_fp32_rounding_of_the_cfg_sampler* and tests/test_cfgrl_cpu.py::test_fp32_rounding_of_the_sampler_at_hidden_512
back (sampler_inputs(n) at head scale 2 and hidden 64, SAMPLER512 at its own scale, sampler512_inputs(n); n = 37 and 2049): the fp32 error
grows with the weight and no bound exists for 1.5, 5, 10 or 30."""
import ctypes as C

import numpy as np
import pytest

from tests import cfgrl_oracle as CO
from tests import iqld_cases as K
from tests import iqld_oracle as DO
from tests.test_gpu_cfgrl import SAMPLER512 as G512
from tests.test_gpu_cfgrl import _agent as _cfgrl_agent
from tests.test_gpu_cfgrl import _cfg as _cfgrl_cfg
from tests.test_gpu_cfgrl import _randomized, sampler512_inputs, sampler512_problem
from tests.test_gpu_iqld import _agent, _built

pytestmark = pytest.mark.gpu
OD, AD = K.OD, K.AD
CYCLE = np.array([0.0, 1.0, 1.5, 3.0, 5.0, 30.0], np.float32)
ATOL = 2e-5


def _cycle(n):
    return CYCLE[np.arange(n) % len(CYCLE)]


def _groups(w):
    return [(float(c), np.flatnonzero(w == c)) for c in sorted(set(np.asarray(w).tolist()))]


def _bitwise(got, w, single):
    """rows of each distinct weight against the scalar call on those rows: single(rows, c) -> [len(rows), act]"""
    assert got.shape[0] == len(w) and got.ndim == 2
    for c, rows in _groups(w):
        np.testing.assert_array_equal(got[rows], single(rows, c).reshape(len(rows), -1), err_msg=f'cfg {c}')


def _restated(got, w, restate):
    """rows with weight 0 or 3 against the fp64 restatement on those rows at 2e-5: restate(rows, c) -> [len(rows), act]"""
    for c, rows in _groups(w):
        if c in (0.0, 3.0):
            want = restate(rows, c).reshape(len(rows), -1)
            print('restatement cfg', c, 'rows', len(rows), 'max err', float(np.abs(got[rows] - want).max()))
            np.testing.assert_allclose(got[rows], want, rtol=0, atol=ATOL)


def _iqld_checks(a, ref, obs, z, w, restate):
    got = a.sample_actions_rows(obs, w, noises=z)
    assert isinstance(got, np.ndarray) and got.shape == (len(w), z.shape[1]) and got.dtype == np.float32
    _bitwise(got, w, lambda rows, c: a.sample_actions(obs[rows], noises=z[rows], cfg=c))
    if restate:
        _restated(got, w, lambda rows, c: ref.sample_actions(obs[rows], z[rows], c))
    return got


# ---- IQL-diffusion ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sampler():
    """tests/test_gpu_iqld.py's sampler problem: hidden 64 x 4, S 16, obs 29, act 8, the head scaled by 2"""
    cfg, params, _ = K.sampler_problem()
    return _agent(cfg, params=params), DO.OracleIQLD(params, cfg, OD, AD, np.float64)


@pytest.mark.parametrize('n', [1, 5, 16, 37])
def test_iqld_rows_are_the_scalar_calls(sampler, n):
    a, ref = sampler
    obs, z = K.sampler_inputs(n)
    got = _iqld_checks(a, ref, obs, z, _cycle(n), restate=n == 37)
    assert (np.abs(got) <= 1).all()
    if n == 37:
        assert (np.abs(got) == 1).any()   # the clip is reached
    assert a.sample_cfgs_stats() == 4 + 16 * 5 + 1 and a.iqld_stats()[2] == 4 + 16 * 6


def test_iqld_chunk_boundary(sampler):
    """2049 rows: the second chunk holds one row, whose weight (0) is the other one than row 2048's neighbour in the first chunk"""
    a, ref = sampler
    n = 2049
    obs, z = K.sampler_inputs(n)
    w = np.where(np.arange(n) % 2 == 0, 0.0, 3.0).astype(np.float32)
    w[0], w[n - 1] = 3.0, 0.0   # row 0 of chunk 0 and row 0 of chunk 1 differ
    _iqld_checks(a, ref, obs, z, w, restate=True)


@pytest.mark.parametrize('name, c', [('S1', K.SHAPES['od70-ad17-S1']), ('S2', K.case(nh=2, S=2)), ('S3', K.case(nh=2, S=3)),
                                     ('od5-ad1', K.case(od=5, ad=1))])
def test_iqld_ping_pong_parity_and_launch_counts(name, c):
    """S = 1 has no fused launch and reads X[0]; S = 2 ends on X[1], S = 3 on X[0] again; act 1 and the padded width 32 of act 17"""
    cfg, params, _ = K.sampler_problem(c=c)
    a = _agent(cfg, c['od'], c['ad'], params=params)
    for n in (5, 17):
        obs, z = K.sampler_inputs(n, c['od'], c['ad'])
        _iqld_checks(a, None, obs, z, _cycle(n), restate=False)
    S, nl = c['S'], c['nh'] + 1
    assert a.sample_cfgs_stats() == 4 + S * nl + 1
    assert a.iqld_stats()[2] == 4 + S * (nl + 1)


def test_iqld_padded_action_width():
    """SAMPLER512: obs 69, act 21 (rows of x stride 32), hidden 512"""
    c = K.SAMPLER512
    cfg, params, _ = K.sampler_problem(K.SAMPLER512_HEAD_SCALE, c)
    a, ref = _agent(cfg, c['od'], c['ad'], params=params), DO.OracleIQLD(params, cfg, c['od'], c['ad'], np.float64)
    obs, z = K.sampler_inputs(37, c['od'], c['ad'])
    got = _iqld_checks(a, ref, obs, z, _cycle(37), restate=True)
    assert (np.abs(got) == 1).any()


# ---- CFGRL ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gsampler():
    cfg, params = sampler512_problem()
    return (_cfgrl_agent(cfg, G512['od'], G512['ad'], G512['gd'], params=params),
            CO.OracleCFGRL(params, dict(cfg), G512['od'], G512['ad'], G512['gd'], np.float64))


def _cfgrl_checks(a, ref, obs, goals, z, w, restate):
    got = a.sample_actions_rows(obs, goals, w, noises=z)
    assert isinstance(got, np.ndarray) and got.shape == (len(w), z.shape[1])
    _bitwise(got, w, lambda rows, c: a.sample_actions(obs[rows], goals[rows], noises=z[rows], cfg=c))
    if restate:
        _restated(got, w, lambda rows, c: ref.sample_actions(obs[rows], goals[rows], z[rows], c))
    return got


def test_cfgrl_rows_are_the_scalar_calls(gsampler):
    a, ref = gsampler
    obs, goals, z = sampler512_inputs(37)
    got = _cfgrl_checks(a, ref, obs, goals, z, _cycle(37), restate=True)
    assert (np.abs(got) == 1).any() and (np.abs(got) <= 1).all()
    one = a.sample_actions_rows(obs, goals[0], _cycle(37), noises=z)            # one [G] for every row
    np.testing.assert_array_equal(one, a.sample_actions_rows(obs, np.tile(goals[:1], (37, 1)), _cycle(37), noises=z))
    nl = len(G512['hidden']) + 1
    assert a.sample_cfgs_stats() == 3 + 16 * nl + 1 and a.cfgrl_stats()[2] == 3 + 16 * (nl + 1)


def test_cfgrl_chunk_boundary(gsampler):
    a, ref = gsampler
    n = 2049
    obs, goals, z = sampler512_inputs(n)
    w = np.where(np.arange(n) % 2 == 0, 0.0, 3.0).astype(np.float32)
    w[0], w[n - 1] = 3.0, 0.0
    _cfgrl_checks(a, ref, obs, goals, z, w, restate=True)


@pytest.mark.parametrize('S', [1, 2, 3])
def test_cfgrl_small_agents(S):
    od, ad, gd = 13, 5, 7
    cfg = _cfgrl_cfg(64, 64, 2, flow_steps=S, actor_layer_norm=True)
    a = _cfgrl_agent(cfg, od, ad, gd)
    params = _randomized(a.get_params(), 20 + S)
    params['modules_actor_flow']['mlp']['Dense_2']['kernel'] *= np.float32(2.0)
    a.set_params(params)
    for n in (5, 17):
        rng = np.random.default_rng(n)
        obs, goals, z = (rng.standard_normal((n, d)).astype(np.float32) for d in (od, gd, ad))
        _cfgrl_checks(a, None, obs, goals, z, _cycle(n), restate=False)
    assert a.sample_cfgs_stats() == 3 + S * 3 + 1 and a.cfgrl_stats()[2] == 3 + S * 4


# ---- sample_actions_sweep ---------------------------------------------------------------------------------------------------------
def test_sweep_shapes_tiling_seeds_and_tensors(sampler):
    import torch
    a, _ = sampler
    n, cfgs = 10, np.array([1.0, 1.5, 3.0, 5.0], np.float32)
    G = len(cfgs)
    obs, z = K.sampler_inputs(n)
    out = a.sample_actions_sweep(obs, cfgs, noises=z)
    assert out.shape == (G, n, AD)
    for g in range(G):
        np.testing.assert_array_equal(out[g], a.sample_actions(obs, noises=z, cfg=float(cfgs[g])))
    tiled_obs, tiled_z = np.tile(obs[None], (G, 1, 1)), np.tile(z[None], (G, 1, 1))
    np.testing.assert_array_equal(a.sample_actions_sweep(tiled_obs, cfgs, noises=z), out)
    np.testing.assert_array_equal(a.sample_actions_sweep(obs, cfgs, noises=tiled_z), out)
    other = tiled_obs.copy()
    other[1] = obs[::-1]                      # one vector env per weight: slice 1 sees other rows
    np.testing.assert_array_equal(a.sample_actions_sweep(other, cfgs, noises=z)[1], a.sample_actions(obs[::-1], noises=z, cfg=1.5))
    s7 = a.sample_actions_sweep(obs, cfgs, seed=7)
    np.testing.assert_array_equal(s7, a.sample_actions_sweep(obs, cfgs, seed=7))
    np.testing.assert_array_equal(s7, a.sample_actions_rows(tiled_obs.reshape(G * n, OD), np.repeat(cfgs, n), seed=7).reshape(G, n, AD))
    assert np.abs(s7 - a.sample_actions_sweep(obs, cfgs, seed=8)).max() > 0
    t = a.sample_actions_sweep(torch.from_numpy(obs).cuda(), torch.from_numpy(cfgs).cuda(), noises=torch.from_numpy(z).cuda())
    assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == (G, n, AD)
    np.testing.assert_array_equal(t.cpu().numpy(), out)


def test_cfgrl_sweep(gsampler):
    a, _ = gsampler
    n, cfgs = 6, np.array([0.0, 3.0, 10.0], np.float32)
    obs, goals, z = sampler512_inputs(n)
    out = a.sample_actions_sweep(obs, goals, cfgs, noises=z)
    assert out.shape == (3, n, G512['ad'])
    for g in range(3):
        np.testing.assert_array_equal(out[g], a.sample_actions(obs, goals, noises=z, cfg=float(cfgs[g])))
    np.testing.assert_array_equal(a.sample_actions_sweep(obs, np.tile(goals[None], (3, 1, 1)), cfgs, noises=z), out)
    one = a.sample_actions_sweep(obs, goals[0], cfgs, noises=z)
    for g in range(3):
        np.testing.assert_array_equal(one[g], a.sample_actions(obs, goals[0], noises=z, cfg=float(cfgs[g])))


# ---- isolation --------------------------------------------------------------------------------------------------------------------
def test_scalar_calls_are_untouched_and_nothing_is_cached():
    cfg, params, batch, noise, _, a = _built(K.STEP_KINDS)
    obs, z = K.sampler_inputs(16)
    w = _cycle(16)
    s1 = a.sample_actions(obs, noises=z, cfg=3.0)
    r0 = a.sample_actions_rows(obs, w, noises=z)
    np.testing.assert_array_equal(a.sample_actions(obs, noises=z, cfg=3.0), s1)
    a.update(batch, noise=noise)
    r1 = a.sample_actions_rows(obs, w, noises=z)
    _bitwise(r1, w, lambda rows, c: a.sample_actions(obs[rows], noises=z[rows], cfg=c))   # the new parameters
    assert np.abs(r1 - r0).max() > 0


def test_rows_wait_for_updates_in_flight():
    """three stream-less update_from_dataset calls (they may still be on the engine's AQL queues), then sample_actions_rows at once"""
    from oracle import fql_oracle as O
    cfg, params, _, _, _, a = _built(K.STEP_KINDS)
    b = _agent(cfg, params=params)
    ds = O.make_synthetic_dataset(512, OD, AD, seed=5)
    obs, z = K.sampler_inputs(16)
    w = _cycle(16)
    for x in (a, b):
        x.upload_dataset(ds)
        for _ in range(3):
            x.update_from_dataset()
        if x is b:
            x.synchronize()
    np.testing.assert_array_equal(a.sample_actions_rows(obs, w, noises=z), b.sample_actions_rows(obs, w, noises=z))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(sampler):
    import fql_amd
    import fql_amd.bc
    import fql_amd.iql
    from fql_amd import _cabi
    from tests.util import make_problem
    lib = _cabi.load()
    E, INV = _cabi.FQL_E_STATE, _cabi.FQL_E_INVALID
    f = lambda arr: arr.ctypes.data_as(C.c_void_p)   # noqa: E731
    a, _ = sampler
    obs, z = K.sampler_inputs(4)
    w = np.ones(4, np.float32)
    out = np.zeros((4, AD), np.float32)
    i64 = C.c_int64()
    fcfg, _, fbatch, _ = make_problem(OD, AD, 64, (64,) * 4, seed=7)
    ex = (fbatch['observations'][:1], fbatch['actions'][:1])
    g = _cfgrl_agent(_cfgrl_cfg())
    others = [fql_amd.FQLAgent.create(1, *ex, fcfg), fql_amd.IQLAgent.create(1, *ex, dict(fql_amd.iql.get_config(), batch_size=64)),
              fql_amd.BCAgent.create(1, *ex, dict(fql_amd.bc.get_config(), batch_size=64))]
    for x in others + [g]:
        assert lib.fql_iqld_sample_actions_cfgs(x._h, f(obs), 4, f(z), 0, f(w), f(out), None) == E
        assert b'fql_iqld_sample_actions_cfgs needs an IQL-diffusion handle' in lib.fql_last_error(x._h)
    for x in others + [a]:
        assert lib.fql_cfgrl_sample_actions_cfgs(x._h, f(obs), f(obs), 4, f(z), 0, f(w), f(out), None) == E
        assert b'fql_cfgrl_sample_actions_cfgs needs' in lib.fql_last_error(x._h)
    for x in others:
        assert lib.fql_sample_cfgs_stats(x._h, C.byref(i64)) == E
        assert b'fql_sample_cfgs_stats' in lib.fql_last_error(x._h)
    assert lib.fql_sample_cfgs_stats(g._h, C.byref(i64)) == 0 and lib.fql_sample_cfgs_stats(a._h, C.byref(i64)) == 0
    h = a._h
    assert lib.fql_iqld_sample_actions_cfgs(h, f(obs), 4, f(z), 0, None, f(out), None) == INV
    assert b'cfgs' in lib.fql_last_error(h)
    assert lib.fql_iqld_sample_actions_cfgs(h, f(obs), 0, f(z), 0, f(w), f(out), None) == INV
    bad = w.copy()
    bad[2] = np.nan
    assert lib.fql_iqld_sample_actions_cfgs(h, f(obs), 4, f(z), 0, f(bad), f(out), None) == INV
    assert b'cfgs[2]' in lib.fql_last_error(h)
    gobs = np.zeros((4, 29), np.float32)
    assert lib.fql_cfgrl_sample_actions_cfgs(g._h, f(gobs), f(gobs), 4, None, 0, None, f(out), None) == INV
    bad[2] = np.inf
    assert lib.fql_cfgrl_sample_actions_cfgs(g._h, f(gobs), f(gobs), 4, None, 0, f(bad), f(out), None) == INV
    assert b'cfgs[2]' in lib.fql_last_error(g._h)
    with pytest.raises(ValueError):
        a.sample_actions_rows(obs, bad, noises=z)
