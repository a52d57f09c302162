"""CPU: the guidance-sweep entry points are declared, exported and bound; NULL handles are refused; the host mirrors validate shapes,
lengths and weights before the library is called; sample_actions_sweep is a flatten, repeat and reshape over sample_actions_rows."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('fql_iqld_sample_actions_cfgs', 'fql_cfgrl_sample_actions_cfgs', 'fql_sample_cfgs_stats')
OD, AD, GD = 7, 3, 4


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fql_amd.h')).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r'\b' + n + r'\s*\(', header), n
        assert n in _cabi.SYMBOLS and hasattr(lib, n), n
    assert lib.fql_abi_version() == 1


def test_null_handles_are_rejected(lib):
    from fql_amd import _cabi
    assert lib.fql_iqld_sample_actions_cfgs(None, None, 1, None, 0, None, None, None) == _cabi.FQL_E_INVALID
    assert lib.fql_cfgrl_sample_actions_cfgs(None, None, None, 1, None, 0, None, None, None) == _cabi.FQL_E_INVALID
    assert lib.fql_sample_cfgs_stats(None, None) == _cabi.FQL_E_INVALID


class _NoLib:
    """any library call fails the test: the checks must come first"""

    def __getattr__(self, name):
        raise AssertionError(f'{name} was called before the arguments were validated')


def _mirror(cls, **config):
    a = cls.__new__(cls)   # no engine: create() is never reached
    a._lib, a._h, a.config, a._seed, a._sample_calls, a._keep = _NoLib(), None, dict(config), 0, 0, []
    return a


@pytest.fixture
def agents(monkeypatch):
    import fql_amd
    from fql_amd import agent as A

    def boom(*a, **k):
        raise AssertionError('create touched the device')
    monkeypatch.setattr(A.FQLAgent, 'create', classmethod(boom))
    monkeypatch.setattr(A.FQLAgent, 'close', lambda self: None)
    return (_mirror(fql_amd.agents['iql_diffusion'], ob_dims=(OD,), action_dim=AD),
            _mirror(fql_amd.CFGRLAgent, ob_dims=(OD,), action_dim=AD, goal_dim=GD))


def _f(*shape):
    return np.zeros(shape, np.float32)


@pytest.mark.parametrize('obs, cfgs, noises', [
    (_f(OD), [1.0], None),                          # no batch axis: rows never squeeze
    (_f(5, OD + 1), _f(5), None),                   # observation width
    (_f(0, OD), _f(0), None),                       # no rows
    (_f(5, OD), _f(4), None),                       # len(cfgs) against the leading axis
    (_f(5, OD), _f(5, 1), None),
    (_f(5, OD), [1.0, 2.0, np.nan, 1.0, 1.0], None),
    (_f(5, OD), [1.0, 2.0, np.inf, 1.0, 1.0], None),
    (_f(5, OD), _f(5), _f(4, AD)),                  # noises
    (_f(5, OD), _f(5), _f(5, AD + 1)),
])
def test_rows_validate_before_the_library(agents, obs, cfgs, noises):
    d, g = agents
    with pytest.raises(ValueError):
        d.sample_actions_rows(obs, cfgs, noises=noises)
    with pytest.raises(ValueError):
        g.sample_actions_rows(obs, _f(GD), cfgs, noises=noises)


def test_cfgrl_rows_validate_goals(agents):
    _, g = agents
    for goals in (None, _f(4, GD), _f(5, GD + 1), _f(GD + 1)):
        with pytest.raises(ValueError):
            g.sample_actions_rows(_f(5, OD), goals, _f(5))


@pytest.mark.parametrize('obs, cfgs, noises', [
    (_f(5, OD), [], None),                          # an empty sweep
    (_f(5, OD), _f(2, 2), None),
    (_f(5, OD), [1.0, np.nan], None),
    (_f(3, 5, OD), _f(2), None),                    # [G, n, od] against len(cfgs)
    (_f(2, 0, OD), _f(2), None),
    (_f(5, OD + 1), _f(2), None),
    (_f(5, OD), _f(2), _f(4, AD)),
    (_f(5, OD), _f(2), _f(3, 5, AD)),
    (_f(5, OD), _f(2), _f(AD)),                     # one noise row is not broadcast
])
def test_sweeps_validate_before_the_library(agents, obs, cfgs, noises):
    d, g = agents
    with pytest.raises(ValueError):
        d.sample_actions_sweep(obs, cfgs, noises=noises)
    with pytest.raises(ValueError):
        g.sample_actions_sweep(obs, _f(GD), cfgs, noises=noises)


def test_sweep_is_flatten_repeat_reshape(agents, monkeypatch):
    d, g = agents
    rng = np.random.default_rng(0)
    G, n = 3, 4
    cfgs = np.array([1.0, 1.5, 3.0], np.float32)
    obs, obs3 = rng.standard_normal((n, OD)).astype(np.float32), rng.standard_normal((G, n, OD)).astype(np.float32)
    z, z3 = rng.standard_normal((n, AD)).astype(np.float32), rng.standard_normal((G, n, AD)).astype(np.float32)
    goals, goals3 = rng.standard_normal((n, GD)).astype(np.float32), rng.standard_normal((G, n, GD)).astype(np.float32)
    seen = {}

    def rows_d(observations, w, seed=None, noises=None):
        seen.update(obs=observations, w=w, seed=seed, z=noises)
        return np.arange(len(w) * AD, dtype=np.float32).reshape(len(w), AD)

    def rows_g(observations, gl, w, seed=None, noises=None):
        seen.update(obs=observations, goals=gl, w=w, seed=seed, z=noises)
        return np.arange(len(w) * AD, dtype=np.float32).reshape(len(w), AD)
    monkeypatch.setattr(d, 'sample_actions_rows', rows_d)
    monkeypatch.setattr(g, 'sample_actions_rows', rows_g)
    want_out = np.arange(G * n * AD, dtype=np.float32).reshape(G, n, AD)   # row g n + j of the flat call is out[g, j]

    out = d.sample_actions_sweep(obs, cfgs, seed=5)
    np.testing.assert_array_equal(out, want_out)
    np.testing.assert_array_equal(seen['obs'], np.tile(obs, (G, 1)))
    np.testing.assert_array_equal(seen['w'], np.repeat(cfgs, n))
    assert seen['seed'] == 5 and seen['z'] is None and seen['w'].dtype == np.float32
    d.sample_actions_sweep(obs3, list(cfgs), noises=z)
    np.testing.assert_array_equal(seen['obs'], obs3.reshape(G * n, OD))
    np.testing.assert_array_equal(seen['z'], np.tile(z, (G, 1)))     # shared by every weight: common random numbers
    d.sample_actions_sweep(obs, cfgs, noises=z3)
    np.testing.assert_array_equal(seen['z'], z3.reshape(G * n, AD))

    out = g.sample_actions_sweep(obs, goals[0], cfgs, noises=z)
    np.testing.assert_array_equal(out, want_out)
    np.testing.assert_array_equal(seen['goals'], np.tile(goals[:1], (G * n, 1)))
    np.testing.assert_array_equal(seen['w'], np.repeat(cfgs, n))
    g.sample_actions_sweep(obs3, goals, cfgs)
    np.testing.assert_array_equal(seen['goals'], np.tile(goals, (G, 1)))
    np.testing.assert_array_equal(seen['obs'], obs3.reshape(G * n, OD))
    g.sample_actions_sweep(obs, goals3, cfgs)
    np.testing.assert_array_equal(seen['goals'], goals3.reshape(G * n, GD))
    with pytest.raises(ValueError):
        g.sample_actions_sweep(obs, None, cfgs)
    with pytest.raises(ValueError):
        g.sample_actions_sweep(obs, _f(G, n + 1, GD), cfgs)


def test_sweep_of_tensors_stays_in_torch(agents, monkeypatch):
    import torch
    d, _ = agents
    seen = {}

    def rows(observations, w, seed=None, noises=None):
        seen.update(obs=observations, w=w, z=noises)
        return torch.zeros(len(w), AD)
    monkeypatch.setattr(d, 'sample_actions_rows', rows)
    obs, cfgs, z = torch.randn(4, OD), torch.tensor([0.0, 3.0]), torch.randn(2, 4, AD)
    out = d.sample_actions_sweep(obs, cfgs, noises=z)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 4, AD)
    assert torch.equal(seen['obs'], obs.repeat(2, 1)) and torch.equal(seen['w'], torch.tensor([0.0] * 4 + [3.0] * 4))
    assert torch.equal(seen['z'], z.reshape(8, AD))
