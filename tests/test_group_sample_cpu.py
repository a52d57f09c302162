"""CPU: the group sampling C ABI (fql_group_sample_actions, fql_group_flow_actions, fql_group_sample_stats) is declared, exported and
bound, refuses a NULL group, and FQLAgentGroup.sample_actions / compute_flow_actions check their shapes before the library is called."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_FNS = ('fql_group_sample_actions', 'fql_group_flow_actions', 'fql_group_sample_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_group_sample_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in SAMPLE_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_group_sample_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, z, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32), np.zeros((2, 1, 3), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    v = C.c_int64(-1)
    assert lib.fql_group_sample_actions(None, o.ctypes.data, 1, z.ctypes.data, seeds, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert lib.fql_group_flow_actions(None, o.ctypes.data, z.ctypes.data, 1, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert lib.fql_group_sample_stats(None, 0, C.byref(v)) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert v.value == -1


K, OD, AD = 3, 5, 2


@pytest.fixture
def group(monkeypatch):
    """A group object without a handle, over members that are not engines: any engine creation or library call fails the test, so a
    ValueError can only come from the Python checks."""
    from fql_amd import agent as A

    def boom(*a, **k):
        raise AssertionError('the device was touched before the arguments were validated')
    monkeypatch.setattr(A.FQLAgent, 'create', classmethod(boom))

    def member(i):
        m = types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, batch_size=16), calls=0)
        m._sample_seed = lambda seed, noises: 0
        return m
    g = A.FQLAgentGroup(None, [member(i) for i in range(K)])
    g._lib = types.SimpleNamespace(fql_group_sample_actions=boom, fql_group_flow_actions=boom, fql_group_destroy=lambda h: 0)
    return g


def _f(*shape):
    return np.zeros(shape, np.float32)


@pytest.mark.parametrize('kw', [
    dict(observations=_f(K + 1, 4, OD)),                               # wrong leading K
    dict(observations=_f(K - 1, 2, 4, OD)),
    dict(observations=_f(K, 4, OD + 1)),                               # wrong last dim
    dict(observations=_f(OD + 1)),
    dict(observations=_f(K, 4, OD), seed=[1, 2]),                      # wrong number of seeds
    dict(observations=_f(K, 4, OD), seed=list(range(K + 1))),
    dict(observations=_f(K, 4, OD), noises=_f(K, 5, AD)),              # noises against the rows
    dict(observations=_f(K, 4, OD), noises=_f(K, 4, AD + 1)),
    dict(observations=_f(K, 4, OD), noises=_f(K - 1, 4, AD)),
    dict(observations=_f(K, 4, OD), noises=_f(4, AD)),                 # (noises are never shared between the members)
    dict(observations=_f(4, OD), noises=_f(K, 5, AD)),                 # shared rows, noises per member
    dict(observations=_f(K, 0, OD)),                                   # no rows
], ids=lambda kw: '-'.join(f'{k}{np.shape(v)}' for k, v in kw.items()))
def test_group_sample_actions_checks_shapes_before_the_library(group, kw):
    with pytest.raises(ValueError):
        group.sample_actions(**kw)


@pytest.mark.parametrize('o, z', [
    (_f(K + 1, 4, OD), _f(K + 1, 4, AD)),
    (_f(K, 4, OD + 1), _f(K, 4, AD)),
    (_f(K, 4, OD), _f(K, 3, AD)),
    (_f(K, 4, OD), None),
], ids=['leading-K', 'last-dim', 'noise-rows', 'no-noises'])
def test_group_flow_actions_checks_shapes_before_the_library(group, o, z):
    with pytest.raises(ValueError):
        group.compute_flow_actions(o, z)


def test_group_sample_actions_reaches_the_library_with_valid_shapes(group):
    """The refusals above are the checks', not a blanket one: valid shapes get as far as the library call."""
    for kw in (dict(observations=_f(K, 4, OD)), dict(observations=_f(4, OD), seed=3), dict(observations=_f(K, OD), seed=[1, 2, 3]),
               dict(observations=_f(K, 2, 2, OD), noises=_f(K, 2, 2, AD)), dict(observations=_f(OD))):
        with pytest.raises(AssertionError, match='device was touched'):
            group.sample_actions(**kw)
