"""CPU: the agent-group C ABI (fql_group_*) is declared, exported and bound; its argument checks and FQLAgentGroup.create's run before
any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_group_create', 'fql_group_destroy', 'fql_group_update_from_dataset', 'fql_group_synchronize')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    assert 'typedef struct fql_group_s* fql_group;' in src
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        assert lib.fql_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
    assert lib.fql_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert lib.fql_group_update_from_dataset(None, None, 256, None, None) == _cabi.FQL_E_INVALID
    assert lib.fql_group_synchronize(None) == _cabi.FQL_E_INVALID
    assert lib.fql_group_destroy(None) == _cabi.FQL_OK


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import agent as A

    def boom(*a, **k):
        raise AssertionError('FQLAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(A.FQLAgent, 'create', classmethod(boom))
    return fql_amd


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[0, 1], alphas=[1.0]), ValueError),
    (dict(seeds=[0], alphas=[1.0, 3.0]), ValueError),
    (dict(seeds=[]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax_partitionable')), NotImplementedError),
])
def test_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.get_config()
    cfg.update(kw.get('cfg', {}))
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(exc):
        fql_amd.FQLAgentGroup.create(kw['seeds'], obs, act, cfg, alphas=kw.get('alphas'))


def test_group_is_exported():
    import fql_amd
    assert 'FQLAgentGroup' in fql_amd.__all__ and fql_amd.FQLAgentGroup is fql_amd.agent.FQLAgentGroup
