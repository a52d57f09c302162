"""CPU: the ReBRAC group C ABI (fql_rebrac_group_*) is declared, exported and bound; its argument checks, ReBRACAgentGroup.create's and
sample_actions' run before any device call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_rebrac_group_create', 'fql_rebrac_group_update_from_dataset', 'fql_rebrac_group_sample_actions', 'fql_rebrac_group_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_rebrac_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_rebrac_group_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, z, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32), np.zeros((2, 1, 3), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    v = [C.c_int64(-1) for _ in range(3)]
    for full in (0, 1):
        assert lib.fql_rebrac_group_update_from_dataset(None, None, 256, full, None, None) == _cabi.FQL_E_INVALID
        assert b'NULL group' in lib.fql_last_error(None)
    assert lib.fql_rebrac_group_sample_actions(None, o.ctypes.data, 1, z.ctypes.data, seeds, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert lib.fql_rebrac_group_stats(None, *[C.byref(x) for x in v]) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert [x.value for x in v] == [-1, -1, -1]


def test_rebrac_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_rebrac_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert b'fql_rebrac_group_create' in lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        g = C.c_void_p(123)
        assert lib.fql_rebrac_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
        assert g.value is None
    assert lib.fql_rebrac_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_rebrac_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert b'out must not be NULL' in lib.fql_last_error(None)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine or to load the library fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import _cabi, agent as A, rebrac as R

    def boom(*a, **k):
        raise AssertionError('ReBRACAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(A.FQLAgent, 'create', classmethod(boom))
    monkeypatch.setattr(R.ReBRACAgent, 'create', classmethod(boom))
    monkeypatch.setattr(_cabi, 'load', boom)
    return fql_amd


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[0, 1], alpha_actors=[1.0]), ValueError),
    (dict(seeds=[0], alpha_actors=[1.0, 3.0]), ValueError),
    (dict(seeds=[0, 1], alpha_critics=[1.0]), ValueError),
    (dict(seeds=[0, 1], alpha_actors=[0.1, 0.2], alpha_critics=[1.0, 2.0, 3.0]), ValueError),
    (dict(seeds=[]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax_partitionable')), NotImplementedError),
])
def test_rebrac_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.rebrac.get_config()
    cfg.update(kw.get('cfg', {}))
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(exc):
        fql_amd.ReBRACAgentGroup.create(kw['seeds'], obs, act, cfg, alpha_actors=kw.get('alpha_actors'), alpha_critics=kw.get('alpha_critics'))


def test_rebrac_group_create_reaches_the_device_with_valid_arguments(no_device):
    """The refusals above are the checks', not a blanket one."""
    fql_amd = no_device
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.ReBRACAgentGroup.create([0, 1], obs, act, fql_amd.rebrac.get_config(), alpha_actors=[0.1, 0.2], alpha_critics=[0.0, 1.0])


def test_rebrac_group_is_exported():
    import fql_amd
    assert 'ReBRACAgentGroup' in fql_amd.__all__ and fql_amd.ReBRACAgentGroup is fql_amd.rebrac.ReBRACAgentGroup


K, OD, AD = 3, 5, 2


@pytest.fixture
def group():
    """A group object without a handle, over members that are not engines: a ValueError can only come from the Python checks."""
    from fql_amd import rebrac as R

    def boom(*a, **k):
        raise AssertionError('the device was touched before the arguments were validated')

    def member(i):
        m = types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, batch_size=16))
        m._sample_seed = lambda seed, noises: 0
        return m
    g = R.ReBRACAgentGroup.__new__(R.ReBRACAgentGroup)
    g._g, g.members, g.batch_size, g._keep = None, [member(i) for i in range(K)], 16, None
    g._lib = types.SimpleNamespace(fql_rebrac_group_sample_actions=boom, fql_rebrac_group_update_from_dataset=boom, fql_group_destroy=lambda h: 0)
    return g


def _f(*shape):
    return np.zeros(shape, np.float32)


@pytest.mark.parametrize('kw', [
    dict(observations=_f(K + 1, 4, OD)),                               # wrong leading K
    dict(observations=_f(K, 4, OD + 1)),                               # wrong last dim
    dict(observations=_f(OD + 1)),
    dict(observations=_f(K, 4, OD), seed=[1, 2]),                      # wrong number of seeds
    dict(observations=_f(K, 4, OD), noises=_f(K, 5, AD)),              # noises against the rows
    dict(observations=_f(K, 4, OD), noises=_f(K, 4, AD + 1)),
    dict(observations=_f(K, 4, OD), noises=_f(4, AD)),                 # (noises are never shared between the members)
    dict(observations=_f(4, OD), noises=_f(K, 5, AD)),                 # shared rows, noises per member
    dict(observations=_f(K, 0, OD)),                                   # no rows
], ids=lambda kw: '-'.join(f'{k}{np.shape(v)}' for k, v in kw.items()))
def test_rebrac_group_sample_actions_checks_shapes_before_the_library(group, kw):
    with pytest.raises(ValueError):
        group.sample_actions(temperature=0.5, **kw)


def test_rebrac_group_sample_actions_reaches_the_library_with_valid_shapes(group):
    for kw in (dict(observations=_f(K, 4, OD)), dict(observations=_f(4, OD), seed=3), dict(observations=_f(K, OD), seed=[1, 2, 3]),
               dict(observations=_f(K, 2, 2, OD), noises=_f(K, 2, 2, AD)), dict(observations=_f(OD))):
        with pytest.raises(AssertionError, match='device was touched'):
            group.sample_actions(**kw)


def test_rebrac_group_update_checks_batch_size_and_rows_before_the_library(group):
    with pytest.raises(ValueError):
        group.update_from_dataset(batch_size=32)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, 16), np.int64))
