"""CPU: the IQL-diffusion group C ABI (fql_iqld_group_*) is declared, exported and bound; its argument checks, IQLDiffusionAgentGroup.create's
and the shape, seed and cfg checks of sample_actions run before any device call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_iqld_group_create', 'fql_iqld_group_update_from_dataset', 'fql_iqld_group_sample_actions', 'fql_iqld_group_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_iqld_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_iqld_group_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, z, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32), np.zeros((2, 1, 3), np.float32)
    w = np.ones((2, 1), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    la, s = (C.c_int64 * 4)(-1, -1, -1, -1), C.c_int64(-1)
    for uc in (0, 1):
        for ua in (0, 1):
            assert lib.fql_iqld_group_update_from_dataset(None, None, 256, uc, ua, None, None) == _cabi.FQL_E_INVALID
            assert b'NULL group' in lib.fql_last_error(None) and b'fql_iqld_group_update_from_dataset' in lib.fql_last_error(None)
    assert lib.fql_iqld_group_sample_actions(None, o.ctypes.data, 1, z.ctypes.data, seeds, w.ctypes.data, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert lib.fql_iqld_group_stats(None, la, C.byref(s)) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None)
    assert list(la) == [-1] * 4 and s.value == -1


def test_iqld_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_iqld_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert b'fql_iqld_group_create' in lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        g = C.c_void_p(123)
        assert lib.fql_iqld_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
        assert g.value is None
    assert lib.fql_iqld_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_iqld_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert b'out must not be NULL' in lib.fql_last_error(None)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine or to load the library fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import _cabi, iql_diffusion as D

    def boom(*a, **k):
        raise AssertionError('IQLDiffusionAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(D.IQLDiffusionAgent, 'create', classmethod(boom))
    monkeypatch.setattr(_cabi, 'load', boom)
    return fql_amd


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[0, 1], softmax_betas=[1.0]), ValueError),
    (dict(seeds=[0], softmax_betas=[1.0, 3.0]), ValueError),
    (dict(seeds=[0, 1], awr_temperatures=[1.0]), ValueError),
    (dict(seeds=[0, 1], awr_temperatures=[0.1, 0.2], softmax_betas=[1.0, 2.0, 3.0]), ValueError),
    (dict(seeds=[]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
])
def test_iqld_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.iql_diffusion.get_config()
    cfg.update(kw.get('cfg', {}))
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(exc):
        fql_amd.IQLDiffusionAgentGroup.create(kw['seeds'], obs, act, cfg, awr_temperatures=kw.get('awr_temperatures'),
                                              softmax_betas=kw.get('softmax_betas'))


def test_iqld_group_create_reaches_the_device_with_valid_arguments(no_device):
    """The refusals above are the checks', not a blanket one."""
    fql_amd = no_device
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.IQLDiffusionAgentGroup.create([1, 2, 3], obs, act, fql_amd.iql_diffusion.get_config(), softmax_betas=[1.0, 2.0, 3.0])


def test_iqld_group_is_exported():
    import fql_amd
    assert 'IQLDiffusionAgentGroup' in fql_amd.__all__ and fql_amd.IQLDiffusionAgentGroup is fql_amd.iql_diffusion.IQLDiffusionAgentGroup


K, OD, AD = 3, 5, 2


@pytest.fixture
def group():
    """A group object without a handle, over members that are not engines: a ValueError can only come from the Python checks.  The
    library call records the weights it was handed and then fails the test's way."""
    from fql_amd import iql_diffusion as D

    seen = {}

    def sample(g, o, n, z, seeds, w, out, stream):
        seen['cfgs'] = np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_float)), shape=(K * n,)).reshape(K, n).copy()
        raise AssertionError('the device was touched')

    def boom(*a, **k):
        raise AssertionError('the device was touched')

    def member(i):
        m = types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, batch_size=16), calls=0)

        def seed_of(seed, noises):
            m.calls += 1
            return 0
        m._sample_seed = seed_of
        return m
    g = D.IQLDiffusionAgentGroup.__new__(D.IQLDiffusionAgentGroup)
    g._g, g.members, g.batch_size, g._keep = None, [member(i) for i in range(K)], 16, None
    g._lib = types.SimpleNamespace(fql_iqld_group_sample_actions=sample, fql_iqld_group_update_from_dataset=boom, fql_group_destroy=lambda h: 0)
    g.seen = seen
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
    dict(observations=_f(K, 4, OD), cfg=np.ones(K + 1, np.float32)),   # one weight per member: wrong K
    dict(observations=_f(K, 4, OD), cfg=np.ones((K, 5), np.float32)),  # one weight per row: wrong n
    dict(observations=_f(K, 4, OD), cfg=np.ones((4,), np.float32)),    # [n] is not a shape: per member or per member and row
    dict(observations=_f(K, 4, OD), cfg=float('nan')),                 # non-finite: scalar, per member, per row
    dict(observations=_f(K, 4, OD), cfg=[1.0, float('inf'), 2.0]),
    dict(observations=_f(K, 4, OD), cfg=np.where(np.arange(K * 4).reshape(K, 4) == 7, -np.inf, 1.0)),
    dict(observations=_f(4, OD), seed=3, cfg=[1.0, 2.0]),              # shared rows, wrong K
], ids=lambda kw: '-'.join(f'{k}{np.shape(v)}' for k, v in kw.items()))
def test_iqld_group_sample_actions_checks_shapes_and_cfg_before_the_library(group, kw):
    with pytest.raises(ValueError):
        group.sample_actions(**kw)


def test_iqld_group_a_non_finite_cfg_is_refused_before_a_seed_counter_moves(group):
    with pytest.raises(ValueError, match='finite'):
        group.sample_actions(_f(K, 4, OD), cfg=[1.0, float('nan'), 2.0])
    assert [m.calls for m in group.members] == [0] * K


def test_iqld_group_sample_actions_broadcasts_cfg_and_reaches_the_library(group):
    per_row = np.arange(K * 4, dtype=np.float32).reshape(K, 4)
    for kw, want in ((dict(observations=_f(K, 4, OD)), np.ones((K, 4))),                                   # the default: cfg 1
                     (dict(observations=_f(K, 4, OD), cfg=3.0), np.full((K, 4), 3.0)),
                     (dict(observations=_f(K, 4, OD), cfg=0), np.zeros((K, 4))),
                     (dict(observations=_f(K, 4, OD), cfg=[1.0, 2.0, 3.0]), np.repeat([[1.0], [2.0], [3.0]], 4, axis=1)),
                     (dict(observations=_f(K, 4, OD), cfg=per_row), per_row),
                     (dict(observations=_f(4, OD), seed=3, cfg=[0.5, 1.5, 2.5]), np.repeat([[0.5], [1.5], [2.5]], 4, axis=1)),   # shared rows
                     (dict(observations=_f(K, OD), seed=[1, 2, 3], cfg=[1.0, 2.0, 3.0]), np.array([[1.0], [2.0], [3.0]])),      # one row each: [K] is per member
                     (dict(observations=_f(K, 2, 2, OD), noises=_f(K, 2, 2, AD), cfg=per_row.reshape(K, 2, 2)), per_row),
                     (dict(observations=_f(OD), cfg=2.0), np.full((K, 1), 2.0))):
        with pytest.raises(AssertionError, match='device was touched'):
            group.sample_actions(**kw)
        np.testing.assert_array_equal(group.seen['cfgs'], want.astype(np.float32), err_msg=str(kw.get('cfg')))


def test_iqld_group_update_checks_batch_size_and_rows_before_the_library(group):
    with pytest.raises(ValueError):
        group.update_from_dataset(batch_size=32)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, 16), np.int64))
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset(update_critic=False, update_actor=False)
