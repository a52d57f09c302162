"""CPU: the SAC group C ABI (fql_sac_group_*) is declared, exported and bound; its NULL-argument checks, SACAgentGroup.create's
refusals and the batch-size, shape and range checks of update_from_dataset and update_balanced run before any device call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_sac_group_create', 'fql_sac_group_update_from_dataset', 'fql_sac_group_update_balanced',
             'fql_sac_group_sample_actions', 'fql_sac_group_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_sac_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_sac_group_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, z, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32), np.zeros((2, 1, 3), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    u, s = C.c_int64(-1), C.c_int64(-1)
    for call, name in ((lambda: lib.fql_sac_group_update_from_dataset(None, None, 256, None, None), b'fql_sac_group_update_from_dataset'),
                       (lambda: lib.fql_sac_group_update_balanced(None, None, None, 256, None, None), b'fql_sac_group_update_balanced'),
                       (lambda: lib.fql_sac_group_sample_actions(None, o.ctypes.data, 1, z.ctypes.data, seeds, 1.0, out.ctypes.data, None),
                        b'fql_sac_group_sample_actions'),
                       (lambda: lib.fql_sac_group_stats(None, C.byref(u), C.byref(s)), b'fql_sac_group_stats')):
        assert call() == _cabi.FQL_E_INVALID
        assert b'NULL group' in lib.fql_last_error(None) and name in lib.fql_last_error(None)
    assert (u.value, s.value) == (-1, -1)
    assert not out.any()


def test_sac_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_sac_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert b'fql_sac_group_create' in lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        g = C.c_void_p(123)
        assert lib.fql_sac_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
        assert g.value is None
    assert lib.fql_sac_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_sac_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert b'out must not be NULL' in lib.fql_last_error(None)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine or to load the library fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import _cabi, sac as S

    def boom(*a, **k):
        raise AssertionError('SACAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(S.SACAgent, 'create', classmethod(boom))
    monkeypatch.setattr(_cabi, 'load', boom)
    return fql_amd


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[]), ValueError),
    (dict(seeds=[], target_entropies=[]), ValueError),
    (dict(seeds=[0, 1], target_entropies=[-4.0]), ValueError),
    (dict(seeds=[0], target_entropies=[-4.0, -2.0]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(state_dependent_std=False)), NotImplementedError),
])
def test_sac_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.sac.get_config()
    cfg.update(kw.get('cfg', {}))
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(exc):
        fql_amd.SACAgentGroup.create(kw['seeds'], obs, act, cfg, target_entropies=kw.get('target_entropies'))


def test_sac_group_create_reaches_the_device_with_valid_arguments(no_device):
    """The refusals above are the checks', not a blanket one."""
    fql_amd = no_device
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.SACAgentGroup.create([1, 2, 3], obs, act, fql_amd.sac.get_config(), target_entropies=[-4.0, None, -1.0])
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.SACAgentGroup.create([1, 2], obs, act, fql_amd.sac.get_config())


def test_sac_agent_create_still_refuses_a_vector_std_before_the_library(monkeypatch):
    """The refusal moved into SACAgent._refuse_config: the single agent's create raises what it raised."""
    import fql_amd
    from fql_amd import _cabi

    def boom(*a, **k):
        raise AssertionError('touched the device')
    monkeypatch.setattr(_cabi, 'load', boom)
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(NotImplementedError, match='state_dependent_std'):
        fql_amd.SACAgent.create(0, obs, act, dict(fql_amd.sac.get_config(), state_dependent_std=False))


def test_sac_group_is_exported():
    import fql_amd
    assert 'SACAgentGroup' in fql_amd.__all__ and fql_amd.SACAgentGroup is fql_amd.sac.SACAgentGroup
    assert 'SACAgentGroup' in fql_amd.sac.__all__


def test_fql_group_points_sac_configs_to_the_sac_group(monkeypatch):
    """FQLAgentGroup keeps refusing a SAC config, before the library, and names the class that takes it."""
    import fql_amd
    from fql_amd import _cabi

    def boom(*a, **k):
        raise AssertionError('touched the device')
    monkeypatch.setattr(_cabi, 'load', boom)
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(NotImplementedError, match='SACAgentGroup'):
        fql_amd.FQLAgentGroup.create([0, 1], obs, act, fql_amd.sac.get_config())


K, OD, AD, B = 3, 5, 2, 16
DS_ROWS, RING_ROWS = 40, (3, 8, 5)


@pytest.fixture
def group():
    """A group object without a handle, over members that are not engines (datasets of 40 rows, rings of 3, 8 and 5): a ValueError can
    only come from the Python checks.  The library calls record what they were handed and then fail the test's way."""
    from fql_amd import sac as S

    seen = {}

    def balanced(g, ia, ib, b, info, stream):
        seen.update(ia=ia, ib=ib, B=b)
        raise AssertionError('the device was touched')

    def boom(*a, **k):
        raise AssertionError('the device was touched')

    def member(i):
        return types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, batch_size=B), dataset_size=lambda: (DS_ROWS, 0),
                                     replay_size=lambda: (RING_ROWS[i], RING_ROWS[i] % 8))
    g = object.__new__(S.SACAgentGroup)
    g._g, g.members, g.batch_size, g._keep = None, [member(i) for i in range(K)], B, None
    g._lib = types.SimpleNamespace(fql_sac_group_update_balanced=balanced, fql_sac_group_update_from_dataset=boom, fql_group_destroy=lambda h: 0)
    g.seen = seen
    return g


def _ok():
    return np.zeros((K, B // 2), np.int64), np.zeros((K, B // 2), np.int64)


def test_sac_group_update_balanced_checks_batch_size_shapes_and_ranges_before_the_library(group):
    d, r = _ok()
    with pytest.raises(ValueError, match='batch size'):
        group.update_balanced(batch_size=32)
    with pytest.raises(ValueError, match='batch size'):
        group.update_balanced(batch_size=32, idxs=(d, r))
    for bad in ((d[:2], r), (d, r[:2]), (np.zeros((K, B), np.int64), r), (d, np.zeros((K, B // 2 + 1), np.int64)), (d.ravel(), r.ravel()),
                (d,), (d, r, r)):
        with pytest.raises(ValueError):
            group.update_balanced(idxs=bad)
    # ranges: against each member's own dataset and its own ring
    for row, col, what in ((0, 0, 'dataset'), (2, 7, 'dataset')):
        d, r = _ok()
        d[row, col] = DS_ROWS
        with pytest.raises(ValueError, match=f'dataset idxs.{row}. out of range'):
            group.update_balanced(idxs=(d, r))
        d[row, col] = -1
        with pytest.raises(ValueError, match='out of range'):
            group.update_balanced(idxs=(d, r))
    for i in range(K):
        d, r = _ok()
        r[i, 3] = RING_ROWS[i]          # one past member i's ring; within another member's where that one is larger
        with pytest.raises(ValueError, match=f'replay idxs.{i}. out of range'):
            group.update_balanced(idxs=(d, r))
        r[i, 3] = -1
        with pytest.raises(ValueError, match='out of range'):
            group.update_balanced(idxs=(d, r))
    assert not group.seen


def test_sac_group_update_balanced_reaches_the_library_with_valid_rows(group):
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_balanced()
    assert group.seen == dict(ia=None, ib=None, B=B)
    d, r = _ok()
    d[:] = DS_ROWS - 1
    for i in range(K):
        r[i] = RING_ROWS[i] - 1
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_balanced(batch_size=B, idxs=(d, r), want_info=True)
    assert group.seen['ia'] and group.seen['ib'] and group.seen['B'] == B
    # lists and int32 arrays are taken as int64 rows
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_balanced(idxs=(d.astype(np.int32), r.tolist()))


def test_sac_group_update_from_dataset_checks_batch_size_and_rows_before_the_library(group):
    with pytest.raises(ValueError):
        group.update_from_dataset(batch_size=32)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K, B + 1), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), DS_ROWS, np.int64))
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset()
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset(batch_size=B, want_info=True)


def test_sac_group_add_transitions_takes_one_transition_per_member(group):
    with pytest.raises(ValueError):
        group.add_transitions([{}] * (K + 1))
    got = []
    for i, m in enumerate(group.members):
        m.add_transition = lambda t, replay=False, i=i: got.append((i, t['k'], replay))
    group.add_transitions([dict(k=10 + i) for i in range(K)])
    assert got == [(i, 10 + i, True) for i in range(K)]
