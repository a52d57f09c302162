"""CPU: the IQL group C ABI (fql_iql_group_*) is declared, exported and bound; its argument checks, IQLAgentGroup.create's and the
shape and seed checks of sample_actions and update_from_dataset run before any device call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_iql_group_create', 'fql_iql_group_update_from_dataset', 'fql_iql_group_sample_actions', 'fql_iql_group_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_iql_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_iql_group_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, z, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32), np.zeros((2, 1, 3), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    u, s = C.c_int64(-1), C.c_int64(-1)
    assert lib.fql_iql_group_update_from_dataset(None, None, 256, None, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_iql_group_update_from_dataset' in lib.fql_last_error(None)
    assert lib.fql_iql_group_sample_actions(None, o.ctypes.data, 1, z.ctypes.data, seeds, 1.0, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_iql_group_sample_actions' in lib.fql_last_error(None)
    assert lib.fql_iql_group_stats(None, C.byref(u), C.byref(s)) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_iql_group_stats' in lib.fql_last_error(None)
    assert (u.value, s.value) == (-1, -1)
    assert not out.any()


def test_iql_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_iql_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert b'fql_iql_group_create' in lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        g = C.c_void_p(123)
        assert lib.fql_iql_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
        assert g.value is None
    assert lib.fql_iql_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_iql_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert b'out must not be NULL' in lib.fql_last_error(None)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine or to load the library fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import _cabi, iql as Q

    def boom(*a, **k):
        raise AssertionError('IQLAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(Q.IQLAgent, 'create', classmethod(boom))
    monkeypatch.setattr(_cabi, 'load', boom)
    return fql_amd


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[0, 1], expectiles=[0.7]), ValueError),
    (dict(seeds=[0], expectiles=[0.7, 0.9]), ValueError),
    (dict(seeds=[0, 1], alphas=[1.0]), ValueError),
    (dict(seeds=[0, 1], alphas=[]), ValueError),
    (dict(seeds=[0, 1], expectiles=[0.7, 0.9], alphas=[0.3, 1.0, 3.0]), ValueError),
    (dict(seeds=[]), ValueError),
    (dict(seeds=[], expectiles=[], alphas=[]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(actor_loss='sac')), ValueError),
])
def test_iql_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.iql.get_config()
    cfg.update(kw.get('cfg', {}))
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(exc):
        fql_amd.IQLAgentGroup.create(kw['seeds'], obs, act, cfg, expectiles=kw.get('expectiles'), alphas=kw.get('alphas'))


def test_iql_group_create_reaches_the_device_with_valid_arguments(no_device):
    """The refusals above are the checks', not a blanket one."""
    fql_amd = no_device
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.IQLAgentGroup.create([1, 2, 3], obs, act, fql_amd.iql.get_config(), expectiles=[0.7, 0.8, 0.9], alphas=[0.3, 1.0, 3.0])
    for loss in ('awr', 'ddpgbc'):
        with pytest.raises(AssertionError, match='touched the device'):
            fql_amd.IQLAgentGroup.create([1, 2], obs, act, dict(fql_amd.iql.get_config(), actor_loss=loss))


def test_iql_group_is_exported():
    import fql_amd
    assert 'IQLAgentGroup' in fql_amd.__all__ and fql_amd.IQLAgentGroup is fql_amd.iql.IQLAgentGroup
    assert 'IQLAgentGroup' in fql_amd.iql.__all__


def test_fql_group_points_iql_configs_to_the_iql_group(monkeypatch):
    """FQLAgentGroup keeps refusing an IQL config, before the library, and names the class that takes it."""
    import fql_amd
    from fql_amd import _cabi

    def boom(*a, **k):
        raise AssertionError('touched the device')
    monkeypatch.setattr(_cabi, 'load', boom)
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(NotImplementedError, match='IQLAgentGroup'):
        fql_amd.FQLAgentGroup.create([0, 1], obs, act, fql_amd.iql.get_config())


K, OD, AD = 3, 5, 2


@pytest.fixture
def group():
    """A group object without a handle, over members that are not engines: a ValueError can only come from the Python checks.  The
    library calls record what they were handed and then fail the test's way."""
    from fql_amd import iql as Q

    seen = {}

    def sample(g, o, n, z, seeds, temperature, out, stream):
        seen.update(n=n, noises=z, seeds=None if seeds is None else list(seeds), temperature=temperature)
        raise AssertionError('the device was touched')

    def boom(*a, **k):
        raise AssertionError('the device was touched')

    def member(i):
        m = types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, batch_size=16), calls=0)

        def seed_of(seed, noises):
            m.calls += 1
            return 100 * i + (0 if seed is None else int(seed))
        m._sample_seed = seed_of
        return m
    g = Q.IQLAgentGroup.__new__(Q.IQLAgentGroup)
    g._g, g.members, g.batch_size, g._keep = None, [member(i) for i in range(K)], 16, None
    g._lib = types.SimpleNamespace(fql_iql_group_sample_actions=sample, fql_iql_group_update_from_dataset=boom, fql_group_destroy=lambda h: 0)
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
], ids=lambda kw: '-'.join(f'{k}{np.shape(v)}' for k, v in kw.items()))
def test_iql_group_sample_actions_checks_shapes_before_the_library(group, kw):
    with pytest.raises(ValueError):
        group.sample_actions(**kw)
    assert not group.seen


def test_iql_group_sampling_reaches_the_library_with_valid_shapes(group):
    for kw, n, seeds, temp in ((dict(observations=_f(K, 4, OD), noises=_f(K, 4, AD)), 4, None, 1.0),
                               (dict(observations=_f(4, OD), noises=_f(K, 4, AD)), 4, None, 1.0),             # shared rows
                               (dict(observations=_f(OD), noises=_f(K, AD)), 1, None, 1.0),                   # one shared observation
                               (dict(observations=_f(K, 2, 2, OD), noises=_f(K, 2, 2, AD), temperature=0.5), 4, None, 0.5),
                               (dict(observations=_f(K, 4, OD), seed=7), 4, [7, 107, 207], 1.0),              # one seed: keyed per member as its own call
                               (dict(observations=_f(K, 4, OD), seed=[1, 2, 3]), 4, [1, 102, 203], 1.0),
                               (dict(observations=_f(4, OD), seed=5, temperature=0.0), 4, [5, 105, 205], 0.0),
                               (dict(observations=_f(K, OD)), 1, [0, 100, 200], 1.0)):                        # one row each; each member's own counter
        with pytest.raises(AssertionError, match='device was touched'):
            group.sample_actions(**kw)
        assert group.seen['n'] == n and group.seen['seeds'] == seeds and group.seen['temperature'] == temp, kw
        assert (group.seen['noises'] is None) == ('noises' not in kw)
    assert [m.calls for m in group.members] == [4] * K   # the four seeded or counted calls, none of the calls with noises


def test_iql_group_update_checks_batch_size_and_rows_before_the_library(group):
    with pytest.raises(ValueError):
        group.update_from_dataset(batch_size=32)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, 16), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K, 17), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((16,), np.int64))
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset()
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset(batch_size=16, want_info=True)
