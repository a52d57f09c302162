"""CPU: the CFGRL group C ABI (fql_cfgrl_group_*) is declared, exported and bound; its argument checks, CFGRLAgentGroup.create's and the
shape, goal, weight and seed checks of sample_actions and update_from_dataset run before any device call."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_FNS = ('fql_cfgrl_group_create', 'fql_cfgrl_group_update_from_dataset', 'fql_cfgrl_group_sample_actions', 'fql_cfgrl_group_stats')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_cfgrl_group_functions_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = open(os.path.join(ROOT, 'include', 'fql_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for n in GROUP_FNS:
        assert re.search(r'\bint\s+' + n + r'\s*\(', code), n
        assert hasattr(lib, n), n
        assert n in _cabi.SYMBOLS, n


def test_cfgrl_group_functions_reject_a_null_group(lib):
    from fql_amd import _cabi
    o, gl, out = np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 5), np.float32), np.zeros((2, 1, 3), np.float32)
    z, w = np.zeros((2, 1, 3), np.float32), np.ones((2, 1), np.float32)
    seeds = (C.c_uint64 * 2)(1, 2)
    u, s = C.c_int64(-1), C.c_int64(-1)
    assert lib.fql_cfgrl_group_update_from_dataset(None, None, 256, None, None, None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_cfgrl_group_update_from_dataset' in lib.fql_last_error(None)
    assert lib.fql_cfgrl_group_sample_actions(None, o.ctypes.data, gl.ctypes.data, 1, z.ctypes.data, seeds, w.ctypes.data, out.ctypes.data,
                                              None) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_cfgrl_group_sample_actions' in lib.fql_last_error(None)
    assert lib.fql_cfgrl_group_stats(None, C.byref(u), C.byref(s)) == _cabi.FQL_E_INVALID
    assert b'NULL group' in lib.fql_last_error(None) and b'fql_cfgrl_group_stats' in lib.fql_last_error(None)
    assert (u.value, s.value) == (-1, -1)
    assert not out.any()


def test_cfgrl_group_create_rejects_null_empty_and_nonpositive_k(lib):
    from fql_amd import _cabi
    g = C.c_void_p(123)
    assert lib.fql_cfgrl_group_create(None, 2, C.byref(g)) == _cabi.FQL_E_INVALID
    assert g.value is None
    assert b'fql_cfgrl_group_create' in lib.fql_last_error(None)
    empty = (C.c_void_p * 1)()
    for k in (0, -1):
        g = C.c_void_p(123)
        assert lib.fql_cfgrl_group_create(empty, k, C.byref(g)) == _cabi.FQL_E_INVALID
        assert g.value is None
    assert lib.fql_cfgrl_group_create(empty, 1, C.byref(g)) == _cabi.FQL_E_INVALID   # a NULL member
    assert b'NULL' in lib.fql_last_error(None)
    assert lib.fql_cfgrl_group_create(empty, 1, None) == _cabi.FQL_E_INVALID
    assert b'out must not be NULL' in lib.fql_last_error(None)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to create an engine or to load the library fails the test: the checks must come first."""
    import fql_amd
    from fql_amd import _cabi, cfgrl as G

    def boom(*a, **k):
        raise AssertionError('CFGRLAgentGroup.create touched the device before validating its arguments')
    monkeypatch.setattr(G.CFGRLAgent, 'create', classmethod(boom))
    monkeypatch.setattr(_cabi, 'load', boom)
    return fql_amd


def _example(od=29, ad=8, gd=29):
    return {'observations': np.zeros((1, od), np.float32), 'actions': np.zeros((1, ad), np.float32), 'value_goals': np.zeros((1, gd), np.float32)}


@pytest.mark.parametrize('kw, exc', [
    (dict(seeds=[0, 1], cfgs=[3.0]), ValueError),
    (dict(seeds=[0], cfgs=[1.5, 3.0]), ValueError),
    (dict(seeds=[0, 1], cfgs=[]), ValueError),
    (dict(seeds=[0, 1], cfgs=[3.0, float('nan')]), ValueError),
    (dict(seeds=[0, 1], cfgs=[float('inf'), 3.0]), ValueError),
    (dict(seeds=[0, 1], goal_mixes=[(0.0, 1.0, 0.0)]), ValueError),
    (dict(seeds=[0, 1], goal_mixes=[]), ValueError),
    (dict(seeds=[0, 1], cfgs=[1.0, 3.0], goal_mixes=[(0.0, 1.0, 0.0)] * 3), ValueError),
    (dict(seeds=[0, 1], goal_mixes=[(0.0, 1.0, 0.0), (0.2, 0.5, 0.2)]), ValueError),        # sums to 0.9
    (dict(seeds=[0, 1], goal_mixes=[(0.5, 0.6, 0.0), (0.0, 1.0, 0.0)]), ValueError),        # sums to 1.1
    (dict(seeds=[0, 1], goal_mixes=[(0.0, 1.0, 0.0), (1.5, -0.5, 0.0)]), ValueError),       # sums to 1 with a negative entry
    (dict(seeds=[0, 1], goal_mixes=[(0.0, 1.0), (0.0, 1.0)]), ValueError),                  # pairs, not triples
    (dict(seeds=[]), ValueError),
    (dict(seeds=[], cfgs=[], goal_mixes=[]), ValueError),
    (dict(seeds=[0, 1], cfg=dict(actor_p_trajgoal=0.5)), ValueError),                       # the config's own mixture
    (dict(seeds=[0, 1], cfg=dict(flow_steps=0)), ValueError),
    (dict(seeds=[0, 1], cfg=dict(encoder='impala_small')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(precision='bf16x3')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(rng='jax')), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(actor_geom_sample=True)), NotImplementedError),
    (dict(seeds=[0, 1], cfg=dict(frame_stack=3)), NotImplementedError),
    (dict(seeds=[0, 1], drop='value_goals'), KeyError),
])
def test_cfgrl_group_create_validates_before_any_device_call(no_device, kw, exc):
    fql_amd = no_device
    cfg = fql_amd.cfgrl.get_config()
    cfg.update(kw.get('cfg', {}))
    ex = _example()
    ex.pop(kw.get('drop'), None)
    with pytest.raises(exc):
        fql_amd.CFGRLAgentGroup.create(kw['seeds'], ex, cfg, cfgs=kw.get('cfgs'), goal_mixes=kw.get('goal_mixes'))


def test_cfgrl_group_create_reaches_the_device_with_valid_arguments(no_device):
    """The refusals above are the checks', not a blanket one."""
    fql_amd = no_device
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.CFGRLAgentGroup.create([1, 2, 3], _example(), fql_amd.cfgrl.get_config(), cfgs=[1.5, 3.0, 5.0],
                                       goal_mixes=[(1.0, 0.0, 0.0), (0.0, 0.5, 0.5), (0.2, 0.5, 0.3)])
    with pytest.raises(AssertionError, match='touched the device'):
        fql_amd.CFGRLAgentGroup.create([1, 2], _example(gd=2), fql_amd.cfgrl.get_config())


def test_cfgrl_group_is_exported():
    import fql_amd
    assert 'CFGRLAgentGroup' in fql_amd.__all__ and fql_amd.CFGRLAgentGroup is fql_amd.cfgrl.CFGRLAgentGroup
    assert 'CFGRLAgentGroup' in fql_amd.cfgrl.__all__


def test_fql_group_points_cfgrl_configs_to_the_cfgrl_group(monkeypatch):
    """FQLAgentGroup keeps refusing a CFGRL config, before the library, and names the class that takes it."""
    import fql_amd
    from fql_amd import _cabi

    def boom(*a, **k):
        raise AssertionError('touched the device')
    monkeypatch.setattr(_cabi, 'load', boom)
    obs, act = np.zeros((1, 29), np.float32), np.zeros((1, 8), np.float32)
    with pytest.raises(NotImplementedError, match='CFGRLAgentGroup'):
        fql_amd.FQLAgentGroup.create([0, 1], obs, act, fql_amd.cfgrl.get_config())


K, OD, AD, GD, B = 3, 5, 2, 4, 16


@pytest.fixture
def group():
    """A group object without a handle, over members that are not engines: a ValueError can only come from the Python checks.  The
    library calls record what they were handed and then fail the test's way."""
    from fql_amd import cfgrl as G

    seen = {}

    def sample(g, o, gl, n, z, seeds, w, out, stream):
        weights = np.ctypeslib.as_array(C.cast(w, C.POINTER(C.c_float)), shape=(K * n,)).reshape(K, n).copy()
        goals = np.ctypeslib.as_array(C.cast(gl, C.POINTER(C.c_float)), shape=(K * n * GD,)).reshape(K, n, GD).copy()
        seen.update(n=n, noises=z, seeds=None if seeds is None else list(seeds), cfgs=weights, goals=goals)
        raise AssertionError('the device was touched')

    def update(g, idx, b, mask, info, stream):
        seen.update(mask=None if mask is None else np.ctypeslib.as_array(C.cast(mask, C.POINTER(C.c_uint8)), shape=(K * b,)).reshape(K, b).copy(),
                    idx=idx)
        raise AssertionError('the device was touched')

    def member(i):
        m = types.SimpleNamespace(config=dict(ob_dims=(OD,), action_dim=AD, goal_dim=GD, batch_size=B, cfg=1.5 + i), calls=0)

        def seed_of(seed, noises):
            m.calls += 1
            return 100 * i + (0 if seed is None else int(seed))
        m._sample_seed = seed_of
        m.dataset_size = lambda: (64, 64)
        return m
    g = G.CFGRLAgentGroup.__new__(G.CFGRLAgentGroup)
    g._g, g.members, g.batch_size, g._keep = None, [member(i) for i in range(K)], B, None
    g._lib = types.SimpleNamespace(fql_cfgrl_group_sample_actions=sample, fql_cfgrl_group_update_from_dataset=update, fql_group_destroy=lambda h: 0)
    g.seen = seen
    return g


def _f(*shape):
    return np.zeros(shape, np.float32)


@pytest.mark.parametrize('kw', [
    dict(observations=_f(K, 4, OD), goals=None),                                       # the conditional pass reads the goals
    dict(observations=_f(K + 1, 4, OD), goals=_f(GD)),                                 # wrong leading K
    dict(observations=_f(K, 4, OD + 1), goals=_f(GD)),                                 # wrong last dim
    dict(observations=_f(OD + 1), goals=_f(GD)),
    dict(observations=_f(K, 4, OD), goals=_f(GD + 1)),                                 # goals: wrong last dim
    dict(observations=_f(K, 4, OD), goals=_f(K, 5, GD)),                               # goals against the rows
    dict(observations=_f(K, 4, OD), goals=_f(K + 1, 4, GD)),
    dict(observations=_f(K, 4, OD), goals=_f(5, GD)),                                  # a shared block of another row count
    dict(observations=_f(K, 4, OD), goals=_f(GD), seed=[1, 2]),                        # wrong number of seeds
    dict(observations=_f(K, 4, OD), goals=_f(GD), noises=_f(K, 5, AD)),                # noises against the rows
    dict(observations=_f(K, 4, OD), goals=_f(GD), noises=_f(K, 4, AD + 1)),
    dict(observations=_f(K, 4, OD), goals=_f(GD), noises=_f(4, AD)),                   # (noises are never shared between the members)
    dict(observations=_f(K, 0, OD), goals=_f(GD)),                                     # no rows
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=float('nan')),                   # a non-finite weight: scalar, per member, per row
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=[1.0, float('inf'), 3.0]),
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=np.full((K, 4), -np.inf, np.float32)),
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=[1.0, 3.0]),                     # weights: neither a scalar, [K] nor [K, n]
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=_f(K, 5)),
    dict(observations=_f(K, 4, OD), goals=_f(GD), cfg=_f(4)),
], ids=lambda kw: '-'.join(f'{k}{np.shape(v)}' for k, v in kw.items()))
def test_cfgrl_group_sample_actions_checks_before_the_library(group, kw):
    with pytest.raises(ValueError):
        group.sample_actions(**kw)
    assert not group.seen
    assert [m.calls for m in group.members] == [0] * K   # no member's seed counter moved


def test_cfgrl_group_sampling_reaches_the_library_with_valid_arguments(group):
    one = np.arange(GD, dtype=np.float32)
    per_row = np.arange(K * 4, dtype=np.float32).reshape(K, 4)
    default = [[1.5] * 4, [2.5] * 4, [3.5] * 4]   # the members' configured weights
    cases = ((dict(observations=_f(K, 4, OD), goals=_f(K, 4, GD), noises=_f(K, 4, AD)), 4, None, default),
             (dict(observations=_f(4, OD), goals=_f(4, GD), noises=_f(K, 4, AD)), 4, None, default),             # shared rows and goals
             (dict(observations=_f(OD), goals=one, noises=_f(K, AD)), 1, None, [[1.5], [2.5], [3.5]]),           # one shared observation
             (dict(observations=_f(K, 2, 2, OD), goals=one, noises=_f(K, 2, 2, AD), cfg=0.5), 4, None, [[0.5] * 4] * K),
             (dict(observations=_f(K, 4, OD), goals=one, seed=7, cfg=[0.0, 1.0, 2.0]), 4, [7, 107, 207], [[0.0] * 4, [1.0] * 4, [2.0] * 4]),
             (dict(observations=_f(K, 4, OD), goals=_f(K, 4, GD), seed=[1, 2, 3], cfg=per_row), 4, [1, 102, 203], per_row),
             (dict(observations=_f(4, OD), goals=_f(K, 4, GD), seed=5), 4, [5, 105, 205], default),              # shared rows, a goal per member
             (dict(observations=_f(K, OD), goals=_f(K, GD)), 1, [0, 100, 200], [[1.5], [2.5], [3.5]]))           # one row each; each member's own counter
    for kw, n, seeds, cfgs in cases:
        with pytest.raises(AssertionError, match='device was touched'):
            group.sample_actions(**kw)
        assert group.seen['n'] == n and group.seen['seeds'] == seeds, kw
        np.testing.assert_array_equal(group.seen['cfgs'], np.asarray(cfgs, np.float32))
        assert (group.seen['noises'] is None) == ('noises' not in kw)
        if kw['goals'] is one:   # one [G] goal reaches every member and row
            np.testing.assert_array_equal(group.seen['goals'], np.broadcast_to(one, (K, n, GD)))
    assert [m.calls for m in group.members] == [4] * K   # the four seeded or counted calls, none of the calls with noises


def test_cfgrl_group_update_checks_batch_size_rows_and_mask_before_the_library(group):
    with pytest.raises(ValueError):
        group.update_from_dataset(batch_size=32)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K, B + 1), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((B,), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), 64, np.int64))     # past the members' 64 rows
    with pytest.raises(ValueError):
        group.update_from_dataset(do_cfg=np.zeros((K + 1, B), bool))
    with pytest.raises(ValueError):
        group.update_from_dataset(do_cfg=np.zeros((K, B - 1), bool))
    with pytest.raises(ValueError):
        group.update_from_dataset(do_cfg=np.zeros((B,), bool))
    assert not group.seen
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset()
    assert group.seen['mask'] is None and group.seen['idx'] is None
    mask = np.zeros((K, B), np.int64)
    mask[1], mask[2, 3] = 7, -1    # any non-zero entry drops the row
    with pytest.raises(AssertionError, match='device was touched'):
        group.update_from_dataset(batch_size=B, do_cfg=mask, want_info=True)
    np.testing.assert_array_equal(group.seen['mask'], (mask != 0).astype(np.uint8))
