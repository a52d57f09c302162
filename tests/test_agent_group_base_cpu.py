"""CPU: the seven agent group classes are subclasses of one AgentGroup base (fql_amd/agent.py) that owns their plumbing; the library
calls a class names are the C ABI's; _group_idx_arg checks a replay ring's rows under its own label.  No device, no library."""
import types

import numpy as np
import pytest

PLUMBING = ('__init__', '_check', 'upload_dataset', 'synchronize', 'close', '__del__')


def group_classes():
    import fql_amd
    return [fql_amd.FQLAgentGroup, fql_amd.ReBRACAgentGroup, fql_amd.IQLDiffusionAgentGroup, fql_amd.IFQLAgentGroup, fql_amd.IQLAgentGroup,
            fql_amd.CFGRLAgentGroup, fql_amd.SACAgentGroup]


def test_every_exported_group_class_is_checked_here():
    import fql_amd
    exported = {n for n in fql_amd.__all__ if n.endswith('AgentGroup')}
    assert exported == {c.__name__ for c in group_classes()}
    assert len(exported) == 7


def test_every_group_class_subclasses_the_base():
    from fql_amd.agent import AgentGroup
    for cls in group_classes():
        assert issubclass(cls, AgentGroup) and cls is not AgentGroup, cls
        assert cls._member is not None and isinstance(cls._member, type), cls
        assert callable(cls._get_config) and cls._get_config()['batch_size'] > 0, cls


def test_no_group_class_redefines_the_shared_plumbing():
    from fql_amd.agent import AgentGroup
    for cls in group_classes():
        for name in PLUMBING:
            assert name not in vars(cls), f'{cls.__name__} redefines {name}'
            assert getattr(cls, name) is getattr(AgentGroup, name), (cls, name)


def test_every_library_call_a_group_class_names_is_in_the_c_abi():
    from fql_amd import _cabi
    from fql_amd.agent import AgentGroup
    slots = [n for n in vars(AgentGroup) if n.endswith('_fn')]
    assert {'_create_fn', '_update_fn', '_sample_fn', '_stats_fn'} <= set(slots)
    for cls in group_classes():
        named = {n: getattr(cls, n) for n in slots if getattr(cls, n) is not None}
        assert {'_create_fn', '_update_fn', '_sample_fn'} <= set(named), cls
        for slot, fn in named.items():
            assert fn in _cabi.SYMBOLS, f'{cls.__name__}.{slot} = {fn!r} is not a symbol of the C ABI'
    for fn in ('fql_group_destroy', 'fql_group_synchronize', 'fql_group_sample_stats'):   # the calls the base and FQLAgentGroup spell out
        assert fn in _cabi.SYMBOLS


K, B = 3, 8
DS_ROWS, RING_ROWS = 40, (3, 8, 5)


def members():
    return [types.SimpleNamespace(dataset_size=lambda: (DS_ROWS, 0), replay_size=lambda i=i: (RING_ROWS[i], 0)) for i in range(K)]


def ring_rows(m):
    return m.replay_size()[0]


def test_group_idx_arg_checks_a_replay_ring_under_its_label():
    from fql_amd.agent import _group_idx_arg
    ms = members()
    for i in range(K):
        r = np.zeros((K, B), np.int64)
        r[i, 3] = RING_ROWS[i]          # one past member i's ring; within another member's where that one is larger
        with pytest.raises(ValueError, match=f'replay idxs.{i}. out of range'):
            _group_idx_arg(ms, r, B, 'replay idxs', ring_rows)
        r[i, 3] = -1
        with pytest.raises(ValueError, match='out of range'):
            _group_idx_arg(ms, r, B, 'replay idxs', ring_rows)
    with pytest.raises(ValueError, match=rf'replay idxs must be \[{K}, {B}\]'):
        _group_idx_arg(ms, np.zeros((K, B + 1), np.int64), B, 'replay idxs', ring_rows)
    r = np.stack([np.full(B, n - 1, np.int64) for n in RING_ROWS])
    keep, ptr, stream = _group_idx_arg(ms, r, B, 'replay idxs', ring_rows)
    assert ptr == keep.ctypes.data and stream is None and (keep == r).all()


def test_group_idx_arg_defaults_to_the_dataset_and_the_plain_label():
    from fql_amd.agent import _group_idx_arg
    ms = members()
    d = np.zeros((K, B), np.int64)
    d[2, 7] = DS_ROWS
    with pytest.raises(ValueError, match=r'^idxs.2. out of range: \[0, 40\] for 40 rows$'):
        _group_idx_arg(ms, d, B)
    with pytest.raises(ValueError, match=r'dataset idxs.2. out of range'):
        _group_idx_arg(ms, d, B, 'dataset idxs')
    with pytest.raises(ValueError, match=rf'^idxs must be \[{K}, {B}\]'):
        _group_idx_arg(ms, d[:2], B)
    d[2, 7] = DS_ROWS - 1                # past every ring, within the dataset
    keep, ptr, stream = _group_idx_arg(ms, d.tolist(), B)
    assert keep.dtype == np.int64 and ptr and stream is None
