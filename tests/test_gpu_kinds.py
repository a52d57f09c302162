"""GPU: which kind of handle may call which entry point of the C ABI.  The matrix below is written out from the refusal macros at the top of
the entry points as they stood before the engine got one admission table (FQL_IFQL_REFUSES also refused ReBRAC handles, FQL_SAC_REFUSES
also IQL handles, the fql_<kind>_* calls took their own kind only), so the same file passes against that older library as well.

A refusal comes before any argument is read, so every refused pair is called with null / zero data: FQL_E_STATE, and fql_last_error
names the entry point and a handle label - the handle's own, or for an fql_<kind>_* call the kind it needs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
OD, AD, H, B = 5, 3, 32, 16
KINDS = ('fql', 'ifql', 'rebrac', 'sac', 'bc', 'iql')
LABEL = {'fql': b'FQL handle', 'ifql': b'IFQL handle', 'rebrac': b'ReBRAC handle', 'sac': b'SAC handle', 'bc': b'BC handle',
         'iql': b'IQL handle'}
OTHERS = 'ifql rebrac sac bc iql'
# entry point -> the kinds it refuses
REFUSED = {
    'fql_update_begin': OTHERS,
    'fql_update_end': OTHERS,
    'fql_update': 'rebrac sac bc iql',
    'fql_total_loss': 'rebrac sac bc iql',
    'fql_sample_actions': 'bc',
    'fql_flow_actions': 'rebrac sac bc iql',
    'fql_noise_from_jax_keys': OTHERS,
    'fql_dataset_add_frames': OTHERS,
    'fql_replay_create': 'ifql rebrac bc iql',
    'fql_replay_add': 'ifql rebrac bc iql',
    'fql_replay_add_frames': OTHERS,
    'fql_replay_size': 'ifql rebrac bc iql',
    'fql_update_balanced': OTHERS,
    'fql_update_from_dataset_begin': OTHERS,
    'fql_update_from_dataset_begin_split': OTHERS,
    'fql_update_begin_split': OTHERS,
    'fql_update_end_split': OTHERS,
    'fql_grad_buckets': OTHERS,
    'fql_update_from_dataset': 'rebrac sac bc iql',
    'fql_info_wait': 'sac bc iql',
    'fql_read_info': 'sac bc iql',
    'fql_profile_update': 'rebrac sac bc iql',
    'fql_debug_workspace': 'rebrac sac bc iql',
    'fql_dataset_upload_frames': OTHERS,
    'fql_update_from_frames': OTHERS,
}
# the calls of one kind alone: refused for the five others, and the message names the kind they need
OWN = {
    'rebrac': ('fql_rebrac_update', 'fql_rebrac_update_from_dataset', 'fql_rebrac_total_loss', 'fql_rebrac_sample_actions',
               'fql_rebrac_stats'),
    'sac': ('fql_sac_update', 'fql_sac_update_from_dataset', 'fql_sac_update_balanced', 'fql_sac_total_loss', 'fql_sac_sample_actions',
            'fql_sac_stats'),
    'iql': ('fql_iql_update', 'fql_iql_update_from_dataset', 'fql_iql_total_loss', 'fql_iql_sample_actions', 'fql_iql_stats'),
    'bc': ('fql_bc_update', 'fql_bc_update_from_dataset', 'fql_bc_policy_loss', 'fql_bc_sample_actions', 'fql_bc_stats'),
}
HINTS = {   # (entry point, kind) -> what the message also says
    ('fql_read_info', 'bc'): b'4 infos', ('fql_read_info', 'sac'): b'14 infos', ('fql_read_info', 'iql'): b'16 or 19 infos',
    ('fql_info_wait', 'bc'): b'4 infos', ('fql_info_wait', 'sac'): b'14 infos', ('fql_info_wait', 'iql'): b'16 or 19 infos',
    ('fql_update', 'rebrac'): b'its batch has no next_actions: fql_rebrac_update',
    ('fql_flow_actions', 'rebrac'): b'the actor is deterministic, there is no flow',
}
# the two diagnostic entry points include/fql_amd.h does not declare
_VP, _I = C.c_void_p, C.c_int
UNDECLARED = {'fql_profile_update': [_VP, _I, _I] + [_VP] * 6, 'fql_debug_workspace': [_VP, _I, _VP, C.c_size_t, _VP]}


@pytest.fixture(scope='module')
def handles():
    import fql_amd
    from fql_amd import bc, ifql, iql, rebrac, sac
    ob, ac = np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32)
    mlp = dict(actor_hidden_dims=(H, H), value_hidden_dims=(H, H), batch_size=B)
    made = {}
    for kind, cls, cfg, dims in (('fql', fql_amd.FQLAgent, fql_amd.get_config(), mlp), ('ifql', fql_amd.IFQLAgent, ifql.get_config(), mlp),
                                 ('rebrac', fql_amd.ReBRACAgent, rebrac.get_config(), mlp), ('sac', fql_amd.SACAgent, sac.get_config(), mlp),
                                 ('bc', fql_amd.BCAgent, bc.get_config(), dict(hidden_dims=(H, H), batch_size=B)),
                                 ('iql', fql_amd.IQLAgent, iql.get_config(), mlp)):
        cfg.update(dims)
        made[kind] = cls.create(1, ob, ac, cfg)
    yield made
    for a in made.values():
        a.close()


def _call(lib, name, h):
    """name(h, nulls and zeros)"""
    from fql_amd import _cabi
    fn = getattr(lib, name)
    if name in UNDECLARED:
        fn.restype, fn.argtypes = _I, UNDECLARED[name]
    types = fn.argtypes[1:]
    return fn(h, *[0.0 if t is C.c_float else 0 if t in (C.c_int, C.c_int64, C.c_uint64, C.c_size_t) else None for t in types]), _cabi


def test_every_refused_pair_is_a_state_error_that_names_the_call_and_the_kind(handles):
    lib = handles['fql']._lib
    pairs = [(ep, k, LABEL[k]) for ep, ks in REFUSED.items() for k in ks.split()]
    pairs += [(ep, k, LABEL[owner]) for owner, eps in OWN.items() for ep in eps for k in KINDS if k != owner]
    assert len(pairs) == 108 + 21 * 5
    for ep, kind, label in pairs:
        h = handles[kind]._h
        rc, _cabi = _call(lib, ep, h)
        msg = lib.fql_last_error(h)
        assert rc == _cabi.FQL_E_STATE, (ep, kind, rc, msg)
        assert ep.encode() in msg and label in msg, (ep, kind, msg)
        if (ep, kind) in HINTS:
            assert HINTS[(ep, kind)] in msg, (ep, kind, msg)


def test_admitted_calls_that_take_no_data_are_not_state_errors(handles):
    from fql_amd import _cabi
    lib = handles['fql']._lib
    E = _cabi.FQL_E_STATE
    for kind in ('fql', 'sac'):   # the replay ring: FQL and SAC
        h = handles[kind]._h
        size, ptr = C.c_int64(-1), C.c_int64(-1)
        assert lib.fql_replay_create(h, 8) == _cabi.FQL_OK, lib.fql_last_error(h)
        assert lib.fql_replay_size(h, C.byref(size), C.byref(ptr)) == _cabi.FQL_OK and (size.value, ptr.value) == (0, 0)
    assert _call(lib, 'fql_grad_buckets', handles['fql']._h)[0] != E
    counts = {'fql': 13, 'ifql': 12, 'rebrac': 12, 'sac': 14, 'bc': 4, 'iql': 19}   # (IQL's default actor_loss is ddpgbc)
    for kind, a in handles.items():
        assert lib.fql_num_info(a._h) == counts[kind]
    for kind in OWN:
        assert _call(lib, f'fql_{kind}_stats', handles[kind]._h)[0] == _cabi.FQL_OK
