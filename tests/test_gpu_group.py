"""GPU: agent groups (fql_group_*, FQLAgentGroup).  A member trained in a group must end bitwise where the same agent trained alone ends
(same seed, alpha, rows and noise): the fused program changes which launch a task rides in, never its arithmetic."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import make_problem, randomize_params, leaf_dict

pytestmark = pytest.mark.gpu


def _assert_same_state(a, b, what=''):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    assert pa.keys() == pb.keys()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=f'{what} {k}')
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step']), what
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{what} {part} {k}')
    assert a.read_info() == b.read_info(), what


def _setup(K, B, H, seeds=None, alphas=None):
    import fql_amd
    seeds = list(range(K)) if seeds is None else seeds
    alphas = [10.0 * (i + 1) for i in range(K)] if alphas is None else alphas
    cfg, ds, batch, noise = make_problem(29, 8, B, (H,) * 4, seed=7)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    group = fql_amd.FQLAgentGroup.create(seeds, ex_o, ex_a, cfg, alphas=alphas)
    group.upload_dataset(ds)
    twins = []
    for i, (s, a) in enumerate(zip(seeds, alphas)):
        c = dict(cfg)
        c['alpha'] = a
        t = fql_amd.FQLAgent.create(s, ex_o, ex_a, c)
        p = randomize_params(t.get_params(), 100 + i)
        t.set_params(p)
        group.members[i].set_params(p)
        t.upload_dataset(ds)
        twins.append(t)
    return cfg, ds, batch, noise, group, twins


@pytest.mark.parametrize('K, B, H, n', [(3, 64, 128, 25), (2, 256, 512, 10), (4, 256, 256, 10), (1, 64, 128, 8)],
                         ids=['side-K3-B64-H128', 'chain-K2-B256-H512', 'chain-K4-B256-H256', 'single-K1'])
def test_group_equals_standalone_twins_device_rng(K, B, H, n):
    seeds, alphas = ([0, 1, 2], [1.0, 10.0, 100.0]) if K == 3 else (None, None)
    cfg, ds, batch, noise, group, twins = _setup(K, B, H, seeds, alphas)
    for _ in range(n):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_explicit_rows_and_lazy_infos():
    K, B = 3, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)
    rng = np.random.default_rng(3)
    n = len(ds['observations'])
    for step in range(6):
        idxs = rng.integers(0, n, size=(K, B))
        infos = group.update_from_dataset(idxs=idxs, want_info=True)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=True)[1] for i, t in enumerate(twins)]
        assert len(infos) == K
        for i in range(K):
            assert infos[i].to_dict() == want[i].to_dict(), (step, i)
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_ordering_without_synchronize():
    """Member entry points straight after group updates (no synchronize) see those updates; a set_params between group updates is
    seen by the next one."""
    K, B = 2, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)
    obs = batch['observations'][:7]
    for rnd in range(2):
        for _ in range(5):
            group.update_from_dataset()
            for t in twins:
                t.update_from_dataset(B)
        for i, (m, t) in enumerate(zip(group.members, twins)):
            pm, pt = leaf_dict(m.get_params()), leaf_dict(t.get_params())
            for k in pm:
                np.testing.assert_array_equal(pm[k], pt[k], err_msg=f'round {rnd} member {i} {k}')
            np.testing.assert_array_equal(m.sample_actions(obs, seed=11), t.sample_actions(obs, seed=11))
            assert m.total_loss(batch) == t.total_loss(batch)
        p = randomize_params(twins[0].get_params(), 55 + rnd, scale=0.05)
        group.members[0].set_params(p)
        twins[0].set_params(p)
    for _ in range(3):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_member_checkpoint_hand_off(tmp_path):
    import fql_amd
    from fql_amd import checkpoint
    K, B = 2, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)
    for _ in range(5):
        group.update_from_dataset()
    m = group.members[1]
    checkpoint.save_agent(m, str(tmp_path), 5)
    c = dict(cfg)
    c['alpha'] = m.config['alpha']
    r = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], c)
    checkpoint.restore_agent(r, str(tmp_path), 5)
    r.upload_dataset(ds)
    pm, pr = leaf_dict(m.get_params()), leaf_dict(r.get_params())
    for k in pm:
        np.testing.assert_array_equal(pm[k], pr[k], err_msg=k)
    rng = np.random.default_rng(9)
    for step in range(4):
        idx = rng.integers(0, len(ds['observations']), size=B)
        nz = O.make_noise(B, 8, 70 + step)
        m.update_from_dataset(B, idxs=idx, noise=nz)
        r.update_from_dataset(B, idxs=idx, noise=nz)
    _assert_same_state(m, r, 'restored')
    group.update_from_dataset()      # the member goes back to group updates after standalone ones
    group.synchronize()
    group.close()


def test_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    cfg, ds, batch, noise = make_problem(29, 8, 64, (128,) * 4, seed=1)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]

    def create(members):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p()
        return lib.fql_group_create(arr, len(members), C.byref(g)), g

    a = fql_amd.FQLAgent.create(0, ex_o, ex_a, cfg)
    wide = fql_amd.FQLAgent.create(1, ex_o, ex_a, dict(cfg, actor_hidden_dims=(256,) * 4, value_hidden_dims=(256,) * 4))
    bf = fql_amd.FQLAgent.create(2, ex_o, ex_a, dict(cfg, precision='bf16x3'))
    vis_cfg = dict(cfg, encoder='impala_small', batch_size=16)
    vis = fql_amd.FQLAgent.create(3, np.zeros((1, 32, 32, 3), np.uint8), ex_a, vis_cfg)
    other_b = fql_amd.FQLAgent.create(4, ex_o, ex_a, dict(cfg, batch_size=32))
    for bad in (wide, bf, vis, other_b):
        rc, g = create([a, bad])
        assert rc == _cabi.FQL_E_INVALID and not g.value, lib.fql_last_error(None)
    rc, g = create([a, a])
    assert rc == _cabi.FQL_E_INVALID
    b = fql_amd.FQLAgent.create(5, ex_o, ex_a, dict(cfg, alpha=3.0))
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value
    assert create([b])[0] == _cabi.FQL_E_INVALID                     # already grouped
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    assert lib.fql_group_update_from_dataset(g, None, 32, None, None) == _cabi.FQL_E_INVALID   # wrong batch size
    assert lib.fql_group_update_from_dataset(g, None, 64, None, None) == _cabi.FQL_E_INVALID   # no dataset uploaded
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK           # released: plain handles again
    b.close()
    assert b._h is None
    for x in (a, wide, bf, vis, other_b):
        x.close()
