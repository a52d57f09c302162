"""GPU: agent groups (fql_group_*, FQLAgentGroup).  A member trained in a group must end bitwise where the same agent trained alone ends
(same seed, alpha, rows and noise): the fused program changes which launch a task rides in, never its arithmetic."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import K_SIDE_BIG, make_problem, randomize_params, leaf_dict, read_plan

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


def _setup(K, B, hidden, seeds=None, alphas=None, od=29, ad=8, scale=0.1, **kw):
    """A group of K members and their standalone twins on one problem: `hidden` is the four equal widths' H or the tuple of widths, `kw`
    are config overrides.  Members and twins differ in seed and alpha only (alphas: the config's alpha times 1, 2, ..) and start from the
    same randomised parameters."""
    import fql_amd
    hidden = (hidden,) * 4 if isinstance(hidden, int) else tuple(hidden)
    seeds = list(range(K)) if seeds is None else seeds
    alphas = [kw.get('alpha', 10.0) * (i + 1) for i in range(K)] if alphas is None else alphas
    cfg, ds, batch, noise = make_problem(od, ad, B, hidden, seed=7, **kw)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    group = fql_amd.FQLAgentGroup.create(seeds, ex_o, ex_a, cfg, alphas=alphas)
    group.upload_dataset(ds)
    twins = []
    for i, (s, a) in enumerate(zip(seeds, alphas)):
        c = dict(cfg)
        c['alpha'] = a
        t = fql_amd.FQLAgent.create(s, ex_o, ex_a, c)
        p = randomize_params(t.get_params(), 100 + i, scale=scale)
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


# The shapes at which the fused program is built differently (fql_group_s::zip / fuse, fql_amd/csrc/fql_engine_groups.h).  Each is pinned to the
# fp64 restatement for a single agent (test_gpu_parity.py, test_gpu_shapes.py, test_gpu_hardening.py; k8 is a shape of the cases above),
# so the twin is a checked reference.
PATHS = [
    # od, ad, B, hidden, cfg overrides, K, n
    pytest.param(40, 4, 1024, (512,) * 4, dict(alpha=300.0), 2, 3, id='b1024_big_tiles'),   # fql_side_big_kernel's four rebased sub-tables, chain<512> at M 1024
    pytest.param(29, 15, 64, (256,) * 4, {}, 2, 5, id='act15_chain'),                        # chain<256>, its 16-column block full
    pytest.param(29, 16, 64, (512,) * 4, {}, 2, 5, id='act16_generic'),                      # generic Euler kernels, fql_dgrad0_multi_kernel at 16 columns
    pytest.param(69, 21, 64, (512,) * 4, dict(alpha=30.0, discount=0.995), 3, 4, id='humanoidmaze'),   # no chain, generic dgrads, ap = 32
    pytest.param(45, 24, 48, (80, 48, 64), dict(q_agg='min'), 3, 5, id='ragged_min'),        # ragged widths, 3 layers
    pytest.param(29, 8, 64, (512,) * 4, dict(actor_layer_norm=True), 2, 5, id='actor_ln'),   # H 512 without chain or OP_WFRAG, unfused Euler finish
    pytest.param(40, 4, 48, (64, 64), dict(actor_layer_norm=True, flow_steps=3), 2, 5, id='two_layer_fs3'),   # 2 layers, short Euler loop
    pytest.param(11, 5, 32, (64,) * 4, dict(normalize_q_loss=True), 2, 5, id='norm_q'),      # the loss / finalize tasks' other branch
    pytest.param(17, 6, 16, (32,) * 4, dict(layer_norm=False), 4, 5, id='no_ln_b16'),        # empty LayerNorm-backward sub-table, minimum batch
    pytest.param(29, 8, 64, (256,) * 4, {}, 8, 5, id='k8'),                                  # eight members per table, blockIdx.y up to 7
    pytest.param(29, 8, 32, (1024,) * 3, {}, 2, 3, id='wide1024'),                           # fused tables through the K > 512 kernels
    pytest.param(29, 8, 32, (50, 50, 50), {}, 2, 5, id='w50_padded'),                        # out 50 of out_p 64: LayerNorm widths and zeroed padding in fused tables
]


@pytest.mark.parametrize('od, ad, B, hidden, kw, K, n', PATHS)
def test_group_equals_standalone_twins_on_every_path(od, ad, B, hidden, kw, K, n, request):
    cfg, ds, batch, noise, group, twins = _setup(K, B, hidden, od=od, ad=ad, scale=0.05 if max(hidden) >= 512 else 0.1, **kw)
    if request.node.callspec.id == 'b1024_big_tiles':
        # a fused table launch is member 0's launch over the members' concatenated tables (fql_group_s::zip), dispatched by the member's
        # own issue(): the kernel in the member's plan is the kernel the group runs
        for m in group.members:
            assert any(L['kernel'] == K_SIDE_BIG and any(t['rows'] == 64 and t['M'] == B for t in L['gemm']) for L in read_plan(m))
    for _ in range(n):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def _info_row(agent):
    from fql_amd import INFO_KEYS
    info = agent.read_info()
    return [info[k] for k in INFO_KEYS]


def test_group_infos_through_the_c_abi():
    """fql_group_update_from_dataset's info13xk: a host buffer (synchronous) and a device buffer (read after the group's synchronize) hold
    every member's 13 infos in the wrapper's key order."""
    import torch
    K, B = 3, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)
    lib = group._lib
    for step in range(4):
        if step % 2 == 0:
            host = np.full((K, 13), np.nan, np.float32)
            group._check(lib.fql_group_update_from_dataset(group._g, None, B, host.ctypes.data, None))
            got = host
        else:
            dev = torch.full((K, 13), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()                     # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_group_update_from_dataset(group._g, None, B, dev.data_ptr(), None))
            group.synchronize()
            got = dev.cpu().numpy()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_from_dataset(B)
            assert got[i].tolist() == _info_row(m), (step, i)
            assert got[i].tolist() == _info_row(t), (step, i)
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_device_rows_on_the_callers_stream():
    """Row indices as a CUDA tensor: the update runs on torch's current stream, here its default stream, which reaches the engine as
    FQL_STREAM_LEGACY.  Alternating with host rows (the group's own stream) with no synchronize in between: each update is ordered behind
    the one before it on the other stream, and the lazily read infos of either kind are the twins'."""
    import torch
    K, B = 2, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)
    assert torch.cuda.current_stream().cuda_stream == 0
    rng = np.random.default_rng(13)
    for step in range(6):
        idxs = rng.integers(0, len(ds['observations']), size=(K, B))
        lazy = step >= 4      # (the first four updates take no infos: nothing but the group's own ordering is between them)
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 2 == 0 else idxs, want_info=lazy)
        want = [t.update_from_dataset(B, idxs=idxs[i], want_info=lazy)[1] for i, t in enumerate(twins)]
        for i in range(K if lazy else 0):
            assert infos[i].to_dict() == want[i].to_dict(), (step, i)
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_member_updates_between_group_updates():
    """A member's own updates between group updates, on the engine's queues and from a host batch, with no synchronize anywhere: the group
    update is ordered behind them, and they behind it."""
    K, B = 3, 64
    cfg, ds, batch, noise, group, twins = _setup(K, B, 128)

    def sequence(update_all, agents):
        for _ in range(3):
            update_all()
            agents[0].update_from_dataset(B)               # stream left to the engine: its own queues
            agents[1].update(batch, noise=noise)           # host batch, explicit noise
            update_all()

    sequence(group.update_from_dataset, group.members)
    sequence(lambda: [t.update_from_dataset(B) for t in twins], twins)
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    assert group.members[0].get_opt_state()['count'] == 9 and group.members[2].get_opt_state()['count'] == 6
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
    r.update_from_dataset(B)         # the restored twin takes the next update alone
    group.update_from_dataset()      # the member goes back to group updates after standalone ones
    group.synchronize()
    _assert_same_state(m, r, 'restored, after a group update')
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
