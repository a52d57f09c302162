"""GPU: FQLAgentGroup.sample_actions / compute_flow_actions (fql_group_sample_actions, fql_group_flow_actions): every member's actions in
one fused call.  The reference is the member's own sample_actions / compute_flow_actions, which test_gpu_parity.py and test_gpu_shapes.py
pin to the fp64 restatement; rows of the 16-row kernels do not depend on their neighbours and each member's tasks keep their arguments,
so every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest

from tests.util import make_problem, randomize_params
from tests.test_gpu_group import _assert_same_state

pytestmark = pytest.mark.gpu

B = 16   # the update's batch: only the ordering and state tests update


def _setup(K, hidden, od=29, ad=8, twins=True, **kw):
    """As tests/test_gpu_group.py::_setup: a group whose members differ in seed and alpha and carry randomised parameters, and (twins)
    standalone agents in the same state."""
    import fql_amd
    cfg, ds, batch, noise = make_problem(od, ad, B, tuple(hidden), seed=7, **kw)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    seeds, alphas = list(range(K)), [10.0 * (i + 1) for i in range(K)]
    group = fql_amd.FQLAgentGroup.create(seeds, ex_o, ex_a, cfg, alphas=alphas)
    group.upload_dataset(ds)
    tw = []
    for i, (s, a) in enumerate(zip(seeds, alphas)):
        p = randomize_params(group.members[i].get_params(), 100 + i, scale=0.1)
        group.members[i].set_params(p)
        if twins:
            c = dict(cfg)
            c['alpha'] = a
            t = fql_amd.FQLAgent.create(s, ex_o, ex_a, c)
            t.set_params(p)
            t.upload_dataset(ds)
            tw.append(t)
    return cfg, group, tw


def _rows(K, n, od, ad, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n, od)).astype(np.float32), rng.standard_normal((K, n, ad)).astype(np.float32)


# od, ad, hidden, K, the n's, config overrides: the shapes at which the sampler's launches are built differently
CASES = [
    (5, 3, (32, 32), 2, (1,), {}),                                              # minimum
    (29, 8, (128,) * 4, 3, (10, 16, 17), {}),                                   # the evaluation default; the pad16 boundary
    (29, 15, (64,) * 4, 2, (10,), {}),                                          # head at ap 16, 15 of its 16 columns used
    (29, 16, (64,) * 4, 2, (10,), {}),                                          # head's 16 columns all used
    (69, 21, (64,) * 4, 2, (10,), {}),                                          # ap = 32
    (29, 8, (1024,) * 3, 2, (10,), {}),                                         # the K > 512 instantiation of the 16-row kernel
    (600, 8, (64,) * 4, 2, (10,), {}),                                          # layer 0 through the K > 512 kernel
    (40, 4, (64, 64), 2, (10,), dict(actor_layer_norm=True, flow_steps=3)),     # LayerNorm in the actor, short Euler loop
    (29, 8, (64,) * 4, 8, (10,), {}),                                           # blockIdx.y up to 7, eight members per table
    (11, 5, (32,) * 4, 2, (4097,), {}),                                         # two chunks, the second of one row
]
IDS = ['minimum', 'eval-default-pad16', 'ad15', 'ad16', 'ap32', 'hidden1024', 'od600', 'actor-ln-flow3', 'K8', 'two-chunks']


@pytest.mark.parametrize('od, ad, hidden, K, ns, kw', CASES, ids=IDS)
def test_group_sample_equals_members_explicit_noise_and_seeds(od, ad, hidden, K, ns, kw):
    cfg, group, _ = _setup(K, hidden, od, ad, twins=False, **kw)
    seeds = [11 + 1000003 * i for i in range(K)]
    for n in ns:
        obs, z = _rows(K, n, od, ad, seed=n)
        got = group.sample_actions(obs, noises=z)
        flow = group.compute_flow_actions(obs, z)
        each = group.sample_actions(obs, seed=seeds)
        one = group.sample_actions(obs, seed=5)
        assert got.shape == flow.shape == each.shape == one.shape == (K, n, ad) and got.dtype == np.float32
        for i, m in enumerate(group.members):
            np.testing.assert_array_equal(got[i], m.sample_actions(obs[i], noises=z[i]), err_msg=f'noises n {n} member {i}')
            np.testing.assert_array_equal(flow[i], m.compute_flow_actions(obs[i], z[i]), err_msg=f'flow n {n} member {i}')
            np.testing.assert_array_equal(each[i], m.sample_actions(obs[i], seed=seeds[i]), err_msg=f'seeds n {n} member {i}')
            np.testing.assert_array_equal(one[i], m.sample_actions(obs[i], seed=5), err_msg=f'one seed n {n} member {i}')
        assert np.isfinite(got).all() and np.abs(got).max() <= 1.0 and np.abs(flow).max() <= 1.0
        if K > 1:   # the members are different agents: a result that repeated one member's rows would not pass
            assert not np.array_equal(each[0], each[1])
    group.close()


def test_group_unseeded_draws_advance_each_members_counter():
    """seed=None: every member draws with its own sample counter, which a group call advances as the member's own call does."""
    K, n = 3, 10
    cfg, group, twins = _setup(K, (64,) * 4)
    obs, _ = _rows(K, n, 29, 8)
    for step in range(3):
        got = group.sample_actions(obs)
        for i, t in enumerate(twins):
            np.testing.assert_array_equal(got[i], t.sample_actions(obs[i]), err_msg=f'call {step} member {i}')
        if step == 0:   # a member's own unseeded call between the group's
            np.testing.assert_array_equal(group.members[1].sample_actions(obs[1]), twins[1].sample_actions(obs[1]))
    assert not np.array_equal(group.sample_actions(obs), got)   # (the counters moved: the next draw is another)
    group.close()


def test_group_shared_observations_and_leading_dims():
    K, n = 3, 10
    cfg, group, _ = _setup(K, (64,) * 4, twins=False)
    obs, z = _rows(K, n, 29, 8)
    rep = np.repeat(obs[:1], K, axis=0)
    np.testing.assert_array_equal(group.sample_actions(obs[0], seed=[1, 2, 3]), group.sample_actions(rep, seed=[1, 2, 3]))
    np.testing.assert_array_equal(group.sample_actions(obs[0], noises=z), group.sample_actions(rep, noises=z))
    np.testing.assert_array_equal(group.compute_flow_actions(obs[0], z), group.compute_flow_actions(rep, z))
    one = group.sample_actions(obs[0, 0], seed=4)                    # [od] -> [K, ad]
    assert one.shape == (K, 8)
    np.testing.assert_array_equal(one, group.sample_actions(rep[:, :1], seed=4)[:, 0])
    want = group.sample_actions(obs, noises=z)
    got = group.sample_actions(obs.reshape(K, 2, 5, 29), noises=z.reshape(K, 2, 5, 8))   # [K, 2, 5, od] -> [K, 2, 5, ad]
    assert got.shape == (K, 2, 5, 8)
    np.testing.assert_array_equal(got.reshape(K, n, 8), want)
    group.close()


def test_group_sample_device_tensors_on_a_side_stream():
    import torch
    K, n = 3, 10
    cfg, group, _ = _setup(K, (64,) * 4, twins=False)
    obs, z = _rows(K, n, 29, 8)
    want = group.sample_actions(obs, noises=z)
    want_seed = group.sample_actions(obs, seed=[7, 8, 9])
    want_flow = group.compute_flow_actions(obs, z)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o_d, z_d = torch.from_numpy(obs).cuda(), torch.from_numpy(z).cuda()
        got = group.sample_actions(o_d, noises=z_d)
        got_seed = group.sample_actions(o_d, seed=[7, 8, 9])
        got_flow = group.compute_flow_actions(o_d, z_d)
        got_mixed = group.sample_actions(o_d, noises=z)          # device rows, host noises: a device result
    for t in (got, got_seed, got_flow, got_mixed):
        assert t.is_cuda and tuple(t.shape) == (K, n, 8)
    s.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got_seed.cpu().numpy(), want_seed)
    np.testing.assert_array_equal(got_flow.cpu().numpy(), want_flow)
    np.testing.assert_array_equal(got_mixed.cpu().numpy(), want)
    group.close()


def test_group_sample_is_ordered_behind_group_and_member_updates():
    """No synchronize anywhere: the fused call sees the group's updates, and a member's own stream-less update, enqueued just before."""
    K, n = 2, 10
    cfg, group, twins = _setup(K, (64,) * 4)
    obs, z = _rows(K, n, 29, 8)
    for _ in range(3):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    got = group.sample_actions(obs, noises=z)
    for i, t in enumerate(twins):
        np.testing.assert_array_equal(got[i], t.sample_actions(obs[i], noises=z[i]), err_msg=f'after the group updates, member {i}')
    group.members[0].update_from_dataset(B)
    got = group.sample_actions(obs, seed=3)
    flow = group.compute_flow_actions(obs, z)
    twins[0].update_from_dataset(B)
    for i, t in enumerate(twins):
        np.testing.assert_array_equal(got[i], t.sample_actions(obs[i], seed=3), err_msg=f"after member 0's update, member {i}")
        np.testing.assert_array_equal(flow[i], t.compute_flow_actions(obs[i], z[i]), err_msg=f"after member 0's update, member {i}")
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_group_sample_changes_no_member_state():
    import torch
    K, n = 3, 10
    cfg, group, twins = _setup(K, (64,) * 4)
    obs, z = _rows(K, n, 29, 8)
    for _ in range(2):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    for _ in range(3):
        group.sample_actions(obs)
        group.sample_actions(obs, noises=z)
        group.compute_flow_actions(obs, z)
    group.sample_actions(torch.from_numpy(obs).cuda(), seed=1)   # (left in flight on torch's stream)
    for i, (m, t) in enumerate(zip(group.members, twins)):       # the twins have sampled nothing
        _assert_same_state(m, t, f'member {i} after sampling')
    group.sample_actions(obs)
    group.update_from_dataset()
    for t in twins:
        t.update_from_dataset(B)
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i} after one more update')
    group.close()


def test_group_sample_launch_count_does_not_depend_on_k():
    """One chunk of a fused call is assemble, one launch per layer of the actor (the hidden layers and the head, each over the members'
    concatenated tasks), extract: 2 + (len(hidden) + 1) launches.  The flow call runs the BC actor's layers once per Euler step between
    the same two end launches: 2 + flow_steps (len(hidden) + 1)."""
    hidden, fs = (64,) * 4, 5
    _, g3, _ = _setup(3, hidden, twins=False, flow_steps=fs)
    _, g1, _ = _setup(1, hidden, twins=False, flow_steps=fs)
    os3, fl3 = g3.sample_launches(False), g3.sample_launches(True)
    assert (os3, fl3) == (g1.sample_launches(False), g1.sample_launches(True))
    assert os3 == 2 + (len(hidden) + 1)
    assert fl3 == fs * (os3 - 2) + 2
    g3.close()
    g1.close()


def test_group_sample_refusals_leave_the_group_working():
    from fql_amd import _cabi
    K, n = 2, 10
    cfg, group, twins = _setup(K, (64,) * 4)
    lib, g = group._lib, group._g
    obs, z = _rows(K, n, 29, 8)
    out = np.zeros((K, n, 8), np.float32)
    seeds = (C.c_uint64 * K)(1, 2)
    o, zp, op = obs.ctypes.data, z.ctypes.data, out.ctypes.data
    bad = [
        lambda: lib.fql_group_sample_actions(g, o, 0, zp, seeds, op, None),
        lambda: lib.fql_group_sample_actions(g, o, -3, zp, seeds, op, None),
        lambda: lib.fql_group_sample_actions(g, None, n, zp, seeds, op, None),
        lambda: lib.fql_group_sample_actions(g, o, n, zp, seeds, None, None),
        lambda: lib.fql_group_sample_actions(g, o, n, None, None, op, None),
        lambda: lib.fql_group_flow_actions(g, o, None, n, op, None),
        lambda: lib.fql_group_flow_actions(g, o, zp, 0, op, None),
        lambda: lib.fql_group_flow_actions(g, None, zp, n, op, None),
        lambda: lib.fql_group_sample_stats(g, 0, None),
    ]
    for k, call in enumerate(bad):
        assert call() == _cabi.FQL_E_INVALID, k
        assert lib.fql_last_error(None), k
        assert not out.any(), k
        got = group.sample_actions(obs, seed=[5, 6])
        flow = group.compute_flow_actions(obs, z)
        group.update_from_dataset()
        for i, t in enumerate(twins):
            np.testing.assert_array_equal(got[i], t.sample_actions(obs[i], seed=[5, 6][i]), err_msg=f'refusal {k} member {i}')
            np.testing.assert_array_equal(flow[i], t.compute_flow_actions(obs[i], z[i]), err_msg=f'refusal {k} member {i}')
            t.update_from_dataset(B)
    assert lib.fql_group_sample_actions(g, o, n, None, seeds, op, None) == _cabi.FQL_OK   # the C call itself, seeds as uint64[K]
    for i, t in enumerate(twins):
        np.testing.assert_array_equal(out[i], t.sample_actions(obs[i], seed=i + 1))
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
    group.close()
