"""GPU: parameter and optimizer-state access while stream-less updates are still in flight on the engine's AQL queues.

An update with no stream (update_from_dataset, update(..., want_info=False), the IFQL and ReBRAC updates) runs as pre-built AQL packets
on the engine's own HSA queues, and up to 6 are in flight when the call returns (fql_amd/csrc/fql_aql.h).  HIP cannot see those queues,
so every entry point that touches the engine's buffers waits for them first.  Here agent `a` queues N updates and, with nothing in
between that waits for them, calls the entry point under test - through the C ABI where the Python wrapper would wait by accident
(leaves() calls fql_leaf_info).  Its twin `b` (same seed, parameters and rows) runs the same updates as the captured graph on a stream of
the caller's and synchronises before each access.  Bitwise equality with the twin, and for writes one update against the fp64
restatement, show that nothing was read early or overwritten afterwards.

Shapes: BASELINE configs[1] (obs 29, act 8, B 256, hidden 512 x 4, 10 flow steps; the FQL actor has the Euler chain, so writes to
modules_actor_bc_flow/ rebuild its fragment-major weights), so the queued updates keep several ms of device work behind the call."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import ifql_oracle as IO
from tests import rebrac_oracle as RO
from tests.util import assert_step_matches, leaf_dict, make_problem, randomize_params

pytestmark = pytest.mark.gpu
N = 6                          # FQL_AQL_INFLIGHT: the most the engine keeps on its queues
OD, AD, B, H = 29, 8, 256, 512


class Setup:
    """One algorithm at configs[1]: problem, agents, randomized parameters, one checked update against the fp64 restatement."""

    def __init__(self, algo, seed=31):
        self.algo = algo
        if algo == 'fql':
            self.cfg, self.ds, self.batch, self.noise = make_problem(OD, AD, B, (H,) * 4, seed=seed)
        elif algo == 'ifql':
            from tests.test_gpu_ifql import _problem
            self.cfg, self.ds, self.batch, self.noise = _problem(H, B, seed=seed)
        else:
            from tests.test_gpu_rebrac import _problem
            self.cfg, self.ds, self.batch, self.noise = _problem(H, B, seed=seed)

    def agent(self, seed=3, params=None, capacity=None):
        import fql_amd
        cls = {'fql': fql_amd.FQLAgent, 'ifql': fql_amd.IFQLAgent, 'rebrac': fql_amd.ReBRACAgent}[self.algo]
        x = cls.create(seed, self.batch['observations'][:1], self.batch['actions'][:1], self.cfg)
        if params is not None:
            x.set_params(params)
        x.upload_dataset(self.ds, capacity=capacity)
        return x

    def randomized(self, params, seed):
        if self.algo == 'rebrac':
            from tests.test_gpu_rebrac import _randomized
            return _randomized(params, seed)
        return randomize_params(params, seed, scale=0.05 if self.algo == 'fql' else 0.1)

    def pair(self, **kw):
        """Twins with the same seed and the same randomized parameters, the dataset uploaded."""
        a = self.agent(**kw)
        self.init = a.get_params()
        p = self.randomized(self.init, 5)
        a.set_params(p)
        return a, self.agent(params=p, **kw)

    def queue(self, x, n=N, stream=None):
        """n updates on engine-drawn rows and noise; ReBRAC alternates full and critic-only steps, so both programs are in flight."""
        for i in range(n):
            if self.algo == 'rebrac':
                x.update_from_dataset(stream=stream, full_update=i % 2 == 0)
            else:
                x.update_from_dataset(stream=stream)

    def update(self, x):
        if self.algo == 'rebrac':
            return x.update(self.batch, full_update=True, noise=self.noise)
        return x.update(self.batch, noise=self.noise)

    def check_first_update(self, x, params):
        """One update from `params` with zero moments, count 0, step 1, against the fp64 restatement under the bounds of the
        algorithm's own parity suite: infos, every leaf's gradient (Adam mu / 0.1), nu and the post-step parameters."""
        if self.algo == 'fql':
            ref = O.OracleFQL(params, dict(self.cfg), OD, AD, np.float64)
            assert_step_matches(x, ref, self.cfg, self.batch, self.noise)
        elif self.algo == 'ifql':
            from tests.test_gpu_ifql import _check_first_update
            ref = IO.OracleIFQL(params, dict(self.cfg), OD, AD, np.float64)
            _check_first_update(x, ref, self.cfg, params, self.batch, self.noise)
        else:
            from tests.test_gpu_rebrac import _check_step
            ref = RO.OracleReBRAC(params, dict(self.cfg), OD, AD, np.float64)
            _check_step(x, ref, self.batch, self.noise, True, self.cfg, leaf_dict(params))


# ---- direct C-ABI access (the Python getters call leaves() first, and fql_leaf_info waits for the queues) -----------------------------
def _get(x, leaves, which=None):
    out = {}
    for name, shape in leaves:
        a = np.empty(shape, np.float32)
        if which is None:
            x._check(x._lib.fql_get_param(x._h, name.encode(), a.ctypes.data, a.size))
        else:
            x._check(x._lib.fql_get_opt_state(x._h, which, name.encode(), a.ctypes.data, a.size))
        out[name] = a
    return out


def _set(x, leaves, values, which=None):
    for name, _ in leaves:
        a = np.ascontiguousarray(values[name], dtype=np.float32)
        if which is None:
            x._check(x._lib.fql_set_param(x._h, name.encode(), a.ctypes.data, a.size))
        else:
            x._check(x._lib.fql_set_opt_state(x._h, which, name.encode(), a.ctypes.data, a.size))


def _get_step(x):
    c, s = C.c_int64(), C.c_int64()
    x._check(x._lib.fql_get_step(x._h, C.byref(c), C.byref(s)))
    return int(c.value), int(s.value)


def _assert_equal(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f'{what} {k}')


def _assert_same_state(a, b, what=''):
    _assert_equal(leaf_dict(a.get_params()), leaf_dict(b.get_params()), f'{what} params')
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step']), what
    for part in ('mu', 'nu'):
        _assert_equal(leaf_dict(oa[part]), leaf_dict(ob[part]), f'{what} {part}')


ALGOS = ['fql', 'ifql', 'rebrac']


@pytest.mark.parametrize('algo', ALGOS)
def test_reads_right_after_queued_updates(algo):
    """fql_get_param for every leaf and fql_get_opt_state for mu and nu straight after N queued updates: the state after all N."""
    import torch
    s = Setup(algo)
    a, b = s.pair()
    leaves = a.leaves()
    st = torch.cuda.Stream()
    s.queue(b, stream=st.cuda_stream)
    st.synchronize()
    want_p, want_o = leaf_dict(b.get_params()), b.get_opt_state()

    s.queue(a)
    got_p, got_mu, got_nu = _get(a, leaves), _get(a, leaves, 0), _get(a, leaves, 1)
    assert _get_step(a) == (want_o['count'], want_o['step']) == (N, N + 1)
    assert a.synchronize() == 'aql'
    _assert_equal(got_p, want_p, 'params')
    _assert_equal(got_mu, leaf_dict(want_o['mu']), 'mu')
    _assert_equal(got_nu, leaf_dict(want_o['nu']), 'nu')


@pytest.mark.parametrize('algo', ALGOS)
def test_writes_right_after_queued_updates_match_fp64_restatement(algo):
    """fql_set_param of every leaf (the BC flow's included), zero moments through fql_set_opt_state and fql_set_step(0, 1) straight
    after N queued updates, then one update: the restatement's first update from those parameters, and bitwise the twin that
    synchronised before it wrote."""
    import torch
    s = Setup(algo)
    a, b = s.pair()
    leaves = a.leaves()
    X = s.randomized(s.init, 17)
    Xd = leaf_dict(X)
    zeros = {name: np.zeros(shape, np.float32) for name, shape in leaves}
    st = torch.cuda.Stream()
    s.queue(b, stream=st.cuda_stream)
    st.synchronize()
    b.set_params(X)
    b.set_opt_state({'mu': zeros, 'nu': zeros, 'count': 0, 'step': 1})
    s.update(b)

    s.queue(a)
    _set(a, leaves, Xd)
    _set(a, leaves, zeros, 0)
    _set(a, leaves, zeros, 1)
    a._check(a._lib.fql_set_step(a._h, 0, 1))
    s.check_first_update(a, X)
    assert a.synchronize() == 'aql'
    b.synchronize()
    _assert_same_state(a, b)
    assert a.read_info() == b.read_info()


def _restore_case(make_restore):
    """Agent `a` (other parameters) gets the state of a trained source while N updates are in flight, through the function
    `make_restore(source)` returns; 5 more updates must end where a fresh agent restored from the same state ends after them."""
    s = Setup('fql')
    src = s.agent(seed=8)
    s.queue(src, 3)
    src.synchronize()
    restore = make_restore(src)      # (everything read from the source before a's updates are queued)
    a = s.agent(seed=3, params=s.randomized(src.get_params(), 21))
    fresh = s.agent(seed=3)
    restore(fresh)
    s.queue(a)
    restore(a)
    rng = np.random.default_rng(4)
    for k in range(5):
        idxs = rng.integers(0, len(s.ds['observations']), size=B)
        nz = O.make_noise(B, AD, 60 + k)
        for x in (a, fresh):
            x.update_from_dataset(idxs=idxs, noise=nz)
    assert a.synchronize() == 'aql'
    fresh.synchronize()
    _assert_same_state(a, fresh)
    assert a.read_info() == fresh.read_info()


def test_python_set_params_and_set_opt_state_right_after_queued_updates():
    """FQLAgent.set_params / set_opt_state call the setters without a leaves() in front."""
    def make_restore(src):
        params, opt = src.get_params(), src.get_opt_state()
        return lambda x: (x.set_params(params), x.set_opt_state(opt))
    _restore_case(make_restore)


def test_checkpoint_restore_right_after_queued_updates():
    """checkpoint.from_state_dict into a live agent (it reads agent.leaves() before it writes)."""
    from fql_amd import checkpoint

    def make_restore(src):
        sd = checkpoint.to_state_dict(src)
        return lambda x: checkpoint.from_state_dict(x, sd)
    _restore_case(make_restore)


# ---- entry points that already wait for the queues: a later fast path that drops the wait fails here ----------------------------------
def _rows(n=32, seed=9):
    rng = np.random.default_rng(seed)
    return [{'observations': rng.normal(size=OD).astype(np.float32), 'actions': rng.uniform(-1, 1, size=AD).astype(np.float32),
             'rewards': np.float32(rng.normal()), 'masks': np.float32(1.0),
             'next_observations': rng.normal(size=OD).astype(np.float32)} for _ in range(n)]


def _switch_batch(x):
    x._check(x._lib.fql_set_batch_size(x._h, B // 2))
    x._check(x._lib.fql_set_batch_size(x._h, B))


PINS = {
    'set_step': lambda x, s: x._check(x._lib.fql_set_step(x._h, 2, 3)),
    'set_rng_stream': lambda x, s: x.set_rng_stream(7),
    'set_grad_scale': lambda x, s: x.set_grad_scale(0.5),
    'dataset_add': lambda x, s: [x.add_transition(t) for t in _rows()],    # the next updates draw rows from the grown dataset
    'set_batch_size': lambda x, s: _switch_batch(x),
    'total_loss': lambda x, s: x.total_loss(s.batch, noise=s.noise),
    'flow_actions': lambda x, s: x.compute_flow_actions(s.batch['observations'][:16], s.noise['x0'][:16]),
}


@pytest.mark.parametrize('entry', list(PINS))
def test_entry_point_right_after_queued_updates(entry):
    import torch
    s = Setup('fql')
    a, b = s.pair(capacity=len(s.ds['observations']) + 64)
    st = torch.cuda.Stream()
    s.queue(b, stream=st.cuda_stream)
    st.synchronize()
    want = PINS[entry](b, s)
    b.synchronize()              # (the entry point ran on b's own stream, the updates go to st)
    s.queue(b, 2, stream=st.cuda_stream)
    st.synchronize()

    s.queue(a)
    got = PINS[entry](a, s)
    s.queue(a, 2)
    assert a.synchronize() == 'aql'
    if entry == 'flow_actions':
        np.testing.assert_array_equal(got, want)
    elif entry == 'total_loss':
        assert got == want
    if entry == 'dataset_add':
        assert a.dataset_size() == b.dataset_size() and a.dataset_size()[0] == len(s.ds['observations']) + 32
    _assert_same_state(a, b, entry)
    assert a.read_info() == b.read_info()


def test_group_member_access_right_after_queued_group_updates():
    """A member's fql_get_param / fql_get_opt_state / fql_set_param straight after N group updates, without group.synchronize()."""
    from tests.test_gpu_group import _setup
    K = 2
    cfg, ds, batch, noise, group, twins = _setup(K, B, H)
    leaves = [m.leaves() for m in group.members]

    def twin_steps(n):
        for t in twins:
            for _ in range(n):
                t.update_from_dataset(B)
            t.synchronize()

    twin_steps(N)
    for _ in range(N):
        group.update_from_dataset()
    got = [(_get(m, leaves[i]), _get(m, leaves[i], 1)) for i, m in enumerate(group.members)]
    for i, t in enumerate(twins):
        _assert_equal(got[i][0], leaf_dict(t.get_params()), f'member {i} params')
        _assert_equal(got[i][1], leaf_dict(t.get_opt_state()['nu']), f'member {i} nu')
    X = leaf_dict(randomize_params(twins[0].get_params(), 77, scale=0.05))
    twin_steps(N)
    twins[0].set_params(X)
    for _ in range(N):
        group.update_from_dataset()
    _set(group.members[0], leaves[0], X)
    twin_steps(2)
    for _ in range(2):
        group.update_from_dataset()
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        _assert_same_state(m, t, f'member {i}')
        assert m.read_info() == t.read_info(), i
    group.close()
