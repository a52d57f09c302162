"""GPU: the FQL update's fused tail (fql_kernels.h fql_adam_body).  By default the update has no finalize launch:
every workgroup of its two Adam launches (critic + BC flow on one lane, one-step actor on another, no edge between them) takes a ticket,
and the one that takes the last runs the finalize code.  An agent created with FQL_FUSED_TAIL=0 keeps the finalize launch.  Only the
workgroup that runs that code differs, so twins with the same seed, rows and noise must agree bitwise: the 13 infos of every update,
every parameter leaf (the target's among them), both Adam moments, the optax count and the step.

FQL_AQL is read once per process, so the captured-graph form of the first case runs in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import assert_same_state, make_problem, randomize_params, read_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'FQL_FUSED_TAIL'
OP_ADAM, OP_FINALIZE = 25, 26     # enum OpType (fql_amd/csrc/fql_engine.hip)
OD, AD = 29, 8


def _with_switch_off(make):
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = '0'
    try:
        return make()
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


def _twins(B, hidden, seed=3):
    """(agent with the default tail, its twin created with the switch off, dataset)."""
    import fql_amd
    cfg, ds, batch, _ = make_problem(OD, AD, B, hidden, seed=seed)

    def make():
        a = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed + 1))
        a.upload_dataset(ds)
        return a
    return make(), _with_switch_off(make), ds


def _adam_grids(agent):
    return [L['grid'] for L in read_plan(agent) if L['type'] == OP_ADAM]


def _assert_fused_and_not(a, b):
    ta, tb = [L['type'] for L in read_plan(a)], [L['type'] for L in read_plan(b)]
    assert OP_FINALIZE not in ta and ta.count(OP_ADAM) == 2, ta
    assert tb.count(OP_FINALIZE) == 1 and tb.count(OP_ADAM) == 2, tb


def _run(a, b, ds, B, steps, rng_seed=5, first_noise=40):
    """`steps` updates of both agents on the same rows and noise: the infos of every update bitwise equal."""
    mode = 'graph' if os.environ.get('FQL_AQL') == '0' else 'aql'
    rng = np.random.default_rng(rng_seed)
    for step in range(steps):
        idxs = rng.integers(0, len(ds['observations']), size=B)
        nz = O.make_noise(B, AD, first_noise + step)
        for x in (a, b):
            x.update_from_dataset(B, idxs=idxs, noise=nz)
        assert a.synchronize() == mode and b.synchronize() == mode
        ia, ib = a.read_info(), b.read_info()
        assert len(ia) == 13 and ia == ib, (step, ia, ib)
        assert all(np.isfinite(v) for v in ia.values()), (step, ia)


def check_twin_40_updates():
    B = 32
    a, b, ds = _twins(B, (64,) * 4)
    _assert_fused_and_not(a, b)
    _run(a, b, ds, B, 40)
    assert_same_state(a, b)
    assert a.get_opt_state()['count'] == 40 and a.get_opt_state()['step'] == 41
    a.close(); b.close()


def test_twin_bitwise_on_the_engines_queues():
    """H 64, B 32, 40 updates on the engine's own AQL queues."""
    assert os.environ.get('FQL_AQL') != '0'
    check_twin_40_updates()


def test_twin_bitwise_as_a_captured_graph():
    """The same 40 updates with FQL_AQL=0: the captured graph, its two Adam launches in parallel branches."""
    code = f'import sys; sys.path.insert(0, {ROOT!r})\nimport tests.test_gpu_fused_tail as t\nt.check_twin_40_updates()\nprint("TWIN OK", flush=True)\n'
    env = dict(os.environ, FQL_AQL='0')
    env.pop(SWITCH, None)
    out = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    assert 'TWIN OK' in out.stdout


def test_kernels_of_more_than_one_chunk():
    """H 128 x 3, B 64: a 128 x 128 kernel is four Adam chunks of 4096, so the finalize fold's quarters each hold a chunk."""
    B = 64
    a, b, ds = _twins(B, (128,) * 3)
    _run(a, b, ds, B, 3)
    assert_same_state(a, b)
    a.close(); b.close()


def test_flagship_shape_under_load():
    """H 512 x 4, B 256: 844 Adam workgroups in two launches that run beside each other and beside the weight-copy refresh, so the last
    ticket falls in either launch and the partials it reads were written on every XCD."""
    B = 256
    a, b, ds = _twins(B, (512,) * 4)
    assert _adam_grids(a) == [637, 207]        # (critic + BC flow, one-step actor: the chunks of the three modules)
    _run(a, b, ds, B, 12)
    assert_same_state(a, b)
    a.close(); b.close()


def test_smallest_last_adam_launch():
    """One hidden layer of 16 units, the narrowest padded width.  An Adam chunk never spans two leaves, so the one-step actor's launch is
    never ONE workgroup: its smallest form is a workgroup per leaf (two kernels, two biases), each a fraction of a chunk, and the
    other launch is as small.  All of them arrive within a few hundred nanoseconds; whichever comes last must find every partial."""
    B = 32
    a, b, ds = _twins(B, (16,))
    assert _adam_grids(a)[-1] == 4 and _adam_grids(b)[-1] == 4, (_adam_grids(a), _adam_grids(b))
    _run(a, b, ds, B, 10)
    assert_same_state(a, b)
    a.close(); b.close()


def test_ticket_returns_to_zero():
    """70 consecutive updates on one handle (rows and noise from the device RNG, so the RNG step counts too), a batch-size change, which
    rebuilds the program around the same ticket word, then 6 more: a ticket that did not return to 0 would name no last arriver (or a
    wrong one) in the next update, and the counters and grad statistics would stop or come early."""
    B = 32
    a, b, ds = _twins(B, (64,) * 4)
    for step in range(70):
        for x in (a, b):
            x.update_from_dataset(B)
        ia, ib = a.read_info(), b.read_info()
        assert ia == ib, (step, ia, ib)
    assert a.get_opt_state()['count'] == 70
    assert_same_state(a, b)
    B2 = 48
    _run(a, b, ds, B2, 5)
    for x in (a, b):
        x.update_from_dataset(B2)                # (device RNG again: its step followed the 75 updates)
    assert a.read_info() == b.read_info()
    assert a.get_opt_state()['count'] == 76 and a.get_opt_state()['step'] == 77
    assert_same_state(a, b)
    a.close(); b.close()


def test_group_members_at_different_counts():
    """Three members at Adam counts 1, 9 and 999 (tests/test_gpu_optimizer.py's group case), one fused update: every member has a ticket of
    its own in the two multi-instance Adam launches, and ends bitwise where its stand-alone agent ends."""
    from tests import optimizer_cases as C
    from tests.test_gpu_group import _assert_same_state, _setup
    od, ad, B, hidden = C.STATE_CASES['ragged']
    cfg, ds, batch, noise, group, twins = _setup(3, B, hidden, od=od, ad=ad)
    assert OP_FINALIZE not in [L['type'] for L in read_plan(group.members[0])]
    for i, count in enumerate((1, 9, 999)):
        ref = O.OracleFQL(twins[i].get_params(), dict(cfg, alpha=10.0 * (i + 1)), od, ad, np.float64)   # (_setup's alphas)
        mu0, nu0 = C.carried_moments(40 + i, C.trainable(ref.grads(batch, noise)[2]), count)
        for x in (group.members[i], twins[i]):
            x.set_opt_state({'mu': C.unflatten(mu0), 'nu': C.unflatten(nu0), 'count': count, 'step': count + 1})
    idxs = np.random.default_rng(5).integers(0, len(ds['observations']), size=(3, B))
    group.update_from_dataset(idxs=idxs)
    for i, t in enumerate(twins):
        t.update_from_dataset(B, idxs=idxs[i])
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        assert m.get_opt_state()['count'] == (1, 9, 999)[i] + 1
        assert all(np.isfinite(v) for v in m.read_info().values()), m.read_info()
        _assert_same_state(m, t, f'member {i}')
    group.close()


def test_plan_of_the_default_agent():
    """No finalize launch, one launch fewer than the twin, and every other launch is the twin's: same lanes, grids and tasks, the Adam
    launches among them.  (The actor-loss metrics keep their launch: taking them into the critic's Adam launch measured nothing.)"""
    a, b, _ = _twins(32, (64,) * 4)
    _assert_fused_and_not(a, b)
    assert a.stats()['launches_per_update'] == b.stats()['launches_per_update'] - 1 == len(read_plan(a))
    assert a.stats()['macs_per_update'] == b.stats()['macs_per_update']
    assert _adam_grids(a) == _adam_grids(b)
    pa, pb = [dict(L, index=0) for L in read_plan(a)], [dict(L, index=0) for L in read_plan(b) if L['type'] != OP_FINALIZE]
    assert pa == pb
    a.close(); b.close()
