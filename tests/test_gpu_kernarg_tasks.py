"""GPU: side-lane launches with their tasks in the kernel arguments (fql_kernels.h find_front; the fql_side*_ka_kernel entry points) against
the same launches reading their tables in HBM (FQL_KERNARG_TASKS=0, read when an agent is created).  Only the place the task bytes come from
differs, so twins with the same seed, rows and noise must agree bitwise: the 13 infos, every parameter leaf and both Adam moments.

Every case runs on the engine's own AQL queues (kernarg blocks the engine fills) and, in one child process for all of them, with
FQL_AQL=0 (the captured graph, kernarg blocks HIP fills).  The form of each launch is read from the diagnostic export
fql_debug_task_forms: 0 = no task table, 1 = table in HBM, 2 = kernel arguments."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.test_gpu_group import _assert_same_state as assert_same_group_state, _setup as group_setup
from tests.util import K_GEMM16_KBIG, OP_GEMM64, assert_same_state, make_problem, randomize_params, read_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 'FQL_KERNARG_TASKS'
CAPS = ('gemm', 'wgrad', 'ln', 'misc')


def task_forms(agent=None, group=None):
    """(capacities of the argument form by family, [form of each launch]) of an agent's update program or a group's fused one."""
    from fql_amd import _cabi
    lib = _cabi.load()
    fn = lib.fql_debug_task_forms
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn.restype = C.c_int
    h, g = (agent._h if agent is not None else None), (group._g if group is not None else None)
    head = np.zeros(1, np.int32)
    assert fn(h, g, head.ctypes.data, 4) == 0
    w = np.zeros(int(head[0]), np.int32)
    assert fn(h, g, w.ctypes.data, w.nbytes) == 0
    w = [int(v) for v in w]
    assert w[5] == len(w) - 6
    return dict(zip(CAPS, w[1:5])), w[6:]


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


def _fql(od, ad, B, hidden, precision, seed=3):
    import fql_amd
    cfg, ds, batch, _ = make_problem(od, ad, B, hidden, seed=seed)
    cfg['precision'] = precision

    def make():
        a = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed + 1, scale=0.05 if max(hidden) >= 512 else 0.1))
        a.upload_dataset(ds)
        return a
    return make, ds, lambda step: O.make_noise(B, ad, 40 + step)


def _ifql(od, ad, B, hidden, precision, seed=3):
    import fql_amd
    _, ds, batch, _ = make_problem(od, ad, B, hidden, seed=seed)
    cfg = fql_amd.ifql.get_config()
    cfg.update(actor_hidden_dims=tuple(hidden), value_hidden_dims=tuple(hidden), batch_size=B)

    def make():
        a = fql_amd.IFQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed + 1))
        a.upload_dataset(ds)
        return a

    def noise(step):
        nz = O.make_noise(B, ad, 40 + step)
        return {'x0': nz['x0'], 't': nz['t']}
    return make, ds, noise


# kind, od, ad, B, hidden, precision
CASES = [pytest.param(k, od, ad, B, hid, prec, id=f'{name}-{prec}')
         for name, k, od, ad, B, hid in [('b32_h64', _fql, 29, 8, 32, (64,) * 4),        # one K chunk: the 16-row heads, the K <= 64 first layers
                                         ('b64_h128', _fql, 29, 8, 64, (128,) * 4),      # two chunks: both pipeline arms
                                         ('ragged', _fql, 80, 48, 32, (64,) * 4)]        # obs 80, act 48: padded widths, ap = 48
         for prec in ('fp32', 'bf16x3')]
CASES += [pytest.param(_ifql, 29, 8, 32, (64,) * 4, 'fp32', id='ifql_b32_h64-fp32'),       # another agent's task mixes
          # tests/test_gpu_shapes.py wide1024: every GEMM on the 16-row K > 512 kernel, which keeps its table (the argument form did not
          # measure there, MEASUREMENTS.md); the side-lane launches of this shape carry weight-gradient, LayerNorm-backward and loss tasks only
          pytest.param(_fql, 29, 8, 32, (1024,) * 3, 'fp32', id='wide1024-fp32')]


def check_case(kind, od, ad, B, hidden, precision):
    """Three updates from given rows and noise on an agent and its twin created with the switch off: bitwise equal.  The agent must hold
    launches in the argument form, the twin none, and both the same table launches."""
    make, ds, noise = kind(od, ad, B, hidden, precision)
    a, b = make(), _with_switch_off(make)
    (_, fa), (_, fb) = task_forms(a), task_forms(b)
    assert 2 in fa and 2 not in fb and [f != 0 for f in fa] == [f != 0 for f in fb], (fa, fb)
    plan = read_plan(a)
    assert all((fa[L['index']] == 2) == (L['type'] == OP_GEMM64) for L in plan), (fa, plan)   # every side-lane launch fits here, no other takes the form
    if max(hidden) > 512:
        assert any(L['kernel'] == K_GEMM16_KBIG for L in plan)
    mode = 'graph' if os.environ.get('FQL_AQL') == '0' else 'aql'
    rng = np.random.default_rng(5)
    for step in range(3):
        idxs = rng.integers(0, len(ds['observations']), size=B)
        nz = noise(step)
        for x in (a, b):
            x.update_from_dataset(B, idxs=idxs, noise=nz)
        assert a.synchronize() == mode and b.synchronize() == mode
        ia, ib = a.read_info(), b.read_info()
        assert len(ia) == 13 or kind is _ifql
        assert ia == ib, (step, ia, ib)
    assert_same_state(a, b)


@pytest.mark.parametrize('kind, od, ad, B, hidden, precision', CASES)
def test_argument_form_equals_table_form_bitwise(kind, od, ad, B, hidden, precision):
    check_case(kind, od, ad, B, hidden, precision)


def run_cases_in_this_process():
    for c in CASES:
        check_case(*c.values)
        print('CASE OK', c.id, flush=True)
    print('CASES', len(CASES), flush=True)


def test_every_case_with_aql_off():
    """FQL_AQL is read once per process, so the captured-graph form of every case above runs in one child."""
    code = f'import sys; sys.path.insert(0, {ROOT!r})\nimport tests.test_gpu_kernarg_tasks as t\nt.run_cases_in_this_process()\n'
    env = dict(os.environ, FQL_AQL='0')
    env.pop(SWITCH, None)
    out = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    assert f'CASES {len(CASES)}' in out.stdout


def test_group_level_over_the_capacity_keeps_its_table():
    """A group whose fused levels carry K times the tasks: K is the smallest size at which some level of the member's program exceeds a
    capacity of the argument form (read from the engine, with the member's plan).  That launch keeps its table, the levels that still fit
    take the argument form, and every member ends bitwise where its stand-alone twin ends."""
    import fql_amd
    od, ad, B, H = 29, 8, 64, 128
    cfg, _, batch, _ = make_problem(od, ad, B, (H,) * 4, seed=7)
    probe = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    caps, forms = task_forms(probe)
    need = []   # per launch in the argument form: the smallest K that exceeds a capacity
    for L in read_plan(probe):
        if forms[L['index']] != 2:
            continue
        counts = [(len(L['gemm']), caps['gemm']), (len(L['wgrad']), caps['wgrad']), (len(L['ln']), caps['ln'])]
        if any(n for n, _ in counts):      # (a launch of loss / metric tasks alone names no count in the plan)
            need.append(min(cap // n + 1 for n, cap in counts if n))
    probe.close()
    K = min(need)
    assert 2 <= K <= 8 and max(need) > K, need     # some level exceeds at K, some other still fits
    _, _, _, _, group, twins = group_setup(K, B, H)
    _, fm = task_forms(group.members[0])
    _, fg = task_forms(group=group)
    assert len(fm) == len(fg) and [f != 0 for f in fm] == [f != 0 for f in fg]
    assert any(m == 2 and g == 1 for m, g in zip(fm, fg)), 'no fused level fell back to its table'
    assert any(g == 2 for g in fg), 'no fused level kept the argument form'
    for _ in range(5):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        assert_same_group_state(m, t, f'member {i}')
    group.close()
