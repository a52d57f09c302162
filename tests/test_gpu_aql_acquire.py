"""GPU: update programs on the engine's own AQL queues without an acquire between their kernel packets (fql_engine.hip build_aql; DESIGN.md
section 4).  Such a program's kernels read everything an earlier launch of the program wrote past the L1 (fql_kernels.h ldx), so no CU can
serve a stale line; the twin of every case runs the captured graph on a caller's stream, where HIP keeps an acquire in front of every kernel.
Same kernels, same arguments, same order: bitwise equal, or a load was missed.

The shapes are small on purpose: a buffer of a few KB that a CU re-reads is the one a stale L1 line would be served from (a 64 KB streaming
read evicts itself and hides the hazard), and 40 updates rewrite and re-read every workspace buffer dozens of times.

Every parity case first reads the packets' fences back through the diagnostic export fql_debug_aql_fences, so parity is never asserted on a
program that silently kept its acquires."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_group import _assert_same_state as assert_same_group_state, _setup as group_setup
from tests.util import assert_same_state, make_problem, randomize_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, AGENT, SYSTEM = 0, 1, 2     # hsa_fence_scope_t


def aql_fences(agent=None, group=None):
    """(every launch binds an L1-independent kernel, FQL_AQL_ACQUIRE was set, [(lane, acquire, release) per kernel packet]) of an agent's
    update program on the engine's queues (no packets before its first update there), or of a group's fused program (never any packets)."""
    from fql_amd import _cabi
    fn = _cabi.load().fql_debug_aql_fences
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn.restype = C.c_int
    h, g = (agent._h if agent is not None else None), (group._g if group is not None else None)
    head = np.zeros(1, np.int32)
    assert fn(h, g, head.ctypes.data, 4) == 0
    w = np.zeros(int(head[0]), np.int32)
    assert fn(h, g, w.ctypes.data, w.nbytes) == 0
    w = [int(v) for v in w]
    assert len(w) == 4 + 3 * w[3]
    return bool(w[1]), bool(w[2]), [tuple(w[4 + 3 * i:7 + 3 * i]) for i in range(w[3])]


def assert_fences(agent, dropped):
    """The program's kernel packets: release agent on every one, acquire system on the first of each lane, and on the others none (dropped) or
    agent (kept)."""
    table, switch, packets = aql_fences(agent)
    assert packets, 'no AQL program: the update did not run on the engine\'s queues'
    assert table == dropped and not switch, (table, switch)
    seen = set()
    for lane, acq, rel in packets:
        assert rel == AGENT, (lane, acq, rel)
        assert acq == (SYSTEM if lane not in seen else NONE if dropped else AGENT), (lane, acq, rel, dropped)
        seen.add(lane)
    assert len(packets) > len(seen)       # there are interior packets to speak of
    return len(packets)


def _pair(od, ad, B, hidden, precision='fp32', seed=11, **cfgkw):
    """tests/test_gpu_aql.py::_pair at a shape, a precision and config overrides of its own."""
    import fql_amd
    cfg, ds, batch, _ = make_problem(od, ad, B, hidden, seed=seed, **cfgkw)
    cfg['precision'] = precision
    agents = []
    for _ in range(2):
        a = fql_amd.FQLAgent.create(3, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed + 1, scale=0.05 if max(hidden) >= 512 else 0.1))
        a.upload_dataset(ds)
        agents.append(a)
    return agents


def check_parity(od, ad, B, hidden, updates, precision='fp32', dropped=True, **cfgkw):
    import torch
    a, b = _pair(od, ad, B, hidden, precision, **cfgkw)
    st = torch.cuda.Stream()
    for step in range(1, updates + 1):
        a.update_from_dataset(B)                              # stream left to the engine: its own queues; rows and noise from the engine RNG
        b.update_from_dataset(B, stream=st.cuda_stream)       # a caller's stream: the captured graph
        if step == 1:                                         # (the packets exist from the first update on)
            assert a.synchronize() == 'aql' and b.synchronize() == 'graph'
            n = assert_fences(a, dropped)
            print(f'{od}x{ad} B {B} hidden {hidden} {precision} {cfgkw}: {n} kernel packets, interior acquires {"dropped" if dropped else "kept"}')
        if step % 10 == 0 or step == updates:
            assert a.synchronize() == 'aql' and b.synchronize() == 'graph'
            st.synchronize()
            ia, ib = a.read_info(), b.read_info()
            assert ia == ib, (step, ia, ib)
    assert_same_state(a, b)
    a.close()
    b.close()


FP32 = [pytest.param(29, 8, 16, (128,) * 4, 40, {}, id='b16_h128'),
        pytest.param(29, 8, 64, (128,) * 4, 40, {}, id='b64_h128'),
        pytest.param(13, 4, 32, (256,) * 2, 40, {}, id='b32_h256x2'),
        pytest.param(29, 8, 256, (512,) * 4, 6, {}, id='b256_h512'),
        # the dynamic dQ scale, the Euler-finish launch and the loss-gradient paths
        pytest.param(29, 8, 16, (128,) * 4, 40, dict(normalize_q_loss=True), id='b16_h128-normalize_q_loss'),
        pytest.param(29, 8, 16, (128,) * 4, 40, dict(actor_layer_norm=True), id='b16_h128-actor_layer_norm')]


@pytest.mark.parametrize('od, ad, B, hidden, updates, cfgkw', FP32)
def test_queues_without_interior_acquires_equal_graph_bitwise(od, ad, B, hidden, updates, cfgkw):
    check_parity(od, ad, B, hidden, updates, **cfgkw)


@pytest.mark.parametrize('B', [16, 64])
def test_bf16x3_queues_without_interior_acquires_equal_graph_bitwise(B):
    check_parity(29, 8, B, (128,) * 4, 40, precision='bf16x3')


def _infos_after_10(tag):
    import fql_amd
    cfg, ds, batch, _ = make_problem(29, 8, 16, (128,) * 4, seed=11)
    a = fql_amd.FQLAgent.create(3, batch['observations'][:1], batch['actions'][:1], cfg)
    a.set_params(randomize_params(a.get_params(), 12))
    a.upload_dataset(ds)
    for _ in range(10):
        a.update_from_dataset(16)
    assert a.synchronize() == 'aql'
    table, switch, packets = aql_fences(a)
    info = a.read_info()
    print(tag, int(table), int(switch), sorted({(acq, rel) for _, acq, rel in packets}), [np.float32(info[k]).view(np.uint32) for k in sorted(info)], flush=True)
    a.close()
    return table, switch, packets, info


def run_switch_child():
    _infos_after_10('SWITCH')


def test_switch_brings_the_acquires_back():
    """FQL_AQL_ACQUIRE=1 (read when an engine is created) in a child process: agent acquires on every interior packet, the same infos."""
    table, switch, packets, info = _infos_after_10('DEFAULT')
    assert table and not switch and NONE in {acq for _, acq, _ in packets}
    code = f'import sys; sys.path.insert(0, {ROOT!r})\nimport tests.test_gpu_aql_acquire as t\nt.run_switch_child()\n'
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, FQL_AQL_ACQUIRE='1'), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith('SWITCH ')][-1]
    want_bits = str([np.float32(info[k]).view(np.uint32) for k in sorted(info)])
    # every packet acquires: system on a lane's first, agent on the rest; release agent throughout
    assert line == f'SWITCH 1 1 {sorted({(SYSTEM, AGENT), (AGENT, AGENT)})} {want_bits}', (line, want_bits)


def test_another_kind_keeps_every_acquire():
    import fql_amd
    _, ds, batch, _ = make_problem(29, 8, 32, (64,) * 2, seed=5)
    cfg = fql_amd.iql.get_config()
    cfg.update(actor_hidden_dims=(64, 64), value_hidden_dims=(64, 64), batch_size=32)
    a = fql_amd.IQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], cfg)
    a.upload_dataset(ds)
    for _ in range(3):
        a.update_from_dataset(32)
    assert a.synchronize() == 'aql'
    assert_fences(a, dropped=False)
    assert all(np.isfinite(v) for v in a.read_info().values())
    a.close()


def test_group_of_two_is_consistent_with_the_table_and_equals_its_members():
    """A group runs its fused program as a captured graph: no packets of its own.  Its table word is that of its kernels (the members' kernels
    or their multi-instance twins), and group against stand-alone members stays bitwise, the members running without interior acquires."""
    K, B, H = 2, 32, 128
    _, _, _, _, group, twins = group_setup(K, B, H)
    for _ in range(12):
        group.update_from_dataset()
        for t in twins:
            t.update_from_dataset(B)
    group.synchronize()
    table, switch, packets = aql_fences(group=group)
    assert not packets and not switch
    for t in twins:
        assert t.synchronize() == 'aql'
        assert_fences(t, dropped=True)
    assert table == aql_fences(twins[0])[0]
    for i, (m, t) in enumerate(zip(group.members, twins)):
        assert_same_group_state(m, t, f'member {i}')
    group.close()
