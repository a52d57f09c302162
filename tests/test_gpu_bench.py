"""GPU: bench.py --dump-outputs.  Two runs with the same arguments time exactly --steps updates and dump the same outputs of the last one,
bit for bit (seeded synthetic replay, seeded device RNG, fixed-order reductions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2', '--rows', '8192',
                        '--no-extras', '--no-cpu-baseline', '--dump-outputs', str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_for_the_same_arguments(tmp_path):
    a, b = _bench(tmp_path / 'a', 7), _bench(tmp_path / 'b', 7)
    for res in (a, b):
        assert res['steps'] == 7 and res['ms_per_step'] > 0
        assert res['dumped_outputs']['bytes'] <= 64 << 20 and not res['dumped_outputs']['sampled']
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert sum(f.startswith('info__') for f in files) == 13 and sum(f.startswith('params__') for f in files) > 0
    for f in files:
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert x.dtype == np.float32 and np.isfinite(x).all(), f
        np.testing.assert_array_equal(x, y, err_msg=f)
    for k, v in a['last_info'].items():
        assert abs(float(np.load(tmp_path / 'a' / ('info__' + k.replace('/', '__') + '.npy'))) - v) <= 1e-5 * max(1.0, abs(v)), k
    # a different number of timed steps is a different last step
    c = _bench(tmp_path / 'c', 8)
    assert c['steps'] == 8
    assert not np.array_equal(np.load(tmp_path / 'a' / 'info__critic__critic_loss.npy'), np.load(tmp_path / 'c' / 'info__critic__critic_loss.npy'))
