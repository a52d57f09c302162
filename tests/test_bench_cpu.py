"""CPU: the bookkeeping around bench.py's static counters - the committed PMC summary names the kernel sources it was measured on, bench.py marks it
stale when they differ."""
import importlib.util
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_source_hash_follows_the_kernel_sources(tmp_path):
    pmc = _load('pmc_summary', os.path.join(ROOT, 'tools', 'pmc_summary.py'))
    root = tmp_path / 'r'
    shutil.copytree(os.path.join(ROOT, 'fql_amd', 'csrc'), root / 'fql_amd' / 'csrc')
    a = pmc.source_sha16(str(root))
    assert a == pmc.source_sha16(ROOT) and len(a) == 16
    with open(root / 'fql_amd' / 'csrc' / 'fql_aux.h', 'a') as f:
        f.write('\n// edited\n')
    assert pmc.source_sha16(str(root)) != a


def test_committed_pmc_summary_belongs_to_this_tree_and_bench_reads_it():
    bench = _load('bench_mod', os.path.join(ROOT, 'bench.py'))
    pmc = _load('pmc_summary', os.path.join(ROOT, 'tools', 'pmc_summary.py'))
    path = os.path.join(ROOT, 'profiles', bench.PMC_FILE)
    assert os.path.exists(path), 'run tools/profile.sh and copy its summary into profiles/'
    pj = json.load(open(path))
    got = bench.pmc_counters(bench.PMC_FILE, 'fql_side_kernel')
    assert got['traffic'] == pj['kernels']['fql_side_kernel']['hbm_bytes_per_launch'] > 0
    assert got['traffic_source_sha16'] == pj['source_sha16']
    assert got['traffic_stale'] == (pj['source_sha16'] != pmc.source_sha16(ROOT))
    if got['traffic_stale']:   # not an error (bench.py says so in its line), but worth seeing in the test log
        import warnings
        warnings.warn('fql_amd/csrc changed after profiles/%s was measured: re-run tools/profile.sh' % bench.PMC_FILE)
    assert bench.pmc_counters('no_such_file.json', 'fql_side_kernel') == {}


def test_dump_outputs_writes_float32_leaves_and_samples_past_the_cap(tmp_path):
    import numpy as np
    bench = _load('bench_mod', os.path.join(ROOT, 'bench.py'))
    rng = np.random.default_rng(0)
    params = {'modules_critic': {'Dense_0': {'kernel': rng.standard_normal((64, 32)), 'bias': rng.standard_normal(32).astype(np.float32)}},
              'modules_actor': {'Dense_0': {'kernel': rng.standard_normal((16, 8)).astype(np.float32)}}}
    info = {'critic/critic_loss': 1.5, 'grad/norm': 2.25}
    full = bench.dump_outputs(str(tmp_path / 'full'), info, params)
    assert full['files'] == 5 and not full['sampled']
    k = np.load(tmp_path / 'full' / 'params__modules_critic__Dense_0__kernel.npy')
    assert k.dtype == np.float32 and k.shape == (64, 32)
    np.testing.assert_array_equal(k, params['modules_critic']['Dense_0']['kernel'].astype(np.float32))
    assert float(np.load(tmp_path / 'full' / 'info__grad__norm.npy')) == 2.25
    # past the cap: a fixed, seeded subset of every leaf, the same on every call, within the byte budget
    cap = 4 * 1000
    a = bench.dump_outputs(str(tmp_path / 'a'), info, params, cap_bytes=cap)
    b = bench.dump_outputs(str(tmp_path / 'b'), info, params, cap_bytes=cap)
    assert a['sampled'] and a['bytes'] <= cap and a['files'] == 5
    for f in sorted(os.listdir(tmp_path / 'a')):
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x, y)
    s = np.load(tmp_path / 'a' / 'params__modules_critic__Dense_0__kernel.npy')
    assert 0 < s.size < 64 * 32 and np.isin(s, params['modules_critic']['Dense_0']['kernel'].astype(np.float32)).all()
