"""IFQL against FQL in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) at B 256 and B 1024.  Both agents
update from a device-resident synthetic dataset on their default path (stream left to the engine = its own queues), timed in alternating
fenced windows.  Also the host-observed latency of one single-observation sample_actions call (IFQL: best of N = 32 flow samples; FQL:
the one-step policy).  Prints one JSON object (and writes it to out.json when given).
usage: python experiments/ifql_rate.py [rounds] [updates per window] [out.json or -] [--ifql-only]
(--ifql-only: IFQL updates at B 256 alone, no FQL agent and no sampling - the run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

ifql_only = '--ifql-only' in sys.argv
if ifql_only:
    sys.argv.remove('--ifql-only')
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 300
out = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] not in ('', '-') else None
H = 512


def window(agent, k):
    agent.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        agent.update_from_dataset()
    agent.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


res = {'shapes': 'obs 29, act 8, hidden 512 x 4, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
if ifql_only:
    _, ds, batch, _ = make_problem(29, 8, 256, (H,) * 4, seed=3)
    a = fql_amd.IFQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], fql_amd.ifql.get_config())
    a.upload_dataset(ds)
    us = [window(a, n) for _ in range(rounds)]
    print(json.dumps({'B': 256, 'ifql_us_per_update': statistics.median(us)}))
    sys.exit(0)
for B in (256, 1024):
    fcfg, ds, batch, _ = make_problem(29, 8, B, (H,) * 4, seed=3)
    icfg = fql_amd.ifql.get_config()
    icfg.update(batch_size=B)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    f = fql_amd.FQLAgent.create(0, ex_o, ex_a, fcfg)
    i = fql_amd.IFQLAgent.create(0, ex_o, ex_a, icfg)
    for a in (f, i):
        a.upload_dataset(ds)
        window(a, 30)
    tf, ti = [], []
    for _ in range(rounds):
        tf.append(window(f, n))
        ti.append(window(i, n))
    st = {}
    for name, a in (('fql', f), ('ifql', i)):
        s = a.stats()
        st[name] = {'launches_per_update': s['launches_per_update'], 'macs_per_sample': s['macs_per_update'] / B}
    res['batches'].append({
        'B': B,
        'fql_us_per_update': statistics.median(tf), 'ifql_us_per_update': statistics.median(ti),
        'fql_updates_per_s': 1e6 / statistics.median(tf), 'ifql_updates_per_s': 1e6 / statistics.median(ti),
        'fql_windows_us': tf, 'ifql_windows_us': ti, 'stats': st,
    })
    if B == 256:   # single-observation sample_actions, host numpy in and out (what an evaluation rollout calls)
        ob = batch['observations'][0]
        lat = {}
        for name, a in (('fql', f), ('ifql', i)):
            for _ in range(20):
                a.sample_actions(ob, seed=1)
            ts = []
            for k in range(200):
                t0 = time.perf_counter()
                a.sample_actions(ob, seed=k)
                ts.append((time.perf_counter() - t0) * 1e6)
            lat[name] = {'median_us': statistics.median(ts), 'p90_us': float(np.percentile(ts, 90))}
        res['sample_actions_single_obs'] = lat
    f.close(); i.close()
print(json.dumps(res, indent=1))
if out:
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
