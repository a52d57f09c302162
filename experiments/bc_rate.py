"""BC against IFQL in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) at B 256 and B 1024.  BC's update is
the flow actor's forward and backward of IFQL's update without the value and critic nets, so IFQL's us per update is the yardstick and the
spread of its own repeated 20-update windows the margin.  Both agents update from a device-resident synthetic dataset on their default path
(stream left to the engine = its own queues), timed in alternating fenced windows.  Also the host-observed latency of one sampling call at
n = 1 and n = 256 rows: BC's sample_actions (denoise_steps = 16 Euler steps) beside IFQL's flow sampler (compute_flow_actions, flow_steps
= 10), each per call and per Euler step.  Prints one JSON object (and writes it to out.json when given).
usage: python experiments/bc_rate.py [rounds] [updates per window] [out.json or -] [--bc-only]
(--bc-only: BC updates at B 256 alone and 20 sampling calls - the run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

bc_only = '--bc-only' in sys.argv
if bc_only:
    sys.argv.remove('--bc-only')
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] not in ('', '-') else None
H = 512


def window(agent, k):
    agent.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        agent.update_from_dataset()
    agent.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def bc_agent(B, ex_o, ex_a):
    cfg = fql_amd.bc.get_config()
    cfg.update(batch_size=B)
    return fql_amd.BCAgent.create(0, ex_o, ex_a, cfg)


def latency(call, reps=200):
    for _ in range(20):
        call(0)
    ts = []
    for k in range(reps):
        t0 = time.perf_counter()
        call(k)
        ts.append((time.perf_counter() - t0) * 1e6)
    return {'median_us': statistics.median(ts), 'p90_us': float(np.percentile(ts, 90))}


res = {'shapes': 'obs 29, act 8, hidden 512 x 4, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
if bc_only:
    _, ds, batch, _ = make_problem(29, 8, 256, (H,) * 4, seed=3)
    a = bc_agent(256, batch['observations'][:1], batch['actions'][:1])
    a.upload_dataset(ds)
    us = [window(a, n) for _ in range(rounds)]
    for k in range(20):
        a.sample_actions(batch['observations'][0], seed=k)
    print(json.dumps({'B': 256, 'bc_us_per_update': statistics.median(us)}))
    sys.exit(0)
for B in (256, 1024):
    _, ds, batch, _ = make_problem(29, 8, B, (H,) * 4, seed=3)
    icfg = fql_amd.ifql.get_config()
    icfg.update(batch_size=B)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    b = bc_agent(B, ex_o, ex_a)
    i = fql_amd.IFQLAgent.create(0, ex_o, ex_a, icfg)
    for a in (b, i):
        a.upload_dataset(ds)
        window(a, 60)
    tb, ti = [], []
    for _ in range(rounds):
        tb.append(window(b, n))
        ti.append(window(i, n))
    la, ma, ls = b.bc_stats()
    s = i.stats()
    res['batches'].append({
        'B': B,
        'bc_us_per_update': statistics.median(tb), 'ifql_us_per_update': statistics.median(ti),
        'ifql_window_spread_us': max(ti) - min(ti), 'bc_window_spread_us': max(tb) - min(tb),
        'bc_below_ifql_by_more_than_the_spread': statistics.median(ti) - statistics.median(tb) > max(ti) - min(ti),
        'bc_windows_us': tb, 'ifql_windows_us': ti,
        'stats': {'bc': {'launches_per_update': la, 'macs_per_sample': ma / B, 'launches_per_sampling_call': ls},
                  'ifql': {'launches_per_update': s['launches_per_update'], 'macs_per_sample': s['macs_per_update'] / B}},
    })
    if B == 256:   # host numpy in and out (what an evaluation rollout calls)
        lat = {}
        for rows in (1, 256):
            ob = batch['observations'][:rows]
            z = np.random.default_rng(0).standard_normal((rows, 8)).astype(np.float32)
            lb = latency(lambda k: b.sample_actions(ob if rows > 1 else ob[0], noises=z if rows > 1 else z[0]))
            li = latency(lambda k: i.compute_flow_actions(ob, z))
            lb['per_euler_step_us'] = lb['median_us'] / 16
            li['per_euler_step_us'] = li['median_us'] / 10
            lat[f'n={rows}'] = {'bc_sample_actions_16_steps': lb, 'ifql_flow_sampler_10_steps': li}
        res['sampling_latency'] = lat
    b.close(); i.close()
print(json.dumps(res, indent=1))
if out:
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
