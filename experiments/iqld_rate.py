"""IQL-diffusion against IQL `awr` in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) at B 256 and B 1024,
for each of the three step kinds (both nets, critic and value only, actor only).  IQL awr runs the same value / critic work with a
Gaussian actor, so its us per update is the yardstick and the spread of its own repeated 20-update windows the margin.  All agents update
from a device-resident synthetic dataset on their default path (stream left to the engine = its own queues), timed in alternating fenced
windows.  Also the host-observed latency of one sampling call at n = 1 and n = 256 rows for cfg = 1: IQL-diffusion's sample_actions (16
Euler steps over 2n rows) beside BC's (16 steps over n rows).  Prints one JSON object and writes it to profiles/iqld_rate.json (or the
path given).
usage: python experiments/iqld_rate.py [rounds] [updates per window] [out.json or -]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fql_amd  # noqa: E402
import fql_amd.bc  # noqa: E402
import fql_amd.iql  # noqa: E402
import fql_amd.iql_diffusion  # noqa: E402
from tests.util import make_problem  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'iqld_rate.json')
KINDS = {'both': (True, True), 'critic_only': (True, False), 'actor_only': (False, True)}


def window(agent, k, **kw):
    agent.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        agent.update_from_dataset(**kw)
    agent.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


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
for B in (256, 1024):
    _, ds, batch, _ = make_problem(29, 8, B, (512,) * 4, seed=3)
    ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
    d = fql_amd.IQLDiffusionAgent.create(0, ex_o, ex_a, dict(fql_amd.iql_diffusion.get_config(), batch_size=B))
    q = fql_amd.IQLAgent.create(0, ex_o, ex_a, dict(fql_amd.iql.get_config(), batch_size=B, actor_loss='awr'))
    for a in (d, q):
        a.upload_dataset(ds)
        window(a, 60)
    for uc, ua in KINDS.values():
        window(d, 20, update_critic=uc, update_actor=ua)
    t = {k: [] for k in KINDS}
    tq = []
    for _ in range(rounds):
        for k, (uc, ua) in KINDS.items():
            t[k].append(window(d, n, update_critic=uc, update_actor=ua))
        tq.append(window(q, n))
    row = {'B': B, 'iql_awr_us_per_update': statistics.median(tq), 'iql_awr_window_spread_us': max(tq) - min(tq), 'iql_awr_windows_us': tq,
           'iql_awr_launches_per_update': q.iql_stats()[0]}
    for k, (uc, ua) in KINDS.items():
        la, ma, ls = d.iqld_stats(uc, ua)
        row[k] = {'us_per_update': statistics.median(t[k]), 'window_spread_us': max(t[k]) - min(t[k]), 'windows_us': t[k],
                  'launches_per_update': la, 'macs_per_sample': ma / B}
    row['launches_per_sampling_call'] = d.iqld_stats()[2]
    res['batches'].append(row)
    if B == 256:   # host numpy in and out (what an evaluation rollout calls)
        b = fql_amd.BCAgent.create(0, ex_o, ex_a, dict(fql_amd.bc.get_config(), batch_size=B))
        lat = {}
        for rows in (1, 256):
            ob = batch['observations'][:rows]
            z = np.random.default_rng(0).standard_normal((rows, 8)).astype(np.float32)
            o1, z1 = (ob, z) if rows > 1 else (ob[0], z[0])
            ld = latency(lambda k: d.sample_actions(o1, noises=z1, cfg=1.0))
            lb = latency(lambda k: b.sample_actions(o1, noises=z1))
            ld['per_euler_step_us'] = ld['median_us'] / 16
            lb['per_euler_step_us'] = lb['median_us'] / 16
            lat[f'n={rows}'] = {'iqld_sample_actions_cfg1_16_steps': ld, 'bc_sample_actions_16_steps': lb}
        res['sampling_latency'] = lat
        res['bc_launches_per_sampling_call'] = b.bc_stats()[2]
        b.close()
    d.close(); q.close()
print(json.dumps(res, indent=1))
if out not in ('', '-'):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
