"""IQL (both actor losses, both const_std values) against IFQL, whose value / critic work it shares, in ONE process: BASELINE.json
configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) at B 256 and B 1024.  Every agent updates from a device-resident synthetic dataset
on its default path (stream left to the engine = its own queues), timed in alternating fenced windows.  At B 256 also the latency of
single-observation sample_actions with host arrays (main.py:226).  With FQL_DUMP=1 in the environment the engine prints each program's
launches, lanes and cross-lane waits (the critical lane of DESIGN.md section 17).  Prints one JSON object (and writes it to out.json
when given).
usage: python experiments/iql_rate.py [rounds] [updates per window] [out.json or -]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 300
out = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] not in ('', '-') else None
H = 512


def window(step, agent, k):
    agent.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(i)
    agent.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def iql_agent(B, batch, ds, actor_loss, const_std):
    cfg = fql_amd.iql.get_config()
    cfg.update(batch_size=B, actor_loss=actor_loss, const_std=const_std)
    a = fql_amd.IQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    a.upload_dataset(ds)
    return a


res = {'shapes': 'obs 29, act 8, hidden 512 x 4, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
for B in (256, 1024):
    _, ds, batch, _ = make_problem(29, 8, B, (H,) * 4, seed=3)
    icfg = fql_amd.ifql.get_config()
    icfg.update(batch_size=B)
    agents = {'ifql': fql_amd.IFQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], icfg)}
    agents['ifql'].upload_dataset(ds)
    for al in ('awr', 'ddpgbc'):
        for cs in (True, False):
            agents[f'iql_{al}_{"const_std" if cs else "log_stds"}'] = iql_agent(B, batch, ds, al, cs)
    for a in agents.values():
        window(lambda i: a.update_from_dataset(), a, 30)
    t = {k: [] for k in agents}
    for _ in range(rounds):
        for k, a in agents.items():
            t[k].append(window(lambda i: a.update_from_dataset(), a, n))
    row = {'B': B, 'stats': {}}
    for k, a in agents.items():
        row[f'{k}_us_per_update'] = statistics.median(t[k])
        row[f'{k}_windows_us'] = t[k]
        st = a.stats()
        row['stats'][k] = {'launches_per_update': st['launches_per_update'], 'macs_per_sample': st['macs_per_update'] / B}
    for k in agents:
        if k != 'ifql':
            row[f'{k}_over_ifql'] = row[f'{k}_us_per_update'] / row['ifql_us_per_update']
    if B == 256:   # single-observation sample_actions with host arrays (the evaluation loop's call)
        s = agents['iql_ddpgbc_log_stds']
        ob = ds['observations'][0]
        for _ in range(50):
            s.sample_actions(ob, seed=1)
        lat = []
        for i in range(500):
            t0 = time.perf_counter()
            s.sample_actions(ob, seed=i)
            lat.append((time.perf_counter() - t0) * 1e6)
        row['iql_sample_actions_single_obs_us'] = {'median': statistics.median(lat), 'p90': float(np.percentile(lat, 90))}
    res['batches'].append(row)
    for a in agents.values():
        a.close()
print(json.dumps(res, indent=1))
if out:
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
