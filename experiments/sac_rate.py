"""SAC against FQL (and a ReBRAC full step, the nearest earlier program) in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8,
H 512 x 4, fp32) at B 256 and B 1024.  Every agent updates from a device-resident synthetic dataset on its default path (stream left to
the engine = its own queues), timed in alternating fenced windows.  At B 256 also RLPD's balanced step (half the rows from a replay ring
of 10^4 transitions, main.py:255-259) and the latency of single-observation sample_actions with host arrays (main.py:226).  Prints one
JSON object (and writes it to out.json when given).
usage: python experiments/sac_rate.py [rounds] [updates per window] [out.json or -] [--sac-only]
(--sac-only: SAC updates at B 256 alone, no other agent - the run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

sac_only = '--sac-only' in sys.argv
if sac_only:
    sys.argv.remove('--sac-only')
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


def sac_agent(B, batch, ds):
    cfg = fql_amd.sac.get_config()
    cfg.update(batch_size=B)
    s = fql_amd.SACAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    s.upload_dataset(ds)
    return s


res = {'shapes': 'obs 29, act 8, hidden 512 x 4, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
if sac_only:
    _, ds, batch, _ = make_problem(29, 8, 256, (H,) * 4, seed=3)
    s = sac_agent(256, batch, ds)
    us = [window(lambda i: s.update_from_dataset(), s, n) for _ in range(rounds)]
    print(json.dumps({'B': 256, 'sac_us_per_update': statistics.median(us)}))
    sys.exit(0)
for B in (256, 1024):
    fcfg, ds, batch, _ = make_problem(29, 8, B, (H,) * 4, seed=3)
    f = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], fcfg)
    f.upload_dataset(ds)
    rcfg = fql_amd.rebrac.get_config()
    rcfg.update(batch_size=B)
    r = fql_amd.ReBRACAgent.create(0, batch['observations'][:1], batch['actions'][:1], rcfg)
    r.upload_dataset(ds)
    s = sac_agent(B, batch, ds)
    kinds = {
        'fql': (f, lambda i: f.update_from_dataset()),
        'rebrac_full': (r, lambda i: r.update_from_dataset(full_update=True)),
        'sac': (s, lambda i: s.update_from_dataset()),
    }
    if B == 256:   # RLPD: a replay ring beside the dataset, half of every batch from it
        sb = sac_agent(B, batch, ds)
        sb.create_replay_buffer(10000)
        rng = np.random.default_rng(0)
        for i in range(10000 if rounds > 1 else 64):
            j = int(rng.integers(0, len(ds['observations'])))
            sb.add_transition({k: ds[k][j] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')}, replay=True)
        kinds['sac_balanced'] = (sb, lambda i: sb.update_balanced(B))
    for a, step in kinds.values():
        window(step, a, 30)
    t = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, (a, step) in kinds.items():
            t[k].append(window(step, a, n))
    row = {'B': B}
    for k in kinds:
        row[f'{k}_us_per_update'] = statistics.median(t[k])
        row[f'{k}_updates_per_s'] = 1e6 / statistics.median(t[k])
        row[f'{k}_windows_us'] = t[k]
    row['sac_over_rebrac_full'] = row['sac_us_per_update'] / row['rebrac_full_us_per_update']
    fs = f.stats()
    la, ma = s.sac_stats()
    lr, mr = r.rebrac_stats(True)
    row['stats'] = {'fql': {'launches_per_update': fs['launches_per_update'], 'macs_per_sample': fs['macs_per_update'] / B},
                    'rebrac_full': {'launches_per_update': lr, 'macs_per_sample': mr / B},
                    'sac': {'launches_per_update': la, 'macs_per_sample': ma / B}}
    if B == 256:   # single-observation sample_actions with host arrays (the online loop's call, main.py:226)
        ob = ds['observations'][0]
        for _ in range(50):
            s.sample_actions(ob, seed=1)
        lat = []
        for i in range(500):
            t0 = time.perf_counter()
            s.sample_actions(ob, seed=i)
            lat.append((time.perf_counter() - t0) * 1e6)
        row['sac_sample_actions_single_obs_us'] = {'median': statistics.median(lat), 'p90': float(np.percentile(lat, 90))}
        sb.close()
    res['batches'].append(row)
    f.close(); r.close(); s.close()
print(json.dumps(res, indent=1))
if out:
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
