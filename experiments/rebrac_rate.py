"""ReBRAC against FQL in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) at B 256 and B 1024.  Every agent
updates from a device-resident synthetic dataset on its default path (stream left to the engine = its own queues), timed in alternating
fenced windows: FQL, ReBRAC on the actor_freq = 2 schedule (full and critic-only steps alternating, main.py:207-208), ReBRAC full steps
only and ReBRAC critic-only steps only.  Prints one JSON object (and writes it to out.json when given).
usage: python experiments/rebrac_rate.py [rounds] [updates per window] [out.json or -] [--rebrac-only]
(--rebrac-only: ReBRAC updates at B 256 on the actor_freq = 2 schedule alone, no FQL agent - the run to put under rocprofv3 --kernel-trace
--stats)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

rebrac_only = '--rebrac-only' in sys.argv
if rebrac_only:
    sys.argv.remove('--rebrac-only')
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


def rebrac_agent(B, batch, ds):
    cfg = fql_amd.rebrac.get_config()
    cfg.update(batch_size=B)
    r = fql_amd.ReBRACAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    r.upload_dataset(ds)
    return r


res = {'shapes': 'obs 29, act 8, hidden 512 x 4, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
if rebrac_only:
    _, ds, batch, _ = make_problem(29, 8, 256, (H,) * 4, seed=3)
    r = rebrac_agent(256, batch, ds)
    us = [window(lambda i: r.update_from_dataset(full_update=i % 2 == 0), r, n) for _ in range(rounds)]
    print(json.dumps({'B': 256, 'rebrac_schedule_us_per_update': statistics.median(us)}))
    sys.exit(0)
for B in (256, 1024):
    fcfg, ds, batch, _ = make_problem(29, 8, B, (H,) * 4, seed=3)
    f = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], fcfg)
    f.upload_dataset(ds)
    r = rebrac_agent(B, batch, ds)
    kinds = {
        'fql': (f, lambda i: f.update_from_dataset()),
        'rebrac_schedule': (r, lambda i: r.update_from_dataset(full_update=i % 2 == 0)),
        'rebrac_full': (r, lambda i: r.update_from_dataset(full_update=True)),
        'rebrac_critic_only': (r, lambda i: r.update_from_dataset(full_update=False)),
    }
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
    s = f.stats()
    row['stats'] = {'fql': {'launches_per_update': s['launches_per_update'], 'macs_per_sample': s['macs_per_update'] / B}}
    for full, name in ((True, 'rebrac_full'), (False, 'rebrac_critic_only')):
        la, ma = r.rebrac_stats(full)
        row['stats'][name] = {'launches_per_update': la, 'macs_per_sample': ma / B}
    res['batches'].append(row)
    f.close(); r.close()
print(json.dumps(res, indent=1))
if out:
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
