"""CFGRL against BC in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4, fp32) with goal_dim = obs_dim, at B 256 and
B 1024.  BC runs the same single-lane flow-matching update on narrower rows, so its us per update is the yardstick and the spread of its
own repeated 20-update windows the margin: CFGRL should cost BC's update plus one prep of wider rows (with the goal draw) and one small
launch (the embedding gradient).  Both agents update from a device-resident synthetic dataset on their default path (stream left to the
engine = its own queues), timed in alternating fenced windows.  Both actors run without LayerNorm (CFGRL's default).  Also the
host-observed latency of one sampling call at n = 1 and n = 256 rows: CFGRL's sample_actions (flow_steps 16 over 2n rows, cfg 3) beside
IQL-diffusion's CFG sampler (16 steps over 2n rows).  Prints one JSON object and writes it to profiles/cfgrl_rate.json (or the path
given).
usage: python experiments/cfgrl_rate.py [rounds] [updates per window] [out.json or -]"""
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
import fql_amd.cfgrl  # noqa: E402
import fql_amd.iql_diffusion  # noqa: E402
from tests.util import make_problem  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'cfgrl_rate.json')
OD, AD = 29, 8


def window(agent, k):
    agent.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        agent.update_from_dataset()
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


res = {'shapes': 'obs 29, goal 29, act 8, hidden 512 x 4, no LayerNorm, fp32', 'rounds': rounds, 'updates_per_window': n, 'batches': []}
for B in (256, 1024):
    _, ds, batch, _ = make_problem(OD, AD, B, (512,) * 4, seed=3)
    ds = dict(ds)
    N = len(ds['observations'])
    ds['terminals'] = np.zeros(N, np.float32)
    ds['terminals'][199::200] = 1.0   # trajectories of 200 rows
    ds['terminals'][-1] = 1.0
    ex = {'observations': batch['observations'][:1], 'actions': batch['actions'][:1], 'value_goals': batch['observations'][:1]}
    g = fql_amd.CFGRLAgent.create(0, ex, dict(fql_amd.cfgrl.get_config(), batch_size=B))
    b = fql_amd.BCAgent.create(0, ex['observations'], ex['actions'], dict(fql_amd.bc.get_config(), batch_size=B, use_layer_norm=0))
    for a in (g, b):
        a.upload_dataset(ds)
        window(a, 60)
    tg, tb = [], []
    for _ in range(rounds):
        tg.append(window(g, n))
        tb.append(window(b, n))
    lg, mg, ls = g.cfgrl_stats()
    lb, mb, _ = b.bc_stats()
    res['batches'].append({'B': B,
                           'bc_us_per_update': statistics.median(tb), 'bc_window_spread_us': max(tb) - min(tb), 'bc_windows_us': tb,
                           'bc_launches_per_update': lb, 'bc_macs_per_sample': mb / B,
                           'cfgrl_us_per_update': statistics.median(tg), 'cfgrl_window_spread_us': max(tg) - min(tg), 'cfgrl_windows_us': tg,
                           'cfgrl_launches_per_update': lg, 'cfgrl_macs_per_sample': mg / B, 'cfgrl_launches_per_sampling_call': ls})
    if B == 256:   # host numpy in and out (what an evaluation rollout calls)
        d = fql_amd.IQLDiffusionAgent.create(0, ex['observations'], ex['actions'], dict(fql_amd.iql_diffusion.get_config(), batch_size=B))
        lat = {}
        for rows in (1, 256):
            ob = batch['observations'][:rows]
            gl = batch['observations'][::-1][:rows].copy()
            z = np.random.default_rng(0).standard_normal((rows, AD)).astype(np.float32)
            o1, g1, z1 = (ob, gl, z) if rows > 1 else (ob[0], gl[0], z[0])
            lc = latency(lambda k: g.sample_actions(o1, g1, noises=z1))
            ld = latency(lambda k: d.sample_actions(o1, noises=z1, cfg=3.0))
            lc['per_euler_step_us'] = lc['median_us'] / 16
            ld['per_euler_step_us'] = ld['median_us'] / 16
            lat[f'n={rows}'] = {'cfgrl_sample_actions_cfg3_16_steps': lc, 'iqld_sample_actions_cfg3_16_steps': ld}
        res['sampling_latency'] = lat
        res['iqld_launches_per_sampling_call'] = d.iqld_stats()[2]
        d.close()
    g.close(); b.close()
print(json.dumps(res, indent=1))
if out not in ('', '-'):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
