"""A guidance sweep in one call against one call per weight, in ONE process: BASELINE.json configs[1] shapes (obs 29, act 8, H 512 x 4,
S 16, fp32), host numpy in and out (what an evaluation rollout over a 10-environment vector env calls at every environment step).  For
IQL-diffusion and CFGRL (goal_dim = obs_dim) it times
  (a) sample_actions at n = 10 and cfg 3: one launch chain, the existing sampler (the parent commit's code, unchanged);
  (b) the same call four times, for the weights [1, 1.5, 3, 5] of main.py:298-330: what a sweep costs today;
  (c) ONE sample_actions_rows of 40 rows (the four weights, 10 rows each): the sweep program, S - 1 launches shorter;
  (d) sample_actions_rows of the 10 rows of (a), every weight 3: the shorter chain alone, at equal rows.
They alternate in windows of `per` calls, `rounds` times (200 calls each by default); reported are the median over all calls and,
as the margin, the max - min of the per-window medians of (a).  Prints one JSON object and writes it to profiles/sweep_latency.json (or
the path given).
usage: python experiments/sweep_latency.py [rounds] [calls per window] [out.json or -]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fql_amd  # noqa: E402
import fql_amd.cfgrl  # noqa: E402
import fql_amd.iql_diffusion  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
per = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'sweep_latency.json')
OD, AD, N_ENVS = 29, 8, 10
CFGS = np.array([1.0, 1.5, 3.0, 5.0], np.float32)


def timed(call, k):
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def measure(calls):
    """calls: {name: callable}; alternating windows -> {name: {median_us, p90_us, window_medians_us, window_spread_us}}"""
    for c in calls.values():
        timed(c, 20)
    ts = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            ts[k].append(timed(c, per))
    res = {}
    for k, w in ts.items():
        flat = [t for win in w for t in win]
        med = [statistics.median(win) for win in w]
        res[k] = {'median_us': statistics.median(flat), 'p90_us': float(np.percentile(flat, 90)), 'window_medians_us': med,
                  'window_spread_us': max(med) - min(med)}
    return res


rng = np.random.default_rng(0)
obs = rng.standard_normal((N_ENVS, OD)).astype(np.float32)
goals = rng.standard_normal((N_ENVS, OD)).astype(np.float32)
z = rng.standard_normal((N_ENVS, AD)).astype(np.float32)
G = len(CFGS)
obs_f, goals_f, z_f, w_f = np.tile(obs, (G, 1)), np.tile(goals, (G, 1)), np.tile(z, (G, 1)), np.repeat(CFGS, N_ENVS)
w_3 = np.full(N_ENVS, 3.0, np.float32)
res = {'shapes': 'obs 29, act 8 (CFGRL: goal 29), hidden 512 x 4, 16 Euler steps, fp32; host numpy in and out', 'n_envs': N_ENVS,
       'cfgs': CFGS.tolist(), 'rounds': rounds, 'calls_per_window': per}

d = fql_amd.IQLDiffusionAgent.create(0, obs[:1], z[:1], dict(fql_amd.iql_diffusion.get_config(), batch_size=256))
res['iql_diffusion'] = measure({
    'a_sample_actions_n10': lambda: d.sample_actions(obs, noises=z, cfg=3.0),
    'b_four_sample_actions_n10': lambda: [d.sample_actions(obs, noises=z, cfg=float(c)) for c in CFGS],
    'c_sample_actions_rows_n40': lambda: d.sample_actions_rows(obs_f, w_f, noises=z_f),
    'd_sample_actions_rows_n10': lambda: d.sample_actions_rows(obs, w_3, noises=z)})
res['iql_diffusion'].update(launches_a=d.iqld_stats()[2], launches_b=4 * d.iqld_stats()[2], launches_c=d.sample_cfgs_stats())
assert np.array_equal(d.sample_actions_rows(obs_f, w_f, noises=z_f).reshape(G, N_ENVS, AD),
                      np.stack([d.sample_actions(obs, noises=z, cfg=float(c)) for c in CFGS]))
d.close()

ex = {'observations': obs[:1], 'actions': z[:1], 'value_goals': goals[:1]}
g = fql_amd.CFGRLAgent.create(0, ex, dict(fql_amd.cfgrl.get_config(), batch_size=256))
res['cfgrl'] = measure({
    'a_sample_actions_n10': lambda: g.sample_actions(obs, goals, noises=z, cfg=3.0),
    'b_four_sample_actions_n10': lambda: [g.sample_actions(obs, goals, noises=z, cfg=float(c)) for c in CFGS],
    'c_sample_actions_rows_n40': lambda: g.sample_actions_rows(obs_f, goals_f, w_f, noises=z_f),
    'd_sample_actions_rows_n10': lambda: g.sample_actions_rows(obs, goals, w_3, noises=z)})
res['cfgrl'].update(launches_a=g.cfgrl_stats()[2], launches_b=4 * g.cfgrl_stats()[2], launches_c=g.sample_cfgs_stats())
assert np.array_equal(g.sample_actions_rows(obs_f, goals_f, w_f, noises=z_f).reshape(G, N_ENVS, AD),
                      np.stack([g.sample_actions(obs, goals, noises=z, cfg=float(c)) for c in CFGS]))
g.close()

print(json.dumps(res, indent=1))
if out not in ('', '-'):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
