"""Evaluating a sweep: ONE FQLAgentGroup.sample_actions call against K member.sample_actions calls, in one process.  BASELINE.json
configs[1]'s shape (obs 29, act 8, H 512 x 4, fp32), host numpy in and out as the reference's evaluation loop passes them
(utils/evaluation.py), so every call ends in a host synchronise and a host clock around a window of calls measures them.  For each K and
each n rows per member: alternating windows of group calls and of K member calls (the group's own members), after a warm-up of both.
Reports the median and the spread (min, max over the rounds) of the time per environment step, i.e. per group call / per K member calls.
usage: python experiments/group_sample_latency.py [Ks (comma list)] [ns (comma list)] [rounds] [calls per window] [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

Ks = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else '2,4,8').split(',')]
ns = [int(k) for k in (sys.argv[2] if len(sys.argv) > 2 else '1,10,256').split(',')]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
calls = int(sys.argv[4]) if len(sys.argv) > 4 else 200
out = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] not in ('', '-') else None
OD, AD, H = 29, 8, 512
ALPHAS = [0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]
cfg, ds, batch, noise = make_problem(OD, AD, 256, (H,) * 4, seed=3)
ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]
rng = np.random.default_rng(0)


def us(ts):
    return dict(median=round(statistics.median(ts) * 1e6, 1), min=round(min(ts) * 1e6, 1), max=round(max(ts) * 1e6, 1))


results = []
for K in Ks:
    group = fql_amd.FQLAgentGroup.create(list(range(K)), ex_o, ex_a, cfg, alphas=ALPHAS[:K])
    launches = group.sample_launches()
    for n in ns:
        obs = rng.standard_normal((K, n, OD)).astype(np.float32)
        rows = [np.ascontiguousarray(obs[i]) for i in range(K)]

        def fused():
            group.sample_actions(obs)

        def members():
            for m, o in zip(group.members, rows):
                m.sample_actions(o)

        for f in (fused, members):   # builds the workspaces of this n, then warms both paths
            for _ in range(50):
                f()
        tg, tm = [], []
        for r in range(rounds):
            for f, ts in ((fused, tg), (members, tm)):
                for _ in range(10):
                    f()
                t0 = time.perf_counter()
                for _ in range(calls):
                    f()
                ts.append((time.perf_counter() - t0) / calls)
        res = dict(K=K, n=n, group_us=us(tg), members_us=us(tm), members_over_group=round(statistics.median(tm) / statistics.median(tg), 3),
                   launches_per_group_call=launches, launches_per_member_round=K * launches)
        results.append(res)
        print(json.dumps(res), flush=True)
    group.close()
    for m in group.members:
        m.close()
for r in results:
    print(f"K={r['K']} n={r['n']}: group call {r['group_us']['median']:.0f} us ({r['group_us']['min']:.0f}-{r['group_us']['max']:.0f}), "
          f"{r['K']} member calls {r['members_us']['median']:.0f} us ({r['members_us']['min']:.0f}-{r['members_us']['max']:.0f}); "
          f"members / group {r['members_over_group']:.2f}")
if out:
    with open(out, 'w') as f:
        json.dump(dict(config='configs[1] shape: obs 29, act 8, H 512x4, fp32; host numpy in and out; time per environment step',
                       rounds=rounds, calls_per_window=calls, results=results), f, indent=1)
