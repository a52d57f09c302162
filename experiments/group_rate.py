"""Agent groups against standalone agents, in ONE process: BASELINE.json configs[1] (obs 29, act 8, B 256, H 512 x 4, fp32), alphas of
the reference's sweep.  For each K: a group of K members and K standalone agents updated round-robin on their default path (stream left to
the engine = its own queues), timed in alternating fenced windows.  Reports total member-updates/s of both and their ratio to ONE
standalone agent (the K = 1 round-robin figure).
usage: python experiments/group_rate.py [Ks (comma list)] [rounds] [updates per window] [out.json] [--group-only]
(--group-only: no standalone agents - the run to put under rocprofv3 --kernel-trace --stats, one K per run)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from tests.util import make_problem  # noqa: E402

group_only = '--group-only' in sys.argv
if group_only:
    sys.argv.remove('--group-only')
Ks = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else '1,2,4,8').split(',')]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 300
out = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] not in ('', '-') else None
B, H = 256, 512
ALPHAS = [0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]
cfg, ds, batch, noise = make_problem(29, 8, B, (H,) * 4, seed=3)
ex_o, ex_a = batch['observations'][:1], batch['actions'][:1]

results = []
for K in Ks:
    group = fql_amd.FQLAgentGroup.create(list(range(K)), ex_o, ex_a, cfg, alphas=ALPHAS[:K])
    group.upload_dataset(ds)
    solo = []
    for i in range(0 if group_only else K):
        a = fql_amd.FQLAgent.create(100 + i, ex_o, ex_a, dict(cfg, alpha=ALPHAS[i]))
        a.upload_dataset(ds)
        solo.append(a)
    for _ in range(30):
        group.update_from_dataset()
        for a in solo:
            a.update_from_dataset(B)
    group.synchronize()
    for a in solo:
        a.synchronize()
    tg, ts = [], []
    for r in range(rounds):
        for _ in range(10):
            group.update_from_dataset()
        group.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            group.update_from_dataset()
        group.synchronize()
        tg.append((time.perf_counter() - t0) / n)
        for _ in range(10):
            for a in solo:
                a.update_from_dataset(B)
        for a in solo:
            a.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            for a in solo:
                a.update_from_dataset(B)
        for a in solo:
            a.synchronize()
        ts.append((time.perf_counter() - t0) / n)
    if group_only:
        print(json.dumps(dict(K=K, group_member_updates_per_s=round(K / statistics.median(tg), 1))), flush=True)
        group.close()
        continue
    g_rate, s_rate = K / statistics.median(tg), K / statistics.median(ts)
    res = dict(K=K, group_member_updates_per_s=round(g_rate, 1), round_robin_member_updates_per_s=round(s_rate, 1),
               group_us_per_fused_update=round(statistics.median(tg) * 1e6, 1), round_robin_us_per_round=round(statistics.median(ts) * 1e6, 1),
               group_over_round_robin=round(g_rate / s_rate, 4), group_spread_us=[round(min(tg) * 1e6, 1), round(max(tg) * 1e6, 1)],
               launches_per_fused_update=group.members[0].stats()['launches_per_update'])
    results.append(res)
    print(json.dumps(res), flush=True)
    group.close()
    for m in group.members + solo:
        m.close()
one = next((r['round_robin_member_updates_per_s'] for r in results if r['K'] == 1), None)
for r in results:
    if one:
        r['group_over_one_standalone'] = round(r['group_member_updates_per_s'] / one, 3)
        r['round_robin_over_one_standalone'] = round(r['round_robin_member_updates_per_s'] / one, 3)
    print(f"K={r['K']}: group {r['group_member_updates_per_s']:.0f} member-updates/s ({r['group_us_per_fused_update']:.0f} us per fused update), "
          f"round-robin {r['round_robin_member_updates_per_s']:.0f}; group / round-robin {r['group_over_round_robin']:.3f}"
          + (f"; group / one standalone agent {r['group_over_one_standalone']:.2f}" if one else ''))
if out:
    with open(out, 'w') as f:
        json.dump(dict(config='configs[1]: obs 29, act 8, B 256, H 512x4, fp32, flow_steps 10', rounds=rounds, updates_per_window=n,
                       results=results), f, indent=1)
