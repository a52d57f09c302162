"""CFGRL agent groups against standalone CFGRL agents, in ONE process: obs 29, act 8, goal 29, hidden 512 x 4, fp32, at B 256 and at the
reference's default B 1024 (a seed x goal-mixture x guidance-weight sweep of the goal-conditioned tasks).  For each batch size and each
K: a group of K members and K standalone agents updated round-robin on their default path (stream left to the engine = its own queues),
timed in alternating fenced windows after a warm-up.  Reports total member-updates/s of both (median and min-max over the rounds) and
their ratio to ONE standalone agent (the K = 1 round-robin figure of that batch size).  Then one table of the fused sample_actions
against K member calls at n = 10 host rows per member (the reference's eval_batch_size) and flow_steps 16.
usage: python experiments/cfgrl_group_rate.py [Ks (comma list)] [rounds] [updates per window] [out.json] [batch sizes (comma list)]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
import fql_amd.cfgrl  # noqa: E402

Ks = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else '1,2,3,4,8').split(',')]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 300
out = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] not in ('', '-') else None
Bs = [int(b) for b in (sys.argv[5] if len(sys.argv) > 5 else '256,1024').split(',')]
OD, AD, H, N_ROWS, N_DS = 29, 8, 512, 10, 8192
CFGS = [1.0, 1.5, 3.0, 5.0, 1.0, 1.5, 3.0, 5.0]
MIXES = [(0.0, 1.0, 0.0), (0.0, 0.5, 0.5), (0.2, 0.5, 0.3), (0.0, 1.0, 0.0), (0.0, 0.5, 0.5), (0.2, 0.5, 0.3), (0.0, 1.0, 0.0), (0.0, 0.5, 0.5)]
rng = np.random.default_rng(3)
ds = {'observations': rng.standard_normal((N_DS, OD)).astype(np.float32),
      'actions': np.clip(rng.standard_normal((N_DS, AD)), -1, 1).astype(np.float32), 'terminals': np.zeros(N_DS, np.float32)}
ds['terminals'][199::200] = 1.0   # trajectories of 200 rows
ds['terminals'][-1] = 1.0
ex = {'observations': ds['observations'][:1], 'actions': ds['actions'][:1], 'value_goals': ds['observations'][:1]}


def window(update, sync, count):
    """`count` updates, fenced; seconds per update."""
    sync()
    t0 = time.perf_counter()
    for _ in range(count):
        update()
    sync()
    return (time.perf_counter() - t0) / count


def spread(ts, per=1.0):
    return [round(per / max(ts), 1), round(per / min(ts), 1)]


results, sampling = [], []
for B in Bs:
    cfg = fql_amd.cfgrl.get_config()
    cfg.update(actor_hidden_dims=(H,) * 4, batch_size=B, flow_steps=16)
    for K in Ks:
        group = fql_amd.CFGRLAgentGroup.create(list(range(1, K + 1)), ex, cfg, cfgs=CFGS[:K], goal_mixes=MIXES[:K])
        group.upload_dataset(ds)
        solo = []
        for i in range(K):
            a = fql_amd.CFGRLAgent.create(100 + i, ex, dict(cfg, cfg=CFGS[i], actor_p_curgoal=MIXES[i][0], actor_p_trajgoal=MIXES[i][1],
                                                            actor_p_randomgoal=MIXES[i][2]))
            a.upload_dataset(ds)
            solo.append(a)

        def solo_sync():
            for a in solo:
                a.synchronize()

        def group_update():
            group.update_from_dataset()

        def solo_update():
            for a in solo:
                a.update_from_dataset(B)

        launches = group.launches()
        window(group_update, group.synchronize, 30)      # warm-up: the program on both sides, the queues' first builds
        window(solo_update, solo_sync, 30)
        tg, ts = [], []
        for r in range(rounds):
            window(group_update, group.synchronize, 10)
            tg.append(window(group_update, group.synchronize, n))
            window(solo_update, solo_sync, 10)
            ts.append(window(solo_update, solo_sync, n))
        g_rate, s_rate = K / statistics.median(tg), K / statistics.median(ts)
        res = dict(B=B, K=K, group_member_updates_per_s=round(g_rate, 1), round_robin_member_updates_per_s=round(s_rate, 1),
                   group_min_max=spread(tg, K), round_robin_min_max=spread(ts, K),
                   group_us_per_fused_update=round(statistics.median(tg) * 1e6, 1), round_robin_us_per_round=round(statistics.median(ts) * 1e6, 1),
                   group_over_round_robin=round(g_rate / s_rate, 4), launches=launches[0], launches_per_member_update=solo[0].cfgrl_stats()[0])
        results.append(res)
        print(json.dumps(res), flush=True)

        if B == Bs[0]:
            # fused sample_actions against K member calls: n = 10 host rows per member, seeded draws, each member's configured cfg, host
            # results (every call synchronous); the sampler does not depend on the batch size
            obs = np.random.default_rng(K).standard_normal((K, N_ROWS, OD)).astype(np.float32)
            goals = np.random.default_rng(K + 100).standard_normal((K, N_ROWS, OD)).astype(np.float32)
            seeds = list(range(K))

            def fused():
                group.sample_actions(obs, goals, seed=seeds)

            def members():
                for i, a in enumerate(solo):
                    a.sample_actions(obs[i], goals[i], seed=seeds[i])

            for f in (fused, members):
                for _ in range(30):
                    f()
            tf, tm = [], []
            for r in range(rounds):
                for f, acc in ((fused, tf), (members, tm)):
                    t0 = time.perf_counter()
                    for _ in range(100):
                        f()
                    acc.append((time.perf_counter() - t0) / 100)
            srow = dict(K=K, rows_per_member=N_ROWS, flow_steps=16, fused_us_per_call=round(statistics.median(tf) * 1e6, 1),
                        fused_us_min_max=[round(min(tf) * 1e6, 1), round(max(tf) * 1e6, 1)],
                        member_calls_us_per_round=round(statistics.median(tm) * 1e6, 1),
                        member_calls_us_min_max=[round(min(tm) * 1e6, 1), round(max(tm) * 1e6, 1)],
                        member_calls_over_fused=round(statistics.median(tm) / statistics.median(tf), 3), launches_per_fused_call=launches[1],
                        launches_per_member_call=solo[0].cfgrl_stats()[2])
            sampling.append(srow)
            print(json.dumps(srow), flush=True)
        group.close()
        for m in group.members + solo:
            m.close()

for B in Bs:
    one = next((r['round_robin_member_updates_per_s'] for r in results if r['K'] == 1 and r['B'] == B), None)
    for r in (r for r in results if r['B'] == B):
        if one:
            r['group_over_one_standalone'] = round(r['group_member_updates_per_s'] / one, 3)
            r['round_robin_over_one_standalone'] = round(r['round_robin_member_updates_per_s'] / one, 3)
        print(f"B={B} K={r['K']}: group {r['group_member_updates_per_s']:.0f} member-updates/s {r['group_min_max']} "
              f"({r['group_us_per_fused_update']:.0f} us per fused update), round-robin {r['round_robin_member_updates_per_s']:.0f} "
              f"{r['round_robin_min_max']}; group / round-robin {r['group_over_round_robin']:.3f}"
              + (f"; group / one standalone agent {r['group_over_one_standalone']:.2f}" if 'group_over_one_standalone' in r else ''))
for s in sampling:
    print(f"K={s['K']}: fused sample_actions {s['fused_us_per_call']:.0f} us, {s['K']} member calls "
          f"{s['member_calls_us_per_round']:.0f} us ({s['member_calls_over_fused']:.2f}x), {s['launches_per_fused_call']} launches per fused call")
if out:
    with open(out, 'w') as f:
        json.dump(dict(config=f'obs {OD}, act {AD}, goal {OD}, hidden {H}x4, no LayerNorm, fp32, flow_steps 16; cfg 1 / 1.5 / 3 / 5 and goal mixtures '
                              '(0, 1, 0) / (0, .5, .5) / (.2, .5, .3) over the members',
                       rounds=rounds, updates_per_window=n, updates=results, sample_actions=sampling), f, indent=1)
