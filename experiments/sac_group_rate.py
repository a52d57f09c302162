"""SAC agent groups against standalone SAC agents, in ONE process: obs 29, act 8, B 256, hidden 512 x 4, fp32 (RLPD's learner, several
seeds of one task).  For each K: a group of K members and K standalone agents updated round-robin on their default path (stream left to
the engine = its own queues), timed in alternating fenced windows after a warm-up.  Measured on both sides:
  update_from_dataset;
  update_balanced with every agent's own replay ring of 10^4 rows;
  sample_actions, fused against K member calls, at n = 1 (the online loop's call, main.py:226) and n = 10 host rows per member;
  one whole online step: sample_actions on one observation per member, K ring inserts, one balanced update (K solo loops do each of
  the three per agent).
Reports total member-updates/s (median and min-max over the rounds) and their ratio to ONE standalone agent (the K = 1 round-robin
figure), and microseconds per call / per online step.
usage: python experiments/sac_group_rate.py [Ks (comma list)] [rounds] [updates per window] [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fql_amd  # noqa: E402
from oracle import fql_oracle as O  # noqa: E402

Ks = [int(k) for k in (sys.argv[1] if len(sys.argv) > 1 else '1,2,3,4,8').split(',')]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 300
out = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] not in ('', '-') else None
OD, AD, B, H, RING = 29, 8, 256, 512, 10000
ROW_COUNTS = (1, 10)
ds = O.make_synthetic_dataset(4 * B, OD, AD, seed=3)
ex_o, ex_a = ds['observations'][:1], ds['actions'][:1]
KEYS = ('observations', 'actions', 'rewards', 'masks', 'next_observations')


def window(update, sync, count):
    """`count` calls of `update`, fenced; seconds per call."""
    sync()
    t0 = time.perf_counter()
    for _ in range(count):
        update()
    sync()
    return (time.perf_counter() - t0) / count


def spread(ts, per=1.0):
    return [round(per / max(ts), 1), round(per / min(ts), 1)]


def us(ts):
    return round(statistics.median(ts) * 1e6, 1), [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]


def alternate(group_fn, group_sync, solo_fn, solo_sync, count):
    """`rounds` alternating fenced windows of `count` calls each side, after a warm-up: (group seconds per call, solo seconds per call)."""
    window(group_fn, group_sync, 30)
    window(solo_fn, solo_sync, 30)
    tg, ts = [], []
    for _ in range(rounds):
        window(group_fn, group_sync, 10)
        tg.append(window(group_fn, group_sync, count))
        window(solo_fn, solo_sync, 10)
        ts.append(window(solo_fn, solo_sync, count))
    return tg, ts


cfg = fql_amd.sac.get_config()
cfg.update(actor_hidden_dims=(H,) * 4, value_hidden_dims=(H,) * 4, batch_size=B)
updates, sampling, online = [], [], []
for K in Ks:
    group = fql_amd.SACAgentGroup.create(list(range(1, K + 1)), ex_o, ex_a, cfg)
    group.upload_dataset(ds)
    group.create_replay_buffers(RING)
    solo = []
    for i in range(K):
        a = fql_amd.SACAgent.create(100 + i, ex_o, ex_a, cfg)
        a.upload_dataset(ds)
        a.create_replay_buffer(RING)
        solo.append(a)
    rng = np.random.default_rng(K)
    for j in rng.integers(0, len(ds['observations']), size=RING if rounds > 1 else 64):
        t = {k: ds[k][int(j)] for k in KEYS}
        for a in group.members + solo:
            a.add_transition(t, replay=True)

    def solo_sync():
        for a in solo:
            a.synchronize()

    launches = group.launches()
    for mode, g_fn, s_fn in (('update_from_dataset', group.update_from_dataset, lambda: [a.update_from_dataset(B) for a in solo]),
                             ('update_balanced', group.update_balanced, lambda: [a.update_balanced(B) for a in solo])):
        tg, ts = alternate(g_fn, group.synchronize, s_fn, solo_sync, n)
        g_rate, s_rate = K / statistics.median(tg), K / statistics.median(ts)
        res = dict(mode=mode, K=K, group_member_updates_per_s=round(g_rate, 1), round_robin_member_updates_per_s=round(s_rate, 1),
                   group_min_max=spread(tg, K), round_robin_min_max=spread(ts, K),
                   group_us_per_fused_update=round(statistics.median(tg) * 1e6, 1), round_robin_us_per_round=round(statistics.median(ts) * 1e6, 1),
                   group_over_round_robin=round(g_rate / s_rate, 4), launches=launches[0], launches_per_member_update=solo[0].sac_stats()[0])
        updates.append(res)
        print(json.dumps(res), flush=True)

    # fused sample_actions against K member calls: host rows, seeded draws, host results (every call synchronous)
    seeds = list(range(K))
    for rows in ROW_COUNTS:
        obs = np.random.default_rng(K + rows).standard_normal((K, rows, OD)).astype(np.float32)
        tf, tm = alternate(lambda: group.sample_actions(obs, seed=seeds), lambda: None,
                           lambda: [a.sample_actions(obs[i], seed=seeds[i]) for i, a in enumerate(solo)], lambda: None, 100)
        (f_us, f_mm), (m_us, m_mm) = us(tf), us(tm)
        srow = dict(K=K, rows_per_member=rows, fused_us_per_call=f_us, fused_us_min_max=f_mm, member_calls_us_per_round=m_us,
                    member_calls_us_min_max=m_mm, member_calls_over_fused=round(m_us / f_us, 3), launches_per_fused_call=launches[1])
        sampling.append(srow)
        print(json.dumps(srow), flush=True)

    # one whole online step (main.py:217-259 with balanced sampling): act on one observation per member, insert, update
    ob = np.random.default_rng(50 + K).standard_normal((K, OD)).astype(np.float32)
    tr = [{k: ds[k][i] for k in KEYS} for i in range(K)]

    def group_step():
        acts = group.sample_actions(ob)
        for i in range(K):
            tr[i]['actions'] = acts[i]
        group.add_transitions(tr)
        group.update_balanced()

    def solo_step():
        for i, a in enumerate(solo):
            tr[i]['actions'] = a.sample_actions(ob[i])
            a.add_transition(tr[i], replay=True)
            a.update_balanced(B)

    tg, ts = alternate(group_step, group.synchronize, solo_step, solo_sync, n)
    (g_us, g_mm), (s_us, s_mm) = us(tg), us(ts)
    orow = dict(K=K, group_us_per_online_step=g_us, group_us_min_max=g_mm, solo_loops_us_per_online_step=s_us, solo_loops_us_min_max=s_mm,
                group_member_steps_per_s=round(K / statistics.median(tg), 1), solo_member_steps_per_s=round(K / statistics.median(ts), 1),
                solo_over_group=round(s_us / g_us, 3))
    online.append(orow)
    print(json.dumps(orow), flush=True)
    group.close()
    for m in group.members + solo:
        m.close()

for mode in ('update_from_dataset', 'update_balanced'):
    one = next((r['round_robin_member_updates_per_s'] for r in updates if r['K'] == 1 and r['mode'] == mode), None)
    for r in (r for r in updates if r['mode'] == mode):
        if one:
            r['group_over_one_standalone'] = round(r['group_member_updates_per_s'] / one, 3)
            r['round_robin_over_one_standalone'] = round(r['round_robin_member_updates_per_s'] / one, 3)
        print(f"{mode} K={r['K']}: group {r['group_member_updates_per_s']:.0f} member-updates/s {r['group_min_max']} "
              f"({r['group_us_per_fused_update']:.0f} us per fused update), round-robin {r['round_robin_member_updates_per_s']:.0f} "
              f"{r['round_robin_min_max']}; group / round-robin {r['group_over_round_robin']:.3f}"
              + (f"; group / one standalone agent {r['group_over_one_standalone']:.2f}" if 'group_over_one_standalone' in r else ''))
for s in sampling:
    print(f"K={s['K']} n={s['rows_per_member']}: fused sample_actions {s['fused_us_per_call']:.0f} us, {s['K']} member calls "
          f"{s['member_calls_us_per_round']:.0f} us ({s['member_calls_over_fused']:.2f}x), {s['launches_per_fused_call']} launches per fused call")
for o in online:
    print(f"K={o['K']}: online step, group {o['group_us_per_online_step']:.0f} us, {o['K']} solo loops {o['solo_loops_us_per_online_step']:.0f} us "
          f"({o['solo_over_group']:.2f}x)")
if out:
    with open(out, 'w') as f:
        json.dump(dict(config=f'obs {OD}, act {AD}, B {B}, hidden {H}x4, fp32, replay rings of {RING} rows, one target entropy', rounds=rounds,
                       updates_per_window=n, updates=updates, sample_actions=sampling, online_step=online), f, indent=1)
