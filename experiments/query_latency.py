"""Host-observed latency of one network.select('critic') query on configs[1]'s nets (obs 29, act 8, hidden 512 x 4) at n = 1, 256, 4096:
host numpy in and out (synchronous), and CUDA tensors in and out with a device synchronise behind the call.  30 warm-up calls per
shape, then three windows of 300 (150 at n = 4096) calls; medians per window and over all calls.  argv[1]: the JSON to write
(default profiles/query_latency.json).  DESIGN.md section 21."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fql_amd

cfg = fql_amd.get_config()
cfg.update(batch_size=256, alpha=10.0)
od, ad = 29, 8
agent = fql_amd.FQLAgent.create(0, np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32), cfg)
critic = agent.network.select('critic')
rng = np.random.default_rng(0)
res = {}
for n in (1, 256, 4096):
    obs = rng.standard_normal((n, od)).astype(np.float32)
    act = rng.uniform(-1, 1, (n, ad)).astype(np.float32)
    dobs, dact = torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()
    torch.cuda.synchronize()
    for kind, call in (('host', lambda: critic(obs, actions=act)), ('device', lambda: critic(dobs, actions=dact))):
        for _ in range(30):
            call()
        torch.cuda.synchronize()
        reps = 300 if n < 4096 else 150
        ts = []
        for rnd in range(3):            # three windows: the spread between them is reported
            w = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = call()
                if kind == 'device':
                    torch.cuda.synchronize()   # the call returns once enqueued on torch's stream
                w.append(time.perf_counter() - t0)
            ts.append(w)
        med = [float(np.median(w)) * 1e6 for w in ts]
        res[f'{kind}_n{n}'] = dict(median_us_per_window=med, median_us=float(np.median(np.concatenate(ts))) * 1e6,
                                   p10_us=float(np.percentile(np.concatenate(ts), 10)) * 1e6, p90_us=float(np.percentile(np.concatenate(ts), 90)) * 1e6,
                                   rows_per_s=n / float(np.median(np.concatenate(ts))))
        print(kind, n, res[f'{kind}_n{n}'], flush=True)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, 'profiles', 'query_latency.json'), 'w'), indent=1)
