"""Shared helpers for the parity tests (HIP engine vs CPU oracle on identical inputs)."""
import numpy as np

from oracle import fql_oracle as O


def make_cfg(hidden=(64, 64, 64, 64), **kw):
    import fql_amd
    cfg = fql_amd.get_config()
    cfg.update(actor_hidden_dims=tuple(hidden), value_hidden_dims=tuple(hidden), alpha=10.0)
    cfg.update(kw)
    return cfg


def randomize_params(params, seed, scale=0.1):
    """Biases / LN params away from their 0/1 init so every leaf matters; target != critic."""
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, dtype=np.float64), params)
    for path, leaf in O.tree_leaves_with_path(out):
        if path.endswith('/bias') or path.endswith('/scale'):
            leaf += scale * rng.standard_normal(leaf.shape)
    out['modules_target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), out['modules_critic'])
    return O.tree_map(lambda a: a.astype(np.float32), out)


def make_problem(od, ad, B, hidden, seed=0, **cfgkw):
    cfg = make_cfg(hidden, batch_size=B, **cfgkw)
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    batch = O.sample_batch(ds, idx)
    noise = O.make_noise(B, ad, seed + 2)
    return cfg, ds, batch, noise


def leaf_dict(tree):
    return dict(O.tree_leaves_with_path(tree))


def assert_same_state(a, b):
    """Two agents bitwise in the same state: every parameter leaf, the optimizer counters and both Adam moments."""
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert oa['count'] == ob['count'] and oa['step'] == ob['step']
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{part} {k}')


def assert_initialised_like_the_reference(p0, p1, opt, n_kernel):
    """get_params of two FQL agents created from seeds 0 and 1, and the first one's optimizer state: Glorot-uniform kernels from the real
    fan-in and fan-out (the bound attained, the variance of U(-lim, lim)), ensemble members drawn independently, Dense biases 0,
    LayerNorm (1, 0), target_critic := critic, different seeds different kernels, zero moments and the counters of a fresh TrainState."""
    n = 0
    for path, w in O.tree_leaves_with_path(p0):
        if path.endswith('/kernel'):
            fan_in, fan_out = w.shape[-2], w.shape[-1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            assert np.abs(w).max() <= lim * (1 + 1e-6), path
            if w.size >= 4096:
                assert np.abs(w).max() >= 0.98 * lim, path                       # the bound is attained, not a smaller box
                assert abs(w.var() / (lim * lim / 3.0) - 1.0) < 0.05, (path, w.var())  # U(-lim, lim): variance lim^2 / 3
                assert abs(w.mean()) < 4 * lim / np.sqrt(3 * w.size), path
            if w.ndim == 3:   # ensemble members are drawn independently
                assert np.abs(w[0] - w[1]).max() > 0.1 * lim, path
            n += 1
        elif 'LayerNorm' in path and path.endswith('/scale'):
            np.testing.assert_array_equal(w, 1.0, err_msg=path)
        else:   # Dense bias, LayerNorm bias
            np.testing.assert_array_equal(w, 0.0, err_msg=path)
    assert n == n_kernel
    for (path, a), (_, b) in zip(O.tree_leaves_with_path(p0['modules_critic']), O.tree_leaves_with_path(p0['modules_target_critic'])):
        np.testing.assert_array_equal(a, b, err_msg=path)
    k = 'modules_actor_bc_flow'
    assert np.abs(leaf_dict(p0[k])['mlp/Dense_1/kernel'] - leaf_dict(p1[k])['mlp/Dense_1/kernel']).max() > 0.01
    assert opt['count'] == 0 and opt['step'] == 1           # utils/flax_utils.py:81: TrainState.step starts at 1
    for path, m in O.tree_leaves_with_path(opt['mu']):
        assert not m.any(), path


def assert_info_close(got, want, rtol=2e-5, atol=2e-6, keys=None):
    for k in (keys or O.INFO_KEYS):
        g, w = float(got[k]), float(want[k])
        assert abs(g - w) <= atol + rtol * abs(w), (k, g, w)


def assert_total_loss_matches(agent, ref, params, batch, noise):
    """total_loss on both sides: the loss and the first 10 infos; the engine's state is unchanged afterwards."""
    loss_ref, info_ref = ref.total_loss(batch, noise)
    loss, info = agent.total_loss(batch, noise=noise)
    assert abs(loss - float(loss_ref)) <= 2e-6 + 2e-5 * abs(float(loss_ref))
    assert_info_close(info, info_ref, keys=O.INFO_KEYS[:10])
    # total_loss must not change any state
    for p, a in leaf_dict(agent.get_params()).items():
        np.testing.assert_array_equal(a, leaf_dict(params)[p], err_msg=p)


def assert_step_matches(agent, ref, cfg, batch, noise, step=None):
    """One update on both sides: 13 infos, every leaf's gradient (Adam mu / 0.1 after the first step from zero moments), nu, post-step
    parameters.  `step(agent, batch, noise)` runs the GPU side (default: agent.update) and returns the infos or None (then read_info).
    The parameter check here is a first-step check only: from zero moments Adam's step is lr g / (|g| + 1e-8), +-lr whatever the gradient is,
    so it says little about the Adam arithmetic; tests/test_gpu_optimizer.py holds Adam, Polyak and the gradient statistics to the fp64
    restatement from non-zero moments and at large counts."""
    _, _, g_ref = ref.grads(batch, noise)
    info_u = step(agent, batch, noise) if step is not None else agent.update(batch, noise=noise)[1]
    if info_u is None:
        info_u = agent.read_info()
    _, info_ru = ref.update(batch, noise)
    assert_info_close(info_u, info_ru, rtol=5e-5, atol=5e-6)
    opt = agent.get_opt_state()
    assert opt['count'] == 1 and opt['step'] == 2
    mu, nu = leaf_dict(opt['mu']), leaf_dict(opt['nu'])
    new, new_ref = leaf_dict(agent.get_params()), leaf_dict(ref.params)
    lr = cfg['lr']
    worst = (0.0, None)
    for p, g in leaf_dict(g_ref).items():
        scale = np.abs(g).max()
        tol = 2e-5 * scale + 1e-9
        err = np.abs(mu[p] / 0.1 - g).max()
        worst = max(worst, (err / max(scale, 1e-30), p))
        np.testing.assert_allclose(mu[p] / 0.1, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p] / 0.001, g * g, rtol=1e-4, atol=tol * scale + 1e-12, err_msg=f'nu {p}')
        d = np.abs(new[p] - new_ref[p])
        stable = np.abs(g) > 50 * tol
        if 'target' in p:
            assert d.max() <= 1e-6, p
        else:
            assert d[stable].max(initial=0) <= 2e-6, (p, d[stable].max())
            assert d.max() <= 2 * lr + 1e-6, p
    return worst


def bf16x3_update_errors(agent, ref, batch, noise):
    """One update on both sides in the form test_gpu_precision.py bounds at 1e-4: (worst |g_gpu - g_ref| / max|g_ref| over the leaves and
    its leaf, {info: |delta| / max(1, |ref|)})."""
    _, _, g_ref = ref.grads(batch, noise)
    _, info = agent.update(batch, noise=noise)
    _, info_r = ref.update(batch, noise)
    mu = leaf_dict(agent.get_opt_state()['mu'])
    worst = (0.0, None)
    for p, g in leaf_dict(g_ref).items():
        sc = np.abs(g).max()
        worst = max(worst, (float(np.abs(mu[p] / 0.1 - g).max() / max(sc, 1e-30)), p))
    deltas = {k: abs(float(info[k]) - float(info_r[k])) / max(1.0, abs(float(info_r[k]))) for k in O.INFO_KEYS}
    return worst, deltas


BF16X3_BOUND = 1e-4          # both bounds of the bf16x3 mode: every info (BASELINE.json's "losses within 1e-4") and every leaf's gradient

# fql_debug_plan's kernel entries and the op types its records name (fql_amd/csrc/fql_engine.hip: the PLAN_K_* codes, enum OpType)
K_OTHER, K_GEMM16, K_GEMM16_KBIG, K_GEMM16_EULER, K_GEMM16_EULER_KBIG, K_SIDE, K_SIDE_SPLIT, K_SIDE_BIG, K_CHAIN, K_CHAIN_SPLIT = range(10)
OP_GEMM, OP_GEMM64, OP_CHAIN = 0, 1, 20
OP_DGRAD0 = 24   # the lean 16-column first-layer input gradient: a launch of its own, 16 rows per workgroup and task, no task records


def plan_lib():
    import ctypes as C
    from fql_amd import _cabi
    lib = _cabi.load()
    lib.fql_debug_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.fql_debug_plan.restype = C.c_int
    return lib


def read_plan(agent):
    """The update program of a state agent as the engine would launch it (the diagnostic export fql_debug_plan): a list of launches
    {index, lane, type, grid, kernel, gemm: [{M, N, K, rows, wk, xg}], wgrad: [{M, Kin, N, split}], ln: [M], chain: {M, H, variant, xg,
    split} or None}."""
    lib = plan_lib()
    head = np.zeros(1, np.int32)
    rc = lib.fql_debug_plan(agent._h, head.ctypes.data, 4)
    assert rc == 0, rc
    w = np.zeros(int(head[0]), np.int32)
    rc = lib.fql_debug_plan(agent._h, w.ctypes.data, w.nbytes)
    assert rc == 0, rc
    w = [int(v) for v in w]
    at, out = 2, []
    for _ in range(w[1]):
        index, lane, ty, grid, kernel, ng, nw, nl, nc = w[at:at + 9]
        at += 9
        L = dict(index=index, lane=lane, type=ty, grid=grid, kernel=kernel, gemm=[], wgrad=[], ln=[], chain=None)
        for _ in range(ng):
            L['gemm'].append(dict(zip(('M', 'N', 'K', 'rows', 'wk', 'xg'), w[at:at + 6])))
            at += 6
        for _ in range(nw):
            L['wgrad'].append(dict(zip(('M', 'Kin', 'N', 'split'), w[at:at + 4])))
            at += 4
        L['ln'] = w[at:at + nl]
        at += nl
        if nc:
            L['chain'] = dict(zip(('M', 'H', 'variant', 'xg', 'split'), w[at:at + 5]))
            at += 5
        out.append(L)
    assert at == len(w) and [L['index'] for L in out] == list(range(len(out)))
    return out


def plan_gemm(plan, kernels=None):
    """Every GEMM task of a plan (of the launches bound to `kernels`, if given) with its launch's kernel entry, type and index."""
    return [dict(t, kernel=L['kernel'], type=L['type'], launch=L['index']) for L in plan if kernels is None or L['kernel'] in kernels
            for t in L['gemm']]


def plan_wgrad(plan):
    return [t for L in plan for t in L['wgrad']]


def plan_ln(plan):
    return [m for L in plan for m in L['ln']]


def plan_has(tasks, M, N, K, **kw):
    return [t for t in tasks if (t['M'], t['N'], t['K']) == (M, N, K) and all(t[k] == v for k, v in kw.items())]


def print_plan(name, plan):
    """One line per family: what a path test prints before it asserts its property."""
    g = plan_gemm(plan)
    print(name, 'gemm (kernel, type, M, N, K, rows):', sorted({(t['kernel'], t['type'], t['M'], t['N'], t['K'], t['rows']) for t in g}))
    print(name, 'wgrad (M, Kin, N):', sorted({(t['M'], t['Kin'], t['N']) for t in plan_wgrad(plan)}), 'ln M:', sorted(set(plan_ln(plan))),
          'other launches (type, grid):', sorted({(L['type'], L['grid']) for L in plan if L['type'] not in (OP_GEMM, OP_GEMM64)}))


def assert_trajectory_tracks_oracle(od, ad, B, hidden, seed, steps=20, **cfgkw):
    """`steps` updates from the engine's own init on fresh rows and noise, against the fp32 oracle on the same sequence: the infos of
    every step within 2e-3 relative.  The optimizer counters advance once per update."""
    import fql_amd
    cfg, ds, batch, noise = make_problem(od, ad, B, hidden, seed=seed, **cfgkw)
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    params = agent.get_params()
    ref = O.OracleFQL(params, dict(cfg), od, ad, np.float32)
    rng = np.random.default_rng(0)
    for s in range(steps):
        idx = rng.integers(0, len(ds['observations']), size=B)
        b = O.sample_batch(ds, idx)
        nz = O.make_noise(B, ad, 100 + s)
        _, ig = agent.update(b, noise=nz)
        _, ir = ref.update(b, nz)
        assert_info_close(ig, ir, rtol=2e-3, atol=2e-4)
    opt = agent.get_opt_state()
    assert opt['count'] == steps and opt['step'] == steps + 1


def sync_restatement(ref, agent):
    """Continue the restatement from the engine's state: parameters, Adam moments and counters, cast to the restatement's dtype.  Two
    trajectories part after one step where |g| is within fp32 error (Adam's first step is lr sign(g) there), and the next step's gradient
    then differs by more than its per-step bound allows; after this call the next step is compared on identical inputs."""
    cast = lambda t: O.tree_map(lambda a: np.array(a, dtype=ref.dtype), t)   # noqa: E731
    opt = agent.get_opt_state()
    ref.params, ref.mu, ref.nu = cast(agent.get_params()), cast(opt['mu']), cast(opt['nu'])
    ref.count, ref.step = opt['count'], opt['step']
