"""GPU: agent.network.select(name)(...) / fql_module_forward - one module's forward on the stored parameters and the caller's rows.

The oracle is oracle.fql_oracle.mlp_forward in fp64 on agent.get_params() leaves after tests.util.randomize_params (IQL-diffusion's
tree has no `modules_` prefix: the same perturbation, restated below).  Bounds: fp32 per element 2e-6 + 2e-5 |ref| (the info bound of
tests/test_gpu_parity.py), bf16x3 1e-4 max(1, |ref|) (tests/test_gpu_precision.py).  Every parity case prints its worst error as a
fraction of its bound before it asserts."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import assert_same_state, leaf_dict, randomize_params

pytestmark = pytest.mark.gpu

# (obs, act, hidden): smallest; the flagship's dims; ragged widths and 3 layers; the two action widths past the 16-column pad; 512-wide
SHAPES = {
    'small': (7, 3, (32,) * 4),
    'h64': (29, 8, (64,) * 4),
    'ragged': (17, 6, (80, 48, 64)),
    'act16': (29, 16, (64,) * 4),
    'act21': (29, 21, (64,) * 4),
    'h512': (29, 8, (512,) * 4),
}
KINDS = ('fql', 'ifql', 'rebrac', 'sac', 'iql', 'iqld')
NS = (1, 5, 16, 37)
B = 16


def _bound_fp32(ref):
    return 2e-6 + 2e-5 * np.abs(ref)


def _bound_bf16x3(ref):
    return 1e-4 * np.maximum(1.0, np.abs(ref))


def _make(kind, od, ad, hidden, seed=0, **kw):
    """An agent of `kind` with MLPs `hidden` and batch size B; kw: layer_norm / actor_layer_norm / precision / further config."""
    import fql_amd
    from fql_amd import ifql, iql, iql_diffusion, rebrac, sac
    ob, ac = np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32)
    if kind == 'iqld':
        cfg = iql_diffusion.get_config()
        cfg.update(actor_hidden_dims=tuple(hidden), hidden_dims=tuple(hidden), batch_size=B)
        cfg.update(kw)
        return fql_amd.IQLDiffusionAgent.create(seed, ob, ac, cfg)
    cls, cfg = {'fql': (fql_amd.FQLAgent, fql_amd.get_config()), 'ifql': (fql_amd.IFQLAgent, ifql.get_config()),
                'rebrac': (fql_amd.ReBRACAgent, rebrac.get_config()), 'sac': (fql_amd.SACAgent, sac.get_config()),
                'iql': (fql_amd.IQLAgent, iql.get_config())}[kind]
    cfg.update(actor_hidden_dims=tuple(hidden), value_hidden_dims=tuple(hidden), batch_size=B)
    cfg.update(kw)
    return cls.create(seed, ob, ac, cfg)


def _randomize(agent, seed):
    """tests.util.randomize_params on the agent's leaves, written back; returns the tree the engine now holds."""
    params = agent.get_params()
    if 'modules_critic' in params:
        params = randomize_params(params, seed)
    else:   # IQL-diffusion: bare 'critic' / 'target_critic' / 'value' / 'actor' trees
        rng = np.random.default_rng(seed)
        out = O.tree_map(lambda a: np.array(a, dtype=np.float64), params)
        for path, leaf in O.tree_leaves_with_path(out):
            if path.endswith('/bias') or path.endswith('/scale'):
                leaf += 0.1 * rng.standard_normal(leaf.shape)
        out['target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), out['critic'])
        params = O.tree_map(lambda a: a.astype(np.float32), out)
    agent.set_params(params)
    return agent.get_params()


def _rows(od, ad, n, seed):
    """observations, actions in [-1, 1], and times off any grid (ActorVectorField takes any real t)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-1, 1, (n, ad)).astype(np.float32),
            rng.uniform(-0.5, 1.5, n).astype(np.float32))


def _oracle(params, name, obs, act=None, t=None):
    """fp64 restatement of the module on the fp32 leaves: Value (utils/networks.py) or ActorVectorField."""
    tree = O.tree_map(lambda a: np.asarray(a, np.float64), params['modules_' + name] if 'modules_' + name in params else params[name])
    cols = [np.asarray(obs, np.float64)]
    if act is not None:
        cols.append(np.asarray(act, np.float64))
    if t is not None:
        cols.append(np.asarray(t, np.float64).reshape(-1, 1))
    x = np.concatenate(cols, axis=-1)
    if name in ('critic', 'target_critic'):
        return np.stack([O.mlp_forward(tree['value_net'], x, member=e)[:, 0] for e in range(2)])
    if name == 'value':
        return O.mlp_forward(tree['value_net'], x)[:, 0]
    return O.mlp_forward(tree['mlp'], x)


def _query(agent, name, obs, act, t):
    fam = agent._modules[name]
    f = agent.network.select(name)
    if fam == 'value':
        return f(obs)
    if fam == 'pair':
        return f(obs, actions=act)
    return f(obs, act, t) if fam == 'field_t' else f(obs, act)


def _want(agent, params, name, obs, act, t):
    fam = agent._modules[name]
    return _oracle(params, name, obs, None if fam == 'value' else act, t if fam == 'field_t' else None)


def _check_all_modules(agent, params, od, ad, bound, tag, ns=NS):
    worst = 0.0
    for name in agent._modules:
        for n in ns:
            obs, act, t = _rows(od, ad, n, 11 * n + len(name))
            got = _query(agent, name, obs, act, t)
            want = _want(agent, params, name, obs, act, t)
            assert got.shape == want.shape and got.dtype == np.float32, (name, n, got.shape, want.shape)
            ratio = float((np.abs(got - want) / bound(want)).max())
            worst = max(worst, ratio)
            print(f'{tag} {name} n={n}: worst error / bound = {ratio:.3f}')
            assert ratio <= 1.0, (tag, name, n, ratio)
    return worst


# ---- 1. oracle parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('kind', KINDS)
def test_every_module_matches_the_fp64_oracle(kind, shape):
    od, ad, hidden = SHAPES[shape]
    agent = _make(kind, od, ad, hidden)
    params = _randomize(agent, 3)
    _check_all_modules(agent, params, od, ad, _bound_fp32, f'{kind}/{shape}')
    agent.close()


@pytest.mark.parametrize('kw', [dict(layer_norm=False), dict(actor_layer_norm=True)], ids=['no_critic_ln', 'actor_ln'])
def test_layer_norm_variants_match_the_oracle(kw):
    od, ad, hidden = SHAPES['h64']
    for kind in ('fql', 'ifql'):
        agent = _make(kind, od, ad, hidden, **kw)
        params = _randomize(agent, 4)
        _check_all_modules(agent, params, od, ad, _bound_fp32, f'{kind}/{kw}')
        agent.close()


def test_bf16x3_fql_matches_the_oracle_within_the_split_bound():
    od, ad, hidden = SHAPES['h512']
    agent = _make('fql', od, ad, hidden, precision='bf16x3')
    params = _randomize(agent, 5)
    _check_all_modules(agent, params, od, ad, _bound_bf16x3, 'fql/bf16x3/h512')
    agent.close()


def test_one_observation_drops_the_row_axis():
    od, ad, hidden = SHAPES['small']
    agent = _make('ifql', od, ad, hidden)
    _randomize(agent, 6)
    obs, act, t = _rows(od, ad, 1, 0)
    net = agent.network
    q, v, f = net.select('critic')(obs[0], actions=act[0]), net.select('value')(obs[0]), net.select('actor_flow')(obs[0], act[0], t[0])
    assert q.shape == (2,) and v.shape == () and f.shape == (ad,)
    np.testing.assert_array_equal(q, net.select('critic')(obs, actions=act)[:, 0])
    np.testing.assert_array_equal(v, net.select('value')(obs)[0])
    np.testing.assert_array_equal(f, net.select('actor_flow')(obs, act, t)[0])
    np.testing.assert_array_equal(f, net.select('actor_flow')(obs, act, t.reshape(1, 1), is_encoded=True)[0])   # times [n, 1]; is_encoded ignored
    agent.close()


# ---- 2. row independence and chunking -------------------------------------------------------------------------------------------
def test_rows_are_independent_across_tiles_and_chunks():
    od, ad, hidden = SHAPES['h64']
    agent = _make('ifql', od, ad, hidden)
    _randomize(agent, 7)
    n = 4096 + 37
    obs, act, t = _rows(od, ad, n, 1)
    for name in ('critic', 'value', 'actor_flow'):
        big = _query(agent, name, obs, act, t)
        row = (lambda a, j: a[:, j]) if name == 'critic' else (lambda a, j: a[j])
        for j in (0, 4095, 4096, n - 1):
            one = _query(agent, name, obs[j:j + 1], act[j:j + 1], t[j:j + 1])
            np.testing.assert_array_equal(row(one, 0), row(big, j), err_msg=f'{name} row {j}')
        for m in (1, 5, 37):
            part = _query(agent, name, obs[:m], act[:m], t[:m])
            np.testing.assert_array_equal(part, big[:, :m] if name == 'critic' else big[:m], err_msg=f'{name} n={m}')
    agent.close()


# ---- 3. against the engine itself -----------------------------------------------------------------------------------------------
def test_onestep_query_clipped_is_sample_actions():
    """sample_actions runs the same layer launches with the clip in the head launch's epilogue (GF_CLIP_OUT); the query's head launch
    has no clip, so the two are not the same launches and the required bound, atol 2e-6, is what is asserted."""
    od, ad, hidden = SHAPES['h64']
    agent = _make('fql', od, ad, hidden)
    params = _randomize(agent, 8)
    head = params['modules_actor_onestep_flow']['mlp'][f'Dense_{len(hidden)}']
    head['kernel'] = head['kernel'] * 8.0                          # a head wide enough that some outputs leave [-1, 1]
    agent.set_params(params)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((37, od)).astype(np.float32)
    z = rng.standard_normal((37, ad)).astype(np.float32)
    raw = agent.network.select('actor_onestep_flow')(obs, z)
    assert np.abs(raw).max() > 1.0, 'no output outside the clip range: the test would not see a clipped query'
    np.testing.assert_allclose(np.clip(raw, -1, 1), agent.sample_actions(obs, noises=z), rtol=0, atol=2e-6)
    agent.close()


def test_target_critic_is_the_critic_at_create_and_parts_after_an_update():
    od, ad, hidden = SHAPES['h64']
    agent = _make('fql', od, ad, hidden, alpha=10.0)
    obs, act, _ = _rows(od, ad, 37, 2)
    net = agent.network
    np.testing.assert_array_equal(net.select('target_critic')(obs, actions=act), net.select('critic')(obs, actions=act))
    ds = O.make_synthetic_dataset(64, od, ad, seed=0)
    agent.update(O.sample_batch(ds, np.arange(B)), noise=O.make_noise(B, ad, 1))
    q, qt = net.select('critic')(obs, actions=act), net.select('target_critic')(obs, actions=act)
    assert np.abs(q - qt).max() > 0
    params = agent.get_params()
    for name, got in (('critic', q), ('target_critic', qt)):
        want = _oracle(params, name, obs, act)
        assert (np.abs(got - want) <= _bound_fp32(want)).all(), name
    agent.close()


def _batch(od, ad, seed):
    ds = O.make_synthetic_dataset(64, od, ad, seed=seed)
    return ds, O.sample_batch(ds, np.arange(B))


def _close(got, want):
    return abs(float(got) - float(want)) <= 2e-6 + 2e-5 * abs(float(want))


def test_fql_q_mean_of_total_loss_is_the_mean_of_the_critic_query():
    od, ad, hidden = SHAPES['h64']
    agent = _make('fql', od, ad, hidden, alpha=10.0)
    _randomize(agent, 9)
    _, batch = _batch(od, ad, 3)
    _, info = agent.total_loss(batch, noise=O.make_noise(B, ad, 2))
    q = agent.network.select('critic')(batch['observations'], actions=batch['actions']).astype(np.float64)
    assert _close(q.mean(), info['critic/q_mean']) and _close(q.max(), info['critic/q_max']) and _close(q.min(), info['critic/q_min'])
    agent.close()


@pytest.mark.parametrize('kind', ['ifql', 'iql'])
def test_value_infos_of_total_loss_are_the_value_query(kind):
    """value/v_* are statistics of value(observations).  critic/q_mean on these kinds is the TD target's mean (agents/ifql.py:48,55,
    agents/iql.py:45,52), r + discount mask value(next_observations): checked through the value query too."""
    od, ad, hidden = SHAPES['h64']
    agent = _make(kind, od, ad, hidden)
    _randomize(agent, 10)
    _, batch = _batch(od, ad, 4)
    _, info = agent.total_loss(batch)
    value = agent.network.select('value')
    v = value(batch['observations']).astype(np.float64)
    assert _close(v.mean(), info['value/v_mean']) and _close(v.max(), info['value/v_max']) and _close(v.min(), info['value/v_min'])
    tq = batch['rewards'] + float(np.float32(agent.config['discount'])) * batch['masks'] * value(batch['next_observations']).astype(np.float64)
    assert _close(tq.mean(), info['critic/q_mean'])
    agent.close()


def test_ifql_best_of_n_returns_the_candidate_the_critic_query_ranks_first():
    od, ad, hidden = SHAPES['h64']
    n, N = 5, 8
    agent = _make('ifql', od, ad, hidden, num_samples=N)
    _randomize(agent, 11)
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((n, od)).astype(np.float32)
    z = rng.standard_normal((n, N, ad)).astype(np.float32)
    chosen = agent.sample_actions(obs, noises=z)
    rep = np.repeat(obs, N, axis=0)
    cand = agent.compute_flow_actions(rep, z.reshape(n * N, ad))
    q = agent.network.select('critic')(rep, actions=cand).min(axis=0).reshape(n, N)
    cand = cand.reshape(n, N, ad)
    for i in range(n):
        ks = [k for k in range(N) if np.array_equal(cand[i, k], chosen[i])]
        assert ks, f'row {i}: the sampled action is none of the flow candidates'
        assert q[i, ks[0]] >= q[i].max(), (i, ks, q[i])
    agent.close()


# ---- 4. no state change, no aliasing --------------------------------------------------------------------------------------------
def _state(agent):
    opt = agent.get_opt_state()
    return leaf_dict(agent.get_params()), leaf_dict(opt['mu']), leaf_dict(opt['nu']), (opt['count'], opt['step']), agent.read_info()


def _mixed_queries(agent, od, ad, seed):
    obs, act, t = _rows(od, ad, 37, seed)
    return [_query(agent, name, obs, act, t) for name in agent._modules]


def test_queries_change_no_state_and_alias_no_workspace():
    od, ad, hidden = SHAPES['h64']
    agent, twin = (_make('fql', od, ad, hidden, alpha=10.0) for _ in range(2))
    ds, batch = _batch(od, ad, 5)
    noise = O.make_noise(B, ad, 3)
    for a in (agent, twin):
        a.upload_dataset(ds)
        a.update(batch, noise=noise)
    before = _state(agent)
    obs = batch['observations']
    _mixed_queries(agent, od, ad, 0)
    s1 = agent.sample_actions(obs, seed=5)
    assert agent.read_info() == before[4]
    # (an FQL handle's loss probe leaves its own infos where read_info reads: the twin runs the same probe, without queries)
    l1 = agent.total_loss(batch, noise=noise)
    _mixed_queries(agent, od, ad, 1)
    assert agent.total_loss(batch, noise=noise) == l1 == twin.total_loss(batch, noise=noise)
    np.testing.assert_array_equal(agent.sample_actions(obs, seed=5), s1)
    np.testing.assert_array_equal(twin.sample_actions(obs, seed=5), s1)
    after = _state(agent)
    for x, y in zip(before[:3], after[:3]):
        assert x.keys() == y.keys()
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)
    assert before[3] == after[3] and after[4] == twin.read_info()
    # five further updates on the engine's own queues; `agent` is queried between them, the twin never
    rng = np.random.default_rng(0)
    for _ in range(5):
        idx = rng.integers(0, 64, size=B)
        agent.update_from_dataset(idxs=idx)
        twin.update_from_dataset(idxs=idx)
        _mixed_queries(agent, od, ad, 2)
    assert_same_state(agent, twin)
    assert agent.read_info() == twin.read_info()
    agent.close(); twin.close()


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------
def test_a_query_sees_updates_still_on_the_engines_queues():
    od, ad, hidden = SHAPES['h64']
    agent, twin = (_make('fql', od, ad, hidden, alpha=10.0) for _ in range(2))
    ds, _ = _batch(od, ad, 6)
    idx = np.random.default_rng(1).integers(0, 64, size=(3, B))
    obs, act, t = _rows(od, ad, 37, 3)
    for a in (agent, twin):
        a.upload_dataset(ds)
    for i in range(3):
        agent.update_from_dataset(idxs=idx[i])
    got = _mixed_queries(agent, od, ad, 3)          # no synchronize in between
    for i in range(3):
        twin.update_from_dataset(idxs=idx[i])
    twin.synchronize()
    want = _mixed_queries(twin, od, ad, 3)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    q0 = _make('fql', od, ad, hidden, alpha=10.0)
    assert np.abs(q0.network.select('critic')(obs, actions=act) - got[0]).max() > 0, 'the updates moved nothing: the test shows no ordering'
    for a in (agent, twin, q0):
        a.close()


# ---- 6. pointers and streams ----------------------------------------------------------------------------------------------------
def test_cuda_tensors_on_either_stream_give_the_host_result():
    import torch
    od, ad, hidden = SHAPES['h64']
    agent = _make('ifql', od, ad, hidden)
    _randomize(agent, 12)
    obs, act, t = _rows(od, ad, 37, 4)
    host = {name: _query(agent, name, obs, act, t) for name in agent._modules}
    side = torch.cuda.Stream()
    for stream in (side, torch.cuda.default_stream()):
        with torch.cuda.stream(stream):
            dev = [torch.from_numpy(a).cuda() for a in (obs, act, t)]
            outs = {name: _query(agent, name, *dev) for name in agent._modules}
        stream.synchronize()
        for name, out in outs.items():
            assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
            np.testing.assert_array_equal(out.cpu().numpy(), host[name], err_msg=name)
    agent.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _still_works(agent, twin, update, sample):
    """After the refused calls `agent` updates and samples as the twin that made none."""
    update(agent); update(twin)
    assert_same_state(agent, twin)
    np.testing.assert_array_equal(sample(agent), sample(twin))


def test_bc_cfgrl_and_visual_handles_are_refused_with_state():
    import fql_amd
    from fql_amd import _cabi, bc, cfgrl
    lib = _cabi.load()
    od, ad, gd = 7, 3, 5
    rng = np.random.default_rng(0)
    obs, act = rng.standard_normal((B, od)).astype(np.float32), rng.uniform(-1, 1, (B, ad)).astype(np.float32)
    goals = rng.standard_normal((B, gd)).astype(np.float32)
    out = np.zeros((2, B), np.float32)

    def refused(agent, label):
        assert lib.fql_module_forward(agent._h, b'critic', _ptr(obs), _ptr(act), None, B, _ptr(out), None) == _cabi.FQL_E_STATE
        msg = lib.fql_last_error(agent._h)
        assert b'fql_module_forward' in msg and label in msg, msg
        with pytest.raises(NotImplementedError):
            agent.network

    bcfg = bc.get_config()
    bcfg.update(hidden_dims=(32, 32), batch_size=B)
    pair = [fql_amd.BCAgent.create(1, obs[:1], act[:1], bcfg) for _ in range(2)]
    refused(pair[0], b'BC handle')
    _still_works(*pair, lambda a: a.update({'observations': obs, 'actions': act}), lambda a: a.sample_actions(obs, seed=7))

    ccfg = cfgrl.get_config()
    ccfg.update(actor_hidden_dims=(32, 32), batch_size=B)
    ex = {'observations': obs[:1], 'actions': act[:1], 'value_goals': goals[:1]}
    pair = [fql_amd.CFGRLAgent.create(1, ex, ccfg) for _ in range(2)]
    refused(pair[0], b'CFGRL handle')
    _still_works(*pair, lambda a: a.update({'observations': obs, 'actions': act, 'actor_goals': goals}),
                 lambda a: a.sample_actions(obs, goals, seed=7))

    vcfg = fql_amd.get_config()
    vcfg.update(encoder='impala_small', actor_hidden_dims=(32, 32), value_hidden_dims=(32, 32), batch_size=B, alpha=3.0)
    img = rng.integers(0, 256, size=(B, 32, 32, 1), dtype=np.uint8)
    nimg = rng.integers(0, 256, size=(B, 32, 32, 1), dtype=np.uint8)
    pair = [fql_amd.FQLAgent.create(1, img[:1], act[:1], vcfg) for _ in range(2)]
    refused(pair[0], b'visual')
    vbatch = {'observations': img, 'actions': act, 'rewards': -np.ones(B, np.float32), 'masks': np.ones(B, np.float32), 'next_observations': nimg}
    _still_works(*pair, lambda a: a.update(vbatch), lambda a: a.sample_actions(img, seed=7))


def test_bad_modules_and_arguments_are_refused_and_the_handle_carries_on():
    from fql_amd import _cabi
    lib = _cabi.load()
    od, ad, hidden = SHAPES['small']
    agent, twin = (_make('ifql', od, ad, hidden) for _ in range(2))
    obs, act, t = _rows(od, ad, 5, 5)
    out = np.zeros((5, max(ad, 2)), np.float32)
    call = lambda m, o, a, tt, n: lib.fql_module_forward(agent._h, m, o, a, tt, n, _ptr(out), None)   # noqa: E731
    # unknown for the kind: FQL's module names on an IFQL handle, the Gaussian actor, anything else
    for name in (b'actor_bc_flow', b'actor_onestep_flow', b'actor', b'nonsense', b''):
        assert call(name, _ptr(obs), _ptr(act), None, 5) == _cabi.FQL_E_NOTFOUND, name
        msg = lib.fql_last_error(agent._h)
        assert all(m in msg for m in (b'critic', b'target_critic', b'value', b'actor_flow')), msg
    with pytest.raises(KeyError, match='critic, target_critic, value, actor_flow'):
        agent.network.select('actor')
    I = _cabi.FQL_E_INVALID
    assert call(b'critic', _ptr(obs), None, None, 5) == I                      # critic without actions
    assert call(b'value', _ptr(obs), _ptr(act), None, 5) == I                  # value with actions
    assert call(b'critic', _ptr(obs), _ptr(act), _ptr(t), 5) == I              # times on a module that takes none
    assert call(b'actor_flow', _ptr(obs), _ptr(act), None, 5) == I             # the vector field without times
    assert call(b'critic', None, _ptr(act), None, 5) == I
    assert lib.fql_module_forward(agent._h, b'critic', _ptr(obs), _ptr(act), None, 5, None, None) == I
    assert lib.fql_module_forward(agent._h, None, _ptr(obs), _ptr(act), None, 5, _ptr(out), None) == I
    assert call(b'critic', _ptr(obs), _ptr(act), None, 0) == I and call(b'critic', _ptr(obs), _ptr(act), None, -3) == I
    net = agent.network
    with pytest.raises(ValueError):
        net.select('critic')(obs)
    with pytest.raises(ValueError):
        net.select('value')(obs, actions=act)
    with pytest.raises(ValueError):
        net.select('actor_flow')(obs, act)
    with pytest.raises(ValueError):
        net.select('critic')(obs[:, :-1], actions=act)
    with pytest.raises(ValueError):
        net.select('critic')(obs, actions=act[:-1])
    with pytest.raises(ValueError):
        net.select('actor_flow')(obs, act, np.zeros((5, 2), np.float32))
    with pytest.raises(ValueError):
        net.select('value')(np.zeros((0, od), np.float32))
    with pytest.raises(NotImplementedError):
        net.select('critic')(obs, actions=act, params=agent.get_params())
    # FQL has its own names and no value net
    fql = _make('fql', od, ad, hidden)
    with pytest.raises(KeyError, match='actor_onestep_flow'):
        fql.network.select('value')
    with pytest.raises(ValueError):
        fql.network.select('actor_onestep_flow')(obs, act, t)                   # actor_onestep_flow takes no times
    assert lib.fql_module_forward(fql._h, b'actor_onestep_flow', _ptr(obs), _ptr(act), _ptr(t), 5, _ptr(out), None) == I
    assert lib.fql_module_forward(fql._h, b'value', _ptr(obs), None, None, 5, _ptr(out), None) == _cabi.FQL_E_NOTFOUND
    fql.close()
    ds, batch = _batch(od, ad, 7)
    noise = {'x0': O.make_noise(B, ad, 4)['x0'], 't': O.make_noise(B, ad, 4)['t']}
    _still_works(agent, twin, lambda a: a.update(batch, noise=noise), lambda a: a.sample_actions(batch['observations'], seed=7))
    agent.close(); twin.close()


# ---- 8. a group member ----------------------------------------------------------------------------------------------------------
def test_a_group_member_answers_right_after_the_groups_update():
    import fql_amd
    od, ad, hidden = SHAPES['h64']
    cfg = fql_amd.get_config()
    cfg.update(actor_hidden_dims=hidden, value_hidden_dims=hidden, batch_size=B, alpha=10.0)
    ex_o, ex_a = np.zeros((1, od), np.float32), np.zeros((1, ad), np.float32)
    ds, _ = _batch(od, ad, 8)
    idx = np.random.default_rng(2).integers(0, 64, size=(2, B))
    group = fql_amd.FQLAgentGroup.create([0, 1], ex_o, ex_a, cfg)
    group.upload_dataset(ds)
    group.update_from_dataset(idxs=idx)
    got = _mixed_queries(group.members[1], od, ad, 4)          # no synchronize in between
    alone = fql_amd.FQLAgent.create(1, ex_o, ex_a, cfg)
    alone.upload_dataset(ds)
    alone.update_from_dataset(idxs=idx[1])
    alone.synchronize()
    for g, w in zip(got, _mixed_queries(alone, od, ad, 4)):
        np.testing.assert_array_equal(g, w)
    group.close()
    alone.close()
    for m in group.members:
        m.close()
