"""GPU: the IQL agent (agents/iql.py) on the engine against the fp64 restatement in tests/iql_oracle.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import iql_oracle as IO
from tests.util import assert_info_close, leaf_dict, sync_restatement

pytestmark = pytest.mark.gpu
SMALL, BIG = (5, 2, 16, 32), (29, 8, 64, 128)   # obs, act, B, H; BIG: action width 8, rows not a multiple of 32 (tests/test_gpu_shapes.py)
MARGIN = 1e-3

# (shape, actor_loss, const_std, actor_layer_norm, seed).  The losses are not smooth at q = v, q1 = q2, |q_actions| = 1, alpha adv =
# log 100 and log_stds in {-5, 2}: each seed was chosen on the CPU so that the fp64 restatement keeps every element at least MARGIN away
# from every kink in both steps (_check_step asserts it), so no element is masked out of any comparison.
UPDATE_CASES = [
    (SMALL, 'awr', True, False, 0), (SMALL, 'awr', False, True, 0), (SMALL, 'ddpgbc', True, False, 0), (SMALL, 'ddpgbc', False, False, 0),
    (BIG, 'awr', True, False, 0), (BIG, 'awr', False, False, 0), (BIG, 'ddpgbc', True, True, 4), (BIG, 'ddpgbc', False, False, 4),
]


def _hidden(shape):
    """(actor hidden, value hidden) of a shape (obs, act, B, H): H is one width for 4 + 4 layers, or the pair of tuples itself."""
    H = shape[3]
    return ((H,) * 4, (H,) * 4) if isinstance(H, int) else (tuple(H[0]), tuple(H[1]))


def _cfg(shape, **kw):
    import fql_amd
    od, ad, B, _ = shape
    actor, value = _hidden(shape)
    cfg = fql_amd.iql.get_config()
    cfg.update(actor_hidden_dims=actor, value_hidden_dims=value, batch_size=B)
    cfg.update(kw)
    return cfg


def _problem(shape=SMALL, seed=0, **kw):
    """(cfg, dataset, batch, noise, params): parameters from the restatement's init, moved away from it (a CPU-only recipe, so the
    kink margins of a seed can be checked without a GPU)."""
    od, ad, B, _ = shape
    cfg = _cfg(shape, **kw)
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=B)
    params = IO.randomize(IO.init_params(seed + 3, od, ad, cfg), seed + 4)
    return cfg, ds, O.sample_batch(ds, idx), IO.make_noise(B, ad, seed + 2), params


def _agent(cfg, batch, seed=3, params=None):
    import fql_amd
    a = fql_amd.IQLAgent.create(seed, batch['observations'][:1], batch['actions'][:1], cfg)
    if params is not None:
        a.set_params(params)
    return a


def _ref(params, cfg, shape):
    return IO.OracleIQL(params, dict(cfg), shape[0], shape[1], np.float64)


def _same_state(a, b):
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
    oa, ob = a.get_opt_state(), b.get_opt_state()
    assert (oa['count'], oa['step']) == (ob['count'], ob['step'])
    for part in ('mu', 'nu'):
        la, lb = leaf_dict(oa[part]), leaf_dict(ob[part])
        for k in la:
            np.testing.assert_array_equal(la[k], lb[k], err_msg=f'{part} {k}')


@pytest.mark.parametrize('const_std', [True, False])
def test_leaves_match_reference_layout_and_init(const_std):
    od, ad, B, H = SMALL
    cfg, _, batch, _, _ = _problem(const_std=const_std)
    a = _agent(cfg, batch)
    want = {p: v.shape for p, v in O.tree_leaves_with_path(IO.init_params(0, od, ad, cfg))}
    assert dict(a.leaves()) == want
    assert ('modules_actor/log_stds' in dict(a.leaves())) == (not const_std)
    p = leaf_dict(a.get_params())
    if not const_std:
        assert p['modules_actor/log_stds'].shape == (ad,) and not p['modules_actor/log_stds'].any()
    assert p['modules_actor/mean_net/kernel'].shape == (H, ad) and p['modules_value/value_net/Dense_4/kernel'].shape == (H, 1)
    for k, v in p.items():
        if k.endswith('/bias'):
            assert not v.any(), k
        if k.endswith('/scale'):
            assert (v == 1).all(), k
        if k.endswith('/kernel'):
            lim = np.sqrt(6.0 * (1e-2 if 'mean_net' in k else 1.0) / (v.shape[-2] + v.shape[-1]))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim, k
        if k.startswith('modules_target_'):
            np.testing.assert_array_equal(v, p[k.replace('modules_target_', 'modules_')])


def _check_step(a, ref, batch, noise, cfg, pre):
    """One update of both sides on (batch, noise) from their current state: the kink margins of the restatement, then infos, every
    leaf's gradient (read back out of Adam's first moment), nu, the post-step parameters and the Polyak target.  Returns the worst
    gradient error relative to its leaf's largest gradient, with the leaf's name, and the restatement's infos."""
    keys = IO.INFO_KEYS[cfg['actor_loss']]
    f = ref._forward(batch, noise)
    margins = ref.kink_margins(batch, noise, f)
    assert min(margins.values()) >= MARGIN, margins
    _, want, g_ref = ref._losses(batch, noise, want_grads=True, f=f)
    mu0 = leaf_dict(a.get_opt_state()['mu'])
    pre_ref = leaf_dict(O.tree_map(np.copy, ref.params))
    _, info = a.update(batch, noise=noise)
    info = info.to_dict()
    assert tuple(info) == keys
    want.update(ref.grad_stats(g_ref))   # OracleIQL.update, on the forward pass and the gradients computed above
    ref.apply_gradients(g_ref)
    want = {k: float(want[k]) for k in keys}
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=keys)
    a.synchronize()
    opt = a.get_opt_state()
    mu, nu, mu_ref, nu_ref = leaf_dict(opt['mu']), leaf_dict(opt['nu']), leaf_dict(ref.mu), leaf_dict(ref.nu)
    new, new_ref = leaf_dict(a.get_params()), leaf_dict(ref.params)
    worst = (0.0, '')
    for p, g in leaf_dict(g_ref).items():
        if p.startswith('modules_target_'):   # Polyak from the PRE-step critic
            np.testing.assert_allclose(new[p], 0.005 * pre[p.replace('target_', '')] + 0.995 * pre[p], atol=1e-6, err_msg=p)
            continue
        # the bounds of tests/test_gpu_sac.py
        tol = 5e-5 * np.abs(g).max() + 1e-5 * np.abs(mu0[p]).max() + 1e-9
        got = (mu[p] - np.float32(0.9) * mu0[p]) / 0.1
        worst = max(worst, (float(np.abs(got - g).max() / max(np.abs(g).max(), 1e-30)), p))
        np.testing.assert_allclose(got, g, rtol=0, atol=tol, err_msg=f'grad {p}')
        np.testing.assert_allclose(nu[p], nu_ref[p], rtol=1e-4, atol=1e-4 * np.abs(nu_ref[p]).max() + 1e-20, err_msg=f'nu {p}')
        d = np.abs((new[p] - pre[p]) - (new_ref[p] - pre_ref[p]))
        stable = (np.abs(g) > 50 * tol) & (np.abs(mu_ref[p]) > 5 * tol)
        assert np.max(d[stable], initial=0) <= 2e-6, (p, np.max(d[stable], initial=0))
        assert d.max() <= 2 * cfg['lr'] + 1e-6, p
    return worst, want


@pytest.mark.parametrize('shape,actor_loss,const_std,actor_ln,seed', UPDATE_CASES)
def test_update_matches_fp64_restatement(shape, actor_loss, const_std, actor_ln, seed):
    """Two steps: the second from non-zero moments.  Infos, every leaf's gradient, nu, post-step parameters, the Polyak target."""
    cfg, _, batch, noise, params = _problem(shape, seed, actor_loss=actor_loss, const_std=const_std, actor_layer_norm=actor_ln)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, shape)
    _check_step(a, ref, batch, noise, cfg, leaf_dict(params))
    _check_step(a, ref, batch, IO.make_noise(shape[2], shape[1], seed + 77), cfg, leaf_dict(a.get_params()))
    opt = a.get_opt_state()
    assert opt['count'] == 2 and opt['step'] == 3


# ---- the shapes that switch kernel paths -----------------------------------------------------------------------------------------------
#
# What each case reaches, from the conditions in fql_amd/csrc/fql_engine.hip.  The critic's first layer has in_p = round64(obs + act).
# Its input gradient (read by fql_iql_actor_grad_kernel at dx[b * in_p + obs + a] under ddpgbc) is the lean 16-column OP_DGRAD0 when
# K = H is a multiple of 512, M is a multiple of 16, act <= 16 and obs + 16 <= in_p; otherwise the generic first-layer dgrad GEMM.
# ap = pad16(act) is the width of the log_stds slot, of ls_part [B, ap] and of g_ls [ap].  The row loops of the AWR, DDPG+BC and
# actor-grad kernels and of iql_reduce_log_stds step by 256 threads; fql_iql_head_kernel takes 256 rows per block.
#   name: ((obs, act, B, (actor hidden, value hidden)), cfg overrides, steps)
H512 = ((512,) * 4, (512,) * 4)
SHAPE_CASES = {
    # IQL's default configuration: OP_DGRAD0 (in_p 64, 29 + 16 <= 64) with 8 live columns; 64x64 LDS-tiled GEMMs with LayerNorm
    # partial sums; the value pass at M = 512
    'default': ((29, 8, 256, H512), {}, 2),
    # OP_DGRAD0 with all 16 columns live; ap = 16 with no padding column
    'act16': ((29, 16, 256, H512), {}, 2),
    # act > 16: the generic dgrad (in_p 128); ap = 32 with 11 padding columns
    'humanoidmaze': ((69, 21, 256, H512), dict(discount=0.995), 2),
    # four rows per thread and four head-kernel blocks; the value pass at M = 2048; OP_DGRAD0 with 4 live columns (in_p 64,
    # 40 + 16 <= 64).  One step: the fp64 restatement costs most here.
    'b1024': ((40, 4, 1024, H512), {}, 1),
    # obs + 16 > in_p = 64 with act <= 16: the generic dgrad at H 512 feeding an action block 4 wide; the actor's LayerNorm at H 512
    'obs50': ((50, 4, 256, H512), dict(actor_layer_norm=True), 1),
    # ragged widths, actor and value networks of different depth; ap = 32 with 8 padding columns; generic dgrad (K = 80)
    'ragged_depths': ((45, 24, 48, ((64, 64), (80, 48, 64))), {}, 2),
    # 256 + 16 rows: threads 0..15 take two rows, the rest one; two head-kernel blocks, the second 16 rows; M no multiple of 64
    'b272': ((11, 5, 272, ((64,) * 4, (64,) * 4)), {}, 2),
    # hidden widths that are no multiple of 16: out 50 of out_p 64 in the value, critic and actor nets (LayerNorm over 50 of 64 columns)
    'w50_padded': ((29, 8, 32, ((50,) * 3, (50,) * 3)), {}, 2),
}

# (case, actor_loss, const_std, seed).  Under ddpgbc with log_stds the |x| = 1 kink is cleared by IO.clear_of_unit_clip at the state
# of each step.  A later step runs from the engine's own state (sync_restatement: the two trajectories part by up to 2 lr per element
# where |g| is within fp32 error), which the CPU cannot know, so there the seed must leave room: each seed is the smallest of 0..7
# for which the fp64 restatement, on its own trajectory, keeps every margin >= MARGIN in the first step and >= 3 MARGIN in the second
# (tests/test_kink_margins_cpu.py checks that on the CPU; _check_step asserts MARGIN at the state it actually runs from).
# ragged_depths with ddpgbc and const_std=True is left out: there x = mean has no noise to move, and no seed in 0..7 keeps all
# 48 x 24 means 1e-3 away from |mean| = 1.
SHAPE_COMBOS = [
    ('default', 'awr', False, 1), ('default', 'ddpgbc', False, 1),
    ('act16', 'awr', False, 1), ('act16', 'ddpgbc', False, 1), ('act16', 'ddpgbc', True, 4),
    ('humanoidmaze', 'awr', False, 0), ('humanoidmaze', 'ddpgbc', False, 0), ('humanoidmaze', 'ddpgbc', True, 2),
    ('b1024', 'awr', False, 0), ('b1024', 'ddpgbc', False, 0),
    ('obs50', 'awr', False, 0), ('obs50', 'ddpgbc', False, 0),
    ('ragged_depths', 'awr', False, 0), ('ragged_depths', 'ddpgbc', False, 0),
    ('b272', 'awr', False, 1), ('b272', 'ddpgbc', False, 2),
    ('w50_padded', 'awr', False, 0), ('w50_padded', 'ddpgbc', False, 0),
]
# the batch-size switch: one ddpgbc agent with log_stds, these batch sizes in turn (data seed SWITCH_SEED + step)
SWITCH_SHAPE, SWITCH_BATCHES, SWITCH_SEED = (29, 8, 64, 64), (64, 16, 272, 64), 0


def _cleared(ref, batch, noise, cfg):
    """`noise` moved off the |x| = 1 kink at ref's current parameters, where the loss reads it (ddpgbc with log_stds)."""
    if cfg['actor_loss'] == 'ddpgbc' and not cfg['const_std']:
        return IO.clear_of_unit_clip(ref, batch, noise, MARGIN)
    return noise


def shape_problem(case, actor_loss, const_std, seed):
    """(shape, steps, cfg, batch, params, noises): the problem of one SHAPE_COMBOS entry, built without an engine.  noises[i] is the
    draw of step i, to be passed through _cleared at the restatement's state before that step."""
    shape, kw, steps = SHAPE_CASES[case]
    cfg, _, batch, noise, params = _problem(shape, seed, actor_loss=actor_loss, const_std=const_std, **kw)
    return shape, steps, cfg, batch, params, [noise, IO.make_noise(shape[2], shape[1], seed + 77)][:steps]


def switch_problem(cfg, i, B):
    """(batch, noise) of step i of the batch-size switch test."""
    od, ad = SWITCH_SHAPE[:2]
    ds = O.make_synthetic_dataset(max(4 * B, 64), od, ad, seed=SWITCH_SEED + i)
    idx = np.random.default_rng(SWITCH_SEED + i + 1).integers(0, len(ds['observations']), size=B)
    return O.sample_batch(ds, idx), IO.make_noise(B, ad, SWITCH_SEED + i + 2)


@pytest.mark.parametrize('case,actor_loss,const_std,seed', SHAPE_COMBOS)
def test_shape_cases_match_fp64_restatement(case, actor_loss, const_std, seed):
    """total_loss (no state change), then the update steps of test_update_matches_fp64_restatement, at the shapes above, the second
    one from the engine's own state and moments.  Nothing is masked out of any comparison."""
    shape, steps, cfg, batch, params, noises = shape_problem(case, actor_loss, const_std, seed)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, shape)
    keys = IO.INFO_KEYS[actor_loss]
    noise = _cleared(ref, batch, noises[0], cfg)
    loss, info = a.total_loss(batch, noise=noise)
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0
    worst, want = _check_step(a, ref, batch, noise, cfg, leaf_dict(params))
    # the first step's infos are total_loss's: the restatement computes them once
    assert tuple(info) == keys[:-3]
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=keys[:-3])
    want_loss = want['value/value_loss'] + want['critic/critic_loss'] + want['actor/actor_loss']
    assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    for nz in noises[1:]:
        sync_restatement(ref, a)
        worst = max(worst, _check_step(a, ref, batch, _cleared(ref, batch, nz, cfg), cfg, leaf_dict(a.get_params()))[0])
    opt = a.get_opt_state()
    assert opt['count'] == steps and opt['step'] == steps + 1
    print(f'worst relative gradient error {worst[0]:.3e} ({worst[1]})')


def test_batch_size_switches_track_restatement():
    """B = 64, 16, 272, 64: each switch rebuilds the workspace and the programs; every step is compared after the rebuild, from the
    engine's own carried state."""
    cfg, _, _, _, params = _problem(SWITCH_SHAPE, SWITCH_SEED, actor_loss='ddpgbc', const_std=False)
    batch0, _ = switch_problem(cfg, 0, SWITCH_BATCHES[0])
    a = _agent(cfg, batch0, params=params)
    ref = _ref(params, cfg, SWITCH_SHAPE)
    for i, B in enumerate(SWITCH_BATCHES):
        batch, noise = switch_problem(cfg, i, B)
        assert a.get_opt_state()['count'] == i
        sync_restatement(ref, a)
        _check_step(a, ref, batch, _cleared(ref, batch, noise, cfg), cfg, leaf_dict(a.get_params()))
    opt = a.get_opt_state()
    assert opt['count'] == 4 and opt['step'] == 5


@pytest.mark.parametrize('case', ['act16', 'humanoidmaze'])
def test_sample_actions_at_hidden_512(case):
    """n = 1, 37 and 4097 (one row past the first 4096-row chunk) with explicit noise at temperature 1 and 0; row n - 1 equals its
    single-observation call bitwise."""
    shape, kw, _ = SHAPE_CASES[case]
    od, ad = shape[:2]
    cfg, _, batch, _, params = _problem(shape, 6, const_std=False, **kw)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, shape)
    rng = np.random.default_rng(6)
    obs = rng.standard_normal((4097, od)).astype(np.float32)
    z = rng.standard_normal((4097, ad)).astype(np.float32)
    want = {t: ref.sample_actions(obs, z, t) for t in (1.0, 0.0)}   # row-wise: the first n rows are the n-row call's
    for n in (1, 37, 4097):
        for temp in (1.0, 0.0):
            got = a.sample_actions(obs[:n], noises=z[:n], temperature=temp)
            assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
            np.testing.assert_allclose(got, want[temp][:n], atol=2e-5, err_msg=f'{n} {temp}')
            np.testing.assert_array_equal(got[n - 1], a.sample_actions(obs[n - 1], noises=z[n - 1], temperature=temp))


@pytest.mark.parametrize('actor_loss', ['awr', 'ddpgbc'])
def test_log_stds_outside_the_clip_get_exactly_zero_gradient(actor_loss):
    """raw log_stds = (-6, 3): both outside [-5, 2], so the clip passes no gradient and Adam leaves the leaf and its moments untouched."""
    cfg, _, batch, noise, params = _problem(SMALL, 1, actor_loss=actor_loss, const_std=False)
    params['modules_actor']['log_stds'] = np.array([-6.0, 3.0], np.float32)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, SMALL)
    _, _, g = ref._losses(batch, noise, want_grads=True)
    assert not g['modules_actor']['log_stds'].any()
    _, info = a.update(batch, noise=noise)
    _, want = ref.update(batch, noise)
    assert_info_close(info.to_dict(), want, rtol=5e-5, atol=5e-6, keys=IO.INFO_KEYS[actor_loss])
    assert abs(want['actor/std'] - 0.5 * (np.exp(-5.0) + np.exp(2.0))) < 1e-12
    a.synchronize()
    opt = a.get_opt_state()
    assert not leaf_dict(opt['mu'])['modules_actor/log_stds'].any() and not leaf_dict(opt['nu'])['modules_actor/log_stds'].any()
    np.testing.assert_array_equal(leaf_dict(a.get_params())['modules_actor/log_stds'], [-6.0, 3.0])
    assert leaf_dict(opt['mu'])['modules_actor/mean_net/bias'].any()


@pytest.mark.parametrize('actor_loss,const_std', [('awr', False), ('ddpgbc', False), ('ddpgbc', True)])
def test_total_loss_matches_update_infos_and_changes_no_state(actor_loss, const_std):
    cfg, _, batch, noise, params = _problem(BIG, 2, actor_loss=actor_loss, const_std=const_std)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, BIG)
    keys = IO.INFO_KEYS[actor_loss][:-3]
    loss, info = a.total_loss(batch, noise=noise)
    want_loss, want = ref.total_loss(batch, noise)
    assert tuple(info) == keys
    assert_info_close(info, want, rtol=5e-5, atol=5e-6, keys=keys)
    assert abs(loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    a.synchronize()
    after = leaf_dict(a.get_params())
    for k, v in leaf_dict(params).items():
        np.testing.assert_array_equal(after[k], v, err_msg=k)
    assert a.get_opt_state()['count'] == 0
    # the update on the same batch reports the same numbers, and a later probe leaves them readable
    _, uinfo = a.update(batch, noise=noise)
    uinfo = uinfo.to_dict()
    assert_info_close(uinfo, info, rtol=5e-5, atol=5e-6, keys=keys)
    a.total_loss(batch, noise=IO.make_noise(BIG[2], BIG[1], 160))
    assert a.read_info() == uinfo


@pytest.mark.parametrize('actor_loss', ['awr', 'ddpgbc'])
def test_update_from_dataset_explicit_rows_equals_update(actor_loss):
    cfg, ds, _, noise, _ = _problem(BIG, 4, actor_loss=actor_loss, const_std=False)
    B, n = cfg['batch_size'], len(ds['observations'])
    idx = np.random.default_rng(4).integers(0, n, size=B)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    a.upload_dataset(ds)
    for _ in range(3):
        a.update_from_dataset(idxs=idx, noise=noise)
        b.update(O.sample_batch(ds, idx), noise=noise)
    a.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()


@pytest.mark.parametrize('actor_loss', ['awr', 'ddpgbc'])
def test_aql_and_graph_updates_bitwise_over_20_steps(actor_loss):
    import torch
    cfg, ds, _, _, _ = _problem(BIG, 5, actor_loss=actor_loss, const_std=False)
    a, b = _agent(cfg, ds), _agent(cfg, ds)
    for x in (a, b):
        x.upload_dataset(ds)
    s = torch.cuda.Stream()
    for i in range(20):
        a.update_from_dataset()
        b.update_from_dataset(stream=s.cuda_stream)
    assert a.synchronize() == 'aql'
    s.synchronize(); b.synchronize()
    _same_state(a, b)
    assert a.read_info() == b.read_info()
    assert leaf_dict(a.get_params())['modules_actor/log_stds'].any()


@pytest.mark.parametrize('const_std', [True, False])
def test_sample_actions_matches_restatement(const_std):
    od, ad, B, H = BIG
    cfg, _, batch, _, params = _problem(BIG, 6, const_std=const_std)
    a = _agent(cfg, batch, params=params)
    ref = _ref(params, cfg, BIG)
    rng = np.random.default_rng(6)
    for n in (1, 5, 64):
        obs = rng.standard_normal((n, od)).astype(np.float32)
        z = rng.standard_normal((n, ad)).astype(np.float32)
        for temp in (0.0, 1.0, 0.5):
            got = a.sample_actions(obs, noises=z, temperature=temp)
            assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
            np.testing.assert_allclose(got, ref.sample_actions(obs, z, temp), atol=2e-5, err_msg=f'{n} {temp}')
            np.testing.assert_array_equal(got[n - 1], a.sample_actions(obs[n - 1], noises=z[n - 1], temperature=temp))
        # temperature 0: clip(mean) exactly, whatever the noise
        np.testing.assert_array_equal(a.sample_actions(obs, noises=z, temperature=0.0), a.sample_actions(obs, noises=-3 * z, temperature=0.0))
        np.testing.assert_array_equal(a.sample_actions(obs, noises=z, temperature=0.0), a.sample_actions(obs, seed=1, temperature=0.0))
    drawn = a.sample_actions(obs, seed=123)
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=123))
    assert np.abs(drawn).max() <= 1.0 and not np.array_equal(drawn, a.sample_actions(obs, seed=124))
    out = np.empty((64, ad), np.float32)   # fql_sample_actions == fql_iql_sample_actions at temperature 1
    assert a._lib.fql_sample_actions(a._h, obs.ctypes.data, 64, z.ctypes.data, 0, out.ctypes.data, None) == 0
    np.testing.assert_array_equal(out, a.sample_actions(obs, noises=z, temperature=1.0))


@pytest.mark.parametrize('const_std', [True, False])
def test_sample_actions_across_the_row_chunk(const_std):
    """n = 4096 + 37 rows: two chunks of the sampling loop, the second one short.  The rows on both sides of the boundary and the last
    row equal their single-observation calls bitwise, and a seeded draw (keyed by the row number of the call) repeats."""
    od, ad, B, H = SMALL
    cfg, _, batch, _, params = _problem(SMALL, 7, const_std=const_std)
    a = _agent(cfg, batch, params=params)
    n = 4096 + 37
    rng = np.random.default_rng(7)
    obs = rng.standard_normal((n, od)).astype(np.float32)
    z = rng.standard_normal((n, ad)).astype(np.float32)
    got = a.sample_actions(obs, noises=z, temperature=1.0)
    assert got.shape == (n, ad) and np.abs(got).max() <= 1.0
    np.testing.assert_allclose(got, _ref(params, cfg, SMALL).sample_actions(obs, z, 1.0), atol=2e-5)
    for row in (4095, 4096, n - 1):
        np.testing.assert_array_equal(got[row], a.sample_actions(obs[row], noises=z[row], temperature=1.0), err_msg=str(row))
    drawn = a.sample_actions(obs, seed=11)
    np.testing.assert_array_equal(drawn, a.sample_actions(obs, seed=11))


def test_checkpoint_round_trip_is_bitwise(tmp_path):
    from fql_amd import checkpoint
    cfg, _, batch, noise, _ = _problem(SMALL, 7, actor_loss='ddpgbc', const_std=False)
    a = _agent(cfg, batch)
    a.update(batch, noise=noise)
    a.update(batch, noise=IO.make_noise(SMALL[2], SMALL[1], 70))
    a.synchronize()
    assert leaf_dict(a.get_params())['modules_actor/log_stds'].all()
    checkpoint.save_agent(a, str(tmp_path), 2)
    b = _agent(cfg, batch, seed=99)
    checkpoint.restore_agent(b, str(tmp_path), 2)
    _same_state(a, b)
    sd = checkpoint.to_state_dict(a)
    assert set(sd['network']['params']) == {'modules_actor', 'modules_critic', 'modules_target_critic', 'modules_value'}
    assert set(sd['network']['params']['modules_actor']) == {'actor_net', 'log_stds', 'mean_net'}
    assert np.shape(sd['network']['params']['modules_actor']['log_stds']) == (SMALL[1],)


def test_iql_interleaved_with_fql_ends_where_it_ends_alone():
    import fql_amd
    from tests.util import make_cfg
    cfg, ds, batch, _, _ = _problem(BIG, 8, actor_loss='awr', const_std=False)
    fcfg = make_cfg((64,) * 4, batch_size=cfg['batch_size'])

    def make():
        f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], fcfg)
        q = _agent(cfg, batch)
        for x in (f, q):
            x.upload_dataset(ds)
        return f, q

    alone = make()
    for x in alone:
        for _ in range(6):
            x.update_from_dataset()
    mixed = make()
    for _ in range(6):
        for x in (mixed[1], mixed[0]):
            x.update_from_dataset()
    for x in alone + mixed:
        x.synchronize()
    for x, y in zip(alone, mixed):
        _same_state(x, y)


def test_stats_agree():
    od, ad, B, H = BIG
    for actor_loss in ('awr', 'ddpgbc'):
        cfg, _, batch, _, _ = _problem(BIG, 0, actor_loss=actor_loss)
        a = _agent(cfg, batch)
        la, ma = a.iql_stats()
        assert la > 0 and a.stats()['launches_per_update'] == la and a.stats()['macs_per_update'] == ma
        cr, va, ac = (od + ad) * H + 3 * H * H + H, od * H + 3 * H * H + H, od * H + 3 * H * H + H * ad
        want = 2 * va + (2 * va - od * H) + 2 * cr + 2 * cr + 2 * (2 * cr - (od + ad) * H) + ac + (2 * ac - od * H)
        if actor_loss == 'ddpgbc':
            want += 4 * cr
        assert ma == want * B


@pytest.mark.parametrize('actor_loss,n', [('awr', 16), ('ddpgbc', 19)])
def test_num_info_and_the_info_calls(actor_loss, n):
    from fql_amd import _cabi
    cfg, _, batch, noise, _ = _problem(SMALL, 13, actor_loss=actor_loss, const_std=False)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    keys = IO.INFO_KEYS[actor_loss]
    assert lib.fql_num_info(h) == n == len(keys) and lib.fql_handle_info_name(h, n) is None
    assert [lib.fql_handle_info_name(h, i).decode() for i in range(n)] == list(keys)
    import fql_amd
    assert fql_amd.IQL_INFO_KEYS[actor_loss] == keys
    _, lazy = a.update(batch, noise=noise)
    assert tuple(lazy) == keys and len(lazy) == n
    vals = lazy.to_dict()
    buf = (C.c_float * n)()
    assert lib.fql_read_info_n(h, buf, n) == 0
    assert [float(x) for x in buf] == [vals[k] for k in keys]
    assert lib.fql_read_info_n(h, buf, n - 1) == _cabi.FQL_E_INVALID
    t = C.c_uint64()
    assert lib.fql_info_enqueue(h, None, C.byref(t)) == 0
    guard = (C.c_float * (n + 1))(*([-7.0] * (n + 1)))
    assert lib.fql_info_wait_n(h, t.value, guard, n + 1) == 0
    assert [float(x) for x in guard[:n]] == [vals[k] for k in keys] and guard[n] == -7.0
    assert lib.fql_info_wait_n(h, t.value, buf, n - 1) == _cabi.FQL_E_INVALID
    b13 = (C.c_float * 13)()
    assert lib.fql_read_info(h, b13) == _cabi.FQL_E_STATE
    assert lib.fql_info_wait(h, t.value, b13) == _cabi.FQL_E_STATE
    assert a.read_info() == vals
    out = (C.c_float * n)()
    bp = [np.ascontiguousarray(batch[k], dtype=np.float32) for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')]
    assert lib.fql_iql_update(h, *[x.ctypes.data for x in bp], cfg['batch_size'], None, out, None) == 0
    assert list(out) == list(a.read_info().values())


def test_refusals_return_documented_codes():
    from fql_amd import _cabi
    import fql_amd
    from tests.util import make_cfg
    od, ad, B, H = BIG
    cfg, ds, batch, noise, _ = _problem(BIG, 9, const_std=False)
    a = _agent(cfg, batch)
    lib, h = a._lib, a._h
    nz = _cabi.FqlNoise()
    st = C.c_size_t * 2
    assert lib.fql_grad_buckets(h, st(), st()) == _cabi.FQL_E_STATE
    obs, act, rew, mask, nobs = (np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                                 ('observations', 'actions', 'rewards', 'masks', 'next_observations'))
    bp = [x.ctypes.data for x in (obs, act, rew, mask, nobs)]
    loss, info = C.c_float(), (C.c_float * 19)()
    assert lib.fql_update(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_total_loss(h, *bp, B, None, C.byref(loss), info, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin(h, *bp, B, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_begin_split(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_end(h, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_end_split(h, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin(h, None, B, 0, 0, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_dataset_begin_split(h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    a.upload_dataset(ds)
    assert lib.fql_update_from_dataset(h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_replay_create(h, 8) == _cabi.FQL_E_STATE   # IQL trains offline: no replay ring, no balanced step
    assert lib.fql_update_balanced(h, None, None, None, B, None, None, None) == _cabi.FQL_E_STATE
    frames = np.zeros((64, 32, 32, 3), np.uint8)
    assert lib.fql_dataset_upload_frames(h, 64, frames.ctypes.data, frames.ctypes.data, ds['actions'][:64].ctypes.data,
                                         ds['rewards'][:64].ctypes.data, ds['masks'][:64].ctypes.data, ds['masks'][:64].ctypes.data,
                                         1, 0.0) == _cabi.FQL_E_STATE
    assert lib.fql_update_from_frames(h, None, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_flow_actions(h, obs.ctypes.data, act.ctypes.data, 4, act.ctypes.data, None) == _cabi.FQL_E_STATE
    for bad in ('x0', 't', 'z', 'eps2'):   # the C ABI reads only eps1 of fql_noise
        other = np.zeros((B, ad), np.float32)
        fields = {'eps1': noise['eps'].ctypes.data, 'x0': None, 't': None, 'z': None, 'eps2': None}
        fields[bad] = other.ctypes.data
        nzb = _cabi.FqlNoise(*[fields[k] for k in ('eps1', 'x0', 't', 'z', 'eps2')])
        assert lib.fql_iql_update(h, *bp, B, C.byref(nzb), None, None) == _cabi.FQL_E_INVALID, bad
    keys = np.zeros(10, dtype=np.uint32)
    assert lib.fql_noise_from_jax_keys(h, keys.ctypes.data, 0, B, C.byref(nz), None) == _cabi.FQL_E_STATE
    grp = C.c_void_p()
    assert lib.fql_group_create((C.c_void_p * 1)(h), 1, C.byref(grp)) == _cabi.FQL_E_STATE
    # the other agents' calls on an IQL handle, and the fql_iql_* calls on an FQL handle
    assert lib.fql_sac_update(h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    f = fql_amd.FQLAgent.create(1, batch['observations'][:1], batch['actions'][:1], make_cfg((64,) * 4, batch_size=B))
    assert lib.fql_iql_update(f._h, *bp, B, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_iql_update_from_dataset(f._h, None, B, 0, 0, None, None, None) == _cabi.FQL_E_STATE
    assert lib.fql_iql_total_loss(f._h, *bp, B, None, C.byref(loss), info, None) == _cabi.FQL_E_STATE
    out = np.empty((1, ad), np.float32)
    assert lib.fql_iql_sample_actions(f._h, obs.ctypes.data, 1, None, 0, 1.0, out.ctypes.data, None) == _cabi.FQL_E_STATE
    la = C.c_int64()
    assert lib.fql_iql_stats(f._h, C.byref(la), None) == _cabi.FQL_E_STATE
    # create-time refusals
    c = _cabi.FqlConfig()
    lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim = od, ad
    qc = _cabi.FqlIqlConfig()
    lib.fql_iql_default_config(C.byref(qc))
    hh = C.c_void_p()
    c.precision = 2
    assert lib.fql_iql_create(C.byref(c), C.byref(qc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    c.precision = 0
    qc.actor_loss = 2
    assert lib.fql_iql_create(C.byref(c), C.byref(qc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    qc.actor_loss = 1
    qc.expectile = 1.0
    assert lib.fql_iql_create(C.byref(c), C.byref(qc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    qc.expectile = 0.9
    c.encoder, c.img_h, c.img_w, c.img_c = 1, 32, 32, 3
    assert lib.fql_iql_create(C.byref(c), C.byref(qc), 0, C.byref(hh)) == _cabi.FQL_E_INVALID
    assert lib.fql_iql_create(C.byref(c), None, 0, C.byref(hh)) == _cabi.FQL_E_INVALID
