"""GPU: Adam, the Polyak target update, the gradient statistics and the counters past the first update, element by element against the
fp64 oracles at bounds measured on the CPU (tests/test_optimizer_cpu.py; MEASUREMENTS.md "Optimizer stage").

The one-call update cannot be handed a gradient, so every case here starts from carried moments (optimizer_cases.carried_moments: mixed
sign, half of them nearly cancelling 0.1 g; nu0 at least the leaf's largest squared gradient, so that the step does not amplify the
gradient's own error) at a count past the first, and is compared with the kind's oracle continued from the same state (tests/util.py
sync_restatement): FQL on the `ragged` (widths (80, 48, 64)) and `h512` (64-chunk leaves) cases at counts 9, 999 and 10^6 and gradient
scales 1 and 0.5, on the engine's own queues and, bitwise equal, as a captured graph; a checkpoint restore in mid-run; group members at
different counts; one step each of IFQL, SAC, CFGRL, ReBRAC and IQL-diffusion at count 999.  build_leaves makes segments with
chunk_w > 0 (one Adam chunk per padded row) for SAC's two actor heads only: test_sac_carries_moments covers that segment kind.

The injected route (a crafted gradient written into the flat gradient buffer between update_begin and update_end; layout,
crafted_gradient and crafted_moments of tests/optimizer_cases.py, exercised on the CPU) has no GPU test here: inside a run of the whole
GPU suite its first update_begin ended the process with a segmentation fault whose cause was not found.  MEASUREMENTS.md has the record.
"""
import numpy as np
import pytest
import torch

from oracle import fql_oracle as O
from tests import optimizer_cases as C
from tests.util import leaf_dict, randomize_params

pytestmark = pytest.mark.gpu


def _create(case, cfg, batch):
    import fql_amd
    return fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)


def _read(agent):
    opt = agent.get_opt_state()
    return dict(params=leaf_dict(agent.get_params()), mu=leaf_dict(opt['mu']), nu=leaf_dict(opt['nu']), count=opt['count'], step=opt['step'],
                info=agent.read_info())


# ------------------------------------------------------------------------------------------------
# the fused update past the first step
# ------------------------------------------------------------------------------------------------
def _tree_state(mu0, nu0, count):
    return {'mu': C.unflatten(mu0), 'nu': C.unflatten(nu0), 'count': count, 'step': count + 1}


def _cuda(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items() if k != 'terminals'}


@pytest.mark.parametrize('scale', C.SCALES)
@pytest.mark.parametrize('count', C.FUSED_COUNTS)
@pytest.mark.parametrize('case', ['ragged', 'h512'])
def test_fused_update_past_the_first_step(case, count, scale):
    """One fql_update from carried moments at `count`, on the engine's own queues, against the fp64 oracle continued from the same state:
    every element of the parameter step, mu, nu and the target (the two-range Adam launch of the critic and the BC flow, the one-step
    actor's launch, the gradient scale); then the same update as a captured graph on a caller's stream, bitwise equal."""
    from tests.util import assert_info_close, assert_same_state, sync_restatement
    cfg, batch, noise, od, ad = C.case_problem(case)
    a, b = _create(case, cfg, batch), _create(case, cfg, batch)
    params = randomize_params(a.get_params(), seed=3)
    ref = O.OracleFQL(params, dict(cfg), od, ad, np.float64)
    g0 = C.trainable(ref.grads(batch, noise)[2])
    if case == 'h512':                               # an unpadded 512 x 512 kernel is 64 Adam chunks of 4096: the finalize fold's quarters of 16
        assert g0['modules_actor_bc_flow/mlp/Dense_1/kernel'].shape == (512, 512)
    mu0, nu0 = C.carried_moments(21, g0, count, scale)
    for g, v in zip(g0.values(), nu0.values()):      # sqrt(nu0 / c2) >= max |g_leaf| s
        assert np.sqrt(v.astype(np.float64).min() / (1 - C.B2 ** (count + 1))) >= np.abs(g).max() * scale * (1 - 1e-6)
    for x in (a, b):
        x.set_params(params)
        x.set_opt_state(_tree_state(mu0, nu0, count))
        x.set_grad_scale(scale)
    sync_restatement(ref, a)
    assert ref.count == count and ref.step == count + 1
    pre = _read(a)
    a.update(batch, noise=noise)
    assert a.synchronize() == 'aql'                      # the engine's own queues
    post = _read(a)
    info_ref, g = C.oracle_update(ref, batch, noise, scale)
    ref_post = dict(params=leaf_dict(ref.params), mu=leaf_dict(ref.mu), nu=leaf_dict(ref.nu))
    gmax = {p: max(float(np.abs(v).max()), 1e-6 * scale) for p, v in g.items()}
    worst = C.fused_step_errors(pre, post, pre, ref_post, gmax, cfg['lr'], cfg['tau'])
    print(case, count, scale, {k: f'{e:.2e}' for k, (e, _) in worst.items()})
    for k, (e, p) in worst.items():
        assert e <= C.BOUNDS_FUSED[k], (k, e, C.BOUNDS_FUSED[k], p)
    assert set(worst) == {'mu', 'nu', 'p', 'target'}
    assert_info_close(post['info'], info_ref, rtol=5e-5, atol=5e-6)
    assert post['count'] == count + 1 and post['step'] == count + 2
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.update(_cuda(batch), noise=_cuda(noise))
    assert b.synchronize() == 'graph'                    # a captured graph on the caller's stream
    torch.cuda.synchronize()
    assert_same_state(a, b)
    assert a.read_info() == b.read_info()
    a.close(); b.close()


@pytest.mark.parametrize('count', [997, 999_997])
def test_restored_agent_continues_bitwise(tmp_path, count):
    """Three updates from `count`; a second agent restored from the checkpoint taken after the second takes the third: bitwise the same
    state.  The running b1pow / b2pow are products, the restored ones std::pow (at 999 997 both have underflowed to 0; at 997 they have
    not)."""
    from fql_amd import checkpoint
    from tests.util import assert_same_state
    cfg, batch, noise, od, ad = C.case_problem('ragged')
    a = _create('ragged', cfg, batch)
    params = randomize_params(a.get_params(), seed=3)
    g0 = C.trainable(O.OracleFQL(params, dict(cfg), od, ad, np.float64).grads(batch, noise)[2])
    mu0, nu0 = C.carried_moments(22, g0, count)
    a.set_params(params)
    a.set_opt_state(_tree_state(mu0, nu0, count))
    b = None
    for k in range(3):
        nz = O.make_noise(batch['actions'].shape[0], ad, 50 + k)
        a.update(batch, noise=nz)
        if k == 1:
            checkpoint.save_agent(a, str(tmp_path), 2)
            b = checkpoint.restore_agent(_create('ragged', cfg, batch), str(tmp_path), 2)
            assert b.get_opt_state()['count'] == count + 2
        if k == 2:
            b.update(batch, noise=nz)
    assert a.get_opt_state()['count'] == count + 3
    assert_same_state(a, b)
    assert a.read_info() == b.read_info()
    a.close(); b.close()


def test_group_members_at_different_counts_equal_their_twins():
    """Three members with crafted moments at counts 1, 9 and 999 (per-member counters in the fused Adam and finalize launches), two
    updates on explicit rows: each bitwise where the same agent trained alone ends."""
    from tests.test_gpu_group import _assert_same_state, _setup
    od, ad, B, hidden = C.STATE_CASES['ragged']
    cfg, ds, batch, noise, group, twins = _setup(3, B, hidden, od=od, ad=ad)
    for i, count in enumerate((1, 9, 999)):
        ref = O.OracleFQL(twins[i].get_params(), dict(cfg, alpha=10.0 * (i + 1)), od, ad, np.float64)   # (_setup's alphas)
        mu0, nu0 = C.carried_moments(40 + i, C.trainable(ref.grads(batch, noise)[2]), count)
        for x in (group.members[i], twins[i]):
            x.set_opt_state(_tree_state(mu0, nu0, count))
    idxs = np.random.default_rng(5).integers(0, len(ds['observations']), size=(2, 3, B))
    for s in range(2):
        group.update_from_dataset(idxs=idxs[s])
        for i, t in enumerate(twins):
            t.update_from_dataset(B, idxs=idxs[s][i])
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        assert m.get_opt_state()['count'] == (1, 9, 999)[i] + 2
        assert all(np.isfinite(v) for v in m.read_info().values()), m.read_info()
        _assert_same_state(m, t, f'member {i}')
    group.close()


# ------------------------------------------------------------------------------------------------
# the other kinds: moments carried at count 999 through the kind's own oracle, hidden 64, B 64
# ------------------------------------------------------------------------------------------------
def _state_of(a):
    opt = a.get_opt_state()
    return dict(params=leaf_dict(a.get_params()), mu=leaf_dict(opt['mu']), nu=leaf_dict(opt['nu']), opt=opt)


def _ref_state(ref):
    return dict(params=leaf_dict(ref.params), mu=leaf_dict(ref.mu), nu=leaf_dict(ref.nu))


def _carried(seed, g_tree, count):
    """Carried moments for the leaves of a gradient tree that are trained (no target leaf)."""
    g = {p: v for p, v in leaf_dict(g_tree).items() if 'target' not in p}
    return g, C.carried_moments(seed, g, count)


def _check_kind_step(pre, post, ref_post, g, lr, tau, target_of, what):
    gmax = {p: max(float(np.abs(v).max()), 1e-6) for p, v in g.items()}
    worst = C.fused_step_errors(pre, post, pre, ref_post, gmax, lr, tau, target_of)
    print(what, {k: f'{e:.2e} {p}' for k, (e, p) in worst.items()})
    for k, (e, p) in worst.items():
        assert e <= C.BOUNDS_FUSED[k], (what, k, e, C.BOUNDS_FUSED[k], p)
    return worst


def _modules_target(paths):
    def target_of(p):
        head, rest = p.split('/', 1)
        t = head.replace('modules_', 'modules_target_', 1) + '/' + rest
        return t if t in paths else None
    return target_of


def test_ifql_carries_moments():
    """IFQL: its all-chunk Adam launch, three trained modules."""
    from tests import test_gpu_ifql as T
    from tests.util import sync_restatement
    cfg, _, batch, noise = T._problem(64, 64, seed=1)
    a = T._agent(cfg, batch)
    params = T._randomized(a.get_params(), 5)
    a.set_params(params)
    ref = T.IO.OracleIFQL(params, dict(cfg), T.OD, T.AD, np.float64)
    g, (mu0, nu0) = _carried(61, ref.grads(batch, noise)[2], 999)
    a.set_opt_state(_tree_state(mu0, nu0, 999))
    sync_restatement(ref, a)
    pre = _state_of(a)
    a.update(batch, noise=noise)
    a.synchronize()
    ref.update(batch, noise)
    post = _state_of(a)
    assert post['opt']['count'] == 1000 and post['opt']['step'] == 1001
    w = _check_kind_step(pre, post, _ref_state(ref), g, cfg['lr'], cfg['tau'], _modules_target(set(pre['params'])), 'ifql')
    assert set(w) == {'mu', 'nu', 'p', 'target'} and any(p.startswith('modules_value/') for p in g)
    a.close()


def test_sac_carries_moments():
    """SAC: the one-element temperature leaf modules_alpha/log_value, and the two actor heads, whose segments have chunk_w > 0 (one
    Adam chunk per padded row of the [H, 2 ap] last layer)."""
    from tests import test_gpu_sac as T
    from tests.util import sync_restatement
    cfg, _, batch, noise = T._problem(64, 64, seed=1, tanh_squash=True, backup_entropy=False, q_agg='min')
    a = T._agent(cfg, batch)
    params = T._randomized(a.get_params(), 5)
    a.set_params(params)
    ref = T.SO.OracleSAC(params, dict(cfg), T.OD, T.AD, np.float64)
    g, (mu0, nu0) = _carried(62, ref._losses(batch, noise, want_grads=True)[2], 999)
    assert g['modules_alpha/log_value'].size == 1 and {'modules_actor/mean_net/kernel', 'modules_actor/log_std_net/kernel'} <= set(g)
    a.set_opt_state(_tree_state(mu0, nu0, 999))
    sync_restatement(ref, a)
    pre = _state_of(a)
    a.update(batch, noise=noise)
    a.synchronize()
    ref.update(batch, noise)
    post = _state_of(a)
    assert post['opt']['count'] == 1000 and post['opt']['step'] == 1001
    w = _check_kind_step(pre, post, _ref_state(ref), g, cfg['lr'], cfg['tau'], _modules_target(set(pre['params'])), 'sac')
    assert set(w) == {'mu', 'nu', 'p', 'target'}
    a.close()


def test_cfgrl_carries_moments():
    """CFGRL: the [1, G] embedding leaf behind the flow actor's."""
    from tests import test_gpu_cfgrl as T
    from tests.util import sync_restatement
    cfg = T._cfg(64, 64)
    batch, noise, mask = T._data(T.OD, T.AD, T.GD, 64, seed=1)
    a = T._agent(cfg)
    params = T._randomized(a.get_params(), 5)
    a.set_params(params)
    ref = T.CO.OracleCFGRL(params, dict(cfg), T.OD, T.AD, T.GD, np.float64)
    g, (mu0, nu0) = _carried(63, ref.grads(batch, noise, mask)[2], 999)
    assert g[T.EMB].shape == (1, T.GD) and np.abs(g[T.EMB]).max() > 0
    a.set_opt_state(_tree_state(mu0, nu0, 999))
    sync_restatement(ref, a)
    pre = _state_of(a)
    a.update(batch, noise=noise, do_cfg=mask)
    a.synchronize()
    ref.update(batch, noise, mask)
    post = _state_of(a)
    assert post['opt']['count'] == 1000 and post['opt']['step'] == 1001
    w = _check_kind_step(pre, post, _ref_state(ref), g, cfg['lr'], 0.0, lambda p: None, 'cfgrl')
    assert set(w) == {'mu', 'nu', 'p'}
    a.close()


def test_rebrac_critic_only_step_decays_the_actor():
    """ReBRAC at count 999.  A critic-only step hands optax a zero gradient for the actor (agents/rebrac.py:105-107, 122-134): Adam still
    decays the actor's moments and moves its parameters by the momentum (tests/test_gpu_rebrac.py asserts that it moves); here every
    element of that step is held to the bound, the critic's beside it, and both targets stay bitwise.  The full step after it moves both
    modules and both targets within the bound."""
    from tests import test_gpu_rebrac as T
    from tests.util import sync_restatement
    cfg, _, batch, noise = T._problem(64, 64, seed=1)
    a = T._agent(cfg, batch)
    params = T._randomized(a.get_params(), 5)
    a.set_params(params)
    ref = T.RO.OracleReBRAC(params, dict(cfg), T.OD, T.AD, np.float64)
    _, (mu0, nu0) = _carried(64, ref._losses(batch, noise, want_grads=True, full_update=True)[2], 999)
    a.set_opt_state(_tree_state(mu0, nu0, 999))
    target_of = _modules_target(set(leaf_dict(params)))
    # critic only
    sync_restatement(ref, a)
    pre = _state_of(a)
    g = {p: v for p, v in leaf_dict(ref._losses(batch, noise, want_grads=True, full_update=False)[2]).items() if 'target' not in p}
    assert all(not v.any() for p, v in g.items() if p.startswith('modules_actor/')) and any(p.startswith('modules_actor/') for p in g)
    a.update(batch, full_update=False, noise=noise)
    a.synchronize()
    ref.update(batch, noise, full_update=False)
    post = _state_of(a)
    for p in pre['params']:
        if p.startswith('modules_target_'):
            np.testing.assert_array_equal(post['params'][p], pre['params'][p], err_msg=p)
    assert any(np.any(post['params'][p] != pre['params'][p]) for p in g if p.startswith('modules_actor/'))
    assert post['opt']['count'] == 1000
    w = _check_kind_step(pre, post, _ref_state(ref), g, cfg['lr'], cfg['tau'], lambda p: None, 'rebrac critic-only')
    assert set(w) == {'mu', 'nu', 'p'}
    # full
    noise2 = T.RO.make_noise(64, T.AD, 77)
    sync_restatement(ref, a)
    pre = post
    g = {p: v for p, v in leaf_dict(ref._losses(batch, noise2, want_grads=True, full_update=True)[2]).items() if 'target' not in p}
    a.update(batch, full_update=True, noise=noise2)
    a.synchronize()
    ref.update(batch, noise2, full_update=True)
    post = _state_of(a)
    assert post['opt']['count'] == 1001
    w = _check_kind_step(pre, post, _ref_state(ref), g, cfg['lr'], cfg['tau'], target_of, 'rebrac full')
    assert set(w) == {'mu', 'nu', 'p', 'target'} and any(np.abs(v).max() > 0 for p, v in g.items() if p.startswith('modules_actor/'))
    assert any(np.any(post['params'][p] != pre['params'][p]) for p in pre['params'] if p.startswith('modules_target_actor/'))
    a.close()


def test_iqld_restored_counter_blocks():
    """IQL-diffusion restored through the checkpoint layer with the critic's count at 1000 and the actor's at 400 (the second counter
    block, which fql_set_step does not write): a step that updates both meets the bound on both blocks."""
    from fql_amd import checkpoint
    from tests import test_gpu_iqld as T
    cfg, params, batch, noise, ref, a = T._built(T.K.FIRST[sorted(T.K.FIRST)[0]])
    g_ref, _ = ref.grads(batch, noise, True, True)
    counts = {'actor': 400, 'critic': 1000, 'value': 1000}
    state = checkpoint.to_state_dict(a)
    g, lr = {}, {}
    for net in T.NETS:
        gn, (mu0, nu0) = _carried(70, g_ref[net], counts[net])
        state[net]['step'] = np.int64(counts[net] + 1)
        state[net]['opt_state'] = {'0': {'count': np.int32(counts[net]), 'mu': C.unflatten(mu0), 'nu': C.unflatten(nu0)}, '1': {}}
        g.update({f'{net}/{p}': v for p, v in gn.items()})
        lr.update({f'{net}/{p}': cfg[T.DO.LR_KEY[net]] for p in gn})
    checkpoint.from_state_dict(a, state)
    opt = a.get_opt_state()
    assert opt['count'] == 1000 and opt['actor_count'] == 400
    T.DO.sync(ref, a)
    T.K.check_margins(ref, batch)
    pre = _state_of(a)
    a.update(batch, update_critic=True, update_actor=True, noise=noise)
    a.synchronize()
    ref.update(batch, noise, True, True)
    post = _state_of(a)
    assert post['opt']['count'] == 1001 and post['opt']['actor_count'] == 401
    target_of = lambda p: 'target_' + p if p.startswith('critic/') else None   # noqa: E731
    w = _check_kind_step(pre, post, _ref_state(ref), g, lr, cfg['tau'], target_of, 'iqld')
    assert set(w) == {'mu', 'nu', 'p', 'target'} and {p.split('/')[0] for p in g} == set(T.NETS)
    a.close()
