"""CPU tests of the IQL-diffusion restatements (tests/iqld_oracle.py, tests/iqld_oracle_torch.py), of the problems the GPU tests run
(tests/iqld_cases.py: every row's distance from the points where the loss weights branch) and of the host-side agent surface."""
import itertools

import numpy as np
import pytest

import fql_amd
from fql_amd import iql_diffusion as dmod
from oracle import fql_oracle as O
from tests import iqld_cases as K
from tests import iqld_oracle as DO
from tests import iqld_oracle_torch as DT

OD, AD, B, S = 7, 3, 16, 4
VARIANTS = list(itertools.product(dmod.OPTIMAL_VARS, (0, 1)))


def _problem(ov='binary_awr_loss', te=1, ln=1, hidden=(12, 10), seed=0):
    cfg = DO.get_config()
    cfg.update(actor_hidden_dims=hidden, hidden_dims=hidden, denoise_steps=S, use_layer_norm=ln, batch_size=B, optimal_var=ov,
               target_extraction=te)
    params = DO.init_params(seed, OD, AD, cfg, np.float64)
    rng = np.random.default_rng(seed + 1)
    for _, v in O.tree_leaves_with_path(params):
        v += 0.1 * rng.standard_normal(v.shape)
    for name in ('critic', 'target_critic'):   # a wide critic: advantages of O(1), away from 0
        params[name]['value_net'][f"Dense_{len(hidden)}"]['kernel'] *= 4.0
    batch = DO.make_batch(OD, AD, B, seed + 2)
    batch = {k: np.asarray(v, np.float64) for k, v in batch.items()}
    ref = DO.center_value(DO.OracleIQLD(params, cfg, OD, AD, np.float64), batch)
    cfg['awr_temperature'] = K.awr_temperature(ref.adv(batch)[0])
    ref.config = dict(cfg)
    m = K.check_margins(ref, batch)
    assert m['adv'] >= 1e-2   # finite differences move the advantages by ~1e-6: far from a weight's branch
    return cfg, ref.params, batch, DO.make_noise(B, AD, S, seed + 3)


@pytest.mark.parametrize('ov,te', VARIANTS)
def test_numpy_equals_torch(ov, te):
    cfg, params, batch, noise = _problem(ov, te)
    a, b = DO.OracleIQLD(params, cfg, OD, AD, np.float64), DT.TorchIQLD(params, cfg)
    ga, info = a.grads(batch, noise)
    lb, gb = b.grads(batch, noise)
    for net, la in (('critic', info['critic_loss']), ('value', info['value_loss']), ('actor', info['actor_loss'])):
        assert abs(la - lb[net]) <= 1e-9 * max(1.0, abs(la)), net
        tb = DT.leaves(gb[net])
        for p, v in O.tree_leaves_with_path(ga[net]):
            np.testing.assert_allclose(v, tb[p], rtol=1e-9, atol=1e-12, err_msg=f'{net}/{p}')
    _, extra = b.actor_loss(batch, noise, b.params['actor'])
    for k, v in extra.items():   # the reference's jnp.sort form of the top-10 mass
        assert abs(info[k] - v) <= 1e-9 * max(1.0, abs(v)), k
    sn = np.random.default_rng(9).standard_normal((5, AD))
    for cs in (0.0, 1.0, 3.0):
        np.testing.assert_allclose(a.sample_actions(batch['observations'][:5], sn, cs), b.sample_actions(batch['observations'][:5], sn, cs), atol=1e-9)
    assert a.sample_actions(batch['observations'][0], sn[0]).shape == (AD,) == a.sample_actions(batch['observations'][:1], sn[:1]).shape


@pytest.mark.parametrize('ov,te', VARIANTS)
def test_finite_differences_on_every_leaf(ov, te):
    """Each net's gradient against central differences of ITS loss, the other uses of every parameter held at their stored values (the
    reference's params=None calls are constants under jax.grad): every leaf, and every element of both embedding rows."""
    cfg, params, batch, noise = _problem(ov, te, hidden=(6, 5))
    ref = DO.OracleIQLD(params, cfg, OD, AD, np.float64)
    ref.frozen = O.tree_map(np.copy, ref.params)
    g, _ = ref.grads(batch, noise)
    loss = {'critic': lambda: ref.critic_part(batch, False)[0], 'value': lambda: ref.value_part(batch, False)[0],
            'actor': lambda: ref.actor_part(batch, noise, False)[0]}
    rng = np.random.default_rng(4)
    for net in DO.TRAINED:
        gl = dict(O.tree_leaves_with_path(g[net]))
        for p, v in O.tree_leaves_with_path(ref.params[net]):
            picks = list(np.ndindex(v.shape)) if p == 'Embed_0/embedding' else [tuple(rng.integers(0, s) for s in v.shape) for _ in range(3)]
            for i in picks:
                old, h = v[i], 1e-6
                v[i] = old + h
                lp = loss[net]()
                v[i] = old - h
                lm = loss[net]()
                v[i] = old
                fd = (lp - lm) / (2 * h)
                assert abs(fd - gl[p][i]) <= 1e-6 * max(1.0, abs(fd)) + 1e-8, (net, p, i, fd, gl[p][i])
    assert np.abs(g['actor']['Embed_0']['embedding']).min() > 0


@pytest.mark.parametrize('ov,te', VARIANTS)
def test_stacked_pass_equals_two_passes(ov, te):
    cfg, params, batch, noise = _problem(ov, te)
    ref = DO.OracleIQLD(params, cfg, OD, AD, np.float64)
    l1, info, _ = ref.actor_part(batch, noise, False)
    l2, rows = ref.actor_loss_two_passes(batch, noise)
    assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
    np.testing.assert_allclose(info['actor_losses'], rows, rtol=1e-12, atol=1e-14)
    assert abs(info['actor_loss'] - (info['actor_loss_positive'] + 0.1 * info['actor_loss_uncond'])) <= 1e-12


@pytest.mark.parametrize('n', [16, 256])
def test_top_10_mass_by_rank_agrees_with_sort_ties_included(n):
    rng = np.random.default_rng(n)
    assert int(0.1 * n) == (1 if n == 16 else 25)
    cases = [rng.uniform(0, 100, n), np.minimum(np.exp(rng.normal(0, 3, n)), 100.0) * (rng.uniform(size=n) > 0.5),   # zeros and 100-caps tie
             (rng.uniform(size=n) > 0.5).astype(np.float64), np.ones(n), np.zeros(n), np.repeat(rng.uniform(size=n // 4), 4)]
    for w in cases:
        for dt in (np.float64, np.float32):
            w = w.astype(dt)
            assert abs(float(DO.top_mass_by_rank(w)) - float(DO.top_mass(w))) <= 4 * np.finfo(dt).eps * max(1.0, float(DO.top_mass(w)))
    assert DO.top_mass(np.ones(5)) == pytest.approx(1.0)   # int(0.1 n) == 0: sorted[-0:] is every element
    assert DO.top_mass_by_rank(np.ones(5)) == pytest.approx(1.0)


def test_info_key_order_per_step_kind_is_the_merge_order():
    """{**critic_info, **value_info, **actor_info} with grad/* appended to each by apply_loss_fn: a later dict overwrites the VALUES of
    grad/* and leaves them where the first dict inserted them."""
    crit, val = ['critic_loss', 'q'], ['value_loss', 'v', 'v_min', 'v_max']
    act = ['actor_q', 'actor_loss', 'actor_positive_ratio', 'actor_loss_positive', 'actor_loss_uncond', 'actor_losses', 'o_mean', 'o_std',
           'o_min', 'o_max', 'o', 'effective_batch_size', 'loss_weights_top_10_mass', 'loss_weights_max', 'loss_weights']
    grad = ['grad/max', 'grad/min', 'grad/norm']

    def merged(uc, ua):
        ci = dict.fromkeys(crit + grad, 'critic') if uc else {}
        vi = dict.fromkeys(val + grad, 'value') if uc else {}
        ai = dict.fromkeys(act + grad, 'actor') if ua else {}
        return {**ci, **vi, **ai}
    for uc, ua in itertools.product((True, False), repeat=2):
        m = merged(uc, ua)
        assert list(m) == list(dmod.info_keys(uc, ua))
        if uc or ua:
            assert m['grad/max'] == ('actor' if ua else 'value')   # never the critic's
    assert dmod.info_keys(False, False) == ()
    assert list(dmod.info_keys(True, True, grads=False)) == crit + val + act
    assert set(dmod.info_keys(True, True)) - set(dmod.IQLD_ROW_KEYS) == set(dmod.IQLD_INFO_KEYS) and len(dmod.IQLD_INFO_KEYS) == 21
    cfg, params, batch, noise = _problem()
    ref = DO.OracleIQLD(params, cfg, OD, AD, np.float64)
    for uc, ua in itertools.product((True, False), repeat=2):
        assert tuple(ref.update(batch, noise, uc, ua)) == dmod.info_keys(uc, ua)
    assert ref.counts == {'critic': 2, 'actor': 2} and ref.updates == 4


def test_step_kinds_touch_only_their_nets():
    cfg, params, batch, noise = _problem()
    ref = DO.OracleIQLD(params, cfg, OD, AD, np.float64)
    p0 = O.tree_map(np.copy, ref.params)
    ref.update(batch, noise, True, False)
    same = lambda a, b: all(np.array_equal(x, y) for (_, x), (_, y) in zip(O.tree_leaves_with_path(a), O.tree_leaves_with_path(b)))   # noqa: E731
    assert same(ref.params['actor'], p0['actor']) and not same(ref.params['critic'], p0['critic']) and not same(ref.params['value'], p0['value'])
    assert not same(ref.params['target_critic'], p0['target_critic'])
    p1 = O.tree_map(np.copy, ref.params)
    ref.update(batch, noise, False, True)
    assert not same(ref.params['actor'], p1['actor']) and all(same(ref.params[n], p1[n]) for n in ('critic', 'value', 'target_critic'))
    p2 = O.tree_map(np.copy, ref.params)
    assert ref.update(batch, noise, False, False) == {} and all(same(ref.params[n], p2[n]) for n in p2) and ref.updates == 3


def test_critic_loss_is_half_of_the_member_sum_and_q_is_member_0():
    cfg, params, batch, noise = _problem()
    ref = DO.OracleIQLD(params, cfg, OD, AD, np.float64)
    loss, info, _ = ref.critic_part(batch, False)
    q = ref._critic('critic', batch['observations'], batch['actions'])
    y = batch['rewards'] + cfg['discount'] * batch['masks'] * ref._value(batch['next_observations'])
    assert abs(loss - 0.5 * np.mean((q[0] - y) ** 2 + (q[1] - y) ** 2)) <= 1e-12 * abs(loss)
    assert info['q'] == q[0].mean() and abs(q[0].mean() - q.mean()) > 1e-6


@pytest.mark.parametrize('name', sorted(K.all_cases()))
def test_every_gpu_case_keeps_its_margins(name):
    """|adv| >= 1e-3 and |adv T - ln 100| >= 1e-3 for every row, rows on both sides of adv = 0, a row at the 100 cap (binary_awr_loss)."""
    c = K.all_cases()[name]
    cfg, params, batch, noise, ref = K.build(c)
    m = K.check_margins(ref, batch, name)
    assert m['positive'] >= 1 and m['negative'] >= 1
    if name == 'step-kinds':   # the batches of the step-kind sequence, the gradient-statistics step and the total_loss probe
        for i, (uc, ua) in enumerate([(True, False), (False, True), (False, False), (True, True), (False, True), (True, False)]):
            b, nz = K.data(c, seed=500 + i)
            K.check_margins(ref, b, (name, i))
            ref.update(b, nz, uc, ua)
        K.check_margins(ref, K.data(c, seed=520)[0], (name, 520))
        ref2 = K.build(c)[4]
        ref2.update(batch, noise)
        K.check_margins(ref2, K.data(c, seed=530)[0], (name, 530))
    if name == 'switch-64':   # one agent through the three batch sizes
        for c2 in K.SWITCH:
            b, nz = K.data(c2)
            K.check_margins(ref, b, (name, c2['B']))
            ref.update(b, nz)
    if name in K.PATH_STEPS:   # the full update, then the critic-only and the actor-only step on fresh rows
        ref.update(batch, noise)
        for s, (uc, ua) in zip(K.PATH_STEPS[name], ((True, False), (False, True))):
            b, nz = K.data(c, seed=s)
            K.check_margins(ref, b, (name, s))
            ref.update(b, nz, uc, ua)
        assert ref.counts == {'critic': 2, 'actor': 2}
    if name in ('walk512', 'walk64'):   # one agent through the batch sizes of the walk
        walk = K.WALK512 if name == 'walk512' else K.WALK64
        assert [c2['B'] for c2 in walk] == ([256, 1024, 272, 256] if name == 'walk512' else [64, 2064, 64])
        for c2 in walk:
            b, nz = K.data(c2)
            assert b['observations'].shape[0] == c2['B']
            K.check_margins(ref, b, (name, c2['B']))
            ref.update(b, nz)
    if name == 'trajectory':
        for i in range(100):
            b, nz = K.data(c, seed=7000 + i)
            K.check_margins(ref, b, (name, i))
            ref.update(b, nz, *K.trajectory_kind(i))
        assert ref.counts['critic'] > 50 and ref.counts['actor'] > 50 and ref.updates == 100


def test_path_cases_take_the_sizes_they_are_named_for():
    """The top-10 count int(0.1 B) per case, the padded widths behind the case names, and b2064-binary's ties: every positive row
    weighs 1, so the top-10 mass is 206 / (positive rows) only if exactly 206 of the tied rows are taken."""
    pad16, pad64 = (lambda x: (x + 15) // 16 * 16), (lambda x: (x + 63) // 64 * 64)
    assert {n: int(0.1 * c['B']) for n, c in K.PATHS.items()} == {'humanoidmaze': 25, 'act16': 25, 'b1024': 102, 'b272': 27, 'b2064-awr': 206,
                                                                 'b2064-binary': 206, 'wide1024': 4, 'ragged': 3}
    h, a = K.PATHS['humanoidmaze'], K.PATHS['act16']
    assert pad16(h['ad']) == 32 and pad64(h['od'] + h['ad'] + 16 + DO.EMBED) == 192 and pad16(a['ad']) == a['ad'] == 16
    assert all(2 * K.PATHS[n]['B'] == m for n, m in (('b1024', 2048), ('b272', 544), ('b2064-awr', 4128), ('b2064-binary', 4128)))
    assert 544 % 64 and 4128 % 64 and 2064 % 64 and 272 % 256 == 16 and 2064 % 256 == 16   # 16-row kernels; strided tails of 16 rows
    cfg, params, batch, noise, ref = K.build(K.PATHS['b2064-binary'])
    info = ref.actor_part(batch, noise, False)[1]
    w = info['loss_weights']
    pos = int((w == 1).sum())
    assert pos > 206 and set(np.unique(w)) == {0.0, 1.0}
    assert abs(info['loss_weights_top_10_mass'] - 206 / pos) <= 1e-9 and abs(DO.top_mass_by_rank(w) - 206 / pos) <= 1e-9
    # a tie-break that counts a row against itself (j <= b) takes the wrong number of tied rows: the mass would move by >= 1 / pos
    assert 1 / pos > 10 * (5e-6 + 5e-5 * 206 / pos)


def test_fp32_rounding_of_the_cfg_sampler():
    """What fp32 arithmetic alone does to sample_actions on the GPU test's inputs: with the head scaled by 2 (the GPU test's scale) the fp32
    numpy restatement stays within 1.2e-5 of fp64 for cfg 0, 1 and 3 (measured: 1.9e-6, 1.7e-6, 8.8e-6 at n = 256), inside the 2e-5 the
    GPU test allows; guidance amplifies the rounding (cfg 3 carries 3 v_pos - 2 v_unc), and at a head scale of 6 fp32 numpy itself leaves
    the bound."""
    obs, sn = K.sampler_inputs(256)
    worst = {}
    for scale in (K.SAMPLER_HEAD_SCALE, 6.0):
        cfg, params, _ = K.sampler_problem(scale)
        r64, r32 = DO.OracleIQLD(params, cfg, K.OD, K.AD, np.float64), DO.OracleIQLD(params, cfg, K.OD, K.AD, np.float32)
        for cs in (0.0, 1.0, 3.0):
            a64 = r64.sample_actions(obs, sn, cs)
            worst[scale, cs] = float(np.abs(r32.sample_actions(obs, sn, cs).astype(np.float64) - a64).max())
            if scale == K.SAMPLER_HEAD_SCALE:
                assert 0.2 < (np.abs(a64) == 1).mean() < 0.9   # the clip is reached
    print(worst)
    assert all(worst[K.SAMPLER_HEAD_SCALE, cs] <= 1.2e-5 for cs in (0.0, 1.0, 3.0)), worst
    assert worst[6.0, 3.0] > 2e-5, worst


def test_fp32_rounding_of_the_cfg_sampler_at_hidden_512():
    """The inputs of tests/test_gpu_iqld.py::test_sample_actions_at_hidden_512_and_padded_action_width_32 (obs 69, act 21, hidden 512,
    head scaled by K.SAMPLER512_HEAD_SCALE, n = 1, 37, 2049, cfg 0 and 3): fp32 numpy stays within 5e-6 of fp64 (measured 2.5e-6 at
    n 2049 / cfg 3, 1.0e-6 at cfg 0), a quarter of the 2e-5 the GPU test allows, and the clip is reached (38 % of the coordinates)."""
    c = K.SAMPLER512
    cfg, params, _ = K.sampler_problem(K.SAMPLER512_HEAD_SCALE, c)
    r64, r32 = DO.OracleIQLD(params, cfg, c['od'], c['ad'], np.float64), DO.OracleIQLD(params, cfg, c['od'], c['ad'], np.float32)
    worst = {}
    for n in K.SAMPLER512_N:
        obs, sn = K.sampler_inputs(n, c['od'], c['ad'])
        assert obs.shape == (n, 69) and sn.shape == (n, 21)
        for cs in (0.0, 3.0):
            a64 = r64.sample_actions(obs, sn, cs)
            a32 = r32.sample_actions(obs, sn, cs)
            assert a32.dtype == np.float32
            worst[n, cs] = float(np.abs(a32.astype(np.float64) - a64).max())
            assert (np.abs(a64) == 1).any(), (n, cs)
            if n > 1:
                assert 0.2 < (np.abs(a64) == 1).mean() < 0.9
    print(worst)
    assert max(worst.values()) <= 5e-6, worst


def test_embedding_init_fan_and_statistics():
    """flax's variance_scaling(1, fan_in, normal, out_axis=0) on [2, 32]: in_axis = -2 and out_axis = 0 both name axis 0, so the
    receptive field is 64 / (2 * 2) = 16 and fan_in = 2 * 16 = 32: N(0, 1 / 32)."""
    shape = (2, 32)
    in_size, out_size = shape[-2], shape[0]
    receptive = np.prod(shape) / in_size / out_size
    assert in_size * receptive == 32 == DO.EMBED
    cfg = dict(DO.get_config(), actor_hidden_dims=(8,), hidden_dims=(8,))
    em = np.stack([DO.init_params(s, OD, AD, cfg)['actor']['Embed_0']['embedding'] for s in range(64)])
    assert abs(em.var() * 32 - 1.0) < 0.1 and abs(em.mean()) < 4.0 / np.sqrt(32 * em.size)


def test_registry_config_and_host_refusals():
    assert fql_amd.agents['iql_diffusion'] is fql_amd.IQLDiffusionAgent
    cfg = dmod.get_config()
    ref = DO.get_config()
    for k, v in ref.items():
        assert cfg[k] == v, k
    assert cfg['optimal_var'] == 'binary_awr_loss' and cfg['target_extraction'] == 1 and cfg['denoise_steps'] == 16
    assert cfg['actor_lr'] == cfg['value_lr'] == cfg['critic_lr'] == 3e-4 and cfg['awr_temperature'] == 0.1 and cfg['softmax_beta'] == 3.0
    ex = (np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32))
    for kw in (dict(optimal_var='softmax'), dict(optimal_var='sampled_adv_softmax'), dict(opt_decay_schedule='cosine'),
               dict(encoder='impala_small'), dict(precision='bf16x3'), dict(activation='relu'), dict(rng='jax'), dict(goal_conditioned=1)):
        with pytest.raises(NotImplementedError) as e:
            fql_amd.IQLDiffusionAgent.create(0, *ex, kw)
        assert any(word in str(e.value) for word in (list(kw)[0], str(list(kw.values())[0]), 'encoder', 'goal')), str(e.value)
    with pytest.raises(ValueError):
        fql_amd.IQLDiffusionAgent.create(0, *ex, dict(optimal_var='quadratic'))


def test_create_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present: tests/test_gpu_iqld.py creates agents')
    with pytest.raises(RuntimeError):
        fql_amd.IQLDiffusionAgent.create(0, np.zeros((1, OD), np.float32), np.zeros((1, AD), np.float32), dict(batch_size=16))
