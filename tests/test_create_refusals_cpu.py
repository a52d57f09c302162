"""CPU: every refusal of a kind's create call, by its whole fql_last_error text.

create_engine validates the common fields it refuses per kind (encoder, precision) and the kind's own config before it looks for a
device, so each text can be read on a machine without a GPU.  One case per refusal of the seven kinds that have a config struct, plus
encoder = 1, precision = 2 and a NULL kind config for each; and one valid config per kind, which answers FQL_E_NODEVICE without a
device and FQL_OK (the handle is destroyed) with one."""
import ctypes as C
import math

import pytest

INF, NAN = math.inf, math.nan
GEOM = ('actor_geom_sample = True is not available: the geometric offset is a ceil of a ratio of logarithms, which the device\'s '
        'log and numpy\'s may round to different integers (uniform trajectory goals only)')
SOFTMAX = ('optimal_var \'softmax\' / \'sampled_adv_softmax\' (the continuous policy with an external bc_agent) is not available: '
           'the binary family only (0 binary, 1 binary_awr_loss, 2 binary_softmax_loss)')
# kind -> (create call, default-config call, config struct, name in messages, name of the NULL argument, [(broken fields, refusal)])
KINDS = {
    'ifql': ('fql_ifql_create', 'fql_ifql_default_config', 'FqlIfqlConfig', 'IFQL', 'icfg', [
        (dict(expectile=2.0), 'expectile must be in (0, 1)'),
        (dict(num_samples=0), 'num_samples must be in [1, 4096]')]),
    'rebrac': ('fql_rebrac_create', 'fql_rebrac_default_config', 'FqlRebracConfig', 'ReBRAC', 'rcfg', [
        (dict(actor_noise=-1.0), 'actor_noise and actor_noise_clip must be >= 0'),
        (dict(actor_fc_scale=0.0), 'actor_fc_scale must be > 0'),
        (dict(alpha_actor=INF), 'alpha_actor and alpha_critic must be finite'),
        (dict(tanh_squash=2), 'tanh_squash must be 0 or 1')]),
    'sac': ('fql_sac_create', 'fql_sac_default_config', 'FqlSacConfig', 'SAC', 'scfg', [
        (dict(state_dependent_std=0), 'only state_dependent_std = 1 is available (the const_std=False vector form is not)'),
        (dict(tanh_squash=2), 'tanh_squash must be 0 or 1'),
        (dict(actor_fc_scale=0.0), 'actor_fc_scale must be > 0'),
        (dict(target_entropy=INF), 'target_entropy must be finite or NaN (automatic)'),
        (dict(target_entropy=NAN, target_entropy_multiplier=INF), 'target_entropy_multiplier must be finite')]),
    'bc': ('fql_bc_create', 'fql_bc_default_config', 'FqlBcConfig', 'BC', 'bcfg', [
        (dict(denoise_steps=0), 'denoise_steps must be in [1, 1024]')]),
    'iql': ('fql_iql_create', 'fql_iql_default_config', 'FqlIqlConfig', 'IQL', 'qcfg', [
        (dict(expectile=2.0), 'expectile must be in (0, 1)'),
        (dict(alpha=INF), 'alpha must be finite'),
        (dict(actor_loss=2), 'actor_loss must be 0 (awr) or 1 (ddpgbc)'),
        (dict(const_std=2), 'const_std must be 0 or 1')]),
    'iqld': ('fql_iqld_create', 'fql_iqld_default_config', 'FqlIqldConfig', 'IQL-diffusion', 'dcfg', [
        (dict(optimal_var=3), SOFTMAX),
        (dict(optimal_var=5), 'optimal_var must be 0 (binary), 1 (binary_awr_loss) or 2 (binary_softmax_loss)'),
        (dict(opt_decay_schedule=1), 'opt_decay_schedule \'cosine\' is not available (a constant actor_lr only)'),
        (dict(expectile=0.0), 'expectile must be in (0, 1)'),
        (dict(value_lr=0.0), 'actor_lr, value_lr and critic_lr must be > 0'),
        (dict(softmax_beta=INF), 'awr_temperature and softmax_beta must be finite'),
        (dict(target_extraction=2), 'target_extraction must be 0 or 1'),
        (dict(denoise_steps=1025), 'denoise_steps must be in [1, 1024]')]),
    'cfgrl': ('fql_cfgrl_create', 'fql_cfgrl_default_config', 'FqlCfgrlConfig', 'CFGRL', 'gcfg', [
        (dict(actor_geom_sample=1), GEOM),
        (dict(goal_dim=0), 'goal_dim must be in [1, 1024] (layer 0 is obs + goal_dim + act + 1 wide)'),
        (dict(flow_steps=0), 'flow_steps must be in [1, 1024]'),
        (dict(cfg=INF), 'cfg must be finite'),
        (dict(p_uncond=2.0), 'p_uncond must be in [0, 1]'),
        (dict(actor_p_trajgoal=0.5), 'actor_p_curgoal + actor_p_trajgoal + actor_p_randomgoal must be 1, each >= 0')]),
}
# (kind, fields of fql_config, fields of the kind's config or None for a NULL one, the whole text)
CASES = []
for _k, (_create, _, _, _name, _arg, _refusals) in KINDS.items():
    CASES += [(_k, {}, broken, f'{_create}: {text}') for broken, text in _refusals]
    CASES += [(_k, dict(encoder=1), {}, f'{_create}: visual encoders are not available for {_name} (encoder must be 0)'),
              (_k, dict(precision=2), {}, f'{_create}: {_name} runs in fp32 only (precision must be 0)'),
              (_k, {}, None, f'{_arg} must not be NULL')]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def configs(lib, kind, common=(), broken=()):
    """The kind's default config over obs 5, act 3 (CFGRL: goal 4), hidden 32 x 4, batch 16, with the given fields overwritten."""
    from fql_amd import _cabi
    c = _cabi.FqlConfig()
    lib.fql_default_config(C.byref(c))
    c.obs_dim, c.act_dim, c.batch_size = 5, 3, 16
    for i in range(4):
        c.actor_hidden[i] = c.value_hidden[i] = 32
    k = getattr(_cabi, KINDS[kind][2])()
    getattr(lib, KINDS[kind][1])(C.byref(k))
    if kind == 'cfgrl':
        k.goal_dim = 4
    for name, v in dict(common).items():
        setattr(c, name, v)
    for name, v in dict(broken).items():
        setattr(k, name, v)
    return c, k


def test_case_counts():
    assert {k: len(v[5]) for k, v in KINDS.items()} == dict(ifql=2, rebrac=4, sac=5, bc=1, iql=4, iqld=8, cfgrl=6)
    assert len(CASES) == 30 + 3 * 7


@pytest.mark.parametrize('kind,common,broken,text', CASES, ids=[f'{c[0]}-{i}' for i, c in enumerate(CASES)])
def test_create_refuses_with_the_whole_text(lib, kind, common, broken, text):
    from fql_amd import _cabi
    c, k = configs(lib, kind, common, broken or {})
    h = C.c_void_p(1)
    rc = getattr(lib, KINDS[kind][0])(C.byref(c), C.byref(k) if broken is not None else None, 0, C.byref(h))
    assert rc == _cabi.FQL_E_INVALID
    assert not h.value
    assert lib.fql_last_error(None).decode() == text


@pytest.mark.parametrize('kind', list(KINDS))
def test_valid_config_reaches_the_device(lib, kind):
    import torch
    from fql_amd import _cabi
    c, k = configs(lib, kind)
    h = C.c_void_p()
    rc = getattr(lib, KINDS[kind][0])(C.byref(c), C.byref(k), 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == _cabi.FQL_OK, lib.fql_last_error(None)
        assert lib.fql_destroy(h) == _cabi.FQL_OK
    else:
        assert rc == _cabi.FQL_E_NODEVICE
        assert not h.value
        assert lib.fql_last_error(None).decode() == 'no HIP device visible: the FQL engine has no CPU fallback'
