"""Host-side mirror of the reference's IQLAgent (agents/iql.py) over the C ABI: implicit Q-learning with an expectile value, a critic
pair with a Polyak target and a plain Gaussian actor trained by AWR or by DDPG+BC.  Same call sites as the reference:

    agent = IQLAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch)                      # info: LazyInfo with 16 (awr) or 19 (ddpgbc) keys
    action = agent.sample_actions(observations=ob, seed=key, temperature=1.0)

State observations and fp32 only: `encoder`, precision 'bf16x3', JAX-key noise, compute_flow_actions, the data-parallel begin / end
halves, gradient buckets and the replay ring are refused here, before the library is called.  Everything else (datasets,
checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on an IQL handle.

IQLAgentGroup advances K such agents - one config but for seed, expectile and alpha - with one fused update program and samples them
in one fused call (fql_iql_group_*).
"""
from __future__ import annotations

import ctypes as C

from . import _cabi
from .agent import AgentGroup, KindAgent, _Arg, _PendingN
from .config import ConfigDict

_IQL_HEAD_KEYS = (
    'value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
)
_GRAD_KEYS = ('grad/max', 'grad/min', 'grad/norm')
IQL_AWR_INFO_KEYS = _IQL_HEAD_KEYS + ('actor/actor_loss', 'actor/adv', 'actor/bc_log_prob', 'actor/mse', 'actor/std') + _GRAD_KEYS
IQL_DDPGBC_INFO_KEYS = _IQL_HEAD_KEYS + ('actor/actor_loss', 'actor/q_loss', 'actor/bc_loss', 'actor/q_mean', 'actor/q_abs_mean',
                                         'actor/bc_log_prob', 'actor/mse', 'actor/std') + _GRAD_KEYS
IQL_INFO_KEYS = {'awr': IQL_AWR_INFO_KEYS, 'ddpgbc': IQL_DDPGBC_INFO_KEYS}
# eps: the raw N(0, 1) [B, act] of dist.sample in the ddpgbc loss with const_std=False (agents/iql.py:89); unused otherwise
IQL_NOISE_KEYS = ('eps',)


def get_config():
    """agents/iql.py:242-261 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='iql',
        ob_dims=None,  # set automatically by create()
        action_dim=None,  # set automatically by create()
        lr=3e-4,
        batch_size=256,
        actor_hidden_dims=(512, 512, 512, 512),
        value_hidden_dims=(512, 512, 512, 512),
        layer_norm=True,
        actor_layer_norm=False,
        discount=0.99,
        tau=0.005,
        expectile=0.9,
        actor_loss='ddpgbc',
        alpha=1.0,
        const_std=True,
        encoder=None,
        rng='engine',  # not a reference key: device Philox noise or explicit tensors (the only sources IQL supports)
        precision='fp32',  # not a reference key: IQL runs in fp32 only
    )


class IQLAgent(KindAgent):
    """Implicit Q-learning agent backed by the MI355X step engine.  update: agents/iql.py update, 16 (awr) or 19 (ddpgbc) infos;
    sample_actions: clip(mean + exp(log_stds) temperature N(0, 1), -1, 1)."""

    _name = 'IQL'
    _modules = {'critic': 'pair', 'target_critic': 'pair', 'value': 'value'}
    _refused = (('compute_flow_actions', 'compute_flow_actions (the actor is a Gaussian, there is no flow)'),
                ('update_balanced', 'balanced sampling (IQL trains offline from one dataset)'))
    _update_fn, _update_dataset_fn, _sample_fn = 'fql_iql_update', 'fql_iql_update_from_dataset', 'fql_iql_sample_actions'
    _pending_cls = _PendingN

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/iql.py:171-239.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        cls._refuse_config(cfg)
        lib = _cabi.load()
        fcfg = ConfigDict(cfg)
        fcfg.update(alpha=0.0, flow_steps=10, q_agg='min')   # fql_config fields IQL does not read (its alpha travels in fql_iql_config)
        c, ob_dims, action_dim = cls._engine_config(lib, fcfg, ex_observations, ex_actions)
        qc = _cabi.FqlIqlConfig()
        lib.fql_iql_default_config(C.byref(qc))
        qc.expectile, qc.alpha = float(cfg['expectile']), float(cfg['alpha'])
        qc.actor_loss, qc.const_std = int(cfg['actor_loss'] == 'ddpgbc'), int(bool(cfg['const_std']))
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_iql_create(C.byref(c), C.byref(qc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        return cls(h, cfg, int(seed))

    @classmethod
    def _refuse_config(cls, cfg):
        """encoder, precision, rng (NotImplementedError) and an unknown actor_loss (ValueError), before any library call."""
        super()._refuse_config(cfg)
        if cfg['actor_loss'] not in IQL_INFO_KEYS:
            raise ValueError(f"Unsupported actor loss: {cfg['actor_loss']}")

    @property
    def _loss_infos(self):
        return len(self._info_keys) - 3

    def _noise_args(self, noise, B):
        """Explicit eps [B, act] (raw N(0, 1)); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(IQL_NOISE_KEYS)
        if extra:
            raise ValueError(f'IQL reads only {IQL_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        e = _Arg(noise.get('eps'), (B, self.config['action_dim']))
        return _cabi.FqlNoise(e.ptr, None, None, None, None), [e]

    def total_loss(self, batch, grad_params=None, rng=None, noise=None):
        """agents/iql.py total_loss with grad_params=None (the validation probe, main.py:284): (loss, info) with the value, critic and
        actor infos.  No state changes."""
        self._probe_guard('total_loss with traced grad_params', grad_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        n = self._loss_infos
        info = (C.c_float * n)()
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_iql_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, C.byref(loss), info,
                                                 stream))
        return float(loss.value), {k: float(info[i]) for i, k in enumerate(self._info_keys[:n])}

    def iql_stats(self):
        """(launches, MACs) of one update."""
        la, ma = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_iql_stats(self._h, C.byref(la), C.byref(ma)))
        return int(la.value), int(ma.value)


class IQLAgentGroup(AgentGroup):
    """K IQL agents of one structure - the same config except `seed`, `expectile` and `alpha` - advanced by ONE fused update program
    (include/fql_amd.h, fql_iql_group_*): every launch of the update carries all K members' tasks.  The alpha x expectile x seed sweep
    every table of the reference's papers runs for this baseline, on one device:

        group = IQLAgentGroup.create(seeds, ex_obs, ex_act, config, alphas=[...], expectiles=[...])
        group.upload_dataset(train_dataset)
        for i in range(1, n + 1):
            infos = group.update_from_dataset(want_info=(i % log_every == 0))
        actions = group.sample_actions(observations, seed=i, temperature=0.0)   # [K, ..., act], one fused call

    `members` are ordinary IQLAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same seed,
    expectile, alpha, rows and noise.  `actor_loss` and `const_std` are the group's: they choose the kernels of the update.  Members are
    state agents with precision 'fp32' and the engine's device RNG; while grouped their batch size is fixed.  FQL agents are grouped by
    FQLAgentGroup, ReBRAC agents by ReBRACAgentGroup, IQL-diffusion agents by IQLDiffusionAgentGroup, IFQL agents by IFQLAgentGroup."""

    _member, _get_config = IQLAgent, staticmethod(get_config)
    _create_fn, _update_fn = 'fql_iql_group_create', 'fql_iql_group_update_from_dataset'
    _sample_fn, _stats_fn = 'fql_iql_group_sample_actions', 'fql_iql_group_stats'   # launches(): (the update program, one sampling call)

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, expectiles=None, alphas=None):
        return cls._create(seeds, config, {'expectile': (expectiles, 'expectiles'), 'alpha': (alphas, 'alphas')}, ex_observations, ex_actions)


__all__ = ['IQLAgent', 'IQLAgentGroup', 'IQL_INFO_KEYS', 'IQL_AWR_INFO_KEYS', 'IQL_DDPGBC_INFO_KEYS', 'IQL_NOISE_KEYS', 'get_config']
