"""Host-side mirror of the reference's IFQLAgent (agents/ifql.py) over the C ABI: implicit flow Q-learning, the flow variant of IDQL.

The update is the IQL value / critic pair plus flow-matching BC of actor_flow (agents/ifql.py:25-120); sample_actions is best-of-N: for each
observation `num_samples` noises through the Euler flow, clipped, scored by min(q1, q2) of the critic, first argmax kept (:123-155).
Same call sites as the reference:

    agent = IFQLAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch)                      # info: LazyInfo with IFQL_INFO_KEYS
    action = agent.sample_actions(observations=ob, seed=key)

State observations and fp32 only: `encoder`, precision 'bf16x3' and rng other than 'engine' are refused here, before the library is called.
Everything else (datasets, checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on an IFQL handle.

IFQLAgentGroup advances K such agents - one config but for seed and expectile - with one fused update program and samples them,
best of N, in one fused call (fql_ifql_group_*).
"""
from __future__ import annotations

import ctypes as C

from . import _cabi
from .agent import AgentGroup, FQLAgent
from .config import ConfigDict

IFQL_INFO_KEYS = (
    'value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm',
)
IFQL_NOISE_KEYS = ('x0', 't')


def get_config():
    """agents/ifql.py:231-250 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='ifql',
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
        num_samples=32,
        flow_steps=10,
        encoder=None,
        rng='engine',  # not a reference key: device Philox noise (the only source IFQL supports)
        precision='fp32',  # not a reference key: IFQL runs in fp32 only
    )


class IFQLAgent(FQLAgent):
    """Implicit flow Q-learning agent backed by the MI355X step engine."""

    _name = 'IFQL'
    _modules = {'critic': 'pair', 'target_critic': 'pair', 'value': 'value', 'actor_flow': 'field_t'}
    _loss_infos = 9
    _jax_sample_noise = False

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/ifql.py:157-228.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        cls._refuse_config(cfg)
        lib = _cabi.load()
        c, ob_dims, action_dim = cls._engine_config(lib, cfg, ex_observations, ex_actions)
        ic = _cabi.FqlIfqlConfig()
        lib.fql_ifql_default_config(C.byref(ic))
        ic.expectile, ic.num_samples = float(cfg['expectile']), int(cfg['num_samples'])
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_ifql_create(C.byref(c), C.byref(ic), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        return cls(h, cfg, int(seed))

    def _noise_args(self, noise, B):
        """Explicit x0 [B, act] and t [B] (agents/ifql.py:64-66); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(IFQL_NOISE_KEYS)
        if extra:
            raise ValueError(f'IFQL reads only {IFQL_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        from .agent import _Arg
        ad = self.config['action_dim']
        x0, t = _Arg(noise.get('x0'), (B, ad)), _Arg(noise.get('t'), (B,))
        return _cabi.FqlNoise(None, x0.ptr, t.ptr, None, None), [x0, t]

    def _sample_noise_shape(self, n, flow):
        ad = self.config['action_dim']
        return (n, ad) if flow else (n, int(self.config['num_samples']), ad)

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """agents/ifql.py:123-155: best of `num_samples` flow samples by min(q1, q2).  [od] -> [act]; [n, od] -> [n, act] (row by row the
        single-observation result).  `noises`: [num_samples, act] for one observation, [n, num_samples, act] for n; None = engine RNG keyed
        by `seed`.  `temperature` is accepted and ignored, as in the reference."""
        return self._eval(observations, noises, seed, flow=False)


class IFQLAgentGroup(AgentGroup):
    """K IFQL agents of one structure - the same config except `seed` and `expectile` - advanced by ONE fused update program
    (include/fql_amd.h, fql_ifql_group_*): every launch of the update carries all K members' tasks.  The seeds of one task, or an
    expectile x seed sweep, on one device:

        group = IFQLAgentGroup.create(seeds, ex_obs, ex_act, config, expectiles=[...])
        group.upload_dataset(train_dataset)
        for i in range(1, n + 1):
            infos = group.update_from_dataset(want_info=(i % log_every == 0))
        actions = group.sample_actions(observations, seed=i)   # [K, ..., act], one fused best-of-N call

    `members` are ordinary IFQLAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same seed,
    expectile, rows and noise.  Members are state agents with precision 'fp32' and the engine's device RNG; while grouped their batch
    size is fixed.  FQL agents are grouped by FQLAgentGroup, ReBRAC agents by ReBRACAgentGroup, IQL-diffusion agents by
    IQLDiffusionAgentGroup."""

    _member, _get_config = IFQLAgent, staticmethod(get_config)
    _create_fn, _update_fn = 'fql_ifql_group_create', 'fql_ifql_group_update_from_dataset'
    _sample_fn, _flow_fn, _sample_temperature = 'fql_ifql_group_sample_actions', 'fql_ifql_group_flow_actions', False
    _stats_fn, _stats_outs = 'fql_ifql_group_stats', 3   # launches(): (the update program, one best-of-N call, one flow call)

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, expectiles=None):
        return cls._create(seeds, config, {'expectile': (expectiles, 'expectiles')}, ex_observations, ex_actions)

    def _noise_per(self):   # best of N: noises [K, ..., num_samples, ad]
        return (int(self.members[0].config['num_samples']),)

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """IFQLAgent.sample_actions of every member - best of `num_samples` - in ONE fused call (fql_ifql_group_sample_actions):
        result[i] is bitwise what members[i].sample_actions(observations[i], seed=..., noises=noises[i]) returns.  Shapes and seeds as in
        FQLAgentGroup.sample_actions: observations [K, ..., od] or one shared block, noises [K, ..., num_samples, ad] or None, seed None
        (each member's own counter advances), one seed or K seeds.  `temperature` is accepted and ignored, as in IFQLAgent.  Returns
        [K, ..., ad]."""
        return super().sample_actions(observations, seed, temperature, noises)

    def compute_flow_actions(self, observations, noises):
        """IFQLAgent.compute_flow_actions of every member in one fused call (fql_ifql_group_flow_actions): noises [K, ..., ad]."""
        return self._flow_actions(observations, noises)


__all__ = ['IFQLAgent', 'IFQLAgentGroup', 'IFQL_INFO_KEYS', 'IFQL_NOISE_KEYS', 'get_config']
