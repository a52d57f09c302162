"""Host-side mirror of the reference's IFQLAgent (agents/ifql.py) over the C ABI: implicit flow Q-learning, the flow variant of IDQL.

The update is the IQL value / critic pair plus flow-matching BC of actor_flow (agents/ifql.py:25-120); sample_actions is best-of-N: for each
observation `num_samples` noises through the Euler flow, clipped, scored by min(q1, q2) of the critic, first argmax kept (:123-155).
Same call sites as the reference:

    agent = IFQLAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch)                      # info: LazyInfo with IFQL_INFO_KEYS
    action = agent.sample_actions(observations=ob, seed=key)

State observations and fp32 only: `encoder`, precision 'bf16x3' and rng other than 'engine' are refused here, before the library is called.
Everything else (datasets, checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on an IFQL handle.
"""
from __future__ import annotations

import ctypes as C

from . import _cabi
from .agent import FQLAgent
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
