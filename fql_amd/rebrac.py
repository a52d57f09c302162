"""Host-side mirror of the reference's ReBRACAgent (agents/rebrac.py) over the C ABI: revisited behavior-regularized actor-critic, TD3+BC
with LayerNorm and separate actor / critic BC penalties.

The update is the TD3-style critic loss with a penalised, noisy target action and, on full steps, the deterministic actor's Q + BC loss
(agents/rebrac.py:26-134).  main.py calls `update(batch, full_update=False)` on every step i with i % actor_freq != 0: a critic-only step
(the actor's gradient is zero, Adam still runs over every leaf, no Polyak).  Same call sites as the reference:

    agent = ReBRACAgent.create(seed, ex_observations, ex_actions, config)
    train_dataset.return_next_actions = True
    agent, info = agent.update(batch, full_update=(i % config['actor_freq'] == 0))   # info: LazyInfo, 12 or 7 keys
    action = agent.sample_actions(observations=ob, seed=key, temperature=1.0)

State observations and fp32 only: `encoder`, precision 'bf16x3' and rng other than 'engine' are refused here, before the library is
called, as are the FQL-only paths (begin / end halves, balanced sampling, compute_flow_actions).  Everything else (datasets,
checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on a ReBRAC handle.
"""
from __future__ import annotations

import ctypes as C

from . import _cabi
from .agent import AgentGroup, KindAgent, LazyInfo, _Arg
from .config import ConfigDict

REBRAC_INFO_KEYS = (
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/total_loss', 'actor/actor_loss', 'actor/bc_loss', 'actor/std', 'actor/mse',
    'grad/max', 'grad/min', 'grad/norm',
)
# a critic-only step (full_update=False): the critic keys, then the grad statistics (slots 0-6 of the info buffer)
REBRAC_CRITIC_INFO_KEYS = REBRAC_INFO_KEYS[:4] + REBRAC_INFO_KEYS[9:]
REBRAC_NOISE_KEYS = ('eps1',)   # the raw N(0, 1) [B, act] of the target-policy noise (agents/rebrac.py:30-34), before actor_noise


def get_config():
    """agents/rebrac.py:222-244 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='rebrac',
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
        tanh_squash=True,
        actor_fc_scale=0.01,
        alpha_actor=0.0,
        alpha_critic=0.0,
        actor_freq=2,
        actor_noise=0.2,
        actor_noise_clip=0.5,
        encoder=None,
        rng='engine',  # not a reference key: device Philox noise (the only source ReBRAC supports)
        precision='fp32',  # not a reference key: ReBRAC runs in fp32 only
    )


class ReBRACAgent(KindAgent):
    """ReBRAC agent backed by the MI355X step engine.  sample_actions (agents/rebrac.py:136-152):
    clip(mode + clip(N(0, 1) actor_noise temperature, +-actor_noise_clip), -1, 1)."""

    _name = 'ReBRAC'
    _refused = (('compute_flow_actions', 'compute_flow_actions (the actor is deterministic)'), ('update_balanced', 'balanced sampling'),
                ('create_replay_buffer', 'a replay ring beside the dataset'))
    _update_fn, _update_dataset_fn, _sample_fn = 'fql_rebrac_update', 'fql_rebrac_update_from_dataset', 'fql_rebrac_sample_actions'
    _loss_infos = 9

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/rebrac.py:154-219.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        cls._refuse_config(cfg)
        cfg.setdefault('flow_steps', 10)   # (an fql_config field ReBRAC does not read)
        lib = _cabi.load()
        c, ob_dims, action_dim = cls._engine_config(lib, cfg, ex_observations, ex_actions)
        rc = _cabi.FqlRebracConfig()
        lib.fql_rebrac_default_config(C.byref(rc))
        rc.alpha_actor, rc.alpha_critic = float(cfg['alpha_actor']), float(cfg['alpha_critic'])
        rc.actor_noise, rc.actor_noise_clip = float(cfg['actor_noise']), float(cfg['actor_noise_clip'])
        rc.tanh_squash, rc.actor_fc_scale = int(bool(cfg['tanh_squash'])), float(cfg['actor_fc_scale'])
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_rebrac_create(C.byref(c), C.byref(rc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        agent = cls(h, cfg, int(seed))
        agent._last_full = True
        return agent

    def _noise_args(self, noise, B):
        """Explicit eps1 [B, act] (agents/rebrac.py:30-34, before scaling); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(REBRAC_NOISE_KEYS)
        if extra:
            raise ValueError(f'ReBRAC reads only {REBRAC_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        eps1 = _Arg(noise.get('eps1'), (B, self.config['action_dim']))
        return _cabi.FqlNoise(eps1.ptr, None, None, None, None), [eps1]

    def _batch_args(self, batch):
        if 'next_actions' not in batch:
            raise KeyError("a ReBRAC batch must carry 'next_actions' (Dataset.return_next_actions = True)")
        B, args = super()._batch_args(batch)
        return B, args + [_Arg(batch['next_actions'], (B, self.config['action_dim']))]

    def _lazy_info(self, stream):
        t = C.c_uint64()
        self._check(self._lib.fql_info_enqueue(self._h, stream, C.byref(t)))
        return LazyInfo(self, int(t.value), REBRAC_INFO_KEYS if self._last_full else REBRAC_CRITIC_INFO_KEYS)

    # -- reference API ----------------------------------------------------------------------
    def update(self, batch, full_update=True, noise=None, want_info=True):
        """agents/rebrac.py:122-134.  Returns (agent, info); info is a LazyInfo with REBRAC_INFO_KEYS (full step) or
        REBRAC_CRITIC_INFO_KEYS (critic-only step), or None with want_info=False."""
        self._last_full = bool(full_update)
        return super().update(batch, noise, want_info, _extra=(int(self._last_full),))

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None, full_update=True):
        """train_dataset.sample(B) (return_next_actions) + update(batch, full_update) without leaving the device."""
        self._last_full = bool(full_update)
        return super().update_from_dataset(batch_size, idxs, noise, shard, want_info, stream, _extra=(int(self._last_full),))

    def read_info(self):
        """The infos of the last update (12 or 7 keys by its kind; blocks until it has run)."""
        buf = (C.c_float * _cabi.FQL_NUM_INFO)()
        self._check(self._lib.fql_read_info(self._h, buf))
        keys = REBRAC_INFO_KEYS if getattr(self, '_last_full', True) else REBRAC_CRITIC_INFO_KEYS
        return {k: float(buf[i]) for i, k in enumerate(keys)}

    def total_loss(self, batch, grad_params=None, rng=None, noise=None, full_update=True):
        """agents/rebrac.py:86-108 with grad_params=None (the validation probe, main.py:284): (loss, info) with 9 infos on a full step,
        the 4 critic infos otherwise.  No state changes."""
        self._probe_guard('total_loss with traced grad_params', grad_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        info = (C.c_float * 10)()
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_rebrac_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None,
                                                    int(bool(full_update)), C.byref(loss), info, stream))
        keys = REBRAC_INFO_KEYS[:9] if full_update else REBRAC_INFO_KEYS[:4]
        return float(loss.value), {k: float(info[i]) for i, k in enumerate(keys)}

    def rebrac_stats(self, full_update=True):
        """(launches, MACs) of one full or critic-only update."""
        la, ma = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_rebrac_stats(self._h, int(bool(full_update)), C.byref(la), C.byref(ma)))
        return int(la.value), int(ma.value)


class ReBRACAgentGroup(AgentGroup):
    """K ReBRAC agents of one structure - the same config except `seed`, `alpha_actor` and `alpha_critic` - advanced by fused update
    programs (include/fql_amd.h, fql_rebrac_group_*): one for the full step, one for the critic-only step, every launch carrying all K
    members' tasks.  The alpha_actor x alpha_critic x seed sweep of the reference's protocol on one device:

        group = ReBRACAgentGroup.create(seeds, ex_obs, ex_act, config, alpha_actors=[...], alpha_critics=[...])
        group.upload_dataset(train_dataset)
        for i in range(1, n + 1):
            infos = group.update_from_dataset(full_update=(i % config['actor_freq'] == 0), want_info=(i % log_every == 0))
        actions = group.sample_actions(observations, seed=i)   # [K, ..., act], one fused call

    `members` are ordinary ReBRACAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same seed,
    alphas, rows and noise.  Members are state agents with precision 'fp32' and the engine's device RNG; while grouped their batch size
    is fixed.  FQL agents are grouped by FQLAgentGroup."""

    _member, _get_config = ReBRACAgent, staticmethod(get_config)
    _create_fn, _update_fn = 'fql_rebrac_group_create', 'fql_rebrac_group_update_from_dataset'
    _sample_fn = 'fql_rebrac_group_sample_actions'
    _stats_fn, _stats_outs = 'fql_rebrac_group_stats', 3   # launches(): (the full program, the critic-only program, one sampling call)

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, alpha_actors=None, alpha_critics=None):
        return cls._create(seeds, config, {'alpha_actor': (alpha_actors, 'alpha_actors'), 'alpha_critic': (alpha_critics, 'alpha_critics')},
                           ex_observations, ex_actions)

    def update_from_dataset(self, batch_size=None, idxs=None, want_info=False, full_update=True):
        """One fused update of every member, full or critic-only: rows from each member's dataset (`idxs` [K, B] int, host or device, or
        None = each member's device RNG) with next_actions = actions[min(idx + 1, size - 1)], noise from each member's device RNG.
        Returns a list of K LazyInfo (want_info; 12 or 7 keys by the step's kind) or None."""
        full = bool(full_update)

        def after(m):
            m._last_full = full
        return self._update(self._batch(batch_size), idxs, want_info, extra=(int(full),), after=after)


__all__ = ['ReBRACAgent', 'ReBRACAgentGroup', 'REBRAC_INFO_KEYS', 'REBRAC_CRITIC_INFO_KEYS', 'REBRAC_NOISE_KEYS', 'get_config']
