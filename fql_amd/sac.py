"""Host-side mirror of the reference's SACAgent (agents/sac.py) over the C ABI: soft actor-critic with a squashed Gaussian actor and a
learned temperature.  RLPD is this agent run online from an empty replay ring with balanced sampling
(main.py --offline_steps=0 --online_steps=1000000 --agent=agents/sac.py --balanced_sampling=1):

    agent = SACAgent.create(seed, ex_observations, ex_actions, config)
    agent.upload_dataset(train_dataset)          # the offline half of every balanced batch
    agent.create_replay_buffer(size)             # starts empty
    action = agent.sample_actions(observations=ob, seed=key, temperature=1.0)
    agent.add_transition(dict(observations=ob, actions=action, rewards=r, masks=m, next_observations=nob), replay=True)
    agent, info = agent.update_balanced(batch_size)   # concat(dataset.sample(B / 2), replay.sample(B / 2)) -> update; 14 keys

State observations and fp32 only: `encoder`, precision 'bf16x3', JAX-key noise, compute_flow_actions, the data-parallel begin / end
halves and gradient buckets are refused here, before the library is called.  Everything else (datasets, the replay
ring, checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on a SAC handle.

SACAgentGroup advances K such agents - one config but for seed and target_entropy - with one fused update program, offline or with
RLPD's balanced batches out of each member's own replay ring, and samples them in one fused call (fql_sac_group_*).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _cabi
from .agent import AgentGroup, KindAgent, _Arg, _PendingN
from .config import ConfigDict

SAC_INFO_KEYS = (
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/total_loss', 'actor/actor_loss', 'actor/alpha_loss', 'actor/alpha', 'actor/entropy', 'actor/std', 'actor/q',
    'grad/max', 'grad/min', 'grad/norm',
)
# eps1: the raw N(0, 1) [B, act] of the next-observation actions of the critic loss (agents/sac.py:27); eps2: of the actor loss's
# actions (agents/sac.py:62)
SAC_NOISE_KEYS = ('eps1', 'eps2')


def get_config():
    """agents/sac.py get_config (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='sac',
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
        target_entropy=None,
        target_entropy_multiplier=0.5,
        tanh_squash=True,
        state_dependent_std=True,
        actor_fc_scale=0.01,
        q_agg='min',
        backup_entropy=False,
        encoder=None,
        rng='engine',  # not a reference key: device Philox noise or explicit tensors (the only sources SAC supports)
        precision='fp32',  # not a reference key: SAC runs in fp32 only
    )


class SACAgent(KindAgent):
    """SAC agent (RLPD's learner) backed by the MI355X step engine.  update: agents/sac.py update, 14 infos (SAC_INFO_KEYS);
    sample_actions: clip(tanh(mean + exp(log_std) temperature N(0, 1)), -1, 1)."""

    _name = 'SAC'
    _refused = (('compute_flow_actions', 'compute_flow_actions (the actor is a Gaussian, there is no flow)'),)
    _update_fn, _update_dataset_fn, _sample_fn = 'fql_sac_update', 'fql_sac_update_from_dataset', 'fql_sac_sample_actions'
    _loss_infos = 11
    _pending_cls = _PendingN

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/sac.py create.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        cls._refuse_config(cfg)
        cfg.setdefault('flow_steps', 10)   # (an fql_config field SAC does not read)
        lib = _cabi.load()
        c, ob_dims, action_dim = cls._engine_config(lib, cfg, ex_observations, ex_actions)
        sc = _cabi.FqlSacConfig()
        lib.fql_sac_default_config(C.byref(sc))
        sc.target_entropy = math.nan if cfg['target_entropy'] is None else float(cfg['target_entropy'])
        sc.target_entropy_multiplier = float(cfg['target_entropy_multiplier'])
        sc.tanh_squash, sc.state_dependent_std = int(bool(cfg['tanh_squash'])), 1
        sc.actor_fc_scale, sc.backup_entropy = float(cfg['actor_fc_scale']), int(bool(cfg['backup_entropy']))
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_sac_create(C.byref(c), C.byref(sc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        if cfg['target_entropy'] is None:   # sac.py create: -target_entropy_multiplier * action_dim
            cfg['target_entropy'] = -cfg['target_entropy_multiplier'] * action_dim
        return cls(h, cfg, int(seed))

    @classmethod
    def _refuse_config(cls, cfg):
        """encoder, precision, rng and state_dependent_std=False (NotImplementedError), before any library call."""
        super()._refuse_config(cfg)
        if not cfg['state_dependent_std']:
            raise NotImplementedError('SAC: only state_dependent_std=True is available')

    def _noise_args(self, noise, B):
        """Explicit eps1 / eps2 [B, act] (raw N(0, 1)); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(SAC_NOISE_KEYS)
        if extra:
            raise ValueError(f'SAC reads only {SAC_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        ad = self.config['action_dim']
        e1, e2 = _Arg(noise.get('eps1'), (B, ad)), _Arg(noise.get('eps2'), (B, ad))
        return _cabi.FqlNoise(e1.ptr, None, None, None, e2.ptr), [e1, e2]

    def update_balanced(self, batch_size=None, idxs=None, noise=None, want_info=False, stream=None):
        """RLPD's step (main.py:255-259) on the device: concat(train_dataset.sample(B // 2), replay_buffer.sample(B // 2)) -> update.
        `idxs` = (dataset_idxs, replay_idxs), B // 2 each, or None (engine RNG)."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        ia = ib = None
        keep = None
        if idxs is not None:
            ka, ia = self._host_idx(idxs[0], B // 2, self.dataset_size()[0], 'dataset idxs')
            kb, ib = self._host_idx(idxs[1], B // 2, self.replay_size()[0], 'replay idxs')
            keep = (ka, kb)
        self._check(self._lib.fql_sac_update_balanced(self._h, ia, ib, B, C.byref(nz) if nz else None, None, stream))
        self._keep = (keep, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    def total_loss(self, batch, grad_params=None, rng=None, noise=None):
        """agents/sac.py total_loss with grad_params=None (the validation probe, main.py:284): (loss, info) with the 11 critic and
        actor infos.  No state changes."""
        self._probe_guard('total_loss with traced grad_params', grad_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        info = (C.c_float * 11)()
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_sac_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, C.byref(loss), info,
                                                 stream))
        return float(loss.value), {k: float(info[i]) for i, k in enumerate(SAC_INFO_KEYS[:11])}

    def sac_stats(self):
        """(launches, MACs) of one update."""
        la, ma = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_sac_stats(self._h, C.byref(la), C.byref(ma)))
        return int(la.value), int(ma.value)


class SACAgentGroup(AgentGroup):
    """K SAC agents of one structure - the same config except `seed` and `target_entropy` - advanced by ONE fused update program
    (include/fql_amd.h, fql_sac_group_*): every launch of the update carries all K members' tasks.  The seeds of an RLPD run on one
    device:

        group = SACAgentGroup.create(seeds, ex_obs, ex_act, config)
        group.upload_dataset(train_dataset)          # the offline half of every member's balanced batch
        group.create_replay_buffers(size)            # K rings, each member's own, empty
        actions = group.sample_actions(obs, seed=i)  # obs [K, od]: one fused call for the K environments
        group.add_transitions(transitions)           # K dicts, one insert per member
        infos = group.update_balanced(want_info=(i % log_every == 0))

    `members` are ordinary SACAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same seed,
    target_entropy, rows and noise.  `tanh_squash`, `backup_entropy`, `q_agg` and every width are the group's.  Members are state agents
    with precision 'fp32' and the engine's device RNG; while grouped their batch size is fixed.  Ring inserts are not fused: a member's
    ring is filled through the member."""

    _member, _get_config = SACAgent, staticmethod(get_config)
    _create_fn, _update_fn, _balanced_fn = 'fql_sac_group_create', 'fql_sac_group_update_from_dataset', 'fql_sac_group_update_balanced'
    _sample_fn, _stats_fn = 'fql_sac_group_sample_actions', 'fql_sac_group_stats'   # launches(): (the update program, one sampling call)

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, target_entropies=None):
        tes = None if target_entropies is None else [None if t is None else float(t) for t in target_entropies]   # (None: automatic)
        return cls._create(seeds, config, {'target_entropy': (tes, 'target_entropies', lambda t: t)}, ex_observations, ex_actions)

    def create_replay_buffers(self, capacity):
        """Every member gets its own empty replay ring of `capacity` rows (SACAgent.create_replay_buffer)."""
        for m in self.members:
            m.create_replay_buffer(capacity)

    def add_transitions(self, transitions):
        """One transition per member into the member's own replay ring: K dicts, K inserts (inserts are not fused)."""
        if len(transitions) != len(self.members):
            raise ValueError(f'{len(self.members)} members but {len(transitions)} transitions')
        for m, t in zip(self.members, transitions):
            m.add_transition(t, replay=True)

    def update_balanced(self, batch_size=None, idxs=None, want_info=False):
        """RLPD's step for every member in one fused update (fql_sac_group_update_balanced): member i trains on concat(its
        dataset.sample(B // 2), its replay ring.sample(B // 2)).  `idxs` = (dataset_idxs [K, B // 2], replay_idxs [K, B // 2]), host or
        device, or None = each member's device RNG.  Returns as update_from_dataset."""
        return self._update(self._batch(batch_size), idxs, want_info, balanced=True)


__all__ = ['SACAgent', 'SACAgentGroup', 'SAC_INFO_KEYS', 'SAC_NOISE_KEYS', 'get_config']
