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

import numpy as np

from . import _cabi
from .agent import FQLAgent, LazyInfo, _Arg, _seed_to_u64
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


class ReBRACAgent(FQLAgent):
    """ReBRAC agent backed by the MI355X step engine."""

    _loss_infos = 9
    _jax_sample_noise = False

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/rebrac.py:154-219.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        if cfg.get('encoder') is not None:
            raise NotImplementedError('ReBRAC: visual encoders are not available (state observations only)')
        if cfg.get('precision', 'fp32') not in ('fp32', 0):
            raise NotImplementedError(f"ReBRAC runs in fp32 only (precision {cfg['precision']!r})")
        if cfg.get('rng', 'engine') != 'engine':
            raise NotImplementedError(f"ReBRAC draws its noise from the engine's RNG or explicit tensors only (rng {cfg['rng']!r})")
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

    def _rebrac_batch(self, batch):
        if 'next_actions' not in batch:
            raise KeyError("a ReBRAC batch must carry 'next_actions' (Dataset.return_next_actions = True)")
        B, args = self._batch_args(batch)
        return B, args + [_Arg(batch['next_actions'], (B, self.config['action_dim']))]

    def _info(self, stream, full_update):
        t = C.c_uint64()
        self._check(self._lib.fql_info_enqueue(self._h, stream, C.byref(t)))
        return LazyInfo(self, int(t.value), REBRAC_INFO_KEYS if full_update else REBRAC_CRITIC_INFO_KEYS)

    # -- reference API ----------------------------------------------------------------------
    def update(self, batch, full_update=True, noise=None, want_info=True):
        """agents/rebrac.py:122-134.  Returns (agent, info); info is a LazyInfo with REBRAC_INFO_KEYS (full step) or
        REBRAC_CRITIC_INFO_KEYS (critic-only step), or None with want_info=False."""
        B, args = self._rebrac_batch(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_rebrac_update(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, int(bool(full_update)),
                                                None, stream))
        self._keep = (args, nargs)
        self._last_full = bool(full_update)
        return self, (self._info(stream, full_update) if want_info else None)

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None, full_update=True):
        """train_dataset.sample(B) (return_next_actions) + update(batch, full_update) without leaving the device."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        ip, keep = None, None
        if idxs is not None:
            keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
        self._check(self._lib.fql_rebrac_update_from_dataset(self._h, ip, B, int(shard[0]), int(shard[1]), C.byref(nz) if nz else None,
                                                             int(bool(full_update)), None, stream))
        self._keep = (keep, nargs)
        self._last_full = bool(full_update)
        return self, (self._info(stream, full_update) if want_info else None)

    def read_info(self):
        """The infos of the last update (12 or 7 keys by its kind; blocks until it has run)."""
        buf = (C.c_float * _cabi.FQL_NUM_INFO)()
        self._check(self._lib.fql_read_info(self._h, buf))
        keys = REBRAC_INFO_KEYS if getattr(self, '_last_full', True) else REBRAC_CRITIC_INFO_KEYS
        return {k: float(buf[i]) for i, k in enumerate(keys)}

    def total_loss(self, batch, grad_params=None, rng=None, noise=None, full_update=True):
        """agents/rebrac.py:86-108 with grad_params=None (the validation probe, main.py:284): (loss, info) with 9 infos on a full step,
        the 4 critic infos otherwise.  No state changes."""
        if grad_params is not None:
            raise NotImplementedError('total_loss with traced grad_params is jax.grad plumbing; use update()')
        if rng is not None:
            raise NotImplementedError('ReBRAC draws its noise from the engine RNG or explicit tensors (noise=), not JAX keys')
        B, args = self._rebrac_batch(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        info = (C.c_float * 10)()
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_rebrac_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None,
                                                    int(bool(full_update)), C.byref(loss), info, stream))
        keys = REBRAC_INFO_KEYS[:9] if full_update else REBRAC_INFO_KEYS[:4]
        return float(loss.value), {k: float(info[i]) for i, k in enumerate(keys)}

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """agents/rebrac.py:136-152: clip(mode + clip(N(0, 1) actor_noise temperature, +-actor_noise_clip), -1, 1).  [od] -> [act];
        [n, od] -> [n, act].  `noises`: the raw N(0, 1) with the actions' shape, or None = engine RNG keyed by `seed`."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        is_torch = hasattr(observations, 'data_ptr')
        if int(observations.shape[-1]) != od:
            raise ValueError(f'observations last dim must be {od}, got {tuple(observations.shape)}')
        lead = tuple(observations.shape[:-1])
        n = int(np.prod(lead)) if lead else 1
        o = _Arg(observations, (n, od))
        z = _Arg(noises, (n, ad))
        if is_torch and observations.is_cuda:
            torch = __import__('torch')
            out = torch.empty(lead + (ad,), dtype=torch.float32, device=observations.device)
            optr = out.data_ptr()
        else:
            out = np.empty(lead + (ad,), dtype=np.float32)
            optr = out.ctypes.data
        if seed is None and noises is None:
            self._sample_calls += 1
            sd = (self._seed << 20) ^ self._sample_calls
        else:
            sd = _seed_to_u64(seed)
        self._check(self._lib.fql_rebrac_sample_actions(self._h, o.ptr, n, z.ptr, sd & 0xFFFFFFFFFFFFFFFF, float(temperature), optr,
                                                        self._stream([o, z])))
        return out

    def rebrac_stats(self, full_update=True):
        """(launches, MACs) of one full or critic-only update."""
        la, ma = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_rebrac_stats(self._h, int(bool(full_update)), C.byref(la), C.byref(ma)))
        return int(la.value), int(ma.value)

    # -- FQL-only paths, refused before the library is called ----------------------------------
    def _refuse(self, what):
        raise NotImplementedError(f'ReBRAC: {what} is not available (FQL agents only)')

    def compute_flow_actions(self, observations, noises):
        self._refuse('compute_flow_actions (the actor is deterministic)')

    def update_balanced(self, *a, **k):
        self._refuse('balanced sampling')

    def create_replay_buffer(self, size):
        self._refuse('a replay ring beside the dataset')

    def update_begin(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_begin_split(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_end(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_end_split(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def grad_buckets(self):
        self._refuse('gradient buckets')


__all__ = ['ReBRACAgent', 'REBRAC_INFO_KEYS', 'REBRAC_CRITIC_INFO_KEYS', 'REBRAC_NOISE_KEYS', 'get_config']
