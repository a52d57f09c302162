"""Host-side mirror of the reference's IQLAgent (agents/iql.py) over the C ABI: implicit Q-learning with an expectile value, a critic
pair with a Polyak target and a plain Gaussian actor trained by AWR or by DDPG+BC.  Same call sites as the reference:

    agent = IQLAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch)                      # info: LazyInfo with 16 (awr) or 19 (ddpgbc) keys
    action = agent.sample_actions(observations=ob, seed=key, temperature=1.0)

State observations and fp32 only: `encoder`, precision 'bf16x3', JAX-key noise, compute_flow_actions, the data-parallel begin / end
halves, gradient buckets, the replay ring and agent groups are refused here, before the library is called.  Everything else (datasets,
checkpoints, get/set_params, synchronize) is FQLAgent's plumbing on an IQL handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi
from .agent import FQLAgent, LazyInfo, _Arg, _seed_to_u64
from .config import ConfigDict
from .sac import _PendingN

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


class IQLAgent(FQLAgent):
    """Implicit Q-learning agent backed by the MI355X step engine."""

    _jax_sample_noise = False
    _pending_cls = _PendingN

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/iql.py:171-239.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        if cfg.get('encoder') is not None:
            raise NotImplementedError('IQL: visual encoders are not available (state observations only)')
        if cfg.get('precision', 'fp32') not in ('fp32', 0):
            raise NotImplementedError(f"IQL runs in fp32 only (precision {cfg['precision']!r})")
        if cfg.get('rng', 'engine') != 'engine':
            raise NotImplementedError(f"IQL draws its noise from the engine's RNG or explicit tensors only (rng {cfg['rng']!r})")
        if cfg['actor_loss'] not in IQL_INFO_KEYS:
            raise ValueError(f"Unsupported actor loss: {cfg['actor_loss']}")
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

    def _info(self, stream):
        t = C.c_uint64()
        self._check(self._lib.fql_info_enqueue(self._h, stream, C.byref(t)))
        return LazyInfo(self, int(t.value), self._info_keys)

    # -- reference API ----------------------------------------------------------------------
    def update(self, batch, noise=None, want_info=True):
        """agents/iql.py update.  Returns (agent, info); info is a LazyInfo with the handle's info keys, or None with want_info=False."""
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_iql_update(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, None, stream))
        self._keep = (args, nargs)
        return self, (self._info(stream) if want_info else None)

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None):
        """train_dataset.sample(B) + update(batch) without leaving the device."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        ip, keep = None, None
        if idxs is not None:
            keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
        self._check(self._lib.fql_iql_update_from_dataset(self._h, ip, B, int(shard[0]), int(shard[1]), C.byref(nz) if nz else None,
                                                          None, stream))
        self._keep = (keep, nargs)
        return self, (self._info(stream) if want_info else None)

    def read_info(self):
        """The infos of the last update (blocks until it has run)."""
        n = len(self._info_keys)
        buf = (C.c_float * n)()
        self._check(self._lib.fql_read_info_n(self._h, buf, n))
        return {k: float(buf[i]) for i, k in enumerate(self._info_keys)}

    def total_loss(self, batch, grad_params=None, rng=None, noise=None):
        """agents/iql.py total_loss with grad_params=None (the validation probe, main.py:284): (loss, info) with the value, critic and
        actor infos.  No state changes."""
        if grad_params is not None:
            raise NotImplementedError('total_loss with traced grad_params is jax.grad plumbing; use update()')
        if rng is not None:
            raise NotImplementedError('IQL draws its noise from the engine RNG or explicit tensors (noise=), not JAX keys')
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

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """agents/iql.py sample_actions: clip(mean + exp(log_stds) temperature N(0, 1), -1, 1).  [od] -> [act]; [n, od] -> [n, act].
        `noises`: the raw N(0, 1) with the actions' shape, or None = engine RNG keyed by `seed`."""
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
        self._check(self._lib.fql_iql_sample_actions(self._h, o.ptr, n, z.ptr, sd & 0xFFFFFFFFFFFFFFFF, float(temperature), optr,
                                                     self._stream([o, z])))
        return out

    def iql_stats(self):
        """(launches, MACs) of one update."""
        la, ma = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_iql_stats(self._h, C.byref(la), C.byref(ma)))
        return int(la.value), int(ma.value)

    # -- FQL-only paths, refused before the library is called ----------------------------------
    def _refuse(self, what):
        raise NotImplementedError(f'IQL: {what} is not available (FQL agents only)')

    def compute_flow_actions(self, observations, noises):
        self._refuse('compute_flow_actions (the actor is a Gaussian, there is no flow)')

    def update_begin(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_begin_split(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_end(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_end_split(self, *a, **k):
        self._refuse('the data-parallel update halves')

    def update_balanced(self, *a, **k):
        self._refuse('balanced sampling (IQL trains offline from one dataset)')

    def grad_buckets(self):
        self._refuse('gradient buckets')


__all__ = ['IQLAgent', 'IQL_INFO_KEYS', 'IQL_AWR_INFO_KEYS', 'IQL_DDPGBC_INFO_KEYS', 'IQL_NOISE_KEYS', 'get_config']
