"""Host-side mirror of the reference's FQLAgent (agents/fql.py:15-246) over the C ABI.

Same method names, keyword names and return shapes as the reference so its call sites keep working:

    agent = FQLAgent.create(seed, ex_observations, ex_actions, config)      # main.py:160
    agent, info = agent.update(batch)                                         # main.py:216
    actions = agent.sample_actions(observations=ob, temperature=1, seed=key)  # main.py:225
    loss, info = agent.total_loss(val_batch, grad_params=None)                # main.py:284
    actions = agent.compute_flow_actions(observations, noises)                # agents/fql.py:155
    qs = agent.network.select('critic')(observations, actions=actions)        # agents/fql.py:36,70 (stored parameters)

The reference is functional (update returns a NEW agent, callers rebind); here the engine owns the
state in HBM, update mutates it and returns ``self`` -- compatible with every reference call site.
All compute happens in libfql_amd.so (HIP, gfx950); there is no Python/torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional

import numpy as np

from . import _cabi, jax_prng
from .config import ConfigDict, get_config

INFO_KEYS = (
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/actor_loss', 'actor/bc_flow_loss', 'actor/distill_loss', 'actor/q_loss',
    'actor/q', 'actor/mse', 'grad/max', 'grad/min', 'grad/norm',
)
NOISE_KEYS = ('eps1', 'x0', 't', 'z', 'eps2')
BATCH_KEYS = ('observations', 'actions', 'rewards', 'masks', 'next_observations')


def _torch():
    import torch
    return torch


def _seed_to_u64(seed) -> int:
    """Accept what reference call sites pass as `seed`: None, int, or a JAX-style uint32[2] key."""
    if seed is None:
        return 0
    a = np.asarray(seed)
    if a.ndim == 0:
        return int(a) & 0xFFFFFFFFFFFFFFFF
    a = a.astype(np.uint64).reshape(-1)
    v = 0
    for x in a[:2]:
        v = ((v << 32) | (int(x) & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
    return v


class _Arg:
    """fp32 contiguous view of a user array + the pointer handed to the C ABI (device or host)."""

    def __init__(self, x, shape=None, u8=False):
        self.keep = None
        if x is None:
            self.ptr = None
            return
        if hasattr(x, 'data_ptr'):  # torch tensor (cuda or cpu)
            torch = _torch()
            t = x.detach()
            want = torch.uint8 if u8 else torch.float32
            if t.dtype != want:
                t = t.to(want)
            t = t.contiguous()
            if shape is not None and int(np.prod(shape)) != t.numel():
                raise ValueError(f'expected {int(np.prod(shape))} elements, got shape {tuple(t.shape)}')
            self.keep = t
            self.ptr = t.data_ptr()
        else:
            a = np.ascontiguousarray(np.asarray(x), dtype=np.uint8 if u8 else np.float32)
            if shape is not None and int(np.prod(shape)) != a.size:
                raise ValueError(f'expected {int(np.prod(shape))} elements, got shape {a.shape}')
            self.keep = a
            self.ptr = a.ctypes.data


class _Pending:
    """The 13 scalars of one update, fetched from the engine's pinned snapshot ring on first use (one blocking wait, then cached)."""

    def __init__(self, agent, ticket):
        self.agent, self.ticket, self.vals = agent, ticket, None

    def get(self):
        if self.vals is None:
            buf = (C.c_float * _cabi.FQL_NUM_INFO)()
            self.agent._check(self.agent._lib.fql_info_wait(self.agent._h, self.ticket, buf))
            self.vals = [float(buf[i]) for i in range(_cabi.FQL_NUM_INFO)]
            self.agent = None
        return self.vals


class _PendingN(_Pending):
    """_Pending over fql_info_wait_n: all fql_num_info(h) scalars of one update."""

    def get(self):
        if self.vals is None:
            n = len(self.agent._info_keys)
            buf = (C.c_float * n)()
            self.agent._check(self.agent._lib.fql_info_wait_n(self.agent._h, self.ticket, buf, n))
            self.vals = [float(buf[i]) for i in range(n)]
            self.agent = None
        return self.vals


class LazyScalar:
    """One info value of an update that may not have run yet - what a JAX device scalar is in the reference's info dict (agents/fql.py:39-44;
    main.py:276 reads them at log time).  float(x), arithmetic, comparisons, formatting, numpy conversion all block until the update has run and
    then behave as the plain float.  Pickles as a float."""
    __slots__ = ('_p', '_i')

    def __init__(self, pending, i):
        self._p, self._i = pending, i

    def __float__(self): return self._p.get()[self._i]
    def item(self): return float(self)
    def __int__(self): return int(float(self))
    def __bool__(self): return bool(float(self))
    def __round__(self, n=None): return round(float(self), n)
    def __repr__(self): return repr(float(self))
    __str__ = __repr__
    def __format__(self, spec): return format(float(self), spec)
    def __array__(self, dtype=None, copy=None): return np.asarray(float(self), dtype=dtype)
    def __reduce__(self): return (float, (float(self),))
    def __hash__(self): return hash(float(self))
    def __eq__(self, o): return float(self) == o
    def __ne__(self, o): return float(self) != o
    def __lt__(self, o): return float(self) < o
    def __le__(self, o): return float(self) <= o
    def __gt__(self, o): return float(self) > o
    def __ge__(self, o): return float(self) >= o
    def __neg__(self): return -float(self)
    def __pos__(self): return float(self)
    def __abs__(self): return abs(float(self))
    def __add__(self, o): return float(self) + o
    def __radd__(self, o): return o + float(self)
    def __sub__(self, o): return float(self) - o
    def __rsub__(self, o): return o - float(self)
    def __mul__(self, o): return float(self) * o
    def __rmul__(self, o): return o * float(self)
    def __truediv__(self, o): return float(self) / o
    def __rtruediv__(self, o): return o / float(self)
    def __pow__(self, o): return float(self) ** o
    def __rpow__(self, o): return o ** float(self)


class LazyInfo(dict):
    """What `update` returns as `info` (the reference returns device scalars nobody waits for until main.py:276 logs them, so its training loop
    never synchronises per step): a REAL dict holding the 13 keys from the start - len(), iteration, json / pickle see all of them - whose values
    are LazyScalar objects that block on first use.  `to_dict()` gives plain floats (json.dumps(info.to_dict()), or json.dumps(info,
    default=float)); pickling and copy() give a plain dict of floats.  Holding it across more than 64 later lazy updates without reading it
    raises on first use (the engine keeps 64 snapshots)."""

    def __init__(self, agent, ticket, keys=None):
        p = getattr(agent, '_pending_cls', _Pending)(agent, ticket)
        keys = keys if keys is not None else getattr(agent, '_info_keys', INFO_KEYS)
        super().__init__((k, LazyScalar(p, i)) for i, k in enumerate(keys))

    def to_dict(self):
        return {k: float(v) for k, v in self.items()}

    def copy(self):
        return self.to_dict()

    def __reduce__(self):
        return (dict, (self.to_dict(),))


class _Network:
    """`agent.network` as far as reference call sites use it for forward queries: select(name) (utils/flax_utils.py:116-118) returns the
    module's forward on the stored parameters (fql_module_forward).  Module names are the reference's without the `modules_` prefix."""

    def __init__(self, agent):
        self._agent = agent

    def select(self, name):
        mods = self._agent._modules
        if name not in mods:
            raise KeyError(f'{self._agent._name} has no module {name!r} (its modules: {", ".join(mods)})')
        agent, family = self._agent, mods[name]
        if family in ('pair', 'value'):
            def module(observations, actions=None, params=None):   # utils/networks.py Value.__call__
                return agent._module_forward(name, family, observations, actions, None, params)
        else:
            def module(observations, actions, times=None, is_encoded=False, params=None):   # ActorVectorField.__call__
                return agent._module_forward(name, family, observations, actions, times, params)   # (is_encoded: no encoder on a state agent)
        module.__name__ = name
        return module


class FQLAgent:
    """Flow Q-learning agent backed by the MI355X step engine."""

    _name = 'FQL'
    _loss_infos = 10          # infos fql_total_loss writes (the total-loss probe has no gradient statistics)
    _jax_sample_noise = True  # sample_actions(seed=<JAX key>) draws the reference's noise on the host
    # network.select(name): the module's family.  'pair': Value(obs, actions) of the 2-member critic -> [2, n]; 'value': Value(obs) -> [n];
    # 'field_t': ActorVectorField(obs, actions, times) -> [n, act]; 'field': ActorVectorField(obs, noises) -> [n, act]
    _modules = {'critic': 'pair', 'target_critic': 'pair', 'actor_bc_flow': 'field_t', 'actor_onestep_flow': 'field'}

    def __init__(self, handle, config, seed):
        self._lib = _cabi.load()
        self._h = handle
        # the info keys of this handle's updates, in order (fql_handle_info_name)
        self._info_keys = tuple(self._lib.fql_handle_info_name(handle, i).decode() for i in range(self._lib.fql_num_info(handle)))
        self.config = config
        self._seed = seed
        self._keep = []
        self._sample_calls = 0
        # agents/fql.py:189-190: rng = PRNGKey(seed); rng, init_rng = split(rng, 2).  Only used when config['rng'] ==
        # 'jax' (noise drawn on the host with the reference's key derivation) or when a caller passes JAX keys.
        self.rng = jax_prng.split(jax_prng.PRNGKey(seed), 2, partitionable=bool(self._jax_mode()))[0]

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/fql.py:173-246.  `config`: dict-like with the keys of get_config()."""
        lib = _cabi.load()
        cfg = get_config()
        cfg.update(dict(config))
        c, ob_dims, action_dim = cls._engine_config(lib, cfg, ex_observations, ex_actions)
        h = C.c_void_p()
        rc = lib.fql_create(C.byref(c), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h))
        _cabi.check(lib, None, rc)
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        return cls(h, cfg, int(seed))

    @classmethod
    def _refuse_config(cls, cfg):
        """The create-time refusals of the agents of another kind than FQL (`_name`)."""
        if cfg.get('encoder') is not None:
            raise NotImplementedError(f'{cls._name}: visual encoders are not available (state observations only)')
        if cfg.get('precision', 'fp32') not in ('fp32', 0):
            raise NotImplementedError(f"{cls._name} runs in fp32 only (precision {cfg['precision']!r})")
        if cfg.get('rng', 'engine') != 'engine':
            raise NotImplementedError(f"{cls._name} draws its noise from the engine's RNG or explicit tensors only (rng {cfg['rng']!r})")

    @staticmethod
    def _engine_config(lib, cfg, ex_observations, ex_actions):
        """(fql_config, ob_dims, action_dim) for the networks `cfg` describes."""
        ex_observations = np.asarray(ex_observations) if not hasattr(ex_observations, 'shape') else ex_observations
        ob_dims = tuple(int(d) for d in ex_observations.shape[1:])
        action_dim = int(ex_actions.shape[-1])
        c = _cabi.FqlConfig()
        lib.fql_default_config(C.byref(c))
        if cfg.get('encoder') is not None:
            # agents/fql.py:196-202: one encoder per module in front of the MLPs; observations are uint8 images [H, W, C]
            if cfg['encoder'] not in ('impala_small', 'impala'):
                raise NotImplementedError(f"encoder {cfg['encoder']!r}: 'impala_small' and 'impala' (utils/encoders.py:104,106) are built")
            if len(ob_dims) != 3:
                raise ValueError(f'image observations [H, W, C] expected with an encoder, got ob_dims={ob_dims}')
            c.encoder, c.img_h, c.img_w, c.img_c = (1 if cfg['encoder'] == 'impala_small' else 2), ob_dims[0], ob_dims[1], ob_dims[2]
            c.obs_dim = 1
        else:
            if len(ob_dims) != 1:
                raise ValueError(f'state-based observations expected, got ob_dims={ob_dims}')
            c.obs_dim = int(ob_dims[0])
        c.act_dim = action_dim
        ah, vh = tuple(cfg['actor_hidden_dims']), tuple(cfg['value_hidden_dims'])
        if len(ah) > _cabi.FQL_MAX_HIDDEN or len(vh) > _cabi.FQL_MAX_HIDDEN:
            raise ValueError('too many hidden layers')
        c.num_actor_hidden, c.num_value_hidden = len(ah), len(vh)
        for i, v in enumerate(ah):
            c.actor_hidden[i] = int(v)
        for i, v in enumerate(vh):
            c.value_hidden[i] = int(v)
        c.layer_norm, c.actor_layer_norm = int(bool(cfg['layer_norm'])), int(bool(cfg['actor_layer_norm']))
        c.lr, c.discount, c.tau = float(cfg['lr']), float(cfg['discount']), float(cfg['tau'])
        c.alpha = float(cfg.get('alpha', c.alpha))
        q_agg = cfg.get('q_agg', 'mean')
        if q_agg not in ('mean', 'min'):
            raise ValueError(f"q_agg must be 'mean' or 'min', got {q_agg!r}")
        c.q_agg = 1 if q_agg == 'min' else 0
        c.flow_steps = int(cfg['flow_steps'])
        c.normalize_q_loss = int(bool(cfg.get('normalize_q_loss', False)))
        c.batch_size = int(cfg['batch_size'])
        prec = cfg.get('precision', 'fp32')
        if prec not in ('fp32', 'bf16x3', 0, 2):
            raise ValueError(f"precision must be 'fp32' or 'bf16x3', got {prec!r}")
        c.precision = 2 if prec in ('bf16x3', 2) else 0
        return c, ob_dims, action_dim

    def close(self):
        if getattr(self, '_h', None):
            rc = self._lib.fql_destroy(self._h)
            if rc == _cabi.FQL_E_STATE:   # a member of an agent group: the handle stays valid until the group is closed
                self._check(rc)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ----------------------------------------------------------------------------
    def _check(self, rc):
        _cabi.check(self._lib, self._h, rc)

    @staticmethod
    def _stream(args):
        """Run on torch's current stream when any argument lives on the GPU (keeps torch's caching allocator and the engine
        stream-ordered, including the dtype / contiguity temporaries made just before the call); otherwise the engine's own
        stream (NULL).  torch's DEFAULT stream has the handle 0, which the C ABI reads as "no stream": it is passed as
        FQL_STREAM_LEGACY (hipStreamLegacy) instead, so the engine's graph is enqueued on that very stream."""
        for a in args:
            k = getattr(a, 'keep', None)
            if k is not None and hasattr(k, 'is_cuda') and k.is_cuda:
                h = _torch().cuda.current_stream().cuda_stream
                return h if h else _cabi.FQL_STREAM_LEGACY
        return None

    def _batch_args(self, batch):
        B = int(np.shape(batch['actions'])[0]) if not hasattr(batch['actions'], 'shape') else int(batch['actions'].shape[0])
        obd, ad = tuple(self.config['ob_dims']), self.config['action_dim']
        shapes = {'observations': (B,) + obd, 'actions': (B, ad), 'rewards': (B,), 'masks': (B,), 'next_observations': (B,) + obd}
        for k in BATCH_KEYS:
            if k not in batch:
                raise KeyError(f'batch is missing {k!r}')
        vis = len(obd) == 3   # image observations travel as uint8 (utils/encoders.py:84 divides by 255 on the device)
        return B, [_Arg(batch[k], shapes[k], u8=vis and k.endswith('observations')) for k in BATCH_KEYS]

    def _noise_args(self, noise, B):
        if noise is None:
            return None, []
        ad = self.config['action_dim']
        shapes = {'eps1': (B, ad), 'x0': (B, ad), 't': (B,), 'z': (B, ad), 'eps2': (B, ad)}
        args = [_Arg(noise.get(k), shapes[k]) for k in NOISE_KEYS]
        nz = _cabi.FqlNoise(*[a.ptr for a in args])
        return nz, args

    def _ensure_batch(self, B):
        if B != self.config['batch_size']:
            self._check(self._lib.fql_set_batch_size(self._h, B))
            self.config['batch_size'] = B

    # -- reference API ----------------------------------------------------------------------
    def update(self, batch, noise: Optional[Dict[str, Any]] = None, want_info=True):
        """agents/fql.py:122-133.  Returns (agent, info).  `noise` (optional) supplies the five random
        tensors explicitly (parity runs); by default they come from the engine's device RNG.
        `info` is a LazyInfo: a dict of the 13 scalars that is read from the device on first access, so a loop that only logs
        every N steps (main.py:216,276) never synchronises in between.  want_info=False returns None (no snapshot at all)."""
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        jax_mode = self._jax_mode()
        if noise is None and jax_mode is not None and not self.config.get('rng_device', True):
            self.rng, noise = jax_prng.fql_update_noise(self.rng, B, self.config['action_dim'], partitionable=jax_mode)
        nz, nargs = self._noise_args(noise, B)
        stream = self._stream(args + nargs)
        if noise is None and jax_mode is not None:
            # the reference's key derivation on the host (a dozen 2-word hashes), the five tensors on the device: nothing but 10 words
            # of keys crosses PCIe (config['rng_device']=False: tensors drawn on the host by fql_amd/jax_prng.py instead)
            self.rng, keys = jax_prng.fql_update_keys(self.rng, partitionable=jax_mode)
            nz = self._device_noise(keys, jax_mode, B, stream)
        self._check(self._lib.fql_update(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, None, stream))
        self._keep = (args, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    def _jax_mode(self):
        """None: engine RNG; False / True: JAX key derivation with the original / partitionable threefry layout."""
        r = self.config.get('rng')
        if r == 'jax':
            return False
        if r == 'jax_partitionable':
            return True
        return None

    def _device_noise(self, keys, partitionable, B, stream):
        k = np.ascontiguousarray(np.stack([np.asarray(keys[n], dtype=np.uint32).reshape(2) for n in NOISE_KEYS]))
        nz = _cabi.FqlNoise()
        self._check(self._lib.fql_noise_from_jax_keys(self._h, k.ctypes.data, int(bool(partitionable)), B, C.byref(nz), stream))
        return nz

    def _lazy_info(self, stream):
        t = C.c_uint64()
        self._check(self._lib.fql_info_enqueue(self._h, stream, C.byref(t)))
        return LazyInfo(self, int(t.value))

    def _resident_noise(self, noise, B, stream):
        """(fql_noise or None, keep-alive) for the device-resident update paths: explicit tensors, else - with config['rng'] = 'jax' /
        'jax_partitionable' - the reference's key derivation advanced on the host and the five tensors generated on the device from the derived
        keys (exactly what update() does), else None = the engine's Philox stream."""
        nz, nargs = self._noise_args(noise, B)
        jax_mode = self._jax_mode()
        if noise is None and jax_mode is not None:
            self.rng, keys = jax_prng.fql_update_keys(self.rng, partitionable=jax_mode)
            nz = self._device_noise(keys, jax_mode, B, stream)
        return nz, nargs

    def _host_idx(self, idxs, n, rows, what):
        """int64 view of HOST gather indices, checked against the rows the device array holds: an index >= size would train on zero rows or read
        past the array on the device.  Device tensors are passed through unchecked (documented in INTEGRATION.md)."""
        if hasattr(idxs, 'data_ptr'):
            keep = idxs.long().contiguous()
            if keep.numel() != n:
                raise ValueError(f'{what} must have {n} entries')
            if not keep.is_cuda:
                lo, hi = (int(keep.min()), int(keep.max())) if n else (0, -1)
                if lo < 0 or hi >= rows:
                    raise ValueError(f'{what} out of range: [{lo}, {hi}] for {rows} rows')
            return keep, keep.data_ptr()
        keep = np.ascontiguousarray(idxs, dtype=np.int64)
        if keep.size != n:
            raise ValueError(f'{what} must have {n} entries')
        if n and (keep.min() < 0 or keep.max() >= rows):
            raise ValueError(f'{what} out of range: [{int(keep.min())}, {int(keep.max())}] for {rows} rows')
        return keep, keep.ctypes.data

    def read_info(self) -> Dict[str, float]:
        """The 13 info scalars of the last update (blocks until that update has run)."""
        buf = (C.c_float * _cabi.FQL_NUM_INFO)()
        self._check(self._lib.fql_read_info(self._h, buf))
        return {k: float(buf[i]) for i, k in enumerate(self._info_keys)}

    def synchronize(self) -> str:
        """Host wait for every update enqueued so far (jax.block_until_ready(agent)): the engine's HIP stream and the hardware queues of
        its own that stream-less updates run on, which torch.cuda.synchronize() does not see.  Returns where the last update ran:
        'aql' (the engine's own queues) or 'graph' (a captured graph on a HIP stream)."""
        m = C.c_int(0)
        self._check(self._lib.fql_synchronize(self._h, C.byref(m)))
        return 'aql' if m.value else 'graph'

    def total_loss(self, batch, grad_params=None, rng=None, noise: Optional[Dict[str, Any]] = None):
        """agents/fql.py:94-111 with grad_params=None (the validation probe, main.py:284)."""
        if grad_params is not None:
            raise NotImplementedError('total_loss with traced grad_params is jax.grad plumbing; use update()')
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        if noise is None and (rng is not None or self._jax_mode() is not None):
            noise = jax_prng.fql_total_loss_noise(self.rng if rng is None else rng, B, self.config['action_dim'],
                                                  partitionable=bool(self._jax_mode()))
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        info = (C.c_float * 10)()
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None,
                                             C.byref(loss), info, stream))
        return float(loss.value), {k: float(info[i]) for i, k in enumerate(self._info_keys[:self._loss_infos])}

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """agents/fql.py:135-153: clip(onestep(obs, N(0, I))).  `temperature` is accepted and ignored,
        as in the reference.  Leading dims of `observations` are preserved ([od] -> [ad])."""
        return self._eval(observations, noises, seed, flow=False)

    def compute_flow_actions(self, observations, noises):
        """agents/fql.py:155-171."""
        return self._eval(observations, noises, None, flow=True)

    def _sample_noise_shape(self, n, flow):
        return (n, self.config['action_dim'])

    def _eval(self, observations, noises, seed, flow):
        obd, ad = tuple(self.config['ob_dims']), self.config['action_dim']
        vis = len(obd) == 3
        od = obd[0] if not vis else None
        if vis and tuple(observations.shape[-3:]) != obd:
            raise ValueError(f'observations must end in {obd}, got {tuple(observations.shape)}')
        lead = tuple(observations.shape[:-3]) if vis else tuple(observations.shape[:-1])
        if self._jax_sample_noise and not flow and noises is None and seed is not None and np.ndim(seed) == 1 and np.size(seed) == 2:
            # a JAX key (what main.py:225 / utils/evaluation.py:98-101 pass): draw exactly the noise the reference draws
            noises = jax_prng.sample_actions_noise(np.asarray(seed), lead, ad, partitionable=bool(self._jax_mode()))
        if not vis and int(observations.shape[-1]) != od:
            raise ValueError(f'observations last dim must be {od}, got {tuple(observations.shape)}')
        n = int(np.prod(lead)) if lead else 1
        o = _Arg(observations, (n,) + obd, u8=vis)
        z = _Arg(noises, self._sample_noise_shape(n, flow))
        out, optr = self._actions_out(observations, lead + (ad,))
        stream = self._stream([o, z])
        if flow:
            self._check(self._lib.fql_flow_actions(self._h, o.ptr, z.ptr, n, optr, stream))
        else:
            self._check(self._lib.fql_sample_actions(self._h, o.ptr, n, z.ptr, self._sample_seed(seed, noises), optr, stream))
        return out

    @staticmethod
    def _actions_out(observations, shape):
        """(array, pointer) for sampled actions: a tensor beside CUDA observations, else a NumPy array."""
        if hasattr(observations, 'data_ptr') and observations.is_cuda:
            out = _torch().empty(shape, dtype=_torch().float32, device=observations.device)
            return out, out.data_ptr()
        out = np.empty(shape, dtype=np.float32)
        return out, out.ctypes.data

    def _sample_seed(self, seed, noises):
        """The uint64 that keys the engine's draw: `seed`, or a counter of this agent's own when neither seed nor noises is given."""
        if seed is None and noises is None:
            self._sample_calls += 1
            return ((self._seed << 20) ^ self._sample_calls) & 0xFFFFFFFFFFFFFFFF
        return _seed_to_u64(seed) & 0xFFFFFFFFFFFFFFFF

    # -- forward queries: agent.network.select(name)(...) -----------------------------------------
    @property
    def network(self):
        """`agent.network.select('critic')(observations, actions=actions)` and the like (utils/flax_utils.py:116-118; 47 call sites in
        agents/*.py): one module's forward on the stored parameters, on the caller's rows.  numpy in, numpy out; CUDA tensors in, a CUDA
        tensor out on torch's current stream.  Parameters are read with get_params()."""
        if not self._modules:
            raise NotImplementedError(f"{self._name}: network.select is not available (the module's input carries host-built embeddings)")
        if len(self.config['ob_dims']) == 3:
            raise NotImplementedError(f"{self._name}: network.select is not available on visual agents (the module's encoder would run first)")
        return _Network(self)

    def _module_forward(self, name, family, observations, actions, times, params):
        if params is not None:
            raise NotImplementedError(f'network.select({name!r})(params=...) is jax.grad plumbing; the stored parameters are used')
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        oshape = tuple(np.shape(observations))
        if not oshape or oshape[-1] != od:
            raise ValueError(f'observations last dim must be {od}, got {oshape}')
        lead = oshape[:-1]
        n = int(np.prod(lead)) if lead else 1
        if n < 1:
            raise ValueError(f'observations hold no rows: {oshape}')
        takes_actions, takes_times = family != 'value', family == 'field_t'
        if takes_actions != (actions is not None):
            raise ValueError(f'{name}: ' + ('actions are required' if takes_actions else 'a value module takes observations only (actions=None)'))
        if actions is not None and tuple(np.shape(actions)) != lead + (ad,):
            raise ValueError(f'{name}: actions must be {lead + (ad,)}, got {tuple(np.shape(actions))}')
        if takes_times != (times is not None):
            raise ValueError(f'{name}: ' + ('times are required' if takes_times else 'the module takes no times (times=None)'))
        if times is not None and tuple(np.shape(times)) not in (lead, lead + (1,)):
            raise ValueError(f'{name}: times must be {lead} or {lead + (1,)}, got {tuple(np.shape(times))}')
        o, a, t = _Arg(observations, (n, od)), _Arg(actions, (n, ad)), _Arg(times, (n,))
        out, optr = self._actions_out(observations, {'pair': (2,) + lead, 'value': lead}.get(family, lead + (ad,)))
        self._check(self._lib.fql_module_forward(self._h, name.encode(), o.ptr, a.ptr, t.ptr, n, optr, self._stream([o, a, t])))
        return out

    # -- device-resident dataset (utils/datasets.py Dataset/ReplayBuffer on the GPU) -------------
    def upload_dataset(self, dataset, capacity: Optional[int] = None, frame_stack: Optional[int] = None, p_aug: Optional[float] = None):
        """Dataset.create(...) arrays -> HBM.  Visual agents: `observations` / `next_observations` are the uint8 FRAMES
        [N, H, W, C / frame_stack] and `terminals` marks episode ends; frame stacking (main.py:120-121 sets
        dataset.frame_stack) and the random crop (dataset.p_aug) then happen in the device-side gather."""
        if len(self.config['ob_dims']) == 3:
            fs = int(frame_stack if frame_stack is not None else (self.config.get('frame_stack') or 1))
            pa = float(p_aug if p_aug is not None else (self.config.get('p_aug') or 0.0))
            n = int(len(dataset['observations']))
            H, W, Cc = self.config['ob_dims']
            fshape = (n, H, W, Cc // fs)
            fr = _Arg(dataset['observations'], fshape, u8=True)
            nf = _Arg(dataset['next_observations'], fshape, u8=True)
            rest = [_Arg(dataset[k]) for k in ('actions', 'rewards', 'masks', 'terminals')]
            self._check(self._lib.fql_dataset_upload_frames(self._h, n, fr.ptr, nf.ptr, *[a.ptr for a in rest], fs, pa))
            self._frame_stack = fs     # (remembered for the shape check of later ring inserts)
            return
        n = int(len(dataset['observations']))
        cap = int(capacity) if capacity is not None else max(n, 1)
        args = [_Arg(dataset[k]) for k in BATCH_KEYS]
        self._check(self._lib.fql_dataset_upload(self._h, n, cap, *[a.ptr for a in args]))

    def reserve_dataset(self, capacity: int):
        """ReplayBuffer.create_from_initial_dataset(dataset, size) (utils/datasets.py:457-473, main.py:111-115): the uploaded dataset
        becomes a ring of `capacity` rows (state or uint8 frames); `add_transition` then inserts at the pointer."""
        self._check(self._lib.fql_dataset_reserve(self._h, int(capacity)))

    def create_replay_buffer(self, size: int):
        """ReplayBuffer.create(example_transition, size) (utils/datasets.py:441-455; main.py:106-109): an empty device ring beside the
        training dataset, the second source of `update_balanced`."""
        self._check(self._lib.fql_replay_create(self._h, int(size)))

    def add_transition(self, transition, replay: bool = False):
        """ReplayBuffer.add_transition (utils/datasets.py:483-491) into the dataset ring (replay=False: the dataset IS the replay
        buffer, main.py:111-115) or into the separate replay ring (replay=True, balanced sampling).  Visual agents pass single uint8
        frames [H, W, C / frame_stack] as observations / next_observations."""
        a = _Arg(transition['actions'], (self.config['action_dim'],))
        r, m = float(transition['rewards']), float(transition['masks'])
        if len(self.config['ob_dims']) == 3:
            H, W, Cc = self.config['ob_dims']
            fs = int(getattr(self, '_frame_stack', 0) or 0)
            fr = _Arg(transition['observations'], u8=True); nf = _Arg(transition['next_observations'], u8=True)
            nel = fr.keep.numel() if hasattr(fr.keep, 'numel') else fr.keep.size
            if fs and nel != H * W * (Cc // fs):
                raise ValueError(f'expected one uint8 frame of {H}x{W}x{Cc // fs}, got {nel} elements')
            f = self._lib.fql_replay_add_frames if replay else self._lib.fql_dataset_add_frames
            self._check(f(self._h, fr.ptr, nf.ptr, a.ptr, r, m))
            return
        od = self.config['ob_dims'][0]
        o = _Arg(transition['observations'], (od,)); no = _Arg(transition['next_observations'], (od,))   # (raises on a wrong element count)
        f = self._lib.fql_replay_add if replay else self._lib.fql_dataset_add
        self._check(f(self._h, o.ptr, a.ptr, r, m, no.ptr))

    def replay_size(self):
        s, p = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_replay_size(self._h, C.byref(s), C.byref(p)))
        return int(s.value), int(p.value)

    def update_balanced(self, batch_size=None, idxs=None, noise=None, want_info=False, stream=None, crop_froms=None):
        """main.py:255-259 + :216 on the device: concat(train_dataset.sample(B // 2), replay_buffer.sample(B // 2)) -> agent.update.
        `idxs` = (dataset_idxs, replay_idxs), B // 2 each, or None (engine RNG)."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._resident_noise(noise, B, stream)
        ia = ib = None
        keep = None
        if idxs is not None:
            ka, ia = self._host_idx(idxs[0], B // 2, self.dataset_size()[0], 'dataset idxs')
            kb, ib = self._host_idx(idxs[1], B // 2, self.replay_size()[0], 'replay idxs')
            keep = (ka, kb)
        cp = None
        if crop_froms is not None:
            ck = np.ascontiguousarray(crop_froms, dtype=np.int32)
            if ck.shape != (B, 2):
                raise ValueError('crop_froms must be [batch_size, 2]')
            cp, keep = ck.ctypes.data, (keep, ck)
        self._check(self._lib.fql_update_balanced(self._h, ia, ib, cp, B, C.byref(nz) if nz else None, None, stream))
        self._keep = (keep, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    def dataset_size(self):
        s, p = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_dataset_size(self._h, C.byref(s), C.byref(p)))
        return int(s.value), int(p.value)

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None,
                            crop_froms=None):
        """train_dataset.sample(B) + agent.update(batch) (main.py:201,216) without leaving the device.  Visual agents:
        `crop_froms` int [B, 2] fixes the random-crop offsets Dataset.augment would draw (None: engine RNG with p_aug)."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._resident_noise(noise, B, stream)
        ip, keep = None, None
        if idxs is not None:
            keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
        if crop_froms is not None:
            ck = np.ascontiguousarray(crop_froms, dtype=np.int32)
            if ck.shape != (B, 2):
                raise ValueError('crop_froms must be [batch_size, 2]')
            self._check(self._lib.fql_update_from_frames(self._h, ip, ck.ctypes.data, B, int(shard[0]), int(shard[1]),
                                                         C.byref(nz) if nz else None, None, stream))
            keep = (keep, ck)
        else:
            self._check(self._lib.fql_update_from_dataset(self._h, ip, B, int(shard[0]), int(shard[1]),
                                                          C.byref(nz) if nz else None, None, stream))
        self._keep = (keep, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    # -- data-parallel halves (fql_amd/parallel.py drives these) ---------------------------------
    def update_begin(self, batch=None, noise=None, idxs=None, shard=(0, 0), batch_size=None, stream=None):
        if batch is not None:
            B, args = self._batch_args(batch)
            self._ensure_batch(B)
            st = stream if stream is not None else self._stream(args)
            nz, nargs = self._resident_noise(noise, B, st)
            self._check(self._lib.fql_update_begin(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, st))
            self._keep = (args, nargs)
        else:
            B = int(batch_size or self.config['batch_size'])
            self._ensure_batch(B)
            nz, nargs = self._resident_noise(noise, B, stream)
            ip, keep = None, None
            if idxs is not None:
                keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
            self._check(self._lib.fql_update_from_dataset_begin(self._h, ip, B, int(shard[0]), int(shard[1]),
                                                                C.byref(nz) if nz else None, stream))
            self._keep = (keep, nargs)

    def update_end(self, stream=None):
        self._check(self._lib.fql_update_end(self._h, None, stream))

    def update_end_split(self, stream0, stream1):
        """fql_update_end_split: Adam of gradient bucket 0 (critic, BC flow) on stream1, of bucket 1 (one-step actor) on stream0."""
        self._check(self._lib.fql_update_end_split(self._h, None, stream0, stream1))

    def grad_buckets(self):
        """[(offset, length)] x 2 in floats inside grad_buffer(), or None if the engine has no split program."""
        off, ln = (C.c_size_t * 2)(), (C.c_size_t * 2)()
        rc = self._lib.fql_grad_buckets(self._h, off, ln)
        if rc != 0:
            return None
        return [(int(off[0]), int(ln[0])), (int(off[1]), int(ln[1]))]

    def update_begin_split(self, stream0, stream1, batch=None, noise=None, idxs=None, shard=(0, 0), batch_size=None):
        """fql_update_begin_split / fql_update_from_dataset_begin_split: lane 0 on stream0, lane 1 on stream1."""
        if batch is not None:
            B, args = self._batch_args(batch)
            self._ensure_batch(B)
            nz, nargs = self._resident_noise(noise, B, stream0)
            self._check(self._lib.fql_update_begin_split(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None,
                                                         stream0, stream1))
            self._keep = (args, nargs)
        else:
            B = int(batch_size or self.config['batch_size'])
            self._ensure_batch(B)
            nz, nargs = self._resident_noise(noise, B, stream0)
            ip, keep = None, None
            if idxs is not None:
                keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
            self._check(self._lib.fql_update_from_dataset_begin_split(self._h, ip, B, int(shard[0]), int(shard[1]),
                                                                      C.byref(nz) if nz else None, stream0, stream1))
            self._keep = (keep, nargs)

    def grad_buffer(self):
        """(device pointer, number of floats) of the flat trainable-gradient buffer."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.fql_grad_buffer(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def set_grad_scale(self, scale: float):
        self._check(self._lib.fql_set_grad_scale(self._h, float(scale)))

    def set_rng_stream(self, stream_id: int):
        """Mix `stream_id` (the rank) into the device RNG key: same seed on every replica, different draws."""
        self._check(self._lib.fql_set_rng_stream(self._h, int(stream_id) & 0xFFFFFFFFFFFFFFFF))

    # -- parameters / optimizer state (reference tree layout, utils/flax_utils.py:16-50) ---------
    def leaves(self):
        out = []
        name = C.create_string_buffer(256)
        nd = C.c_int()
        shp = (C.c_int64 * 4)()
        for i in range(self._lib.fql_num_leaves(self._h)):
            self._check(self._lib.fql_leaf_info(self._h, i, name, 256, C.byref(nd), shp))
            out.append((name.value.decode(), tuple(int(shp[k]) for k in range(nd.value))))
        return out

    def _get_tree(self, getter):
        tree: Dict[str, Any] = {}
        for path, shape in self.leaves():
            a = np.empty(shape, dtype=np.float32)
            self._check(getter(path.encode(), a.ctypes.data, a.size))
            node = tree
            keys = path.split('/')
            for k in keys[:-1]:
                node = node.setdefault(k, {})
            node[keys[-1]] = a
        return tree

    def _set_tree(self, tree, setter, prefix=''):
        for k, v in tree.items():
            p = f'{prefix}/{k}' if prefix else k
            if isinstance(v, dict):
                self._set_tree(v, setter, p)
            else:
                a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
                self._check(setter(p.encode(), a.ctypes.data, a.size))

    def get_params(self):
        """agent.network.params as a nested dict of numpy arrays (reference leaf names and shapes)."""
        return self._get_tree(lambda p, d, n: self._lib.fql_get_param(self._h, p, d, n))

    def set_params(self, params):
        self._set_tree(params, lambda p, d, n: self._lib.fql_set_param(self._h, p, d, n))

    def get_opt_state(self):
        """optax.adam state: {'count', 'mu', 'nu'}."""
        c, s = C.c_int64(), C.c_int64()
        self._check(self._lib.fql_get_step(self._h, C.byref(c), C.byref(s)))
        return {'count': int(c.value), 'step': int(s.value),
                'mu': self._get_tree(lambda p, d, n: self._lib.fql_get_opt_state(self._h, 0, p, d, n)),
                'nu': self._get_tree(lambda p, d, n: self._lib.fql_get_opt_state(self._h, 1, p, d, n))}

    def set_opt_state(self, state):
        self._set_tree(state['mu'], lambda p, d, n: self._lib.fql_set_opt_state(self._h, 0, p, d, n))
        self._set_tree(state['nu'], lambda p, d, n: self._lib.fql_set_opt_state(self._h, 1, p, d, n))
        self._check(self._lib.fql_set_step(self._h, int(state['count']), int(state.get('step', state['count'] + 1))))

    def stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.fql_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {'launches_per_update': int(a.value), 'macs_per_update': int(b.value), 'param_count': int(c.value)}


_HALVES = tuple((m, 'the data-parallel update halves') for m in ('update_begin', 'update_begin_split', 'update_end', 'update_end_split'))


class KindAgent(FQLAgent):
    """What the agents of another kind than FQL share: state observations, fp32 and the engine's RNG only, and the FQL-only paths
    refused before the library is called.  A subclass names itself (`_name`), lists its `_refused` (method, reason) pairs beside the
    data-parallel halves and gradient buckets, and names the library calls (`_update_fn`, ...) of the shared methods it keeps."""

    _refused = ()
    _update_fn = _update_dataset_fn = _sample_fn = None
    _modules = {'critic': 'pair', 'target_critic': 'pair'}   # (a Gaussian actor returns a distribution object in the reference: not a query)
    _jax_sample_noise = False

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        for method, reason in _HALVES + (('grad_buckets', 'gradient buckets'),) + tuple(cls._refused):
            def refused(self, *a, _reason=reason, **k):
                raise NotImplementedError(f'{self._name}: {_reason} is not available (FQL agents only)')
            refused.__name__ = method
            setattr(cls, method, refused)

    def _probe_guard(self, what, params, rng):
        """A loss probe takes the stored parameters and the engine's or explicit noise."""
        if params is not None:
            raise NotImplementedError(f'{what} is jax.grad plumbing; use update()')
        if rng is not None:
            raise NotImplementedError(f'{self._name} draws its noise from the engine RNG or explicit tensors (noise=), not JAX keys')

    # -- reference API: `extra` is what a kind's library call takes between the noise and the info pointer (ReBRAC: the step kind) --
    def update(self, batch, noise=None, want_info=True, _extra=()):
        """The agent's update.  Returns (agent, info); info is a LazyInfo with the handle's info keys, or None with want_info=False."""
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        stream = self._stream(args + nargs)
        fn = getattr(self._lib, self._update_fn)
        self._check(fn(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, *_extra, None, stream))
        self._keep = (args, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None, _extra=()):
        """train_dataset.sample(B) + update(batch) without leaving the device."""
        B = int(batch_size or self.config['batch_size'])
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        ip, keep = None, None
        if idxs is not None:
            keep, ip = self._host_idx(idxs, B, self.dataset_size()[0], 'idxs')
        fn = getattr(self._lib, self._update_dataset_fn)
        self._check(fn(self._h, ip, B, int(shard[0]), int(shard[1]), C.byref(nz) if nz else None, *_extra, None, stream))
        self._keep = (keep, nargs)
        return self, (self._lazy_info(stream) if want_info else None)

    def read_info(self):
        """The infos of the last update (blocks until it has run)."""
        n = len(self._info_keys)
        buf = (C.c_float * n)()
        self._check(self._lib.fql_read_info_n(self._h, buf, n))
        return {k: float(buf[i]) for i, k in enumerate(self._info_keys)}

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """The kind's sample_actions on its actor's output.  [od] -> [act]; [n, od] -> [n, act].  `noises`: the raw N(0, 1) with the
        actions' shape, or None = engine RNG keyed by `seed`."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        if int(observations.shape[-1]) != od:
            raise ValueError(f'observations last dim must be {od}, got {tuple(observations.shape)}')
        lead = tuple(observations.shape[:-1])
        n = int(np.prod(lead)) if lead else 1
        o = _Arg(observations, (n, od))
        z = _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, lead + (ad,))
        fn = getattr(self._lib, self._sample_fn)
        self._check(fn(self._h, o.ptr, n, z.ptr, self._sample_seed(seed, noises), float(temperature), optr, self._stream([o, z])))
        return out


def _group_sample_args(members, observations, noises, seed, flow, per=()):
    """The shape rules of a group's fused sampling call (FQLAgentGroup, ReBRACAgentGroup, ...), checked before any library call:
    observations [K, ..., od] or one shared block without the leading K, noises [K, ..., ad] or None, seed None / one / K.  `per`: the
    dims of a row's noise in front of ad (IFQLAgentGroup's best of N: (num_samples,), noises [K, ..., N, ad]).  Returns what the library
    call takes: (observations _Arg [K, n, od], noises _Arg, seeds array or None, n, out, out pointer, stream)."""
    per = tuple(int(d) for d in per)
    K, cfg = len(members), members[0].config
    od, ad = int(cfg['ob_dims'][0]), int(cfg['action_dim'])
    is_t = hasattr(observations, 'data_ptr')
    if not is_t:
        observations = np.asarray(observations)
    oshape = tuple(int(d) for d in observations.shape)
    if not oshape or oshape[-1] != od:
        raise ValueError(f'observations last dim must be {od}, got {oshape}')
    zshape = None
    if noises is not None:
        if not hasattr(noises, 'data_ptr'):
            noises = np.asarray(noises)
        zshape = tuple(int(d) for d in noises.shape)
    if len(oshape) >= 3:
        if oshape[0] != K:
            raise ValueError(f'observations must lead with the {K} members: [{K}, ..., {od}], got {oshape}')
        shared = False
    elif zshape is not None:
        shared = len(zshape) - len(per) == len(oshape) + 1
    else:
        shared = not (len(oshape) == 2 and oshape[0] == K)
    lead = oshape[:-1] if shared else oshape[1:-1]
    if zshape is not None and zshape != (K,) + lead + per + (ad,):
        raise ValueError(f'noises must be {(K,) + lead + per + (ad,)} for observations {oshape}, got {zshape}')
    n = int(np.prod(lead)) if lead else 1
    if n < 1:
        raise ValueError(f'observations hold no rows: {oshape}')
    seeds = None
    if not flow and noises is None:
        if seed is None or np.ndim(seed) == 0:
            vals = [m._sample_seed(seed, None) for m in members]
        else:
            if len(seed) != K:
                raise ValueError(f'{K} members but {len(seed)} seeds')
            vals = [m._sample_seed(s, None) for m, s in zip(members, seed)]
        seeds = (C.c_uint64 * K)(*vals)
    if shared:   # the same rows for every member: broadcast here, the library takes one block per member
        observations = (observations.unsqueeze(0).expand((K,) + oshape) if is_t else np.broadcast_to(observations, (K,) + oshape))
    o = _Arg(observations, (K, n, od))
    z = _Arg(noises, (K, n) + per + (ad,))
    out, optr = FQLAgent._actions_out(observations, (K,) + lead + (ad,))
    return o, z, seeds, n, out, optr, FQLAgent._stream([o, z])


def _group_idx_arg(members, idxs, B, what='idxs', rows=lambda m: m.dataset_size()[0]):
    """`idxs` [K, B] of a group update (host array or tensor, CUDA tensors on torch's current stream): (keep-alive, pointer, stream).
    Host rows are range-checked against `rows(member)`, each member's dataset (or, `what` = 'replay idxs', its replay ring): an
    out-of-range row never reaches the device."""
    K = len(members)
    stream = None
    if hasattr(idxs, 'data_ptr'):
        keep = idxs.long().contiguous()
        if tuple(keep.shape) != (K, B):
            raise ValueError(f'{what} must be [{K}, {B}], got {tuple(keep.shape)}')
        if keep.is_cuda:
            h = _torch().cuda.current_stream().cuda_stream
            stream = h if h else _cabi.FQL_STREAM_LEGACY
        ip = keep.data_ptr()
    else:
        keep = np.ascontiguousarray(idxs, dtype=np.int64)
        if keep.shape != (K, B):
            raise ValueError(f'{what} must be [{K}, {B}], got {keep.shape}')
        ip = keep.ctypes.data
    if not (hasattr(keep, 'is_cuda') and keep.is_cuda):
        a = keep.numpy() if hasattr(keep, 'numpy') else keep
        for i, m in enumerate(members):
            n = rows(m)
            if B and (a[i].min() < 0 or a[i].max() >= n):
                raise ValueError(f'{what}[{i}] out of range: [{int(a[i].min())}, {int(a[i].max())}] for {n} rows')
    return keep, ip, stream


class AgentGroup:
    """What the agent groups share: K members of one structure behind one group handle of the library.  A subclass names its members'
    class (`_member`), its module's get_config (`_get_config`) and its library calls (`_create_fn`, `_update_fn`, `_sample_fn`,
    `_stats_fn` with `_stats_outs` out-values), and keeps the methods whose signature or result is its kind's own."""

    _member = _get_config = None
    _create_fn = _update_fn = _balanced_fn = _sample_fn = _flow_fn = _stats_fn = None
    _stats_outs = 2
    _sample_temperature = True   # the kind's sampling call takes a temperature

    def __init__(self, handle, members):
        self._lib = _cabi.load()
        self._g = handle
        self.members = members
        self.batch_size = int(members[0].config['batch_size'])
        self._keep = None

    @classmethod
    def _refuse(cls, cfg, *example):
        """A member config's refusals before any library call (encoder, precision, rng and the member class's own)."""
        cls._member._refuse_config(cfg)

    @classmethod
    def _create(cls, seeds, config, sweeps, *example, more=None):
        """The group of one member per seed.  `sweeps`: {config key: (K values or None = the config's for every member, plural name,
        conversion = float)}, what differs between members beside the seed; `more(cfg, K, lists)` checks and adds a kind's further
        per-member keys.  Every check runs before the library is loaded."""
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError('an agent group needs at least one seed')
        cfg = cls._get_config()
        cfg.update(dict(config))
        lists = {}
        for key, (vals, name, *conv) in sweeps.items():
            conv = conv[0] if conv else float
            lists[key] = [conv(v) for v in ([cfg[key]] * len(seeds) if vals is None else vals)]
            if len(lists[key]) != len(seeds):
                raise ValueError(f'{len(seeds)} seeds but {len(lists[key])} {name}')
        if more is not None:
            more(cfg, len(seeds), lists)
        cfgs = [dict(cfg, **{key: vals[i] for key, vals in lists.items()}) for i in range(len(seeds))]
        for c in cfgs:
            cls._refuse(c, *example)
        lib = _cabi.load()
        members = [cls._member.create(s, *example, c) for s, c in zip(seeds, cfgs)]
        arr = (C.c_void_p * len(members))(*[m._h for m in members])
        g = C.c_void_p()
        _cabi.check(lib, None, getattr(lib, cls._create_fn)(arr, len(members), C.byref(g)))
        return cls(g, members)

    def _check(self, rc):
        _cabi.check(self._lib, None, rc)

    def _batch(self, batch_size):
        B = int(batch_size or self.batch_size)
        if B != self.batch_size:
            raise ValueError(f'batch_size {B}: the members of a group keep the batch size they were grouped with ({self.batch_size})')
        return B

    def upload_dataset(self, dataset, capacity: Optional[int] = None):
        """Every member gets its own device copy of `dataset` (the member class's upload_dataset)."""
        for m in self.members:
            m.upload_dataset(dataset, capacity=capacity)

    def _update(self, B, idxs, want_info, extra=(), hold=None, after=None, info=None, balanced=False):
        """One fused update.  `extra`: what the kind's call takes between the batch size and the info pointer; `hold`: an _Arg behind
        one of them, kept alive (and, without device rows, the stream the call runs on); `after(member)`: what the step leaves in a
        member; `info(member)`: its infos, where they are not the member's _lazy_info."""
        ptrs = (None, None) if balanced else (None,)
        keep = stream = None
        if idxs is not None and balanced:
            if len(idxs) != 2:
                raise ValueError('idxs must be (dataset_idxs, replay_idxs)')
            ka, ia, sa = _group_idx_arg(self.members, idxs[0], B // 2, 'dataset idxs')
            kb, ib, sb = _group_idx_arg(self.members, idxs[1], B // 2, 'replay idxs', lambda m: m.replay_size()[0])
            ptrs, keep, stream = (ia, ib), (ka, kb), (sb if sb is not None else sa)
        elif idxs is not None:
            keep, ip, stream = _group_idx_arg(self.members, idxs, B)
            ptrs = (ip,)
        if stream is None and hold is not None:
            stream = FQLAgent._stream([hold])
        fn = getattr(self._lib, self._balanced_fn if balanced else self._update_fn)
        self._check(fn(self._g, *ptrs, B, *extra, None, stream))
        self._keep = keep if hold is None else (keep, hold)
        if after is not None:
            for m in self.members:
                after(m)
        if not want_info:
            return None
        return [info(m) if info is not None else m._lazy_info(None) for m in self.members]

    def update_from_dataset(self, batch_size=None, idxs=None, want_info=False):
        """One fused update of every member: rows from each member's dataset (`idxs` [K, B] int, host or device, or None = each member's
        device RNG), noise from each member's device RNG.  Returns a list of K LazyInfo with the members' info keys (want_info) or None."""
        return self._update(self._batch(batch_size), idxs, want_info)

    def _noise_per(self):
        """The dims of a row's sampling noise in front of the action dim."""
        return ()

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """The member class's sample_actions of every member in ONE fused call: result[i] is bitwise what
        members[i].sample_actions(observations[i], seed=..., temperature=..., noises=noises[i]) returns.  Shapes and seeds as in
        FQLAgentGroup.sample_actions: observations [K, ..., od] or one shared block, noises [K, ..., ad] or None, seed None (each
        member's own counter advances), one seed or K seeds.  Returns [K, ..., ad]."""
        o, z, seeds, n, out, optr, stream = _group_sample_args(self.members, observations, noises, seed, False, per=self._noise_per())
        t = (float(temperature),) if self._sample_temperature else ()
        self._check(getattr(self._lib, self._sample_fn)(self._g, o.ptr, n, z.ptr, seeds, *t, optr, stream))
        return out

    def _flow_actions(self, observations, noises):
        """compute_flow_actions of every member in one fused call (`_flow_fn`): noises [K, ..., ad]."""
        if noises is None:
            raise ValueError('compute_flow_actions needs noises [K, ..., action_dim]')
        o, z, _, n, out, optr, stream = _group_sample_args(self.members, observations, noises, None, True)
        self._check(getattr(self._lib, self._flow_fn)(self._g, o.ptr, z.ptr, n, optr, stream))
        return out

    def launches(self):
        """Kernel launches of the group's fused update program(s), then of its fused sampling call(s) on a single chunk, as the
        kind's stats call counts them from the built programs."""
        if self._stats_fn is None:
            raise NotImplementedError(f'{type(self).__name__} counts its sampling launches with sample_launches()')
        outs = [C.c_int64(0) for _ in range(self._stats_outs)]
        self._check(getattr(self._lib, self._stats_fn)(self._g, *[C.byref(v) for v in outs]))
        return tuple(int(v.value) for v in outs)

    def synchronize(self):
        """Host wait for the group's last update or sampling call."""
        self._check(self._lib.fql_group_synchronize(self._g))

    def close(self):
        """Destroy the fused program(s); the members stay usable as standalone agents.  A second close is a no-op."""
        if getattr(self, '_g', None):
            self._lib.fql_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FQLAgentGroup(AgentGroup):
    """K agents of one structure - the same config except `seed` and `alpha` - trained side by side by ONE fused update program
    (include/fql_amd.h, fql_group_*): every launch of the update carries all K members' tasks.  The seed / alpha sweeps the reference
    recommends (README "Tips for hyperparameter tuning") on one device:

        group = FQLAgentGroup.create([0, 1, 2], ex_obs, ex_act, config, alphas=[0.3, 3, 30])
        group.upload_dataset(train_dataset)
        for step in range(n):
            infos = group.update_from_dataset(want_info=(step % log_every == 0))

    `members` are ordinary FQLAgent objects (sample_actions, total_loss, get/set_params, checkpoints, ...); a member's trajectory is
    bitwise the one it has when trained alone with the same seed, alpha, rows and noise.  Members are state agents with precision 'fp32'
    and the engine's device RNG; while grouped their batch size is fixed."""

    _member, _get_config = FQLAgent, staticmethod(get_config)
    _create_fn, _update_fn, _sample_fn, _flow_fn = 'fql_group_create', 'fql_group_update_from_dataset', 'fql_group_sample_actions', 'fql_group_flow_actions'
    _sample_temperature = False
    _other_groups = {'sac': 'SAC', 'iql': 'IQL', 'cfgrl': 'CFGRL'}   # agent_name -> the kind whose own group class takes such a config

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, alphas=None):
        return cls._create(seeds, config, {'alpha': (alphas, 'alphas')}, ex_observations, ex_actions)

    @classmethod
    def _refuse(cls, cfg, *example):
        kind = cls._other_groups.get(cfg.get('agent_name'))
        if kind:
            raise NotImplementedError(f'agent groups take FQL agents only ({kind} agents are grouped by {kind}AgentGroup)')
        if cfg.get('encoder') is not None:
            raise NotImplementedError('agent groups take state agents only (encoder=None)')
        if cfg.get('precision', 'fp32') not in ('fp32', 0):
            raise NotImplementedError("agent groups take precision='fp32' members only")
        if cfg.get('rng') is not None and cfg.get('rng') != 'engine':
            raise NotImplementedError(f"agent groups draw rows and noise from the engine's device RNG; rng={cfg.get('rng')!r} is not supported")

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """FQLAgent.sample_actions of every member in ONE fused call (fql_group_sample_actions): result[i] is bitwise what
        members[i].sample_actions(observations[i], seed=..., noises=noises[i]) returns.

        observations: [K, ..., od], one block of rows per member (each member acts in its own environments), or one block without the
        leading K - [od], [n, od] - that every member acts on.  An array of three or more dims must lead with K; a 2-D array of exactly K
        rows is read as one row per member.  noises: [K, ..., ad] or None.  seed: None, one seed (every member is keyed with it as its own
        call would be) or a sequence of K; with neither seed nor noises each member's own sample counter advances as its own call would
        advance it.  numpy in, numpy out; CUDA tensors in, a CUDA tensor out on torch's current stream.  `temperature` is accepted and
        ignored, as in FQLAgent.  Returns [K, ..., ad]."""
        return super().sample_actions(observations, seed, temperature, noises)

    def compute_flow_actions(self, observations, noises):
        """FQLAgent.compute_flow_actions of every member in one fused call (fql_group_flow_actions); shapes as in sample_actions."""
        return self._flow_actions(observations, noises)

    def sample_launches(self, flow=False):
        """Kernel launches of one fused sampling call on a single chunk, counted from the built program (fql_group_sample_stats)."""
        v = C.c_int64(0)
        self._check(self._lib.fql_group_sample_stats(self._g, int(bool(flow)), C.byref(v)))
        return int(v.value)
