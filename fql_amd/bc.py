"""Host-side mirror of the reference's BCAgent (agents/bc.py) over the C ABI: flow-matching behavioural cloning.

The policy is MLP(hidden_dims, GELU, LayerNorm) + Dense(action_dim) on [obs | x_t | emb(t)], emb the 16-wide sinusoidal timestep embedding
(agents/bc.py:15-24); t lies on the grid {0, 1/S, ..., 1}, S = denoise_steps.  sample_actions is S Euler steps and a clip (:86-101).
Same call sites as the reference:

    agent = BCAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch)                      # info: LazyInfo with BC_INFO_KEYS
    loss, info = agent.policy_loss(batch)
    action = agent.sample_actions(observations=ob, seed=key)

State observations, fp32 and GELU only: `encoder`, precision 'bf16x3', another `activation` and rng other than 'engine' are refused
here, before the library is called.  Datasets, checkpoints (TrainState key 'policy'), get/set_params and synchronize are FQLAgent's
plumbing on a BC handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi
from .agent import KindAgent, _Arg, _PendingN
from .config import ConfigDict

BC_INFO_KEYS = ('bc_loss', 'grad/max', 'grad/min', 'grad/norm')
BC_NOISE_KEYS = ('x0', 't')
EMB_SIZE = 16
MAX_PERIOD = 10000


def timestep_embedding(k, denoise_steps):
    """The engine's embedding of t = k / S (agents/bc.py:15-24, pinned): freq_i = float32(exp_f64(-ln(10000) i / 8)),
    arg = float32(float32(t 10000) freq_i), [cos(arg) | sin(arg)] in fp64 of that fp32 argument, rounded to fp32.  k: ints, any shape."""
    k = np.asarray(k)
    half = EMB_SIZE // 2
    t = k.astype(np.float32) / np.float32(denoise_steps)
    ts = (t * np.float32(MAX_PERIOD)).astype(np.float32)
    freqs = np.exp(-np.log(float(MAX_PERIOD)) * np.arange(half, dtype=np.float64) / half).astype(np.float32)
    args = (ts[..., None] * freqs).astype(np.float32)
    return np.concatenate([np.cos(args.astype(np.float64)), np.sin(args.astype(np.float64))], axis=-1).astype(np.float32)


def grid_index(t, denoise_steps):
    """k with t = k / S; ValueError when a t is off the grid {0, 1/S, ..., 1}."""
    t = np.asarray(t, dtype=np.float64)
    ts = t * denoise_steps
    k = np.rint(ts)
    if t.size and (np.any(k < 0) or np.any(k > denoise_steps) or np.any(np.abs(ts - k) > 1e-3)):
        raise ValueError(f't must lie on the grid {{0, 1/{denoise_steps}, ..., 1}} (agents/bc.py:61)')
    return k.astype(np.int64)


def get_config():
    """agents/bc.py:135-148 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='bc',
        batch_size=256,
        hidden_dims=(512, 512, 512, 512),
        bc_lr=3e-4,
        use_layer_norm=1,
        activation='gelu',
        denoise_steps=16,
        rng='engine',  # not a reference key: device Philox noise (the only source BC supports)
        precision='fp32',  # not a reference key: BC runs in fp32 only
    )


class BCAgent(KindAgent):
    """Flow-matching BC agent backed by the MI355X step engine.  update: agents/bc.py:72-84, 4 infos (BC_INFO_KEYS)."""

    _name = 'BC'
    _modules = {}   # network.select: the policy's input carries the host-built time embedding
    _refused = (('total_loss', 'total_loss (BCAgent has policy_loss)'),
                ('compute_flow_actions', 'compute_flow_actions (sample_actions(noises=) is the flow)'),
                ('create_replay_buffer', 'the replay ring'), ('update_balanced', 'balanced sampling'))
    _update_fn, _update_dataset_fn = 'fql_bc_update', 'fql_bc_update_from_dataset'
    _loss_infos = 1
    _pending_cls = _PendingN
    _train_state_key = 'policy'   # agents/bc.py:45: the TrainState's field name (checkpoint layout)

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/bc.py:103-132.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        if cfg.get('activation', 'gelu') != 'gelu':
            raise NotImplementedError(f"BC: only activation 'gelu' is built (got {cfg['activation']!r})")
        cls._refuse_config(cfg)
        if int(cfg['denoise_steps']) < 1:
            raise ValueError('denoise_steps must be >= 1')
        lib = _cabi.load()
        # fql_config mapping (include/fql_amd.h): hidden_dims -> actor_hidden, use_layer_norm -> actor_layer_norm, bc_lr -> lr
        ec = dict(actor_hidden_dims=tuple(cfg['hidden_dims']), value_hidden_dims=tuple(cfg['hidden_dims']), layer_norm=False,
                  actor_layer_norm=bool(cfg['use_layer_norm']), lr=cfg['bc_lr'], discount=0.99, tau=0.005, flow_steps=1,
                  batch_size=cfg['batch_size'], precision='fp32', encoder=None)
        c, ob_dims, action_dim = cls._engine_config(lib, ec, ex_observations, ex_actions)
        bc = _cabi.FqlBcConfig()
        lib.fql_bc_default_config(C.byref(bc))
        bc.denoise_steps = int(cfg['denoise_steps'])
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_bc_create(C.byref(c), C.byref(bc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        return cls(h, cfg, int(seed))

    def _batch_args(self, batch):   # BC batches carry observations and actions only
        for k in ('observations', 'actions'):
            if k not in batch:
                raise KeyError(f'batch is missing {k!r}')
        B = int(batch['actions'].shape[0]) if hasattr(batch['actions'], 'shape') else int(np.shape(batch['actions'])[0])
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        return B, [_Arg(batch['observations'], (B, od)), _Arg(batch['actions'], (B, ad))]

    def _noise_args(self, noise, B):
        """Explicit x0 [B, act] and t [B] (agents/bc.py:60-61); other keys are refused, and so is a t off the grid."""
        if noise is None:
            return None, []
        extra = set(noise) - set(BC_NOISE_KEYS)
        if extra:
            raise ValueError(f'BC reads only {BC_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        t = noise.get('t')
        if t is not None:
            grid_index(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, int(self.config['denoise_steps']))
        ad = self.config['action_dim']
        x0, ta = _Arg(noise.get('x0'), (B, ad)), _Arg(t, (B,))
        return _cabi.FqlNoise(None, x0.ptr, ta.ptr, None, None), [x0, ta]

    def policy_loss(self, batch, policy_params=None, rng=None, noise=None):
        """agents/bc.py:48-70 with the stored parameters (the validation probe of train_bc_agent): (loss, {'bc_loss': loss}).
        No state changes."""
        self._probe_guard('policy_loss with traced policy_params', policy_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        self._check(self._lib.fql_bc_policy_loss(self._h, args[0].ptr, args[1].ptr, B, C.byref(nz) if nz else None, C.byref(loss),
                                                 self._stream(args + nargs)))
        return float(loss.value), {'bc_loss': float(loss.value)}

    def sample_actions(self, observations, seed=None, temperature=1.0, noises=None):
        """agents/bc.py:86-101: x ~ N(0, I), denoise_steps Euler steps, clip.  [od] and [1, od] -> [act] (the reference's squeeze);
        [n, od] -> [n, act], row by row the single-observation result.  `noises`: x with the shape [n, act] (or [act]), or None = engine
        RNG keyed by `seed`.  `temperature` is accepted and ignored, as in the reference."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        if not hasattr(observations, 'shape'):
            observations = np.asarray(observations, dtype=np.float32)
        if int(observations.shape[-1]) != od or len(observations.shape) > 2:
            raise ValueError(f'observations must be [{od}] or [n, {od}], got {tuple(observations.shape)}')
        n = int(observations.shape[0]) if len(observations.shape) == 2 else 1
        shape = (ad,) if n == 1 else (n, ad)
        o = _Arg(observations, (n, od))
        z = _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, shape)
        self._check(self._lib.fql_bc_sample_actions(self._h, o.ptr, n, z.ptr, self._sample_seed(seed, noises), optr, self._stream([o, z])))
        return out

    def bc_stats(self):
        """(launches of one update, MACs of one update, launches of one sampling call of <= 4096 rows)."""
        la, ma, ls = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.fql_bc_stats(self._h, C.byref(la), C.byref(ma), C.byref(ls)))
        return int(la.value), int(ma.value), int(ls.value)


def train_bc(agent, dataset, steps, log_every, val_dataset=None, val_batch_size=None, log=None):
    """utils/train.py::train_bc_agent's loop without wandb, environments and rollouts: `steps` device-resident updates on `dataset`
    (uploaded once), the infos of every `log_every`-th step read lazily, and policy_loss on `val_dataset` rows at the same steps.
    Returns the list of logged rows [{'step', 'training/<info>', 'validation/bc_loss'?}].  `log(row)` is called per row when given."""
    agent.upload_dataset(dataset)
    B = int(agent.config['batch_size'])
    rows, pending = [], []
    rs = np.random.RandomState(agent._seed & 0x7FFFFFFF)

    def flush():   # lazily: the infos are read long after their updates were enqueued
        for row, info in pending:
            row.update({f'training/{k}': float(v) for k, v in info.items()})
            if log is not None:
                log(row)
        pending.clear()

    for i in range(1, int(steps) + 1):
        want = i % int(log_every) == 0
        _, info = agent.update_from_dataset(B, want_info=want)
        if not want:
            continue
        row = {'step': i}
        pending.append((row, info))
        if val_dataset is not None:
            vb = int(val_batch_size or B)
            idx = rs.randint(val_dataset.size, size=vb)
            batch = {k: np.asarray(val_dataset[k])[idx] for k in ('observations', 'actions')}
            row['validation/bc_loss'] = agent.policy_loss(batch)[0]
            agent._ensure_batch(B)
        rows.append(row)
        if len(pending) >= 32:   # the engine keeps 64 info snapshots: read before they expire
            flush()
    flush()
    return rows


__all__ = ['BCAgent', 'BC_INFO_KEYS', 'BC_NOISE_KEYS', 'get_config', 'timestep_embedding', 'grid_index', 'train_bc']
