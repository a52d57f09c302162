"""Host-side mirror of the reference's IQLDiffusionAgent (agents/iql_diffusion.py) over the C ABI: IQL critics (expectile value, critic
pair with a Polyak target) under an optimality-conditioned flow actor sampled with classifier-free guidance.  The BINARY optimality
family: optimal_var in {'binary', 'binary_awr_loss', 'binary_softmax_loss'}, whose actor is DiffusionPolicy with nn.Embed(2, 32).
Same call sites as the reference's main.py:

    agent = IQLDiffusionAgent.create(seed, ex_observations, ex_actions, config)
    agent, info = agent.update(batch, update_critic=True, update_actor=True)
    loss, info = agent.total_loss(val_batch, grad_params=None)
    action = agent.sample_actions(observations=ob, seed=key, temperature=1, cfg=3.0, o=1.0)

Refused here, before the library is called: optimal_var 'softmax' / 'sampled_adv_softmax' (the continuous policy, which needs an external
bc_agent), opt_decay_schedule 'cosine', an encoder, precision other than fp32, an activation other than GELU, goal conditioning and rng
other than 'engine'.  Datasets, get/set_params and synchronize are FQLAgent's plumbing on the handle; checkpoints carry the reference's
fields rng / critic / target_critic / value / actor (fql_amd/checkpoint.py).

IQLDiffusionAgentGroup advances K such agents - one config but for seed, awr_temperature and softmax_beta - with one fused program per
step kind and samples them in one fused call (fql_iqld_group_*).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi
from .agent import AgentGroup, FQLAgent, KindAgent, LazyInfo, _Arg, _PendingN, _group_sample_args
from .bc import grid_index
from .config import ConfigDict

OPTIMAL_VARS = ('binary', 'binary_awr_loss', 'binary_softmax_loss')
_CONTINUOUS = ('softmax', 'sampled_adv_softmax')
# the 21 scalars in the handle's buffer order (fql_handle_info_name)
IQLD_INFO_KEYS = ('critic_loss', 'q', 'value_loss', 'v', 'v_min', 'v_max', 'actor_q', 'actor_loss', 'actor_positive_ratio',
                  'actor_loss_positive', 'actor_loss_uncond', 'o_mean', 'o_std', 'o_min', 'o_max', 'effective_batch_size',
                  'loss_weights_top_10_mass', 'loss_weights_max', 'grad/max', 'grad/min', 'grad/norm')
IQLD_ROW_KEYS = ('actor_losses', 'o', 'loss_weights')
IQLD_NOISE_KEYS = ('x0', 't')
_GRAD = ('grad/max', 'grad/min', 'grad/norm')
_CRITIC = ('critic_loss', 'q')
_VALUE = ('value_loss', 'v', 'v_min', 'v_max')
# agents/iql_diffusion.py:197-213: the actor's info dict as it is written, the per-row arrays among the scalars
_ACTOR = ('actor_q', 'actor_loss', 'actor_positive_ratio', 'actor_loss_positive', 'actor_loss_uncond', 'actor_losses', 'o_mean', 'o_std',
          'o_min', 'o_max', 'o', 'effective_batch_size', 'loss_weights_top_10_mass', 'loss_weights_max', 'loss_weights')


def info_keys(update_critic=True, update_actor=True, grads=True):
    """The keys one step kind returns, in the reference's insertion order: {**critic_info, **value_info, **actor_info}, where
    apply_loss_fn appends grad/* to each net's infos and a later dict only overwrites the values of keys an earlier one inserted.  So
    grad/* sit behind the critic's keys when the critic steps (holding the value net's, then the actor's statistics) and behind the
    actor's keys on an actor-only step.  grads=False: total_loss (no grad statistics)."""
    keys = []
    if update_critic:
        keys += list(_CRITIC) + (list(_GRAD) if grads else []) + list(_VALUE)
    if update_actor:
        keys += list(_ACTOR) + (list(_GRAD) if grads and not update_critic else [])
    return tuple(keys)


def get_config():
    """agents/iql_diffusion.py:362-396 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='iql_diffusion',
        batch_size=256,
        goal_conditioned=0,
        actor_lr=3e-4,
        value_lr=3e-4,
        critic_lr=3e-4,
        num_qs=2,
        actor_hidden_dims=(512, 512, 512, 512),
        hidden_dims=(512, 512, 512, 512),
        discount=0.99,
        expectile=0.9,
        dropout_rate=0,
        use_tanh=0,
        state_dependent_std=0,
        use_layer_norm=1,
        activation='gelu',
        fixed_std=0,
        tau=0.005,
        opt_decay_schedule='none',
        target_extraction=1,
        denoise_steps=16,
        action_distribution='data',
        critic_train_steps=None,
        actor_start_steps=None,
        total_steps=None,
        optimal_var='binary_awr_loss',
        awr_temperature=0.1,
        softmax_beta=3.0,
        encoder=None,   # not a reference key: state observations only
        rng='engine',  # not a reference key: device Philox noise or explicit tensors
        precision='fp32',  # not a reference key: fp32 only
    )


def as_array(x):
    """`x` itself when it has a shape (numpy array, torch tensor), else a float32 numpy array of it."""
    return x if hasattr(x, 'shape') else np.asarray(x, dtype=np.float32)


def check_cfgs(cfgs, n, per):
    """[n] finite guidance weights (numpy or torch), or ValueError: the checks of both CFG samplers' per-row calls."""
    cfgs = as_array(cfgs)
    if len(cfgs.shape) != 1 or int(cfgs.shape[0]) != n:
        raise ValueError(f'cfgs must hold one guidance weight per {per}: [{n}], got {tuple(cfgs.shape)}')
    finite = cfgs.isfinite().all() if hasattr(cfgs, 'data_ptr') else np.isfinite(np.asarray(cfgs, dtype=np.float64)).all()
    if not bool(finite):
        raise ValueError('cfgs: every guidance weight must be finite')
    return cfgs


def sweep_inputs(cfgs, items):
    """The flatten and repeat of sample_actions_sweep.  cfgs: [G], G >= 1.  items: (name, array, width[, one_ok]) tuples, the first
    the observations: each array is [n, width] (shared by every weight), [G, n, width], None, or with one_ok one [width] row for
    every row.  Returns G, n, the arrays as [G n, width] with row g n + j = (weight g, row j), and the weights repeated to [G n]."""
    cfgs = as_array(cfgs)
    if len(cfgs.shape) != 1 or int(cfgs.shape[0]) < 1:
        raise ValueError(f'cfgs must be [G] with G >= 1 (an empty sweep has no rows), got {tuple(cfgs.shape)}')
    G = int(cfgs.shape[0])
    check_cfgs(cfgs, G, 'sweep entry')
    ob, od = as_array(items[0][1]), items[0][2]
    sh = tuple(int(d) for d in ob.shape)
    if len(sh) not in (2, 3) or sh[-1] != od or sh[-2] < 1 or (len(sh) == 3 and sh[0] != G):
        raise ValueError(f'observations must be [n, {od}] or [{G}, n, {od}] with n >= 1, got {sh}')
    n = sh[-2]
    flat = []
    for name, x, w, *one_ok in items:
        if x is None:
            flat.append(None)
            continue
        x = as_array(x)
        sh = tuple(int(d) for d in x.shape)
        if one_ok and one_ok[0] and sh in ((w,), (1, w)):
            x, sh = x.reshape(1, w).expand(n, w) if hasattr(x, 'data_ptr') else np.broadcast_to(np.reshape(x, (1, w)), (n, w)), (n, w)
        if sh == (n, w):
            x = x.unsqueeze(0).expand(G, n, w) if hasattr(x, 'data_ptr') else np.broadcast_to(x[None], (G, n, w))
        elif sh != (G, n, w):
            raise ValueError(f'{name} must be [{n}, {w}] or [{G}, {n}, {w}], got {sh}')
        flat.append(x.reshape(G * n, w))
    rep = cfgs.repeat_interleave(n) if hasattr(cfgs, 'data_ptr') else np.repeat(np.asarray(cfgs, dtype=np.float32), n)
    return G, n, flat, rep


class _Rows:
    """One per-row info array of an update, read from the engine on first use (fql_iqld_read_rows) and cached.  The engine keeps the
    rows of the LAST actor step only: a first read after a later actor step raises instead of returning that later step's rows."""

    def __init__(self, agent, which, n):
        self._agent, self._which, self._n, self._a = agent, which, n, None
        self._step = agent._actor_steps

    def get(self):
        if self._a is None:
            if self._agent._actor_steps != self._step:
                raise RuntimeError('the per-row infos of this update were not read before a later actor step overwrote them '
                                   '(read them, or info.to_dict(), before the next update_actor step)')
            self._a = self._agent._read_rows(self._which, self._n)
            self._agent = None
        return self._a

    def __array__(self, dtype=None, copy=None):
        return self.get() if dtype is None else self.get().astype(dtype)

    def __len__(self): return self._n
    def __getitem__(self, i): return self.get()[i]
    def __repr__(self): return repr(self.get())


class StepInfo(LazyInfo):
    """The info dict of one step kind: LazyScalar values, and _Rows for the per-row arrays.  to_dict() gives floats and numpy arrays."""

    def __init__(self, items):
        dict.__init__(self, items)

    def to_dict(self):
        return {k: (v.get() if isinstance(v, _Rows) else float(v)) for k, v in self.items()}


class IQLDiffusionAgent(KindAgent):
    """IQL-diffusion agent backed by the MI355X step engine."""

    _name = 'IQL-diffusion'
    _modules = {'critic': 'pair', 'target_critic': 'pair', 'value': 'value'}   # (the actor's input carries host-built embeddings)
    _refused = (('compute_flow_actions', 'compute_flow_actions (sample_actions(noises=) is the flow)'),
                ('create_replay_buffer', 'the replay ring'), ('update_balanced', 'balanced sampling'))
    _update_dataset_fn = 'fql_iqld_update_from_dataset'
    _pending_cls = _PendingN
    _train_states = ('actor', 'critic', 'target_critic', 'value')   # agents/iql_diffusion.py:87-91: bare fields (checkpoint layout)
    _actor_steps = 0   # actor steps issued through this object: a _Rows remembers the one it belongs to

    @classmethod
    def create(cls, seed, ex_observations, ex_actions, config):
        """agents/iql_diffusion.py:287-359.  `config`: dict-like with the keys of get_config()."""
        cfg = get_config()
        cfg.update(dict(config))
        ov = cfg['optimal_var']
        if ov in _CONTINUOUS:
            raise NotImplementedError(f"IQL-diffusion: optimal_var {ov!r} (the continuous policy with an external bc_agent) is not built; "
                                      f'the binary family only: {OPTIMAL_VARS}')
        if ov not in OPTIMAL_VARS:
            raise ValueError(f'Invalid optimal_var: {ov}')
        if cfg['opt_decay_schedule'] not in ('none', None):
            raise NotImplementedError(f"IQL-diffusion: opt_decay_schedule {cfg['opt_decay_schedule']!r} is not built (a constant actor_lr only)")
        if cfg.get('activation', 'gelu') != 'gelu':
            raise NotImplementedError(f"IQL-diffusion: only activation 'gelu' is built (got {cfg['activation']!r})")
        if cfg.get('goal_conditioned'):
            raise NotImplementedError('IQL-diffusion: goal conditioning is not built')
        if int(cfg.get('num_qs', 2)) != 2:
            raise NotImplementedError('IQL-diffusion: num_qs must be 2')
        cls._refuse_config(cfg)
        lib = _cabi.load()
        ln = bool(cfg['use_layer_norm'])
        ec = dict(actor_hidden_dims=tuple(cfg['actor_hidden_dims']), value_hidden_dims=tuple(cfg['hidden_dims']), layer_norm=ln,
                  actor_layer_norm=ln, lr=cfg['critic_lr'], discount=cfg['discount'], tau=cfg['tau'], flow_steps=1,
                  batch_size=cfg['batch_size'], precision='fp32', encoder=None)
        c, ob_dims, action_dim = cls._engine_config(lib, ec, ex_observations, ex_actions)
        dc = _cabi.FqlIqldConfig()
        lib.fql_iqld_default_config(C.byref(dc))
        dc.actor_lr, dc.value_lr, dc.critic_lr = float(cfg['actor_lr']), float(cfg['value_lr']), float(cfg['critic_lr'])
        dc.expectile, dc.awr_temperature, dc.softmax_beta = float(cfg['expectile']), float(cfg['awr_temperature']), float(cfg['softmax_beta'])
        dc.optimal_var, dc.target_extraction = OPTIMAL_VARS.index(ov), int(bool(cfg['target_extraction']))
        dc.denoise_steps, dc.opt_decay_schedule = int(cfg['denoise_steps']), 0
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_iqld_create(C.byref(c), C.byref(dc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        return cls(h, cfg, int(seed))

    def _noise_args(self, noise, B):
        """Explicit x0 [B, act] and t [B] on the grid (agents/iql_diffusion.py:174-175); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(IQLD_NOISE_KEYS)
        if extra:
            raise ValueError(f'IQL-diffusion reads only {IQLD_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        t = noise.get('t')
        if t is not None:
            grid_index(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, int(self.config['denoise_steps']))
        ad = self.config['action_dim']
        x0, ta = _Arg(noise.get('x0'), (B, ad)), _Arg(t, (B,))
        return _cabi.FqlNoise(None, x0.ptr, ta.ptr, None, None), [x0, ta]

    def _read_rows(self, which, n):
        a = np.empty(n, np.float32)
        self._check(self._lib.fql_iqld_read_rows(self._h, int(which), a.ctypes.data, n))
        return a

    def _step_info(self, stream, update_critic, update_actor, B):
        """The reference's info dict of this step kind: lazily read scalars, and the three per-row arrays when the actor stepped."""
        lazy = self._lazy_info(stream)   # all 21 scalars of the handle, in buffer order
        return StepInfo((k, _Rows(self, IQLD_ROW_KEYS.index(k), B) if k in IQLD_ROW_KEYS else lazy[k])
                        for k in info_keys(update_critic, update_actor))

    def update(self, batch, update_critic=True, update_actor=True, bc_agent=None, noise=None, want_info=True):
        """agents/iql_diffusion.py:215-247.  Returns (agent, info); info holds the keys of the nets that stepped (info_keys)."""
        if bc_agent is not None:
            raise NotImplementedError('IQL-diffusion: bc_agent belongs to the continuous optimal_var family, which is not built')
        uc, ua = bool(update_critic), bool(update_actor)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        stream = self._stream(args + nargs)
        self._check(self._lib.fql_iqld_update(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, int(uc), int(ua), None, stream))
        self._keep = (args, nargs)
        self._actor_steps += int(ua)
        return self, (self._step_info(stream, uc, ua, B) if want_info else None)

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None,
                            update_critic=True, update_actor=True):
        """train_dataset.sample(B) + update(batch, update_critic, update_actor) without leaving the device."""
        uc, ua = bool(update_critic), bool(update_actor)
        B = int(batch_size or self.config['batch_size'])
        super().update_from_dataset(batch_size, idxs, noise, shard, False, stream, _extra=(int(uc), int(ua)))
        self._actor_steps += int(ua)
        return self, (self._step_info(stream, uc, ua, B) if want_info else None)

    def read_info(self, update_critic=True, update_actor=True):
        """The scalars of the last update (blocks until it has run); with the step kind given, its keys only, in the reference's order."""
        all21 = super().read_info()
        return {k: all21[k] for k in info_keys(update_critic, update_actor) if k not in IQLD_ROW_KEYS}

    def total_loss(self, batch, grad_params=None, rng=None, bc_agent=None, noise=None):
        """agents/iql_diffusion.py:272-285 with the stored parameters (the validation probe of main.py): (critic + value + actor loss,
        every info but grad/*).  No state changes."""
        if bc_agent is not None:
            raise NotImplementedError('IQL-diffusion: bc_agent belongs to the continuous optimal_var family, which is not built')
        self._probe_guard('total_loss with traced grad_params', grad_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        loss = C.c_float()
        n = len(IQLD_INFO_KEYS) - 3
        buf = (C.c_float * n)()
        self._check(self._lib.fql_iqld_total_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, C.byref(loss), buf,
                                                  self._stream(args + nargs)))
        vals = {k: float(buf[i]) for i, k in enumerate(IQLD_INFO_KEYS[:n])}
        info = {}
        for k in info_keys(True, True, grads=False):
            info[k] = self._read_rows(3 + IQLD_ROW_KEYS.index(k), B) if k in IQLD_ROW_KEYS else vals[k]
        return float(loss.value), info

    def sample_actions(self, observations, seed=None, temperature=1.0, cfg=1.0, o=1.0, noises=None):
        """agents/iql_diffusion.py:249-270: x ~ N(0, I); denoise_steps times v = v_unc + cfg (v_pos - v_unc), x += v / S; clip.  [od]
        and [1, od] -> [act] (the reference's squeeze); [n, od] -> [n, act], row by row the single-observation result.  `noises`: x
        with the shape [n, act] (or [act]), or None = engine RNG keyed by `seed`.  `temperature` and `o` are accepted and not read, as
        in the reference for the binary family."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        if not hasattr(observations, 'shape'):
            observations = np.asarray(observations, dtype=np.float32)
        if int(observations.shape[-1]) != od or len(observations.shape) > 2:
            raise ValueError(f'observations must be [{od}] or [n, {od}], got {tuple(observations.shape)}')
        n = int(observations.shape[0]) if len(observations.shape) == 2 else 1
        shape = (ad,) if n == 1 else (n, ad)
        ob = _Arg(observations, (n, od))
        z = _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, shape)
        self._check(self._lib.fql_iqld_sample_actions(self._h, ob.ptr, n, z.ptr, self._sample_seed(seed, noises), float(cfg), optr,
                                                      self._stream([ob, z])))
        return out

    # -- guidance sweeps: one weight per row --------------------------------------------------------
    def sample_actions_rows(self, observations, cfgs, seed=None, noises=None):
        """sample_actions with one guidance weight per row, in ONE call: observations [N, od], cfgs [N] -> [N, act] (no squeeze).  Row
        j is, bit for bit, sample_actions(observations[j], cfg=cfgs[j], noises=noises[j]); with engine noise (`noises=None`) row j draws
        what row j of sample_actions(observations, seed=seed) draws.  A call costs 4 + S nl + 1 launches whatever N <= 2048 is."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        observations = as_array(observations)
        if len(observations.shape) != 2 or int(observations.shape[1]) != od or int(observations.shape[0]) < 1:
            raise ValueError(f'observations must be [N, {od}] with N >= 1, got {tuple(observations.shape)}')
        n = int(observations.shape[0])
        cfgs = check_cfgs(cfgs, n, 'row')
        if noises is not None and tuple(as_array(noises).shape) != (n, ad):
            raise ValueError(f'noises must be [{n}, {ad}], got {tuple(as_array(noises).shape)}')
        ob, w, z = _Arg(observations, (n, od)), _Arg(cfgs, (n,)), _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, (n, ad))
        self._check(self._lib.fql_iqld_sample_actions_cfgs(self._h, ob.ptr, n, z.ptr, self._sample_seed(seed, noises), w.ptr, optr,
                                                           self._stream([ob, z, w])))
        return out

    def sample_actions_sweep(self, observations, cfgs, seed=None, noises=None):
        """Every weight of an evaluation sweep in one call: cfgs [G] -> [G, n, act], slice g = sample_actions(.., cfg=cfgs[g]).
        observations: [n, od] (every weight sees the same rows) or [G, n, od] (one vector env per weight).  noises: None (engine RNG:
        row g n + j of the flat call), [n, act] (shared by every weight: common random numbers) or [G, n, act]."""
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        G, n, (ob, z), w = sweep_inputs(cfgs, [('observations', observations, od), ('noises', noises, ad)])
        return self.sample_actions_rows(ob, w, seed=seed, noises=z).reshape(G, n, ad)

    def sample_cfgs_stats(self):
        """Launches of one sample_actions_rows / sample_actions_sweep call of <= 2048 rows."""
        ls = C.c_int64()
        self._check(self._lib.fql_sample_cfgs_stats(self._h, C.byref(ls)))
        return int(ls.value)

    # -- per-TrainState optimizer state ------------------------------------------------------------
    def get_steps(self):
        """{'updates': RNG step, 'critic': the critic's and value net's Adam count, 'actor': the actor's}."""
        s = (C.c_int64 * 3)()
        self._check(self._lib.fql_iqld_get_steps(self._h, s))
        return {'updates': int(s[0]), 'critic': int(s[1]), 'actor': int(s[2])}

    def set_steps(self, updates, critic, actor):
        self._check(self._lib.fql_iqld_set_steps(self._h, (C.c_int64 * 3)(int(updates), int(critic), int(actor))))

    def get_opt_state(self):
        """{'count', 'step'} of the critic (and value) TrainState, 'actor_count', 'updates', and the moment trees of every leaf."""
        st = super().get_opt_state()
        s = self.get_steps()
        st.update(actor_count=s['actor'], updates=s['updates'])
        return st

    def set_opt_state(self, state):
        self._set_tree(state['mu'], lambda p, d, n: self._lib.fql_set_opt_state(self._h, 0, p, d, n))
        self._set_tree(state['nu'], lambda p, d, n: self._lib.fql_set_opt_state(self._h, 1, p, d, n))
        c = int(state['count'])
        self.set_steps(int(state.get('updates', c)), c, int(state.get('actor_count', c)))

    def iqld_stats(self, update_critic=True, update_actor=True):
        """(launches of one update of that step kind, its MACs, launches of one sampling call of <= 2048 observations)."""
        la, ma, ls = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.fql_iqld_stats(self._h, int(bool(update_critic)), int(bool(update_actor)), C.byref(la), C.byref(ma), C.byref(ls)))
        return int(la.value), int(ma.value), int(ls.value)


def group_cfgs(cfg, K, lead):
    """The guidance weights of a group's fused sampling call as [K, n] (n = prod(lead)), checked before any library call: a scalar (every
    member, every row), [K] (one per member) or [K, *lead] (one per member and row); every weight finite (check_cfgs)."""
    n = int(np.prod(lead)) if lead else 1
    c = as_array(cfg)
    is_t = hasattr(c, 'data_ptr')
    sh = tuple(int(d) for d in c.shape)
    if sh == ():
        c = c.reshape(1, 1).expand(K, n) if is_t else np.broadcast_to(np.asarray(c, dtype=np.float32).reshape(1, 1), (K, n))
    elif sh == (K,) and sh != (K,) + tuple(lead):
        c = c.reshape(K, 1).expand(K, n) if is_t else np.broadcast_to(np.asarray(c, dtype=np.float32).reshape(K, 1), (K, n))
    elif sh != (K,) + tuple(lead):
        raise ValueError(f'cfg must be a scalar, [{K}] (one guidance weight per member) or {(K,) + tuple(lead)} (one per row), got {sh}')
    c = c.float() if is_t else np.asarray(c, dtype=np.float32)
    return check_cfgs(c.reshape(K * n), K * n, 'member and row').reshape(K, n)


class IQLDiffusionAgentGroup(AgentGroup):
    """K IQL-diffusion agents of one structure - the same config except `seed`, `awr_temperature` and `softmax_beta` - advanced by fused
    update programs (include/fql_amd.h, fql_iqld_group_*): one per step kind, every launch carrying all K members' tasks.  The
    softmax_beta x seed sweep of the reference's scripts on one device:

        group = IQLDiffusionAgentGroup.create(seeds, ex_obs, ex_act, config, softmax_betas=[...])
        group.upload_dataset(train_dataset)
        for i in range(1, n + 1):
            infos = group.update_from_dataset(update_critic=..., update_actor=..., want_info=(i % log_every == 0))
        actions = group.sample_actions(observations, seed=i, cfg=3.0)   # [K, ..., act], one fused call

    `members` are ordinary IQLDiffusionAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same
    seed, coefficients, rows and noise.  Members are state agents with precision 'fp32' and the engine's device RNG; while grouped their
    batch size is fixed.  FQL agents are grouped by FQLAgentGroup, ReBRAC agents by ReBRACAgentGroup."""

    _member, _get_config = IQLDiffusionAgent, staticmethod(get_config)
    _create_fn, _update_fn = 'fql_iqld_group_create', 'fql_iqld_group_update_from_dataset'
    _sample_fn, _stats_fn = 'fql_iqld_group_sample_actions', 'fql_iqld_group_stats'

    @classmethod
    def create(cls, seeds, ex_observations, ex_actions, config, awr_temperatures=None, softmax_betas=None):
        return cls._create(seeds, config, {'awr_temperature': (awr_temperatures, 'awr_temperatures'), 'softmax_beta': (softmax_betas, 'softmax_betas')},
                           ex_observations, ex_actions)

    def update_from_dataset(self, batch_size=None, idxs=None, want_info=False, update_critic=True, update_actor=True):
        """One fused update of every member of the step kind (update_critic, update_actor): rows from each member's dataset (`idxs`
        [K, B] int, host or device, or None = each member's device RNG), x_0 and t from each member's device RNG.  Returns a list of K
        StepInfo keyed by info_keys(update_critic, update_actor) (want_info) or None."""
        B = self._batch(batch_size)
        uc, ua = bool(update_critic), bool(update_actor)

        def after(m):
            m._actor_steps += int(ua)
        return self._update(B, idxs, want_info, extra=(int(uc), int(ua)), after=after, info=lambda m: m._step_info(None, uc, ua, B))

    def sample_actions(self, observations, seed=None, cfg=1.0, noises=None):
        """IQLDiffusionAgent.sample_actions of every member in ONE fused call (fql_iqld_group_sample_actions): result[i] is bitwise
        what members[i].sample_actions(observations[i], seed=..., cfg=..., noises=noises[i]) returns.  `cfg`: a scalar, [K] (one
        guidance weight per member) or [K, ...] (one per row: members[i].sample_actions_rows); every weight finite.  Shapes and seeds as
        in FQLAgentGroup.sample_actions: observations [K, ..., od] or one shared block, noises [K, ..., ad] or None, seed None (each
        member's own counter advances), one seed or K seeds.  Returns [K, ..., ad]."""
        K = len(self.members)
        c = as_array(cfg)
        check_cfgs(c.reshape(-1), int(np.prod(c.shape)), 'entry')   # finite, whatever the shape: before a member's seed counter moves
        o, z, seeds, n, out, optr, stream = _group_sample_args(self.members, observations, noises, seed, False)
        w = _Arg(group_cfgs(c, K, tuple(int(d) for d in out.shape[1:-1])), (K, n))
        self._check(getattr(self._lib, self._sample_fn)(self._g, o.ptr, n, z.ptr, seeds, w.ptr, optr, FQLAgent._stream([o, z, w])))
        return out

    def launches(self):
        """Kernel launches of (the full, critic-only, actor-only and neither program, one fused sampling call on a single chunk)."""
        la, s = (C.c_int64 * 4)(), C.c_int64(0)
        self._check(getattr(self._lib, self._stats_fn)(self._g, la, C.byref(s)))
        return int(la[0]), int(la[1]), int(la[2]), int(la[3]), int(s.value)


__all__ = ['IQLDiffusionAgent', 'IQLDiffusionAgentGroup', 'IQLD_INFO_KEYS', 'IQLD_ROW_KEYS', 'IQLD_NOISE_KEYS', 'OPTIMAL_VARS', 'info_keys', 'get_config']
