"""Host-side mirror of the reference's CFGRLAgent (agents/cfgrl.py) over the C ABI: a goal-conditioned flow-matching policy trained with
a per-row goal dropout and sampled with classifier-free guidance.

actor_flow is GCActorVectorField: MLP((*actor_hidden_dims, act), GELU, LayerNorm optional) on [obs | goals | x_t | t]; unc_embed is the
learned [1, goal_dim] row that stands in for the goal of a dropped row (probability 0.1) and for every goal of the unconditional pass of
sample_actions.  Same call sites as the reference:

    agent = CFGRLAgent.create(seed, example_batch, config)      # reads observations, actions, value_goals
    agent, info = agent.update(batch)                           # reads observations, actions, actor_goals; info: CFGRL_INFO_KEYS
    action = agent.sample_actions(observations=ob, goals=goal, seed=key)

GCDataset.sample runs on the device: upload_dataset builds the per-row `final` table from `terminals`, and update_from_dataset draws
idx, the goal of each row from its own trajectory (utils/datasets.py:224-255, actor_p_curgoal / trajgoal / randomgoal) and the dropout
mask there.  read_rows() returns the raw 32-bit draws of the last update, so the rule can be restated on the host from the same draws.

State observations, fp32 and GELU only: `encoder`, precision 'bf16x3', rng other than 'engine', frame stacking and actor_geom_sample
are refused here, before the library is called.  Checkpoints (TrainState key 'network'), get/set_params and synchronize are FQLAgent's
plumbing on a CFGRL handle.

CFGRLAgentGroup advances K such agents - one config but for seed, cfg and the actor's goal mixture - with one fused update program and
samples them in one fused call (fql_cfgrl_group_*).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _cabi
from .agent import AgentGroup, FQLAgent, KindAgent, _Arg, _PendingN, _group_sample_args
from .config import ConfigDict
from .iql_diffusion import as_array, check_cfgs, group_cfgs, sweep_inputs

CFGRL_INFO_KEYS = ('actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm')
CFGRL_NOISE_KEYS = ('x0', 't')
CFGRL_DRAW_KEYS = ('idx', 'random', 'dist', 'traj', 'cur', 'mask')   # rows of read_rows()['draws']
P_UNCOND = 0.1   # agents/cfgrl.py:34


def get_config():
    """agents/cfgrl.py:162-191 (same keys and defaults), plus the engine's own 'rng' and 'precision' keys."""
    return ConfigDict(
        agent_name='cfgrl',
        lr=3e-4,
        batch_size=1024,
        actor_hidden_dims=(512, 512, 512, 512),
        actor_layer_norm=False,
        discount=0.99,
        flow_steps=16,
        cfg=3.0,
        encoder=None,
        action_dim=None,
        dataset_class='GCDataset',
        value_p_curgoal=0.0,
        value_p_trajgoal=1.0,
        value_p_randomgoal=0.0,
        value_geom_sample=False,
        actor_p_curgoal=0.0,
        actor_p_trajgoal=1.0,
        actor_p_randomgoal=0.0,
        actor_geom_sample=False,
        gc_negative=True,
        p_aug=0.0,
        frame_stack=None,
        rng='engine',  # not a reference key: device Philox noise or explicit tensors
        precision='fp32',  # not a reference key: fp32 only
    )


def final_indices(terminals):
    """utils/datasets.py:151-153,234: per row, the last row of its trajectory, terminal_locs[searchsorted(terminal_locs, i)]."""
    (terminal_locs,) = np.nonzero(np.asarray(terminals) > 0)
    n = len(terminals)
    assert len(terminal_locs) and terminal_locs[-1] == n - 1, 'the last row of the dataset must be terminal'
    return terminal_locs[np.searchsorted(terminal_locs, np.arange(n))].astype(np.int64)


class CFGRLAgent(KindAgent):
    """CFGRL agent backed by the MI355X step engine.  update: agents/cfgrl.py:58-68, 4 infos (CFGRL_INFO_KEYS)."""

    _name = 'CFGRL'
    _modules = {}   # network.select: actor_flow's input carries the goals and the unc_embed row
    _refused = (('total_loss', 'total_loss (CFGRLAgent has policy_loss)'),
                ('compute_flow_actions', 'compute_flow_actions (sample_actions(noises=) is the flow)'),
                ('create_replay_buffer', 'the replay ring'), ('update_balanced', 'balanced sampling'),
                ('add_transition', 'ring inserts (the goal table describes the uploaded rows)'))
    _update_dataset_fn = 'fql_cfgrl_update_from_dataset'
    _loss_infos = 1
    _pending_cls = _PendingN
    _train_state_key = 'network'   # agents/cfgrl.py:19: the TrainState's field name (checkpoint layout)

    @classmethod
    def create(cls, seed, example_batch, config):
        """agents/cfgrl.py:102-159.  `example_batch`: observations, actions and value_goals (goal_dim is its last axis)."""
        cfg = get_config()
        cfg.update(dict(config))
        cls._check_create(cfg, example_batch)
        lib = _cabi.load()
        # fql_config mapping (include/fql_amd.h): actor_hidden_dims -> actor_hidden, actor_layer_norm, lr
        ec = dict(actor_hidden_dims=tuple(cfg['actor_hidden_dims']), value_hidden_dims=tuple(cfg['actor_hidden_dims']), layer_norm=False,
                  actor_layer_norm=bool(cfg['actor_layer_norm']), lr=cfg['lr'], discount=cfg['discount'], tau=0.005, flow_steps=1,
                  batch_size=cfg['batch_size'], precision='fp32', encoder=None)
        c, ob_dims, action_dim = cls._engine_config(lib, ec, example_batch['observations'], example_batch['actions'])
        gc = _cabi.FqlCfgrlConfig()
        lib.fql_cfgrl_default_config(C.byref(gc))
        gc.goal_dim = int(example_batch['value_goals'].shape[-1])
        gc.flow_steps, gc.cfg, gc.p_uncond = int(cfg['flow_steps']), float(cfg['cfg']), P_UNCOND
        gc.actor_p_curgoal, gc.actor_p_trajgoal = float(cfg['actor_p_curgoal']), float(cfg['actor_p_trajgoal'])
        gc.actor_p_randomgoal, gc.actor_geom_sample = float(cfg['actor_p_randomgoal']), 0
        h = C.c_void_p()
        _cabi.check(lib, None, lib.fql_cfgrl_create(C.byref(c), C.byref(gc), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)))
        cfg['ob_dims'] = ob_dims
        cfg['action_dim'] = action_dim
        cfg['goal_dim'] = int(gc.goal_dim)
        return cls(h, cfg, int(seed))

    @classmethod
    def _check_create(cls, cfg, example_batch):
        """The refusals of create (and of CFGRLAgentGroup.create, per member), before any library call."""
        cls._refuse_config(cfg)
        if cfg.get('actor_geom_sample'):
            raise NotImplementedError('CFGRL: actor_geom_sample=True is not built (uniform trajectory goals only)')
        if cfg.get('frame_stack') is not None:
            raise NotImplementedError('CFGRL: frame_stack is not built (state observations only)')
        if int(cfg['flow_steps']) < 1:
            raise ValueError('flow_steps must be >= 1')
        psum = float(cfg['actor_p_curgoal']) + float(cfg['actor_p_trajgoal']) + float(cfg['actor_p_randomgoal'])
        if not np.isclose(psum, 1.0):   # utils/datasets.py:159-161
            raise ValueError('actor_p_curgoal + actor_p_trajgoal + actor_p_randomgoal must be 1')
        for k in ('observations', 'actions', 'value_goals'):
            if k not in example_batch:
                raise KeyError(f'example_batch is missing {k!r}')

    def _batch_args(self, batch):   # CFGRL reads observations, actions and actor_goals of the goal-conditioned batch
        for k in ('observations', 'actions', 'actor_goals'):
            if k not in batch:
                raise KeyError(f'batch is missing {k!r}')
        B = int(batch['actions'].shape[0]) if hasattr(batch['actions'], 'shape') else int(np.shape(batch['actions'])[0])
        od, ad, G = self.config['ob_dims'][0], self.config['action_dim'], self.config['goal_dim']
        return B, [_Arg(batch['observations'], (B, od)), _Arg(batch['actions'], (B, ad)), _Arg(batch['actor_goals'], (B, G))]

    def _noise_args(self, noise, B):
        """Explicit x0 [B, act] and t [B] or [B, 1] (agents/cfgrl.py:27-29); other keys are refused."""
        if noise is None:
            return None, []
        extra = set(noise) - set(CFGRL_NOISE_KEYS)
        if extra:
            raise ValueError(f'CFGRL reads only {CFGRL_NOISE_KEYS} of the noise dict, got {sorted(extra)}')
        x0, ta = _Arg(noise.get('x0'), (B, self.config['action_dim'])), _Arg(noise.get('t'), (B,))
        return _cabi.FqlNoise(None, x0.ptr, ta.ptr, None, None), [x0, ta]

    @staticmethod
    def _mask_arg(do_cfg, B):
        """[B] booleans as bytes (agents/cfgrl.py:34), or None = the engine's draw."""
        if do_cfg is None:
            return _Arg(None)
        if hasattr(do_cfg, 'data_ptr'):
            do_cfg = do_cfg != 0
        else:
            do_cfg = np.asarray(do_cfg) != 0
        return _Arg(do_cfg, (B,), u8=True)

    def update(self, batch, noise=None, do_cfg=None, want_info=True):
        """agents/cfgrl.py:58-68.  `noise`: explicit x0 / t; `do_cfg`: the explicit [B] dropout mask.  Returns (agent, info)."""
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        m = self._mask_arg(do_cfg, B)
        stream = self._stream(args + nargs + [m])
        self._check(self._lib.fql_cfgrl_update(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, m.ptr, None, stream))
        self._keep = (args, nargs, m)
        return self, (self._lazy_info(stream) if want_info else None)

    def policy_loss(self, batch, grad_params=None, rng=None, noise=None, do_cfg=None):
        """agents/cfgrl.py:22-42 with the stored parameters: (loss, {'actor_loss': loss}).  No state changes."""
        self._probe_guard('actor_loss with traced grad_params', grad_params, rng)
        B, args = self._batch_args(batch)
        self._ensure_batch(B)
        nz, nargs = self._noise_args(noise, B)
        m = self._mask_arg(do_cfg, B)
        loss = C.c_float()
        self._check(self._lib.fql_cfgrl_policy_loss(self._h, *[a.ptr for a in args], B, C.byref(nz) if nz else None, m.ptr, C.byref(loss),
                                                    self._stream(args + nargs + [m])))
        return float(loss.value), {'actor_loss': float(loss.value)}

    def upload_dataset(self, dataset, capacity=None):
        """GCDataset(Dataset.create(...)) -> HBM: the transitions, the per-row `final` table built from `terminals` (the last row must be
        terminal, utils/datasets.py:153) and `oracle_reps` as the goal representations when the dataset has that key."""
        final = final_indices(dataset['terminals'])
        n = int(len(dataset['observations']))
        od, ad = self.config['ob_dims'][0], self.config['action_dim']
        zeros = np.zeros(n, np.float32)   # CFGRL reads neither rewards, masks nor next_observations (compact datasets have none)
        args = [_Arg(dataset['observations'], (n, od)), _Arg(dataset['actions'], (n, ad)), _Arg(zeros), _Arg(zeros),
                _Arg(dataset['observations'], (n, od))]
        self._check(self._lib.fql_dataset_upload(self._h, n, int(capacity) if capacity is not None else max(n, 1), *[a.ptr for a in args]))
        reps = _Arg(dataset['oracle_reps'], (n, self.config['goal_dim'])) if 'oracle_reps' in dataset else _Arg(None)
        self._check(self._lib.fql_cfgrl_dataset_goals(self._h, final.ctypes.data, reps.ptr))

    def update_from_dataset(self, batch_size=None, idxs=None, noise=None, shard=(0, 0), want_info=False, stream=None, do_cfg=None):
        """GCDataset.sample(B) + update(batch) without leaving the device."""
        B = int(batch_size or self.config['batch_size'])
        m = self._mask_arg(do_cfg, B)
        out = super().update_from_dataset(batch_size, idxs, noise, shard, want_info, stream, _extra=(m.ptr,))
        self._keep = (self._keep, m)
        return out

    def read_rows(self, probe=False):
        """The rows of the last update (probe=True: of the last policy_loss): idx, goal_idx (-1 where the goals came with the batch),
        do_cfg, the raw 32-bit draws by name (CFGRL_DRAW_KEYS) and the goal columns of the assembled input rows."""
        B, G = int(self.config['batch_size']), self.config['goal_dim']
        idx, gi = np.empty(B, np.int64), np.empty(B, np.int64)
        m, dr, goals = np.empty(B, np.uint8), np.empty((len(CFGRL_DRAW_KEYS), B), np.uint32), np.empty((B, G), np.float32)
        self._check(self._lib.fql_cfgrl_read_rows(self._h, int(bool(probe)), idx.ctypes.data, gi.ctypes.data, m.ctypes.data, dr.ctypes.data,
                                                  goals.ctypes.data, B))
        return {'idx': idx, 'goal_idx': gi, 'do_cfg': m.astype(bool), 'draws': dict(zip(CFGRL_DRAW_KEYS, dr)), 'goals': goals}

    def sample_actions(self, observations, goals=None, seed=None, temperature=1.0, cfg=None, noises=None):
        """agents/cfgrl.py:70-100: x ~ N(0, I); flow_steps times v = v_unc + cfg (v_cond - v_unc), x += v / flow_steps; clip.  [od] with
        [G] -> [act]; [n, od] with [n, G], or with one [G] for every row, -> [n, act], row by row the single-observation result.
        `cfg=None`: the config's value.  `noises`: x with the shape [n, act] (or [act]), or None = engine RNG keyed by `seed`.
        `temperature` is accepted and ignored, as in the reference."""
        if goals is None:
            raise ValueError('CFGRL: sample_actions needs goals (the conditional pass reads them, agents/cfgrl.py:93)')
        od, ad, G = self.config['ob_dims'][0], self.config['action_dim'], self.config['goal_dim']
        if not hasattr(observations, 'shape'):
            observations = np.asarray(observations, dtype=np.float32)
        if not hasattr(goals, 'shape'):
            goals = np.asarray(goals, dtype=np.float32)
        if int(observations.shape[-1]) != od or len(observations.shape) > 2:
            raise ValueError(f'observations must be [{od}] or [n, {od}], got {tuple(observations.shape)}')
        n = int(observations.shape[0]) if len(observations.shape) == 2 else 1
        if int(goals.shape[-1]) != G or tuple(goals.shape[:-1]) not in ((), (1,), (n,)):
            raise ValueError(f'goals must be [{G}] or [{n}, {G}], got {tuple(goals.shape)}')
        if int(np.prod(goals.shape)) == G and n > 1:   # one goal for every row
            goals = goals.reshape(1, G).expand(n, G) if hasattr(goals, 'data_ptr') else np.broadcast_to(np.reshape(goals, (1, G)), (n, G))
        shape = (ad,) if n == 1 else (n, ad)
        o, g, z = _Arg(observations, (n, od)), _Arg(goals, (n, G)), _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, shape)
        scale = float(self.config['cfg'] if cfg is None else cfg)
        self._check(self._lib.fql_cfgrl_sample_actions(self._h, o.ptr, g.ptr, n, z.ptr, self._sample_seed(seed, noises), scale, optr,
                                                       self._stream([o, g, z])))
        return out

    # -- guidance sweeps: one weight per row --------------------------------------------------------
    def sample_actions_rows(self, observations, goals, cfgs, seed=None, noises=None):
        """sample_actions with one guidance weight per row, in ONE call: observations [N, od], goals [N, G] or one [G], cfgs [N] ->
        [N, act] (no squeeze).  Row j is, bit for bit, sample_actions(observations[j], goals[j], cfg=cfgs[j], noises=noises[j]); with
        engine noise row j draws what row j of sample_actions(.., seed=seed) draws.  3 + S nl + 1 launches whatever N <= 2048 is."""
        if goals is None:
            raise ValueError('CFGRL: sample_actions_rows needs goals (the conditional pass reads them, agents/cfgrl.py:93)')
        od, ad, G = self.config['ob_dims'][0], self.config['action_dim'], self.config['goal_dim']
        observations, goals = as_array(observations), as_array(goals)
        if len(observations.shape) != 2 or int(observations.shape[1]) != od or int(observations.shape[0]) < 1:
            raise ValueError(f'observations must be [N, {od}] with N >= 1, got {tuple(observations.shape)}')
        n = int(observations.shape[0])
        if tuple(int(d) for d in goals.shape) not in ((G,), (1, G), (n, G)):
            raise ValueError(f'goals must be [{G}] or [{n}, {G}], got {tuple(goals.shape)}')
        if int(np.prod(goals.shape)) == G and n > 1:   # one goal for every row
            goals = goals.reshape(1, G).expand(n, G) if hasattr(goals, 'data_ptr') else np.broadcast_to(np.reshape(goals, (1, G)), (n, G))
        cfgs = check_cfgs(cfgs, n, 'row')
        if noises is not None and tuple(as_array(noises).shape) != (n, ad):
            raise ValueError(f'noises must be [{n}, {ad}], got {tuple(as_array(noises).shape)}')
        o, g, w, z = _Arg(observations, (n, od)), _Arg(goals, (n, G)), _Arg(cfgs, (n,)), _Arg(noises, (n, ad))
        out, optr = self._actions_out(observations, (n, ad))
        self._check(self._lib.fql_cfgrl_sample_actions_cfgs(self._h, o.ptr, g.ptr, n, z.ptr, self._sample_seed(seed, noises), w.ptr, optr,
                                                            self._stream([o, g, z, w])))
        return out

    def sample_actions_sweep(self, observations, goals, cfgs, seed=None, noises=None):
        """Every weight of an evaluation sweep in one call: cfgs [K] -> [K, n, act], slice k = sample_actions(.., cfg=cfgs[k]).
        observations: [n, od] (every weight sees the same rows) or [K, n, od] (one vector env per weight); goals: [G], [n, G] or
        [K, n, G] by the same rule; noises: None (engine RNG: row k n + j of the flat call), [n, act] (shared by every weight: common
        random numbers) or [K, n, act]."""
        if goals is None:
            raise ValueError('CFGRL: sample_actions_sweep needs goals (the conditional pass reads them, agents/cfgrl.py:93)')
        od, ad, G = self.config['ob_dims'][0], self.config['action_dim'], self.config['goal_dim']
        K, n, (ob, g, z), w = sweep_inputs(cfgs, [('observations', observations, od), ('goals', goals, G, True), ('noises', noises, ad)])
        return self.sample_actions_rows(ob, g, w, seed=seed, noises=z).reshape(K, n, ad)

    def sample_cfgs_stats(self):
        """Launches of one sample_actions_rows / sample_actions_sweep call of <= 2048 rows."""
        ls = C.c_int64()
        self._check(self._lib.fql_sample_cfgs_stats(self._h, C.byref(ls)))
        return int(ls.value)

    def cfgrl_stats(self):
        """(launches of one update, MACs of one update, launches of one sampling call of <= 2048 observations)."""
        la, ma, ls = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.fql_cfgrl_stats(self._h, C.byref(la), C.byref(ma), C.byref(ls)))
        return int(la.value), int(ma.value), int(ls.value)


MIX_KEYS = ('actor_p_curgoal', 'actor_p_trajgoal', 'actor_p_randomgoal')


class CFGRLAgentGroup(AgentGroup):
    """K CFGRL agents of one structure - the same config except `seed`, `cfg` and the actor's goal mixture (actor_p_curgoal /
    actor_p_trajgoal / actor_p_randomgoal) - advanced by ONE fused update program (include/fql_amd.h, fql_cfgrl_group_*): every launch of
    the update's single lane carries all K members' tasks.  The seed x goal-mixture x guidance-weight sweeps of the goal-conditioned
    benchmarks on one device:

        group = CFGRLAgentGroup.create(seeds, example_batch, config, cfgs=[1.5, 3, 5], goal_mixes=[(0, 1, 0), (0, .5, .5), (.2, .5, .3)])
        group.upload_dataset(train_dataset)
        for i in range(1, n + 1):
            infos = group.update_from_dataset(want_info=(i % log_every == 0))
        actions = group.sample_actions(observations, goals, seed=i)   # [K, ..., act], one fused call, each member's own cfg

    `members` are ordinary CFGRLAgent objects; a member's trajectory is bitwise the one it has when trained alone with the same seed,
    mixture, rows, mask and noise.  Members are state agents with precision 'fp32' and the engine's device RNG; while grouped their batch
    size is fixed.  The other kinds have groups of their own (FQLAgentGroup, ReBRACAgentGroup, IQLDiffusionAgentGroup, IFQLAgentGroup,
    IQLAgentGroup)."""

    _member, _get_config = CFGRLAgent, staticmethod(get_config)
    _create_fn, _update_fn = 'fql_cfgrl_group_create', 'fql_cfgrl_group_update_from_dataset'
    _sample_fn, _stats_fn = 'fql_cfgrl_group_sample_actions', 'fql_cfgrl_group_stats'   # launches(): (the update program, one sampling call)

    @classmethod
    def create(cls, seeds, example_batch, config, cfgs=None, goal_mixes=None):
        """`cfgs`: K default guidance weights (None: the config's).  `goal_mixes`: K triples (p_cur, p_traj, p_random), each summing to
        1 (None: the config's mixture for every member)."""
        def mixtures(cfg, K, lists):
            if not np.isfinite(lists['cfg']).all():
                raise ValueError('cfgs: every guidance weight must be finite')
            mixes = [tuple(float(cfg[k]) for k in MIX_KEYS)] * K if goal_mixes is None else [tuple(float(p) for p in mix) for mix in goal_mixes]
            if len(mixes) != K:
                raise ValueError(f'{K} seeds but {len(mixes)} goal_mixes')
            for i, mix in enumerate(mixes):
                if len(mix) != 3 or min(mix) < 0.0 or not np.isclose(sum(mix), 1.0):
                    raise ValueError(f'goal_mixes[{i}] = {mix}: three probabilities (p_cur, p_traj, p_random) that sum to 1')
            lists.update((k, [mix[j] for mix in mixes]) for j, k in enumerate(MIX_KEYS))
        return cls._create(seeds, config, {'cfg': (cfgs, 'cfgs')}, example_batch, more=mixtures)

    @classmethod
    def _refuse(cls, cfg, example_batch):   # encoder, precision, rng, actor_geom_sample, frame_stack, flow_steps, the example's keys
        CFGRLAgent._check_create(cfg, example_batch)

    def update_from_dataset(self, batch_size=None, idxs=None, do_cfg=None, want_info=False):
        """One fused update of every member: rows from each member's dataset (`idxs` [K, B] int, host or device, or None = each member's
        device RNG), the goal of each row drawn with the member's own mixture, `do_cfg` [K, B] booleans (host or device) or None = each
        member's own mask draw; x_0 and t from each member's device RNG.  Returns a list of K LazyInfo over CFGRL_INFO_KEYS (want_info)
        or None."""
        K = len(self.members)
        B = self._batch(batch_size)
        mask = _Arg(None)
        if do_cfg is not None:
            do_cfg = do_cfg if hasattr(do_cfg, 'data_ptr') else np.asarray(do_cfg)
            if tuple(int(d) for d in do_cfg.shape) != (K, B):
                raise ValueError(f'do_cfg must be [{K}, {B}], got {tuple(do_cfg.shape)}')
            mask = _Arg(do_cfg != 0, (K, B), u8=True)
        return self._update(B, idxs, want_info, extra=(mask.ptr,), hold=mask)

    def sample_actions(self, observations, goals, seed=None, cfg=None, noises=None):
        """CFGRLAgent.sample_actions of every member in ONE fused call (fql_cfgrl_group_sample_actions): result[i] is bitwise what
        members[i].sample_actions(observations[i], goals[i], seed=..., cfg=..., noises=noises[i]) returns.  `cfg`: None (each member's
        configured default), a scalar, [K] (one guidance weight per member) or [K, ...] (one per row: members[i].sample_actions_rows);
        every weight finite.  observations [K, ..., od] or one shared block; goals [K, ..., G], one shared block [..., G] or one [G] for
        every member and row; noises [K, ..., ad] or None; seed None (each member's own counter advances), one seed or K seeds, as in
        FQLAgentGroup.sample_actions.  Returns [K, ..., ad]."""
        if goals is None:
            raise ValueError('CFGRL: sample_actions needs goals (the conditional pass reads them, agents/cfgrl.py:93)')
        K, G = len(self.members), int(self.members[0].config['goal_dim'])
        c = as_array([float(m.config['cfg']) for m in self.members] if cfg is None else cfg)
        check_cfgs(c.reshape(-1), int(np.prod(c.shape)), 'entry')   # finite, whatever the shape: before a member's seed counter moves
        goals = as_array(goals)
        # (flow=True: the shape rules alone - no seed is drawn, no counter moves before the goals and the weights are checked)
        lead = tuple(int(d) for d in _group_sample_args(self.members, observations, noises, seed, True)[4].shape[1:-1])
        gs = tuple(int(d) for d in goals.shape)
        if gs not in ((K,) + lead + (G,), lead + (G,), (G,)):
            raise ValueError(f'goals must be {(K,) + lead + (G,)}, one shared block {lead + (G,)} or one [{G}], got {gs}')
        if gs != (K,) + lead + (G,):   # shared: broadcast here, the library takes one block per member
            goals = goals.expand((K,) + lead + (G,)) if hasattr(goals, 'data_ptr') else np.broadcast_to(goals, (K,) + lead + (G,))
        w = group_cfgs(c, K, lead)
        o, z, seeds, n, out, optr, _ = _group_sample_args(self.members, observations, noises, seed, False)
        g, w = _Arg(goals, (K, n, G)), _Arg(w, (K, n))
        self._check(getattr(self._lib, self._sample_fn)(self._g, o.ptr, g.ptr, n, z.ptr, seeds, w.ptr, optr, FQLAgent._stream([o, g, z, w])))
        return out


__all__ = ['CFGRLAgent', 'CFGRLAgentGroup', 'CFGRL_INFO_KEYS', 'CFGRL_NOISE_KEYS', 'CFGRL_DRAW_KEYS', 'get_config', 'final_indices']
