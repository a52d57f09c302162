"""fp64 numpy restatement of the reference's CFGRLAgent (agents/cfgrl.py) with a hand-derived backward, and of GCDataset.sample_goals
(utils/datasets.py:224-255) driven by given draws.

actor_flow(obs, x_t, t, goals) = MLP((*hidden, act), GELU(tanh), LayerNorm optional, no final activation) on [obs | goals | x_t | t];
goals = where(do_cfg, unc_embed, actor_goals).  The input gradient of the goal columns, summed over the dropped rows, is the gradient of
unc_embed: the where sends nothing through the kept rows.
"""
import numpy as np

from oracle import fql_oracle as O

INFO_KEYS = ('actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm')
FLOW, EMBED = 'modules_actor_flow', 'modules_unc_embed'


def get_config() -> dict:
    """agents/cfgrl.py:162-191, the keys the agent itself reads."""
    return dict(agent_name='cfgrl', lr=3e-4, batch_size=1024, actor_hidden_dims=(512, 512, 512, 512), actor_layer_norm=False,
                discount=0.99, flow_steps=16, cfg=3.0)


def init_params(seed, obs_dim, act_dim, goal_dim, config, dtype=np.float32):
    """agents/cfgrl.py:132-156: every Dense kernel default_init (Glorot uniform), zero biases, LayerNorm (1, 0); nn.Embed(1, G)'s default
    variance_scaling(1, fan_in, normal, out_axis=0), whose fan_in on [1, G] is G: N(0, 1 / G)."""
    rng = np.random.default_rng(seed)
    mlp, prev = {}, obs_dim + goal_dim + act_dim + 1
    dims = tuple(config['actor_hidden_dims']) + (act_dim,)
    for i, h in enumerate(dims):
        mlp[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, prev, h, (prev, h), dtype), 'bias': np.zeros(h, dtype)}
        if config['actor_layer_norm'] and i + 1 < len(dims):
            mlp[f'LayerNorm_{i}'] = {'scale': np.ones(h, dtype), 'bias': np.zeros(h, dtype)}
        prev = h
    emb = (rng.standard_normal((1, goal_dim)) / np.sqrt(goal_dim)).astype(dtype)
    return {FLOW: {'mlp': mlp}, EMBED: {'Embed_0': {'embedding': emb}}}


class OracleCFGRL:
    def __init__(self, params, config, obs_dim, act_dim, goal_dim, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.params = O.tree_map(lambda a: np.array(a, dtype=self.dtype), params)
        self.config = dict(config)
        self.S = int(self.config['flow_steps'])
        self.od, self.ad, self.G = obs_dim, act_dim, goal_dim
        self.mu = O.tree_map(np.zeros_like, self.params)
        self.nu = O.tree_map(np.zeros_like, self.params)
        self.count, self.step = 0, 1

    def _c(self, x):
        return np.asarray(x, dtype=self.dtype)

    def unc(self):
        return self.params[EMBED]['Embed_0']['embedding']

    def flow(self, obs, goals, x, t, keep=False):
        """[obs | goals | x | t] (utils/networks.py:277-281: that order) through the MLP."""
        return O.mlp_forward(self.params[FLOW]['mlp'], np.concatenate([obs, goals, x, t], axis=-1), keep=keep)

    def _losses(self, batch, noise, do_cfg, want_grads):
        """agents/cfgrl.py:22-42.  noise: {'x0': [B, act], 't': [B]}; do_cfg: [B] booleans."""
        a, x0 = self._c(batch['actions']), self._c(noise['x0'])
        t = self._c(noise['t']).reshape(-1, 1)
        drop = np.asarray(do_cfg).astype(bool)
        x_t = (1 - t) * x0 + t * a
        vel = a - x0
        goals = np.where(drop[:, None], self.unc(), self._c(batch['actor_goals']))
        out = self.flow(self._c(batch['observations']), goals, x_t, t, keep=want_grads)
        pred, cache = out if want_grads else (out, None)
        d = pred - vel
        loss = float(np.mean(d * d))
        if not want_grads:
            return loss, {'actor/actor_loss': loss}, None
        dx, g = O.mlp_backward(self.params[FLOW]['mlp'], cache, 2.0 * d / d.size)
        dgoal = dx[:, self.od:self.od + self.G]
        dU = dgoal[drop].sum(axis=0, keepdims=True)   # where(): the dropped rows only
        return loss, {'actor/actor_loss': loss}, {FLOW: {'mlp': g}, EMBED: {'Embed_0': {'embedding': dU}}}

    def policy_loss(self, batch, noise, do_cfg):
        loss, info, _ = self._losses(batch, noise, do_cfg, False)
        return loss, info

    def grads(self, batch, noise, do_cfg):
        return self._losses(batch, noise, do_cfg, True)

    def apply_gradients(self, grads):
        """optax.adam(lr) + apply_updates (utils/flax_utils.py:120-130); no target network."""
        dt = self.dtype.type
        b1, b2, eps, lr = dt(0.9), dt(0.999), dt(1e-8), dt(self.config['lr'])
        self.count += 1
        c1, c2 = dt(1.0 - 0.9 ** self.count), dt(1.0 - 0.999 ** self.count)

        def upd(p, g, m, v):
            m[...] = b1 * m + (dt(1) - b1) * g
            v[...] = b2 * v + (dt(1) - b2) * g * g
            return p - lr * (m / c1) / (np.sqrt(v / c2) + eps)

        self.params = O.tree_map(upd, self.params, grads, self.mu, self.nu)
        self.step += 1

    def update(self, batch, noise, do_cfg):
        loss, info, grads = self._losses(batch, noise, do_cfg, True)
        info.update(O.OracleFQL.grad_stats(grads))
        self.apply_gradients(grads)
        return loss, {k: float(info[k]) for k in INFO_KEYS}

    def sample_actions(self, observations, goals, noises, cfg=None):
        """agents/cfgrl.py:70-100 with explicit x ~ N(0, I): flow_steps Euler steps of v_unc + cfg (v_cond - v_unc), then the clip.  t is
        the Python float i / flow_steps cast to the working dtype, as jnp.full makes it."""
        cfg = self.dtype.type(self.config['cfg'] if cfg is None else cfg)
        obs = self._c(observations)
        single = obs.ndim == 1
        obs = obs[None] if single else obs
        n = obs.shape[0]
        g = np.broadcast_to(self._c(goals).reshape(-1, self.G), (n, self.G))
        u = np.broadcast_to(self.unc(), (n, self.G))
        x = self._c(noises).reshape(n, self.ad).copy()
        dt = self.dtype.type(self.S)
        for i in range(self.S):
            t = np.full((n, 1), i / self.S, dtype=self.dtype)
            vu, vc = self.flow(obs, u, x, t), self.flow(obs, g, x, t)
            x = x + (vu + cfg * (vc - vu)) / dt
        x = x[0] if single or n == 1 else x
        return np.clip(x, -1, 1)


def make_noise(batch_size, act_dim, seed):
    """x0 ~ N(0, I) and t ~ U[0, 1); row 0 holds t = 0 (when B >= 1)."""
    rng = np.random.default_rng(seed)
    t = rng.random(batch_size).astype(np.float32)
    t[0] = 0.0
    return {'x0': rng.standard_normal((batch_size, act_dim)).astype(np.float32), 't': t}


# ---- GCDataset.sample_goals from given draws ------------------------------------------------------------------------------------------
TRAJ_LENGTHS = (1, 2, 3, 17, 200, 1)


def make_gc_dataset(obs_dim, act_dim, seed, lengths=TRAJ_LENGTHS, reps_dim=None):
    """A dataset of len(lengths) trajectories: observations, actions, terminals (1 on each trajectory's last row) and, with reps_dim, oracle_reps."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    terminals = np.zeros(n, np.float32)
    terminals[np.cumsum(lengths) - 1] = 1.0
    ds = {'observations': rng.standard_normal((n, obs_dim)).astype(np.float32),
          'actions': np.clip(rng.standard_normal((n, act_dim)), -1, 1).astype(np.float32), 'terminals': terminals}
    if reps_dim is not None:
        ds['oracle_reps'] = rng.standard_normal((n, reps_dim)).astype(np.float32)
    return ds


def final_indices(terminals):
    """utils/datasets.py:151-153,234: terminal_locs[searchsorted(terminal_locs, i)] for every row i."""
    (terminal_locs,) = np.nonzero(np.asarray(terminals) > 0)
    assert terminal_locs[-1] == len(terminals) - 1
    return terminal_locs[np.searchsorted(terminal_locs, np.arange(len(terminals)))]


def sample_goals(idxs, terminals, draws, p_curgoal, p_trajgoal, p_randomgoal):
    """GCDataset.sample_goals (utils/datasets.py:224-255, geom_sample=False), its random numbers given as raw 32-bit draws: the random goal
    is floor(u32 size / 2^32); distances and the uniforms of the two where()s are u32 / 2^32, exact in fp64.  draws: 'random', 'dist',
    'traj', 'cur' (uint32 [B])."""
    idxs = np.asarray(idxs, np.int64)
    size = len(terminals)
    (terminal_locs,) = np.nonzero(np.asarray(terminals) > 0)
    u = {k: np.asarray(draws[k]).astype(np.uint64) for k in ('random', 'dist', 'traj', 'cur')}
    random_goal_idxs = ((u['random'] * np.uint64(size)) >> np.uint64(32)).astype(np.int64)
    final_state_idxs = terminal_locs[np.searchsorted(terminal_locs, idxs)]
    distances = u['dist'].astype(np.float64) / 4294967296.0
    traj_goal_idxs = np.round(np.minimum(idxs + 1, final_state_idxs) * distances + final_state_idxs * (1 - distances)).astype(int)
    if p_curgoal == 1.0:
        return idxs
    goal_idxs = np.where(u['traj'].astype(np.float64) / 4294967296.0 < p_trajgoal / (1.0 - p_curgoal), traj_goal_idxs, random_goal_idxs)
    return np.where(u['cur'].astype(np.float64) / 4294967296.0 < p_curgoal, idxs, goal_idxs)


__all__ = ['OracleCFGRL', 'INFO_KEYS', 'get_config', 'init_params', 'make_noise', 'make_gc_dataset', 'final_indices', 'sample_goals',
           'TRAJ_LENGTHS']
