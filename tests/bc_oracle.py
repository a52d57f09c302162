"""fp64 numpy restatement of the reference's BCAgent (agents/bc.py) with a hand-derived backward: flow-matching behavioural cloning.

policy(obs, x_t, t) = Dense_0(MLP_0([obs | x_t | emb(t)])), MLP_0 = Dense -> GELU(tanh) -> LayerNorm per hidden layer (activate_final).
The timestep embedding is the one pinned definition shared with the engine (fql_amd/bc.py::timestep_embedding).
"""
import numpy as np

from oracle import fql_oracle as O
from fql_amd.bc import timestep_embedding, grid_index

INFO_KEYS = ('bc_loss', 'grad/max', 'grad/min', 'grad/norm')


def get_config() -> dict:
    """agents/bc.py:135-148."""
    return dict(agent_name='bc', batch_size=256, hidden_dims=(512, 512, 512, 512), bc_lr=3e-4, use_layer_norm=1, activation='gelu',
                denoise_steps=16)


def lecun_normal(rng, fan_in, shape, dtype):
    """flax's default Dense kernel init: variance_scaling(1, fan_in, truncated_normal): N(0, 1) truncated to [-2, 2], scaled by
    sqrt(1 / fan_in) / 0.87962566103423978."""
    v = rng.standard_normal(shape)
    bad = np.abs(v) > 2.0
    while bad.any():
        v[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(v) > 2.0
    return (v * np.sqrt(1.0 / fan_in) / 0.87962566103423978).astype(dtype)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/bc.py:122-126: MLP_0 kernels default_init (Glorot uniform), zero biases, LayerNorm (1, 0); Dense_0 lecun_normal."""
    rng = np.random.default_rng(seed)
    hidden = tuple(config['hidden_dims'])
    mlp, prev = {}, obs_dim + act_dim + 16
    for i, h in enumerate(hidden):
        mlp[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, prev, h, (prev, h), dtype), 'bias': np.zeros(h, dtype)}
        if config['use_layer_norm']:
            mlp[f'LayerNorm_{i}'] = {'scale': np.ones(h, dtype), 'bias': np.zeros(h, dtype)}
        prev = h
    return {'MLP_0': mlp, 'Dense_0': {'kernel': lecun_normal(rng, prev, (prev, act_dim), dtype), 'bias': np.zeros(act_dim, dtype)}}


def _as_net(params):
    """The policy as ONE net of O.mlp_forward's form: MLP_0's layers, then the head as the last (linear) Dense."""
    mlp = params['MLP_0']
    n = sum(1 for k in mlp if k.startswith('Dense_'))
    net = {k: v for k, v in mlp.items()}
    net[f'Dense_{n}'] = params['Dense_0']
    return net, n


def _from_net_grads(g, n):
    return {'MLP_0': {k: v for k, v in g.items() if k != f'Dense_{n}'}, 'Dense_0': g[f'Dense_{n}']}


class OracleBC:
    def __init__(self, params, config, obs_dim, act_dim, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.params = O.tree_map(lambda a: np.array(a, dtype=self.dtype), params)
        self.config = dict(config)
        self.S = int(self.config['denoise_steps'])
        self.od, self.ad = obs_dim, act_dim
        self.mu = O.tree_map(np.zeros_like, self.params)
        self.nu = O.tree_map(np.zeros_like, self.params)
        self.count, self.step = 0, 1

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _c(self, x):
        return np.asarray(x, dtype=self.dtype)

    def policy(self, obs, x, k, keep=False):
        emb = self._c(timestep_embedding(np.broadcast_to(np.asarray(k), (obs.shape[0],)), self.S))
        net, _ = _as_net(self.params)
        return O.mlp_forward(net, np.concatenate([self._c(obs), self._c(x), emb], axis=-1), keep=keep)

    def _losses(self, batch, noise, want_grads):
        """agents/bc.py:48-70.  noise: {'x0': [B, act], 't': [B] on the grid}."""
        a, x0 = self._c(batch['actions']), self._c(noise['x0'])
        k = grid_index(noise['t'], self.S)
        t = self._c(k.astype(np.float32) / np.float32(self.S))[:, None]
        x_t = x0 * (1 - t) + a * t
        vel = a - x0
        out = self.policy(batch['observations'], x_t, k, keep=want_grads)
        pred, cache = out if want_grads else (out, None)
        d = pred - vel
        loss = float(np.mean(d * d))
        if not want_grads:
            return loss, {'bc_loss': loss}, None
        net, n = _as_net(self.params)
        _, g = O.mlp_backward(net, cache, 2.0 * d / d.size)
        return loss, {'bc_loss': loss}, _from_net_grads(g, n)

    def policy_loss(self, batch, noise):
        loss, info, _ = self._losses(batch, noise, False)
        return loss, info

    def grads(self, batch, noise):
        return self._losses(batch, noise, True)

    def apply_gradients(self, grads):
        """optax.adam(bc_lr) + apply_updates (utils/flax_utils.py:120-130); no target network."""
        dt = self.dtype.type
        b1, b2, eps, lr = dt(0.9), dt(0.999), dt(1e-8), dt(self.config['bc_lr'])
        self.count += 1
        c1, c2 = dt(1.0 - 0.9 ** self.count), dt(1.0 - 0.999 ** self.count)

        def upd(p, g, m, v):
            m[...] = b1 * m + (dt(1) - b1) * g
            v[...] = b2 * v + (dt(1) - b2) * g * g
            return p - lr * (m / c1) / (np.sqrt(v / c2) + eps)

        self.params = O.tree_map(upd, self.params, grads, self.mu, self.nu)
        self.step += 1

    def update(self, batch, noise):
        loss, info, grads = self._losses(batch, noise, True)
        info.update(O.OracleFQL.grad_stats(grads))
        self.apply_gradients(grads)
        return loss, {k: float(info[k]) for k in INFO_KEYS}

    def sample_actions(self, observations, noises):
        """agents/bc.py:86-101 with explicit x ~ N(0, I): S Euler steps, then the squeeze ([1, od] -> [act]) and the clip."""
        obs = self._c(observations)
        obs = obs[None] if obs.ndim == 1 else obs
        x = self._c(noises).reshape(obs.shape[0], self.ad).copy()
        dt = self.dtype.type(1.0 / self.S)
        for i in range(self.S):
            x = x + self.policy(obs, x, i) * dt
        x = x[0] if obs.shape[0] == 1 else x
        return np.clip(x, -1, 1)


def make_noise(batch_size, act_dim, denoise_steps, seed):
    """x0 ~ N(0, I) and t = k / S with k ~ randint[0, S]; rows 0 and 1 hold k = 0 and k = S (when B >= 2)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, denoise_steps + 1, size=batch_size)
    if batch_size >= 2:
        k[0], k[1] = 0, denoise_steps
    return {'x0': rng.standard_normal((batch_size, act_dim)).astype(np.float32),
            't': (k.astype(np.float32) / np.float32(denoise_steps)).astype(np.float32)}


__all__ = ['OracleBC', 'INFO_KEYS', 'get_config', 'init_params', 'make_noise', 'lecun_normal']
