"""fp64 numpy restatement of the reference's SACAgent (agents/sac.py) with explicit noise: the CPU oracle of the SAC engine (RLPD's
learner).

It reuses the MLP / LayerNorm / GELU helpers and the tree utilities of oracle/fql_oracle.py with a hand-derived backward pass.  The Actor
(utils/networks.py:82-150, tanh_squash, state_dependent_std) is actor_net (an MLP with activate_final: GELU, and with actor_layer_norm
LayerNorm, after every hidden Dense) followed by two Dense heads, mean_net and log_std_net: as one MLP, actor_net's Dense_0..n-1 plus
both heads side by side as Dense_n ([H, 2 act]).  LogParam (utils/networks.py:64-72) is the 0-d leaf modules_alpha/log_value.
Noise of one update: eps1 = eps_n and eps2 = eps_c, each [B, act] raw N(0, 1) (agents/sac.py:27,62).

Gradients, as jax.grad gives them through distrax's sample_and_log_prob (x = mean + s eps; the Gaussian part of log_prob depends on the
mean only through x, so that dependence cancels):
    g_x = (alpha 2 a - (1 - a^2) dqbar/da) / B   (tanh),   -dqbar/da / B   (no tanh)
    dL/dmean = g_x,   dL/dls_raw = clipmask (g_x s eps - alpha / B),   dL/dlog_value = alpha (entropy - target_entropy)
clipmask is 1 strictly inside [-5, 2], 0 outside and 1/2 at a bound (jnp.clip's max / min split the gradient at a tie).
"""
import copy
import math

import numpy as np

from oracle import fql_oracle as O

INFO_KEYS = (
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/total_loss', 'actor/actor_loss', 'actor/alpha_loss', 'actor/alpha', 'actor/entropy', 'actor/std', 'actor/q',
    'grad/max', 'grad/min', 'grad/norm',
)
LOG_STD_MIN, LOG_STD_MAX = -5.0, 2.0


def get_config() -> dict:
    """agents/sac.py get_config."""
    return dict(agent_name='sac', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                target_entropy=None, target_entropy_multiplier=0.5, tanh_squash=True, state_dependent_std=True, actor_fc_scale=0.01,
                q_agg='min', backup_entropy=False, encoder=None)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/sac.py create: Glorot-uniform kernels, mean_net / log_std_net variance_scaling(actor_fc_scale, fan_avg, uniform), zero
    biases, LN scale 1, log_value = log(1) = 0; the target critic is a copy."""
    rng = np.random.default_rng(seed)
    vh, ah = tuple(config['value_hidden_dims']), tuple(config['actor_hidden_dims'])
    dims = (obs_dim + act_dim,) + vh + (1,)
    vnet = {}
    for i in range(len(dims) - 1):
        vnet[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, dims[i], dims[i + 1], (2, dims[i], dims[i + 1]), dtype),
                              'bias': np.zeros((2, dims[i + 1]), dtype)}
        if config['layer_norm'] and i + 1 < len(dims) - 1:
            vnet[f'LayerNorm_{i}'] = {'scale': np.ones((2, dims[i + 1]), dtype), 'bias': np.zeros((2, dims[i + 1]), dtype)}
    adims = (obs_dim,) + ah
    anet = {}
    for i in range(len(ah)):
        anet[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, adims[i], adims[i + 1], (adims[i], adims[i + 1]), dtype),
                              'bias': np.zeros((adims[i + 1],), dtype)}
        if config['actor_layer_norm']:
            anet[f'LayerNorm_{i}'] = {'scale': np.ones((adims[i + 1],), dtype), 'bias': np.zeros((adims[i + 1],), dtype)}
    lim = math.sqrt(6.0 * float(config['actor_fc_scale']) / (ah[-1] + act_dim))
    head = lambda: {'kernel': rng.uniform(-lim, lim, size=(ah[-1], act_dim)).astype(dtype), 'bias': np.zeros((act_dim,), dtype)}
    actor = {'actor_net': anet, 'mean_net': head(), 'log_std_net': head()}
    critic = {'value_net': vnet}
    return {'modules_actor': actor, 'modules_alpha': {'log_value': np.zeros((), dtype)}, 'modules_critic': critic,
            'modules_target_critic': copy.deepcopy(critic)}


def merged(actor):
    """The Actor as one MLP: actor_net's layers, then [mean_net | log_std_net] as the last Dense."""
    net = dict(actor['actor_net'])
    n = O._n_layers(actor['actor_net'])
    net[f'Dense_{n}'] = {'kernel': np.concatenate([actor['mean_net']['kernel'], actor['log_std_net']['kernel']], axis=1),
                         'bias': np.concatenate([actor['mean_net']['bias'], actor['log_std_net']['bias']])}
    return net


def split(grads, n_hidden, act_dim):
    """Gradients of `merged` back into the Actor's tree."""
    g = dict(grads)
    h = g[f'Dense_{n_hidden}']
    return {'actor_net': {k: v for k, v in g.items() if k != f'Dense_{n_hidden}'},
            'mean_net': {'kernel': h['kernel'][:, :act_dim], 'bias': h['bias'][:act_dim]},
            'log_std_net': {'kernel': h['kernel'][:, act_dim:], 'bias': h['bias'][act_dim:]}}


def softplus(y):
    return np.maximum(y, 0) + np.log1p(np.exp(-np.abs(y)))


def clip_mask(raw):
    """d clip(raw, -5, 2) / d raw as jnp.clip's max / min give it: 1 inside, 0 outside, 1/2 at a bound."""
    inside = (raw > LOG_STD_MIN) & (raw < LOG_STD_MAX)
    at = (raw == LOG_STD_MIN) | (raw == LOG_STD_MAX)
    return np.where(inside, 1.0, np.where(at, 0.5, 0.0)).astype(raw.dtype)


class OracleSAC(O.OracleFQL):
    """Restatement of SACAgent (agents/sac.py) with explicit noise."""

    entropy_override = None   # test hook: hold the entropy of alpha_loss (a stop_gradient in the reference) fixed for finite differences

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _nh(self):
        return O._n_layers(self.params['modules_actor']['actor_net'])

    def target_entropy(self):
        te = self.config.get('target_entropy')
        return -self.config['target_entropy_multiplier'] * self.act_dim if te is None else te

    def actor_heads(self, obs, keep=False, stored=False):
        """(mean, raw log-std[, cache])."""
        r = O.mlp_forward(merged(self._P(stored)['modules_actor']), self._c(obs), keep=keep)
        out = r[0] if keep else r
        m, raw = out[:, :self.act_dim], out[:, self.act_dim:]
        return (m, raw, r[1]) if keep else (m, raw)

    def sample(self, m, raw, eps, temperature=1.0):
        """distrax sample_and_log_prob of the (tanh-)Gaussian: (a, log_prob, x, s)."""
        dt = self.dtype.type
        ls = np.clip(raw, LOG_STD_MIN, LOG_STD_MAX)
        s = np.exp(ls) * dt(temperature)
        eps = self._c(eps)
        x = m + s * eps
        with np.errstate(divide='ignore'):   # (temperature 0: lp = +inf, unused by sample_actions)
            lp = np.sum(-0.5 * eps * eps - np.log(s) - 0.5 * math.log(2 * math.pi), axis=-1)
        if self.config['tanh_squash']:
            lp = lp - np.sum(2.0 * (math.log(2.0) - x - softplus(-2.0 * x)), axis=-1)
            a = np.tanh(x)
        else:
            a = x
        return a, lp, x, s

    def _losses(self, batch, noise, want_grads: bool):
        cfg = self.config
        dt = self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        nobs, rew, mask = self._c(batch['next_observations']), self._c(batch['rewards']), self._c(batch['masks'])
        B, A = act.shape
        alpha = np.exp(self._P(True)['modules_alpha']['log_value'])
        disc = dt(cfg['discount'])
        info = {}
        # critic loss (sac.py:23-56)
        mn, rn = self.actor_heads(nobs, stored=True)
        a_n, lp_n, _, _ = self.sample(mn, rn, noise['eps1'])
        tq = self._critic('modules_target_critic', nobs, a_n, stored=True)
        next_q = tq.min(axis=0) if cfg['q_agg'] == 'min' else tq.mean(axis=0)
        y = rew + disc * mask * next_q
        if cfg['backup_entropy']:
            y = y - disc * mask * lp_n * alpha
        q, c_caches = self._critic('modules_critic', obs, act, keep=True)
        critic_loss = np.mean(np.square(q - y))
        info.update({'critic/critic_loss': critic_loss, 'critic/q_mean': q.mean(), 'critic/q_max': q.max(), 'critic/q_min': q.min()})
        # actor loss (sac.py:58-92)
        m, raw, a_cache = self.actor_heads(obs, keep=True)
        a, lp, x, s = self.sample(m, raw, noise['eps2'])
        qs, q_caches = self._critic('modules_critic', obs, a, keep=True, stored=True)
        qbar = qs.mean(axis=0)
        actor_loss = np.mean(lp * alpha - qbar)
        alpha_g = np.exp(self.params['modules_alpha']['log_value'])
        entropy = -lp.mean() if self.entropy_override is None else dt(self.entropy_override)
        alpha_loss = alpha_g * (entropy - dt(self.target_entropy()))
        info.update({'actor/total_loss': actor_loss + alpha_loss, 'actor/actor_loss': actor_loss, 'actor/alpha_loss': alpha_loss,
                     'actor/alpha': alpha_g, 'actor/entropy': -lp.mean(), 'actor/std': s.mean(), 'actor/q': qbar.mean()})
        loss = critic_loss + actor_loss + alpha_loss
        if not want_grads:
            return loss, info, None
        grads = O.tree_map(np.zeros_like, self.params)
        gc = grads['modules_critic']['value_net']
        for e in range(2):
            dq = (2.0 / (2 * B)) * (q[e] - y)
            _, g = O.mlp_backward(self.params['modules_critic']['value_net'], c_caches[e], dq[:, None].astype(self.dtype), member=e)
            for ln, sub in g.items():
                for k, val in sub.items():
                    gc[ln][k][e] = val
        da = np.zeros_like(a)   # dL/da through -mean(qbar), stored critic
        for e in range(2):
            dq = np.full((B,), -0.5 / B, dtype=self.dtype)
            dx, _ = O.mlp_backward(self._P(True)['modules_critic']['value_net'], q_caches[e], dq[:, None], member=e,
                                   want_param_grads=False)
            da += dx[:, self.obs_dim:]
        if cfg['tanh_squash']:
            gx = alpha * 2.0 * a / B + (1.0 - a * a) * da
        else:
            gx = da
        dls = clip_mask(raw) * (gx * s * self._c(noise['eps2']) - alpha / B)
        dhead = np.concatenate([gx, dls], axis=1).astype(self.dtype)
        _, g = O.mlp_backward(merged(self.params['modules_actor']), a_cache, dhead)
        grads['modules_actor'] = split(g, self._nh(), A)
        grads['modules_alpha'] = {'log_value': np.asarray(alpha_g * (entropy - dt(self.target_entropy())), dtype=self.dtype)}
        return loss, info, grads

    def kink_margins(self, batch, noise):
        """Distance of every element from each point where the loss is not smooth: the raw log-std at -5 / 2 over all 2B actor rows
        (next observations under the stored parameters, observations under the differentiated ones), and q1 = q2 of the target pair
        where q_agg = 'min' takes the smaller (the actor loss takes the pair's mean)."""
        mn, rn = self.actor_heads(batch['next_observations'], stored=True)
        raw = np.concatenate([rn, self.actor_heads(batch['observations'])[1]])
        m = {'log_std_clip': float(np.minimum(np.abs(raw - LOG_STD_MIN), np.abs(raw - LOG_STD_MAX)).min())}
        if self.config['q_agg'] == 'min':
            a_n = self.sample(mn, rn, noise['eps1'])[0]
            tq = self._critic('modules_target_critic', self._c(batch['next_observations']), a_n, stored=True)
            m['q_tie'] = float(np.abs(tq[0] - tq[1]).min())
        return m

    def total_loss(self, batch, noise):
        loss, info, _ = self._losses(batch, noise, want_grads=False)
        return loss, info

    def apply_gradients(self, grads):
        """optax.adam over the whole tree (the target critic's zero gradients too), then Polyak of the target critic from the PRE-step
        critic (agents/sac.py:104-122)."""
        cfg = self.config
        dt = self.dtype.type
        b1, b2, eps, lr = dt(0.9), dt(0.999), dt(1e-8), dt(cfg['lr'])
        self.count += 1
        c1 = dt(1.0 - 0.9 ** self.count); c2 = dt(1.0 - 0.999 ** self.count)
        old_critic = copy.deepcopy(self.params['modules_critic'])

        def upd(p, g, m, v):
            m[...] = b1 * m + (dt(1) - b1) * g
            v[...] = b2 * v + (dt(1) - b2) * g * g
            return p - lr * (m / c1) / (np.sqrt(v / c2) + eps)

        for mod in ('modules_actor', 'modules_alpha', 'modules_critic'):
            self.params[mod] = O.tree_map(upd, self.params[mod], grads[mod], self.mu[mod], self.nu[mod])
        tau = dt(cfg['tau'])
        self.params['modules_target_critic'] = O.tree_map(lambda p, tp: p * tau + tp * (dt(1) - tau), old_critic,
                                                          self.params['modules_target_critic'])
        self.step += 1

    def update(self, batch, noise):
        """agents/sac.py update (+ utils/flax_utils.py:120-159)."""
        loss, info, grads = self._losses(batch, noise, want_grads=True)
        info.update(self.grad_stats(grads))
        self.apply_gradients(grads)
        return loss, {k: float(info[k]) for k in INFO_KEYS}

    def sample_actions(self, observations, noises, temperature=1.0):
        """agents/sac.py sample_actions with the normal draw passed in."""
        m, raw = self.actor_heads(observations, stored=True)
        a, _, _, _ = self.sample(m, raw, noises, temperature)
        return np.clip(a, -1, 1)


def make_noise(batch_size, act_dim, seed):
    rng = np.random.default_rng(seed)
    return {'eps1': rng.standard_normal((batch_size, act_dim)).astype(np.float32),
            'eps2': rng.standard_normal((batch_size, act_dim)).astype(np.float32)}


def randomize(params, seed, scale=0.3, ls_bias=(-1.0, 0.5)):
    """Parameters moved away from init so that the log-std clip and the tanh saturation occur: every leaf gets uniform noise and the
    log-std head a wide bias spread (a fixture and test helper)."""
    rng = np.random.default_rng(seed)
    p = O.tree_map(lambda a: (a + rng.uniform(-scale, scale, size=np.shape(a)) * (np.abs(a).max() if np.size(a) > 1 and
                                                                                   np.abs(a).max() > 0 else scale)).astype(a.dtype),
                   params)
    ls = p['modules_actor']['log_std_net']
    ls['bias'] = (ls['bias'] + rng.uniform(-6.0, 4.0, size=ls['bias'].shape)).astype(ls['bias'].dtype)
    mn = p['modules_actor']['mean_net']
    mn['bias'] = (mn['bias'] + rng.uniform(-3.0, 3.0, size=mn['bias'].shape)).astype(mn['bias'].dtype)
    p['modules_alpha']['log_value'] = np.asarray(rng.uniform(-1.0, 0.5), dtype=p['modules_alpha']['log_value'].dtype)
    p['modules_target_critic'] = O.tree_map(lambda a: (a + rng.uniform(-0.05, 0.05, size=np.shape(a))).astype(a.dtype),
                                            p['modules_critic'])
    return p
