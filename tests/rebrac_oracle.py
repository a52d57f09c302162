"""fp64 numpy restatement of the reference's ReBRACAgent (agents/rebrac.py) with explicit noise: the CPU oracle of the ReBRAC engine.

It reuses the MLP / LayerNorm / GELU helpers and the tree utilities of oracle/fql_oracle.py with a hand-derived backward pass.  The Actor
(utils/networks.py:82-150) is actor_net (an MLP with activate_final, so every hidden Dense has GELU and, with actor_layer_norm, LayerNorm)
followed by mean_net: as one MLP, actor_net's Dense_0..n-1 plus mean_net as Dense_n.  Noise of one update: eps1 [B, act], the raw N(0, 1)
of the target-policy noise (agents/rebrac.py:30-34).
"""
import copy
import math

import numpy as np

from oracle import fql_oracle as O

INFO_KEYS = (
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/total_loss', 'actor/actor_loss', 'actor/bc_loss', 'actor/std', 'actor/mse',
    'grad/max', 'grad/min', 'grad/norm',
)
CRITIC_INFO_KEYS = INFO_KEYS[:4] + INFO_KEYS[9:]


def get_config() -> dict:
    """agents/rebrac.py:222-244."""
    return dict(agent_name='rebrac', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                tanh_squash=True, actor_fc_scale=0.01, alpha_actor=0.0, alpha_critic=0.0, actor_freq=2, actor_noise=0.2,
                actor_noise_clip=0.5, encoder=None)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/rebrac.py:182-219: Glorot-uniform kernels, mean_net variance_scaling(actor_fc_scale, fan_avg, uniform), zero biases,
    LN scale 1; both targets are copies."""
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
    actor = {'actor_net': anet, 'mean_net': {'kernel': rng.uniform(-lim, lim, size=(ah[-1], act_dim)).astype(dtype),
                                             'bias': np.zeros((act_dim,), dtype)}}
    critic = {'value_net': vnet}
    return {'modules_actor': actor, 'modules_critic': critic,
            'modules_target_actor': copy.deepcopy(actor), 'modules_target_critic': copy.deepcopy(critic)}


def merged(actor):
    """The Actor as one MLP: actor_net's layers, then mean_net as the last Dense."""
    net = dict(actor['actor_net'])
    net[f'Dense_{O._n_layers(actor["actor_net"])}'] = actor['mean_net']
    return net


def split(grads, n_hidden):
    """Gradients of `merged` back into the Actor's tree."""
    g = dict(grads)
    return {'actor_net': {k: v for k, v in g.items() if k != f'Dense_{n_hidden}'}, 'mean_net': g[f'Dense_{n_hidden}']}


class OracleReBRAC(O.OracleFQL):
    """Restatement of ReBRACAgent (agents/rebrac.py:16-219) with explicit noise."""

    lam_override = None   # test hook: hold lam (a stop_gradient in the reference) fixed for finite differences

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _nh(self):
        return O._n_layers(self.params['modules_actor']['actor_net'])

    def _mode(self, mean):
        return np.tanh(mean) if self.config['tanh_squash'] else mean

    def actor_mean(self, name, obs, keep=False, stored=False):
        return O.mlp_forward(merged(self._P(stored)[name]), self._c(obs), keep=keep)

    def _losses(self, batch, noise, want_grads: bool, full_update=True):
        cfg = self.config
        dt = self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        nobs, nact = self._c(batch['next_observations']), self._c(batch['next_actions'])
        rew, mask = self._c(batch['rewards']), self._c(batch['masks'])
        B, A = act.shape
        info = {}
        # critic loss (:26-53)
        nz = np.clip(self._c(noise['eps1']) * dt(cfg['actor_noise']), -dt(cfg['actor_noise_clip']), dt(cfg['actor_noise_clip']))
        a_next = np.clip(self._mode(self.actor_mean('modules_target_actor', nobs, stored=True)) + nz, -1, 1)
        tq = self._critic('modules_target_critic', nobs, a_next, stored=True)
        next_q = tq.min(axis=0) - dt(cfg['alpha_critic']) * np.square(a_next - nact).sum(axis=-1)
        y = rew + dt(cfg['discount']) * mask * next_q
        q, c_caches = self._critic('modules_critic', obs, act, keep=True)
        critic_loss = np.mean(np.square(q - y))
        info.update({'critic/critic_loss': critic_loss, 'critic/q_mean': q.mean(), 'critic/q_max': q.max(), 'critic/q_min': q.min()})
        loss = critic_loss
        if full_update:   # actor loss (:55-84)
            mean, a_cache = self.actor_mean('modules_actor', obs, keep=True)
            a = self._mode(mean)
            qs, q_caches = self._critic('modules_critic', obs, a, keep=True, stored=True)
            qm = qs.min(axis=0)
            mse = np.square(a - act).sum(axis=-1)
            lam = dt(1) / np.abs(qm).mean() if self.lam_override is None else dt(self.lam_override)
            actor_loss = -(lam * qm).mean()
            bc_loss = (dt(cfg['alpha_actor']) * mse).mean()
            info.update({'actor/total_loss': actor_loss + bc_loss, 'actor/actor_loss': actor_loss, 'actor/bc_loss': bc_loss,
                         'actor/std': dt(1.0), 'actor/mse': mse.mean(), '_lam': lam})
            loss = loss + actor_loss + bc_loss
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
        if full_update:
            # d min / d q_e: 1 for the smaller member, 1/2 each at a tie (jnp.min's gradient)
            w = [np.where(qs[0] < qs[1], 1.0, np.where(qs[0] == qs[1], 0.5, 0.0)),
                 np.where(qs[1] < qs[0], 1.0, np.where(qs[0] == qs[1], 0.5, 0.0))]
            da = np.zeros_like(a)
            for e in range(2):
                dq = (-lam / B) * w[e]
                dx, _ = O.mlp_backward(self._P(True)['modules_critic']['value_net'], q_caches[e], dq[:, None].astype(self.dtype),
                                       member=e, want_param_grads=False)
                da += dx[:, self.obs_dim:]
            da += dt(cfg['alpha_actor']) * 2.0 / B * (a - act)
            dmean = da * (1 - a * a) if cfg['tanh_squash'] else da
            _, g = O.mlp_backward(merged(self.params['modules_actor']), a_cache, dmean.astype(self.dtype))
            grads['modules_actor'] = split(g, self._nh())
        return loss, info, grads

    def kink_margins(self, batch, noise=None):
        """Distance of every row from the one point where a full step's loss is not smooth in what it differentiates: q1 = q2 of the
        stored critic pair at (obs, actor action), where the actor loss takes the smaller (tests/sac_oracle.py's q_tie: the smallest
        |q1 - q2| over the rows, unnormalised).  The target side (noise clip, action clip, min of the target pair) carries no gradient
        and is continuous, so it needs no margin, and `noise` is not read: the actor's action is its mode."""
        a = self._mode(self.actor_mean('modules_actor', batch['observations']))
        qs = self._critic('modules_critic', self._c(batch['observations']), a, stored=True)
        return {'q_tie': float(np.abs(qs[0] - qs[1]).min())}

    def total_loss(self, batch, noise, full_update=True):
        loss, info, _ = self._losses(batch, noise, want_grads=False, full_update=full_update)
        info.pop('_lam', None)
        return loss, info

    def apply_gradients(self, grads, full_update=True):
        """optax.adam over modules_actor and modules_critic (every leaf, also on critic-only steps), then - full steps only - Polyak of
        both targets from the PRE-step critic and actor (agents/rebrac.py:112-133)."""
        cfg = self.config
        dt = self.dtype.type
        b1, b2, eps, lr = dt(0.9), dt(0.999), dt(1e-8), dt(cfg['lr'])
        self.count += 1
        c1 = dt(1.0 - 0.9 ** self.count); c2 = dt(1.0 - 0.999 ** self.count)
        old = {m: copy.deepcopy(self.params[m]) for m in ('modules_actor', 'modules_critic')}

        def upd(p, g, m, v):
            m[...] = b1 * m + (dt(1) - b1) * g
            v[...] = b2 * v + (dt(1) - b2) * g * g
            return p - lr * (m / c1) / (np.sqrt(v / c2) + eps)

        for mod in ('modules_actor', 'modules_critic'):
            self.params[mod] = O.tree_map(upd, self.params[mod], grads[mod], self.mu[mod], self.nu[mod])
        if full_update:
            tau = dt(cfg['tau'])
            for mod in ('actor', 'critic'):
                self.params[f'modules_target_{mod}'] = O.tree_map(lambda p, tp: p * tau + tp * (dt(1) - tau), old[f'modules_{mod}'],
                                                                  self.params[f'modules_target_{mod}'])
        self.step += 1

    def update(self, batch, noise, full_update=True):
        """agents/rebrac.py:122-134 (+ utils/flax_utils.py:120-159)."""
        loss, info, grads = self._losses(batch, noise, want_grads=True, full_update=full_update)
        info.update(self.grad_stats(grads))
        self.apply_gradients(grads, full_update)
        keys = INFO_KEYS if full_update else CRITIC_INFO_KEYS
        return loss, {k: float(info[k]) for k in keys}

    def sample_actions(self, observations, noises, temperature=1.0):
        """agents/rebrac.py:136-152 with the normal draw passed in."""
        dt = self.dtype.type
        a = self._mode(self.actor_mean('modules_actor', observations, stored=True))
        nz = np.clip(self._c(noises) * dt(self.config['actor_noise']) * dt(temperature), -dt(self.config['actor_noise_clip']),
                     dt(self.config['actor_noise_clip']))
        return np.clip(a + nz, -1, 1)


def next_actions(actions, idxs, size):
    """utils/datasets.py:96-100: actions[min(idxs + 1, size - 1)]."""
    return actions[np.minimum(np.asarray(idxs) + 1, size - 1)]


def make_batch(ds, idxs):
    b = O.sample_batch(ds, idxs)
    b['next_actions'] = next_actions(ds['actions'], idxs, len(ds['actions']))
    return b


def make_noise(batch_size, act_dim, seed):
    return {'eps1': np.random.default_rng(seed).standard_normal((batch_size, act_dim)).astype(np.float32)}
