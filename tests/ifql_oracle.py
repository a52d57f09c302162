"""fp64 numpy restatement of the reference's IFQLAgent (agents/ifql.py) with explicit noise: the CPU oracle of the IFQL engine.

It reuses the MLP / LayerNorm / GELU helpers, Adam and Polyak of oracle/fql_oracle.py (OracleFQL.apply_gradients reads the PRE-step critic
for Polyak, agents/ifql.py:100-120 is the same code as FQL's).  Noise of one update: x0 [B, act], t [B] (agents/ifql.py:64-66).
"""
import numpy as np

from oracle import fql_oracle as O

INFO_KEYS = (
    'value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm',
)


def get_config() -> dict:
    """agents/ifql.py:231-250."""
    return dict(agent_name='ifql', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                expectile=0.9, num_samples=32, flow_steps=10, encoder=None)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/ifql.py:188-225: Glorot-uniform kernels, zero biases, LN scale 1; value is a 1-member (unstacked) Value; target := critic."""
    rng = np.random.default_rng(seed)

    def mlp(in_dim, hidden, out_dim, ln, members=None):
        net, dims = {}, [in_dim] + list(hidden) + [out_dim]
        lead = () if members is None else (members,)
        for i in range(len(dims) - 1):
            net[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, dims[i], dims[i + 1], lead + (dims[i], dims[i + 1]), dtype),
                                 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
            if ln and i < len(dims) - 2:
                net[f'LayerNorm_{i}'] = {'scale': np.ones(lead + (dims[i + 1],), dtype), 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
        return net

    vh, ah = config['value_hidden_dims'], config['actor_hidden_dims']
    critic = {'value_net': mlp(obs_dim + act_dim, vh, 1, config['layer_norm'], 2)}
    return {
        'modules_actor_flow': {'mlp': mlp(obs_dim + act_dim + 1, ah, act_dim, config['actor_layer_norm'])},
        'modules_critic': critic,
        'modules_target_critic': O.tree_map(np.copy, critic),
        'modules_value': {'value_net': mlp(obs_dim, vh, 1, config['layer_norm'])},
    }


class OracleIFQL(O.OracleFQL):
    """Restatement of IFQLAgent (agents/ifql.py:15-228) with explicit noise."""

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _value(self, obs, keep=False, stored=False):
        r = O.mlp_forward(self._P(stored)['modules_value']['value_net'], self._c(obs), keep=keep)
        return (r[0][:, 0], r[1]) if keep else r[:, 0]

    def _losses(self, batch, noise, want_grads: bool):
        cfg = self.config
        dt = self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        nobs = self._c(batch['next_observations'])
        rew, mask = self._c(batch['rewards']), self._c(batch['masks'])
        B, A = act.shape
        info = {}
        # value loss (:31-43): target critic at (obs, act), expectile weight with >= 0
        tq = self._critic('modules_target_critic', obs, act, stored=True)
        q = np.minimum(tq[0], tq[1])
        v, v_cache = self._value(obs, keep=True)
        diff = q - v
        w = np.where(diff >= 0, dt(cfg['expectile']), dt(1 - cfg['expectile']))
        value_loss = np.mean(w * diff ** 2)
        info.update({'value/value_loss': value_loss, 'value/v_mean': v.mean(), 'value/v_max': v.max(), 'value/v_min': v.min()})
        # critic loss (:45-58): stored value at next_obs, SUM over members, mean over B; stats of the target y
        y = rew + dt(cfg['discount']) * mask * self._value(nobs, stored=True)
        cq, c_caches = self._critic('modules_critic', obs, act, keep=True)
        critic_loss = np.mean((cq[0] - y) ** 2 + (cq[1] - y) ** 2)
        info.update({'critic/critic_loss': critic_loss, 'critic/q_mean': y.mean(), 'critic/q_max': y.max(), 'critic/q_min': y.min()})
        # actor loss (:60-77): flow matching
        x0, t = self._c(noise['x0']), self._c(noise['t']).reshape(B, 1)
        x_t = (1 - t) * x0 + t * act
        vel = act - x0
        pred, a_cache = self._actor('modules_actor_flow', obs, x_t, t, keep=True)
        actor_loss = np.mean((pred - vel) ** 2)
        info['actor/actor_loss'] = actor_loss
        loss = value_loss + critic_loss + actor_loss
        if not want_grads:
            return loss, info, None
        grads = O.tree_map(np.zeros_like, self.params)
        dv = (-2.0 / B) * w * diff
        _, grads['modules_value']['value_net'] = O.mlp_backward(self.params['modules_value']['value_net'], v_cache,
                                                                dv[:, None].astype(self.dtype))
        gc = grads['modules_critic']['value_net']
        for e in range(2):
            dq = (2.0 / B) * (cq[e] - y)
            _, g = O.mlp_backward(self.params['modules_critic']['value_net'], c_caches[e], dq[:, None].astype(self.dtype), member=e)
            for ln, sub in g.items():
                for k, val in sub.items():
                    gc[ln][k][e] = val
        dpred = (2.0 / (B * A)) * (pred - vel)
        _, grads['modules_actor_flow']['mlp'] = O.mlp_backward(self.params['modules_actor_flow']['mlp'], a_cache, dpred.astype(self.dtype))
        return loss, info, grads

    def update(self, batch, noise):
        """agents/ifql.py:108-120 (+ utils/flax_utils.py:120-159)."""
        loss, info, grads = self._losses(batch, noise, want_grads=True)
        info.update(self.grad_stats(grads))
        self.apply_gradients(grads)
        return loss, {k: float(info[k]) for k in INFO_KEYS}

    def compute_flow_actions(self, observations, noises):
        """The Euler flow of actor_flow (agents/ifql.py:143-147), clipped (:148)."""
        obs, a = self._c(observations), self._c(noises)
        n = int(self.config['flow_steps'])
        for i in range(n):
            t = np.full(obs.shape[:-1] + (1,), i / n, dtype=self.dtype)
            a = a + self._actor('modules_actor_flow', obs, a, t, stored=True) / self.dtype.type(n)
        return np.clip(a, -1, 1)

    def sample_actions(self, observation, noises):
        """agents/ifql.py:123-155 for ONE observation [od] and noises [N, act]: best of N by min(q1, q2), first argmax."""
        N = noises.shape[0]
        obs = np.repeat(self._c(observation)[None], N, axis=0)
        acts = self.compute_flow_actions(obs, noises)
        q = self._critic('modules_critic', obs, acts, stored=True).min(axis=0)
        return acts[int(np.argmax(q))], q
