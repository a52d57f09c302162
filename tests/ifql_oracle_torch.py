"""Torch-autograd restatement of the reference's IFQLAgent (agents/ifql.py): the second, independent CPU oracle of the IFQL engine.

Gradients come from torch.autograd on a direct transcription of agents/ifql.py:25-98; the "no params => stored, constant" rule of
utils/flax_utils.py:90-118 is `.detach()` on the stored tree; Adam is optax.adam's rule and Polyak reads the pre-step critic (:100-120).
It shares no code with tests/ifql_oracle.py's hand-derived backward (only the MLP / LayerNorm / GELU transcription of
oracle/fql_oracle_torch.py).  tests/test_ifql_cpu.py checks the two against each other.
"""
import torch

from oracle.fql_oracle import tree_leaves_with_path
from oracle.fql_oracle_torch import _map, _mlp, _to_torch

INFO_KEYS = (
    'value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
    'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min',
    'actor/actor_loss', 'grad/max', 'grad/min', 'grad/norm',
)


def _critic(mod, obs, act):
    x = torch.cat([obs, act], -1)
    return torch.stack([_mlp(mod['value_net'], x, e).squeeze(-1) for e in range(2)], 0)


def _value(mod, obs):
    return _mlp(mod['value_net'], obs).squeeze(-1)


class TorchIFQL:
    def __init__(self, params, config, dtype=torch.float64):
        self.dtype = dtype
        self.config = dict(config)
        self.params = _to_torch(params, dtype)
        self.mu = _map(torch.zeros_like, self.params)
        self.nu = _map(torch.zeros_like, self.params)
        self.count = 0

    def _t(self, a):
        return torch.as_tensor(a, dtype=self.dtype)

    def total_loss(self, batch, noise, grad_params=None):
        """agents/ifql.py:79-98 with explicit x_0 and t."""
        cfg = self.config
        stored = _map(lambda p: p.detach(), self.params)
        gp = stored if grad_params is None else grad_params
        obs, act, nobs = self._t(batch['observations']), self._t(batch['actions']), self._t(batch['next_observations'])
        rew, mask = self._t(batch['rewards']).reshape(-1), self._t(batch['masks']).reshape(-1)
        # value_loss :31-43
        q = _critic(stored['modules_target_critic'], obs, act).min(0).values
        v = _value(gp['modules_value'], obs)
        adv = q - v
        weight = torch.where(adv >= 0, torch.tensor(cfg['expectile'], dtype=self.dtype),
                             torch.tensor(1 - cfg['expectile'], dtype=self.dtype))
        value_loss = (weight * adv ** 2).mean()
        # critic_loss :45-58
        y = rew + cfg['discount'] * mask * _value(stored['modules_value'], nobs)
        q1, q2 = _critic(gp['modules_critic'], obs, act)
        critic_loss = ((q1 - y) ** 2 + (q2 - y) ** 2).mean()
        # actor_loss :60-77
        x0, t = self._t(noise['x0']), self._t(noise['t']).reshape(-1, 1)
        x_t = (1 - t) * x0 + t * act
        pred = _mlp(gp['modules_actor_flow']['mlp'], torch.cat([obs, x_t, t], -1))
        actor_loss = ((pred - (act - x0)) ** 2).mean()
        info = {'value/value_loss': value_loss, 'value/v_mean': v.mean(), 'value/v_max': v.max(), 'value/v_min': v.min(),
                'critic/critic_loss': critic_loss, 'critic/q_mean': y.mean(), 'critic/q_max': y.max(), 'critic/q_min': y.min(),
                'actor/actor_loss': actor_loss}
        return value_loss + critic_loss + actor_loss, info

    def grads(self, batch, noise):
        gp = _map(lambda p: p.detach().clone().requires_grad_(True), self.params)
        loss, info = self.total_loss(batch, noise, grad_params=gp)
        loss.backward()
        return loss.detach(), info, _map(lambda p: torch.zeros_like(p) if p.grad is None else p.grad, gp)

    def update(self, batch, noise):
        """agents/ifql.py:108-120 + utils/flax_utils.py:120-159."""
        cfg = self.config
        loss, info, grads = self.grads(batch, noise)
        leaves = [g for _, g in tree_leaves_with_path(grads)]
        info = {k: float(v.detach()) for k, v in info.items()}
        info['grad/max'] = max(float(g.max()) for g in leaves)
        info['grad/min'] = min(float(g.min()) for g in leaves)
        info['grad/norm'] = float(sum(torch.linalg.norm(g.reshape(-1)) for g in leaves))
        self.count += 1
        c1, c2 = 1 - 0.9 ** self.count, 1 - 0.999 ** self.count
        old_c = _map(lambda p: p.clone(), self.params['modules_critic'])
        old_t = self.params['modules_target_critic']

        def adam(p, g, m, v):
            m.mul_(0.9).add_(g, alpha=0.1)
            v.mul_(0.999).addcmul_(g, g, value=0.001)
            return p - cfg['lr'] * (m / c1) / (torch.sqrt(v / c2) + 1e-8)

        with torch.no_grad():
            self.params = _map(adam, self.params, grads, self.mu, self.nu)
            tau = cfg['tau']
            self.params['modules_target_critic'] = _map(lambda p, tp: p * tau + tp * (1 - tau), old_c, old_t)
        return float(loss), {k: info[k] for k in INFO_KEYS}

    def sample_actions(self, observation, noises):
        """agents/ifql.py:123-155 for one observation [od] and noises [N, act]."""
        with torch.no_grad():
            n = int(self.config['flow_steps'])
            a = self._t(noises)
            obs = self._t(observation).unsqueeze(0).expand(a.shape[0], -1)
            for i in range(n):
                t = torch.full((a.shape[0], 1), i / n, dtype=self.dtype)
                a = a + _mlp(self.params['modules_actor_flow']['mlp'], torch.cat([obs, a, t], -1)) / n
            a = torch.clamp(a, -1, 1)
            q = _critic(self.params['modules_critic'], obs, a).min(0).values
            return a[int(torch.argmax(q))], q
