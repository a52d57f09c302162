"""torch-autograd restatement of the reference's CFGRLAgent (agents/cfgrl.py) in the reference's own form: goals = where(do_cfg,
unc_embed, actor_goals) and autograd through the where, so the gradient of unc_embed is whatever the dropped rows send back."""
import numpy as np
import torch

from oracle.fql_oracle import tree_leaves_with_path
from oracle.fql_oracle_torch import _map, _to_torch, _gelu, _layer_norm

FLOW, EMBED = 'modules_actor_flow', 'modules_unc_embed'


def _flow(params, x):
    mlp = params[FLOW]['mlp']
    n = sum(1 for k in mlp if k.startswith('Dense_'))
    for i in range(n):   # MLP(activate_final=False): GELU and LayerNorm behind every Dense but the last
        x = x @ mlp[f'Dense_{i}']['kernel'] + mlp[f'Dense_{i}']['bias']
        if i + 1 < n:
            x = _gelu(x)
            if f'LayerNorm_{i}' in mlp:
                x = _layer_norm(x, mlp[f'LayerNorm_{i}']['scale'], mlp[f'LayerNorm_{i}']['bias'])
    return x


class TorchCFGRL:
    def __init__(self, params, config, dtype=torch.float64):
        self.dtype = dtype
        self.params = _to_torch(params, dtype)
        self.config = dict(config)
        self.S = int(self.config['flow_steps'])
        self.mu = _map(torch.zeros_like, self.params)
        self.nu = _map(torch.zeros_like, self.params)
        self.count = 0

    def _t(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dtype)

    def policy_loss(self, batch, noise, do_cfg, params=None):
        params = self.params if params is None else params
        a, x0 = self._t(batch['actions']), self._t(noise['x0'])
        t = self._t(noise['t']).reshape(-1, 1)
        x_t = (1 - t) * x0 + t * a
        vel = a - x0
        unc = params[EMBED]['Embed_0']['embedding']   # (1, goal_dim)
        drop = torch.as_tensor(np.asarray(do_cfg).astype(bool))
        goals = torch.where(drop[:, None], unc, self._t(batch['actor_goals']))
        pred = _flow(params, torch.cat([self._t(batch['observations']), goals, x_t, t], dim=-1))
        return torch.mean((pred - vel) ** 2)

    def grads(self, batch, noise, do_cfg):
        params = _map(lambda p: p.clone().requires_grad_(True), self.params)
        loss = self.policy_loss(batch, noise, do_cfg, params)
        loss.backward()
        return float(loss.detach()), _map(lambda p: p.grad if p.grad is not None else torch.zeros_like(p), params)

    def update(self, batch, noise, do_cfg):
        loss, g = self.grads(batch, noise, do_cfg)
        self.count += 1
        c1, c2, lr = 1.0 - 0.9 ** self.count, 1.0 - 0.999 ** self.count, float(self.config['lr'])

        def adam(p, g, m, v):
            m.mul_(0.9).add_(0.1 * g)
            v.mul_(0.999).add_(0.001 * g * g)
            return p - lr * (m / c1) / (torch.sqrt(v / c2) + 1e-8)

        self.params = _map(adam, self.params, g, self.mu, self.nu)
        return loss, g

    def sample_actions(self, observations, goals, noises, cfg=None):
        cfg = float(self.config['cfg'] if cfg is None else cfg)
        obs = self._t(observations)
        obs = obs[None] if obs.ndim == 1 else obs
        n = obs.shape[0]
        unc = self.params[EMBED]['Embed_0']['embedding']
        g = self._t(goals).reshape(-1, unc.shape[1]).expand(n, -1)
        u = unc.expand(n, -1)
        x = self._t(noises).reshape(n, -1).clone()
        with torch.no_grad():
            for i in range(self.S):
                t = torch.full((n, 1), i / self.S, dtype=self.dtype)
                vu = _flow(self.params, torch.cat([obs, u, x, t], dim=-1))
                vc = _flow(self.params, torch.cat([obs, g, x, t], dim=-1))
                x = x + (vu + cfg * (vc - vu)) / self.S
        x = x[0] if n == 1 else x
        return torch.clip(x, -1, 1).numpy()


def leaves(tree):
    return {p: (v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v)) for p, v in tree_leaves_with_path(tree)}
