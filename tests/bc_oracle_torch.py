"""torch-autograd restatement of the reference's BCAgent (agents/bc.py): the same math as tests/bc_oracle.py, gradients by autograd."""
import numpy as np
import torch

from oracle.fql_oracle import tree_leaves_with_path
from oracle.fql_oracle_torch import _map, _to_torch, _gelu, _layer_norm
from fql_amd.bc import timestep_embedding, grid_index


def _policy(params, x):
    mlp = params['MLP_0']
    n = sum(1 for k in mlp if k.startswith('Dense_'))
    for i in range(n):   # MLP(activate_final=True): every Dense is followed by GELU and LayerNorm
        x = _gelu(x @ mlp[f'Dense_{i}']['kernel'] + mlp[f'Dense_{i}']['bias'])
        if f'LayerNorm_{i}' in mlp:
            x = _layer_norm(x, mlp[f'LayerNorm_{i}']['scale'], mlp[f'LayerNorm_{i}']['bias'])
    return x @ params['Dense_0']['kernel'] + params['Dense_0']['bias']


class TorchBC:
    def __init__(self, params, config, dtype=torch.float64):
        self.dtype = dtype
        self.params = _to_torch(params, dtype)
        self.config = dict(config)
        self.S = int(self.config['denoise_steps'])
        self.mu = _map(torch.zeros_like, self.params)
        self.nu = _map(torch.zeros_like, self.params)
        self.count = 0

    def _t(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dtype)

    def policy(self, params, obs, x, k):
        emb = self._t(timestep_embedding(np.broadcast_to(np.asarray(k), (obs.shape[0],)), self.S))
        return _policy(params, torch.cat([obs, x, emb], dim=-1))

    def policy_loss(self, batch, noise, params=None):
        params = self.params if params is None else params
        a, x0 = self._t(batch['actions']), self._t(noise['x0'])
        k = grid_index(noise['t'], self.S)
        t = self._t(k.astype(np.float32) / np.float32(self.S))[:, None]
        pred = self.policy(params, self._t(batch['observations']), x0 * (1 - t) + a * t, k)
        return torch.mean((a - x0 - pred) ** 2)

    def grads(self, batch, noise):
        params = _map(lambda p: p.clone().requires_grad_(True), self.params)
        loss = self.policy_loss(batch, noise, params)
        loss.backward()
        return float(loss.detach()), _map(lambda p: p.grad, params)

    def update(self, batch, noise):
        loss, g = self.grads(batch, noise)
        self.count += 1
        c1, c2, lr = 1.0 - 0.9 ** self.count, 1.0 - 0.999 ** self.count, float(self.config['bc_lr'])

        def adam(p, g, m, v):
            m.mul_(0.9).add_(0.1 * g)
            v.mul_(0.999).add_(0.001 * g * g)
            return p - lr * (m / c1) / (torch.sqrt(v / c2) + 1e-8)

        self.params = _map(adam, self.params, g, self.mu, self.nu)
        return loss, g

    def sample_actions(self, observations, noises):
        obs = self._t(observations)
        obs = obs[None] if obs.ndim == 1 else obs
        x = self._t(noises).reshape(obs.shape[0], -1).clone()
        with torch.no_grad():
            for i in range(self.S):
                x = x + self.policy(self.params, obs, x, i) / self.S
        x = x[0] if obs.shape[0] == 1 else x
        return torch.clip(x, -1, 1).numpy()


def leaves(tree):
    return {p: (v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v)) for p, v in tree_leaves_with_path(tree)}
