"""torch-autograd restatement of the reference's IQLDiffusionAgent (agents/iql_diffusion.py, binary optimality family): the same math
as tests/iqld_oracle.py written the reference's way (a positive and an unconditional actor pass of B rows each, jnp.sort for the top-10
mass), gradients by autograd."""
import numpy as np
import torch

from oracle.fql_oracle import tree_leaves_with_path
from oracle.fql_oracle_torch import _map, _to_torch, _gelu, _layer_norm
from fql_amd.bc import timestep_embedding, grid_index


def _mlp(net, x, member=None, activate_final=False):
    leaf = (lambda a: a) if member is None else (lambda a: a[member])
    n = sum(1 for k in net if k.startswith('Dense_'))
    for i in range(n):
        x = x @ leaf(net[f'Dense_{i}']['kernel']) + leaf(net[f'Dense_{i}']['bias'])
        if i + 1 < n or activate_final:
            x = _gelu(x)
            if f'LayerNorm_{i}' in net:
                x = _layer_norm(x, leaf(net[f'LayerNorm_{i}']['scale']), leaf(net[f'LayerNorm_{i}']['bias']))
    return x


class TorchIQLD:
    def __init__(self, params, config, dtype=torch.float64):
        self.dtype = dtype
        self.params = _to_torch(params, dtype)
        self.config = dict(config)
        self.S = int(self.config['denoise_steps'])

    def _t(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dtype)

    def actor(self, p, obs, is_positive, x, k):
        emb = self._t(timestep_embedding(np.broadcast_to(np.asarray(k), (obs.shape[0],)), self.S))
        row = p['Embed_0']['embedding'][torch.full((obs.shape[0],), int(is_positive), dtype=torch.long)]
        h = _mlp(p['MLP_0'], torch.cat([obs, x, emb, row], dim=-1), activate_final=True)
        return h @ p['Dense_0']['kernel'] + p['Dense_0']['bias']

    def critic(self, p, obs, act):
        x = torch.cat([obs, act], dim=-1)
        return torch.stack([_mlp(p['value_net'], x, member=e)[:, 0] for e in range(2)])

    def value(self, p, obs):
        return _mlp(p['value_net'], obs)[:, 0]

    def critic_loss(self, batch, critic_params):
        P = self.params
        next_v = self.value(P['value'], self._t(batch['next_observations']))
        target_q = self._t(batch['rewards']) + self.config['discount'] * self._t(batch['masks']) * next_v
        qs = self.critic(critic_params, self._t(batch['observations']), self._t(batch['actions']))
        return ((qs - target_q[None]) ** 2).mean()

    def value_loss(self, batch, value_params):
        qs = self.critic(self.params['target_critic'], self._t(batch['observations']), self._t(batch['actions']))
        d = torch.min(qs, dim=0).values - self.value(value_params, self._t(batch['observations']))
        w = torch.where(d > 0, torch.full_like(d, self.config['expectile']), torch.full_like(d, 1 - self.config['expectile']))
        return (w * d ** 2).mean()

    def loss_weight(self, batch):
        P, cfg = self.params, self.config
        obs, act = self._t(batch['observations']), self._t(batch['actions'])
        qs = self.critic(P['target_critic'] if cfg['target_extraction'] else P['critic'], obs, act)
        adv = torch.min(qs, dim=0).values - self.value(P['value'], obs)
        ov = cfg['optimal_var']
        if ov == 'binary':
            return (adv > 0).to(self.dtype)
        if ov == 'binary_awr_loss':
            w = torch.where(adv > 0, torch.clip(torch.exp(adv * cfg['awr_temperature']), 0, 1e8), torch.zeros_like(adv))
            return torch.minimum(w, torch.full_like(w, 100.0))
        e = torch.where(adv > 0, torch.clip(torch.exp(adv * cfg['softmax_beta']), 0, 1e8), torch.zeros_like(adv))
        return e / (e.sum() + 1e-8)

    def actor_loss(self, batch, noise, actor_params):
        obs, a, x0 = self._t(batch['observations']), self._t(batch['actions']), self._t(noise['x0'])
        w = self.loss_weight(batch).detach()
        k = grid_index(noise['t'], self.S)
        t = self._t(k.astype(np.float32) / np.float32(self.S))[:, None]
        x_t, vel = x0 * (1 - t) + a * t, a - x0
        lp = ((vel - self.actor(actor_params, obs, 1, x_t, k)) ** 2).mean(dim=-1) * w
        lu = ((vel - self.actor(actor_params, obs, 0, x_t, k)) ** 2).mean(dim=-1)
        sw = torch.sort(w).values
        top = sw[-int(0.1 * len(sw)):].sum() / (sw.sum() + 1e-8)
        return (lp + lu * 0.1).mean(), {'loss_weights_top_10_mass': float(top), 'effective_batch_size': float(w.sum() ** 2 / ((w ** 2).sum() + 1e-8))}

    def grads(self, batch, noise):
        """({net: loss}, {net: gradient tree}) of the three trained nets, each with the others at their stored values."""
        losses, out = {}, {}
        for net, fn in (('critic', lambda p: self.critic_loss(batch, p)), ('value', lambda p: self.value_loss(batch, p)),
                        ('actor', lambda p: self.actor_loss(batch, noise, p)[0])):
            p = _map(lambda v: v.clone().requires_grad_(True), self.params[net])
            loss = fn(p)
            loss.backward()
            losses[net], out[net] = float(loss.detach()), _map(lambda v: v.grad, p)
        return losses, out

    def sample_actions(self, observations, noises, cfg=1.0):
        obs = self._t(observations)
        obs = obs[None] if obs.ndim == 1 else obs
        x = self._t(noises).reshape(obs.shape[0], -1).clone()
        with torch.no_grad():
            for i in range(self.S):
                vp, vu = self.actor(self.params['actor'], obs, 1, x, i), self.actor(self.params['actor'], obs, 0, x, i)
                x = x + (vu + cfg * (vp - vu)) / self.S
        x = x[0] if obs.shape[0] == 1 else x
        return torch.clip(x, -1, 1).numpy()


def leaves(tree):
    return {p: (v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v)) for p, v in tree_leaves_with_path(tree)}
