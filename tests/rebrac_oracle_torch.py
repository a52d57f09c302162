"""torch-autograd restatement of ReBRACAgent.total_loss (agents/rebrac.py:26-108), fp64 on the CPU: an independent check of the hand-derived
backward pass in tests/rebrac_oracle.py.  The stored critic of the actor loss and lam are constants, as in the reference (the actor loss
calls the critic without grad_params; lam is a stop_gradient); the targets are constants."""
import numpy as np
import torch

from oracle import fql_oracle as O

SQRT_2_OVER_PI = float(np.sqrt(2.0 / np.pi))


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(SQRT_2_OVER_PI * (x + 0.044715 * x ** 3)))


def _ln(x, scale, bias):
    mean = x.mean(-1, keepdim=True)
    var = torch.clamp((x * x).mean(-1, keepdim=True) - mean * mean, min=0.0)
    return (x - mean) / torch.sqrt(var + O.LN_EPS) * scale + bias


def _mlp(net, x, member=None):
    leaf = (lambda a: a) if member is None else (lambda a: a[member])
    n = sum(1 for k in net if k.startswith('Dense_'))
    for i in range(n):
        x = x @ leaf(net[f'Dense_{i}']['kernel']) + leaf(net[f'Dense_{i}']['bias'])
        if i + 1 < n:
            x = _gelu(x)
            if f'LayerNorm_{i}' in net:
                x = _ln(x, leaf(net[f'LayerNorm_{i}']['scale']), leaf(net[f'LayerNorm_{i}']['bias']))
    return x


def _actor(actor, x):
    net = dict(actor['actor_net'])
    net[f'Dense_{sum(1 for k in net if k.startswith("Dense_"))}'] = actor['mean_net']
    return _mlp(net, x)


def _critic(critic, obs, act):
    x = torch.cat([obs, act], -1)
    return torch.stack([_mlp(critic['value_net'], x, e)[:, 0] for e in range(2)])


def losses(params, config, batch, noise, full_update=True):
    """(loss, info, grads) with grads over modules_actor / modules_critic (zeros for the targets), all fp64 numpy."""
    P = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True), params)
    stored = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64)), params)
    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in batch.items()}
    mode = torch.tanh if config['tanh_squash'] else (lambda m: m)
    nz = torch.clamp(torch.tensor(np.asarray(noise['eps1'], np.float64)) * config['actor_noise'], -config['actor_noise_clip'],
                     config['actor_noise_clip'])
    a_next = torch.clamp(mode(_actor(stored['modules_target_actor'], t['next_observations'])) + nz, -1, 1)
    next_q = _critic(stored['modules_target_critic'], t['next_observations'], a_next).min(0).values
    next_q = next_q - config['alpha_critic'] * ((a_next - t['next_actions']) ** 2).sum(-1)
    y = t['rewards'] + config['discount'] * t['masks'] * next_q
    q = _critic(P['modules_critic'], t['observations'], t['actions'])
    critic_loss = ((q - y) ** 2).mean()
    info = {'critic/critic_loss': critic_loss.item(), 'critic/q_mean': q.mean().item(), 'critic/q_max': q.max().item(),
            'critic/q_min': q.min().item()}
    loss = critic_loss
    if full_update:
        a = mode(_actor(P['modules_actor'], t['observations']))
        qs = _critic(stored['modules_critic'], t['observations'], a)
        qm = torch.amin(qs, 0)   # (amin: an equal split of the gradient at ties, as jnp.min)
        mse = ((a - t['actions']) ** 2).sum(-1)
        lam = (1.0 / qm.abs().mean()).detach()
        actor_loss = -(lam * qm).mean()
        bc_loss = (config['alpha_actor'] * mse).mean()
        info.update({'actor/total_loss': (actor_loss + bc_loss).item(), 'actor/actor_loss': actor_loss.item(), 'actor/bc_loss': bc_loss.item(),
                     'actor/std': 1.0, 'actor/mse': mse.mean().item()})
        loss = loss + actor_loss + bc_loss
    loss.backward()
    grads = O.tree_map(lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy(), P)
    return loss.item(), info, grads
