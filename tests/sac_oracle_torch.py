"""torch-autograd restatement of SACAgent.total_loss (agents/sac.py), fp64 on the CPU, composed as the reference composes it: the actor's
sample x = mean + exp(clip(ls)) eps, the base Normal's log-prob of that sample, then the tanh log-det-Jacobian (distrax Tanh) - an
independent check of the hand-derived backward pass in tests/sac_oracle.py.  The stored critic of the actor loss, the stored alpha of the
actor loss and critic target, and the target critic are constants, as in the reference."""
import math

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


def _mlp(net, x, member=None, activate_final=False):
    leaf = (lambda a: a) if member is None else (lambda a: a[member])
    n = sum(1 for k in net if k.startswith('Dense_'))
    for i in range(n):
        x = x @ leaf(net[f'Dense_{i}']['kernel']) + leaf(net[f'Dense_{i}']['bias'])
        if i + 1 < n or activate_final:
            x = _gelu(x)
            if f'LayerNorm_{i}' in net:
                x = _ln(x, leaf(net[f'LayerNorm_{i}']['scale']), leaf(net[f'LayerNorm_{i}']['bias']))
    return x


def _dist_sample(actor, obs, eps, tanh_squash, temperature=1.0):
    """utils/networks.py Actor + distrax sample_and_log_prob: (action, log_prob, scale)."""
    h = _mlp(actor['actor_net'], obs, activate_final=True)
    mean = h @ actor['mean_net']['kernel'] + actor['mean_net']['bias']
    log_std = torch.clamp(h @ actor['log_std_net']['kernel'] + actor['log_std_net']['bias'], -5.0, 2.0)
    scale = torch.exp(log_std) * temperature
    x = mean + scale * eps
    z = (x - mean) / scale   # MultivariateNormalDiag.log_prob(x)
    lp = (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2 * math.pi)).sum(-1)
    if not tanh_squash:
        return x, lp, scale
    # distrax Tanh forward_log_det_jacobian: 2 (log 2 - x - softplus(-2 x)), summed by Block(ndims=1)
    lp = lp - (2.0 * (math.log(2.0) - x - torch.nn.functional.softplus(-2.0 * x))).sum(-1)
    return torch.tanh(x), lp, scale


def _critic(critic, obs, act):
    x = torch.cat([obs, act], -1)
    return torch.stack([_mlp(critic['value_net'], x, e)[:, 0] for e in range(2)])


def losses(params, config, batch, noise, act_dim):
    """(loss, info, grads) with grads over the whole tree (zeros for the target critic), all fp64 numpy."""
    P = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True), params)
    stored = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64)), params)
    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in batch.items()}
    e_n = torch.tensor(np.asarray(noise['eps1'], np.float64))
    e_c = torch.tensor(np.asarray(noise['eps2'], np.float64))
    te = config.get('target_entropy')
    te = -config['target_entropy_multiplier'] * act_dim if te is None else te
    alpha_c = torch.exp(stored['modules_alpha']['log_value'])
    with torch.no_grad():
        a_n, lp_n, _ = _dist_sample(stored['modules_actor'], t['next_observations'], e_n, config['tanh_squash'])
        tq = _critic(stored['modules_target_critic'], t['next_observations'], a_n)
        next_q = tq.min(0).values if config['q_agg'] == 'min' else tq.mean(0)
        y = t['rewards'] + config['discount'] * t['masks'] * next_q
        if config['backup_entropy']:
            y = y - config['discount'] * t['masks'] * lp_n * alpha_c
    q = _critic(P['modules_critic'], t['observations'], t['actions'])
    critic_loss = ((q - y) ** 2).mean()
    a, lp, scale = _dist_sample(P['modules_actor'], t['observations'], e_c, config['tanh_squash'])
    qbar = _critic(stored['modules_critic'], t['observations'], a).mean(0)
    actor_loss = (lp * alpha_c - qbar).mean()
    alpha = torch.exp(P['modules_alpha']['log_value'])
    entropy = -lp.detach().mean()
    alpha_loss = alpha * (entropy - te)
    loss = critic_loss + actor_loss + alpha_loss
    info = {'critic/critic_loss': critic_loss.item(), 'critic/q_mean': q.mean().item(), 'critic/q_max': q.max().item(),
            'critic/q_min': q.min().item(), 'actor/total_loss': (actor_loss + alpha_loss).item(), 'actor/actor_loss': actor_loss.item(),
            'actor/alpha_loss': alpha_loss.item(), 'actor/alpha': alpha.item(), 'actor/entropy': -lp.mean().item(),
            'actor/std': scale.mean().item(), 'actor/q': qbar.mean().item()}
    loss.backward()
    grads = O.tree_map(lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy(), P)
    return loss.item(), info, grads
