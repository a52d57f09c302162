"""torch-autograd restatement of IQLAgent.total_loss (agents/iql.py), fp64 on the CPU, composed as the reference composes it - an
independent check of the hand-derived backward pass in tests/iql_oracle.py.  The target critic, value(next_obs), the AWR weight's critic
and value, the ddpgbc loss's critic and its normaliser mean|q| are constants, as in the reference."""
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


def _dist(actor, obs):
    """utils/networks.py Actor with state_dependent_std=False: (mean, scale_diag [act])."""
    h = _mlp(actor['actor_net'], obs, activate_final=True)
    mean = h @ actor['mean_net']['kernel'] + actor['mean_net']['bias']
    log_stds = actor['log_stds'] if 'log_stds' in actor else torch.zeros(mean.shape[-1], dtype=mean.dtype)
    return mean, torch.exp(torch.clamp(log_stds, -5.0, 2.0))


def _log_prob(a, mean, scale):
    z = (a - mean) / scale
    return (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2 * math.pi)).sum(-1)


def _critic(critic, obs, act):
    x = torch.cat([obs, act], -1)
    return torch.stack([_mlp(critic['value_net'], x, e)[:, 0] for e in range(2)])


def _value(value, obs):
    return _mlp(value['value_net'], obs)[:, 0]


def losses(params, config, batch, noise):
    """(loss, info, grads) with grads over the whole tree (zeros for the target critic), all fp64 numpy."""
    P = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True), params)
    S = O.tree_map(lambda a: torch.tensor(np.asarray(a, np.float64)), params)
    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in batch.items()}
    obs, act = t['observations'], t['actions']
    with torch.no_grad():
        tq = _critic(S['modules_target_critic'], obs, act)
        q = torch.minimum(tq[0], tq[1])
        y = t['rewards'] + config['discount'] * t['masks'] * _value(S['modules_value'], t['next_observations'])
    v = _value(P['modules_value'], obs)
    diff = q - v
    w = torch.where(diff >= 0, torch.tensor(float(config['expectile']), dtype=torch.float64),
                    torch.tensor(1.0 - float(config['expectile']), dtype=torch.float64))
    value_loss = (w * diff ** 2).mean()
    cq = _critic(P['modules_critic'], obs, act)
    critic_loss = ((cq[0] - y) ** 2 + (cq[1] - y) ** 2).mean()
    info = {'value/value_loss': value_loss.item(), 'value/v_mean': v.mean().item(), 'value/v_max': v.max().item(),
            'value/v_min': v.min().item(), 'critic/critic_loss': critic_loss.item(), 'critic/q_mean': y.mean().item(),
            'critic/q_max': y.max().item(), 'critic/q_min': y.min().item()}
    mean, scale = _dist(P['modules_actor'], obs)
    lp = _log_prob(act, mean, scale)
    tail = {'actor/bc_log_prob': lp.mean().item(), 'actor/mse': ((mean - act) ** 2).mean().item(), 'actor/std': scale.mean().item()}
    if config['actor_loss'] == 'awr':
        with torch.no_grad():
            sq = _critic(S['modules_critic'], obs, act)
            adv = torch.minimum(sq[0], sq[1]) - _value(S['modules_value'], obs)
            ea = torch.clamp(torch.exp(adv * config['alpha']), max=100.0)
        actor_loss = -(ea * lp).mean()
        info.update({'actor/actor_loss': actor_loss.item(), 'actor/adv': adv.mean().item()})
    else:
        x = mean if config['const_std'] else mean + scale * torch.tensor(np.asarray(noise['eps'], np.float64))
        qq = _critic(S['modules_critic'], obs, torch.clamp(x, -1.0, 1.0))
        qm = torch.minimum(qq[0], qq[1])
        q_loss = -qm.mean() / qm.abs().mean().detach()
        bc_loss = -(config['alpha'] * lp).mean()
        actor_loss = q_loss + bc_loss
        info.update({'actor/actor_loss': actor_loss.item(), 'actor/q_loss': q_loss.item(), 'actor/bc_loss': bc_loss.item(),
                     'actor/q_mean': qm.mean().item(), 'actor/q_abs_mean': qm.abs().mean().item()})
    info.update(tail)
    loss = value_loss + critic_loss + actor_loss
    loss.backward()
    grads = O.tree_map(lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy(), P)
    return loss.item(), info, grads
