"""fp64 numpy restatement of the reference's IQLAgent (agents/iql.py) with explicit noise: the CPU oracle of the IQL engine.

It reuses the MLP / LayerNorm / GELU helpers, Adam and Polyak of oracle/fql_oracle.py (OracleFQL.apply_gradients reads the PRE-step critic
for Polyak, agents/iql.py:136-156 is the same code as FQL's) with a hand-derived backward pass.  The Actor (utils/networks.py:82-150 with
state_dependent_std=False, no tanh) is actor_net (an MLP with activate_final) followed by mean_net: as one MLP, actor_net's Dense_0..n-1
plus mean_net as Dense_n.  With const_std=False the vector leaf modules_actor/log_stds [act] (zeros at init) is clipped to [-5, 2]; with
const_std=True there is no such leaf and the log-std is 0.  Noise of one update: eps [B, act] raw N(0, 1), read by the ddpgbc loss with
const_std=False only (agents/iql.py:89).

Gradients, as jax.grad gives them (u = (a - mean) / s, s = exp(clip(log_stds)), log_prob = sum_j(-u_j^2 / 2 - ls_j - log(2 pi) / 2)):
    d log_prob / d mean_j = u_j / s_j,    d log_prob / d ls_j = u_j^2 - 1
    awr:    w = min(exp(alpha adv), 100) is a constant (stored parameters only); dL/dmean = -(w / B) u / s, dL/dls = -(w / B)(u^2 - 1)
    ddpgbc: x = mean + s eps, q_actions = clip(x, -1, 1), g = clipmask(x) dL_q/dq_actions with dL_q/dq_e = -(1 / B) / mean|q| routed to
            the smaller member; dL/dmean = g - (alpha / B) u / s, dL/dls = g s eps - (alpha / B)(u^2 - 1)
    dL/dlog_stds = lsmask(raw) sum_b dL/dls
jnp.minimum and jnp.clip pass 1/2 of the gradient at an exact tie / bound.
"""
import copy
import math

import numpy as np

from oracle import fql_oracle as O

_HEAD = ('value/value_loss', 'value/v_mean', 'value/v_max', 'value/v_min',
         'critic/critic_loss', 'critic/q_mean', 'critic/q_max', 'critic/q_min')
_GRAD = ('grad/max', 'grad/min', 'grad/norm')
AWR_INFO_KEYS = _HEAD + ('actor/actor_loss', 'actor/adv', 'actor/bc_log_prob', 'actor/mse', 'actor/std') + _GRAD
DDPGBC_INFO_KEYS = _HEAD + ('actor/actor_loss', 'actor/q_loss', 'actor/bc_loss', 'actor/q_mean', 'actor/q_abs_mean',
                            'actor/bc_log_prob', 'actor/mse', 'actor/std') + _GRAD
INFO_KEYS = {'awr': AWR_INFO_KEYS, 'ddpgbc': DDPGBC_INFO_KEYS}
LOG_STD_MIN, LOG_STD_MAX = -5.0, 2.0


def get_config() -> dict:
    """agents/iql.py:242-261."""
    return dict(agent_name='iql', lr=3e-4, batch_size=256, actor_hidden_dims=(512, 512, 512, 512),
                value_hidden_dims=(512, 512, 512, 512), layer_norm=True, actor_layer_norm=False, discount=0.99, tau=0.005,
                expectile=0.9, actor_loss='ddpgbc', alpha=1.0, const_std=True, encoder=None)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/iql.py:200-237: Glorot-uniform kernels, mean_net variance_scaling(1e-2, fan_avg, uniform), zero biases, LN scale 1, zero
    log_stds (const_std=False only); value is a 1-member (unstacked) Value; target := critic."""
    rng = np.random.default_rng(seed)

    def mlp(in_dim, hidden, out_dim, ln, members=None, head=True):
        net, dims = {}, [in_dim] + list(hidden) + ([out_dim] if head else [])
        lead = () if members is None else (members,)
        for i in range(len(dims) - 1):
            net[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, dims[i], dims[i + 1], lead + (dims[i], dims[i + 1]), dtype),
                                 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
            if ln and (i < len(dims) - 2 or not head):
                net[f'LayerNorm_{i}'] = {'scale': np.ones(lead + (dims[i + 1],), dtype), 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
        return net

    vh, ah = tuple(config['value_hidden_dims']), tuple(config['actor_hidden_dims'])
    lim = math.sqrt(6.0 * 1e-2 / (ah[-1] + act_dim))
    actor = {'actor_net': mlp(obs_dim, ah, None, config['actor_layer_norm'], head=False),
             'mean_net': {'kernel': rng.uniform(-lim, lim, size=(ah[-1], act_dim)).astype(dtype), 'bias': np.zeros((act_dim,), dtype)}}
    if not config['const_std']:
        actor['log_stds'] = np.zeros((act_dim,), dtype)
    critic = {'value_net': mlp(obs_dim + act_dim, vh, 1, config['layer_norm'], 2)}
    return {'modules_actor': actor, 'modules_critic': critic, 'modules_target_critic': copy.deepcopy(critic),
            'modules_value': {'value_net': mlp(obs_dim, vh, 1, config['layer_norm'])}}


def merged(actor):
    """The Actor as one MLP: actor_net's layers, then mean_net as the last Dense."""
    net = dict(actor['actor_net'])
    net[f"Dense_{O._n_layers(actor['actor_net'])}"] = actor['mean_net']
    return net


def clip_mask(raw):
    """d clip(raw, -5, 2) / d raw as jnp.clip's max / min give it: 1 inside, 0 outside, 1/2 at a bound."""
    raw = np.asarray(raw)
    inside = (raw > LOG_STD_MIN) & (raw < LOG_STD_MAX)
    at = (raw == LOG_STD_MIN) | (raw == LOG_STD_MAX)
    return np.where(inside, 1.0, np.where(at, 0.5, 0.0)).astype(raw.dtype)


def unit_clip_mask(x):
    """d clip(x, -1, 1) / d x: 1 inside, 0 outside, 1/2 at |x| = 1."""
    ax = np.abs(x)
    return np.where(ax < 1.0, 1.0, np.where(ax == 1.0, 0.5, 0.0)).astype(x.dtype)


def expectile_weight(diff, expectile):
    """agents/iql.py:23-26: expectile where diff >= 0, else 1 - expectile."""
    return np.where(diff >= 0, expectile, 1 - expectile)


def awr_weight(adv, alpha):
    """agents/iql.py:66-67: min(exp(alpha adv), 100)."""
    with np.errstate(over='ignore'):   # (exp may overflow to inf: the cap takes it)
        return np.minimum(np.exp(adv * alpha), 100.0)


def gaussian_log_prob(a, mean, log_std):
    """MultivariateNormalDiag(mean, exp(log_std)).log_prob(a)."""
    u = (a - mean) / np.exp(log_std)
    return np.sum(-0.5 * u * u - log_std - 0.5 * math.log(2 * math.pi), axis=-1)


class OracleIQL(O.OracleFQL):
    """Restatement of IQLAgent (agents/iql.py:15-239) with explicit noise."""

    q_abs_override = None   # test hook: hold the normaliser mean|q| (a stop_gradient in the reference) fixed for finite differences

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _value(self, obs, keep=False, stored=False):
        r = O.mlp_forward(self._P(stored)['modules_value']['value_net'], self._c(obs), keep=keep)
        return (r[0][:, 0], r[1]) if keep else r[:, 0]

    def actor_mean(self, obs, keep=False, stored=False):
        return O.mlp_forward(merged(self._P(stored)['modules_actor']), self._c(obs), keep=keep)

    def raw_log_stds(self, stored=False):
        a = self._P(stored)['modules_actor']
        return a['log_stds'] if 'log_stds' in a else np.zeros((self.act_dim,), self.dtype)

    def _forward(self, batch, noise):
        """Every quantity of total_loss (and the caches of the differentiated passes)."""
        cfg = self.config
        dt = self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        nobs, rew, mask = self._c(batch['next_observations']), self._c(batch['rewards']), self._c(batch['masks'])
        B, A = act.shape
        f = {'B': B, 'A': A, 'act': act}
        # value loss (iql.py:28-40)
        tq = self._critic('modules_target_critic', obs, act, stored=True)
        f['v'], f['v_cache'] = self._value(obs, keep=True)
        f['vdiff'] = np.minimum(tq[0], tq[1]) - f['v']
        f['vw'] = expectile_weight(f['vdiff'], dt(cfg['expectile'])).astype(self.dtype)
        f['value_loss'] = np.mean(f['vw'] * f['vdiff'] ** 2)
        # critic loss (iql.py:42-55)
        f['y'] = rew + dt(cfg['discount']) * mask * self._value(nobs, stored=True)
        f['cq'], f['c_caches'] = self._critic('modules_critic', obs, act, keep=True)
        f['critic_loss'] = np.mean((f['cq'][0] - f['y']) ** 2 + (f['cq'][1] - f['y']) ** 2)
        # actor (iql.py:57-112)
        f['mean'], f['a_cache'] = self.actor_mean(obs, keep=True)
        f['raw'] = self.raw_log_stds()
        f['ls'] = np.clip(f['raw'], LOG_STD_MIN, LOG_STD_MAX)
        f['s'] = np.exp(f['ls'])
        f['u'] = (act - f['mean']) / f['s']
        f['lp'] = gaussian_log_prob(act, f['mean'], f['ls'])
        f['mse'] = np.mean((f['mean'] - act) ** 2)
        f['std'] = np.mean(f['s'])
        alpha = dt(cfg['alpha'])
        if cfg['actor_loss'] == 'awr':
            sq = self._critic('modules_critic', obs, act, stored=True)
            f['adv'] = np.minimum(sq[0], sq[1]) - self._value(obs, stored=True)
            f['w'] = awr_weight(f['adv'], alpha)
            f['actor_loss'] = -np.mean(f['w'] * f['lp'])
        elif cfg['actor_loss'] == 'ddpgbc':
            f['eps'] = np.zeros_like(act) if cfg['const_std'] else self._c(noise['eps'])
            f['x'] = f['mean'] if cfg['const_std'] else f['mean'] + f['s'] * f['eps']
            qa = np.clip(f['x'], -1, 1)
            f['qq'], f['q_caches'] = self._critic('modules_critic', obs, qa, keep=True, stored=True)
            q = np.minimum(f['qq'][0], f['qq'][1])
            f['q_mean'], f['q_abs_mean'] = q.mean(), np.abs(q).mean()
            f['q_loss'] = -f['q_mean'] / (f['q_abs_mean'] if self.q_abs_override is None else dt(self.q_abs_override))
            f['bc_loss'] = -np.mean(alpha * f['lp'])
            f['actor_loss'] = f['q_loss'] + f['bc_loss']
        else:
            raise ValueError(f"Unsupported actor loss: {cfg['actor_loss']}")
        return f

    def kink_margins(self, batch, noise, f=None):
        """Distance of every element from each point where the loss is not smooth (or its value branches): q - v = 0 (expectile weight),
        q1 = q2 of the ddpgbc critic pair, |x| = 1 of the clipped q_actions, alpha adv = log 100 (AWR's cap), log_stds at -5 / 2.  `f`: this
        state's _forward(batch, noise), where the caller has it already."""
        f = self._forward(batch, noise) if f is None else f
        m = {'expectile': float(np.abs(f['vdiff']).min())}
        if 'log_stds' in self.params['modules_actor']:
            m['log_stds'] = float(np.minimum(np.abs(f['raw'] - LOG_STD_MIN), np.abs(f['raw'] - LOG_STD_MAX)).min())
        if self.config['actor_loss'] == 'awr':
            m['exp_cap'] = float(np.abs(self.config['alpha'] * f['adv'] - math.log(100.0)).min())
        else:
            m['q_tie'] = float(np.abs(f['qq'][0] - f['qq'][1]).min())
            m['unit_clip'] = float(np.abs(np.abs(f['x']) - 1.0).min())
        return m

    def _losses(self, batch, noise, want_grads: bool, f=None):
        cfg = self.config
        dt = self.dtype.type
        f = self._forward(batch, noise) if f is None else f
        B, A, act = f['B'], f['A'], f['act']
        alpha = dt(cfg['alpha'])
        info = {'value/value_loss': f['value_loss'], 'value/v_mean': f['v'].mean(), 'value/v_max': f['v'].max(), 'value/v_min': f['v'].min(),
                'critic/critic_loss': f['critic_loss'], 'critic/q_mean': f['y'].mean(), 'critic/q_max': f['y'].max(),
                'critic/q_min': f['y'].min(), 'actor/actor_loss': f['actor_loss']}
        if cfg['actor_loss'] == 'awr':
            info.update({'actor/adv': f['adv'].mean(), 'actor/bc_log_prob': f['lp'].mean(), 'actor/mse': f['mse'], 'actor/std': f['std']})
        else:
            info.update({'actor/q_loss': f['q_loss'], 'actor/bc_loss': f['bc_loss'], 'actor/q_mean': f['q_mean'],
                         'actor/q_abs_mean': f['q_abs_mean'], 'actor/bc_log_prob': f['lp'].mean(), 'actor/mse': f['mse'],
                         'actor/std': f['std']})
        loss = f['value_loss'] + f['critic_loss'] + f['actor_loss']
        if not want_grads:
            return loss, info, None
        grads = O.tree_map(np.zeros_like, self.params)
        dv = (-2.0 / B) * f['vw'] * f['vdiff']
        _, grads['modules_value']['value_net'] = O.mlp_backward(self.params['modules_value']['value_net'], f['v_cache'],
                                                                dv[:, None].astype(self.dtype))
        gc = grads['modules_critic']['value_net']
        for e in range(2):
            dq = (2.0 / B) * (f['cq'][e] - f['y'])
            _, g = O.mlp_backward(self.params['modules_critic']['value_net'], f['c_caches'][e], dq[:, None].astype(self.dtype), member=e)
            for ln, sub in g.items():
                for k, val in sub.items():
                    gc[ln][k][e] = val
        u, s = f['u'], f['s']
        if cfg['actor_loss'] == 'awr':
            wb = (f['w'] / B)[:, None]
            dmean = -wb * u / s
            dls = -wb * (u * u - 1.0)
        else:
            qa_, qb_ = f['qq'][0], f['qq'][1]
            route = np.where(qa_ < qb_, 1.0, np.where(qa_ == qb_, 0.5, 0.0))
            gq = -(1.0 / B) / f['q_abs_mean']
            da = np.zeros_like(act)
            for e, r in enumerate((route, 1.0 - route)):
                dx, _ = O.mlp_backward(self._P(True)['modules_critic']['value_net'], f['q_caches'][e], (gq * r)[:, None].astype(self.dtype),
                                       member=e, want_param_grads=False)
                da += dx[:, self.obs_dim:]
            g = unit_clip_mask(f['x']) * da
            dmean = g - (alpha / B) * u / s
            dls = g * s * f['eps'] - (alpha / B) * (u * u - 1.0)
        _, ga = O.mlp_backward(merged(self.params['modules_actor']), f['a_cache'], dmean.astype(self.dtype))
        n = O._n_layers(self.params['modules_actor']['actor_net'])
        grads['modules_actor']['mean_net'] = ga.pop(f'Dense_{n}')
        grads['modules_actor']['actor_net'] = ga
        if 'log_stds' in self.params['modules_actor']:
            grads['modules_actor']['log_stds'] = (clip_mask(f['raw']) * dls.sum(axis=0)).astype(self.dtype)
        return loss, info, grads

    def update(self, batch, noise=None):
        """agents/iql.py:145-156 (+ utils/flax_utils.py:120-159)."""
        loss, info, grads = self._losses(batch, noise, want_grads=True)
        info.update(self.grad_stats(grads))
        self.apply_gradients(grads)
        return loss, {k: float(info[k]) for k in INFO_KEYS[self.config['actor_loss']]}

    def sample_actions(self, observations, noises, temperature=1.0):
        """agents/iql.py:158-169 with the normal draw passed in."""
        mean = self.actor_mean(observations, stored=True)
        s = np.exp(np.clip(self.raw_log_stds(stored=True), LOG_STD_MIN, LOG_STD_MAX)) * self.dtype.type(temperature)
        return np.clip(mean + s * self._c(noises), -1, 1)


def make_noise(batch_size, act_dim, seed):
    return {'eps': np.random.default_rng(seed).standard_normal((batch_size, act_dim)).astype(np.float32)}


def clear_of_unit_clip(ref, batch, noise, margin):
    """A copy of `noise` whose ddpgbc q_actions x = mean + exp(ls) eps keep 2 * margin from the |x| = 1 kink under `ref`'s current
    parameters.  At B x act in the thousands no seed clears that kink by itself, so each element with ||x| - 1| < 2 * margin gets the
    eps that puts it at |x| = 1 -/+ 2 * margin on the side it was on, rounded to float32 as the engine receives it (the rounding moves
    x by about 1e-7 |x - mean|, far inside the second margin).  The mean does not depend on eps, so the move is exact and touches no
    other element.  Two conditions keep this an ordinary random problem: at most 1 % of the elements move, and between 20 % and 80 %
    of them end up clipped, so both branches of the clip mask stay live."""
    mean = ref.actor_mean(batch['observations'])
    s = np.exp(np.clip(ref.raw_log_stds(), LOG_STD_MIN, LOG_STD_MAX))
    eps = np.asarray(noise['eps'], np.float32)
    x = mean + s * eps.astype(np.float64)
    near = np.abs(np.abs(x) - 1.0) < 2 * margin
    target = np.sign(x) * (1.0 + np.where(np.abs(x) < 1.0, -2.0, 2.0) * margin)
    out = np.where(near, ((target - mean) / s).astype(np.float32), eps)
    x = mean + s * out.astype(np.float64)
    clipped = float(np.mean(np.abs(x) > 1.0))
    assert near.mean() <= 0.01, f'{int(near.sum())} of {near.size} elements moved'
    assert 0.2 <= clipped <= 0.8, f'{clipped:.3f} of the q_actions clipped'
    assert np.abs(np.abs(x) - 1.0).min() >= margin
    return dict(noise, eps=out)


def randomize(params, seed, scale=0.3, log_stds=(-1.5, 1.0)):
    """Parameters moved away from init (a fixture and test helper): every leaf gets uniform noise, the mean head a bias spread so that
    some q_actions leave [-1, 1], log_stds a spread inside (-5, 2), and the target critic differs from the critic."""
    rng = np.random.default_rng(seed)
    p = O.tree_map(lambda a: (a + rng.uniform(-scale, scale, size=np.shape(a)) * (np.abs(a).max() if np.size(a) > 1 and
                                                                                   np.abs(a).max() > 0 else scale)).astype(a.dtype),
                   params)
    mn = p['modules_actor']['mean_net']
    mn['bias'] = (mn['bias'] + rng.uniform(-1.5, 1.5, size=mn['bias'].shape)).astype(mn['bias'].dtype)
    if 'log_stds' in p['modules_actor']:
        ls = p['modules_actor']['log_stds']
        p['modules_actor']['log_stds'] = rng.uniform(*log_stds, size=ls.shape).astype(ls.dtype)
    p['modules_target_critic'] = O.tree_map(lambda a: (a + rng.uniform(-0.05, 0.05, size=np.shape(a))).astype(a.dtype),
                                            p['modules_critic'])
    return p
