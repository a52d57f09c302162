"""fp64 numpy restatement of the reference's IQLDiffusionAgent (agents/iql_diffusion.py), binary optimality family, with explicit noise
and a hand-derived backward: the CPU oracle of the IQL-diffusion engine.

Four bare TrainStates: critic (2 members), target_critic, value (1 member), actor.  The actor is DiffusionPolicy: Dense_0(MLP_0([obs |
x_t | emb(t) | Embed_0[is_positive]])), MLP_0 = Dense -> GELU(tanh) -> LayerNorm per hidden layer; emb is the pinned 16-wide timestep
embedding shared with BC (fql_amd/bc.py::timestep_embedding).  Noise of one update: {'x0': [B, act], 't': [B] on the grid k / S}.

Losses (line numbers of agents/iql_diffusion.py):
    critic (:94-103)  y = r + discount mask v(next_obs) (stored value); loss = mean over BOTH members and the batch of (q_e - y)^2;
                      dL/dq_e = (q_e - y) / B;  info q = mean of member 0
    value  (:105-116) d = min(target q1, q2) - v; loss = mean(where(d > 0, expectile, 1 - expectile) d^2); dL/dv = -2 w d / B
    actor  (:118-213) adv = min(q1, q2)(obs, act) - v(obs) on stored parameters (target pair with target_extraction, else the critic);
                      w = loss_weight(adv), a constant; lp_b = mean_a((vel - v_pos)^2) w_b, lu_b = mean_a((vel - v_unc)^2);
                      loss = mean_b(lp + 0.1 lu).  As ONE pass over 2B rows (rows [0, B): Embed[1], rows [B, 2B): Embed[0]) the seed is
                      -2 w_b (vel - pred) / (B act) in the first half and -0.2 (vel - pred) / (B act) in the second, and dEmbed[r] is the
                      column sum over that half of the input gradient's last 32 columns.
Each TrainState has its own Adam (three learning rates) and count; Polyak reads the PRE-step critic; update(batch, update_critic,
update_actor) as the reference's static flags (:215-247).
"""
import copy
import math

import numpy as np

from oracle import fql_oracle as O
from fql_amd.bc import timestep_embedding, grid_index
from fql_amd.iql_diffusion import info_keys, IQLD_ROW_KEYS
from tests.bc_oracle import lecun_normal, _as_net, _from_net_grads

EMBED = 32
LOG100 = math.log(100.0)
TRAINED = ('actor', 'critic', 'value')
LR_KEY = {'actor': 'actor_lr', 'critic': 'critic_lr', 'value': 'value_lr'}


def get_config() -> dict:
    """agents/iql_diffusion.py:362-396 (the keys the losses read)."""
    return dict(agent_name='iql_diffusion', batch_size=256, actor_lr=3e-4, value_lr=3e-4, critic_lr=3e-4, num_qs=2,
                actor_hidden_dims=(512, 512, 512, 512), hidden_dims=(512, 512, 512, 512), discount=0.99, expectile=0.9, use_layer_norm=1,
                activation='gelu', tau=0.005, opt_decay_schedule='none', target_extraction=1, denoise_steps=16,
                optimal_var='binary_awr_loss', awr_temperature=0.1, softmax_beta=3.0)


def init_params(seed, obs_dim, act_dim, config, dtype=np.float32):
    """agents/iql_diffusion.py:303-357: MLP kernels default_init (Glorot uniform), zero biases, LayerNorm (1, 0); the actor's head
    lecun_normal; Embed_0 N(0, 1 / 32) (flax's variance_scaling(1, fan_in, normal, out_axis=0): fan_in of [2, 32] is 32); target := critic."""
    rng = np.random.default_rng(seed)
    ln = bool(config['use_layer_norm'])

    def mlp(in_dim, hidden, out_dim, members=None):
        net, dims = {}, [in_dim] + list(hidden) + ([out_dim] if out_dim else [])
        lead = () if members is None else (members,)
        for i in range(len(dims) - 1):
            net[f'Dense_{i}'] = {'kernel': O.glorot_uniform(rng, dims[i], dims[i + 1], lead + (dims[i], dims[i + 1]), dtype),
                                 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
            if ln and (i < len(dims) - 2 or not out_dim):
                net[f'LayerNorm_{i}'] = {'scale': np.ones(lead + (dims[i + 1],), dtype), 'bias': np.zeros(lead + (dims[i + 1],), dtype)}
        return net

    ah, vh = tuple(config['actor_hidden_dims']), tuple(config['hidden_dims'])
    actor = {'MLP_0': mlp(obs_dim + act_dim + 16 + EMBED, ah, None),
             'Dense_0': {'kernel': lecun_normal(rng, ah[-1], (ah[-1], act_dim), dtype), 'bias': np.zeros(act_dim, dtype)},
             'Embed_0': {'embedding': (rng.standard_normal((2, EMBED)) / math.sqrt(EMBED)).astype(dtype)}}
    critic = {'value_net': mlp(obs_dim + act_dim, vh, 1, 2)}
    return {'actor': actor, 'critic': critic, 'target_critic': copy.deepcopy(critic), 'value': {'value_net': mlp(obs_dim, vh, 1)}}


def loss_weight(adv, config):
    """agents/iql_diffusion.py:155-167."""
    ov = config['optimal_var']
    pos = adv > 0
    if ov == 'binary':
        return pos.astype(adv.dtype)
    temp = config['awr_temperature'] if ov == 'binary_awr_loss' else config['softmax_beta']
    with np.errstate(over='ignore'):
        e = np.where(pos, np.clip(np.exp(adv * adv.dtype.type(temp)), 0, 1e8), 0).astype(adv.dtype)
    if ov == 'binary_awr_loss':
        return np.minimum(e, adv.dtype.type(100.0))
    if ov == 'binary_softmax_loss':
        return e / (np.sum(e, axis=0) + adv.dtype.type(1e-8))
    raise ValueError(f'Invalid optimal_var: {ov}')


def top_mass(w):
    """agents/iql_diffusion.py:193-195, by np.sort: sorted[-int(0.1 n):].sum() / (sum + 1e-8) (int(0.1 n) == 0 takes every element)."""
    s = np.sort(w)
    return s[-int(0.1 * len(s)):].sum() / (s.sum() + w.dtype.type(1e-8))


def top_mass_by_rank(w):
    """The engine's selection restated: rank(b) = #{j : w_j > w_b or (w_j == w_b and j < b)}; rows with rank < int(0.1 n) are summed in
    index order (all rows when that count is 0)."""
    n = len(w)
    k = int(0.1 * n)
    idx = np.arange(n)
    rank = ((w[None, :] > w[:, None]) | ((w[None, :] == w[:, None]) & (idx[None, :] < idx[:, None]))).sum(axis=1)
    take = np.ones(n, bool) if k == 0 else rank < k
    assert k == 0 or take.sum() == k
    return w[take].sum() / (w.sum() + w.dtype.type(1e-8))


class OracleIQLD:
    def __init__(self, params, config, obs_dim, act_dim, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.params = O.tree_map(lambda a: np.array(a, dtype=self.dtype), params)
        self.config = dict(config)
        self.S = int(self.config['denoise_steps'])
        self.od, self.ad = obs_dim, act_dim
        self.mu = O.tree_map(np.zeros_like, self.params)
        self.nu = O.tree_map(np.zeros_like, self.params)
        self.counts = {'actor': 0, 'critic': 0}   # the value net steps with the critic
        self.updates = 0
        self.frozen = None   # test hook (finite differences): the tree every stored-parameter use reads, as in OracleFQL

    @classmethod
    def create(cls, seed, obs_dim, act_dim, config, dtype=np.float32):
        return cls(init_params(seed, obs_dim, act_dim, config, dtype), config, obs_dim, act_dim, dtype)

    def _c(self, x):
        return np.asarray(x, dtype=self.dtype)

    def _P(self, stored=False):
        return self.frozen if (stored and self.frozen is not None) else self.params

    # -- networks -------------------------------------------------------------------------------
    def _value(self, obs, keep=False, stored=False):
        r = O.mlp_forward(self._P(stored)['value']['value_net'], self._c(obs), keep=keep)
        return (r[0][:, 0], r[1]) if keep else r[:, 0]

    def _critic(self, name, obs, act, keep=False, stored=False):
        x = np.concatenate([self._c(obs), self._c(act)], axis=-1)
        net = self._P(stored)[name]['value_net']
        outs, caches = [], []
        for e in range(2):
            r = O.mlp_forward(net, x, member=e, keep=keep)
            outs.append(r[0][:, 0] if keep else r[:, 0])
            if keep:
                caches.append(r[1])
        q = np.stack(outs, axis=0)
        return (q, caches) if keep else q

    def policy(self, obs, is_positive, x, k, keep=False, stored=False):
        """DiffusionPolicy(obs, is_positive, x, t = k / S) (:54-67)."""
        p = self._P(stored)['actor']
        n = obs.shape[0]
        emb = self._c(timestep_embedding(np.broadcast_to(np.asarray(k), (n,)), self.S))
        row = p['Embed_0']['embedding'][np.broadcast_to(np.asarray(is_positive), (n,))]
        net, _ = _as_net(p)
        return O.mlp_forward(net, np.concatenate([self._c(obs), self._c(x), emb, row], axis=-1), keep=keep)

    # -- losses ---------------------------------------------------------------------------------
    def adv(self, batch):
        """adv = min(q1, q2)(obs, actions) - v(obs) and that min, on stored parameters (:131-137)."""
        name = 'target_critic' if self.config['target_extraction'] else 'critic'
        q = np.min(self._critic(name, batch['observations'], batch['actions'], stored=True), axis=0)
        return q - self._value(batch['observations'], stored=True), q

    def kink_margins(self, batch, noise=None):
        """Distance of every row from the points where the losses branch: adv = 0 (the weights are DISCONTINUOUS there in all three
        variants), adv awr_temperature = ln 100 (binary_awr_loss's cap), and q - v = 0 of the expectile weight."""
        adv, _ = self.adv(batch)
        tq = self._critic('target_critic', batch['observations'], batch['actions'], stored=True)
        m = {'adv': float(np.abs(adv).min()), 'expectile': float(np.abs(np.min(tq, axis=0) - self._value(batch['observations'])).min()),
             'positive': int((adv > 0).sum()), 'negative': int((adv <= 0).sum())}
        if self.config['optimal_var'] == 'binary_awr_loss':
            z = adv * self.config['awr_temperature']
            m['exp_cap'] = float(np.abs(z - LOG100).min())
            m['capped'] = int((z > LOG100).sum())
        return m

    def critic_part(self, batch, want_grads):
        cfg, dt = self.config, self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        B = act.shape[0]
        y = self._c(batch['rewards']) + dt(cfg['discount']) * self._c(batch['masks']) * self._value(batch['next_observations'], stored=True)
        q, caches = self._critic('critic', obs, act, keep=True)
        loss = np.mean((q - y[None]) ** 2)
        info = {'critic_loss': loss, 'q': q[0].mean()}
        if not want_grads:
            return loss, info, None
        g = O.tree_map(np.zeros_like, self.params['critic'])
        for e in range(2):
            dq = (q[e] - y) / B
            _, ge = O.mlp_backward(self.params['critic']['value_net'], caches[e], dq[:, None].astype(self.dtype), member=e)
            for ln, sub in ge.items():
                for k, val in sub.items():
                    g['value_net'][ln][k][e] = val
        return loss, info, g

    def value_part(self, batch, want_grads):
        cfg, dt = self.config, self.dtype.type
        obs, act = self._c(batch['observations']), self._c(batch['actions'])
        B = act.shape[0]
        tq = np.min(self._critic('target_critic', obs, act, stored=True), axis=0)
        v, cache = self._value(obs, keep=True)
        d = tq - v
        w = np.where(d > 0, dt(cfg['expectile']), dt(1 - cfg['expectile']))
        loss = np.mean(w * d ** 2)
        info = {'value_loss': loss, 'v': v.mean(), 'v_min': v.min(), 'v_max': v.max()}
        if not want_grads:
            return loss, info, None
        dv = (-2.0 / B) * w * d
        _, g = O.mlp_backward(self.params['value']['value_net'], cache, dv[:, None].astype(self.dtype))
        return loss, info, {'value_net': g}

    def _flow_inputs(self, batch, noise):
        a, x0 = self._c(batch['actions']), self._c(noise['x0'])
        k = grid_index(noise['t'], self.S)
        t = self._c(k.astype(np.float32) / np.float32(self.S))[:, None]
        return a, k, x0 * (1 - t) + a * t, a - x0

    def actor_part(self, batch, noise, want_grads):
        """The stacked form: ONE policy pass over 2B rows."""
        cfg = self.config
        obs = self._c(batch['observations'])
        a, k, x_t, vel = self._flow_inputs(batch, noise)
        B, A = a.shape
        adv, q = self.adv(batch)
        w = loss_weight(adv, cfg)
        rows = np.concatenate([np.ones(B, np.int64), np.zeros(B, np.int64)])
        out = self.policy(np.concatenate([obs, obs]), rows, np.concatenate([x_t, x_t]), np.concatenate([k, k]), keep=want_grads)
        pred, cache = out if want_grads else (out, None)
        dpos, dunc = vel - pred[:B], vel - pred[B:]
        lp = np.mean(dpos ** 2, axis=-1) * w
        lu = np.mean(dunc ** 2, axis=-1)
        losses = lp + lu * 0.1
        loss = np.mean(losses)
        o = np.ones(B, self.dtype)
        info = {'actor_q': q.mean(), 'actor_loss': loss, 'actor_positive_ratio': (adv > 0).mean(), 'actor_loss_positive': lp.mean(),
                'actor_loss_uncond': lu.mean(), 'actor_losses': losses, 'o_mean': o.mean(), 'o_std': o.std(), 'o_min': o.min(),
                'o_max': o.max(), 'o': o, 'effective_batch_size': np.sum(w) ** 2 / (np.sum(w ** 2) + 1e-8),
                'loss_weights_top_10_mass': top_mass(w), 'loss_weights_max': np.max(w), 'loss_weights': w}
        if not want_grads:
            return loss, info, None
        seed = np.concatenate([-2.0 * w[:, None] * dpos, -0.2 * dunc]) / (B * A)
        net, n = _as_net(self.params['actor'])
        dx, g = O.mlp_backward(net, cache, seed.astype(self.dtype))
        grads = _from_net_grads(g, n)
        grads['Embed_0'] = {'embedding': np.stack([dx[B:, -EMBED:].sum(axis=0), dx[:B, -EMBED:].sum(axis=0)])}
        return loss, info, grads

    def actor_loss_two_passes(self, batch, noise):
        """The reference's form (:180-189): a positive and an unconditional pass of B rows each.  (loss, per-row losses)."""
        obs = self._c(batch['observations'])
        a, k, x_t, vel = self._flow_inputs(batch, noise)
        w = loss_weight(self.adv(batch)[0], self.config)
        vp = self.policy(obs, 1, x_t, k)
        vu = self.policy(obs, 0, x_t, k)
        losses = np.mean((vel - vp) ** 2, axis=-1) * w + np.mean((vel - vu) ** 2, axis=-1) * 0.1
        return np.mean(losses), losses

    def total_loss(self, batch, noise):
        """:272-285: critic + value + actor loss; every info but grad/*, in the merge order."""
        lc, ic, _ = self.critic_part(batch, False)
        lv, iv, _ = self.value_part(batch, False)
        la, ia, _ = self.actor_part(batch, noise, False)
        info = {**ic, **iv, **ia}
        return lc + lv + la, {k: info[k] for k in info_keys(True, True, grads=False)}

    def grads(self, batch, noise, update_critic=True, update_actor=True):
        """{net: gradient tree} of the nets this step kind differentiates, and the merged infos (grad/* as the merge leaves them)."""
        info, g = {}, {}
        if update_critic:
            _, ic, g['critic'] = self.critic_part(batch, True)
            ic.update(O.OracleFQL.grad_stats(g['critic']))
            _, iv, g['value'] = self.value_part(batch, True)
            iv.update(O.OracleFQL.grad_stats(g['value']))
            info = {**ic, **iv}
        if update_actor:
            _, ia, g['actor'] = self.actor_part(batch, noise, True)
            ia.update(O.OracleFQL.grad_stats(g['actor']))
            info = {**info, **ia}
        return g, info

    def apply_gradients(self, net, grads):
        """optax.adam(<net>_lr) on one TrainState with its own count."""
        dt = self.dtype.type
        b1, b2, eps, lr = dt(0.9), dt(0.999), dt(1e-8), dt(self.config[LR_KEY[net]])
        c = self.counts['actor' if net == 'actor' else 'critic'] + 1
        c1, c2 = dt(1.0 - 0.9 ** c), dt(1.0 - 0.999 ** c)

        def upd(p, g, m, v):
            m[...] = b1 * m + (dt(1) - b1) * g
            v[...] = b2 * v + (dt(1) - b2) * g * g
            return p - lr * (m / c1) / (np.sqrt(v / c2) + eps)

        self.params[net] = O.tree_map(upd, self.params[net], grads, self.mu[net], self.nu[net])

    def update(self, batch, noise, update_critic=True, update_actor=True):
        """:215-247.  Returns the info dict of this step kind (info_keys order); per-row arrays stay arrays."""
        g, info = self.grads(batch, noise, update_critic, update_actor)
        if update_critic:
            old_critic, old_target = copy.deepcopy(self.params['critic']), self.params['target_critic']
            self.apply_gradients('critic', g['critic'])
            tau = self.dtype.type(self.config['tau'])
            self.params['target_critic'] = O.tree_map(lambda p, tp: p * tau + tp * (self.dtype.type(1) - tau), old_critic, old_target)
            self.apply_gradients('value', g['value'])
            self.counts['critic'] += 1
        if update_actor:
            self.apply_gradients('actor', g['actor'])
            self.counts['actor'] += 1
        self.updates += 1
        return {k: (info[k] if k in IQLD_ROW_KEYS else float(info[k])) for k in info_keys(update_critic, update_actor)}

    def sample_actions(self, observations, noises, cfg=1.0):
        """:249-270 with explicit x ~ N(0, I): S Euler steps of v = v_unc + cfg (v_pos - v_unc), the squeeze, then the clip."""
        obs = self._c(observations)
        obs = obs[None] if obs.ndim == 1 else obs
        x = self._c(noises).reshape(obs.shape[0], self.ad).copy()
        dt, c = self.dtype.type(1.0 / self.S), self.dtype.type(cfg)
        for i in range(self.S):
            vp = self.policy(obs, 1, x, i, stored=True)
            vu = self.policy(obs, 0, x, i, stored=True)
            x = x + (vu + c * (vp - vu)) * dt
        x = x[0] if obs.shape[0] == 1 else x
        return np.clip(x, -1, 1)


def make_noise(batch_size, act_dim, denoise_steps, seed):
    """x0 ~ N(0, I) and t = k / S with k ~ randint[0, S]; rows 0 and 1 hold k = 0 and k = S."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, denoise_steps + 1, size=batch_size)
    if batch_size >= 2:
        k[0], k[1] = 0, denoise_steps
    return {'x0': rng.standard_normal((batch_size, act_dim)).astype(np.float32),
            't': (k.astype(np.float32) / np.float32(denoise_steps)).astype(np.float32)}


def make_batch(obs_dim, act_dim, batch_size, seed):
    ds = O.make_synthetic_dataset(max(4 * batch_size, 64), obs_dim, act_dim, seed=seed)
    idx = np.random.default_rng(seed + 1).integers(0, len(ds['observations']), size=batch_size)
    return O.sample_batch(ds, idx)


def randomize(params, seed, scale=0.1, q_spread=1.0):
    """Parameters away from init (a fixture): biases and LayerNorm parameters get noise so every leaf matters, the target differs from
    the critic, and the value head's bias is set so that adv = min q - v straddles 0 on a random batch (q_spread widens the critic's
    output through its head kernel, which spreads adv)."""
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, np.float64), params)
    for p, v in O.tree_leaves_with_path(out):
        if not p.endswith('/kernel') and not p.endswith('/embedding'):
            v += scale * rng.standard_normal(v.shape)
    out['target_critic'] = O.tree_map(lambda a: a + 0.01 * rng.standard_normal(a.shape), out['critic'])
    for name in ('critic', 'target_critic'):
        head = out[name]['value_net'][f"Dense_{O._n_layers(out[name]['value_net']) - 1}"]
        head['kernel'] *= q_spread
    return O.tree_map(lambda a: a.astype(np.float32), out)


def center_value(ref, batch, quantile=0.5):
    """Shift the value head's bias so that `quantile` of the batch has adv <= 0 under ref's parameters: rows on both sides of adv = 0."""
    adv, _ = ref.adv(batch)
    net = ref.params['value']['value_net']
    head = net[f'Dense_{O._n_layers(net) - 1}']
    head['bias'] = head['bias'] + np.quantile(adv, quantile)
    return ref


def sync(ref, agent):
    """Continue the restatement from the engine's state: parameters, moments and the per-TrainState counters (tests/util.py::
    sync_restatement for this agent)."""
    cast = lambda t: O.tree_map(lambda a: np.array(a, dtype=ref.dtype), t)   # noqa: E731
    opt = agent.get_opt_state()
    ref.params, ref.mu, ref.nu = cast(agent.get_params()), cast(opt['mu']), cast(opt['nu'])
    ref.counts = {'critic': opt['count'], 'actor': opt['actor_count']}
    ref.updates = opt['updates']


__all__ = ['OracleIQLD', 'get_config', 'init_params', 'loss_weight', 'top_mass', 'top_mass_by_rank', 'make_noise', 'make_batch', 'randomize',
           'center_value', 'sync']
