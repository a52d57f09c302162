"""The problems the IQL-diffusion GPU tests run, built on the CPU: configuration, parameters (set into the engine with set_params), batch
and noise per case, from seeds chosen so that every row keeps its distance from the points where the loss weights branch.

The weights are DISCONTINUOUS at adv = 0 in all three optimal_var variants and kinked at adv awr_temperature = ln 100: one row on the
other side in fp32 moves the actor loss by O(1 / B), which no tolerance may absorb.  So a case is admitted only if, on the fp64 values,
|adv| >= MARGIN and |adv awr_temperature - ln 100| >= MARGIN for every row, rows lie on both sides of adv = 0, and (binary_awr_loss) at
least one row sits at the 100 cap.  tests/test_iqld_cpu.py checks this for every case without a GPU; the GPU tests assert it again on the
values they compare.  awr_temperature is set per case from the batch's advantages (LOG100 over their `cap_q` quantile among the positive
rows, 85 % unless the case says otherwise, rounded to 3 digits) so that some rows reach the cap.
"""
import numpy as np

from tests import iqld_oracle as DO

MARGIN = 1e-3
OD, AD = 29, 8


def case(od=OD, ad=AD, H=64, nh=4, B=64, S=16, ov='binary_awr_loss', te=1, ln=1, seed=0, actor_hidden=None, cap_q=0.85, hidden=None):
    """hidden: the critic's and the value net's widths (default (H,) * nh); actor_hidden: the actor's (default: the same)."""
    c = dict(od=od, ad=ad, H=H, nh=nh, B=B, S=S, ov=ov, te=te, ln=ln, seed=seed, actor_hidden=actor_hidden, cap_q=cap_q)
    if hidden is not None:   # (a case without it is the dict it always was: tests/golden/iqld records its case)
        c['hidden'] = tuple(hidden)
    return c


# one update against the fp64 oracle: H 64 / B 64 for the three variants x both target_extraction values; the default shape; B 16 (the
# top-10 count is 1); no LayerNorm
FIRST = {f'{ov}-te{te}': case(ov=ov, te=te, seed=10 + 3 * i + te)
         for i, ov in enumerate(('binary', 'binary_awr_loss', 'binary_softmax_loss')) for te in (0, 1)}
FIRST['default-shape'] = case(H=512, B=256, seed=131)
FIRST['b16'] = case(B=16, seed=132)
FIRST['no-ln'] = case(ln=0, seed=33)
# shapes that switch kernel paths: act 1, 8, 17 (the padded action width crossing 16), obs 5 and 70, 2 and 4 layers, actor_hidden_dims
# differing from hidden_dims, denoise_steps 1, 4, 16
SHAPES = {
    'od5-ad1': case(od=5, ad=1, B=32, seed=40),
    'nh2-S4': case(nh=2, S=4, B=32, seed=41, ov='binary'),
    'od70-ad17-S1': case(od=70, ad=17, S=1, B=32, seed=42, ov='binary_softmax_loss'),
    'ad17-nh2': case(ad=17, nh=2, B=32, seed=43, te=0),
    'od5-S4': case(od=5, S=4, B=32, seed=44),
    'actor-hidden': case(B=32, seed=45, actor_hidden=(128, 64)),
    'w50-padded': case(B=32, seed=46, hidden=(50, 50, 50)),   # widths that are no multiple of 16: out 50 of out_p 64 in all three nets
}
STEP_KINDS = case(seed=50)
SWITCH = [case(B=64, seed=60), case(B=16, seed=61), case(B=256, seed=62)]   # one agent, the batch and noise of each size
# the shapes and batches at which the update's kernels change (tests/test_gpu_iqld.py::test_paths_match_fp64_restatement asserts each
# path from the engine's plan): the 2B-row passes at M 2048 (b1024), 544 (b272) and 4128 (b2064-*), the weight kernel past its 2048-row
# LDS stage (b2064-awr; b2064-binary with every positive weight tied), padded action width 32 and an actor in_p of 192 under hidden 512
# (humanoidmaze), act == padded width 16 (act16), hidden 1024 (wide1024) and widths that differ layer to layer in both families (ragged)
PATHS = {
    'humanoidmaze': case(od=69, ad=21, H=512, B=256, seed=200),
    'act16': case(ad=16, H=512, B=256, seed=220, ov='binary_softmax_loss'),
    'b1024': case(od=40, ad=4, H=512, B=1024, seed=242, ov='binary'),
    'b272': case(H=512, B=272, seed=261),
    'b2064-awr': case(B=2064, seed=280),
    'b2064-binary': case(B=2064, seed=300, ov='binary'),
    'wide1024': case(H=1024, nh=2, B=48, seed=320),
    'ragged': case(B=32, seed=340, ov='binary_softmax_loss', hidden=(48, 80, 64), actor_hidden=(128, 64, 96)),
}
# after the full update of these two: a critic-only and then an actor-only step on the batch and noise of these data seeds (the other
# two update programs at those sizes)
PATH_STEPS = {'humanoidmaze': (600, 620), 'b1024': (680, 700)}
# one agent through these batch sizes, full updates: hidden 512 across M 512 -> 2048 -> 544 -> 512 of the 2B-row passes, and hidden 64 across
# the weight kernel's 2048-row stage and back.  The first entry's seed builds the parameters, every entry's seed its own batch and noise.
WALK512 = [case(H=512, B=256, seed=300), case(H=512, B=1024, seed=700), case(H=512, B=272, seed=730), case(H=512, B=256, seed=761)]
WALK64 = [case(B=64, seed=340), case(B=2064, seed=805), case(B=64, seed=830)]
TRAJECTORY = case(seed=470, cap_q=0.1)   # a high temperature: the value net learns and the advantages sink, rows still reach the cap at every step


def config(c):
    cfg = DO.get_config()
    hidden = tuple(c.get('hidden') or (c['H'],) * c['nh'])
    cfg.update(actor_hidden_dims=tuple(c['actor_hidden'] or hidden), hidden_dims=hidden, batch_size=c['B'],
               denoise_steps=c['S'], optimal_var=c['ov'], target_extraction=c['te'], use_layer_norm=c['ln'])
    return cfg


def data(c, seed=None):
    seed = c['seed'] if seed is None else seed
    return DO.make_batch(c['od'], c['ad'], c['B'], 1000 + seed), DO.make_noise(c['B'], c['ad'], c['S'], 2000 + seed)


def awr_temperature(adv, cap_q=0.85):
    pos = adv[adv > 0]
    return float(f'{DO.LOG100 / np.quantile(pos, cap_q):.3g}')


def build(c, dtype=np.float64):
    """(cfg, params float32, batch, noise, restatement in `dtype` on those parameters)."""
    cfg = config(c)
    params = DO.randomize(DO.init_params(c['seed'], c['od'], c['ad'], cfg), c['seed'] + 1, q_spread=3.0)
    batch, noise = data(c)
    ref = DO.center_value(DO.OracleIQLD(params, cfg, c['od'], c['ad'], np.float64), batch)
    cfg['awr_temperature'] = awr_temperature(ref.adv(batch)[0], c.get('cap_q', 0.85))
    params = DO.O.tree_map(lambda a: a.astype(np.float32), ref.params)
    return cfg, params, batch, noise, DO.OracleIQLD(params, cfg, c['od'], c['ad'], dtype)


def check_margins(ref, batch, what=''):
    """The admission rule above on ref's current (fp64) parameters."""
    m = ref.kink_margins(batch)
    assert m['adv'] >= MARGIN, (what, m)
    assert m['expectile'] >= MARGIN, (what, m)
    assert m['positive'] >= 1 and m['negative'] >= 1, (what, m)
    if ref.config['optimal_var'] == 'binary_awr_loss':
        assert m['exp_cap'] >= MARGIN and m['capped'] >= 1, (what, m)
    return m


def all_cases():
    out = dict(FIRST)
    out.update(SHAPES)
    out['step-kinds'] = STEP_KINDS
    out['trajectory'] = TRAJECTORY
    out.update({f'switch-{c["B"]}': c for c in SWITCH})
    out.update(PATHS)
    out['walk512'], out['walk64'] = WALK512[0], WALK64[0]
    return out


def trajectory_kind(i):
    """(update_critic, update_actor) of step i of the mixed trajectory: full, critic-only and actor-only steps, and every tenth neither."""
    if i % 10 == 9:
        return False, False
    return [(True, True), (True, False), (False, True)][i % 3]


SAMPLER_HEAD_SCALE = 2.0
# the sampler at the humanoidmaze shape (act 21: padded action width 32; hidden 512).  fp32 numpy at a head scale of 2 is 1.2e-5 from
# fp64 at cfg 3 on these inputs, at 1 it is 4.6e-6; at 0.5 it is 2.5e-6, a factor of 2 inside the 5e-6 that
# tests/test_iqld_cpu.py::test_fp32_rounding_of_the_cfg_sampler_at_hidden_512 asserts, and 38 % of the coordinates still end on the clip
SAMPLER512 = case(od=69, ad=21, H=512, seed=81)
SAMPLER512_HEAD_SCALE = 0.5
SAMPLER512_N = (1, 37, 2049)


def sampler_problem(scale=SAMPLER_HEAD_SCALE, c=None):
    """(cfg, params, None) of the sampler tests: randomized parameters with the head kernel scaled so that the clip is reached."""
    c = c or case(seed=80)
    cfg = config(c)
    params = DO.randomize(DO.init_params(c['seed'], c['od'], c['ad'], cfg), c['seed'] + 1)
    params['actor']['Dense_0']['kernel'] = (params['actor']['Dense_0']['kernel'] * np.float32(scale)).astype(np.float32)
    return cfg, params, None


def sampler_inputs(n, od=OD, ad=AD):
    rng = np.random.default_rng(n)
    return rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal((n, ad)).astype(np.float32)
