"""GPU: the visual encoder's kernels against the fp64 oracle at every image shape that switches a kernel path (DESIGN.md section 2,
"pinned routing").

Each case runs one update and reads every encoder pass back through the diagnostic export fql_debug_enc (activations, pool winners,
and the plan: pool fusion, bf16 x 3 split, rows per workgroup).  Then:
* forward: pool, c1, y, the final ReLU, z and E of every pass (and c0 where the first convolution is not fused with its pool) within a
  bound relative to the tensor's largest magnitude;
* decisions: every pool winner and ReLU sign the engine took equals the oracle's, except inside a near-tie band (top-two gap, or
  distance from 0, within DECISION_EPS times the tensor's scale), and that band holds at most 1e-4 of all decisions;
* gradients: the oracle is given the engine's decisions (OracleFQL(routing=...)), so a tie decided the other way moves no gradient;
  then every leaf - convolutions and their biases included - within the tight per-leaf bound of the state path (tests/util.py);
  the 13 infos, post-step parameters and Polyak too;
* sample_actions / compute_flow_actions, and on the frame-stacked shapes the device gather, bitwise against the oracle's.
The fp64 oracle of a case is computed once and shared by its fp32 and bf16x3 runs (recomputed only if the engine's decisions differ).
"""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import encoder_oracle as E
from oracle import fql_oracle as O
from tests.util import assert_info_close, leaf_dict, randomize_params

pytestmark = pytest.mark.gpu

AD = 4
HIDDEN = (64, 64, 64, 64)
ENC_PASSES = (  # (fql_debug_enc index, module, images)  - the onestep pass encodes [obs ; next_obs], the target pass next_obs
    (0, 'modules_critic', 'obs'), (1, 'modules_actor_bc_flow', 'obs'), (2, 'modules_actor_onestep_flow', 'both'),
    (3, 'modules_target_critic', 'next'))
DIFFERENTIATED = ('modules_critic', 'modules_actor_bc_flow', 'modules_actor_onestep_flow')

# id: (H, W, C, B, encoder, plan).  plan: 'fused' = stack 0's first convolution runs fused with its pool; 'R' = {(stack, conv):
# (rows forward, rows data gradient, rows weight gradient)} for the convolutions whose tiling the case is there for.
SHAPES = {
    'c1_b48': (32, 32, 1, 48, 'impala_small', dict(fused=True)),                         # Ci_real 1, B % 32 != 0, generic Dense
    'unfused': (64, 64, 12, 64, 'impala_small', dict(fused=False, R={(0, 0): (2, 0, 2)})),  # 7 W C > 4096: u8 kernel + stand-alone pool
    'w96_fused': (32, 96, 4, 64, 'impala_small', dict(fused=True, R={(1, 1): (2, 2, 2), (2, 1): (4, 4, 4)})),   # 48/24/12-pixel rows
    'w96_unfused': (64, 96, 9, 64, 'impala_small', dict(fused=False, R={(0, 0): (1, 0, 1), (2, 1): (8, 8, 8)})),
    # the pool tile exceeds LDS at W = 128; at 8 x 32 x 32 a 4-row weight-gradient tile would overflow the float staging (rows left unwritten)
    'w128': (32, 128, 6, 64, 'impala_small', dict(fused=False, R={(0, 0): (1, 0, 1), (1, 1): (2, 2, 2), (2, 0): (2, 2, 2)})),
    'tall_c16': (128, 32, 16, 64, 'impala_small', dict(fused=True, R={(2, 1): (16, 16, 16)})),   # C = 16: no channel padding
    'w96_tall': (96, 96, 3, 64, 'impala_small', dict(fused=True, R={(2, 1): (4, 4, 4), (2, 2): (4, 4, 4)})),   # R = 4 at 12 x 12
    'impala_2blk': (32, 64, 3, 64, 'impala', dict(fused=True)),                          # num_blocks 2: c1[1], y[1]
}
CASES = [(k, 'fp32') for k in SHAPES] + [(k, 'bf16x3') for k in ('unfused', 'w96_fused', 'w96_unfused')]

# forward bound relative to the tensor's largest magnitude
FWD_TOL = {'fp32': 2e-5, 'bf16x3': 1e-4}
# near-tie band of the decisions, relative to the scale of the tensor decided on: a few times the engine's forward error there
DECISION_EPS = {'fp32': 2e-6, 'bf16x3': 1e-5}
# gradient bound relative to the leaf's largest gradient (tests/util.py: MLP leaves 2e-5, the visual path's leaves 5e-5; bf16x3 2e-4)
GRAD_TOL = {'fp32': (2e-5, 5e-5), 'bf16x3': (2e-4, 2e-4)}
MAX_PINNED = 1e-4            # decisions inside the near-tie band, as a fraction of all decisions of the update

_ORACLE = {}                 # shape id -> (params, batch, noise, forward caches)
_GRADS = {}                  # (shape id, routing digest) -> (info, grads, post-step params)
REPORT = {}


def _lib():
    from fql_amd import _cabi
    lib = _cabi.load()
    lib.fql_debug_enc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.fql_debug_enc.restype = C.c_int
    return lib


def _read(agent, enc, code, shape, dt=np.float32):
    a = np.empty(shape, dt)
    rc = _lib().fql_debug_enc(agent._h, enc, code, a.ctypes.data, a.nbytes)
    assert rc == 0, (enc, code, shape, rc)
    return a


def _plan(agent, enc, s, nconv):
    p = _read(agent, enc, 100 * s + 50, (1 + 4 * nconv,), np.int32)
    return {'fused': bool(p[0]), 'split': [bool(v) for v in p[1::4]], 'R': [tuple(int(v) for v in p[2 + 4 * j:5 + 4 * j]) for j in range(nconv)]}


def _problem(sid):
    H, W, Cc, B, enc, _ = SHAPES[sid]
    rng = np.random.default_rng(100 + list(SHAPES).index(sid))
    batch = {'observations': rng.integers(0, 256, size=(B, H, W, Cc), dtype=np.uint8),
             'next_observations': rng.integers(0, 256, size=(B, H, W, Cc), dtype=np.uint8),
             'actions': rng.uniform(-1, 1, size=(B, AD)).astype(np.float32),
             'rewards': -(rng.random(B) < 0.9).astype(np.float32), 'masks': (rng.random(B) < 0.9).astype(np.float32)}
    return batch, O.make_noise(B, AD, 7)


def _cfg(sid, precision):
    H, W, Cc, B, enc, _ = SHAPES[sid]
    cfg = O.get_config()
    cfg.update(encoder=enc, actor_hidden_dims=HIDDEN, value_hidden_dims=HIDDEN, alpha=3.0, batch_size=B, precision=precision)
    return cfg


def _images(batch, which):
    return {'obs': batch['observations'], 'next': batch['next_observations'],
            'both': np.concatenate([batch['observations'], batch['next_observations']])}[which]


def _oracle_forward(sid, params, batch):
    """The oracle's own forward of every encoder pass, decisions included (fp64)."""
    out = {}
    for enc, mod, which in ENC_PASSES:
        p = O.tree_map(lambda a: np.asarray(a, np.float64), params[mod]['encoder'])
        e, cache = E.impala_forward(p, _images(batch, which), keep=True, dtype=np.float64)
        out[enc] = (e, cache)
    return out


def _engine_pass(agent, enc, n, H, W, nblk):
    """Every activation of one encoder pass and its pool winners, as the engine computed them."""
    st = []
    h, w = H, W
    for s, Co in enumerate((16, 32, 32)):
        d = {'c0': _read(agent, enc, 100 * s, (n, h, w, Co)),
             'pool': _read(agent, enc, 100 * s + 1, (n, h // 2, w // 2, Co)),
             'arg': _read(agent, enc, 100 * s + 4, (n, h // 2, w // 2, Co), np.uint8),
             'c1': [_read(agent, enc, 100 * s + 10 * b + 2, (n, h // 2, w // 2, Co)) for b in range(nblk)],
             'y': [_read(agent, enc, 100 * s + 10 * b + 3, (n, h // 2, w // 2, Co)) for b in range(nblk)]}
        st.append(d)
        h, w = h // 2, w // 2
    flat = h * w * 32
    return st, _read(agent, enc, 900, (n, flat)), _read(agent, enc, 901, (n, 512)), _read(agent, enc, 902, (n, 512))


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _pool_gap(c0):
    """Top-two gap of every 3x3 / stride 2 window (the pool's tie distance), shaped like the pool output."""
    n, h, w, c = c0.shape
    xp = np.pad(c0, ((0, 0), (0, 1), (0, 1), (0, 0)), constant_values=-np.inf)
    win = np.lib.stride_tricks.sliding_window_view(xp, (3, 3), axis=(1, 2))[:, ::2, ::2].reshape(n, h // 2, w // 2, c, 9)
    top2 = -np.partition(-win, 1, axis=-1)[..., :2]
    return top2[..., 0] - top2[..., 1]


def _check_decisions(got, want, dist, scale, eps, what, stats):
    """got / want: the engine's / oracle's decisions; dist: how far the oracle's value is from the tie.  Outside the band
    (dist <= eps scale) they agree."""
    near = dist <= eps * scale
    flip = got != want
    stats['flip_eps'] = max(stats['flip_eps'], float(dist[flip].max(initial=0) / scale))
    bad = flip & ~near
    assert not bad.any(), (what, int(bad.sum()), float(dist[bad].max() / scale), np.argwhere(bad)[:4].tolist())
    stats['pinned'] += int(near.sum())
    stats['flipped'] += int(flip.sum())
    stats['decisions'] += got.size


def _run_case(sid, precision):
    import fql_amd
    H, W, Cc, B, enc_name, plan_want = SHAPES[sid]
    nblk = 2 if enc_name == 'impala' else 1
    nconv = 1 + 2 * nblk
    cfg = _cfg(sid, precision)
    if sid not in _ORACLE:
        batch, noise = _problem(sid)
        agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
        params = randomize_params(agent.get_params(), seed=3, scale=0.05)
        _ORACLE[sid] = (params, batch, noise, _oracle_forward(sid, params, batch))
    else:
        params, batch, noise, _ = _ORACLE[sid]
        agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    params, batch, noise, fwd = _ORACLE[sid]
    agent.set_params(params)
    _, info = agent.update(batch, noise=noise)

    # ---- the plan this case is there for
    plans = [_plan(agent, 0, s, nconv) for s in range(3)]
    assert plans[0]['fused'] == plan_want['fused'], plans[0]
    for (s, j), r in plan_want.get('R', {}).items():
        assert plans[s]['R'][j] == r, (s, j, plans[s]['R'][j], r)
    for s in range(3):
        assert plans[s]['split'] == [precision == 'bf16x3'] * nconv, (s, plans[s])
    for e in range(1, 4):
        assert [_plan(agent, e, s, nconv) for s in range(3)] == plans       # every pass is planned alike

    # ---- forward, decisions
    tol, eps = FWD_TOL[precision], DECISION_EPS[precision]
    stats = {'pinned': 0, 'flipped': 0, 'decisions': 0, 'flip_eps': 0.0}
    fwd_err = {}
    routing = {}
    for enc, mod, which in ENC_PASSES:
        e_ref, cache = fwd[enc]
        n = e_ref.shape[0]
        st, frelu, z, e_got = _engine_pass(agent, enc, n, H, W, nblk)
        rt = {'arg': [], 'c1': [], 'inp': []}
        p = params[mod]['encoder']
        for s, sc in enumerate(cache['stacks']):
            k = p[f'stack_blocks_{s}']['Conv_0']
            c0_ref = E.conv3x3(sc['x0'], np.asarray(k['kernel'], np.float64), np.asarray(k['bias'], np.float64))
            pool_ref = cache['stacks'][s]['blocks'][0][0]
            checks = {'pool': (st[s]['pool'], pool_ref)}
            if not plans[s]['fused']:
                checks['c0'] = (st[s]['c0'], c0_ref)
            _check_decisions(st[s]['arg'], sc['arg'], _pool_gap(c0_ref), np.abs(c0_ref).max(), eps, (sid, enc, s, 'arg'), stats)
            rt['arg'].append(st[s]['arg'])
            rt['c1'].append([]); rt['inp'].append([])
            for b, (inp_ref, c1_ref, _, _) in enumerate(sc['blocks']):
                y_ref = sc['blocks'][b + 1][0] if b + 1 < nblk else (cache['stacks'][s + 1]['x0'] if s < 2 else cache['final'])
                checks[f'c1[{b}]'] = (st[s]['c1'][b], c1_ref)
                checks[f'y[{b}]'] = (st[s]['y'][b], y_ref)
                inp_got = st[s]['pool'] if b == 0 else st[s]['y'][b - 1]
                for nm, g, r in (('c1', st[s]['c1'][b], c1_ref), ('inp', inp_got, inp_ref)):
                    _check_decisions(g > 0, r > 0, np.abs(r), np.abs(r).max(), eps, (sid, enc, s, b, nm), stats)
                    rt[nm][s].append(g > 0)
            for nm, (g, r) in checks.items():
                err = _rel(g, r)
                fwd_err[nm] = max(fwd_err.get(nm, 0.0), err)
                assert err <= tol, (sid, precision, enc, s, nm, err)
        fin_ref = cache['final']
        fin_got = st[2]['y'][-1]
        _check_decisions(fin_got > 0, fin_ref > 0, np.abs(fin_ref), np.abs(fin_ref).max(), eps, (sid, enc, 'final'), stats)
        rt['final'] = fin_got > 0
        # the z buffer holds GELU'(z), what the backward pass reads (GF_SAVE_Z)
        for nm, g, r in (('frelu', frelu, cache['flat']), ("gelu'(z)", z, E.gelu_tanh_grad(cache['mlp'][0][1])), ('E', e_got, e_ref)):
            err = _rel(g, r)
            fwd_err[nm] = max(fwd_err.get(nm, 0.0), err)
            assert err <= tol, (sid, precision, enc, nm, err)
        if mod in DIFFERENTIATED:     # the differentiated pass covers batch['observations']: the first B images
            routing[mod] = {'arg': [a[:B] for a in rt['arg']], 'c1': [[m[:B] for m in l] for l in rt['c1']],
                            'inp': [[m[:B] for m in l] for l in rt['inp']], 'final': rt['final'][:B]}
    assert stats['pinned'] <= MAX_PINNED * stats['decisions'], stats

    # ---- gradients with the engine's decisions
    digest = hash(b''.join(np.packbits(np.asarray(m, bool)).tobytes() for mod in DIFFERENTIATED
                           for m in [*routing[mod]['arg'], *sum(routing[mod]['c1'], []), *sum(routing[mod]['inp'], []), routing[mod]['final']]))
    key = (sid, digest)
    if key not in _GRADS:
        ref = O.OracleFQL(params, dict(cfg), (H, W, Cc), AD, np.float64, routing=routing)
        _, info_r, g_ref = ref.grads(batch, noise)
        info_r.update(ref.grad_stats(g_ref))
        ref.apply_gradients(g_ref)
        _GRADS[key] = ({k: float(info_r[k]) for k in O.INFO_KEYS}, g_ref, leaf_dict(ref.params))
    info_r, g_ref, new_ref = _GRADS[key]
    if precision == 'fp32':
        assert_info_close(info, info_r, rtol=5e-5, atol=5e-6)
    else:
        for k in O.INFO_KEYS:
            assert abs(info[k] - info_r[k]) <= 1e-4 * max(1.0, abs(info_r[k])), (k, info[k], info_r[k])
    opt = agent.get_opt_state()
    mu, nu = leaf_dict(opt['mu']), leaf_dict(opt['nu'])
    new = leaf_dict(agent.get_params())
    t_mlp, t_enc = GRAD_TOL[precision]
    worst = {'MLP': 0.0, 'Dense': 0.0, 'conv': 0.0}
    for path, g in leaf_dict(g_ref).items():
        if path.startswith('modules_target_critic'):
            assert np.abs(new[path] - new_ref[path]).max() <= 1e-6, path          # Polyak, encoder leaves included
            continue
        group = 'conv' if '/stack_blocks_' in path else 'Dense' if '/encoder/' in path else 'MLP'
        scale = np.abs(g).max()
        tol_g = (t_enc if group != 'MLP' else t_mlp) * scale + 1e-9
        err = np.abs(mu[path] / 0.1 - g).max()
        worst[group] = max(worst[group], float(err / max(scale, 1e-30)))
        assert err <= tol_g, (sid, precision, path, err / scale)
        np.testing.assert_allclose(nu[path] / 0.001, g * g, rtol=1e-4 if precision == 'fp32' else 1e-3,
                                   atol=tol_g * scale + 1e-12, err_msg=f'nu {path}')
        d = np.abs(new[path] - new_ref[path])
        stable = np.abs(g) > 50 * tol_g                                             # Adam's first step is sign-like near g = 0
        assert d[stable].max(initial=0) <= 3e-6, (path, d[stable].max())
        assert d.max() <= 2 * cfg['lr'] + 1e-6, path
    REPORT[(sid, precision)] = dict(plan=[(p['fused'], p['R']) for p in plans], worst=worst, fwd=max(fwd_err.values()), **stats)
    return agent, params, batch


@pytest.mark.parametrize('sid,precision', CASES, ids=[f'{s}-{p}' for s, p in CASES])
def test_visual_shape_matches_the_oracle_leaf_by_leaf(sid, precision):
    t0 = time.time()
    agent, params, batch = _run_case(sid, precision)
    if precision == 'fp32':     # sample_actions / compute_flow_actions at test_gpu_visual.py's bounds, on the updated parameters
        H, W, Cc, B, enc_name, _ = SHAPES[sid]
        ref = O.OracleFQL(agent.get_params(), dict(_cfg(sid, precision)), (H, W, Cc), AD, np.float64)
        obs, z = batch['observations'][:20], O.make_noise(20, AD, 8)['z']
        np.testing.assert_allclose(agent.sample_actions(obs, noises=z), ref.sample_actions(obs, z), atol=5e-6)
        np.testing.assert_allclose(agent.compute_flow_actions(obs, z), ref.compute_flow_actions(obs, z), atol=2e-5)
    print(f'\n[{sid} {precision}] {REPORT[(sid, precision)]} {time.time() - t0:.1f}s')


def test_debug_hook_refuses_reads_past_a_buffer():
    """fql_debug_enc checks the request against the buffer it was allocated with: one float too many is FQL_E_INVALID, an unknown code
    or a block that does not exist FQL_E_NOTFOUND."""
    import fql_amd
    sid = 'c1_b48'
    batch, _ = _problem(sid)
    H, W, Cc, B, _, _ = SHAPES[sid]
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], _cfg(sid, 'fp32'))
    lib = _lib()
    exact = (B, H // 2, W // 2, 16)
    buf = np.empty(int(np.prod(exact)) + 64, np.float32)
    assert lib.fql_debug_enc(agent._h, 0, 1, buf.ctypes.data, 4 * int(np.prod(exact))) == 0
    assert lib.fql_debug_enc(agent._h, 0, 1, buf.ctypes.data, 4 * int(np.prod(exact)) + 4) == -1
    assert lib.fql_debug_enc(agent._h, 3, 902, buf.ctypes.data, 4 * B * 512 + 4) == -1
    assert lib.fql_debug_enc(agent._h, 0, 12, buf.ctypes.data, 4) == -5                  # impala_small has one block per stack
    assert lib.fql_debug_enc(agent._h, 0, 950, buf.ctypes.data, 4) == -5
    assert lib.fql_debug_enc(agent._h, 0, 350, buf.ctypes.data, 4) == -5                # three stacks
    assert lib.fql_debug_enc(agent._h, 4, 1, buf.ctypes.data, 4) == -1
    assert lib.fql_debug_enc(agent._h, 0, 50, buf.ctypes.data, 4 * 14) == -1            # the plan is 1 + 4 x 3 int32


@pytest.mark.parametrize('sid,fs', [('unfused', 4), ('w96_unfused', 3), ('w128', 2)])
def test_visual_shape_dataset_gather_is_bitwise_the_oracle(sid, fs):
    """utils/datasets.py:73-112 on the device at this shape: update_from_dataset(idxs, crop_froms) == update(batch stacked and cropped
    by the oracle), with crop offsets 0 and 6 and rows at episode starts."""
    import fql_amd
    H, W, Cc, B, _, _ = SHAPES[sid]
    cfg = _cfg(sid, 'fp32')
    rng = np.random.default_rng(31)
    n, fc = 160, Cc // fs
    frames = rng.integers(0, 256, size=(n, H, W, fc), dtype=np.uint8)
    nxt = rng.integers(0, 256, size=(n, H, W, fc), dtype=np.uint8)
    terminals = (rng.random(n) < 0.05).astype(np.float32); terminals[-1] = 1
    terminals[[9, 40]] = 1
    ds = {'observations': frames, 'next_observations': nxt, 'terminals': terminals,
          'actions': rng.uniform(-1, 1, size=(n, AD)).astype(np.float32), 'rewards': -np.ones(n, np.float32), 'masks': 1 - terminals}
    ex = np.zeros((1, H, W, Cc), np.uint8)
    a = fql_amd.FQLAgent.create(3, ex, ds['actions'][:1], cfg)
    b = fql_amd.FQLAgent.create(3, ex, ds['actions'][:1], cfg)
    params = randomize_params(a.get_params(), seed=8, scale=0.05)
    a.set_params(params); b.set_params(params)
    a.upload_dataset(ds, frame_stack=fs, p_aug=0.5)
    idxs = rng.integers(0, n, size=B)
    idxs[:6] = [0, 1, 10, 11, 41, n - 1]                                   # episode starts and their successors: clamped stacking
    crops = rng.integers(0, 7, size=(B, 2))
    crops[:4] = [[0, 0], [6, 6], [0, 6], [6, 0]]
    nz = O.make_noise(B, AD, 12)
    _, ia = a.update_from_dataset(B, idxs=idxs, noise=nz, want_info=True, crop_froms=crops)
    obs, nobs = E.stack_frames(frames, nxt, terminals, idxs, fs)
    batch = {'observations': E.random_crop_batch(obs, crops), 'next_observations': E.random_crop_batch(nobs, crops),
             'actions': ds['actions'][idxs], 'rewards': ds['rewards'][idxs], 'masks': ds['masks'][idxs]}
    _, ib = b.update(batch, noise=nz)
    assert ia == ib
    pa, pb = leaf_dict(a.get_params()), leaf_dict(b.get_params())
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
