"""CPU: the numpy encoder oracle against an independent torch-autograd restatement (conv2d / max_pool2d / gelu)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_oracle as E


def torch_forward(p, x_u8):
    x = torch.as_tensor(np.asarray(x_u8), dtype=torch.float64) / 255.0
    x = x.permute(0, 3, 1, 2)
    ns = sum(1 for k in p if k.startswith('stack_blocks_'))

    def conv(x, c):
        return F.conv2d(x, c['kernel'].permute(3, 2, 0, 1), c['bias'], padding=1)

    for s in range(ns):
        st = p[f'stack_blocks_{s}']
        x = conv(x, st['Conv_0'])
        x = F.max_pool2d(F.pad(x, (0, 1, 0, 1), value=float('-inf')), 3, 2)
        for b in range((len(st) - 1) // 2):
            inp = x
            x = conv(F.relu(x), st[f'Conv_{1 + 2 * b}'])
            x = conv(F.relu(x), st[f'Conv_{2 + 2 * b}'])
            x = x + inp
    x = F.relu(x).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    for i in range(len(p['MLP_0'])):
        d = p['MLP_0'][f'Dense_{i}']
        x = F.gelu(x @ d['kernel'] + d['bias'], approximate='tanh')
    return x


def to_torch(tree):
    if isinstance(tree, dict):
        return {k: to_torch(v) for k, v in tree.items()}
    return torch.tensor(np.asarray(tree, np.float64), requires_grad=True)


def flat(tree, prefix=''):
    out = {}
    for k in sorted(tree):
        v = tree[k]
        if isinstance(v, dict):
            out.update(flat(v, f'{prefix}{k}/'))
        else:
            out[prefix + k] = v
    return out


@pytest.mark.parametrize('name,hw,c', [('impala_small', 16, 9), ('impala_debug', 8, 3), ('impala', 16, 3)])
def test_encoder_forward_backward_match_torch(name, hw, c):
    rng = np.random.default_rng(0)
    p = E.init_encoder_params(rng, (hw, hw, c), name, np.float64)
    for path, leaf in flat(p).items():          # non-zero biases so their gradients are exercised
        if path.endswith('bias'):
            leaf[...] = rng.normal(size=leaf.shape) * 0.1
    x = rng.integers(0, 256, size=(3, hw, hw, c), dtype=np.uint8)
    out, cache = E.impala_forward(p, x, keep=True, dtype=np.float64)
    tp = to_torch(p)
    tout = torch_forward(tp, x)
    np.testing.assert_allclose(out, tout.detach().numpy(), rtol=1e-10, atol=1e-12)
    dout = rng.normal(size=out.shape)
    g = E.impala_backward(p, cache, dout)
    (tout * torch.as_tensor(dout)).sum().backward()
    fg, ft = flat(g), flat(tp)
    assert set(fg) == set(ft)
    for path in fg:
        np.testing.assert_allclose(fg[path], ft[path].grad.numpy(), rtol=1e-9, atol=1e-11, err_msg=path)


def test_leaf_names_and_shapes_impala_small():
    p = E.init_encoder_params(np.random.default_rng(1), (64, 64, 9), 'impala_small')
    f = flat(p)
    assert f['stack_blocks_0/Conv_0/kernel'].shape == (3, 3, 9, 16)
    assert f['stack_blocks_1/Conv_0/kernel'].shape == (3, 3, 16, 32)
    assert f['stack_blocks_2/Conv_2/kernel'].shape == (3, 3, 32, 32)
    assert f['MLP_0/Dense_0/kernel'].shape == (2048, 512)      # 8 * 8 * 32
    assert len(f) == 2 * 9 + 2


def test_max_pool_same_padding_sits_at_the_end():
    x = np.arange(16, dtype=np.float64).reshape(1, 4, 4, 1)
    y, arg = E.max_pool(x)
    np.testing.assert_array_equal(y[0, :, :, 0], [[10, 11], [14, 15]])
    np.testing.assert_array_equal(arg[0, :, :, 0], [[8, 7], [5, 4]])   # last window row/col only see 2 valid rows/cols


def test_stack_frames_clamps_to_episode_start():
    n = 10
    frames = np.arange(n, dtype=np.uint8).reshape(n, 1, 1, 1)
    nxt = frames + 100
    terminals = np.zeros(n); terminals[4] = 1; terminals[9] = 1          # episodes [0..4], [5..9]
    obs, nobs = E.stack_frames(frames, nxt, terminals, np.array([0, 1, 5, 6, 9]), 3)
    np.testing.assert_array_equal(obs[:, 0, 0, :], [[0, 0, 0], [0, 0, 1], [5, 5, 5], [5, 5, 6], [7, 8, 9]])
    np.testing.assert_array_equal(nobs[:, 0, 0, :], [[0, 0, 100], [0, 1, 101], [5, 5, 105], [5, 6, 106], [8, 9, 109]])


def test_random_crop_matches_edge_pad_slice():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(2, 8, 8, 3), dtype=np.uint8)
    out = E.random_crop_batch(img, np.array([[3, 3], [0, 6]]))
    np.testing.assert_array_equal(out[0], img[0])                          # offset == padding: identity
    np.testing.assert_array_equal(out[1, 3:, :5], img[1, :5, 3:])          # shifted down 3, left 3
    np.testing.assert_array_equal(out[1, 0, :5], img[1, 0, 3:])            # top rows replicate the edge


def make_visual_problem(B=4, hw=16, c=3, ad=4, enc='impala_debug', hidden=(32, 32), seed=0, dtype=np.float64):
    from oracle import fql_oracle as O
    cfg = O.get_config()
    cfg.update(encoder=enc, actor_hidden_dims=hidden, value_hidden_dims=hidden, alpha=3.0)
    rng = np.random.default_rng(seed)
    batch = {
        'observations': rng.integers(0, 256, size=(B, hw, hw, c), dtype=np.uint8),
        'next_observations': rng.integers(0, 256, size=(B, hw, hw, c), dtype=np.uint8),
        'actions': rng.uniform(-1, 1, size=(B, ad)).astype(np.float32),
        'rewards': -np.ones(B, np.float32), 'masks': np.ones(B, np.float32),
    }
    agent = O.OracleFQL.create(seed + 1, (hw, hw, c), ad, cfg, dtype)
    return O, cfg, agent, batch, O.make_noise(B, ad, seed + 2)


def test_visual_total_loss_gradients_match_finite_differences():
    """jax.grad over the whole tree (utils/flax_utils.py:137) incl. the three encoders, against central differences."""
    O, cfg, agent, batch, noise = make_visual_problem()
    loss, info, grads = agent.grads(batch, noise)
    agent.frozen = O.tree_map(lambda a: a.copy(), agent.params)   # stored-param uses stay put while a leaf is perturbed
    leaves = dict(O.tree_leaves_with_path(agent.params))
    gl = dict(O.tree_leaves_with_path(grads))
    assert any('/encoder/' in k for k in gl)
    assert all(np.all(v == 0) for k, v in gl.items() if k.startswith('modules_target_critic'))
    rng = np.random.default_rng(5)
    paths = [k for k in leaves if not k.startswith('modules_target_critic')]
    checked, kinks = 0, 0
    for path in paths:
        leaf = leaves[path]
        for _ in range(2):
            idx = tuple(rng.integers(0, n) for n in leaf.shape)
            old = leaf[idx]
            h = 1e-6
            leaf[idx] = old + h; lp, _ = agent.total_loss(batch, noise)
            leaf[idx] = old - h; lm, _ = agent.total_loss(batch, noise)
            leaf[idx] = old
            fd = (lp - lm) / (2 * h)
            err = abs(fd - gl[path][idx])
            assert err <= 1e-6 + 2e-2 * abs(fd), (path, idx, fd, gl[path][idx])
            kinks += err > 1e-7 + 1e-4 * abs(fd)        # a ReLU / max-pool switch inside +-h (piecewise-linear nets)
            checked += 1
    assert checked >= 100 and kinks <= checked // 20


def test_visual_update_runs_and_moves_every_trainable_leaf():
    O, cfg, agent, batch, noise = make_visual_problem(dtype=np.float32)
    before = {k: v.copy() for k, v in O.tree_leaves_with_path(agent.params)}
    loss, info = agent.update(batch, noise)
    assert set(info) == set(O.INFO_KEYS) and all(np.isfinite(v) for v in info.values())
    after = dict(O.tree_leaves_with_path(agent.params))
    for k in before:
        if k.endswith('kernel'):
            assert not np.array_equal(before[k], after[k]), k


def test_visual_numpy_oracle_equals_torch_autograd_restatement():
    """The hand-derived visual backward (fql_oracle + encoder_oracle) against torch.autograd over F.conv2d / F.max_pool2d."""
    from oracle.fql_oracle_torch import TorchFQL
    O, cfg, agent, batch, noise = make_visual_problem(B=4, hw=16, c=3, enc='impala_debug')
    tref = TorchFQL(agent.params, cfg, torch.float64)
    loss, info, grads = agent.grads(batch, noise)
    tl, tinfo, tg = tref.grads(batch, noise)
    assert abs(float(tl) - loss) <= 1e-10 * abs(loss)
    for k, v in tinfo.items():
        assert abs(float(v.detach()) - info[k]) <= 1e-9 * (1 + abs(info[k])), k
    gl = dict(O.tree_leaves_with_path(grads))
    for path, g in O.tree_leaves_with_path(tg):
        np.testing.assert_allclose(g.numpy(), gl[path], rtol=1e-8, atol=1e-11, err_msg=path)
    # three updates stay together (Adam, Polyak incl. the encoder leaves)
    for s in range(3):
        nz = O.make_noise(4, 4, 30 + s)
        _, ia = agent.update(batch, nz)
        _, ib = tref.update(batch, nz)
        for k in ia:
            assert abs(ia[k] - ib[k]) <= 1e-8 * (1 + abs(ia[k])), k


def _random_encoder(name, hw, c, seed):
    rng = np.random.default_rng(seed)
    p = E.init_encoder_params(rng, hw + (c,), name, np.float64)
    for path, leaf in flat(p).items():
        if path.endswith('bias'):
            leaf[...] = rng.normal(size=leaf.shape) * 0.1
    x = rng.integers(0, 256, size=(3,) + hw + (c,), dtype=np.uint8)
    return rng, p, x


@pytest.mark.parametrize('name,hw,c', [('impala_small', (16, 24), 5), ('impala', (16, 16), 3)])
def test_routing_with_own_decisions_is_bitwise_the_default(name, hw, c):
    rng, p, x = _random_encoder(name, hw, c, 3)
    out, cache = E.impala_forward(p, x, keep=True, dtype=np.float64)
    routing = E.routing_of(cache)
    assert len(routing['arg']) == 3 and len(routing['c1'][0]) == (2 if name == 'impala' else 1)
    out_r, cache_r = E.impala_forward(p, x, keep=True, dtype=np.float64, routing=routing)
    np.testing.assert_array_equal(out_r, out)
    dout = rng.normal(size=out.shape)
    g, g_r = flat(E.impala_backward(p, cache, dout)), flat(E.impala_backward(p, cache_r, dout))
    for path in g:
        np.testing.assert_array_equal(g_r[path], g[path], err_msg=path)


def test_oracle_fql_routing_with_own_decisions_is_bitwise_the_default():
    O, cfg, agent, batch, noise = make_visual_problem(enc='impala_small', hw=16)
    _, _, g = agent.grads(batch, noise)
    routing = {}
    for m in ('modules_critic', 'modules_actor_bc_flow', 'modules_actor_onestep_flow'):
        _, cache = E.impala_forward(agent.params[m]['encoder'], batch['observations'], keep=True, dtype=np.float64)
        routing[m] = E.routing_of(cache)
    pinned = O.OracleFQL(agent.params, cfg, (16, 16, 3), 4, np.float64, routing=routing)
    loss_p, info_p, g_p = pinned.grads(batch, noise)
    loss, info, _ = agent.grads(batch, noise)
    assert loss_p == loss and info_p == info
    for path, leaf in O.tree_leaves_with_path(g):
        np.testing.assert_array_equal(dict(O.tree_leaves_with_path(g_p))[path], leaf, err_msg=path)


def test_pool_routing_sends_the_gradient_to_the_named_input_at_a_tie():
    """A window whose maximum sits at two offsets: by default the first wins (row-major); routed, the named one does."""
    rng = np.random.default_rng(4)
    x = rng.normal(size=(2, 6, 8, 3))
    x[0, 2, 3, 1] = x[0, 2, 4, 1] = x[0, 2:5, 2:5, 1].max() + 1.0          # window (1, 1): offsets 3 * 0 + 1 and 3 * 0 + 2
    y, arg = E.max_pool(x)
    assert arg[0, 1, 1, 1] == 1
    routed = arg.copy()
    routed[0, 1, 1, 1] = 2
    y_r, arg_r = E.max_pool(x, routed)
    np.testing.assert_array_equal(y_r, y)                                  # same value either way: it is a tie
    np.testing.assert_array_equal(arg_r, routed)
    dy = rng.normal(size=y.shape)
    # hand scatter with torch: every window's gradient to input (2 oh + a // 3, 2 ow + a % 3), added up
    n, ho, wo, c = dy.shape
    idx = np.zeros(dy.shape, np.int64)
    for o in np.ndindex(*dy.shape):
        a = int(routed[o])
        idx[o] = (2 * o[1] + a // 3) * (x.shape[2] + 1) + 2 * o[2] + a % 3
    t = torch.zeros(n, c, (x.shape[1] + 1) * (x.shape[2] + 1), dtype=torch.float64)
    t.scatter_add_(2, torch.as_tensor(idx).permute(0, 3, 1, 2).reshape(n, c, -1),
                   torch.as_tensor(dy).permute(0, 3, 1, 2).reshape(n, c, -1))
    want = t.reshape(n, c, x.shape[1] + 1, x.shape[2] + 1).permute(0, 2, 3, 1).numpy()[:, :-1, :-1]
    got = E.max_pool_bwd(arg_r, dy, x.shape[1:3])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)             # overlapping windows: another order of adds
    moved = got - E.max_pool_bwd(arg, dy, x.shape[1:3])                      # only window (1, 1)'s gradient moved: (2, 3) -> (2, 4)
    want_moved = np.zeros_like(moved)
    want_moved[0, 2, 4, 1], want_moved[0, 2, 3, 1] = dy[0, 1, 1, 1], -dy[0, 1, 1, 1]
    np.testing.assert_allclose(moved, want_moved, rtol=0, atol=1e-15)


def test_relu_routing_passes_the_gradient_where_the_mask_is_set():
    """One decision of each ReLU kind (block input, c1, final output) flipped against its sign: forward and every leaf's
    gradient follow the given masks, checked against torch autograd through x * mask and a gather at the routed pool offsets."""
    rng, p, x = _random_encoder('impala_debug', (8, 8), 3, 5)
    _, cache = E.impala_forward(p, x, keep=True, dtype=np.float64)
    routing = E.routing_of(cache)
    # flip one decision of each kind (value need not be a tie: routing is followed as given)
    for key, where in (('inp', (0, 1, 2, 0)), ('c1', (1, 0, 1, 3))):
        m = routing[key][0][0].copy()
        m[where] = ~m[where]
        routing[key][0][0] = m
    fm = routing['final'].copy()
    fm[2, 0, 1, 2] = ~fm[2, 0, 1, 2]
    routing['final'] = fm
    out_r, cache_r = E.impala_forward(p, x, keep=True, dtype=np.float64, routing=routing)
    dout = rng.normal(size=out_r.shape)
    g_r = flat(E.impala_backward(p, cache_r, dout))
    # torch restatement of the same masked network: relu replaced by x * mask, pool by a gather at the routed offsets
    tp = to_torch(p)

    def conv(x, k, b):
        return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)

    def pool(x, arg):
        n, h, w, c = x.shape
        xp = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1), value=-float('inf'))
        win = xp.unfold(1, 3, 2).unfold(2, 3, 2)                            # [N, H/2, W/2, C, 3, 3]
        return torch.gather(win.reshape(*win.shape[:4], 9), -1, torch.as_tensor(arg, dtype=torch.int64)[..., None])[..., 0]

    h = torch.as_tensor(x, dtype=torch.float64) / 255.0
    for s in range(2):
        st = tp[f'stack_blocks_{s}']
        h = pool(conv(h, st['Conv_0']['kernel'], st['Conv_0']['bias']), routing['arg'][s])
        inp = h
        c1 = conv(inp * torch.as_tensor(routing['inp'][s][0]), st['Conv_1']['kernel'], st['Conv_1']['bias'])
        h = conv(c1 * torch.as_tensor(routing['c1'][s][0]), st['Conv_2']['kernel'], st['Conv_2']['bias']) + inp
    f = (h * torch.as_tensor(routing['final'])).reshape(h.shape[0], -1)
    d = tp['MLP_0']['Dense_0']
    z = f @ d['kernel'] + d['bias']
    out_t = 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    np.testing.assert_allclose(out_r, out_t.detach().numpy(), rtol=1e-10, atol=1e-12)
    (out_t * torch.as_tensor(dout)).sum().backward()
    ft = flat(tp)
    for path in g_r:
        np.testing.assert_allclose(g_r[path], ft[path].grad.numpy(), rtol=1e-9, atol=1e-11, err_msg=path)
    g = flat(E.impala_backward(p, cache, dout))
    assert any(np.abs(g[k] - g_r[k]).max() > 1e-9 for k in g)                # the flips moved some gradient
