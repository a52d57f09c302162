"""GPU: CFGRL agent groups (fql_cfgrl_group_*, CFGRLAgentGroup).  A member advanced by the group's fused program and sampled by the fused
call must be bitwise where its standalone twin is - a CFGRLAgent created with the member's seed, cfg and goal mixture, given the same
parameters, dataset and calls one at a time: fusing changes which launch a task rides in, never its arithmetic.  The standalone agent is
pinned to the fp64 restatement at these shapes by tests/test_gpu_cfgrl.py, so the twin is a checked reference and no tolerance is
involved."""
import ctypes as C

import numpy as np
import pytest

from oracle import fql_oracle as O
from tests import cfgrl_oracle as CO
from tests.util import assert_same_state, leaf_dict

pytestmark = pytest.mark.gpu
OD, AD = 29, 8
EMB = 'modules_unc_embed/Embed_0/embedding'
MIXES = ((1.0, 0.0, 0.0), (0.0, 0.5, 0.5), (0.2, 0.5, 0.3))   # actor_p_curgoal (1: the all_cur path), actor_p_trajgoal, actor_p_randomgoal
LENGTHS = (1, 2, 3, 17, 200, 1, 777, 1500)                    # eight trajectories, 2501 rows
ROW_KEYS = ('idx', 'goal_idx', 'do_cfg', 'goals')


def _cfg(H=64, B=64, nh=2, **kw):
    import fql_amd.cfgrl
    cfg = fql_amd.cfgrl.get_config()
    cfg.update(actor_hidden_dims=(H,) * nh, batch_size=B)
    cfg.update(kw)
    return cfg


def _example(od, ad, gd):
    return {'observations': np.zeros((1, od), np.float32), 'actions': np.zeros((1, ad), np.float32), 'value_goals': np.zeros((1, gd), np.float32)}


def _randomized(params, seed, scale=0.1):
    """Every bias, LayerNorm leaf and the unc_embed row moved off its initial value (kernels keep their init)."""
    rng = np.random.default_rng(seed)
    out = O.tree_map(lambda a: np.array(a, np.float32), params)
    for p, v in O.tree_leaves_with_path(out):
        if not p.endswith('/kernel'):
            v += (scale * rng.standard_normal(v.shape)).astype(np.float32)
    return out


_DATASETS = {}


def _dataset(reps, od=OD, ad=AD):
    """The synthetic goal-conditioned dataset, built once per (reps, od, ad) and left unchanged."""
    key = (bool(reps), od, ad)
    if key not in _DATASETS:
        _DATASETS[key] = CO.make_gc_dataset(od, ad, seed=70, lengths=LENGTHS, reps_dim=2 if reps else None)
    return _DATASETS[key]


def _setup(K, cfg, reps=False, mixes=None, cfgs=None, seeds=None, upload=True, same_params=False):
    """A group of K members and their standalone twins on one dataset: member and twin share the create seed, cfg, mixture and the
    randomised parameters; members differ from each other in all of them (same_params: in all but the parameters)."""
    import fql_amd
    ds = _dataset(reps)
    gd = 2 if reps else OD
    ex = _example(OD, AD, gd)
    seeds = list(seeds) if seeds is not None else [3 + i for i in range(K)]
    mixes = list(mixes) if mixes is not None else [MIXES[(i + 1) % 3] for i in range(K)]
    cfgs = list(cfgs) if cfgs is not None else [1.5 + i for i in range(K)]
    group = fql_amd.CFGRLAgentGroup.create(seeds, ex, cfg, cfgs=cfgs, goal_mixes=mixes)
    twins = []
    for i in range(K):
        t = fql_amd.CFGRLAgent.create(seeds[i], ex, dict(cfg, cfg=cfgs[i], actor_p_curgoal=mixes[i][0], actor_p_trajgoal=mixes[i][1],
                                                         actor_p_randomgoal=mixes[i][2]))
        p = _randomized(t.get_params(), 100 + (0 if same_params else i))
        t.set_params(p)
        group.members[i].set_params(p)
        if upload:
            t.upload_dataset(ds)
        twins.append(t)
    if upload:
        group.upload_dataset(ds)
    return ds, group, twins


def _assert_rows(m, t, what):
    rm, rt = m.read_rows(), t.read_rows()
    for k in ROW_KEYS:
        np.testing.assert_array_equal(rm[k], rt[k], err_msg=f'{what} {k}')
    for k in rm['draws']:
        np.testing.assert_array_equal(rm['draws'][k], rt['draws'][k], err_msg=f'{what} draws {k}')
    return rm


def _assert_infos(infos, want, what):
    from fql_amd.cfgrl import CFGRL_INFO_KEYS
    assert len(infos) == len(want)
    for i, (g, w) in enumerate(zip(infos, want)):
        g, w = g.to_dict(), w.to_dict()
        assert tuple(g) == CFGRL_INFO_KEYS == tuple(w), (what, i)
        assert g == w, (what, i, g, w)
        assert all(np.isfinite(v) for v in g.values()) and g['actor/actor_loss'] > 0 and g['grad/norm'] > 0, (what, i, g)


def _step(group, twins, B, want_info=False, idxs=None, do_cfg=None):
    infos = group.update_from_dataset(want_info=want_info, idxs=idxs, do_cfg=do_cfg)
    want = [t.update_from_dataset(B, want_info=want_info, idxs=None if idxs is None else np.asarray(idxs)[i],
                                  do_cfg=None if do_cfg is None else np.asarray(do_cfg)[i])[1] for i, t in enumerate(twins)]
    return infos, want


def _check(group, twins, what=''):
    group.synchronize()
    for i, (m, t) in enumerate(zip(group.members, twins)):
        assert_same_state(m, t)
        assert m.read_info() == t.read_info(), (what, i)


# ---- 1. twins on device-drawn rows, goals and masks, at the shapes that switch a path ------------------------------------------------
# hidden 64 x 2 at B 16: one chunk of everything.  B 272: the embed-gradient kernel's 256-row compaction loop runs twice, the second
# chunk ragged (16 rows).  hidden 512 x 4 at B 64: two of each thread's four column slots.  hidden 1024 x 2: all four.  Every shape runs
# at K = 1, 2 and 3; across its three runs it sees actor_layer_norm on and off and both goal tables (goal_dim 2 with oracle_reps;
# goal_dim == obs_dim, the observations), and each of the four (layer norm, table) pairs occurs at K >= 2.
SHAPES = {'h64-b16': (64, 2, 16), 'h64-b272': (64, 2, 272), 'h512x4-b64': (512, 4, 64), 'h1024-b16': (1024, 2, 16)}
LN_REPS = {'h64-b16': ((0, 0), (1, 1), (0, 1)), 'h64-b272': ((1, 1), (0, 0), (1, 0)), 'h512x4-b64': ((0, 1), (1, 0), (1, 1)),
           'h1024-b16': ((1, 0), (0, 1), (0, 0))}


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_cfgrl_group_equals_standalone_twins_device_rng(shape, K):
    """3 fused updates; after each: the 4 infos, and read_rows() - idx, goal_idx, do_cfg, the six raw draws and the goal columns of the
    assembled rows - of every member against its twin; then parameters, both Adam moments and the counters."""
    H, nh, B = SHAPES[shape]
    ln, reps = LN_REPS[shape][K - 1]
    ds, group, twins = _setup(K, _cfg(H, B, nh, actor_layer_norm=bool(ln)), reps=bool(reps))
    dropped = 0
    for step in range(3):
        infos, want = _step(group, twins, B, want_info=True)
        _assert_infos(infos, want, f'step {step}')
        for i, (m, t) in enumerate(zip(group.members, twins)):
            r = _assert_rows(m, t, f'step {step} member {i}')
            dropped += int(r['do_cfg'].sum())
            assert r['idx'].min() >= 0 and r['idx'].max() < len(ds['terminals'])
    if B == 272:
        print('dropped rows', dropped)
        assert dropped > 0   # (p = 0.1 over 816 K rows: the embedding gradient had rows to sum)
    _check(group, twins, shape)
    for m in group.members:
        assert m.get_opt_state()['count'] == 3
    group.close()


# ---- 2. mask extremes -------------------------------------------------------------------------------------------------------------------
def test_cfgrl_group_mask_extremes_with_an_explicit_mask():
    """do_cfg [K, B]: member 0 drops no row, member 1 every row, member 2 some - as a host array and as a CUDA tensor.  Each matches its
    twin given the same mask.  On member 0 the unc_embed row never moves and both its Adam moments stay exactly zero: mu = 0.1 g after
    the first step, so a zero mu is a zero gradient."""
    import torch
    K, B = 3, 64
    ds, group, twins = _setup(K, _cfg(64, B))
    rng = np.random.default_rng(5)
    emb0 = leaf_dict(group.members[0].get_params())[EMB].copy()
    assert np.abs(emb0).max() > 0
    for step in range(4):
        mask = np.zeros((K, B), bool)
        mask[1] = True
        mask[2] = rng.random(B) < 0.25
        mask[2, 0], mask[2, 1] = True, False
        infos = group.update_from_dataset(do_cfg=torch.from_numpy(mask).cuda() if step % 2 else mask, want_info=True)
        want = [t.update_from_dataset(B, do_cfg=mask[i], want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, f'step {step}')
        for i, (m, t) in enumerate(zip(group.members, twins)):
            r = _assert_rows(m, t, f'step {step} member {i}')
            np.testing.assert_array_equal(r['do_cfg'], mask[i])
            assert not r['draws']['mask'].any()   # an explicit mask: no mask draw
        m0 = group.members[0]
        opt = m0.get_opt_state()
        np.testing.assert_array_equal(leaf_dict(m0.get_params())[EMB], emb0)
        assert not leaf_dict(opt['mu'])[EMB].any() and not leaf_dict(opt['nu'])[EMB].any(), step
        assert leaf_dict(group.members[1].get_opt_state()['mu'])[EMB].any()
    _check(group, twins)
    with pytest.raises(ValueError):
        group.update_from_dataset(do_cfg=np.zeros((K, B + 1), bool))
    group.close()


# ---- 3. goal mixtures -------------------------------------------------------------------------------------------------------------------
def test_cfgrl_group_members_draw_goals_with_their_own_mixture():
    """Three members with ONE create seed and one set of parameters, mixtures (1, 0, 0), (0, .5, .5) and (.2, .5, .3): the index draw
    and the raw goal draws of members 1 and 2 coincide, so goal indices that differ come from the thresholds each member's CfgrlSrc
    carries.  Member 0 takes the all_cur path: no goal draw, goal = idx.  Every member's goal_idx and draws equal its twin's and the host
    restatement of GCDataset.sample_goals on the member's own draws."""
    K, B = 3, 256
    ds, group, twins = _setup(K, _cfg(64, B), mixes=MIXES, seeds=[5, 5, 5], same_params=True)
    differ = 0
    for step in range(4):
        _step(group, twins, B)
        rows = [_assert_rows(m, t, f'step {step} member {i}') for i, (m, t) in enumerate(zip(group.members, twins))]
        for i, r in enumerate(rows):
            np.testing.assert_array_equal(r['goal_idx'], CO.sample_goals(r['idx'], ds['terminals'], r['draws'], *MIXES[i]), err_msg=f'member {i}')
        np.testing.assert_array_equal(rows[0]['goal_idx'], rows[0]['idx'])
        for k in ('random', 'dist', 'traj', 'cur'):
            assert not rows[0]['draws'][k].any(), k
            np.testing.assert_array_equal(rows[1]['draws'][k], rows[2]['draws'][k])
            assert rows[1]['draws'][k].any()
        np.testing.assert_array_equal(rows[1]['idx'], rows[2]['idx'])
        differ += int((rows[1]['goal_idx'] != rows[2]['goal_idx']).sum())
    assert differ > 0
    _check(group, twins)
    group.close()


# ---- 4. explicit rows, infos through the C ABI ---------------------------------------------------------------------------------------------
def test_cfgrl_group_explicit_rows_host_and_device():
    """idxs [K, B] as a host array (the group's own stream) and as a CUDA tensor (torch's current stream), alternating with no
    synchronize, once with an explicit mask beside them; every member's rows include N - 1."""
    import torch
    K, B = 3, 64
    ds, group, twins = _setup(K, _cfg(64, B), reps=True)
    rng = np.random.default_rng(13)
    N = len(ds['terminals'])
    for step in range(5):
        idxs = rng.integers(0, N, size=(K, B))
        idxs[:, step % B] = N - 1
        mask = (rng.random((K, B)) < 0.3) if step == 3 else None
        infos = group.update_from_dataset(idxs=torch.from_numpy(idxs).cuda() if step % 2 == 0 else idxs, do_cfg=mask, want_info=True)
        want = [t.update_from_dataset(B, idxs=idxs[i], do_cfg=None if mask is None else mask[i], want_info=True)[1] for i, t in enumerate(twins)]
        _assert_infos(infos, want, f'step {step}')
        for i, (m, t) in enumerate(zip(group.members, twins)):
            r = _assert_rows(m, t, f'step {step} member {i}')
            np.testing.assert_array_equal(r['idx'], idxs[i])
            assert not r['draws']['idx'].any()
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.zeros((K + 1, B), np.int64))
    with pytest.raises(ValueError):
        group.update_from_dataset(idxs=np.full((K, B), N, np.int64))
    _check(group, twins)
    group.close()


def test_cfgrl_group_infos_through_the_c_abi():
    """A host buffer (synchronous) and a device buffer (read after the group's synchronize) hold every member's 4 infos in
    fql_read_info_n's layout."""
    import torch
    from fql_amd.cfgrl import CFGRL_INFO_KEYS
    K, B = 2, 64
    ds, group, twins = _setup(K, _cfg(64, B))
    lib = group._lib
    for step in range(4):
        if step % 2 == 0:
            host = np.full((K, 4), np.nan, np.float32)
            group._check(lib.fql_cfgrl_group_update_from_dataset(group._g, None, B, None, host.ctypes.data, None))
            got = host
        else:
            dev = torch.full((K, 4), float('nan'), dtype=torch.float32, device='cuda')
            torch.cuda.synchronize()    # the fill ran on torch's stream, the update runs on the group's own
            group._check(lib.fql_cfgrl_group_update_from_dataset(group._g, None, B, None, dev.data_ptr(), None))
            group.synchronize()
            got = dev.cpu().numpy()
        for i, (m, t) in enumerate(zip(group.members, twins)):
            t.update_from_dataset(B)
            want = t.read_info()
            assert got[i].tolist() == [want[k] for k in CFGRL_INFO_KEYS], (step, i)
            assert got[i].tolist() == list(m.read_info().values()), (step, i)
            assert np.isfinite(got[i]).all() and got[i, 0] > 0
    _check(group, twins)
    group.close()


# ---- 5. member work between group updates ---------------------------------------------------------------------------------------------
def test_cfgrl_group_member_work_between_group_updates(tmp_path):
    """Between group updates, with no synchronize: a member's own update_from_dataset, policy_loss (the probe shares the input rows with
    the update), sample_actions, set_params, and a checkpoint saved, the member overwritten, and the checkpoint restored into it.  The
    same calls go to the twins one at a time; the next group update continues bitwise as the twin's sequence does."""
    from fql_amd import checkpoint
    K, B = 3, 64
    ds, group, twins = _setup(K, _cfg(64, B, flow_steps=2))
    rng = np.random.default_rng(2)
    rows = rng.integers(0, len(ds['terminals']), size=B)
    batch = {'observations': ds['observations'][rows], 'actions': ds['actions'][rows], 'actor_goals': ds['observations'][rows[::-1]]}
    noise, mask = CO.make_noise(B, AD, 9), rng.random(B) < 0.2
    obs, goals, z = (rng.standard_normal((10, d)).astype(np.float32) for d in (OD, OD, AD))
    seen = {}

    def sequence(update_all, agents, tag):
        out = []
        for rnd in range(2):
            update_all()
            agents[0].update_from_dataset(B)                                       # the member's own update
            update_all()
            out.append(agents[1].policy_loss(batch, noise=noise, do_cfg=mask)[0])
            out.append(agents[2].read_rows()['goal_idx'])                          # probe = 0: the last update's rows, a group update's here
            update_all()
            out.append(agents[0].sample_actions(obs, goals, noises=z, cfg=2.0))
            out.append(agents[1].sample_actions(obs, goals, seed=4))
            update_all()
            p = _randomized(agents[1].get_params(), 60 + rnd, scale=0.05)
            agents[1].set_params(p)
            update_all()
            d = tmp_path / f'{tag}{rnd}'
            d.mkdir()
            checkpoint.save_agent(agents[2], str(d), rnd)
            agents[2].set_params(_randomized(agents[2].get_params(), 70 + rnd))    # overwritten, then restored
            checkpoint.restore_agent(agents[2], str(d), rnd)
            update_all()
        seen[tag] = out

    sequence(lambda: group.update_from_dataset(), group.members, 'group')
    sequence(lambda: [t.update_from_dataset(B) for t in twins], twins, 'twins')
    assert len(seen['group']) == len(seen['twins']) == 8
    for a, b in zip(seen['group'], seen['twins']):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    _check(group, twins)
    assert [m.get_opt_state()['count'] for m in group.members] == [14, 12, 12]
    group.close()


def test_cfgrl_group_members_checkpoint_as_standalone_agents(tmp_path):
    """A grouped member's checkpoint restored into a fresh agent: its own next update equals the group's for that member."""
    import fql_amd
    from fql_amd import checkpoint
    K, B = 2, 64
    cfg = _cfg(64, B)
    ds, group, twins = _setup(K, cfg)
    for _ in range(3):
        _step(group, twins, B)
    checkpoint.save_agent(group.members[1], str(tmp_path), 3)
    b = fql_amd.CFGRLAgent.create(4, _example(OD, AD, OD), dict(cfg, cfg=2.5, actor_p_curgoal=MIXES[2][0], actor_p_trajgoal=MIXES[2][1],
                                                               actor_p_randomgoal=MIXES[2][2]))   # member 1's seed, cfg and mixture
    checkpoint.restore_agent(b, str(tmp_path), 3)
    b.upload_dataset(ds)
    _step(group, twins, B)
    b.update_from_dataset(B)
    group.synchronize()
    assert_same_state(group.members[1], b)
    _check(group, twins)
    group.close()


# ---- 6. sampling ----------------------------------------------------------------------------------------------------------------------
def _sampler_group(K, H, od, ad, gd, nh=2):
    """A group whose members carry parameters of their own (and so an unc_embed row of their own), flow_steps 2."""
    import fql_amd
    cfg = _cfg(H, 16, nh, flow_steps=2)
    group = fql_amd.CFGRLAgentGroup.create([3 + i for i in range(K)], _example(od, ad, gd), cfg, cfgs=[1.5 + i for i in range(K)])
    for i, m in enumerate(group.members):
        m.set_params(_randomized(m.get_params(), 80 + i, scale=0.3))
    return group


@pytest.mark.parametrize('K, H, od, ad, gd, ns', [(2, 64, OD, AD, OD, (1, 32, 17, 2049)), (3, 64, OD, AD, 2, (1, 17, 2049)), (2, 512, 21, 17, 21, (1, 17))],
                         ids=['K2-H64', 'K3-H64-goal2', 'K2-H512-act17'])
def test_cfgrl_group_sample_actions_equal_the_members_own(K, H, od, ad, gd, ns):
    """n = 1; n = 17 (n_pad 32: 15 dead rows in either half, here once straight after a call that filled all 32); n = 2049 (one row into
    a second chunk per member); act 17 pads to 32 columns.  cfg as None, a scalar, [K] and [K, n]; observations and goals per member,
    as one shared block, and one [G] goal; explicit noises, one seed, K seeds and no seed.  Every slice is bitwise the member's own
    sample_actions_rows (scalar weights: its sample_actions)."""
    import torch
    group = _sampler_group(K, H, od, ad, gd)
    ms = group.members
    defaults = [float(m.config['cfg']) for m in ms]
    assert defaults == [1.5 + i for i in range(K)]
    before = [leaf_dict(m.get_params()) for m in ms]
    for i in range(K):
        for j in range(i):
            assert not np.array_equal(before[i][EMB], before[j][EMB])
    rng = np.random.default_rng(17)
    side = torch.cuda.Stream()
    for n in ns:
        obs = rng.standard_normal((K, n, od)).astype(np.float32)
        gl = rng.standard_normal((K, n, gd)).astype(np.float32)
        z = rng.standard_normal((K, n, ad)).astype(np.float32)
        got = group.sample_actions(obs, gl, noises=z)    # cfg None: each member's configured default
        assert got.shape == (K, n, ad) and np.abs(got).max() <= 1.0 and np.abs(got).max() > 0
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], gl[i], noises=z[i]).reshape(n, ad), err_msg=f'n {n} default member {i}')
            np.testing.assert_array_equal(got[i], ms[i].sample_actions_rows(obs[i], gl[i], np.full(n, defaults[i], np.float32), noises=z[i]))
        for cfg_w in (0.0, 3.0):    # a scalar; 0: the unconditional half alone, each member's own unc_embed row
            got = group.sample_actions(obs, gl, noises=z, cfg=cfg_w)
            for i in range(K):
                np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], gl[i], noises=z[i], cfg=cfg_w).reshape(n, ad), err_msg=f'n {n} cfg {cfg_w} member {i}')
        per_member = [0.0, 1.5, 3.0][:K]
        got = group.sample_actions(obs, gl, noises=z, cfg=per_member)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], gl[i], noises=z[i], cfg=per_member[i]).reshape(n, ad), err_msg=f'n {n} per member {i}')
        per_row = rng.uniform(0.0, 5.0, size=(K, n)).astype(np.float32)
        per_row[:, 0] = 0.0
        got = group.sample_actions(obs, gl, noises=z, cfg=per_row)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions_rows(obs[i], gl[i], per_row[i], noises=z[i]), err_msg=f'n {n} per row member {i}')
            for j in sorted({0, n // 2, n - 1}):   # row j at its own weight is the member's scalar call
                np.testing.assert_array_equal(got[i, j], ms[i].sample_actions(obs[i, j], gl[i, j], noises=z[i, j], cfg=float(per_row[i, j])))
        if n == 2049:
            continue
        seeds = [50 + n + i for i in range(K)]
        got = group.sample_actions(obs, gl, seed=seeds, cfg=3.0)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions(obs[i], gl[i], seed=seeds[i], cfg=3.0).reshape(n, ad), err_msg=f'n {n} seeds member {i}')
        got = group.sample_actions(obs, gl, seed=9, cfg=per_row)
        for i in range(K):
            np.testing.assert_array_equal(got[i], ms[i].sample_actions_rows(obs[i], gl[i], per_row[i], seed=9), err_msg=f'n {n} one seed member {i}')
        # no seed: member i's counter advances once, and the draw is keyed as its own unseeded call would key it
        calls = [m._sample_calls for m in ms]
        got = group.sample_actions(obs, gl)
        assert [m._sample_calls for m in ms] == [c + 1 for c in calls]
        for i, m in enumerate(ms):
            key = ((m._seed << 20) ^ m._sample_calls) & 0xFFFFFFFFFFFFFFFF
            np.testing.assert_array_equal(got[i], m.sample_actions(obs[i], gl[i], seed=key).reshape(n, ad), err_msg=f'n {n} unseeded member {i}')
        assert np.abs(got - group.sample_actions(obs, gl)).max() > 0
        # one shared block of rows and goals against the same rows tiled; one [G] goal against that goal repeated
        shared = group.sample_actions(obs[0], gl[0], seed=seeds, cfg=per_member)
        np.testing.assert_array_equal(shared, group.sample_actions(np.tile(obs[:1], (K, 1, 1)), np.tile(gl[:1], (K, 1, 1)), seed=seeds, cfg=per_member))
        one = group.sample_actions(obs, gl[0, 0], seed=seeds)
        for i in range(K):
            np.testing.assert_array_equal(shared[i], ms[i].sample_actions(obs[0], gl[0], seed=seeds[i], cfg=per_member[i]).reshape(n, ad))
            np.testing.assert_array_equal(one[i], ms[i].sample_actions(obs[i], gl[0, 0], seed=seeds[i]).reshape(n, ad))
        # CUDA tensors on a side stream, the weights on the device too
        with torch.cuda.stream(side):
            to, tg_, tz, tw = (torch.from_numpy(x).cuda() for x in (obs, gl, z, per_row))
            tg = group.sample_actions(to, tg_, noises=tz, cfg=tw)
            assert tg.is_cuda and tuple(tg.shape) == (K, n, ad)
            want = [ms[i].sample_actions_rows(to[i], tg_[i], tw[i], noises=tz[i]) for i in range(K)]
        side.synchronize()
        for i in range(K):
            np.testing.assert_array_equal(tg[i].cpu().numpy(), want[i].cpu().numpy(), err_msg=f'n {n} cuda member {i}')
            np.testing.assert_array_equal(tg[i].cpu().numpy(), ms[i].sample_actions_rows(obs[i], gl[i], per_row[i], noises=z[i]))
    o7, g7 = rng.standard_normal((K, 7, od)).astype(np.float32), rng.standard_normal((K, 7, gd)).astype(np.float32)
    calls = [m._sample_calls for m in ms]
    with pytest.raises(ValueError):
        group.sample_actions(o7, g7, cfg=float('inf'))
    with pytest.raises(ValueError):
        group.sample_actions(o7, None)
    with pytest.raises(ValueError):
        group.sample_actions(o7, g7[:, :6])
    assert [m._sample_calls for m in ms] == calls
    from fql_amd import _cabi
    w = np.ones((K, 7), np.float32)
    out, seeds = np.zeros((K, 7, ad), np.float32), (C.c_uint64 * K)(*range(K))
    assert group._lib.fql_cfgrl_group_sample_actions(group._g, o7.ctypes.data, None, 7, None, seeds, w.ctypes.data, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'goals' in group._lib.fql_last_error(None)
    w[K - 1, 3] = np.nan   # past the Python check: the library refuses a non-finite host weight itself
    assert group._lib.fql_cfgrl_group_sample_actions(group._g, o7.ctypes.data, g7.ctypes.data, 7, None, seeds, w.ctypes.data, out.ctypes.data, None) == _cabi.FQL_E_INVALID
    assert b'finite' in group._lib.fql_last_error(None)
    assert not out.any()
    # no state change
    group.synchronize()
    for i, m in enumerate(ms):
        after = leaf_dict(m.get_params())
        for k in after:
            np.testing.assert_array_equal(after[k], before[i][k], err_msg=f'member {i} {k}')
        assert m.get_opt_state()['count'] == 0
    group.close()


def test_cfgrl_group_sampling_sees_group_updates_without_a_synchronize():
    K, B = 2, 64
    ds, group, twins = _setup(K, _cfg(64, B, flow_steps=2))
    rng = np.random.default_rng(4)
    obs, gl = rng.standard_normal((K, 10, OD)).astype(np.float32), rng.standard_normal((K, 10, OD)).astype(np.float32)
    for rnd in range(3):
        for _ in range(2):
            _step(group, twins, B)
        got = group.sample_actions(obs, gl, seed=21 + rnd)
        for i in range(K):
            np.testing.assert_array_equal(got[i], twins[i].sample_actions(obs[i], gl[i], seed=21 + rnd), err_msg=f'round {rnd} member {i}')
    _check(group, twins)
    group.close()


# ---- 7. launch counts -----------------------------------------------------------------------------------------------------------------
def test_cfgrl_group_launch_counts_do_not_depend_on_k():
    """The fused program has a member's launch count, whatever K; a fused sampling chunk costs what the member's sweep call does:
    3 + S (hidden layers + head) + 1 at the default shape (hidden 512 x 4, flow_steps 16)."""
    import fql_amd
    counts = set()
    for K in (1, 2, 4):
        group = fql_amd.CFGRLAgentGroup.create(list(range(K)), _example(OD, AD, OD), _cfg(512, 256, 4), cfgs=[1.0 + i for i in range(K)])
        la = group.launches()
        assert la[0] == group.members[0].cfgrl_stats()[0], K
        assert la[1] == group.members[0].sample_cfgs_stats(), K
        assert la == (group.members[K - 1].cfgrl_stats()[0], group.members[K - 1].sample_cfgs_stats()), K
        counts.add(la)
        group.close()
        for x in group.members:
            x.close()
    assert len(counts) == 1 and next(iter(counts))[1] == 3 + 16 * 5 + 1, counts


# ---- 8. refusals and release ----------------------------------------------------------------------------------------------------------
def test_cfgrl_group_refusals_and_release():
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    B = 64
    cfg = _cfg(64, B)
    ds = _dataset(False)
    ex = _example(OD, AD, OD)
    ex_o, ex_a = ex['observations'], ex['actions']

    def create(members, fn=lib.fql_cfgrl_group_create):
        arr = (C.c_void_p * len(members))(*[a._h for a in members])
        g = C.c_void_p(123)
        return fn(arr, len(members), C.byref(g)), g

    def cfgrl(seed, example=ex, **kw):
        return fql_amd.CFGRLAgent.create(seed, example, dict(cfg, **kw))

    a, twin_a = cfgrl(0), cfgrl(0)
    fq_cfg = fql_amd.get_config()
    fq_cfg.update(actor_hidden_dims=(64,) * 4, value_hidden_dims=(64,) * 4, batch_size=B)
    f0, f1 = fql_amd.FQLAgent.create(0, ex_o, ex_a, fq_cfg), fql_amd.FQLAgent.create(1, ex_o, ex_a, fq_cfg)
    others = {}
    for name, mod, cls in (('rebrac', fql_amd.rebrac, fql_amd.ReBRACAgent), ('iqld', fql_amd.iql_diffusion, fql_amd.IQLDiffusionAgent),
                           ('ifql', fql_amd.ifql, fql_amd.IFQLAgent), ('iql', fql_amd.iql, fql_amd.IQLAgent)):
        c = mod.get_config()
        c.update(batch_size=B, **{k: (64,) * 4 for k in c if k.endswith('hidden_dims')})
        others[name] = cls.create(0, ex_o, ex_a, c)
    for other in [f0] + list(others.values()):    # another kind's handle
        rc, g = create([a, other])
        assert rc == _cabi.FQL_E_STATE and not g.value and b'CFGRL' in lib.fql_last_error(None), lib.fql_last_error(None)
    bad = dict(flow_steps=cfgrl(1, flow_steps=8), goal_dim=cfgrl(2, example=_example(OD, AD, 2)), hidden=cfgrl(3, actor_hidden_dims=(128, 128)),
               lr=cfgrl(4, lr=1e-4), layer_norm=cfgrl(5, actor_layer_norm=True), batch=cfgrl(6, batch_size=32))
    for what, x in bad.items():
        rc, g = create([a, x])
        assert rc == _cabi.FQL_E_INVALID and not g.value, (what, lib.fql_last_error(None))
        assert b'member 1' in lib.fql_last_error(None), what
        if what != 'batch':
            assert b'cfg / actor_p_curgoal / actor_p_trajgoal / actor_p_randomgoal' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert create([a, a])[0] == _cabi.FQL_E_INVALID and b'twice' in lib.fql_last_error(None)
    # the other kinds' creates keep refusing CFGRL handles, and name the call that takes them
    for fn in (lib.fql_group_create, lib.fql_rebrac_group_create, lib.fql_iqld_group_create, lib.fql_ifql_group_create, lib.fql_iql_group_create):
        rc, g = create([a, cfgrl(9)], fn=fn)
        assert rc == _cabi.FQL_E_STATE and not g.value and b'fql_cfgrl_group_create' in lib.fql_last_error(None), lib.fql_last_error(None)
    mix = dict(cfg=5.0, actor_p_curgoal=0.2, actor_p_trajgoal=0.5, actor_p_randomgoal=0.3)   # what may differ
    b, twin_b = cfgrl(5, **mix), cfgrl(5, **mix)
    rc, g = create([a, b])
    assert rc == _cabi.FQL_OK and g.value, lib.fql_last_error(None)
    assert create([b])[0] == _cabi.FQL_E_INVALID and b'already' in lib.fql_last_error(None)
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_E_STATE
    assert lib.fql_destroy(b._h) == _cabi.FQL_E_STATE
    # every other kind's group call on a CFGRL group names the call that serves it
    o, out = np.zeros((2, 1, OD), np.float32), np.zeros((2, 1, AD), np.float32)
    gl, z, w = np.zeros((2, 1, OD), np.float32), np.zeros((2, 1, AD), np.float32), np.ones((2, 1), np.float32)
    seeds, v, la = (C.c_uint64 * 2)(1, 2), C.c_int64(-1), (C.c_int64 * 4)(-1, -1, -1, -1)
    op, zp, outp = o.ctypes.data, z.ctypes.data, out.ctypes.data
    for rc in (lib.fql_group_update_from_dataset(g, None, B, None, None),
               lib.fql_group_sample_actions(g, op, 1, None, seeds, outp, None),
               lib.fql_group_flow_actions(g, op, zp, 1, outp, None),
               lib.fql_group_sample_stats(g, 0, C.byref(v)),
               lib.fql_rebrac_group_update_from_dataset(g, None, B, 1, None, None),
               lib.fql_rebrac_group_sample_actions(g, op, 1, None, seeds, 1.0, outp, None),
               lib.fql_rebrac_group_stats(g, C.byref(v), None, None),
               lib.fql_iqld_group_update_from_dataset(g, None, B, 1, 1, None, None),
               lib.fql_iqld_group_sample_actions(g, op, 1, None, seeds, w.ctypes.data, outp, None),
               lib.fql_iqld_group_stats(g, la, C.byref(v)),
               lib.fql_ifql_group_update_from_dataset(g, None, B, None, None),
               lib.fql_ifql_group_sample_actions(g, op, 1, None, seeds, outp, None),
               lib.fql_ifql_group_flow_actions(g, op, zp, 1, outp, None),
               lib.fql_ifql_group_stats(g, C.byref(v), C.byref(v), C.byref(v)),
               lib.fql_iql_group_update_from_dataset(g, None, B, None, None),
               lib.fql_iql_group_sample_actions(g, op, 1, None, seeds, 1.0, outp, None),
               lib.fql_iql_group_stats(g, C.byref(v), C.byref(v))):
        assert rc == _cabi.FQL_E_STATE and b'fql_cfgrl_group_' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert v.value == -1 and list(la) == [-1] * 4 and not out.any()
    # and the CFGRL group calls on every other kind's group
    groups = [(create([f0, f1], fn=lib.fql_group_create), b'fql_group_'), (create([others['rebrac']], fn=lib.fql_rebrac_group_create), b'fql_rebrac_group_'),
              (create([others['iqld']], fn=lib.fql_iqld_group_create), b'fql_iqld_group_'), (create([others['ifql']], fn=lib.fql_ifql_group_create), b'fql_ifql_group_'),
              (create([others['iql']], fn=lib.fql_iql_group_create), b'fql_iql_group_')]
    for (rc, og), name in groups:
        assert rc == _cabi.FQL_OK and og.value, (name, lib.fql_last_error(None))
        for rc in (lib.fql_cfgrl_group_update_from_dataset(og, None, B, None, None, None),
                   lib.fql_cfgrl_group_sample_actions(og, op, gl.ctypes.data, 1, None, seeds, w.ctypes.data, outp, None),
                   lib.fql_cfgrl_group_stats(og, C.byref(v), C.byref(v))):
            assert rc == _cabi.FQL_E_STATE and name in lib.fql_last_error(None), lib.fql_last_error(None)
        assert lib.fql_group_destroy(og) == _cabi.FQL_OK
    assert v.value == -1 and not out.any()
    assert lib.fql_cfgrl_group_update_from_dataset(g, None, 32, None, None, None) == _cabi.FQL_E_INVALID   # another batch size
    # a member without a goal table at update time: none, then member 0 alone has one
    assert lib.fql_cfgrl_group_update_from_dataset(g, None, B, None, None, None) == _cabi.FQL_E_INVALID
    assert b'member 0' in lib.fql_last_error(None) and b'goal table' in lib.fql_last_error(None), lib.fql_last_error(None)
    a.upload_dataset(ds)
    assert lib.fql_cfgrl_group_update_from_dataset(g, None, B, None, None, None) == _cabi.FQL_E_INVALID
    assert b'member 1' in lib.fql_last_error(None) and b'goal table' in lib.fql_last_error(None), lib.fql_last_error(None)
    assert a.get_opt_state()['count'] == 0
    # released: plain handles again, bitwise with their twins through grouped and standalone steps
    for x in (b, twin_a, twin_b):
        x.upload_dataset(ds)
    for _ in range(3):
        assert lib.fql_cfgrl_group_update_from_dataset(g, None, B, None, None, None) == _cabi.FQL_OK, lib.fql_last_error(None)
        for x in (twin_a, twin_b):
            x.update_from_dataset(B)
    assert lib.fql_group_synchronize(g) == _cabi.FQL_OK
    assert lib.fql_group_destroy(g) == _cabi.FQL_OK
    assert lib.fql_set_batch_size(a._h, 32) == _cabi.FQL_OK and lib.fql_set_batch_size(a._h, B) == _cabi.FQL_OK
    for _ in range(2):
        for x in (a, b, twin_a, twin_b):
            x.update_from_dataset(B)
    assert_same_state(a, twin_a)
    assert_same_state(b, twin_b)
    for x in [a, b, twin_a, twin_b, f0, f1] + list(others.values()) + list(bad.values()):
        x.close()


def test_cfgrl_group_close_is_idempotent_and_members_update_alone_afterwards():
    K, B = 2, 64
    ds, group, twins = _setup(K, _cfg(64, B))
    for _ in range(2):
        _step(group, twins, B)
    group.close()
    group.close()    # a no-op
    assert group._g is None
    for m, t in zip(group.members, twins):
        m.update_from_dataset(B)
        t.update_from_dataset(B)
        assert_same_state(m, t)
        assert m.read_info() == t.read_info()
