"""Two builds of the library build and compute the same thing, bit for bit: the equality pass of a host-side refactor.

usage: python experiments/compare_builds.py <library a> <library b> [out dir, default build/compare_builds]

For each library in turn, and one at a time, a fresh child process per job below loads it through FQL_AMD_LIB with FQL_DUMP=1 under its
own `timeout -k 10`, and writes what it read to <out dir>/<a|b>/<job>/: arrays.npz (the fql_debug_plan and fql_debug_task_forms words,
the *_stats counts, the sampler outputs, and after 8 update_from_dataset calls from one seed every parameter leaf, both Adam moments and
the counters) and dump.txt (its stderr: the FQL_DUMP lines of every program the handles build, sampler programs included).  The first
non-zero exit or time-out stops the script.  This process never opens the GPU: it compares the two directories, prints the first
difference and the number of arrays and lines compared, and exits 1 on a difference.

Jobs: `kinds`: FQL, IFQL, ReBRAC, SAC with and without tanh_squash, IQL ddpgbc and awr with const_std and with the log_stds leaf, BC,
IQL-diffusion, CFGRL at hidden 64 x 2, batch 32 (ReBRAC alternates critic-only and full steps, IQL-diffusion runs its four step kinds; one
sample_actions of 5 rows each, cfg 3 and one per-row sweep call for the two CFG kinds).  Around that, what a handle's kind decides on the
host: right after create every parameter leaf, fql_num_info and every fql_handle_info_name; behind the state read-out a total_loss /
policy_loss probe on one fixed batch with explicit noise (loss and infos), one network.select query of 5 rows per module the kind answers
for, the fql_last_error text of a query of a module it does not have and of an update whose explicit noise carries a field it does not
read, and a second sampling call (explicit noises where the first used a seed, and the reverse; temperature 0.5 for ReBRAC, SAC and IQL).
`h512_<precision>`: FQL at hidden 512 x 4, batch 256, then one update_begin_split / update_end_split pair.
`edges_<precision>`: the FQL shapes of tests/test_gpu_batch_edges.py CASES.  `frames`: a 32 x 32 x 3 frames handle in both precisions (no
plan: the read-out refuses visual handles).  `group`: the two members of a K = 2 FQL group at hidden 256 x 4, batch 64.
`group_<kind>` (rebrac, iqld, ifql, iql_ddpgbc, iql_awr, cfgrl, sac): a K = 2 group of that kind at hidden 64 x 2, batch 32, its free fields
differing - launches() and the fused program's task forms; 8 fused updates (ReBRAC alternates its step kinds, IQL-diffusion runs its four,
SAC runs four from the dataset and four balanced over rings of 64 rows); one fused sample_actions of 5 host rows per member with explicit
noises and one with a seed (the CFG kinds: cfg 3 and one per-row weight array; IFQL: compute_flow_actions too); every member's state; the
infos of one more update per update call of the kind, read through the C ABI into a NaN-filled host buffer; and, as uint8, the
fql_last_error text of every other kind's group entry points called on this group and of the creates it refuses (another kind's member,
a member of another structure, a member listed twice, a member already grouped)."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OD, AD, UPDATES = 29, 8, 8
PRECISIONS = ('fp32', 'bf16x3')
# job -> its time limit in seconds (each takes 1 - 3 s on an MI355X; a cold start of the runtime can add several)
JOBS = {'kinds': 30, 'h512_fp32': 30, 'h512_bf16x3': 30, 'edges_fp32': 30, 'edges_bf16x3': 30, 'frames': 20, 'group': 20,
        'group_rebrac': 30, 'group_iqld': 30, 'group_ifql': 30, 'group_iql_ddpgbc': 30, 'group_iql_awr': 30, 'group_cfgrl': 30, 'group_sac': 30}


# ---- child: one job on one library ---------------------------------------------------------------------------------------------------
def flat(tree, prefix):
    for k, v in sorted(tree.items()):
        if isinstance(v, dict):
            yield from flat(v, f'{prefix}/{k}')
        else:
            yield f'{prefix}/{k}', np.asarray(v)


def words(fn, *handles):
    """The int32 words of a diagnostic read-out (size in word 0), or its refusal code."""
    head = np.zeros(1, np.int32)
    rc = fn(*handles, head.ctypes.data, 4)
    if rc != 0:
        return np.array([rc], np.int32)
    w = np.zeros(int(head[0]), np.int32)
    assert fn(*handles, w.ctypes.data, w.nbytes) == 0
    return w


def plan_and_forms(out, tag, agent=None, group=None):
    from fql_amd import _cabi
    lib = _cabi.load()
    lib.fql_debug_plan.argtypes, lib.fql_debug_plan.restype = [C.c_void_p, C.c_void_p, C.c_size_t], C.c_int
    lib.fql_debug_task_forms.argtypes, lib.fql_debug_task_forms.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t], C.c_int
    if agent is not None:
        out[f'{tag}/plan'] = words(lib.fql_debug_plan, agent._h)
    out[f'{tag}/forms'] = words(lib.fql_debug_task_forms, agent._h if agent is not None else None, group._g if group is not None else None)


def state(out, tag, agent):
    agent.synchronize()
    out.update(flat(agent.get_params(), f'{tag}/params'))
    st = agent.get_opt_state()
    out.update(flat(st.pop('mu'), f'{tag}/mu'))
    out.update(flat(st.pop('nu'), f'{tag}/nu'))
    out[f'{tag}/counters'] = np.array([st[k] for k in sorted(st)], np.int64)


def dataset(n, seed=0):
    from fql_amd.synthetic import make_synthetic_dataset
    ds = make_synthetic_dataset(n, OD, AD, seed=seed)
    ds['terminals'][-1] = 1.0
    return ds


def fql_handle(out, tag, B, hidden, precision):
    """One FQL handle: plan, forms, stats, both samplers, UPDATES updates, state.  Returns it for what a job adds."""
    import fql_amd
    cfg = fql_amd.get_config()
    cfg.update(actor_hidden_dims=tuple(hidden), value_hidden_dims=tuple(hidden), alpha=10.0, batch_size=B, precision=precision)
    ds = dataset(max(4 * B, 64), seed=3)
    a = fql_amd.FQLAgent.create(0, ds['observations'][:1], ds['actions'][:1], cfg)
    created(out, tag, a)
    plan_and_forms(out, tag, agent=a)
    out[f'{tag}/stats'] = np.array([v for _, v in sorted(a.stats().items())], np.int64)
    a.upload_dataset(ds)
    z = np.random.default_rng(1).standard_normal((5, AD)).astype(np.float32)
    out[f'{tag}/sample'] = a.sample_actions(ds['observations'][:5], noises=z)
    out[f'{tag}/flow'] = a.compute_flow_actions(ds['observations'][:5], z)
    for _ in range(UPDATES):
        a.update_from_dataset(B)
    state(out, tag, a)
    return a


def loss_noise(kind, B):
    """The explicit noise of one loss probe: the fields the kind reads, from one fixed draw (t on the grid k / 16 for BC and IQL-diffusion)."""
    rng = np.random.default_rng(5)
    n = {k: rng.standard_normal((B, AD)).astype(np.float32) for k in ('eps1', 'x0', 'z', 'eps2')}
    n['t'] = rng.uniform(size=B).astype(np.float32)
    grid = (rng.integers(0, 17, size=B) / 16.0).astype(np.float32)
    return {'fql': n, 'ifql': {k: n[k] for k in ('x0', 't')}, 'rebrac': {'eps1': n['eps1']}, 'sac': {k: n[k] for k in ('eps1', 'eps2')},
            'iql': {'eps': n['eps1']}, 'bc': {'x0': n['x0'], 't': grid}, 'iqld': {'x0': n['x0'], 't': grid},
            'cfgrl': {k: n[k] for k in ('x0', 't')}}[kind]


def created(out, tag, a):
    """Right after create: every parameter leaf (the initialisers), the info count and every info name as bytes."""
    from fql_amd import _cabi
    lib = _cabi.load()
    out.update(flat(a.get_params(), f'{tag}/init'))
    n = lib.fql_num_info(a._h)
    out[f'{tag}/num_info'] = np.array([n], np.int32)
    for i in range(n):
        out[f'{tag}/info_name/{i:02d}'] = np.frombuffer(lib.fql_handle_info_name(a._h, i), np.uint8)


def refusal_text(out, tag, lib, a, rc):
    out[f'{tag}/rc'] = np.array([rc], np.int32)
    out[f'{tag}/text'] = np.frombuffer(lib.fql_last_error(a._h), np.uint8)


def probes(out, tag, a, ds, goals=None):
    """Behind the updates and the state read-out, what the handle's kind decides on the host: a loss probe on one fixed batch with explicit
    noise, one query of every module the kind answers for, the refusal of a module it does not have and of a noise field it does not
    read, and a second sampling call (explicit noises where the first used a seed, and the reverse; temperature 0.5 where the kind has one)."""
    import fql_amd
    from fql_amd import _cabi
    lib = _cabi.load()
    kind, B = tag.split('_')[0], 32
    batch = {k: ds[k][:B] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')}
    batch['next_actions'] = ds['actions'][1:B + 1]
    batch['actor_goals'] = ds['next_observations'][:B]
    noise = loss_noise(kind, B)
    if kind == 'rebrac':
        losses = [(f'loss{f}', a.total_loss(batch, noise=noise, full_update=bool(f))) for f in (1, 0)]
    elif kind == 'bc':
        losses = [('loss', a.policy_loss(batch, noise=noise))]
    elif kind == 'cfgrl':
        losses = [('loss', a.policy_loss(batch, noise=noise, do_cfg=np.arange(B) % 3 == 0))]
    else:
        losses = [('loss', a.total_loss(batch, noise=noise))]
    for name, (loss, info) in losses:
        out[f'{tag}/{name}'] = np.array([loss], np.float32)
        for k, v in info.items():
            out[f'{tag}/{name}/{k}'] = np.asarray(v)
    rng = np.random.default_rng(6)
    obs, act = ds['observations'][:5], ds['actions'][:5]
    z, t = rng.standard_normal((5, AD)).astype(np.float32), rng.uniform(size=5).astype(np.float32)
    for name, family in a._modules.items():
        m = a.network.select(name)
        out[f'{tag}/module/{name}'] = {'pair': lambda: m(obs, actions=act), 'value': lambda: m(obs), 'field_t': lambda: m(obs, act, t),
                                       'field': lambda: m(obs, z)}[family]()
    missing = 'value' if 'value' not in a._modules else 'actor_onestep_flow'
    refusal_text(out, f'{tag}/no_module', lib, a, lib.fql_module_forward(a._h, missing.encode(), None, None, None, 5, None, None))
    if kind in ('rebrac', 'sac', 'iql'):
        out[f'{tag}/sample2'] = a.sample_actions(obs, noises=z, temperature=0.5)
    elif kind == 'ifql':
        out[f'{tag}/sample2'] = a.sample_actions(obs, noises=rng.standard_normal((5, int(a.config['num_samples']), AD)).astype(np.float32))
    elif kind == 'bc':
        out[f'{tag}/sample2'] = a.sample_actions(obs, noises=z)
    elif kind == 'cfgrl':
        out[f'{tag}/sample2'] = a.sample_actions(obs, goals, seed=7, cfg=3.0)
    elif kind == 'iqld':
        out[f'{tag}/sample2'] = a.sample_actions(obs, seed=7, cfg=3.0)
    else:
        out[f'{tag}/sample2'] = a.sample_actions(obs, seed=7)
    if kind != 'fql':   # a field the kind does not read (z is FQL's alone), past the Python layer's own check of the dict
        a._noise_args = lambda noise, B: fql_amd.FQLAgent._noise_args(a, noise, B)
        try:
            a.update_from_dataset(B, noise={'z': rng.standard_normal((B, AD)).astype(np.float32)})
            rc = 0
        except (ValueError, KeyError, _cabi.FqlError) as e:
            rc = {ValueError: _cabi.FQL_E_INVALID, KeyError: _cabi.FQL_E_NOTFOUND}.get(type(e), _cabi.FQL_E_STATE)
        del a._noise_args
        assert rc != 0, tag
        refusal_text(out, f'{tag}/noise_refusal', lib, a, rc)


def job_kinds(out):
    import fql_amd
    import fql_amd.cfgrl
    ds = dataset(256)
    obs, z = ds['observations'][:5], np.random.default_rng(1).standard_normal((5, AD)).astype(np.float32)
    w = np.array([1.0, 1.5, 3.0, 5.0, 3.0], np.float32)
    hid = dict(actor_hidden_dims=(64, 64), value_hidden_dims=(64, 64), hidden_dims=(64, 64), batch_size=32)
    f = fql_handle(out, 'fql', 32, (64, 64), 'fp32')
    probes(out, 'fql', f, dataset(max(4 * 32, 64), seed=3))
    f.close()
    ex = (ds['observations'][:1], ds['actions'][:1])
    iql, sac = fql_amd.iql.get_config(), fql_amd.sac.get_config()
    kinds = [('ifql', fql_amd.IFQLAgent, fql_amd.ifql.get_config(), lambda a: a.stats().values()),
             ('rebrac', fql_amd.ReBRACAgent, fql_amd.rebrac.get_config(), lambda a: a.rebrac_stats(True) + a.rebrac_stats(False)),
             ('sac', fql_amd.SACAgent, sac, lambda a: a.sac_stats()),
             ('sac_nosquash', fql_amd.SACAgent, dict(sac, tanh_squash=False), lambda a: a.sac_stats()),
             ('iql_ddpgbc', fql_amd.IQLAgent, dict(iql, actor_loss='ddpgbc'), lambda a: a.iql_stats()),
             ('iql_awr', fql_amd.IQLAgent, dict(iql, actor_loss='awr'), lambda a: a.iql_stats()),
             ('iql_ddpgbc_logstds', fql_amd.IQLAgent, dict(iql, actor_loss='ddpgbc', const_std=False), lambda a: a.iql_stats()),
             ('iql_awr_logstds', fql_amd.IQLAgent, dict(iql, actor_loss='awr', const_std=False), lambda a: a.iql_stats()),
             ('bc', fql_amd.BCAgent, fql_amd.bc.get_config(), lambda a: a.bc_stats()),
             ('iqld', fql_amd.IQLDiffusionAgent, fql_amd.iql_diffusion.get_config(),
              lambda a: sum((a.iqld_stats(c, p) for c in (1, 0) for p in (1, 0)), ()) + (a.sample_cfgs_stats(),))]
    for tag, cls, cfg, stats in kinds:
        cfg = dict(cfg, **hid)
        a = cls.create(0, *ex, cfg)
        created(out, tag, a)
        plan_and_forms(out, tag, agent=a)
        out[f'{tag}/stats'] = np.array([int(v) for v in stats(a)], np.int64)
        a.upload_dataset(ds)
        if tag == 'iqld':
            out[f'{tag}/sample'] = a.sample_actions(obs, noises=z, cfg=3.0)
            out[f'{tag}/rows'] = a.sample_actions_rows(obs, w, noises=z)
        else:
            out[f'{tag}/sample'] = a.sample_actions(obs, seed=7)
        for i in range(UPDATES):
            if tag == 'rebrac':
                a.update_from_dataset(32, full_update=bool(i % 2))
            elif tag == 'iqld':
                a.update_from_dataset(32, update_critic=i % 4 < 2, update_actor=i % 2 == 0)
            else:
                a.update_from_dataset(32)
        state(out, tag, a)
        probes(out, tag, a, ds)
        a.close()
    goals = ds['next_observations'][:5]
    g = fql_amd.CFGRLAgent.create(0, {'observations': ex[0], 'actions': ex[1], 'value_goals': goals[:1]}, dict(fql_amd.cfgrl.get_config(), **hid))
    created(out, 'cfgrl', g)
    plan_and_forms(out, 'cfgrl', agent=g)
    out['cfgrl/stats'] = np.array(g.cfgrl_stats() + (g.sample_cfgs_stats(),), np.int64)
    g.upload_dataset(ds)
    out['cfgrl/sample'] = g.sample_actions(obs, goals, noises=z, cfg=3.0)
    out['cfgrl/rows'] = g.sample_actions_rows(obs, goals, w, noises=z)
    for _ in range(UPDATES):
        g.update_from_dataset(32)
    state(out, 'cfgrl', g)
    probes(out, 'cfgrl', g, ds, goals)
    g.close()


def job_h512(out, precision):
    import torch
    a = fql_handle(out, 'h512', 256, (512,) * 4, precision)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    a.update_begin_split(s0.cuda_stream, s1.cuda_stream, batch_size=256)
    a.update_end_split(s0.cuda_stream, s1.cuda_stream)
    torch.cuda.synchronize()
    state(out, 'h512/split', a)
    a.close()


def job_edges(out, precision):
    from tests.test_gpu_batch_edges import CASES
    for cid, (B, hidden) in CASES.items():
        fql_handle(out, cid, B, hidden, precision).close()


def job_frames(out):
    import fql_amd
    from fql_amd.synthetic import make_synthetic_frames
    ds = make_synthetic_frames(150, 4, h=32, w=32, c=3, seed=0, episode_len=25)
    for precision in PRECISIONS:
        cfg = fql_amd.get_config()
        cfg.update(encoder='impala_small', actor_hidden_dims=(64, 64), value_hidden_dims=(64, 64), alpha=3.0, batch_size=32, precision=precision)
        a = fql_amd.FQLAgent.create(0, np.zeros((1, 32, 32, 9), np.uint8), ds['actions'][:1], cfg)
        a.upload_dataset(ds, frame_stack=3, p_aug=0.5)
        rng = np.random.default_rng(2)
        out[f'{precision}/sample'] = a.sample_actions(rng.integers(0, 256, size=(5, 32, 32, 9), dtype=np.uint8),
                                                      noises=rng.standard_normal((5, 4)).astype(np.float32))
        for _ in range(UPDATES):
            a.update_from_dataset(32)
        state(out, precision, a)
        a.close()


def job_group(out):
    import fql_amd
    cfg = fql_amd.get_config()
    cfg.update(actor_hidden_dims=(256,) * 4, value_hidden_dims=(256,) * 4, batch_size=64)
    ds = dataset(256, seed=3)
    g = fql_amd.FQLAgentGroup.create([0, 1], ds['observations'][:1], ds['actions'][:1], cfg, alphas=[3.0, 30.0])
    plan_and_forms(out, 'group', group=g)
    g.upload_dataset(ds)
    for _ in range(UPDATES):
        g.update_from_dataset()
    g.synchronize()
    for i, m in enumerate(g.members):
        state(out, f'member{i}', m)
    g.close()


# every group entry point but the creates, with arguments its kind check never reads: (name, arguments behind the group handle)
GROUP_CALLS = {
    'fql': [('fql_group_update_from_dataset', (None, 32, None, None)), ('fql_group_sample_actions', (None, 1, None, None, None, None)),
            ('fql_group_flow_actions', (None, None, 1, None, None)), ('fql_group_sample_stats', (0, None))],
    'rebrac': [('fql_rebrac_group_update_from_dataset', (None, 32, 1, None, None)),
               ('fql_rebrac_group_sample_actions', (None, 1, None, None, 1.0, None, None)), ('fql_rebrac_group_stats', (None, None, None))],
    'iqld': [('fql_iqld_group_update_from_dataset', (None, 32, 1, 1, None, None)),
             ('fql_iqld_group_sample_actions', (None, 1, None, None, None, None, None)), ('fql_iqld_group_stats', (None, None))],
    'ifql': [('fql_ifql_group_update_from_dataset', (None, 32, None, None)), ('fql_ifql_group_sample_actions', (None, 1, None, None, None, None)),
             ('fql_ifql_group_flow_actions', (None, None, 1, None, None)), ('fql_ifql_group_stats', (None, None, None))],
    'iql': [('fql_iql_group_update_from_dataset', (None, 32, None, None)), ('fql_iql_group_sample_actions', (None, 1, None, None, 1.0, None, None)),
            ('fql_iql_group_stats', (None, None))],
    'cfgrl': [('fql_cfgrl_group_update_from_dataset', (None, 32, None, None, None)),
              ('fql_cfgrl_group_sample_actions', (None, None, 1, None, None, None, None, None)), ('fql_cfgrl_group_stats', (None, None))],
    'sac': [('fql_sac_group_update_from_dataset', (None, 32, None, None)), ('fql_sac_group_update_balanced', (None, None, 32, None, None)),
            ('fql_sac_group_sample_actions', (None, 1, None, None, 1.0, None, None)), ('fql_sac_group_stats', (None, None))],
}


def refusal(out, tag, lib, rc):
    """The code and the full fql_last_error text of a refused group call, as uint8."""
    assert rc != 0, tag
    out[f'{tag}/rc'] = np.array([rc], np.int32)
    out[f'{tag}/text'] = np.frombuffer(lib.fql_last_error(None), np.uint8)


def job_group_kind(out, job):
    """A K = 2 group of one kind at hidden 64 x 2, batch 32, its free fields differing: launches and task forms, 8 fused updates, fused
    sampling with explicit noises and with a seed, every member's state, and what the library says to every other kind's group calls on
    this group and to the creates it refuses."""
    import fql_amd
    import fql_amd.cfgrl
    from fql_amd import _cabi
    kind = job.split('_')[0]
    ds = dataset(256, seed=3)
    ex = (ds['observations'][:1], ds['actions'][:1])
    gex = ({'observations': ex[0], 'actions': ex[1], 'value_goals': ds['next_observations'][:1]},)
    hid = dict(actor_hidden_dims=(64, 64), value_hidden_dims=(64, 64), hidden_dims=(64, 64), batch_size=32)
    mod, cls, member, create_fn, sweep, example = {
        'rebrac': (fql_amd.rebrac, fql_amd.ReBRACAgentGroup, fql_amd.ReBRACAgent, 'fql_rebrac_group_create', dict(alpha_actors=[0.01, 0.1], alpha_critics=[0.0, 0.01]), ex),
        'iqld': (fql_amd.iql_diffusion, fql_amd.IQLDiffusionAgentGroup, fql_amd.IQLDiffusionAgent, 'fql_iqld_group_create',
                 dict(awr_temperatures=[1.0, 3.0], softmax_betas=[1.0, 10.0]), ex),
        'ifql': (fql_amd.ifql, fql_amd.IFQLAgentGroup, fql_amd.IFQLAgent, 'fql_ifql_group_create', dict(expectiles=[0.7, 0.9]), ex),
        'iql': (fql_amd.iql, fql_amd.IQLAgentGroup, fql_amd.IQLAgent, 'fql_iql_group_create', dict(expectiles=[0.7, 0.9], alphas=[1.0, 10.0]), ex),
        'cfgrl': (fql_amd.cfgrl, fql_amd.CFGRLAgentGroup, fql_amd.CFGRLAgent, 'fql_cfgrl_group_create',
                  dict(cfgs=[1.5, 3.0], goal_mixes=[(0.0, 1.0, 0.0), (0.2, 0.5, 0.3)]), gex),
        'sac': (fql_amd.sac, fql_amd.SACAgentGroup, fql_amd.SACAgent, 'fql_sac_group_create', dict(target_entropies=[-4.0, None]), ex),
    }[kind]
    cfg = dict(mod.get_config(), **hid)
    if kind == 'iql':
        cfg['actor_loss'] = job.split('_')[1]
    g = cls.create([0, 1], *example, cfg, **sweep)
    out['launches'] = np.array(g.launches(), np.int64)
    plan_and_forms(out, 'group', group=g)
    g.upload_dataset(ds)
    if kind == 'sac':
        g.create_replay_buffers(64)
        for j in range(64):
            g.add_transitions([{k: ds[k][(j + 64 * i) % 256] for k in ('observations', 'actions', 'rewards', 'masks', 'next_observations')} for i in range(2)])
    for i in range(UPDATES):
        if kind == 'rebrac':
            g.update_from_dataset(full_update=bool(i % 2))
        elif kind == 'iqld':
            g.update_from_dataset(update_critic=i % 4 < 2, update_actor=i % 2 == 0)
        elif kind == 'sac' and i >= UPDATES // 2:
            g.update_balanced()
        else:
            g.update_from_dataset()
    g.synchronize()
    rng = np.random.default_rng(1)
    obs = np.stack([ds['observations'][:5], ds['observations'][5:10]])
    z = rng.standard_normal((2, 5, AD)).astype(np.float32)
    if kind in ('iqld', 'cfgrl'):
        goals = (np.stack([ds['next_observations'][:5], ds['next_observations'][5:10]]),) if kind == 'cfgrl' else ()
        w = np.array([[1.0, 1.5, 3.0, 5.0, 3.0], [0.0, 3.0, 1.0, 2.5, 7.0]], np.float32)
        out['sample'] = g.sample_actions(obs, *goals, noises=z, cfg=3.0)
        out['sample_rows'] = g.sample_actions(obs, *goals, noises=z, cfg=w)
        out['sample_seed'] = g.sample_actions(obs, *goals, seed=7, cfg=3.0)
    elif kind == 'ifql':
        N = int(cfg['num_samples'])
        out['sample'] = g.sample_actions(obs, noises=rng.standard_normal((2, 5, N, AD)).astype(np.float32))
        out['sample_seed'] = g.sample_actions(obs, seed=7)
        out['flow'] = g.compute_flow_actions(obs, z)
    else:
        out['sample'] = g.sample_actions(obs, noises=z)
        out['sample_seed'] = g.sample_actions(obs, seed=7)
    for i, m in enumerate(g.members):
        state(out, f'member{i}', m)
    # one more fused update per update call of the kind, through the C ABI into a NaN-filled host buffer: the infos' stride and extent
    lib = _cabi.load()
    for fn, args in [c for c in GROUP_CALLS[kind] if 'update' in c[0]]:
        infos = np.full(64, np.nan, np.float32)
        assert getattr(lib, fn)(g._g, *args[:-2], infos.ctypes.data, None) == 0, lib.fql_last_error(None)
        out[f'infos/{fn}'] = infos
    # every other kind's group calls on this group
    for other, calls in GROUP_CALLS.items():
        for fn, args in calls if other != kind else ():
            refusal(out, f'on_this_group/{fn}', lib, getattr(lib, fn)(g._g, *args))
    # the creates this kind refuses: another kind's member (an FQL agent; a CFGRL agent), a member of another structure, a member twice, a
    # member already grouped
    create = getattr(lib, create_fn)
    fresh = [member.create(2 + i, *example, c) for i, c in enumerate((cfg, dict(cfg, discount=0.9)))]
    strangers = [fql_amd.FQLAgent.create(4, *ex, dict(fql_amd.get_config(), **hid))]
    if kind != 'cfgrl':
        strangers.append(fql_amd.CFGRLAgent.create(5, *gex, dict(fql_amd.cfgrl.get_config(), **hid)))
    refused = [(f'stranger{i}', [fresh[0], s]) for i, s in enumerate(strangers)]
    refused += [('structure', fresh), ('twice', [fresh[0], fresh[0]]), ('grouped', [fresh[0], g.members[0]])]
    for tag, members in refused:
        h = C.c_void_p()
        refusal(out, f'create/{tag}', lib, create((C.c_void_p * len(members))(*[m._h for m in members]), len(members), C.byref(h)))
        assert not h.value, tag
    g.close()
    for a in fresh + strangers:
        a.close()


def child(job, where):
    out = {}
    name, _, precision = job.partition('_')
    if name == 'group' and precision:
        job_group_kind(out, precision)
    elif precision:
        {'h512': job_h512, 'edges': job_edges}[name](out, precision)
    else:
        {'kinds': job_kinds, 'frames': job_frames, 'group': job_group}[name](out)
    np.savez(os.path.join(where, 'arrays.npz'), **{k.replace('/', '|'): v for k, v in out.items()})


# ---- parent: run the children, compare what they wrote -------------------------------------------------------------------------------
def run(lib, where):
    for job, limit in JOBS.items():
        d = os.path.join(where, job)
        os.makedirs(d, exist_ok=True)
        env = dict(os.environ, FQL_AMD_LIB=os.path.abspath(lib), FQL_DUMP='1')
        t0 = time.perf_counter()
        with open(os.path.join(d, 'dump.txt'), 'w') as err, open(os.path.join(d, 'stdout.txt'), 'w') as so:
            rc = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', job, d],
                                env=env, stdout=so, stderr=err, cwd=ROOT).returncode
        print(f'{lib} {job}: exit {rc} after {time.perf_counter() - t0:.1f} s (limit {limit})', flush=True)
        if rc != 0:
            print(f'stopped: see {d}/dump.txt' + (' (time limit)' if rc in (124, 137) else ''))
            sys.exit(2)


def compare(da, db):
    arrays = lines = 0
    for job in JOBS:
        with np.load(os.path.join(da, job, 'arrays.npz')) as a, np.load(os.path.join(db, job, 'arrays.npz')) as b:
            if sorted(a.files) != sorted(b.files):
                return f'{job}: array names differ: {sorted(set(a.files) ^ set(b.files))[:5]}', arrays, lines
            for k in a.files:
                x, y = a[k], b[k]
                if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                    return f'{job}: {k} differs', arrays, lines
                arrays += 1
            n, nwords = len(a.files), sum(a[k].size for k in a.files if k.endswith(('plan', 'forms')))
        la, lb = (open(os.path.join(d, job, 'dump.txt')).read().splitlines() for d in (da, db))
        for i, (x, y) in enumerate(zip(la, lb)):
            if x != y:
                return f'{job}: dump line {i + 1} differs:\n  a: {x}\n  b: {y}', arrays, lines
        if len(la) != len(lb):
            return f'{job}: {len(la)} dump lines against {len(lb)}', arrays, lines
        lines += len(la)
        print(f'{job}: {n} arrays ({nwords} plan and form words), {len(la)} dump lines')
    return None, arrays, lines


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--child':
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    top = sys.argv[3] if len(sys.argv) == 4 else os.path.join(ROOT, 'build', 'compare_builds')
    for lib, side in ((sys.argv[1], 'a'), (sys.argv[2], 'b')):
        run(lib, os.path.join(top, side))
    diff, arrays, lines = compare(os.path.join(top, 'a'), os.path.join(top, 'b'))
    print(f'compared {arrays} arrays and {lines} dump lines: ' + ('all bitwise equal' if diff is None else 'FIRST DIFFERENCE'))
    if diff is not None:
        print(diff)
        sys.exit(1)
