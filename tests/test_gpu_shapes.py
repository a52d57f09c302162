"""GPU: FQL at the action widths and shapes where the engine switches kernel paths, against the fp64 oracle on identical params, batch
and noise (tests/util.py's bounds, the same as test_gpu_parity.py's).

The switches these cases sit on either side of (fql_amd/csrc/fql_engine.hip):
  * act_dim <= 15 (with H 256 / 512 and >= 3 equal hidden layers): the BC flow's Euler chain kernel and the fused Euler chain, whose
    16-wide rank update is the action block plus t.  act_dim 15 fills all 16 columns; 16 is the first width on the generic path.
  * the critic's input gradient: the lean 16-column OP_DGRAD0 when K % 512 == 0, obs_dim + 16 <= in_p and act_dim <= 16.  At act_dim 21
    the generic first-layer dgrad runs, and the padded action block is 32 wide.
  * sample_actions / compute_flow_actions run in chunks of 4096 rows; a seeded draw keys each chunk by its first row.
  * a contraction longer than 512 (hidden widths up to 1024, inputs wider than 512): the 16-row GEMM launches switch to
    fql_gemm16_kernel<true> / fql_gemm16_euler_kernel<true>, whose K > 512 tasks hold sixteen B fragments per wave, and ask for
    16 (K + 4) + 2304 floats of dynamic LDS (about 75 KB at K 1024, the largest request of any launch).
"""
import numpy as np
import pytest

from oracle import fql_oracle as O
from tests.util import (K_GEMM16_KBIG, OP_CHAIN, assert_same_state, assert_step_matches, assert_total_loss_matches,
                        assert_trajectory_tracks_oracle, make_problem, randomize_params, read_plan)

pytestmark = pytest.mark.gpu

CASES = [
    # od, ad, B, hidden, cfg overrides
    pytest.param(29, 15, 256, (512,) * 4, {}, id='act15_chain'),                    # last width with the chain and fused Euler
    pytest.param(29, 16, 256, (512,) * 4, {}, id='act16_generic'),                  # first width without; full 16-column OP_DGRAD0
    pytest.param(69, 21, 256, (512,) * 4, dict(alpha=30.0, discount=0.995), id='humanoidmaze'),   # generic paths, ap = 32
    pytest.param(39, 30, 64, (256,) * 4, {}, id='relocate'),                         # 2 padding columns in ap = 32
    pytest.param(45, 24, 48, (80, 48, 64), dict(q_agg='min'), id='ragged_wide'),   # ragged widths with a wide action
    pytest.param(29, 8, 32, (1024,) * 3, {}, id='wide1024'),                        # every hidden contraction at K 1024, no chain
    pytest.param(600, 4, 16, (64, 64, 64), {}, id='obs600'),                        # K <= 128, <= 512 and > 512 tasks in one launch
]


# the path a case's id names, asserted from the engine's plan (fql_debug_plan) before any number is compared
PATH = {
    'act15_chain': lambda plan: any(L['type'] == OP_CHAIN for L in plan),
    'act16_generic': lambda plan: not any(L['type'] == OP_CHAIN for L in plan),
    'humanoidmaze': lambda plan: not any(L['type'] == OP_CHAIN for L in plan),
    'wide1024': lambda plan: any(L['kernel'] == K_GEMM16_KBIG for L in plan),
    'obs600': lambda plan: any(L['kernel'] == K_GEMM16_KBIG for L in plan),
}


def _setup(od, ad, B, hidden, kw, seed=3):
    import fql_amd
    cfg, ds, batch, noise = make_problem(od, ad, B, hidden, seed=seed, **kw)
    agent = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
    params = randomize_params(agent.get_params(), seed=5, scale=0.05 if max(hidden) >= 512 else 0.1)
    agent.set_params(params)
    return cfg, batch, noise, agent, params


@pytest.mark.parametrize('od,ad,B,hidden,kw', CASES)
def test_total_loss_and_update_match_oracle(od, ad, B, hidden, kw, request):
    cfg, batch, noise, agent, params = _setup(od, ad, B, hidden, kw)
    on_path = PATH.get(request.node.callspec.id)
    assert on_path is None or on_path(read_plan(agent)), request.node.callspec.id
    ref = O.OracleFQL(params, dict(cfg), od, ad, np.float64)
    assert_total_loss_matches(agent, ref, params, batch, noise)
    worst = assert_step_matches(agent, ref, cfg, batch, noise)
    print(f'worst relative gradient error {worst[0]:.3e} ({worst[1]})')


@pytest.mark.parametrize('od,ad,B,hidden,kw', CASES)
def test_sample_and_flow_actions_across_the_row_chunk(od, ad, B, hidden, kw):
    """Explicit noises at n = 1, 37 and 4097 (one row past the first 4096-row chunk), then the seeded draw's chunk keying."""
    cfg, batch, noise, agent, params = _setup(od, ad, B, hidden, kw)
    ref = O.OracleFQL(params, dict(cfg), od, ad, np.float64)
    rng = np.random.default_rng(11)
    obs = rng.standard_normal((4097, od)).astype(np.float32)
    z = rng.standard_normal((4097, ad)).astype(np.float32)
    for n in (1, 37, 4097):
        np.testing.assert_allclose(agent.sample_actions(obs[:n], noises=z[:n]), ref.sample_actions(obs[:n], z[:n]), atol=2e-6,
                                   err_msg=str(n))
        np.testing.assert_allclose(agent.compute_flow_actions(obs[:n], z[:n]), ref.compute_flow_actions(obs[:n], z[:n]), atol=5e-6,
                                   err_msg=str(n))
    # one observation 4097 times: the draw of row 4096 (the second chunk's first row) is not row 0's, and chunking does not change the
    # first chunk's draw
    same = np.repeat(obs[:1], 4097, axis=0)
    drawn = agent.sample_actions(same, seed=7)
    assert np.abs(drawn).max() <= 1.0
    assert np.abs(drawn[4096] - drawn[0]).max() > 1e-3
    np.testing.assert_array_equal(drawn[:4096], agent.sample_actions(same[:4096], seed=7))


def test_humanoidmaze_shape_trajectory_tracks_oracle():
    assert_trajectory_tracks_oracle(69, 21, 256, (512,) * 4, seed=23, alpha=30.0, discount=0.995)


def test_wide1024_aql_update_equals_graph_update_bitwise():
    """The K > 512 launches and their > 64 KB LDS request in both dispatch forms: the engine's own queues against the captured graph on a
    caller's stream, three updates from the same rows and noise."""
    import torch
    import fql_amd
    od, ad, B, hidden = 29, 8, 32, (1024,) * 3
    cfg, ds, batch, noise = make_problem(od, ad, B, hidden, seed=3)
    agents = []
    for _ in range(2):
        a = fql_amd.FQLAgent.create(0, batch['observations'][:1], batch['actions'][:1], cfg)
        a.set_params(randomize_params(a.get_params(), seed=5, scale=0.05))
        a.upload_dataset(ds)
        agents.append(a)
    a, b = agents
    st = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    for step in range(3):
        idxs = rng.integers(0, len(ds['observations']), size=B)
        nz = O.make_noise(B, ad, 40 + step)
        a.update_from_dataset(B, idxs=idxs, noise=nz)                          # stream left to the engine -> its own queues
        b.update_from_dataset(B, idxs=idxs, noise=nz, stream=st.cuda_stream)    # a caller's stream -> the captured graph
        assert a.synchronize() == 'aql'
        assert b.synchronize() == 'graph'
        st.synchronize()
        assert a.read_info() == b.read_info()
    assert_same_state(a, b)
