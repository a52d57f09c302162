"""CPU: the FQL problems of tests/test_gpu_padded_widths.py (tests/padded_cases.py), built exactly as the GPU test builds them, with no
engine: the numpy and the torch restatement agree at these widths within tests/test_oracle.py's bounds, and the table covers what the
GPU test's docstring claims of it.  This file runs on a machine with no GPU, so the table cannot rot silently."""
import numpy as np
import pytest
import torch

from oracle import fql_oracle as O
from oracle.fql_oracle_torch import TorchFQL
from tests import padded_cases as PC


@pytest.mark.parametrize('cid', list(PC.FQL_CASES))
def test_numpy_matches_torch_autograd_fp64_at_the_padded_widths(cid):
    """tests/test_oracle.py::test_numpy_matches_torch_autograd_fp64's comparison and bounds: loss and infos within 1e-11, every gradient
    leaf at rtol 1e-9 / atol 1e-12."""
    od, ad, B, hidden, kw = PC.FQL_CASES[cid]
    cfg, ds, batch, noise, params = PC.fql_problem(cid)
    assert batch['observations'].shape == (B, od) and noise['x0'].shape == (B, ad)
    assert tuple(cfg['actor_hidden_dims']) == tuple(cfg['value_hidden_dims']) == hidden and all(cfg[k] == v for k, v in kw.items())
    scales = [leaf for path, leaf in O.tree_leaves_with_path(params) if 'LayerNorm' in path]
    assert all(np.abs(leaf - np.round(leaf)).max() > 1e-3 for leaf in scales)      # randomize_params moved the LayerNorm leaves
    cfg = dict(cfg)
    a = O.OracleFQL(params, cfg, od, ad, np.float64)
    b = TorchFQL(params, cfg, torch.float64)
    la, ia, ga = a.grads(batch, noise)
    lb, ib, gb = b.grads(batch, noise)
    assert abs(float(la) - float(lb)) < 1e-11
    for k in ia:
        assert abs(float(ia[k]) - float(ib[k].detach())) < 1e-11, k
    for (pa, xa), (pb, xb) in zip(O.tree_leaves_with_path(ga), O.tree_leaves_with_path(gb)):
        assert pa == pb
        np.testing.assert_allclose(xa, xb.numpy(), rtol=1e-9, atol=1e-12, err_msg=pa)


def test_the_table_covers_what_is_claimed_of_it():
    asked = ['w50', 'w33_100_17', 'w50_actor_ln', 'w100_no_ln', 'w250', 'w500', 'w300_b256', 'w300_b1024', 'w1000']
    assert list(PC.FQL_CASES)[:len(asked)] == asked and list(PC.FQL_CASES)[len(asked):] == ['w250_b1024']
    assert PC.FQL_CASES['w50'] == (29, 8, 32, (50, 50, 50), {})
    assert PC.FQL_CASES['w33_100_17'] == (29, 8, 32, (33, 100, 17), dict(q_agg='min'))
    assert PC.FQL_CASES['w50_actor_ln'] == (29, 8, 32, (50, 50, 50), dict(actor_layer_norm=True))
    assert PC.FQL_CASES['w100_no_ln'] == (29, 8, 16, (100, 100), dict(layer_norm=False))
    assert PC.FQL_CASES['w250'] == (29, 8, 64, (250,) * 4, {}) and PC.FQL_CASES['w500'] == (29, 8, 64, (500,) * 4, {})
    assert PC.FQL_CASES['w300_b256'] == (29, 8, 256, (300, 300, 300), {})
    assert PC.FQL_CASES['w300_b1024'] == (40, 4, 1024, (300, 300), dict(alpha=300.0))
    assert PC.FQL_CASES['w1000'] == (29, 8, 32, (1000,) * 3, {})
    widths = [w for case in PC.FQL_CASES.values() for w in case[3]]
    for cid, case in PC.FQL_CASES.items():
        assert any(w % 16 for w in case[3]), cid                  # every tuple pads at least one width
        assert all(1 <= w <= 1024 for w in case[3]) and case[2] % 16 == 0
    assert any(w % 4 for w in widths)                             # a width the 4-wide vector loads do not divide
    assert {256, 512, 1008} <= {PC.pad16(w) for w in widths if w % 16}
    assert [PC.pad16(w) for w in (33, 100, 17)] == [48, 112, 32] and PC.pad16(50) - 50 == 14 and 50 % 4 == 2
    # the 32- and 64-row tile bodies take N % 64 == 0 and K % 64 == 0: out_p 304 is outside, out_p 256 at M 1024 inside
    assert PC.pad16(300) % 64 and PC.pad16(250) % 64 == 0 and PC.FQL_CASES['w250_b1024'][2] == 1024
    # no case is larger than the configs[1] / configs[2] cases the suite already runs (B x H^2)
    assert all(case[2] * max(case[3]) ** 2 <= 1024 * 512 ** 2 for case in PC.FQL_CASES.values())
