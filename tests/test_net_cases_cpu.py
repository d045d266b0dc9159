"""The cases of tests/test_gpu_net_contract.py, checked on the CPU: conditions on the REFERENCE alone (torch fp32 and float64
on the case networks and inputs) that keep the GPU assertions meaningful.  A case that breaks one is changed in
tests/net_cases.py (its seed or damping) -- never the condition."""
import pytest
import torch

import net_cases as nc

PKG = nc.torch_only_pkg()
COMBOS = [(f, b) for b in (8, 6) for f in (16, 32, 64, 128)]   # every (filters, board) the build matrix uses


def test_inputs_are_what_the_docstring_says():
    for board, n in ((8, 291), (6, 207)):
        x = nc.case_inputs(board)
        cells = board * board
        assert tuple(x.shape) == (n, 3, board, board) and set(x.unique().tolist()) == {0.0, 1.0}
        s = x[nc.structured_slice(board)]
        assert len(s) == 3 * cells + 3 == n - nc.N_RANDOM
        assert (s[:3 * cells].flatten(1).sum(1) == 1).all() and len({tuple(r.flatten().tolist()) for r in s}) == len(s)
        assert s[-3].sum() == 0 and s[-2, 0].sum() == cells == s[-2].sum() and s[-1, 1].sum() == cells == s[-1].sum()
        assert max(nc.alone_indices(board)) == n - 1
        assert (x[:nc.N_RANDOM, 0] * x[:nc.N_RANDOM, 1]).sum() == 0     # own and opponent disjoint in the random ones


def test_edge_case_holds_its_edges():
    net = nc.case_net(PKG, "edge", 64, 8)
    gam = torch.cat([m.weight.detach() for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)])
    assert 0.2 < (gam < 0).float().mean().item() < 0.4
    assert net.conv_block.bn.running_var[0].item() == net.res_blocks[0].bn1.running_var[1].item() == pytest.approx(1e-3)
    assert not net.res_blocks[-1].bn2.weight.any() and not net.res_blocks[0].conv2.weight.any()
    assert len(net.res_blocks) == nc.EDGE_BLOCKS and 3 <= nc.EDGE_BLOCKS <= 5
    assert len(nc.case_net(PKG, "shallow", 16, 6).res_blocks) == 1
    assert len(nc.case_net(PKG, "deep", 16, 6).res_blocks) == nc.DEEP_BLOCKS == 23


@pytest.mark.parametrize("filters,board", COMBOS)
@pytest.mark.parametrize("case", nc.CASES)
def test_reference_conditions(case, filters, board):
    """fp32's own distance from float64 small enough that `3 x noise + 1e-6` is a sharp bound (<= 2e-5 on log-probs),
    activations far inside the tightest clamp (< 900 = half of 1875), sane log-probs (> -60), and a value head that is not a
    row of saturated tanh (|v| < 0.99 on >= 90 % of the inputs)."""
    net = nc.case_net(PKG, case, filters, board)
    r = nc.reference(PKG, net, nc.case_inputs(board))
    unsat = (r["tv"].abs() < 0.99).double().mean().item()
    print("\n    %-7s %3d filters %dx%d: fp32 noise logp %.2e value %.2e, largest activation %.0f, min logp %.1f, |v| < 0.99 on "
          "%.0f %%" % (case, filters, board, board, r["noise_l"], r["noise_v"], r["amax"], r["tl"].min().item(), 100 * unsat))
    assert r["noise_l"] <= 2e-5
    assert r["amax"] < 900
    assert r["tl"].min().item() > -60
    assert unsat >= 0.9
    assert torch.isfinite(r["tl"]).all() and torch.isfinite(r["tv"]).all()
