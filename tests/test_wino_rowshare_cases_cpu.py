"""The conditions the row-tap cases of tests/wino_rowshare_cases.py must meet before the GPU test may rely on them: the
float64 reference of every degenerate network is finite, torch fp32's own distance from it is nonzero (the bound
3 x noise + 1e-6 is not just its floor for the log-probs), the networks really keep one row tap, and the row inputs tell
the rows apart."""
import pytest
import torch

import net_cases as nc
import wino_rowshare_cases as wc


@pytest.fixture(scope="module")
def pkg():
    return nc.torch_only_pkg()


@pytest.mark.parametrize("blocks", wc.BLOCKS)
@pytest.mark.parametrize("tap", wc.TAPS)
def test_one_tap_reference_is_finite_and_noisy(pkg, blocks, tap):
    net = wc.one_tap_net(pkg, blocks, tap)
    for blk in net.res_blocks:
        for conv in (blk.conv1, blk.conv2):
            rows = conv.weight.abs().amax(dim=(0, 1, 3))
            assert (rows > 0).tolist() == [k == tap for k in range(3)]
    x = wc.row_inputs()
    r = nc.reference(pkg, net, x)
    print("\n    blocks %d tap %d: noise logp %.2e value %.2e, largest activation %.1f" % (blocks, tap, r["noise_l"], r["noise_v"],
                                                                                    r["amax"]), end="")
    assert torch.isfinite(r["tl"]).all() and torch.isfinite(r["tv"]).all()
    assert r["noise_l"] > 0 and r["amax"] < 1875.0          # inside the Winograd trunk's clamp at the default scale
    # the nine inputs give nine different outputs, far apart on the scale of the bound: an error that moves a row is
    # visible in the policy (the closest pair: a row that the kept tap pushes off the board, and the empty board)
    tl = r["tl"]
    d = (tl[:, None, :] - tl[None, :, :]).abs().amax(dim=2) + torch.eye(9, dtype=tl.dtype)
    print(", closest pair of outputs %.2e" % d.min().item(), end="")
    assert d.min().item() > 30 * (3 * r["noise_l"] + 1e-6)


def test_row_inputs():
    x = wc.row_inputs()
    assert tuple(x.shape) == (9, 3, 8, 8) and x[8].abs().sum() == 0
    for r in range(8):
        assert x[r].sum() == 8 and x[r, 0, r].sum() == 8
