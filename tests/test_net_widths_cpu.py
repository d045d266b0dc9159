"""The package's OthelloResNet at filter counts between and beyond 16 / 32 / 64 / 128 against the reference's own module
(tests/golden/g10_net_widths.npz, written by tests/golden/make_golden_widths.py): under the same seed it has the reference's
state-dict keys and weights (SHA-256 per tensor) and reproduces its outputs.  CPU only; tests/test_gpu_net_widths.py runs the
HIP trunks on the same nets."""
import numpy as np
import pytest
import torch

import net_cases as nc


@pytest.mark.parametrize("seed", [0, 42])
@pytest.mark.parametrize("board", [8, 6])
def test_width_nets_same_init_and_outputs(golden, board, seed):
    g = golden("g10_net_widths.npz")
    pkg = nc.torch_only_pkg()
    x = nc.widths_inputs(golden, board)
    for nb, nf in nc.WIDTH_NETS[board]:
        tag, net = nc.widths_net(pkg, g, board, seed, nb, nf)
        with torch.no_grad():
            logp, v = net(x)
        assert tuple(logp.shape) == (len(x), board * board + 1) and tuple(v.shape) == (len(x), 1)
        assert np.allclose(logp.numpy(), g[tag + "_logp"], atol=1e-6), tag
        assert np.allclose(v.numpy(), g[tag + "_v"], atol=1e-6), tag
