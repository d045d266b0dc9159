"""The package's OthelloResNet at filter counts between and beyond 16 / 32 / 64 / 128 against the reference's own module
(tests/golden/g10_net_widths.npz, written by tests/golden/make_golden_widths.py): under the same seed it has the reference's
state-dict keys and weights (SHA-256 per tensor) and reproduces its outputs.  CPU only; tests/test_gpu_net_widths.py runs the
HIP trunks on the same nets."""
import hashlib

import numpy as np
import pytest
import torch

import net_cases as nc
import oracle_lib as ol

NETS = {8: ((2, 48), (3, 96), (2, 160), (2, 192), (4, 256)), 6: ((2, 96), (2, 176), (2, 256))}


def widths_inputs(golden, board):
    """(N,3,S,S) float32 inputs of the fixture's nets: g4's 32 positions on 8x8, g7's planes on 6x6"""
    if board == 8:
        return torch.from_numpy(np.stack([ol.tensor(ol.board(s, o)) for s, o in golden("g4_net.npz")["pos"]]))
    return torch.from_numpy(golden("g7_net6.npz")["x"])


def widths_net(pkg, g, board, seed, nb, nf):
    """the package's seeded net, checked against the fixture's key names and hashes -> (tag, net)"""
    tag = "b%d_s%d_%dx%d" % (board, seed, nb, nf)
    torch.manual_seed(seed)
    net = pkg.OthelloResNet(nb, nf, board_size=board).eval()
    sd = net.state_dict()
    assert list(sd.keys()) == list(g[tag + "_keys"])
    for k, h in zip(g[tag + "_keys"], g[tag + "_sha"]):
        assert hashlib.sha256(sd[k].numpy().tobytes()).hexdigest() == h, (tag, k)
    return tag, net


@pytest.mark.parametrize("seed", [0, 42])
@pytest.mark.parametrize("board", [8, 6])
def test_width_nets_same_init_and_outputs(golden, board, seed):
    g = golden("g10_net_widths.npz")
    pkg = nc.torch_only_pkg()
    x = widths_inputs(golden, board)
    for nb, nf in NETS[board]:
        tag, net = widths_net(pkg, g, board, seed, nb, nf)
        with torch.no_grad():
            logp, v = net(x)
        assert tuple(logp.shape) == (len(x), board * board + 1) and tuple(v.shape) == (len(x), 1)
        assert np.allclose(logp.numpy(), g[tag + "_logp"], atol=1e-6), tag
        assert np.allclose(v.numpy(), g[tag + "_v"], atol=1e-6), tag
