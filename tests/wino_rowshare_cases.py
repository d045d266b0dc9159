"""Builders of the row-tap tests of the Winograd trunk (tests/test_gpu_wino_rowshare.py runs them on the GPU,
tests/test_wino_rowshare_cases_cpu.py checks their own conditions on the CPU): degenerate 128-filter 8x8 networks whose
residual convolutions keep ONE row tap, and the inputs that light one board row at a time.  Deterministic functions of
seeds; nothing here touches the GPU or the native library."""
import numpy as np
import torch

TAPS = (0, 1, 2)          # kernel row kept: dy = -1, 0, +1
BLOCKS = (1, 2)
RAGGED_N = (1, 2, 3, 257, 259)     # one and two positions per workgroup, an odd tail (a workgroup whose second position is
                                   # dead), and both sides of the 256-position switch between the two builds
ALONE = (0, 1, 2, 255, 256, 257, 258)


def one_tap_net(pkg, blocks, tap):
    """OthelloResNet(blocks, 128) in eval mode, freshly initialised (BatchNorm: mean 0, variance 1, gamma 1, beta 0 -- the
    identity up to its eps), every residual convolution with the kernel rows other than `tap` zeroed: each layer moves
    information by exactly tap - 1 board rows, so a fragment paired with the wrong row tap, or a row off by one (the zero
    rows -1 and 8 included), puts a whole board row of the trunk's output in the wrong place."""
    torch.manual_seed(1000 + 10 * blocks + tap)
    net = pkg.OthelloResNet(blocks, 128, board_size=8).eval()
    with torch.no_grad():
        for blk in net.res_blocks:
            for conv in (blk.conv1, blk.conv2):
                keep = conv.weight[:, :, tap, :].clone()
                conv.weight.zero_()
                conv.weight[:, :, tap, :] = keep
    return net


def row_inputs():
    """(9, 3, 8, 8): row r of the own-stones plane full, r = 0..7; then the empty board"""
    x = np.zeros((9, 3, 8, 8), dtype=np.float32)
    for r in range(8):
        x[r, 0, r, :] = 1.0
    return torch.from_numpy(x)
