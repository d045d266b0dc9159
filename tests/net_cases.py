"""Shared builders of the network-contract tests (tests/test_net_cases_cpu.py checks them on the CPU,
tests/test_gpu_net_contract.py runs every trunk build on them): the networks, the inputs and the float64 reference, all
deterministic functions of seeds.  Nothing here touches the GPU or the native library: `pkg` is anything with an
``OthelloResNet`` attribute (the package on the GPU box; `torch_only_pkg()` where the library may not be built)."""
import hashlib
import os
import types

import numpy as np
import torch

CASES = ("shallow", "deep", "edge")
DEEP_BLOCKS = 23          # the most oth_net_create accepts: 1 + 2 * 23 = 47 <= kMaxTrunkLayers = 48
EDGE_BLOCKS = 4


def torch_only_pkg():
    """The package's net.py loaded by path: the torch side of the network without importing the package (whose __init__ pulls
    in the native library)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "othello_reinforcement_learning_test_amd", "net.py")
    spec = importlib.util.spec_from_file_location("_oth_net_torch_only", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return types.SimpleNamespace(OthelloResNet=mod.OthelloResNet)


def _trained_like(pkg, blocks, filters, board, boost=1.0, seed=123):
    """Non-trivial BatchNorm statistics, uneven per-channel scales, peaked policies (what a trained checkpoint looks like);
    boost > 1: the stem's BatchNorm scaled up and the two head convolutions scaled down by the same factor, so the whole
    trunk's activations are ~boost times larger while the outputs stay those of an ordinary network."""
    torch.manual_seed(seed)
    net = pkg.OthelloResNet(blocks, filters, board_size=board).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 1.2 + 0.1)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) * 1.8 + 0.3)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.3)
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.mul_(torch.exp(torch.randn(mod.weight.shape[0], 1, 1, 1, generator=g) * 0.45))
        net.policy_head.fc.weight.mul_(2.0)
        if boost != 1.0:
            net.conv_block.bn.weight.mul_(boost)
            net.conv_block.bn.bias.mul_(boost)
            net.policy_head.conv.weight.div_(boost)
            net.value_head.conv.weight.div_(boost)
    return net


def _max_activation(net, x):
    """largest post-ReLU activation of the trunk under torch fp32 (what the fp16-split kernels clamp)"""
    mx = [0.0]
    hooks = [m.register_forward_hook(lambda _m, _i, o: mx.__setitem__(0, max(mx[0], float(o.max()))))
             for m in [net.conv_block] + list(net.res_blocks)]
    with torch.no_grad():
        out = net(x)
    for h in hooks:
        h.remove()
    return mx[0], out


def max_activation_per_position(net, x):
    """(N,) largest post-ReLU trunk activation of every position, over EVERY layer the fp16-split kernels clamp: the hooks of
    _max_activation (the stem's and the blocks' outputs) and each block's inner activation relu(bn1(conv1(.))), which the
    fused kernels store in f16 halves like any other (measured: on the boosted 64-filter networks it is the larger one)."""
    mx = [None]

    def hook(_m, _i, o):
        a = o.detach().amax(dim=(1, 2, 3)).clamp_min(0)      # (bn1's output is hooked before its ReLU)
        mx[0] = a if mx[0] is None else torch.maximum(mx[0], a)
    hooks = [m.register_forward_hook(hook) for m in [net.conv_block] + list(net.res_blocks) + [b.bn1 for b in net.res_blocks]]
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return mx[0]


def case_net(pkg, case, filters, board):
    """The three networks every trunk build is run on (the board and the filter count are the build's):
    shallow -- one block: the shortest layer pipeline the library accepts;
    deep    -- 23 blocks, the longest; every block's bn2 damped by 0.25 (undamped, 23 trained-like blocks reach activations of
               4 000-13 000 and log-probs of -1 900: nothing a checkpoint looks like, and fp32 itself is 2e-3 off float64);
    edge    -- four blocks with what BN folding and the per-layer power-of-two weight scaling meet in real checkpoints: ~30 %
               of all BatchNorm gammas negative, two near-dead channels (running_var 1e-3: folded scale ~30x), a zero-init
               residual branch (gamma = 0) and an all-zero convolution (the packers' mx == 0 branch)."""
    if case == "shallow":
        return _trained_like(pkg, 1, filters, board)
    if case == "deep":
        net = _trained_like(pkg, DEEP_BLOCKS, filters, board)
        with torch.no_grad():
            for blk in net.res_blocks:
                blk.bn2.weight.mul_(0.25)
                blk.bn2.bias.mul_(0.25)
        return net
    if case == "edge":
        net = _trained_like(pkg, EDGE_BLOCKS, filters, board)
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for mod in net.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    flip = torch.rand(mod.num_features, generator=g) < 0.3
                    mod.weight.mul_(torch.where(flip, -1.0, 1.0))
            net.conv_block.bn.running_var[0] = 1e-3
            net.res_blocks[0].bn1.running_var[1] = 1e-3
            net.res_blocks[-1].bn2.weight.zero_()
            net.res_blocks[0].conv2.weight.zero_()
        return net
    raise ValueError(case)


def random_planes(n, board, seed=5, occupancy=0.6):
    """n random 0/1 plane triples: own / opponent disjoint, the third plane on empty cells (test_wave_trunks_ragged_batches)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    occ = rng.random((n, board, board)) < occupancy
    own = occ & (rng.random((n, board, board)) < 0.5)
    return np.stack([own, occ & ~own, (~occ) & (rng.random((n, board, board)) < 0.5)], axis=1).astype(np.float32)


N_RANDOM = 96


def case_inputs(board):
    """(N,3,S,S) float32: 96 random positions, then the structured ones -- one cell set in one plane (3 * cells inputs: every
    edge and corner of the convolution's padding, alone), the all-zero input, plane 0 full, plane 1 full.  291 positions on
    8x8, 207 on 6x6."""
    cells = board * board
    single = np.zeros((3 * cells, 3, cells), dtype=np.float32)
    for p in range(3):
        for c in range(cells):
            single[p * cells + c, p, c] = 1.0
    zero = np.zeros((1, 3, cells), dtype=np.float32)
    full0, full1 = zero.copy(), zero.copy()
    full0[0, 0, :] = 1.0
    full1[0, 1, :] = 1.0
    rest = np.concatenate([single, zero, full0, full1]).reshape(-1, 3, board, board)
    return torch.from_numpy(np.concatenate([random_planes(N_RANDOM, board), rest]))


def structured_slice(board):
    return slice(N_RANDOM, N_RANDOM + 3 * board * board + 3)


def alone_indices(board):
    """positions whose outputs are compared between the full batch and a launch of their own: a random one, single cells in
    a corner / on an edge / inside (each plane once), the three uniform inputs, the batch's last"""
    cells = board * board
    n = N_RANDOM + 3 * cells + 3
    return [0, N_RANDOM, N_RANDOM + cells + board - 1, N_RANDOM + 2 * cells + board + 1, n - 3, n - 2, n - 1]


def double_copy(pkg, net):
    """the same module in float64 on the same state dict"""
    net64 = pkg.OthelloResNet(net.num_blocks, net.num_filters, board_size=net.board_size).eval().double()
    net64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in net.state_dict().items()})
    return net64


def reference(pkg, net, x, device="cpu"):
    """torch fp32 and float64 forwards of `net` on `x` (on `device`; the network is left on the CPU) ->
    dict(rl, rv: fp32 outputs; tl, tv: float64 outputs; noise_l, noise_v: max |fp32 - float64|, the reference's own rounding;
    amax: largest trunk activation)."""
    x = x.to(device)
    net64 = double_copy(pkg, net).to(device)
    net.to(device)
    try:
        amax = float(max_activation_per_position(net, x).max())
        with torch.no_grad():
            rl, rv = net(x)
    finally:
        net.cpu()
    with torch.no_grad():
        tl, tv = net64(x.double())
    return {"rl": rl, "rv": rv, "tl": tl, "tv": tv, "amax": amax,
            "noise_l": (rl.double() - tl).abs().max().item(), "noise_v": (rv.double() - tv).abs().max().item()}


# ---------------------------------------------------------------------------------------------- the widths fixture
# the nets of tests/golden/g10_net_widths.npz (tests/test_net_widths_cpu.py on the CPU, tests/test_gpu_net_widths.py on the HIP trunks)
WIDTH_NETS = {8: ((2, 48), (3, 96), (2, 160), (2, 192), (4, 256)), 6: ((2, 96), (2, 176), (2, 256))}


def widths_inputs(golden, board):
    """(N,3,S,S) float32 inputs of the fixture's nets: g4's 32 positions on 8x8, g7's planes on 6x6"""
    if board == 8:
        import oracle_lib as ol
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
