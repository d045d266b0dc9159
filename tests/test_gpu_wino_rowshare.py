"""The Winograd trunk's row-sharing loop (k_trunk_w, net_wino.hip): an N-tile is the even or the odd rows of a position, and
each of the four operand fragments F0..F3 = rows {2r - 1 + f} is read once and multiplied with the row taps of BOTH N-tiles
that use it.  What can go wrong there and nowhere else: a fragment paired with the wrong row tap, a row off by one (the zero
rows -1 and 8 included), and the two builds (one / two positions per workgroup) drifting apart.

128 filters on 8x8 is the only shape this kernel has, so the cases are small in blocks and positions
(tests/wino_rowshare_cases.py; their own conditions: tests/test_wino_rowshare_cases_cpu.py).  Bounds: the float64 rule of
tests/test_gpu_net_contract.py, |HIP - float64| <= 3 x noise + 1e-6 with noise = torch fp32's own distance from float64 on
the same inputs, and |HIP - torch fp32| < 1e-4."""
import contextlib
import os

import pytest
import torch

import net_cases as nc
import wino_rowshare_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import othello_reinforcement_learning_test_amd as p
    p._lib.require_device()
    return p


@contextlib.contextmanager
def _tp(tp):
    """OTH_WINO_TP (read per launch) forced to `tp`, or unset for None; put back afterwards"""
    old = os.environ.get("OTH_WINO_TP")
    try:
        os.environ.pop("OTH_WINO_TP", None)
        if tp is not None:
            os.environ["OTH_WINO_TP"] = str(tp)
        yield
    finally:
        os.environ.pop("OTH_WINO_TP", None)
        if old is not None:
            os.environ["OTH_WINO_TP"] = old


def _forward(ev, x, kernel=None):
    if kernel is not None:
        assert ev.kernel_info(len(x))["kernel"].startswith(kernel), ev.kernel_info(len(x))["kernel"]
    logp, v = ev.forward_planes(x, rescue=False)
    torch.cuda.synchronize()
    return logp.clone(), v.clone()


def _check(tag, logp, v, r):
    e32 = ((logp.cpu() - r["rl"].cpu()).abs().max().item(), (v.cpu() - r["rv"].cpu()).abs().max().item())
    e64 = ((logp.double().cpu() - r["tl"].cpu()).abs().max().item(), (v.double().cpu() - r["tv"].cpu()).abs().max().item())
    bound = (3 * r["noise_l"] + 1e-6, 3 * r["noise_v"] + 1e-6)
    print("\n    %-30s logp: err64 %.2e noise %.2e of-bound %4.2f | value: err64 %.2e noise %.2e of-bound %4.2f"
          % (tag, e64[0], r["noise_l"], e64[0] / bound[0], e64[1], r["noise_v"], e64[1] / bound[1]), end="")
    assert torch.isfinite(logp).all() and torch.isfinite(v).all(), tag
    assert e32[0] < 1e-4 and e32[1] < 1e-4, (tag, e32)
    assert e64[0] <= bound[0], (tag, "logp", e64[0], r["noise_l"])
    assert e64[1] <= bound[1], (tag, "value", e64[1], r["noise_v"])


@pytest.mark.parametrize("blocks", wc.BLOCKS)
@pytest.mark.parametrize("tap", wc.TAPS)
def test_row_tap_pairing(pkg, blocks, tap):
    """Residual convolutions with ONE row tap, one board row lit at a time (and the empty board), both builds, against the
    float64 forward of the same module."""
    net = wc.one_tap_net(pkg, blocks, tap)
    x = wc.row_inputs()
    r = nc.reference(pkg, net, x)
    ev = pkg.HipResNetEvaluator(net, precision="f16x3")
    outs = []
    for tp in (1, 2):
        with _tp(tp):
            logp, v = _forward(ev, x.cuda(), "k_trunk_w<%d>" % tp)
        assert not ev.saturated()
        _check("%d block(s) dy %+d TP %d" % (blocks, tap - 1, tp), logp, v, r)
        outs.append((logp, v))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_ragged_launches(pkg):
    """n = 1, 2, 3, 257, 259 positions in both builds: the two builds agree bit for bit at every n, and a position alone is
    the same position inside any batch, bit for bit (odd n under two positions per workgroup: the last workgroup's second
    position is dead)."""
    net = nc.case_net(pkg, "shallow", 128, 8)
    x = torch.from_numpy(nc.random_planes(max(wc.RAGGED_N), 8, seed=11)).cuda()
    ev = pkg.HipResNetEvaluator(net, precision="f16x3")
    alone = {}
    with _tp(1):
        for i in wc.ALONE:
            alone[i] = _forward(ev, x[i:i + 1], "k_trunk_w<1>")
    with _tp(2):
        for i in wc.ALONE:
            l2, v2 = _forward(ev, x[i:i + 1], "k_trunk_w<2>")
            assert torch.equal(l2, alone[i][0]) and torch.equal(v2, alone[i][1]), ("alone, TP 1 vs 2", i)
    for n in wc.RAGGED_N:
        outs = []
        for tp in (1, 2, None):     # None: the library's own choice (one position per workgroup up to 256 positions)
            with _tp(tp):
                outs.append(_forward(ev, x[:n], None if tp is None else "k_trunk_w<%d>" % tp))
            assert tuple(outs[-1][0].shape) == (n, 65) and tuple(outs[-1][1].shape) == (n, 1)
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), ("TP 1 vs 2", n)
        for i in wc.ALONE:
            if i < n:
                assert torch.equal(outs[0][0][i], alone[i][0][0]) and torch.equal(outs[0][1][i], alone[i][1][0]), (n, i)
    assert not ev.saturated()
    # launch-to-launch reproducible
    with _tp(2):
        a, b = _forward(ev, x), _forward(ev, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", ("shallow", "edge"))
def test_independent_summation(pkg, case):
    """The Winograd trunk and the direct kernel (k_trunk16: another transform, another summation order, another LDS image) on
    the single-cell / uniform / random positions of net_cases, each inside the float64 bound."""
    net = nc.case_net(pkg, case, 128, 8)
    x = nc.case_inputs(8).cuda()
    r = nc.reference(pkg, net, x, device="cuda")
    for prec, kernel in (("f16x3", "k_trunk_w"), ("f16x3_direct", "k_trunk16")):
        ev = pkg.HipResNetEvaluator(net, precision=prec)
        with _tp(None):
            logp, v = _forward(ev, x, kernel)
        assert not ev.saturated()
        _check("%s %s" % (case, prec), logp, v, r)
