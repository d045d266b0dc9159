"""The network forward's contract at its edges: EVERY trunk build the library can dispatch against a float64 forward (log-probs
AND value), on the shortest and the longest layer pipeline oth_net_create accepts and on weights with the corners real
checkpoints have (tests/net_cases.py; the cases' own conditions are checked on the CPU in tests/test_net_cases_cpu.py), at
every activation scale, and the rule that the activation scale is a function of the weights -- at construction too.

Two bounds everywhere: |HIP - torch fp32| < 1e-4 (the project's contract) and |HIP - float64| <= 3 x noise + 1e-6, where noise is
torch fp32's OWN distance from the float64 forward on the same inputs (the rule of test_trunk_on_trained_like_weights): the first
alone leaves ~100x of slack over the observed error, enough to hide a lost lo x hi product or a mis-scaled layer.  Every test
prints `err / noise` and the error as a fraction of its bound (the value's noise is mostly below the 1e-6 floor); DESIGN.md section 1 keeps the worst ratios per build family."""
import contextlib
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import net_cases as nc

pytestmark = pytest.mark.gpu

ENV_KEYS = ("OTH_WINO", "OTH_WINO6", "OTH_TRUNK_TP", "OTH_WINO_TP")


@pytest.fixture(scope="module")
def pkg():
    import othello_reinforcement_learning_test_amd as p
    p._lib.require_device()
    return p


def _b(prec, filters, board, kernel, issued, clamp16=0.0, **env):
    return {"prec": prec, "filters": filters, "board": board, "kernel": kernel, "issued": issued, "clamp16": clamp16, "env": env}


def _h3_issued(positions_per_wave, board):
    """three split products over N-tiles of 16 cells that cover the P positions of a wave: 3 * ceil16(P * cells) / (P * cells)"""
    cells = positions_per_wave * board * board
    return 3 * ((cells + 15) // 16 * 16) / cells


# every trunk build the library can dispatch: name -> how it is selected, what kernel_info must report (the kernel, the MFMA
# FLOPs it issues per algorithmic FLOP -- bench.py's roofline multiplies by that figure -- and its clamp at scale 16)
BUILDS = {}
for _bs in (8, 6):
    for _f in (16, 32, 64, 128):
        BUILDS["f32-%d-%dx%d" % (_f, _bs, _bs)] = _b("f32", _f, _bs, "k_trunk_f32", 1.0)
BUILDS.update({
    # k_trunk_h3: one position per wave on 8x8 (3.0) and for 128 filters on 6x6 (4.0); on 6x6 two with 64 filters (10/3), four with 32 (3.0)
    "h3-32-8x8": _b("f16x3", 32, 8, "k_trunk_h3", _h3_issued(1, 8), 3750.0),
    "h3-64-8x8": _b("f16x3", 64, 8, "k_trunk_h3", _h3_issued(1, 8), 3750.0),
    "h3-32-6x6": _b("f16x3", 32, 6, "k_trunk_h3", _h3_issued(4, 6), 3750.0),
    "h3-128-6x6": _b("f16x3", 128, 6, "k_trunk_h3", _h3_issued(1, 6), 3750.0),
    "h3-64-6x6": _b("f16x3", 64, 6, "k_trunk_h3", _h3_issued(2, 6), 3750.0, OTH_WINO6="0"),     # read when the weights are packed
    "w6-64-6x6": _b("f16x3", 64, 6, "k_trunk_w6", 2.0, 1875.0),
    "direct-tp1": _b("f16x3_direct", 128, 8, "k_trunk16", 2.75, 3750.0, OTH_TRUNK_TP="1"),   # read per launch; kernel_info cannot
    "direct-tp2": _b("f16x3_direct", 128, 8, "k_trunk16", 2.75, 3750.0, OTH_TRUNK_TP="2"),   # see it: bit-identity test below
    "wino-tp1": _b("f16x3", 128, 8, "k_trunk_w<1>", 2.0, 1875.0, OTH_WINO_TP="1"),
    "wino-tp2": _b("f16x3", 128, 8, "k_trunk_w<2>", 2.0, 1875.0, OTH_WINO_TP="2"),
})
assert [_h3_issued(1, 8), _h3_issued(2, 6), _h3_issued(4, 6), _h3_issued(1, 6)] == [3.0, 10 / 3, 3.0, 4.0]
SPLIT_BUILDS = [k for k, b in BUILDS.items() if b["prec"] != "f32"]


@contextlib.contextmanager
def _build_env(build):
    """the four switches of the dispatch set to what the build needs (unset unless named), put back afterwards"""
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(BUILDS[build]["env"])
        yield
    finally:
        for k, val in old.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


@pytest.fixture(scope="module")
def shared():
    """What the tests of this module share -- every case's network, inputs and reference (computed once, left unchanged) and
    the builds' outputs -- freed with the module."""
    store = {"refs": {}, "outs": {}, "wild": {}}
    yield store
    for d in store.values():
        d.clear()
    torch.cuda.empty_cache()


def _case(pkg, shared, case, filters, board):
    """(network, inputs on the GPU, reference) of a case: the float64 and fp32 forwards run once, on the GPU, and are shared"""
    key = (case, filters, board)
    if key not in shared["refs"]:
        net = nc.case_net(pkg, case, filters, board)
        x = nc.case_inputs(board).cuda()
        shared["refs"][key] = (net, x, nc.reference(pkg, net, x, device="cuda"))
    return shared["refs"][key]


def _set_scale(pkg, ev, s):
    pkg._lib.call("oth_net_set_act_scale", ev.handle, C.c_float(s))


def _check_bounds(tag, logp, v, r, rel=1.0):
    """the two bounds, for log-probs and value; prints the measured figures first.  rel > 1 only for the boosted networks."""
    e32 = ((logp - r["rl"]).abs().max().item(), (v - r["rv"]).abs().max().item())
    e64 = ((logp.double() - r["tl"]).abs().max().item(), (v.double() - r["tv"]).abs().max().item())
    bound = ((3 * r["noise_l"] + 1e-6) * rel, 3 * r["noise_v"] + 1e-6)
    print("\n    RATIO %-34s logp: err64 %.2e noise %.2e err/noise %5.2f of-bound %4.2f (vs fp32 %.2e) | value: err64 %.2e noise "
          "%.2e of-bound %4.2f (vs fp32 %.2e)" % (tag, e64[0], r["noise_l"], e64[0] / max(r["noise_l"], 1e-30), e64[0] / bound[0],
                                                  e32[0], e64[1], r["noise_v"], e64[1] / bound[1], e32[1]), end="")
    assert torch.isfinite(logp).all() and torch.isfinite(v).all(), tag
    assert e32[0] < 1e-4 and e32[1] < 1e-4, (tag, e32)
    assert e64[0] <= bound[0], (tag, "logp", e64[0], r["noise_l"])
    assert e64[1] <= bound[1], (tag, "value", e64[1], r["noise_v"])
    assert (logp.double().exp().sum(1) - 1).abs().max().item() < 1e-5, tag


def _run_build(pkg, shared, build, case):
    """outputs of `build` on `case` (kept in `shared`: the bit-identity test of the build pairs reads them again, and
    computes them itself when the matrix test was deselected)"""
    if (build, case) in shared["outs"]:
        return shared["outs"][(build, case)]
    b = BUILDS[build]
    net, x, r = _case(pkg, shared, case, b["filters"], b["board"])
    with _build_env(build):
        ev = pkg.HipResNetEvaluator(net, precision=b["prec"])
        assert ev.precision == b["prec"] and ev.act_scale == 16.0 and ev.rescues == []
        info = ev.kernel_info(len(x))
        assert info["kernel"].startswith(b["kernel"]), (build, info["kernel"])      # the intended kernel, not one tested twice
        assert info["clamp"] == b["clamp16"]
        assert info["issued_per_flop"] == b["issued"], (build, info["issued_per_flop"])
        logp, v = ev.forward_planes(x, rescue=False)
        torch.cuda.synchronize()
        logp, v = logp.clone(), v.clone()
        assert b["prec"] == "f32" or not ev.saturated()
        # a position alone == the same position inside the batch, bit for bit
        assert ev.kernel_info(1)["kernel"].startswith(b["kernel"])
        for i in nc.alone_indices(b["board"]):
            l1, v1 = ev.forward_planes(x[i:i + 1], rescue=False)
            torch.cuda.synchronize()
            assert torch.equal(l1[0], logp[i]) and torch.equal(v1[0], v[i]), (build, case, i)
    shared["outs"][(build, case)] = (logp, v)
    return logp, v


@pytest.mark.parametrize("case", nc.CASES)
@pytest.mark.parametrize("build", list(BUILDS))
def test_build_vs_float64(pkg, shared, build, case):
    """One trunk build on one case: the kernel the library says it ran is the intended one; log-probs and value within 1e-4 of
    torch fp32 and within 3 x noise + 1e-6 of float64; policies sum to one and everything is finite (the structured inputs --
    single cells, empty and full boards -- included); a position's outputs do not depend on the batch it is evaluated in."""
    b = BUILDS[build]
    _, x, r = _case(pkg, shared, case, b["filters"], b["board"])
    logp, v = _run_build(pkg, shared, build, case)
    _check_bounds("%s %s" % (build, case), logp, v, r)
    s = nc.structured_slice(b["board"])
    assert torch.isfinite(logp[s]).all() and torch.isfinite(v[s]).all()
    assert tuple(logp.shape) == (len(x), b["board"] ** 2 + 1) and tuple(v.shape) == (len(x), 1)


@pytest.mark.parametrize("case", nc.CASES)
def test_direct_builds_are_bit_identical(pkg, shared, case):
    """kernel_info does not see OTH_TRUNK_TP: the one- and two-position builds of k_trunk16 are told apart by nothing but this
    -- they sum every accumulator in the same order and must agree bit for bit (as the Winograd pair does)."""
    for pair in (("direct-tp1", "direct-tp2"), ("wino-tp1", "wino-tp2")):
        (l1, v1), (l2, v2) = (_run_build(pkg, shared, k, case) for k in pair)
        assert torch.equal(l1, l2) and torch.equal(v1, v2), pair


def test_twenty_four_blocks_are_refused(pkg):
    """1 + 2 * 24 = 49 layers > kMaxTrunkLayers = 48: refused by oth_net_create, not run (23 blocks is the `deep` case)."""
    net = pkg.OthelloResNet(24, 16).eval()
    with pytest.raises(pkg.OthelloHipError, match="num_blocks 24 out of range"):
        pkg.HipResNetEvaluator(net, precision="f32")


@pytest.mark.parametrize("build", SPLIT_BUILDS)
def test_activation_scale_ladder(pkg, shared, build):
    """Every fp16-split build at every activation scale (16, 8, 4, 2, 1 -- 2 and 1 are what a checkpoint with activations above
    ~7 500 runs at) on the `edge` case: the same two bounds, nothing saturates, and the clamp the library reports doubles with
    every step."""
    b = BUILDS[build]
    net, x, r = _case(pkg, shared, "edge", b["filters"], b["board"])
    with _build_env(build):
        ev = pkg.HipResNetEvaluator(net, precision=b["prec"])
        for scale in (16.0, 8.0, 4.0, 2.0, 1.0):
            _set_scale(pkg, ev, scale)
            logp, v = ev.forward_planes(x, rescue=False)
            torch.cuda.synchronize()
            info = ev.kernel_info(len(x))
            assert info["kernel"].startswith(b["kernel"]) and info["act_scale"] == scale == ev.act_scale
            assert info["clamp"] == b["clamp16"] * 16.0 / scale
            assert not ev.saturated()
            _check_bounds("%s edge scale %g" % (build, scale), logp, v, r)
        assert ev.rescues == [] and ev.precision == b["prec"]


@pytest.mark.parametrize("build,target", [("wino-tp2", 24000.0), ("w6-64-6x6", 24000.0), ("h3-64-8x8", 48000.0),
                                          ("direct-tp2", 48000.0)])
def test_boosted_network_settles_at_scale_one(pkg, build, target):
    """A network whose largest activation is `target` = 24 000 in the Winograd trunks, 48 000 in the direct ones: 0.8 x their
    clamps at scale 1 (30 000 / 60 000).  Construction with the probe launch and the default, rescued call walk the scale down
    to 1, STAY in the fp16-split precision and meet the bounds -- the float64 one relative to the log-probs' magnitude, as in
    test_saturation_beyond_scale_one_falls_back_to_fp32."""
    b = BUILDS[build]
    clamp1 = b["clamp16"] * 16.0
    assert target == 0.8 * clamp1
    from othello_reinforcement_learning_test_amd.engine import probe_positions
    x = nc.case_inputs(b["board"]).cuda()
    # sized over the call's inputs AND the probe positions a calibrate=True constructor evaluates: neither may pass the clamp
    both = torch.cat([x, _planes(probe_positions(b["board"]), b["board"]).cuda()])
    boost = 1.0
    for _ in range(3):      # (the residual blocks' own BatchNorm biases are not boosted: not exactly linear)
        net = nc._trained_like(pkg, 3, b["filters"], b["board"], boost=boost)
        amax = nc.max_activation_per_position(net.cuda(), both).max().item()
        boost *= target / amax
    net = nc._trained_like(pkg, 3, b["filters"], b["board"], boost=boost)
    amax = nc.max_activation_per_position(net.cuda(), both).max().item()     # every clamped layer, the blocks' inner ones too
    r = nc.reference(pkg, net, x, device="cuda")
    assert 0.78 * clamp1 < amax < 0.82 * clamp1 and r["amax"] <= amax, (amax, r["amax"])
    assert amax > clamp1 / 2                                        # beyond the scale-2 clamp
    with _build_env(build), warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        ev = pkg.HipResNetEvaluator(net, precision=b["prec"], calibrate=True)
        logp, v = ev.forward_planes(x)
        info = ev.kernel_info(len(x))
        assert not ev.saturated()
    assert ev.act_scale == 1.0 and ev.precision == b["prec"] and info["kernel"].startswith(b["kernel"])
    assert info["clamp"] == clamp1 > r["amax"]
    assert len(ev.rescues) == 4 == len(wlist) and all("activation scale" in str(w_.message) for w_ in wlist)
    _check_bounds("%s boosted to %.0f" % (build, r["amax"]), logp, v, r, rel=max(1.0, r["tl"].abs().max().item()))


# ============================================================ the activation scale is a function of the weights
def _reachable_pool(pkg, board, n=400, seed=99):
    """n positions of seeded random games played with the library's host rules (as engine.probe_positions, another seed).
    Measured on the CPU under the boosted weights below: 107 of them stay below 0.8 x the scale-16 clamp on 2x64 8x8, 161 on
    5x64 6x6 -- counting every clamped layer (net_cases.max_activation_per_position): a call batch chosen by the blocks'
    OUTPUTS alone saturated at scale 16 in a block's inner activation."""
    lib = pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = []
    while len(pos) < n:
        b = pkg._lib.Board()
        lib.oth_board_reset_n(board, C.byref(b))
        while not lib.oth_board_is_terminal_n(board, C.byref(b)) and len(pos) < n:
            legal = int(lib.oth_legal_moves_n(board, b.self_board, b.opp_board))
            pos.append((b.self_board, b.opp_board, legal))
            moves = [a for a in range(board * board) if (legal >> a) & 1] or [board * board]
            lib.oth_board_make_move_n(board, C.byref(b), int(moves[int(rng.integers(len(moves)))]))
    return tuple(np.array([p[j] for p in pos], dtype=np.uint64) for j in range(3))


def _planes(bits, board):
    """(self, opp, legal) uint64 arrays -> (N,3,S,S) float32 planes, cell c = bit c"""
    sh = np.arange(board * board, dtype=np.uint64)
    a = np.stack([((b[:, None] >> sh) & np.uint64(1)).astype(np.float32) for b in bits], 1)
    return torch.from_numpy(a.reshape(-1, 3, board, board))


def _dev(bits):
    return tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in bits)


def _wild_weights(pkg, shared, blocks, filters, board, clamp16):
    """(tame network, boosted network whose PROBE set peaks at 1.3 x the scale-16 clamp, call batch: the pool positions whose
    largest activation under the boosted weights stays below 0.8 x that clamp)"""
    key = (blocks, filters, board)
    if key in shared["wild"]:
        return shared["wild"][key]
    from othello_reinforcement_learning_test_amd.engine import probe_positions
    xp = _planes(probe_positions(board), board).cuda()
    boost = 1.0
    for _ in range(3):
        net = nc._trained_like(pkg, blocks, filters, board, boost=boost)
        boost *= 1.3 * clamp16 / nc.max_activation_per_position(net.cuda(), xp).max().item()
    wild = nc._trained_like(pkg, blocks, filters, board, boost=boost)
    pmax = nc.max_activation_per_position(wild.cuda(), xp).max().item()
    assert 1.25 * clamp16 < pmax < 1.35 * clamp16, pmax
    pool = _reachable_pool(pkg, board)
    amax = nc.max_activation_per_position(wild, _planes(pool, board).cuda()).cpu().numpy()
    wild.cpu()
    keep = amax < 0.8 * clamp16
    assert keep.sum() >= 32, (int(keep.sum()), len(amax))
    call = tuple(a[keep] for a in pool)
    shared["wild"][key] = (nc._trained_like(pkg, blocks, filters, board), wild, call)
    return shared["wild"][key]


def _copy_weights(dst, src):
    with torch.no_grad():
        for p_, q_ in zip(list(dst.parameters()) + list(dst.buffers()), list(src.parameters()) + list(src.buffers())):
            p_.copy_(q_)


@pytest.mark.parametrize("blocks,filters,board,kernel,clamp16", [(2, 64, 8, "k_trunk_h3", 3750.0),
                                                                 (5, 64, 6, "k_trunk_w6", 1875.0)])
def test_scale_is_a_function_of_the_weights_at_construction_too(pkg, shared, blocks, filters, board, kernel, clamp16):
    """Weights whose probe positions saturate at scale 16 while the call's positions do not: an evaluator CONSTRUCTED on them
    as the workers construct theirs (A, calibrate=True) and one that reached them through an in-place update and refresh() (B)
    must run them at the same scale and return the same bits -- those of an evaluator set to that scale by hand.  (Without the
    probe launch at construction A stayed at 16, B went to 8, and the same weights gave different low bits.)"""
    tame, wild, call = _wild_weights(pkg, shared, blocks, filters, board, clamp16)
    sb, ob, lg = _dev(call)
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        ev_a = pkg.HipResNetEvaluator(wild, calibrate=True)
        assert len(ev_a.rescues) == len(wl) >= 1            # recorded and warned about like any other rescue
        model = pkg.OthelloResNet(blocks, filters, board_size=board).eval()
        model.load_state_dict(tame.state_dict())
        ev_b = pkg.HipResNetEvaluator(model, calibrate=True)
        assert ev_b.act_scale == 16.0 and ev_b.rescues == []
        _copy_weights(model, wild)
        ev_b.refresh()
        ev_c = pkg.HipResNetEvaluator(wild)                  # bare: starts at 16, set by hand below
    assert ev_a.kernel_info(len(sb))["kernel"].startswith(kernel)
    assert ev_a.act_scale == ev_b.act_scale < 16.0, (ev_a.act_scale, ev_b.act_scale)
    assert ev_a.precision == ev_b.precision == "f16x3" and ev_a.rescues == ev_b.rescues
    _set_scale(pkg, ev_c, ev_a.act_scale)
    outs = []
    for ev in (ev_a, ev_b, ev_c):
        logp, v = ev.forward_bits(sb, ob, lg, rescue=False)
        torch.cuda.synchronize()
        assert not ev.saturated()                            # the call's positions fit every scale: nothing to rescue
        outs.append((logp.clone(), v.clone()))
    for logp, v in outs[1:]:
        assert torch.equal(logp, outs[0][0]) and torch.equal(v, outs[0][1])
    _set_scale(pkg, ev_c, 16.0)      # what an uncalibrated constructor leaves A at: fits as well, but other low bits
    l16, v16 = ev_c.forward_bits(sb, ob, lg, rescue=False)
    torch.cuda.synchronize()
    assert not ev_c.saturated()
    print("\n    %dx%d on %dx%d: %d call positions, scale %g; outputs that differ between scale 16 and %g: %d log-probs, %d values"
          % (blocks, filters, board, board, len(sb), ev_a.act_scale, ev_a.act_scale, int((l16 != outs[0][0]).sum()),
             int((v16 != outs[0][1]).sum())), end="")


def test_worker_constructed_on_wild_weights_equals_one_updated_to_them(pkg, shared):
    """The wild-weights form of test_weight_update_resets_the_activation_scale's 'identical to a worker that never saw the other
    weights': a worker constructed on the boosted weights and one constructed on tame weights, run, and then updated to the
    boosted ones in place return identical tuples at the same activation scale."""
    tame, wild, _ = _wild_weights(pkg, shared, 2, 64, 8, 3750.0)
    same = lambda a, b: len(a) == len(b) and all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2]   # noqa: E731
                                                 for p, q in zip(a, b))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w1 = pkg.ParallelSelfPlayWorker(pkg.OthelloBitboard, wild, num_simulations=4, num_parallel_games=8, verbose=False)
        np.random.seed(11)
        d1 = w1.execute_episodes(6)
        model = pkg.OthelloResNet(2, 64).eval()
        model.load_state_dict(tame.state_dict())
        w2 = pkg.ParallelSelfPlayWorker(pkg.OthelloBitboard, model, num_simulations=4, num_parallel_games=8, verbose=False)
        np.random.seed(5)
        w2.execute_episodes(2)
        assert w2.batch_mcts.evaluator.act_scale == 16.0 and w2.batch_mcts.evaluator.rescues == []
        _copy_weights(model, wild)
        np.random.seed(11)
        d2 = w2.execute_episodes(6)
    e1, e2 = w1.batch_mcts.evaluator, w2.batch_mcts.evaluator
    assert e1.act_scale == e2.act_scale < 16.0 and e1.precision == e2.precision == "f16x3"
    assert len(d1) > 0 and same(d1, d2)
