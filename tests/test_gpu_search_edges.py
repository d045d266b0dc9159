"""The tree search (engine.hip: k_tree, expand_pending, k_cache_insert, k_results, k_policy_exp) pinned to the CPU oracle
where the EVALUATOR'S outputs go wrong: all-zero, denormal and overflowing masked sums, exp() of log-probs below -87 / -104,
total PUCT ties, c_puct 0 and 3, partly filled workgroups, engine reuse and a thrashing evaluation cache.  The inputs are
tests/search_cases.py's (their reference-side conditions: tests/test_search_cases_cpu.py).

EVERY comparison with the oracle is bit for bit (np.array_equal on visits, float64 value sums, float32 priors and pi); the
only tolerance in this module is the accuracy of expf in test_policy_exp_vs_float64."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
import search_cases as sc
from stub_eval import stub_index_value

pytestmark = pytest.mark.gpu
U64 = np.uint64
F32 = np.float32
SIMS = 64
CPUCTS = (0.0, 1.0, 3.0)


@pytest.fixture(scope="module")
def pkg():
    import othello_reinforcement_learning_test_amd as p
    p._lib.require_device()   # fail loudly, never skip
    return p


def device_exp(pkg, x):
    """oth_policy_exp (k_policy_exp: the engine's expf) of a float32 array, computed on the device."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).cuda()
    out = torch.empty_like(t)
    pkg._lib.call("oth_policy_exp", t.data_ptr(), out.data_ptr(), t.numel(), pkg._lib.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle_rows(olib, pick, sims, cp, ev, temperature=1.0):
    return [olib.search(olib.board(s, o), sims, cp, temperature, ev) for s, o, *_ in pick]


def assert_rows_equal(got, want, what):
    """got = (pi, visits, wsum, prior) arrays of the engine; want = the oracle's rows (prior float64 -> float32)."""
    pi, visits, wsum, prior = got
    assert len(want) == len(visits)
    for i, (opi, on, ow, opr) in enumerate(want):
        assert np.array_equal(visits[i], on), (what, i, "visits", visits[i].tolist(), on.tolist())
        assert np.array_equal(wsum[i], ow), (what, i, "value sums")
        assert np.array_equal(prior[i], opr.astype(F32)), (what, i, "priors")
        assert np.array_equal(pi[i], opi), (what, i, "pi")


# ==================================================================================== a. families vs oracle, 8x8
@pytest.mark.parametrize("cp", CPUCTS)
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_families_vs_oracle(pkg, name, cp):
    """expand_pending's uniform fallback (pass nodes included), denormal sums and quotients, the sum that overflows to inf,
    zero priors, total ties (ballot / first set bit all the way down) and c_puct 0 / 1 / 3 against the oracle; the T = 0 pi is
    k_results's first arg-max under the heavy visit-count ties these families produce."""
    pick = sc.pick_positions(8)
    ev = ol.make_eval(sc.oracle_fn(name))
    eng = pkg.SearchEngine(len(pick), SIMS, c_puct=cp)
    got = eng.search_with([p[0] for p in pick], [p[1] for p in pick], sc.engine_fn(name))
    pi0 = eng.search_results(0.0)[0]
    assert eng.counters()["simulations"] == SIMS * len(pick)
    assert_rows_equal(got, oracle_rows(ol, pick, SIMS, cp, ev), (name, cp))
    want0 = oracle_rows(ol, pick, SIMS, cp, ev, temperature=0.0)
    for i, row in enumerate(want0):
        assert np.array_equal(pi0[i], row[0]), (name, cp, i, "T = 0 pi")


def test_onehot_deep_narrow_line(pkg):
    """`onehot` at 300 simulations from three mid-game positions: the tree is little more than a single line (one root child
    takes > 250 of the 300 visits) that runs down to terminal leaves (25 terminal simulations on the oracle's tree) and backs
    values up through the same long path again and again."""
    pick = sc.mid_game_positions(3)
    ev = ol.make_eval(sc.oracle_fn("onehot"))
    eng = pkg.SearchEngine(len(pick), 300, c_puct=1.0)
    got = eng.search_with([p[0] for p in pick], [p[1] for p in pick], sc.engine_fn("onehot"))
    c = eng.counters()
    assert c["simulations"] == 300 * len(pick) and c["terminal_sims"] >= 10, c
    assert got[1].max() > 250
    assert_rows_equal(got, oracle_rows(ol, pick, 300, 1.0, ev), "onehot-300")


# ==================================================================================== b. families vs oracle, 6x6
@pytest.mark.parametrize("name", ["zero", "denormal", "huge", "ties"])
def test_families_vs_oracle_6x6(pkg, name):
    """NP = 37: the masked sum is four groups of eight plus five trailing adds -- over zeros, denormals and the overflow."""
    import oracle_lib6 as ol6
    pick = sc.pick_positions(6)
    ev = ol6.make_eval(sc.oracle_fn(name, ol6))
    eng = pkg.SearchEngine(len(pick), SIMS, c_puct=1.0, board_size=6)
    got = eng.search_with([p[0] for p in pick], [p[1] for p in pick], sc.engine_fn(name, ol6))
    assert got[0].shape == (len(pick), 37)
    assert_rows_equal(got, oracle_rows(ol6, pick, SIMS, 1.0, ev), (name, "6x6"))


# ==================================================================================== c. is_log = 1 at the edges
def drive(eng, pick, eval_fn, is_log, sims=SIMS):
    """The step-wise API by hand (what SearchEngine.search_with does, with is_log passed through)."""
    eng.search_begin([p[0] for p in pick], [p[1] for p in pick])
    for i in range(sims + 1):
        if i:
            eng.search_select()
        s, o, _ = eng.search_leaves()
        if len(s):
            p, v = eval_fn(s, o)
        else:
            p, v = np.zeros((1, eng.npol), F32), np.zeros(1, F32)
        eng.search_expand(p, v, is_log=is_log)
    return eng.search_results(1.0)


@pytest.fixture(scope="module")
def exp_table(pkg):
    """oth_policy_exp of the 16 logits of search_cases.LOGIT_TABLE, as the device returns them."""
    t = device_exp(pkg, sc.LOGIT_TABLE)
    print("\n    device exp of the logit table:", t.tolist())
    return t


def probs_on_device(pkg, exp_table):
    """(s, o) -> (P = oth_policy_exp(L) computed on the device for this very batch, v); the device's exp is a pure function of
    its argument, so P must also be the 16-entry table looked up (what the oracle is fed)."""
    def fn(s, o):
        logits, v = sc.logit_values(s, o)
        p = device_exp(pkg, logits)
        idx, _ = stub_index_value(s, o)
        assert np.array_equal(p, exp_table[idx])
        return p, v
    return fn


def test_is_log_expansion_at_the_edges(pkg, exp_table):
    """oth_search_expand(is_log=1): expf inside expand_pending on logits -inf, -200, -104.5 (exp = 0), -103 .. -88 (denormal)
    up to -0.0 and 0 == the same search fed P = oth_policy_exp(L) with is_log=0 == the oracle fed P.  Nodes whose legal
    logits are all in the exp = 0 group take the uniform fallback after the exp."""
    pick = sc.pick_positions(8)

    def table_fn(s, o):
        idx, v = stub_index_value(s, o)
        return exp_table[idx], v
    tally = sc.Tally(table_fn)
    ev = ol.make_eval(tally)
    for cp in CPUCTS:
        eng = pkg.SearchEngine(len(pick), SIMS, c_puct=cp)
        got_log = drive(eng, pick, sc.logit_values, True)
        eng2 = pkg.SearchEngine(len(pick), SIMS, c_puct=cp)
        got_p = drive(eng2, pick, probs_on_device(pkg, exp_table), False)
        for a, b in zip(got_log, got_p):
            assert np.array_equal(a, b), ("is_log=1 vs is_log=0 on exp'd probabilities", cp)
        assert_rows_equal(got_log, oracle_rows(ol, pick, SIMS, cp, ev), ("is_log", cp))
    print("\n    is_log nodes by masked sum (as the device's exp gives it):", tally.counts)
    assert tally.counts["zero"] >= 50          # legal entries all -inf / -200 / -104.5 (from P == 0: whatever the device returns)
    assert tally.counts["denormal"] >= 50


# ==================================================================================== d. oth_policy_exp vs float64
def test_policy_exp_vs_float64(pkg, record_property):
    """k_policy_exp (the engine's expf, trusted by every exact self-play test to make the oracle's inputs) against numpy's
    float64 exp rounded to float32 on ~20 000 inputs in [-110, 0]: no flush to zero in the denormal range, monotone, exact at
    -inf and +-0, within 2 float32 ulps where the result is normal (1 ulp is the accuracy the HIP math documentation states for
    expf, plus one for rounding the float64 reference onto the float32 grid; no ROCm math documentation ships with the
    toolchain to cite a different figure) and within 2 * 2^-149 absolute where it is denormal."""
    specials = sc.LOGIT_TABLE
    near = []
    for c in (F32(-87.3365), F32(-103.972)):       # log(2^-126) = -87.3365 (first denormal result), log(2^-150) = -103.972 (last non-zero)
        lo = hi = c
        for _ in range(8):
            lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
            near += [lo, hi]
        near.append(c)
    x = np.unique(np.concatenate([np.linspace(-110.0, 0.0, 20000).astype(F32), specials, np.array(near, dtype=F32)]))
    x = np.concatenate([x, np.array([-0.0, 0.0], dtype=F32)])     # (unique keeps one of the two zeros)
    assert 20000 <= len(x) <= 20100 and np.all(np.diff(x[:-2]) > 0)
    y = device_exp(pkg, x)
    with np.errstate(under="ignore"):
        ref64 = np.exp(x.astype(np.float64))
        ref32 = ref64.astype(F32)
    assert y[0] == 0 and np.isneginf(x[0])
    assert y[-1] == 1 and y[-2] == 1 and np.all(y[x == 0] == 1)
    assert np.isfinite(y).all() and (y >= 0).all() and (y <= 1).all()
    assert np.all(np.diff(y[:-2]) >= 0), "not monotone"
    live = ref64 >= 2.0 ** -148
    assert np.all(y[live] > 0), "flushed to zero at x = %r" % x[live][y[live] == 0][:4].tolist()
    normal = ref32 >= sc.TINY
    err = np.abs(y.astype(np.float64) - ref32.astype(np.float64))
    ulps = err[normal] / np.spacing(ref32[normal]).astype(np.float64)
    den_err = err[~normal] / 2.0 ** -149
    worst, worst_den = float(ulps.max()), float(den_err.max())
    print("\n    oth_policy_exp vs float64 on %d inputs: worst error %.3g ulp (normal range, at x = %r), %.3g x 2^-149 (denormal "
          "range); %d denormal results, %d zeros" % (len(x), worst, float(x[normal][ulps.argmax()]), worst_den,
                                                     int(((y > 0) & (y < sc.TINY)).sum()), int((y == 0).sum())))
    record_property("expf_worst_ulp", worst)
    assert worst <= 2.0
    assert worst_den <= 2.0
    assert ((y > 0) & (y < sc.TINY)).sum() > 1000       # the denormal range is really there


# ==================================================================================== e. partly filled blocks, engine reuse
def test_partly_filled_blocks_and_engine_reuse(pkg, golden):
    """ONE SearchEngine(7, 32) searched with n = 1, 2, 3, 5, 7 and 2 roots in turn (a workgroup is four waves = four games:
    idle waves, idle slots of a used block, a second block that comes and goes), the `sparse` and `onehot` families
    alternating, terminal roots and late positions in the batch: nothing of the previous search (pend, eval_slot, path,
    tree) may leak into the next one."""
    term = golden("g9_terminal.npz")["pos"]
    allpos = sc.pick_positions(8)
    late = [p for p in allpos if p[2] >= 50]
    early = [p for p in allpos if p[2] < 50]
    eng = pkg.SearchEngine(7, 32)
    for k, n in enumerate((1, 2, 3, 5, 7, 2)):
        name = ("sparse", "onehot")[k % 2]
        pick = [early[(3 * k + j) % len(early)] for j in range(n)]
        if n >= 3:
            pick[1] = (int(term[k % len(term)][0]), int(term[k % len(term)][1]), -1)
            pick[n - 1] = late[k % len(late)]
            assert ol.lib().orc_is_terminal(ol.board(pick[1][0], pick[1][1]))
        got = eng.search_with([p[0] for p in pick], [p[1] for p in pick], sc.engine_fn(name))
        assert got[1].shape == (n, 65)
        assert eng.counters()["simulations"] == 32 * n, (n, eng.counters())
        assert_rows_equal(got, oracle_rows(ol, pick, 32, 1.0, ol.make_eval(sc.oracle_fn(name))), ("reuse", k, n, name))


# ==================================================================================== f. step-wise search, thrashing cache
def test_stepwise_search_with_a_thrashing_cache(pkg, exp_table):
    """k_cache_insert / cache_fetch through oth_search_expand with a table of 16 entries (8 sets of two ways) under ~5000
    evaluations: nearly every insert evicts, hits still happen (the 33 games' inserts and look-ups of one step), and the
    search is the oracle's.  Then once on the is_log=1 path, where the cached row holds raw log-probs and goes through expf
    at every hit."""
    pick = sc.pick_positions(8)
    s, o = [p[0] for p in pick], [p[1] for p in pick]
    want = oracle_rows(ol, pick, SIMS, 1.0, ol.make_eval(sc.oracle_fn("sparse")))
    plain = pkg.SearchEngine(len(pick), SIMS, eval_cache_log2=0)
    assert_rows_equal(plain.search_with(s, o, sc.engine_fn("sparse")), want, "no cache")
    c0 = plain.counters()
    assert c0["cache_hits"] == 0 and plain.cache_stats()["entries"] == 0
    eng = pkg.SearchEngine(len(pick), SIMS, eval_cache_log2=4)
    assert eng.cache_stats()["entries"] == 16
    assert_rows_equal(eng.search_with(s, o, sc.engine_fn("sparse")), want, "16-entry cache")
    c1, st = eng.counters(), eng.cache_stats()
    print("\n    16-entry cache: %s %s; without: evals %d" % (c1, st, c0["evals"]))
    assert c1["cache_hits"] > 0 and c1["evals"] + c1["cache_hits"] == c0["evals"]
    assert st["conflict_evictions"] > 0 and st["distinct_positions"] + st["repeated_evals"] == c1["evals"]
    # the is_log = 1 path on the same (reused) engine
    def table_fn(s_, o_):
        idx, v = stub_index_value(s_, o_)
        return exp_table[idx], v
    want_log = oracle_rows(ol, pick, SIMS, 1.0, ol.make_eval(table_fn))
    got_log = drive(eng, pick, sc.logit_values, True)
    c2 = eng.counters()
    assert c2["cache_hits"] > 0
    assert_rows_equal(got_log, want_log, "16-entry cache, is_log")
    assert_rows_equal(drive(plain, pick, sc.logit_values, True), want_log, "no cache, is_log")
    assert c2["evals"] + c2["cache_hits"] == plain.counters()["evals"]


# ==================================================================================== g. self-play, saturated policy head
class RecordingEvaluator:
    """Passes forward_bits / policy_probs through to a HipResNetEvaluator and keeps (legal mask, probabilities) of every
    launch the oracle's callback makes (hip_net_eval)."""

    def __init__(self, ev):
        self.ev, self.rows, self._lg = ev, [], None

    def forward_bits(self, s, o, lg):
        self._lg = lg
        return self.ev.forward_bits(s, o, lg)

    def policy_probs(self, logp):
        p = self.ev.policy_probs(logp)
        self.rows.append((self._lg.cpu().numpy().view(U64).copy(), p.cpu().numpy()))
        return p


PASS_BIAS = {"zero": 200.0, "denormal": 95.0}    # added to policy_head.fc.bias[64]


@pytest.mark.parametrize("regime", ["zero", "denormal"])
def test_selfplay_under_a_saturated_policy_head(pkg, regime):
    """A 2x16 network whose pass logit is raised by 200 / 95: log_softmax puts every legal move of a non-pass node at about
    -200 (expf = 0: the uniform fallback at every such node) / about -95 (denormal priors).  The whole device self-play
    (run_search's in-kernel expf, the sampling from pi, the refill) == the oracle driven by the HIP network's own outputs."""
    from gpu_support import assert_streams_equal, hip_net_eval
    torch.manual_seed(321)
    net = pkg.OthelloResNet(2, 16).eval()
    with torch.no_grad():
        net.policy_head.fc.bias[64] += PASS_BIAS[regime]
    ev = pkg.HipResNetEvaluator(net)
    slots, sims, thr, games, seed = 16, 8, 6, 24, 0xC0FFEE
    eng = pkg.SearchEngine(slots, sims, temperature_threshold=thr, evaluator=ev)
    n = eng.selfplay_run(games, seed)
    got = eng.selfplay_fetch(n)
    rec = RecordingEvaluator(ev)
    cb = hip_net_eval(rec, slots)
    ws, wp, wz, _, wl = ol.selfplay_philox(games, seed, sims, thr, cb, parallel_games=slots)
    assert_streams_equal(got, (ws, wp, wz, wl), regime)
    assert eng.counters()["evals"] == cb.calls["pos"]
    # the regime, from the evaluator's own outputs
    lg = np.concatenate([r[0] for r in rec.rows])
    p = np.concatenate([r[1] for r in rec.rows])
    nonpass = lg != 0                                    # (padding rows of a launch are empty boards: no legal move)
    bits = ((lg[:, None] >> np.arange(64, dtype=U64)[None, :]) & U64(1)).astype(bool)
    sq = p[:, :64]
    all_zero = np.array([np.all(sq[i][bits[i]] == 0) for i in range(len(lg))])
    all_den = np.array([np.all((sq[i][bits[i]] > 0) & (sq[i][bits[i]] < sc.TINY)) for i in range(len(lg))])
    hit = (all_zero if regime == "zero" else all_den)[nonpass]
    print("\n    pass bias +%g: %d of %d evaluated non-pass positions have their legal probabilities all %s"
          % (PASS_BIAS[regime], int(hit.sum()), int(nonpass.sum()), "zero" if regime == "zero" else "denormal and non-zero"))
    assert nonpass.sum() > 1000 and hit.mean() > 0.5
