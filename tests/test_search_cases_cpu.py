"""The cases of tests/test_gpu_search_edges.py, checked on the CPU: conditions on the ORACLE alone (64 simulations, c_puct in
{0, 1, 3}, the picked positions) that keep the GPU comparisons meaningful -- every family reaches the branch of the expansion
it exists for, often; pass nodes are expanded; the searches do not degenerate into a single line; nothing the oracle returns
is NaN or inf.  These are conditions on the INPUTS: a family or picker that breaks one is changed in tests/search_cases.py,
never the condition."""
import numpy as np
import pytest

import oracle_lib as ol
import oracle_lib6 as ol6
import search_cases as sc

SIMS = 64
CPUCTS = (0.0, 1.0, 3.0)
# family -> the class of masked float32 sum it exists to produce (search_cases.classify)
BRANCH = {"zero": "zero", "illegal": "zero", "sparse": "zero", "denormal": "denormal", "quot": "denormal", "huge": "inf"}
# 8x8 floors: >= 200 nodes on the intended branch, >= 100 pass nodes.  Measured: zero / illegal 5105 of 5105 nodes, sparse 470
# of 4994, denormal 5072 of 5072, quot 3042 of 5054, huge 3126 inf-sum and 1951 finite-sum of 5077; 353-458 pass nodes.
# 6x6 floors: HALF of what the 6x6 oracle gave when this test was written (a 6x6 game has few passes), family by family:
#            branch nodes, pass nodes, finite-sum nodes (huge only)
MEASURED6 = {"zero": (5190, 63), "illegal": (5190, 63), "sparse": (322, 54), "denormal": (5194, 58), "quot": (3694, 72),
             "huge": (1759, 70, 3435), "ties": (None, 60), "onehot": (None, 137)}


@pytest.fixture(scope="module")
def runs():
    """{(board, family): (Tally counts, searches, searches that spread, all finite, all visit totals right)}: every search
    of the module, run once."""
    out = {}
    for board, olib in ((8, ol), (6, ol6)):
        pick = sc.pick_positions(board)
        for name in sc.FAMILIES:
            tally = sc.Tally(sc.oracle_fn(name, olib), olib)
            ev = olib.make_eval(tally)
            n_search = spread = 0
            finite = totals = True
            for cp in CPUCTS:
                for s, o, _ in pick:
                    pi, visits, wsum, prior = olib.search(olib.board(s, o), SIMS, cp, 1.0, ev)
                    finite &= bool(np.isfinite(pi).all() and np.isfinite(wsum).all() and np.isfinite(prior).all())
                    totals &= int(visits.sum()) == SIMS
                    spread += int((visits > 0).sum() > 1)
                    n_search += 1
            out[(board, name)] = (tally.counts, n_search, spread, finite, totals)
    return out


def test_pickers():
    p8, p6 = sc.pick_positions(8), sc.pick_positions(6)
    assert len(p8) == 33 and len(p6) == 33
    assert sum(p[2] >= 50 for p in p8) >= 12 and sum(20 <= p[2] < 30 for p in p8) >= 6
    assert sum(p[2] >= 26 for p in p6) >= 8
    assert [p[2] for p in sc.mid_game_positions(3)] == [23, 24, 25]
    assert sc.pick_positions(8) == p8          # deterministic


def test_families_are_what_the_docstring_says():
    for olib, board in ((ol, 8), (ol6, 6)):
        pos = sc.pick_positions(board)
        s = np.array([p[0] for p in pos], dtype=np.uint64)
        o = np.array([p[1] for p in pos], dtype=np.uint64)
        bits, pas = sc.legal_bits(s, o, olib)
        nl = bits.sum(1)
        for name in sc.FAMILIES:
            p, v = sc.family_probs_values(name, s, o, olib)
            assert p.dtype == np.float32 and p.shape == (len(pos), olib.NPOL) and np.isfinite(p).all() and (p >= 0).all()
            assert v.dtype == np.float32 and (np.abs(v) <= 1).all()
            p2, v2 = sc.family_probs_values(name, s, o, olib)
            assert np.array_equal(p, p2) and np.array_equal(v, v2)
        p, _ = sc.family_probs_values("illegal", s, o, olib)
        assert not p[:, :olib.CELLS][bits].any() and p[:, :olib.CELLS][~bits].all()
        assert np.array_equal(p[:, olib.CELLS] == 0, pas)
        p, _ = sc.family_probs_values("onehot", s, o, olib)
        assert (p.sum(1) == 1).all() and (p[:, :olib.CELLS][~bits] == 0).all() and np.array_equal(p[:, olib.CELLS] == 1, nl == 0)
        p, _ = sc.family_probs_values("denormal", s, o, olib)
        assert (p > 0).all() and (p < sc.TINY).all()
        p, _ = sc.family_probs_values("quot", s, o, olib)
        assert ((p == 1) | ((p > 0) & (p < sc.TINY))).all()
        p, v = sc.family_probs_values("ties", s, o, olib)
        assert (p == 1).all() and set(np.unique(v)) <= {-1.0, 0.0, 1.0}
        p, _ = sc.family_probs_values("huge", s, o, olib)
        assert p.max() <= np.float32(8.0e37) and p.min() >= np.float32(2e37)
    sums = np.array([0, 1e-45, 1e-39, 1.1754944e-38, 1.0, 3e38, np.inf], dtype=np.float32)
    assert sc.classify(sums) == {"nodes": 7, "zero": 1, "denormal": 2, "inf": 1, "normal": 3}
    lt = sc.LOGIT_TABLE
    assert lt.dtype == np.float32 and len(lt) == 16 and np.isneginf(lt[0]) and not np.isnan(lt).any() and (lt <= 0).all()


@pytest.mark.parametrize("board", [8, 6])
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_oracle_conditions(runs, name, board):
    counts, n_search, spread, finite, totals = runs[(board, name)]
    print("\n    %dx%d %-8s %s; %d of %d searches spread over several root children"
          % (board, board, name, counts, spread, n_search))
    assert finite, "a pi, value sum or prior of the oracle is not finite"
    assert totals, "visits do not sum to the number of simulations"
    assert n_search == 3 * 33
    if board == 8:
        branch_floor, pass_floor, finite_floor = 200, 100, 200
    else:
        m = MEASURED6[name]
        branch_floor, pass_floor, finite_floor = (m[0] or 0) // 2, m[1] // 2, (m[2] // 2 if len(m) > 2 else 0)
    if name in BRANCH:
        assert counts[BRANCH[name]] >= branch_floor
    if name in ("zero", "illegal"):
        assert counts["zero"] == counts["nodes"]          # the fallback at EVERY node
    if name == "huge":
        assert counts["normal"] >= finite_floor           # both sides of the overflow are live
        assert counts["zero"] == counts["denormal"] == 0
    if name in ("ties", "onehot"):
        assert counts["normal"] == counts["nodes"]
    assert counts["pass"] >= pass_floor
    assert spread >= 0.8 * n_search
