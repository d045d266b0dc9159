"""Evaluator families, positions and a node classifier for the tree search at the EVALUATOR'S edges, shared by
tests/test_search_cases_cpu.py (conditions on the oracle alone) and tests/test_gpu_search_edges.py (the HIP search against
the oracle, bit for bit).  No GPU and no native library besides the CPU oracle.

The closed-form stub (stub_eval.py) and a network only ever hand the search positive, normal "probabilities" that are never
all zero on the legal moves.  The families below are deterministic functions of the position (self, opp) alone -- built on
stub_eval.stub_index_value, legality taken from the oracle's own rules -- that drive the expansion (reference node.py:62-89)
into the branches those evaluators never reach:

    zero      all 0                                          masked sum 0 at every node: the uniform fallback (node.py:78-80)
    illegal   1 on every NON-legal action, 0 on the legal    the same through the mask: what is summed is what was masked
    sparse    0 if idx < 8 else idx - 7                      zero-sum and ordinary nodes mixed; zero priors next to 1..8
    denormal  float32(1e-42) * (idx + 1)                     denormal masked sum, normal quotients
    quot      1 if idx == 0 else float32(1e-41) * idx        denormal sums, and normal sums with denormal quotients m / sum
    huge      float32(2e37) * (1 + (idx & 3))                float32 sum overflows to +inf: priors all 0 (NOT the fallback)
    ties      all 1, values sign(v) in {-1, 0, +1}           equal priors and exact values: the descent is tie-breaking
    onehot    1 on the (idx[:, 0] % n_legal)-th legal move   one prior 1, the rest 0: a single line, deep and narrow

`idx` (0..15 per action) and the dyadic value `v` are stub_index_value's.  A pass node (no legal move, terminal roots
included) has the pass action as its only child; `illegal` gives that action 0 and `onehot` gives it 1.

NaN and inf evaluator outputs are OUT OF SCOPE: no family produces either in its probabilities (every one is checked to be
finite), because the reference's behaviour on them is an accident of numpy's comparison rules, not a contract.  The LOGIT
family (logit_values) holds -inf on purpose -- exp(-inf) = 0 is a probability like any other.
"""
import numpy as np

import oracle_lib as ol
from stub_eval import stub_index_value

U64 = np.uint64
F32 = np.float32
FAMILIES = ("zero", "illegal", "sparse", "denormal", "quot", "huge", "ties", "onehot")

# logits for the is_log = 1 path: exp is 0 below about -104 (the first three), denormal down from about -87.34, then ordinary
LOGIT_TABLE = np.array([-np.inf, -200.0, -104.5, -103.0, -95.0, -88.0, -87.0, -40.0, -10.0, -3.0, -1.0, -0.5, -0.1, -1e-7,
                        -0.0, 0.0], dtype=F32)


def legal_bits(s, o, olib=ol):
    """-> (legal bool[n, CELLS], pass_node bool[n]) from the oracle's rules."""
    lg = olib.legal_batch(s, o)
    bits = ((lg[:, None] >> np.arange(olib.CELLS, dtype=U64)[None, :]) & U64(1)).astype(bool)
    return bits, lg == 0


def family_probs_values(name, s, o, olib=ol):
    """(self u64[n], opp u64[n]) -> (probs f32[n, NPOL], values f32[n]) of family `name` on olib's board."""
    s = np.asarray(s, dtype=U64).reshape(-1)
    o = np.asarray(o, dtype=U64).reshape(-1)
    n, cells, npol = len(s), olib.CELLS, olib.NPOL
    idx, v = stub_index_value(s, o, npol)
    if name == "zero":
        p = np.zeros((n, npol), dtype=F32)
    elif name == "illegal":
        bits, pas = legal_bits(s, o, olib)
        p = np.zeros((n, npol), dtype=F32)
        p[:, :cells] = (~bits).astype(F32)
        p[:, cells] = (~pas).astype(F32)
    elif name == "sparse":
        p = np.where(idx < 8, 0, idx - 7).astype(F32)
    elif name == "denormal":
        p = F32(1e-42) * (idx + 1).astype(F32)
    elif name == "quot":
        p = np.where(idx == 0, F32(1.0), F32(1e-41) * idx.astype(F32)).astype(F32)
    elif name == "huge":
        p = F32(2e37) * (1 + (idx & 3)).astype(F32)
    elif name == "ties":
        p = np.ones((n, npol), dtype=F32)
        v = np.sign(v).astype(F32)
    elif name == "onehot":
        bits, pas = legal_bits(s, o, olib)
        p = np.zeros((n, npol), dtype=F32)
        k = idx[:, 0] % np.maximum(bits.sum(1), 1)
        rank = np.cumsum(bits, axis=1) - 1                 # rank of a legal square among the legal squares, ascending
        p[:, :cells] = (bits & (rank == k[:, None])).astype(F32)
        p[:, cells] = pas.astype(F32)
    else:
        raise KeyError(name)
    assert p.dtype == F32 and p.shape == (n, npol) and np.isfinite(p).all()
    return p, v.astype(F32)


def oracle_fn(name, olib=ol):
    """What olib.make_eval takes: fn(s, o) -> (probs, values)."""
    return lambda s, o: family_probs_values(name, s, o, olib)


def engine_fn(name, olib=ol):
    """What SearchEngine.search_with takes: fn(s, o, legal) -> (probs, values); `legal` is ignored, so the engine and the
    oracle are fed by the same function of (s, o)."""
    return lambda s, o, lg: family_probs_values(name, s, o, olib)


def logit_values(s, o, olib=ol):
    """(self, opp) -> (logits f32[n, NPOL] = LOGIT_TABLE[idx], values f32[n]): the evaluator of the is_log = 1 path."""
    idx, v = stub_index_value(np.asarray(s, dtype=U64).reshape(-1), np.asarray(o, dtype=U64).reshape(-1), olib.NPOL)
    return LOGIT_TABLE[idx], v


# ---------------------------------------------------------------------------------------------- positions
def game_positions(n_games, seed, olib=ol):
    """(self, opp, ply) of every position of n_games random playouts on the oracle (PCG64(seed)), game after game."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n_games):
        b = olib.board()
        while not olib.lib().orc_is_terminal(b):
            out.append((int(b.self_board), int(b.opp_board), int(b.move_count)))
            mv = olib.legal_list(b)
            olib.lib().orc_make_move(b, int(mv[rng.integers(len(mv))]))
    return out


_PICKS = {}


def pick_positions(board=8):
    """The positions every search-edge test runs on: six random oracle games (PCG64 seed 77); every 4th of the first 60
    positions (an opening-to-endgame sweep; on 6x6 that is two games), late positions (8x8: 12 of ply >= 50, 6x6: 8 of
    ply >= 26 -- terminal leaves, forced passes) and mid-game ones (8x8: 6 of ply 20..29, 6x6: 10 of ply 10..14; a 6x6
    game is over after ~32 plies and its late positions have one or two moves, so fewer of them keep the share of searches
    that spread over several root children above 80 % for every family).  33 positions on either board.
    -> list of (self, opp, ply)."""
    if board not in _PICKS:
        if board == 8:
            pos = game_positions(6, 77, ol)
            late, n_late, mid, n_mid = 50, 12, (20, 30), 6
        else:
            import oracle_lib6
            pos = game_positions(6, 77, oracle_lib6)
            late, n_late, mid, n_mid = 26, 8, (10, 15), 10
        _PICKS[board] = (pos[:60:4] + [p for p in pos if p[2] >= late][:n_late]
                         + [p for p in pos if mid[0] <= p[2] < mid[1]][:n_mid])
    return list(_PICKS[board])


def mid_game_positions(n=3):
    """n positions of ply 20..29 (the deep, narrow `onehot` case starts from them)."""
    return [p for p in pick_positions(8) if 20 <= p[2] < 30][-n:]


# ---------------------------------------------------------------------------------------------- node classes
def masked_sums(probs, s, o, olib=ol):
    """The float32 masked sum node.py:76 computes for each evaluated node, evaluated by numpy itself (the same pairwise
    add.reduce over a contiguous float32 row): -> (sums f32[n], pass_node bool[n])."""
    bits, pas = legal_bits(s, o, olib)
    probs = np.asarray(probs, dtype=F32)
    masked = np.zeros_like(probs)
    masked[:, :olib.CELLS] = np.where(bits, probs[:, :olib.CELLS], F32(0))
    masked[:, olib.CELLS] = np.where(pas, probs[:, olib.CELLS], F32(0))
    with np.errstate(over="ignore"):
        sums = np.array([np.ascontiguousarray(r).sum() for r in masked], dtype=F32)
    return sums, pas


TINY = np.finfo(F32).tiny   # smallest normal float32, 2^-126


def classify(sums):
    """Counts of the classes of a masked float32 sum: zero, denormal (0 < sum < 2^-126), inf, normal."""
    sums = np.asarray(sums, dtype=F32)
    zero = int((sums == 0).sum())
    den = int(((sums > 0) & (sums < TINY)).sum())
    inf = int(np.isinf(sums).sum())
    return {"nodes": len(sums), "zero": zero, "denormal": den, "inf": inf, "normal": len(sums) - zero - den - inf}


class Tally:
    """Wraps a family's fn(s, o) and classifies every node it is asked to evaluate (counts accumulate over searches)."""

    def __init__(self, fn, olib=ol):
        self.fn, self.olib = fn, olib
        self.counts = {"nodes": 0, "zero": 0, "denormal": 0, "inf": 0, "normal": 0, "pass": 0}

    def __call__(self, s, o):
        p, v = self.fn(s, o)
        sums, pas = masked_sums(p, s, o, self.olib)
        for k, c in classify(sums).items():
            self.counts[k] += c
        self.counts["pass"] += int(pas.sum())
        return p, v
