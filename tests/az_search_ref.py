"""Independent definitions for the search-semantics tests (test infrastructure only; nothing under the package imports this).

``py_search_az``   -- one position's PUCT search under the AlphaZero semantics (``search="alphazero"``):
                      std_rules_ref.py_search with semantics="alphazero" -- the root counts itself once plus every
                      simulation, and the value is negated BEFORE each update on the way up, so a child holds the value
                      from the view of the side that chose it.
``dirichlet_ref``  -- the root noise of the device restated in numpy float64 from its specification: Philox4x32-10,
                      counter (c0, c1, 0x44495249 + attempt words, child rank), Marsaglia-Tsang gamma variates, normalised.
"""
import numpy as np

import std_rules_ref as sr

U64 = np.uint64
NOISE_WORD = 0x44495249


def py_search_az(rules, s, o, sims, c_puct, eval_fn, root_prior=None):
    """-> the rows of sr.py_search.  root_prior: the noisy priors of the root's children, read back from the device."""
    return sr.py_search(rules, s, o, sims, c_puct, eval_fn, "alphazero", root_prior)


def winner_of(s, o):
    """+1 / 0 / -1 relative to the side to move (the owner of `s`)."""
    d = sr.popcount(s) - sr.popcount(o)
    return (d > 0) - (d < 0)


# ---------------------------------------------------------------------------------------------- the noise stream
def philox4x32(seed, c0, c1, c2, c3):
    """Philox4x32-10, key = the two halves of `seed`, counter words as uint64 arrays (values below 2^32; they broadcast).
    -> (ua, ub): float64 arrays in [0, 1) built as (x0>>5, x1>>6) and (x2>>5, x3>>6), 53 random bits each."""
    m32 = U64(0xFFFFFFFF)
    x0, x1, x2, x3 = np.broadcast_arrays(*(np.asarray(c, dtype=U64) & m32 for c in (c0, c1, c2, c3)))
    k0, k1 = U64(int(seed) & 0xFFFFFFFF), U64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * x0, U64(0xCD9E8D57) * x2      # 32 x 32 -> 64 bits: exact in uint64
        x0, x1, x2, x3 = (p1 >> U64(32)) ^ x1 ^ k0, p1 & m32, (p0 >> U64(32)) ^ x3 ^ k1, p0 & m32
        k0, k1 = (k0 + U64(0x9E3779B9)) & m32, (k1 + U64(0xBB67AE85)) & m32

    def dbl(a, b):
        return ((a >> U64(5)).astype(np.float64) * 67108864.0 + (b >> U64(6)).astype(np.float64)) / 9007199254740992.0
    return dbl(x0, x1), dbl(x2, x3)


def gamma_ref(seed, c0, c1, rank, alpha):
    """Gamma(alpha, 1) variates for the keys (c0, c1, rank) (arrays that broadcast), float64: Marsaglia-Tsang with the
    alpha < 1 boost, attempt t on counters (c0, c1, NOISE_WORD + 2t, rank) and (c0, c1, NOISE_WORD + 2t + 1, rank)."""
    c0, c1, rank = np.broadcast_arrays(*(np.asarray(x, dtype=U64) for x in (c0, c1, rank)))
    alpha = float(alpha)
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = np.full(c0.shape, d, dtype=np.float64)      # what 64 rejections in a row would leave
    todo = np.ones(c0.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(64):
            if not todo.any():
                break
            u1, u2 = philox4x32(seed, c0, c1, NOISE_WORD + 2 * t, rank)
            u3, u4 = philox4x32(seed, c0, c1, NOISE_WORD + 2 * t + 1, rank)
            x = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)
            w = 1.0 + c * x
            v = w * w * w
            ok = v > 0.0
            vv = np.where(ok, v, 1.0)
            acc = ok & (np.log(u3) < x * x / 2.0 + d - d * vv + d * np.log(vv))
            gv = d * vv
            if alpha < 1.0:
                gv = gv * np.exp(np.log(1.0 - u4) / alpha)
            take = todo & acc
            g = np.where(take, gv, g)
            todo = todo & ~acc
    return g


def dirichlet_ref(seed, c0, c1, nch, alpha):
    """eta ~ Dir(alpha) over nch children for the key (seed, c0, c1): float64 [nch].  c0 may be an array of keys: -> [len, nch]."""
    c0 = np.asarray(c0, dtype=U64)
    g = gamma_ref(seed, c0[..., None], c1, np.arange(nch, dtype=U64), alpha)
    tot = g.sum(axis=-1, keepdims=True)
    bad = ~(np.isfinite(tot) & (tot > 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(bad, 1.0 / nch, g / tot)
    return eta
