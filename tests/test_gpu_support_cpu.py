"""gpu_support.check_stream, the replay checker the GPU tests hold every self-play stream to, held itself to streams it must
accept and streams it must refuse.  The streams are seeded random games played through the library's host ABI, pi uniform
over the legal moves, z written by either of the two rules.  No GPU."""
import numpy as np
import pytest

import az_search_ref as az
import std_rules_ref as sr
from gpu_support import check_stream

F32 = np.float32
# (board, rule set, its id in the host ABI, seed of sr.random_games, the two games taken): all four games are of odd length,
# where the two z rules differ, and the first of either pair has a position that must pass
CASES = [(8, "othello", 1, 20258, (9, 10)), (6, "reference", 0, 20256, (2, 3))]
OTHER = {"reference": "alphazero", "alphazero": "reference"}


def planes(bits, bs):
    return np.array([(bits >> i) & 1 for i in range(bs * bs)], dtype=F32).reshape(bs, bs)


def stream(bs, rules_id, games):
    """-> (states [T, 3, bs, bs], pis [T, bs*bs+1], {z rule: zs [T]}, game lengths) of `games` (lists of (self, opp, action)
    plies, the terminal position last)."""
    states, pis, zs, lens = [], [], {"reference": [], "alphazero": []}, []
    for g in games:
        n = len(g) - 1
        w = az.winner_of(g[-1][0], g[-1][1])           # relative to the side to move at the end
        for p, (s, o, _) in enumerate(g[:-1]):
            lg = sr.host_legal(bs, rules_id, s, o)
            states.append(np.stack([planes(s, bs), planes(o, bs), planes(lg, bs)]))
            legal = [a for a in range(bs * bs) if (lg >> a) & 1] or [bs * bs]
            pi = np.zeros(bs * bs + 1, dtype=F32)
            pi[legal] = F32(1.0) / F32(len(legal))
            pis.append(pi)
            zs["reference"].append(w * (1.0 if p % 2 == 0 else -1.0))
            zs["alphazero"].append(w * (1.0 if (n - p) % 2 == 0 else -1.0))
        lens.append(n)
    return np.stack(states), np.stack(pis), {k: np.array(v, dtype=F32) for k, v in zs.items()}, lens


@pytest.mark.parametrize("z", ["reference", "alphazero"])
@pytest.mark.parametrize("bs,name,rules_id,seed,picks", CASES, ids=["8x8-othello", "6x6-reference"])
def test_check_stream_accepts_a_sound_stream_and_refuses_a_broken_one(bs, name, rules_id, seed, picks, z):
    all_games = sr.random_games(bs, rules_id, 200, seed)
    games = [all_games[k] for k in picks]
    assert all((len(g) - 1) % 2 == 1 for g in games), "a game of odd length"
    assert any(a == bs * bs for s, o, a in games[0]), "a game with a pass"
    assert all(az.winner_of(g[-1][0], g[-1][1]) != 0 for g in games), "no draw: a negated z is another z"
    st, pi, zs, lens = stream(bs, rules_id, games)
    n_pass = sum(a == bs * bs for g in games for s, o, a in g)

    assert check_stream(bs, name, st, pi, zs[z], 2, z=z) == (lens, n_pass)
    assert check_stream(bs, name, st, pi, zs[z], 2, lens, z=z) == (lens, n_pass)

    def refused(what, st=st, pi=pi, zs=zs[z], n_games=2, game_len=None):
        try:
            check_stream(bs, name, st, pi, zs, n_games, game_len, z=z)
        except AssertionError:
            return
        pytest.fail("check_stream accepted " + what)

    refused("z written by the other rule", zs=zs[OTHER[z]])
    for t in (0, lens[0] - 1, lens[0] + 1):
        bad = zs[z].copy()
        bad[t] = -bad[t]
        refused("z[%d] negated" % t, zs=bad)
    t = lens[0] // 2
    legal = np.flatnonzero(pi[t])
    illegal = next(a for a in range(bs * bs) if pi[t][a] == 0)
    bad = pi.copy()
    bad[t, illegal], bad[t, legal[0]] = bad[t, legal[0]], 0.0
    assert abs(float(bad[t].astype(np.float64).sum()) - 1.0) < 1e-6      # (the sum alone would pass)
    refused("pi mass on an illegal square", pi=bad)
    for r, c in ((0, 0), tuple(int(x) for x in np.argwhere(st[t, 2] == 1)[0])):
        bad = st.copy()
        bad[t, 2, r, c] = 1.0 - bad[t, 2, r, c]
        refused("bit (%d, %d) of plane 2 flipped" % (r, c), st=bad)
    swap = np.arange(len(st))
    swap[[t, t + 1]] = t + 1, t
    refused("plies %d and %d swapped" % (t, t + 1), st=st[swap], pi=pi[swap], zs=zs[z][swap])
    refused("the last ply dropped", st=st[:-1], pi=pi[:-1], zs=zs[z][:-1])
    keep = np.arange(len(st)) != lens[0] - 1
    refused("the last ply of the first game dropped", st=st[keep], pi=pi[keep], zs=zs[z][keep])
    refused("one game too many expected", n_games=3)
    refused("one game too few expected", n_games=1)
    refused("other game lengths", game_len=[lens[0] + 1, lens[1] - 1])
