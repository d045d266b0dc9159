"""What the GPU test files share (test infrastructure only; it holds no tests and touches no GPU at import): the uint64 <->
device plumbing, the evaluators handed to the engine and to the Python searches, the memoised Python search of the 64 roots,
the row-by-row comparison, the replay checker of a self-play stream, the lock-step self-play driver, and the host-side
restatements (HIP network as the oracle's evaluator, the streaming schedule) of the exact self-play tests.
tests/test_gpu_support_cpu.py holds ``check_stream`` to streams it must accept and streams it must refuse."""
import numpy as np
import torch

import az_search_ref as az
import std_rules_ref as sr
from stub_eval import stub_probs_values

U64 = np.uint64
F32 = np.float32
REF, STD = 0, 1


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(U64)


def bits_of(planes):
    """[n, cells] 0/1 -> uint64[n]"""
    w = U64(1) << np.arange(planes.shape[1], dtype=U64)
    return (planes.astype(U64) * w[None, :]).sum(axis=1, dtype=U64)


def split(roots):
    return [r[0] for r in roots], [r[1] for r in roots]


def roots_of(bs, name, n=64):
    return sr.search_roots(bs, STD if name == "othello" else REF, n)


def stream_of(data):
    """A worker's list of (state, pi, z) -> (states, pis, zs)."""
    return (np.stack([d[0] for d in data]), np.stack([d[1] for d in data]), np.array([d[2] for d in data], dtype=F32))


# ---------------------------------------------------------------------------------------------- evaluators
def stub_host_eval(npol):
    """What SearchEngine.search_with takes, from the closed-form stub evaluator."""
    table = sr.stub_table()
    return lambda s, o, lg: stub_probs_values(s, o, table, npol)


def hip_eval_fn(ev, cap, bs):
    """eval_fn of the Python searches whose answers are the HIP network's own: one position in a launch of `cap` rows (the
    shape the engine launches), priors through oth_policy_exp (the engine's expf).  Memoised per position."""
    memo = {}

    def fn(s, o, lg):
        if (s, o) not in memo:
            ss, oo, ll = (np.zeros(cap, dtype=U64) for _ in range(3))
            ss[0], oo[0], ll[0] = s, o, lg
            logp, v = ev.forward_bits(dev_u64(ss), dev_u64(oo), dev_u64(ll))
            memo[(s, o)] = (ev.policy_probs(logp)[0].cpu().numpy(), float(v[0, 0].cpu()))
        return memo[(s, o)]
    return fn


def hip_net_eval(ev, cap, olib=None):
    """orc_eval_fn whose answers are the HIP network's: oth_net_forward_bits on launches of `cap` rows (the shape
    the engine launches, so the same kernel build runs) and oth_policy_exp (the engine's expf) for the priors.
    olib: the oracle binding the callback is for (oracle_lib, or oracle_lib6 for a 6x6 network)."""
    if olib is None:
        import oracle_lib as olib
    calls = {"n": 0, "pos": 0}

    def fn(s, o):
        n = len(s)
        probs = np.empty((n, olib.NPOL), dtype=np.float32)
        vals = np.empty(n, dtype=np.float32)
        for i in range(0, n, cap):
            m = min(cap, n - i)
            ss, oo = np.zeros(cap, dtype=U64), np.zeros(cap, dtype=U64)
            ss[:m], oo[:m] = s[i:i + m], o[i:i + m]
            lg = olib.legal_batch(ss, oo)
            logp, v = ev.forward_bits(dev_u64(ss), dev_u64(oo), dev_u64(lg))
            probs[i:i + m] = ev.policy_probs(logp)[:m].cpu().numpy()
            vals[i:i + m] = v[:m, 0].cpu().numpy()
        calls["n"] += 1
        calls["pos"] += n
        return probs, vals
    cb = olib.make_eval(fn)
    cb.calls = calls
    return cb


# ---------------------------------------------------------------------------------------------- searches and rows
_WANT = {}


def want_search(bs, name, sims, cp, semantics):
    """sr.py_search of the 64 roots of (board, rule set) under the stub evaluator -> (roots, rows).  The Python search is the
    cost of the files that call this: computed once per (board, rules, sims, c_puct, semantics)."""
    key = (bs, name, sims, cp, semantics)
    if key not in _WANT:
        fn = sr.stub_eval_fn(bs * bs + 1)
        roots = roots_of(bs, name)
        _WANT[key] = (roots, [sr.py_search(sr.rules_obj(bs, name), s, o, sims, cp, fn, semantics) for s, o in roots])
    return _WANT[key]


def assert_rows_equal(got, want, what=""):
    """got = (pi, visits, wsum, prior) arrays of the engine; want = rows (visits, wsum, prior, pi) of a Python search."""
    pi, visits, wsum, prior = got
    for i, (wv, ww, wp, wpi) in enumerate(want):
        assert np.array_equal(visits[i], wv), "%svisits of root %d" % (what, i)
        assert np.array_equal(wsum[i], ww), "%svalue sums of root %d" % (what, i)
        assert np.array_equal(prior[i], wp), "%spriors of root %d" % (what, i)
        assert np.array_equal(pi[i], wpi), "%spi of root %d" % (what, i)


def assert_streams_equal(got, want, what=""):
    st, pi, z, gl = got
    ws, wp, wz, wl = want
    assert np.array_equal(gl, wl), "%s: game lengths differ: %s vs %s" % (what, gl[:16], wl[:16])
    assert len(z) == len(wz)
    assert np.array_equal(st, ws), "%s: states differ" % what
    assert np.array_equal(pi, wp), "%s: pi differ" % what
    assert np.array_equal(z, wz), "%s: z differ" % what


# ---------------------------------------------------------------------------------------------- self-play streams
def check_stream(bs, rules_name, states, pis, zs, n_games, game_len=None, z="reference"):
    """Replay every game of a self-play stream with the Python rules of `rules_name`: the planes are 0 / 1, the stream holds
    n_games games (of the lengths game_len), recorded positions are not terminal, plane 2 is the legal mask, pi lives on the
    legal moves and sums to 1, a move of positive pi links each position to the next, the last move ends the game, and z
    follows the rule named by `z`:
      "reference"  z[t] = winner (relative to the side to move at the end) x (+1 on even plies, -1 on odd)   [L16]
      "alphazero"  z[t] = sign(own - opponent's discs at the end) from the view of the side to move at ply t.
    -> (the game lengths, the number of recorded positions that had to pass)."""
    assert z in sr.SEMANTICS
    rules = sr.rules_obj(bs, rules_name)
    cells = bs * bs
    s0, o0 = sr.start_position(bs)
    st = states.reshape(len(states), 3, cells)
    assert set(np.unique(st)) <= {0.0, 1.0}
    sb, ob, lb = (bits_of(st[:, j]) for j in range(3))
    starts = [i for i in range(len(zs)) if (int(sb[i]), int(ob[i])) == (s0, o0)]
    assert len(starts) == n_games, "games in the stream"
    bounds = starts + [len(zs)]
    lens = [bounds[g + 1] - bounds[g] for g in range(n_games)]
    if game_len is not None:
        assert lens == list(game_len)
    passes = 0
    for g in range(n_games):
        lo, hi = bounds[g], bounds[g + 1]
        ends = []
        for t in range(lo, hi):
            s, o = int(sb[t]), int(ob[t])
            lg = rules.legal(s, o)
            assert int(lb[t]) == lg, "plane 2 is the legal mask"
            assert not (lg == 0 and rules.legal(o, s) == 0), "a recorded position is not terminal"
            legal = sr.legal_actions(rules, s, o)
            passes += legal == [cells]
            pi = pis[t]
            assert all(pi[a] == 0 for a in range(cells + 1) if a not in legal), "pi is zero off the legal set"
            assert abs(float(pi.astype(np.float64).sum()) - 1.0) < 1e-6
            moves = [a for a in legal if pi[a] > 0]
            succ = [sr.apply_move(rules, s, o, a) for a in moves]
            if rules_name == "othello":     # the ray-walk board accepts these moves and makes them the same way
                for a, nxt in zip(moves, succ):
                    nb = sr.RayBoard(bs, s, o)
                    assert nb.make_move(a) and nb.bits() == nxt
            if t + 1 < hi:      # linked to the next recorded state by a legal move (or the pass) with pi > 0
                assert (int(sb[t + 1]), int(ob[t + 1])) in succ, "game %d ply %d: no legal move leads to the next state" % (g, t - lo)
            else:               # the last ply: the game ends exactly at a terminal position
                ends = [(cs, co) for cs, co in succ if rules.legal(cs, co) == 0 and rules.legal(co, cs) == 0]
                assert ends, "game %d: its last move does not end the game" % g
        n = hi - lo
        if z == "reference":
            # z = winner (relative to the side to move at the end) x (+1 on even plies, -1 on odd)   [L16]
            winners = {az.winner_of(cs, co) for cs, co in ends}
            sign = np.array([1.0 if (t - lo) % 2 == 0 else -1.0 for t in range(lo, hi)], dtype=np.float32)
            assert any(np.array_equal(zs[lo:hi], np.float32(w) * sign) for w in winners), "game %d: z" % g
        else:
            # the side to move at the end is the mover of ply p exactly when n - p is even (the sides alternate every ply)
            wants = [np.array([az.winner_of(cs, co) * (1.0 if (n - p) % 2 == 0 else -1.0) for p in range(n)], dtype=F32)
                     for cs, co in ends]
            assert any(np.array_equal(zs[lo:hi], w) for w in wants), "game %d (%d plies): z" % (g, n)
    return lens, passes


def lockstep_selfplay(eng, rules, games, max_plies, choose):
    """Lock-step self-play of `games` games from the start position, at most max_plies plies (it stops once every game is
    over): per ply one selfplay_search, whose `active` flags must be the games still running, then for every running game
    choose(game, ply, self, opp, pi row) -> action, then one selfplay_apply, which must report the games left.
    -> dict(tuples = (states, pis, zs), gl, n = tuples harvested, plies per game, over per game, actions per ply)."""
    bs = rules.n
    pos = [sr.start_position(bs)] * games
    over, plies, played = [False] * games, [0] * games, []
    eng.selfplay_begin(games)
    for ply in range(max_plies):
        if all(over):
            break
        pi, active = eng.selfplay_search()
        assert active.tolist() == [0 if f else 1 for f in over]
        actions = np.zeros(games, dtype=np.int32)
        for i, (s, o) in enumerate(pos):
            if over[i]:
                continue
            a = choose(i, ply, s, o, pi[i])
            actions[i], plies[i] = a, plies[i] + 1
            pos[i] = s, o = sr.apply_move(rules, s, o, a)
            over[i] = rules.legal(s, o) == 0 and rules.legal(o, s) == 0
        played.append(actions.copy())
        assert eng.selfplay_apply(actions) == over.count(False)
    n = eng.selfplay_end()
    st, p, z, gl = eng.selfplay_fetch(n)
    return dict(tuples=(st, p, z), gl=gl, n=n, plies=plies, over=over, actions=played)


def pi_checked_move(rules, sims, eval_fn, semantics, rng):
    """A choose() of lockstep_selfplay: the engine's pi must be sr.py_search's at c_puct 1, bit for bit; -> a move of positive
    pi drawn from `rng` (different games take different lines)."""
    def choose(i, ply, s, o, pi):
        want = sr.py_search(rules, s, o, sims, 1.0, eval_fn, semantics)[3]
        assert np.array_equal(pi, want), "game %d ply %d" % (i, ply)
        moves = np.flatnonzero(pi > 0)
        a = int(moves[int(rng.integers(len(moves)))])
        assert a in sr.legal_actions(rules, s, o)
        return a
    return choose


def simulate_stream(lengths, slots, stagger, targets):
    """The streaming schedule restated on the host from the oracle's game lengths: which game ids each step
    returns.  Slot g starts game g at round g*stagger//slots; a finished slot takes the next id; a step ends with
    the round after the one at which >= target games had finished since the last harvest (at least two rounds)."""
    join = [(g * stagger) // slots for g in range(slots)]
    playing = {}          # gid -> plies played
    next_id = slots
    for g in range(slots):
        if join[g] == 0:
            playing[g] = 0
    rnd, done_total, harvested, steps = 0, [], 0, []
    done_after = {0: 0}
    for target in targets:
        first = rnd + 1
        while True:
            rnd += 1
            finished = []
            for gid in list(playing):
                playing[gid] += 1
                if playing[gid] == lengths[gid]:
                    finished.append(gid)
                    del playing[gid]
            for gid in finished:
                done_total.append(gid)
                playing[next_id] = 0
                next_id += 1
            for g in range(slots):
                if join[g] == rnd:
                    playing[g] = 0
            done_after[rnd] = len(done_total)
            if rnd > first and done_after[rnd - 1] - harvested >= target:
                break
        steps.append(sorted(done_total[harvested:]))
        harvested = len(done_total)
    return steps, next_id
