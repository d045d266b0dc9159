"""The opt-in search semantics (search="alphazero") without a device: the numpy restatement of the root noise is a
Dirichlet, the Python reference search differs from the reference-semantics one exactly where intended (the sign of a
child's value), and the selector travels from the YAML key to the engine configuration."""
import numpy as np
import pytest

import az_search_ref as az
import search_cases as sc
import std_rules_ref as sr
from othello_reinforcement_learning_test_amd import _lib


# ---- 1. the noise restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.3, 1.5])      # 0.3: Gamma(alpha + 1) and the boost step; 1.5: no boost
def test_dirichlet_restatement_is_a_dirichlet(alpha):
    n, nch = 20000, 4
    eta = az.dirichlet_ref(12345, np.arange(n), 3, nch, alpha)
    assert eta.shape == (n, nch) and np.isfinite(eta).all() and (eta >= 0).all()
    assert np.abs(eta.sum(axis=1) - 1.0).max() < 1e-12
    # a Dir(alpha) component over nch children is Beta(alpha, (nch-1) alpha): mean 1/nch, variance below
    var = (1.0 / nch) * (1.0 - 1.0 / nch) / (nch * alpha + 1.0)
    # the variable lies in [0, 1], so its fourth central moment is at most its variance: the standard error of the sample
    # variance is at most sqrt(var / n), the same bound as the mean's
    tol = 5.0 * np.sqrt(var / n)
    mean, svar = eta.mean(axis=0), eta.var(axis=0, ddof=1)
    print("alpha", alpha, "mean", mean, "var", svar, "want", 1.0 / nch, var, "+-", tol)
    assert np.abs(mean - 1.0 / nch).max() < tol
    assert np.abs(svar - var).max() < tol
    # one key at a time gives the same numbers, and another seed or ply gives others
    assert np.array_equal(az.dirichlet_ref(12345, 7, 3, nch, alpha), eta[7])
    assert not np.array_equal(az.dirichlet_ref(12346, 7, 3, nch, alpha), eta[7])
    assert not np.array_equal(az.dirichlet_ref(12345, 7, 4, nch, alpha), eta[7])


def test_philox_restatement_is_the_action_draws_generator():
    """The first double of the four-word generator at the action draw's counter words is the oracle's uniform."""
    import oracle_lib as ol
    for seed, gid, ply in ((1, 0, 0), (2**62 + 12345, 17, 33), (0xFFFFFFFFFFFFFFFF, 4095, 127)):
        ua, _ = az.philox4x32(seed, gid, ply, 0x2545F491, 0x9E3779B9)
        assert float(ua) == ol.philox_uniform(seed, gid, ply)


# ---- 2. the backup sign, on the Python searches alone --------------------------------------------------------------------
def terminal_children(rules, s, o):
    """[(action, winner relative to the side to move at the child)] of the root children that end the game."""
    out = []
    for a in sr.legal_actions(rules, s, o):
        cs, co = sr.apply_move(rules, s, o, a)
        if rules.legal(cs, co) == 0 and rules.legal(co, cs) == 0:
            out.append((a, az.winner_of(cs, co)))
    return out


def late_positions():
    """The late positions of search_cases' six games: the twelve of pick_positions (terminal leaves below the root) and
    the last position of every game (a move from it ends the game, so the root itself has a terminal child)."""
    pos = sc.game_positions(6, 77)
    last = [p for p, q in zip(pos, pos[1:] + [(0, 0, 0)]) if q[2] < p[2]]
    assert len(last) == 6 and all(p[2] >= 50 for p in last)
    return [(s, o) for s, o, ply in sc.pick_positions(8) if ply >= 50] + [(s, o) for s, o, _ in last]


def test_backup_sign_differs_between_the_two_python_searches():
    rules = sr.MaskRules(8, swapped=True)          # search_cases' positions are games of the reference's rules
    fn = sr.stub_eval_fn(65)
    seen_az = seen_ref = nonzero = 0
    for s, o in late_positions():
        kids = terminal_children(rules, s, o)
        if not kids:
            continue
        v_az, w_az, _, _ = az.py_search_az(rules, s, o, 50, 1.0, fn)
        v_rf, w_rf, _, _ = sr.py_search(rules, s, o, 50, 1.0, fn)
        assert int(v_az.sum()) == 50 and int(v_rf.sum()) == 50
        for a, win in kids:
            if v_az[a]:
                assert w_az[a] / v_az[a] == -win, "alphazero: a terminal child holds -winner(child)"
                seen_az += 1
                nonzero += win != 0
            if v_rf[a]:
                assert w_rf[a] / v_rf[a] == win, "reference: a terminal child holds +winner(child)"
                seen_ref += 1
    print("terminal root children visited: alphazero %d (%d decided), reference %d" % (seen_az, nonzero, seen_ref))
    assert seen_az >= 3 and seen_ref >= 1 and nonzero >= 1


def test_first_descent_takes_the_largest_prior():
    """With the root counted once before any simulation, U > 0 at the root: one simulation visits the child of the
    largest prior (first one on ties), not the first legal move as the reference's search does."""
    rules = sr.MaskRules(8, swapped=True)
    fn = sr.stub_eval_fn(65)
    differ = 0
    for s, o, _ in sc.pick_positions(8)[:15]:
        v, _, p, _ = az.py_search_az(rules, s, o, 1, 1.0, fn)
        legal = sr.legal_actions(rules, s, o)
        best = legal[int(np.argmax([p[a] for a in legal]))]
        assert v[best] == 1 and int(v.sum()) == 1
        differ += best != legal[0]
        assert sr.py_search(rules, s, o, 1, 1.0, fn)[0][legal[0]] == 1
    assert differ >= 1


# ---- 3. the selector's plumbing --------------------------------------------------------------------------------------------
def test_selector_plumbing(monkeypatch):
    assert _lib.search_id("alphazero") == 1 and _lib.search_id("reference") == 0 and _lib.search_id(1) == 1
    assert _lib.search_name(0) == "reference" and _lib.search_name("alphazero") == "alphazero"
    assert _lib.EngineCfg._fields_[-1][0] == "search"
    assert _lib.EngineCfg(4, 4, 15, 1.0, 0.3, 0.25, 0, 0, 8, 0).search == 0        # (ten positional fields: the default)
    for bad in ("muzero", 2, True, None):
        with pytest.raises(ValueError):
            _lib.search_id(bad)
    # an unknown name is refused before any device call: a ValueError with or without a GPU
    import othello_reinforcement_learning_test_amd as pkg
    from othello_reinforcement_learning_test_amd import parallel_self_play as psp
    with pytest.raises(ValueError):
        pkg.SearchEngine(4, 4, search="muzero")
    with pytest.raises(ValueError):
        pkg.ParallelSelfPlayWorker(pkg.OthelloBitboard, None, search="muzero")
    with pytest.raises(ValueError):
        pkg.MCTS(None, search="muzero")
    # the YAML key: mcts.semantics -> the worker's `search`; absent = "reference"; a keyword argument wins
    monkeypatch.setattr(psp, "ParallelSelfPlayWorker", lambda **kw: kw)
    base = {"mcts": {"num_simulations": 7}, "self_play": {}}
    assert psp.create_parallel_self_play_worker(base, None)["search"] == "reference"
    cfg = {"mcts": {"num_simulations": 7, "semantics": "alphazero"}, "game": {"rules": "othello"}}
    kw = psp.create_parallel_self_play_worker(cfg, None)
    assert kw["search"] == "alphazero" and kw["num_simulations"] == 7 and kw["board_class"].rules == "othello"
    assert psp.create_parallel_self_play_worker(cfg, None, search="reference")["search"] == "reference"
    with pytest.raises(ValueError):
        psp.create_parallel_self_play_worker({"mcts": {"semantics": "muzero"}}, None)


def test_root_values():
    from othello_reinforcement_learning_test_amd import SearchEngine
    visits = np.array([[0, 3, 1], [0, 0, 0]], dtype=np.int32)
    wsum = np.array([[0.0, 1.5, -0.5], [0.0, 0.0, 0.0]])
    assert SearchEngine.root_values(visits, wsum).tolist() == [0.25, 0.0]
