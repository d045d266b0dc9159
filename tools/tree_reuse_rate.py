"""Self-play rate with and without tree reuse, interleaved in ONE GPU session: bench.py's streaming Workload under
rules="othello", search="alphazero" at the flagship shape (8x8, 10x128 network, 50 sims/move, 4096 slots in two lanes) and at
BASELINE configs[3]'s (400 sims/move, c_puct 1.5, threshold 20, 4608 slots in three lanes), engines built with
tree_reuse=False and tree_reuse=True in turn.  One JSON line per (shape, round, setting): games/s, evaluations and new
simulations per game, the mean V0 / S of the inherited roots, and -- from one extra step with the HIP-event hooks on --
k_reroot's time per ply round beside the tree kernels' and the trunk's.
usage: python tools/tree_reuse_rate.py [--shapes flagship configs3] [--rounds 2] [--steps K] [--warmup W]"""
import argparse
import importlib.util
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import othello_reinforcement_learning_test_amd as pkg  # noqa: E402

spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

SHAPES = {
    "flagship": dict(board=8, blocks=10, filters=128, sims=50, games=4096, lanes=2, stagger=61, step_games=1536,
                     c_puct=1.0, temp_threshold=15, warmup=4, steps=8),
    "configs3": dict(board=8, blocks=10, filters=128, sims=400, games=4608, lanes=3, stagger=61, step_games=255,
                     c_puct=1.5, temp_threshold=20, warmup=2, steps=4),
}


def with_reuse(tree_reuse):
    """The package as bench.Workload sees it, every SearchEngine on standard Othello and the AlphaZero search, root noise on."""
    def engine(*a, **kw):
        eng = pkg.SearchEngine(*a, rules="othello", search="alphazero", tree_reuse=tree_reuse, **kw)
        eng.set_root_noise(True)
        return eng
    return types.SimpleNamespace(OthelloResNet=pkg.OthelloResNet, HipResNetEvaluator=pkg.HipResNetEvaluator,
                                 SearchEngine=engine, engine=pkg.engine)


def leg(shape, tree_reuse, warmup, steps):
    sh = dict(SHAPES[shape])
    warmup = sh["warmup"] if warmup is None else warmup
    steps = sh["steps"] if steps is None else steps
    w = bench.Workload(with_reuse(tree_reuse), torch, sh["board"], sh["blocks"], sh["filters"], sh["sims"], sh["games"],
                       sh["lanes"], sh["stagger"], sh["step_games"], c_puct=sh["c_puct"], temp_threshold=sh["temp_threshold"])
    for _ in range(warmup):
        w.play(sh["step_games"], check=True)
    torch.cuda.synchronize()
    c0, t0, n = w.counters(), time.time(), 0
    r0 = [e.reuse_stats() for e in w.engs]
    for _ in range(steps):
        n += w.play(sh["step_games"])[0]
    torch.cuda.synchronize()
    dt = time.time() - t0
    c1 = w.counters()
    r1 = [e.reuse_stats() for e in w.engs]
    st = {k: c1[k] - c0.get(k, 0) for k in c1}
    roots = sum(b["inherited_roots"] - a["inherited_roots"] for a, b in zip(r0, r1))
    v0 = sum(b["inherited_visits"] - a["inherited_visits"] for a, b in zip(r0, r1))
    # one more step with the HIP-event hooks on: the kernels' own time
    rounds0 = sum(e.counters()["net_batches"] for e in w.engs)
    prof = w.profiled_steps(1, lambda: w.play(sh["step_games"])[0])
    rr = [e.reuse_stats() for e in w.engs]
    ply_rounds = (sum(e.counters()["net_batches"] for e in w.engs) - rounds0) / (sh["sims"] + 1)
    w.ev.check_saturation()
    out = {"shape": shape, "tree_reuse": bool(tree_reuse), "games_per_s": round(n / dt, 2), "games_timed": n,
           "seconds_timed": round(dt, 2), "evals_per_game": round(st["evals"] / max(1, st["games"]), 1),
           "new_sims_per_game": round(st["simulations"] / max(1, st["games"]), 1),
           "plies_per_game": round(st["plies"] / max(1, st["games"]), 2),
           "inherited_roots_per_ply": round(roots / max(1, st["plies"]), 4),
           "mean_v0_over_s": round(v0 / max(1, roots) / sh["sims"], 4),
           "profiled_step": {"ply_rounds": round(ply_rounds, 1), "net_ms": round(prof["net_ms"], 1),
                             "tree_ms": round(prof["tree_ms"], 2),
                             "reroot_ms": round(sum(r["reroot_ms"] for r in rr), 3),
                             "reroot_launches": sum(r["reroot_launches"] for r in rr),
                             "reroot_ms_per_ply_round": round(sum(r["reroot_ms"] for r in rr) /
                                                              max(1, sum(r["reroot_launches"] for r in rr)), 4),
                             "positions_per_launch": round(prof["evals"] / max(1, prof["net_launches"]), 1),
                             "net_time_share": round(prof["union_ms"] * 1e-3 / prof["wall_s"], 4) if prof["wall_s"] else None}}
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["flagship", "configs3"], choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    args = ap.parse_args()
    for shape in args.shapes:
        for rnd in range(args.rounds):
            for reuse in (False, True):
                r = leg(shape, reuse, args.warmup, args.steps)
                print(json.dumps(dict({"round": rnd}, **r)), flush=True)


if __name__ == "__main__":
    main()
