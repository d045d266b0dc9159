"""Self-play rate of the flagship workload (8x8, 50 sims/move, 10x128 network, 4096 games in two lanes) under each search
semantics, in ONE GPU session: bench.py's run_leg -- the same streaming schedule as its secondary legs -- with the engines
built at search="reference" and at search="alphazero" with the root noise on.  One JSON line per semantics: games/s, plies
per game, evaluations per game.
usage: python tools/az_search_rate.py [--steps K] [--warmup W] [--search reference alphazero]"""
import argparse
import importlib.util
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import othello_reinforcement_learning_test_amd as pkg  # noqa: E402

spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def with_search(search):
    """The package as run_leg sees it, with every SearchEngine it builds on `search` (a stream binds the noise at its begin)."""
    def engine(*a, **kw):
        eng = pkg.SearchEngine(*a, search=search, **kw)
        eng.set_root_noise(search == "alphazero")
        return eng
    return types.SimpleNamespace(OthelloResNet=pkg.OthelloResNet, HipResNetEvaluator=pkg.HipResNetEvaluator,
                                 SearchEngine=engine, engine=pkg.engine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--search", nargs="+", default=["reference", "alphazero"])
    args = ap.parse_args()
    keep = ("value", "unit", "plies_per_game", "evals_per_game", "games_timed", "seconds_timed", "kernel", "tree_kernels_ms",
            "net_time_share", "positions_per_launch", "lanes_overlap", "lanes_serialised")
    for search in args.search:
        r = bench.run_leg(with_search(search), torch, "configs[1] search=" + search, board=8, blocks=10, filters=128, sims=50,
                          games=4096, lanes=2, step_games=1536, warmup=args.warmup, steps=args.steps)
        print(json.dumps(dict({"search": search}, **{k: r[k] for k in keep if k in r})), flush=True)


if __name__ == "__main__":
    main()
