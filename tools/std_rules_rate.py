"""Self-play rate of the flagship workload (8x8, 50 sims/move, 10x128 network, 4096 games in two lanes) under each rule set,
in ONE GPU session: bench.py's run_leg -- the same streaming schedule as its secondary legs -- with the engines built at
rules="reference" and at rules="othello".  One JSON line per rule set: games/s, plies per game, evaluations per game.
usage: python tools/std_rules_rate.py [--steps K] [--warmup W] [--rules reference othello]"""
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


def with_rules(rules):
    """The package as run_leg sees it, with every SearchEngine it builds on `rules`."""
    def engine(*a, **kw):
        return pkg.SearchEngine(*a, rules=rules, **kw)
    return types.SimpleNamespace(OthelloResNet=pkg.OthelloResNet, HipResNetEvaluator=pkg.HipResNetEvaluator,
                                 SearchEngine=engine, engine=pkg.engine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rules", nargs="+", default=["reference", "othello"])
    args = ap.parse_args()
    keep = ("value", "unit", "plies_per_game", "evals_per_game", "games_timed", "seconds_timed", "kernel", "tree_kernels_ms",
            "net_time_share", "positions_per_launch", "lanes_overlap", "lanes_serialised")
    for rules in args.rules:
        r = bench.run_leg(with_rules(rules), torch, "configs[1] rules=" + rules, board=8, blocks=10, filters=128, sims=50,
                          games=4096, lanes=2, step_games=1536, warmup=args.warmup, steps=args.steps)
        print(json.dumps(dict({"rules": rules}, **{k: r[k] for k in keep if k in r})), flush=True)


if __name__ == "__main__":
    main()
