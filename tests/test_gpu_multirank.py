"""BASELINE.json configs[2] (N-GPU data-parallel self-play with an RCCL all-gather of the replay tuples) kept from
rotting while no multi-GPU node is available.  Three child stages, run one after the other by tests/gpu_children.py (started
by tests/conftest.py at session start, before this process initialises the GPU):

* ``rehearsal``    a PLAIN ``python bench.py --gpus 4`` (no torch.distributed.run around it: bench.py launches its own ranks
                   as a child process before it touches the GPU -- what an 8-GPU node's first contact runs): the N>1 path
                   by FOUR ranks sharing GPU 0, collectives over gloo (RCCL needs one GPU per rank; the
                   box admits six processes on its card, so eight ranks cannot share it -- the world-size-8 exchange step
                   runs on CPU tensors in tests/test_distributed_cpu.py);
* ``rccl_bench``   the SAME code path on a ONE-RANK nccl (= RCCL) group (OTHELLO_FORCE_DIST=1, torch.distributed.run
                   --nproc-per-node 1): the exchange's persistent buffers, the rate all-gather, the device barrier and the
                   final all-reduces run on device tensors through RCCL, as they will on an 8-GPU node;
* ``rccl_worker``  tests/rccl_one_rank_check.py: all_gather_replay with two lane parts over six steps, and
                   DistributedSelfPlayWorker.execute_episodes_tensors with a shrinking second call, on that backend.

These tests wait for the stages and check what they printed."""
import json

import pytest

pytestmark = pytest.mark.gpu


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 must print exactly one JSON line, got %d" % len(lines)
    return json.loads(lines[0])


def _check_small_bench(d, w, err):
    assert d["n_gpus"] == w and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["unit"] == "games/s" and d["value"] > 0 and d["higher_is_better"] is True
    cfg = d["config"]
    assert cfg["games_timed"] >= 2 * w * 29           # every rank's games are counted (shares within +-10 % of 32)
    assert "dp%d" % w in cfg["parallelism"] and "all-gather" in cfg["parallelism"]
    # the all-gathered tuple count of the last step covers all ranks: ~60 plies per game, ~32 games per rank
    assert cfg["samples_last_step"] > w * 29 * 40
    assert d["roofline"]["launches"] > 0 and d["cpu_baseline"] is None
    assert d["roofline"]["kernel"].startswith("k_trunk_f32")      # the 2x16 network: named by the library itself
    rr = d["roofline_rollout"]           # the tree kernel against the HBM roofline, measured live in the profiled step
    assert rr["bound"] == "hbm" and rr["unit"] == "GB/s" and rr["achieved"] > 0 and rr["launches"] > 0
    assert abs(rr["frac"] - rr["achieved"] / rr["peak"]) < 1e-4
    assert "step 2/2" in err                            # heartbeat lines on stderr
    # the N>1 line says how many ranks really ran, what each of them did and what the exchange cost
    assert d["ranks"] == w and len(d["per_rank_games_per_s"]) == w and all(r > 0 for r in d["per_rank_games_per_s"])
    assert abs(sum(d["per_rank_games_per_s"]) - d["value"]) < 0.25 * d["value"]   # (each rank's own clock vs the slowest's)
    assert d["exchange_ms_per_step"] is not None and d["exchange_ms_per_step"] > 0
    # round 6: every rank's lane overlap and mean launch duration (a slow rank is attributable to serialisation vs clock), and
    # the runtime knobs the ranks ran under
    assert len(d["per_rank_lanes_overlap"]) == w and len(d["per_rank_avg_launch_ms"]) == w
    assert all(o > 0 for o in d["per_rank_lanes_overlap"]) and all(m > 0 for m in d["per_rank_avg_launch_ms"])
    env = d["runtime_env"]
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["GPU_MAX_HW_QUEUES"] and env["package_imported_before_hip_runtime"] is True
    r = d["roofline"]
    assert r["lanes_overlap"] > 0 and r["lanes_serialised"] is False      # (toy launches are launch-bound: measured, never flagged)
    assert "lanes_overlap" in r["lanes_check_warmup"]


def test_bench_multi_rank_rehearsal(children):
    rc, out, err = children("rehearsal")
    assert rc == 0, "rehearsal failed (rc %d):\n%s" % (rc, err[-3000:])
    d = _json_line(out)
    _check_small_bench(d, children.ranks, err)
    par = d["config"]["parallelism"]
    assert "REHEARSAL" in par and "gloo" in par         # never reads as an RCCL measurement
    assert d["backend"].startswith("gloo")
    # the stage is a PLAIN `python bench.py --gpus 4`: bench.py itself started the four ranks as a child
    assert d["launched_by"].startswith("bench.py itself")
    assert "--gpus 4 without WORLD_SIZE: starting 4 ranks as a child" in err


def test_bench_n_gt_1_path_on_rccl_one_rank(children):
    """bench.py's N>1 code on RCCL: one rank is all this pool offers, but the calls are the ones an 8-GPU node makes."""
    rc, out, err = children("rccl_bench")
    assert rc == 0, "one-rank RCCL bench failed (rc %d):\n%s" % (rc, err[-3000:])
    d = _json_line(out)
    _check_small_bench(d, 1, err)
    par = d["config"]["parallelism"]
    assert "RCCL all-gather" in par and "REHEARSAL" not in par and "gloo" not in par
    assert d["backend"].startswith("nccl") and d["launched_by"].startswith("torch.distributed.run")
    assert "one-rank group" in par                      # and never reads as a multi-GPU measurement either


def test_distributed_worker_and_exchange_on_rccl_one_rank(children):
    rc, out, err = children("rccl_worker")
    assert rc == 0, "one-rank RCCL worker check failed (rc %d):\n%s" % (rc, err[-3000:])
    d = _json_line(out)
    assert d["ok"] is True and d["backend"] == "nccl" and d["world"] == 1 and d["exchange_steps"] == 6
    calls = d["worker_calls"]
    assert len(calls) == 3 and calls[1] < calls[0]      # the second call's tuple count shrank


def test_bench_other_configs_leg_small():
    """bench.py's secondary legs (`other_configs`: BASELINE configs[3], configs[4], configs[1] + evaluation cache) run only
    behind the full-size headline, so their code path is exercised here at toy size: run_leg on a 6x6 2x32 network (three
    lanes, as the configs[4] leg) and on an 8x8 2x16 network with the evaluation cache -- keys, kernel names from the library,
    positive rates, cache hits counted."""
    import importlib.util
    import os

    import torch

    import othello_reinforcement_learning_test_amd as pkg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.run_leg(pkg, torch, "toy 6x6", "three lanes", board=6, blocks=2, filters=32, sims=4, games=96, step_games=48,
                      warmup=1, steps=2, lanes=3, stagger=8)
    assert a["value"] > 0 and a["games_timed"] >= 96 and a["kernel"].startswith("k_trunk_h3") and a["lanes"] == 3
    assert a["lanes_overlap"] > 0 and a["lanes_serialised"] is False and "lanes_overlap" in a["lanes_check_warmup"]
    assert 0 < a["roofline_frac"] < 1 and a["mfma_flops_issued_per_algorithmic_flop"] >= 3.0 and a["plies_per_game"] > 20
    b = bench.run_leg(pkg, torch, "toy cache", "cache on", board=8, blocks=2, filters=16, sims=6, games=64, step_games=32,
                      warmup=1, steps=2, eval_cache=12, c_puct=1.5, temp_threshold=20, stagger=8)
    assert b["value"] > 0 and b["kernel"].startswith("k_trunk_f32") and b["eval_cache"]["hits"] > 0
    assert 0 < b["eval_cache"]["hit_rate"] < 1 and "c_puct 1.50" in b["workload"] and "threshold 20" in b["workload"]
    ec = b["eval_cache"]   # the misses split into first evaluations and repeats; evictions counted
    assert ec["compulsory_misses"] > 0 and ec["compulsory_misses"] + ec["repeat_misses"] > 0 and ec["conflict_evictions"] >= 0


def test_bench_plain_run_is_lean_and_dumps_identical_outputs(tmp_path, monkeypatch, capsys):
    """A plain run (no --full) at toy size, in this process: the result line carries the headline keys and none of the figures
    that need runs of their own, and --dump-outputs writes the last timed step's tuples -- identical from run to run."""
    import importlib.util
    import os
    import sys

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "OTHELLO_FORCE_DIST"):
        monkeypatch.delenv(k, raising=False)
    outs = []
    for name in ("a", "b"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--games", "64", "--step-games", "32",
                                          "--sims", "6", "--blocks", "2", "--filters", "16", "--stagger", "8",
                                          "--dump-outputs", str(tmp_path / name)])
        bench.main()
        cap = capsys.readouterr()
        d = _json_line(cap.out)
        assert "step 3/3" in cap.err and "step 4/3" not in cap.err and "profiled step" not in cap.err
        assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "games/s"
        assert d["higher_is_better"] is True and d["dtype"].startswith("f32") and "8x8, 6 MCTS sims" in d["metric"]
        assert abs(d["ms_per_step"] * 3e-3 * d["value"] - d["config"]["games_timed"]) < 0.01 * d["config"]["games_timed"]
        assert d["roofline"] is None and d["roofline_rollout"] is None and d["cpu_baseline"] is None and "other_configs" not in d
        arr = {k: np.load(tmp_path / name / (k + ".npy")) for k in ("states", "pis", "zs", "counts")}
        games, n, kept = (int(v) for v in arr["counts"])
        assert games >= 32 and n == kept == d["config"]["samples_last_step"] and n > games * 20
        assert arr["states"].shape == (n, 3, 8, 8) and arr["pis"].shape == (n, 65) and arr["zs"].shape == (n,)
        assert all(arr[k].dtype == np.float32 for k in ("states", "pis", "zs"))
        assert np.allclose(arr["pis"].sum(1), 1.0, atol=1e-5) and set(np.unique(arr["zs"])) <= {-1.0, 0.0, 1.0}
        assert set(np.unique(arr["states"])) <= {0.0, 1.0}
        outs.append(arr)
    assert all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
