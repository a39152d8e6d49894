#!/usr/bin/env python3
"""Measurement of planning.simplify_multi (the reference's SHORTCUT and BSPLINE routines for many paths in lockstep on the
device, one call) against the way paths were simplified before it: a loop of <robot>.simplify, one path at a time.

Workloads (only files of this tree are read): the solved paths planning.rrtc_multi returns for
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Environments are built, finalized and prepared for the robot, and the paths planned, outside the timed region.  Both
methods end synchronised with the device (host buffers in, host results out), so every time is a host clock around a
window; windows alternate between the methods and are warmed first.  The loop runs an evenly spaced subset of the paths
(--loop-paths, 0 = all) and is compared per path; the lockstep call runs all of them and is also timed on that subset.
The two run different algorithms (the loop is a greedy all-pairs shortcut pass), so the mean cost and waypoint count of
both results are reported beside the times.  --sweep times the whole batch at every questions_per_round.

    python tools/bench_simplify_multi.py [--reps 3] [--workloads mbm,cage] [--loop-paths 64] [--sweep] [--out DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vamp_mvt_amd as vamp  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402
from bench_rrtc_multi import workload_cage, workload_mbm  # noqa: E402

QUESTIONS = (2, 4, 8, 16, 32, 64)


def timed(variants, reps):
    """warm every variant once (those results are reported), then `reps` alternated windows -> results, times in ms"""
    results = {k: f() for k, f in variants.items()}
    times = {k: [] for k in variants}
    for rep in range(reps):
        for k in (list(variants) if rep % 2 == 0 else list(variants)[::-1]):
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return results, times


def shape(paths, costs):
    return {"mean_waypoints": round(float(np.mean([len(p) for p in paths])), 3), "mean_cost": round(float(np.mean(costs)), 4)}


def run(name, starts, goals, envs, skips, args, log):
    robot = vamp.panda
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    plans = planning.rrtc_multi(robot, starts, goals, envs, planning.RRTCMultiSettings(
        range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples), skips)
    solved = [i for i, r in enumerate(plans) if r.solved]
    paths = [np.stack(plans[i].path) for i in solved]
    penvs = [envs[i] for i in solved]
    n = len(paths)
    sub = np.arange(n) if args.loop_paths <= 0 or args.loop_paths >= n else \
        np.unique(np.linspace(0, n - 1, args.loop_paths).astype(np.int64))
    s = planning.SimplifyMultiSettings(questions_per_round=args.questions, check_every=args.check_every)
    loop_settings = vamp.SimplifySettings()

    def multi_all():
        return planning.simplify_multi(robot, paths, penvs, s)

    def multi_sub():
        return planning.simplify_multi(robot, [paths[i] for i in sub], [penvs[i] for i in sub], s)

    def loop_sub():
        return [robot.simplify(list(paths[i]), penvs[i], loop_settings, None) for i in sub]

    variants = {"multi_all": multi_all, "multi_subset": multi_sub, "loop_subset": loop_sub}
    results, times = timed(variants, args.reps)

    def summary(k, count):
        med = statistics.median(times[k])
        return {"paths": count, "median_ms": round(med, 3), "min_ms": round(min(times[k]), 3),
                "windows_ms": [round(t, 3) for t in times[k]], "us_per_path": round(med * 1e3 / count, 3)}

    rec = {"workload": name, "input": shape(paths, [planning.path_cost(list(p)) for p in paths]),
           "settings": {"questions_per_round": s.questions_per_round, "check_every": s.check_every, "max_iterations": s.max_iterations,
                        "operations": list(s.operations), "max_steps": s.max_steps, "min_change": s.min_change},
           "multi_all": summary("multi_all", n), "multi_subset": summary("multi_subset", len(sub)),
           "loop_subset": summary("loop_subset", len(sub))}
    for k in ("multi_all", "multi_subset"):
        r = results[k]
        rec[k].update(shape([x.path for x in r], [x.cost for x in r]))
        rec[k].update({"rounds": r[0].validity_calls, "questions": r[0].edges_checked,
                       "mean_us_per_round": round(rec[k]["median_ms"] * 1e3 / max(r[0].validity_calls, 1), 3),
                       "mean_iterations": round(float(np.mean([x.iterations for x in r])), 3),
                       "status": {st: sum(x.status == st for x in r) for st in planning.SIMPLIFY_STATUS}})
    rec["loop_subset"].update(shape([x.path for x in results["loop_subset"]], [x.cost for x in results["loop_subset"]]))
    rec["same_in_batch_and_subset"] = all(
        len(results["multi_all"][i].path) == len(r.path) and all(np.array_equal(a, b) for a, b in zip(results["multi_all"][i].path, r.path))
        for i, r in zip(sub, results["multi_subset"]))
    rec["loop_over_multi_all_per_path"] = round(rec["loop_subset"]["us_per_path"] / rec["multi_all"]["us_per_path"], 2)
    rec["loop_over_multi_subset"] = round(rec["loop_subset"]["median_ms"] / rec["multi_subset"]["median_ms"], 2)
    log(rec)

    if args.sweep:
        sweeps = {f"w{w}": (lambda w=w: planning.simplify_multi(robot, paths, penvs, planning.SimplifyMultiSettings(
            questions_per_round=w, check_every=args.check_every))) for w in QUESTIONS}
        results, times = timed(sweeps, args.reps)
        base = [[q.tobytes() for q in x.path] for x in results["w2"]]
        log({"workload": name, "sweep": {k: {"median_ms": round(statistics.median(times[k]), 3), "min_ms": round(min(times[k]), 3),
                                             "rounds": results[k][0].validity_calls, "questions": results[k][0].edges_checked,
                                             "us_per_path": round(statistics.median(times[k]) * 1e3 / n, 3),
                                             "same_bytes_as_w2": [[q.tobytes() for q in x.path] for x in results[k]] == base}
                                         for k in sweeps}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--loop-paths", type=int, default=64, help="paths of the <robot>.simplify loop (0 = all)")
    ap.add_argument("--questions", type=int, default=0, help="questions_per_round (0 = the library's default)")
    ap.add_argument("--check-every", type=int, default=0)
    ap.add_argument("--sweep", action="store_true", help="also time the whole batch at every questions_per_round")
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=8192)
    ap.add_argument("--out", default=None, help="directory for simplify_multi_bench.json")
    args = ap.parse_args()
    vamp.set_device(0)
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for name in args.workloads.split(","):
        run(name, *{"mbm": workload_mbm, "cage": workload_cage}[name](), args, log)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "simplify_multi_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
