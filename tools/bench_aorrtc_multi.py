#!/usr/bin/env python3
"""Measurement of planning.aorrtc_multi (first solution, simplification, then cost-bounded RRT-Connect searches in lockstep)
against the same call with optimize = False (the first solution and its simplification alone: rrtc_multi's and
simplify_multi's kernels) in the same session.

Workloads (only files of this tree are read):
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023);
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal.

Environments are built, finalized and prepared for the robot outside the timed region.  Both variants end synchronised
with the device (host buffers in, host results out), so every time is a host clock around a window; windows alternate
between the variants and are warmed first.  Per workload: the median time of a call of each variant, the problems
solved, those improved, the median of cost / first_cost over the solved problems and over the improved ones, and the
searches, rounds and questions of the call.

    python tools/bench_aorrtc_multi.py [--reps 3] [--workloads cage,mbm] [--max-iterations 6000] [--internal 500]
                                       [--searches 6] [--resamples 4] [--out FILE]
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
from bench_rrtc_multi import workload_cage, workload_mbm  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402


def run(name, starts, goals, envs, skips, args, log):
    robot = vamp.panda
    n = len(envs)
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    base = dict(range=1.0, max_iterations=args.max_iterations, max_internal_iterations=args.internal, max_samples=8192,
                max_cost_bound_resamples=args.resamples, max_searches=args.searches)
    variants = {"first_only": planning.AORRTCMultiSettings(optimize=False, **base),
                "aorrtc": planning.AORRTCMultiSettings(optimize=True, **base)}
    call = lambda s: planning.aorrtc_multi(robot, starts, goals, envs, s, skips)
    results = {k: call(s) for k, s in variants.items()}  # warm-up, and the results that are reported
    times = {k: [] for k in variants}
    for rep in range(args.reps):
        order = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for k in order:
            t0 = time.perf_counter()
            call(variants[k])
            times[k].append((time.perf_counter() - t0) * 1e3)
    rec = {"workload": name, "problems": n, "settings": base}
    for k, res in results.items():
        solved = [r for r in res if len(r.path) > 0]
        searched = [r for r in solved if r.searches > 0]
        improved = [r for r in solved if r.improvements > 0]
        ratio = lambda rs: round(float(np.median([r.cost / r.first_cost for r in rs])), 4) if rs else None
        rec[k] = {"median_ms": round(statistics.median(times[k]), 3), "windows_ms": [round(t, 3) for t in times[k]],
                  "solved": len(solved), "direct": sum(len(r.path) == 2 for r in solved), "searched": len(searched),
                  "improved": len(improved), "share_improved_of_solved": round(len(improved) / max(len(solved), 1), 4),
                  "share_improved_of_searched": round(len(improved) / max(len(searched), 1), 4),
                  "median_cost_ratio_solved": ratio(solved), "median_cost_ratio_searched": ratio(searched),
                  "median_cost_ratio_improved": ratio(improved),
                  "mean_first_cost": round(float(np.mean([r.first_cost for r in solved])), 4) if solved else None,
                  "mean_cost": round(float(np.mean([r.cost for r in solved])), 4) if solved else None,
                  "searches": int(sum(r.searches for r in res)), "improvements": int(sum(r.improvements for r in res)),
                  "rounds": res[0].validity_calls, "questions": res[0].edges_checked}
    rec["time_ratio_aorrtc_over_first_only"] = round(rec["aorrtc"]["median_ms"] / rec["first_only"]["median_ms"], 3)
    same = all(a.first_cost == b.first_cost or (a.first_cost != a.first_cost) for a, b in zip(results["aorrtc"], results["first_only"]))
    rec["first_costs_equal_in_both"] = bool(same)
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="cage,mbm")
    ap.add_argument("--max-iterations", type=int, default=6000)
    ap.add_argument("--internal", type=int, default=500, help="max_internal_iterations")
    ap.add_argument("--searches", type=int, default=6, help="max_searches")
    ap.add_argument("--resamples", type=int, default=4, help="max_cost_bound_resamples")
    ap.add_argument("--out", default=None, help="text file for the records (one JSON line per workload)")
    args = ap.parse_args()
    vamp.set_device(0)
    lines = []

    def log(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name in args.workloads.split(","):
        run(name, *{"mbm": workload_mbm, "cage": workload_cage}[name](), args, log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/bench_aorrtc_multi.py, one MI355X; times are host clocks around whole calls (ms)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
