#!/usr/bin/env python3
"""Measurement of planning.prm_multi (a roadmap per problem for many problems, one call, a fixed number of launches)
against planning.rrtc_multi on the same problems in the same session, and against the loop of <robot>.prm.

Workloads (only files of this tree are read):
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Environments are built, finalized and prepared for the robot outside the timed region.  Every method ends synchronised
with the device (host buffers in, host results out), so every time is a host clock around a window; windows alternate
between the variants and are warmed first.  The solve rate is reported next to every time: a call that is faster but
solves fewer problems is another trade, not a win.  The loop of <robot>.prm (one problem at a time, the host prototype's
k-NN and A*) runs an evenly spaced subset of the problems (--loop-problems, 0 = none).

    python tools/bench_prm_multi.py [--reps 3] [--workloads mbm,cage] [--samples 512,1024,2048,4096] [--k 8]
                                    [--loop-problems 64] [--loop-max-samples 2048] [--no-rrtc] [--out DIR]
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
    t0 = time.perf_counter()
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    prepare_s = time.perf_counter() - t0
    sizes = [int(x) for x in args.samples.split(",")]
    variants = {}
    for ns in sizes:
        s = planning.PRMMultiSettings(n_samples=ns, k=args.k)
        variants[f"prm_multi_{ns}"] = lambda s=s: planning.prm_multi(robot, starts, goals, envs, s, skips)
    if not args.no_rrtc:  # the settings of profiles/r11_rrtc_multi_bench.txt
        rs = planning.RRTCMultiSettings(range=1.0, max_iterations=10000, max_samples=8192)
        variants["rrtc_multi"] = lambda: planning.rrtc_multi(robot, starts, goals, envs, rs, skips)
    results = {k: f() for k, f in variants.items()}  # warm-up, and the results that are reported
    times = {k: [] for k in variants}
    for rep in range(args.reps):
        order = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for k in order:
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    rec = {"workload": name, "problems": n, "k": args.k, "prepare_s": round(prepare_s, 3)}
    for k in variants:
        res = results[k]
        solved = [r for r in res if len(r.path) > 0]
        med = statistics.median(times[k])
        row = {"solved": len(solved), "median_ms": round(med, 3), "min_ms": round(min(times[k]), 3),
               "windows_ms": [round(t, 3) for t in times[k]], "ms_per_problem": round(med / n, 5),
               "ms_per_solved_plan": round(med / max(len(solved), 1), 5),
               "mean_cost_of_solved": round(float(np.mean([planning.path_cost(r.path) for r in solved])), 4) if solved else None,
               "mean_waypoints_of_solved": round(float(np.mean([len(r.path) for r in solved])), 2) if solved else None,
               "status": {st: sum(r.status == st for r in res) for st in planning.PLAN_STATUS},
               "validation_calls": res[0].validity_calls}
        if k.startswith("prm_multi"):
            row.update({"direct": sum(r.solved and r.iterations == 0 for r in res),
                        "valid_vertices": int(sum(r.size[0] for r in res)), "valid_edges": int(sum(r.size[1] for r in res)),
                        "candidate_edges": int(sum(r.edges_checked for r in res)),
                        "configurations_checked": n * (int(k.rsplit("_", 1)[1]) + 2)})
        else:
            row["questions"] = res[0].edges_checked
        rec[k] = row
    if "rrtc_multi" in variants:  # which problems each method solves
        r_solved = np.array([len(r.path) > 0 for r in results["rrtc_multi"]])
        for ns in sizes:
            p_solved = np.array([len(r.path) > 0 for r in results[f"prm_multi_{ns}"]])
            rec[f"prm_multi_{ns}"]["against_rrtc_multi"] = {
                "both": int((p_solved & r_solved).sum()), "only_prm": int((p_solved & ~r_solved).sum()),
                "only_rrtc": int((~p_solved & r_solved).sum()), "neither": int((~p_solved & ~r_solved).sum())}
    if args.loop_problems > 0:  # <robot>.prm, one problem at a time
        sub = np.unique(np.linspace(0, n - 1, min(args.loop_problems, n)).astype(np.int64))
        settings = vamp.PRMSettings(vamp.PRMNeighborParams(robot.dimension(), robot.space_measure()))
        settings.max_samples = args.loop_max_samples  # (it starts at 512 samples and doubles while unsolved)

        def loop():
            out = []
            for i in sub:
                rng = robot.halton()
                rng.skip(int(skips[i]))
                out.append(robot.prm(starts[i], goals[i], envs[i], settings, rng))
            return out

        robot.prm(starts[sub[0]], goals[sub[0]], envs[sub[0]], settings, robot.halton())  # warm-up
        t0 = time.perf_counter()
        res = loop()
        ms = (time.perf_counter() - t0) * 1e3
        solved = sum(r.solved for r in res)
        rec["prm_loop_subset"] = {"problems": len(sub), "solved": solved, "ms": round(ms, 3), "ms_per_problem": round(ms / len(sub), 4),
                                  "ms_per_solved_plan": round(ms / max(solved, 1), 4), "max_samples": settings.max_samples}
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--samples", default="512,1024,2048,4096", help="n_samples of the prm_multi variants")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--loop-problems", type=int, default=64, help="problems of the <robot>.prm loop (0 = none)")
    ap.add_argument("--loop-max-samples", type=int, default=2048, help="max_samples of the <robot>.prm loop")
    ap.add_argument("--no-rrtc", action="store_true", help="leave rrtc_multi out (a kernel trace of prm_multi alone)")
    ap.add_argument("--out", default=None, help="directory for prm_multi_bench.json")
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
        with open(os.path.join(args.out, "prm_multi_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
