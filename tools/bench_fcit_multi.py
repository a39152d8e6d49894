#!/usr/bin/env python3
"""Measurement of planning.fcit_multi (a lazy A* search of the complete graph over each problem's samples, many problems
per call in lockstep rounds) against planning.prm_multi (k = 8) at the same samples and against planning.rrtc_multi, on
the same problems in the same session.

Workloads (only files of this tree are read), as tools/bench_prm_multi.py:
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Environments are built, finalized and prepared for the robot outside the timed region.  Every method ends synchronised
with the device (host buffers in, host results out), so every time is a host clock around a window; windows alternate
between the variants and are warmed first.  Solved counts, questions and rounds are reported next to every time.  The
sweep runs fcit_multi at --sweep-samples with questions_per_round 1, 4, 8 and 16.

    python tools/bench_fcit_multi.py [--reps 3] [--workloads mbm,cage] [--samples 256,512,1024] [--sweep-samples 512]
                                     [--sweep 1,4,8,16] [--questions-per-round 8] [--no-rrtc] [--out DIR]
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
    sweep = [int(x) for x in args.sweep.split(",")] if args.sweep else []
    variants = {}
    for ns in sizes:
        fs = planning.FCITMultiSettings(n_samples=ns, max_iterations=args.max_iterations, questions_per_round=args.questions_per_round)
        ps = planning.PRMMultiSettings(n_samples=ns, k=8)
        variants[f"fcit_multi_{ns}"] = lambda s=fs: planning.fcit_multi(robot, starts, goals, envs, s, skips)
        variants[f"prm_multi_{ns}"] = lambda s=ps: planning.prm_multi(robot, starts, goals, envs, s, skips)
    for w in sweep:
        fs = planning.FCITMultiSettings(n_samples=args.sweep_samples, max_iterations=args.max_iterations, questions_per_round=w)
        variants[f"fcit_multi_{args.sweep_samples}_w{w}"] = lambda s=fs: planning.fcit_multi(robot, starts, goals, envs, s, skips)
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
    rec = {"workload": name, "problems": n, "prepare_s": round(prepare_s, 3), "max_iterations": args.max_iterations}
    for k in variants:
        res = results[k]
        solved = [r for r in res if len(r.path) > 0]
        med = statistics.median(times[k])
        row = {"solved": len(solved), "median_ms": round(med, 3), "windows_ms": [round(t, 3) for t in times[k]],
               "ms_per_problem": round(med / n, 5), "ms_per_solved_plan": round(med / max(len(solved), 1), 5),
               "mean_cost_of_solved": round(float(np.mean([planning.path_cost(r.path) for r in solved])), 4) if solved else None,
               "mean_waypoints_of_solved": round(float(np.mean([len(r.path) for r in solved])), 2) if solved else None,
               "status": {st: sum(r.status == st for r in res) for st in planning.PLAN_STATUS},
               "validation_calls": res[0].validity_calls}
        if k.startswith("fcit_multi"):
            row.update({"questions": res[0].edges_checked, "searches": int(sum(r.iterations for r in res)),
                        "max_searches_of_a_problem": int(max(r.iterations for r in res)),
                        "blocked_edges": int(sum(r.size[1] for r in res)),
                        "known_valid_edges": int(sum(r.known_valid_edges for r in res))})
        elif k.startswith("prm_multi"):
            row["candidate_edges"] = int(sum(r.edges_checked for r in res))
        else:
            row["questions"] = res[0].edges_checked
        rec[k] = row
    for ns in sizes:  # inclusion: what prm_multi solves, fcit_multi solves, at no higher cost
        f, p = results[f"fcit_multi_{ns}"], results[f"prm_multi_{ns}"]
        f_solved, p_solved = np.array([r.solved for r in f]), np.array([r.solved for r in p])
        both = f_solved & p_solved
        rec[f"fcit_multi_{ns}"]["against_prm_multi"] = {
            "both": int(both.sum()), "only_fcit": int((f_solved & ~p_solved).sum()), "only_prm": int((~f_solved & p_solved).sum()),
            "cost_above_prm": int(sum(f[i].cost > p[i].cost * (1 + 1e-4) for i in np.flatnonzero(both))),
            "mean_cost_ratio_where_both": round(float(np.mean([f[i].cost / p[i].cost for i in np.flatnonzero(both)])), 4) if both.any() else None}
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--samples", default="256,512,1024", help="n_samples of the fcit_multi and prm_multi variants")
    ap.add_argument("--sweep", default="1,4,8,16", help="questions_per_round values of the sweep ('' = none)")
    ap.add_argument("--sweep-samples", type=int, default=512)
    ap.add_argument("--max-iterations", type=int, default=100000)
    ap.add_argument("--questions-per-round", type=int, default=8, help="of the fcit_multi rows outside the sweep")
    ap.add_argument("--no-rrtc", action="store_true", help="leave rrtc_multi out")
    ap.add_argument("--out", default=None, help="directory for fcit_multi_bench.json")
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
        with open(os.path.join(args.out, "fcit_multi_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
