#!/usr/bin/env python3
"""Measurement of planning.rrtc_multi (many RRT-Connect problems in lockstep on the device, one call) against the way the
same work was done before it: a loop of planning.rrtc, one problem at a time, with the same settings.

Workloads (only files of this tree are read):
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Environments are built, finalized and prepared for the robot outside the timed region; the loop's samplers are built and
skipped outside it too.  Both methods end synchronised with the device (host buffers in, host results out), so every time
is a host clock around a window; windows alternate between the two methods and are warmed first.  The loop is slow
(tens of milliseconds per plan), so by default it runs an evenly spaced subset of the problems (--loop-problems, 0 = all)
and is compared per problem; the lockstep call always runs all of them, and is also timed on that same subset.
Agreement of the solved sets is reported, not asserted: planning.rrtc computes in float64 intermediates and may take
another decision than the fp32 contract of rrtc_multi.  --dynamic-domain and --goals G measure the lockstep
call with the reference's dynamic domain, and with G goals per problem (planning.rrtc_multi_goals); the loop takes the
same goal arrays but has no dynamic domain.

    python tools/bench_rrtc_multi.py [--reps 3] [--workloads mbm,cage] [--loop-problems 64] [--dynamic-domain] [--goals G]
                                     [--out DIR]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vamp_mvt_amd as vamp  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402
from vamp_mvt_amd.workloads import environment_from_spec  # noqa: E402


def workload_mbm():
    from test_mbm import problem_primitives

    g = np.load(os.path.join(ROOT, "tests", "golden", "mbm_panda.npz"))
    n = len(g["names"])
    envs = [environment_from_spec(problem_primitives(vamp, g, i)) for i in range(n)]
    return (np.ascontiguousarray(g["start"], np.float32), np.ascontiguousarray(g["goal"], np.float32), envs,
            np.zeros(n, np.int64))


def workload_cage(n=1024):
    from envs import spec_for
    from oracle_lib import CAGE_GOAL, CAGE_START

    env = environment_from_spec(spec_for("cage"))
    return (np.tile(np.array(CAGE_START, np.float32), (n, 1)), np.tile(np.array(CAGE_GOAL, np.float32), (n, 1)),
            [env] * n, np.arange(n, dtype=np.int64))


def goal_sets(robot, goals, envs, count, seed=29):
    """per problem its own goal and count - 1 configurations valid in its environment, drawn uniformly with a fixed seed"""
    n, dim, tries = len(envs), goals.shape[1], 256 * (count - 1)  # (about 1 in 25 uniform draws is valid in the sphere cage)
    rng = np.random.default_rng(seed)
    q = (robot._lower + robot._span * rng.random((n * tries, dim), dtype=np.float32)).astype(np.float32)
    ok = robot.validate_batch_multi(q, envs, [tries] * n).reshape(n, tries)
    q = q.reshape(n, tries, dim)
    sets = []
    for p in range(n):
        extra = q[p][ok[p]][:count - 1]
        if len(extra) != count - 1:
            raise RuntimeError(f"problem {p}: {len(extra)} of {tries} drawn configurations are valid, {count - 1} are needed")
        sets.append(np.concatenate([goals[p:p + 1], extra]))
    return sets


def run(name, starts, goals, envs, skips, args, log):
    robot = vamp.panda
    n = len(envs)
    s = planning.RRTCMultiSettings(range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples,
                                   check_every=args.check_every, dynamic_domain=args.dynamic_domain)
    s1 = planning.RRTCSettings(range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples)
    t0 = time.perf_counter()
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    prepare_s = time.perf_counter() - t0
    if args.goals > 1:  # goal sets: rrtc_multi_goals against the loop of planning.rrtc with the same goal arrays
        sets = goal_sets(robot, goals, envs, args.goals)
        goals = np.empty(n, object)
        goals[:] = sets

        def rrtc_multi(starts, goals, envs, s, skips):
            return planning.rrtc_multi_goals(robot, starts, list(goals), envs, s, skips)
    else:
        def rrtc_multi(starts, goals, envs, s, skips):
            return planning.rrtc_multi(robot, starts, goals, envs, s, skips)
    sub = np.arange(n) if args.loop_problems <= 0 or args.loop_problems >= n else \
        np.unique(np.linspace(0, n - 1, args.loop_problems).astype(np.int64))
    samplers = []
    for i in sub:
        h = planning.Halton(robot)
        h.skip(int(skips[i]))
        samplers.append(h)

    def multi_all():
        return rrtc_multi(starts, goals, envs, s, skips)

    def multi_sub():
        return rrtc_multi(starts[sub], goals[sub], [envs[i] for i in sub], s, skips[sub])

    def loop_sub():
        fresh = copy.deepcopy(samplers)  # (a run consumes its sampler; the copy is cheap next to the plans)
        return [planning.rrtc(robot, starts[i], goals[i], envs[i], s1, fresh[k]) for k, i in enumerate(sub)]

    variants = {"multi_all": multi_all, "multi_subset": multi_sub, "loop_subset": loop_sub}
    results = {k: f() for k, f in variants.items()}  # warm-up, and the results that are reported
    times = {k: [] for k in variants}
    for rep in range(args.reps):
        order = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for k in order:
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)

    def summary(k, count):
        solved = sum(r.solved for r in results[k])
        med = statistics.median(times[k])
        return {"problems": count, "solved": solved, "median_ms": round(med, 3), "min_ms": round(min(times[k]), 3),
                "windows_ms": [round(t, 3) for t in times[k]], "ms_per_problem": round(med / count, 5),
                "ms_per_solved_plan": round(med / max(solved, 1), 5)}

    rec = {"workload": name, "settings": {"range": s.range, "max_iterations": s.max_iterations, "max_samples": s.max_samples,
                                          "check_every": s.check_every, "dynamic_domain": s.dynamic_domain, "goals": args.goals},
           "prepare_s": round(prepare_s, 3),
           "multi_all": summary("multi_all", n), "multi_subset": summary("multi_subset", len(sub)),
           "loop_subset": summary("loop_subset", len(sub))}
    for k, count in (("multi_all", n), ("multi_subset", len(sub))):
        rounds, questions = results[k][0].validity_calls, results[k][0].edges_checked
        rec[k].update({"rounds": rounds, "questions": questions,
                       "mean_us_per_round": round(rec[k]["median_ms"] * 1e3 / max(rounds, 1), 3),
                       "status": {st: sum(r.status == st for r in results[k]) for st in planning.PLAN_STATUS}})
    rec["loop_subset"]["validity_calls"] = sum(r.validity_calls for r in results["loop_subset"])
    both = [(a.solved, b.solved) for a, b in zip(results["multi_subset"], results["loop_subset"])]
    rec["subset_agreement"] = {"both_solved": sum(a and b for a, b in both), "only_multi": sum(a and not b for a, b in both),
                               "only_loop": sum(b and not a for a, b in both), "neither": sum(not a and not b for a, b in both)}
    rec["same_in_batch_and_subset"] = all(
        results["multi_all"][i].iterations == r.iterations and len(results["multi_all"][i].path) == len(r.path)
        for i, r in zip(sub, results["multi_subset"]))
    rec["loop_over_multi_all_per_problem"] = round(rec["loop_subset"]["ms_per_problem"] / rec["multi_all"]["ms_per_problem"], 1)
    rec["loop_over_multi_subset"] = round(rec["loop_subset"]["median_ms"] / rec["multi_subset"]["median_ms"], 1)
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--loop-problems", type=int, default=64, help="problems of the planning.rrtc loop (0 = all)")
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=8192)
    ap.add_argument("--check-every", type=int, default=0)
    ap.add_argument("--dynamic-domain", action="store_true",
                    help="the reference's dynamic domain (radius 4, alpha 0.0001, min_radius 1); the loop of planning.rrtc has none")
    ap.add_argument("--goals", type=int, default=1,
                    help="goals per problem: its own and G - 1 valid configurations drawn with a fixed seed (rrtc_multi_goals)")
    ap.add_argument("--out", default=None, help="directory for rrtc_multi_bench.json")
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
        with open(os.path.join(args.out, "rrtc_multi_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
