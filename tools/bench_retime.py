#!/usr/bin/env python3
"""Measurement of planning.retime_multi (time-optimal trajectories along many paths, one call on the device).

Workloads (only files of this tree are read): the solved paths of planning.rrtc_multi, simplified by
planning.simplify_multi, for
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Everything up to the simplified paths is outside the timed region.  A call ends synchronised with the device (host buffers
in, host results out), so every time is a host clock around a warmed window, with and without environments.  There is no
parent to compare against: for scale only, the numpy statement (tests/retime_serial.py) is timed on the first paths - an
interpreter's time, not a competitor's.  The velocity and acceleration limits are this tool's choice (no robot model here
carries any).  --once runs one retime_multi call per workload and nothing else (for a kernel trace of its own).

    python tools/bench_retime.py [--reps 5] [--workloads mbm,cage] [--once] [--out DIR]
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
import retime_serial  # noqa: E402

VEL = np.array([2.0, 2.0, 2.0, 2.0, 2.5, 2.5, 2.5], np.float32)  # rad/s
ACC = np.array([5.0, 5.0, 5.0, 5.0, 7.5, 7.5, 7.5], np.float32)  # rad/s^2


def run(name, starts, goals, envs, skips, args, log):
    robot = vamp.panda
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    plans = planning.rrtc_multi(robot, starts, goals, envs, planning.RRTCMultiSettings(
        range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples), skips)
    solved = [i for i, r in enumerate(plans) if r.solved]
    penvs = [envs[i] for i in solved]
    paths = [np.stack(r.path) for r in planning.simplify_multi(robot, [plans[i].path for i in solved], penvs)]
    s = planning.RetimeSettings()
    n = len(paths)

    def call(with_envs):
        return robot.retime_multi_raw(paths, VEL, ACC, penvs if with_envs else None, s)

    if args.once:
        t0 = time.perf_counter()
        raw = call(True)
        log({"workload": name, "paths": n, "once_ms": round((time.perf_counter() - t0) * 1e3, 3), "questions": raw["questions"]})
        return
    raw = call(True)
    call(False)
    times = {True: [], False: []}
    for rep in range(args.reps):
        for with_envs in ((True, False) if rep % 2 == 0 else (False, True)):
            t0 = time.perf_counter()
            call(with_envs)
            times[with_envs].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    objects = planning.retime_multi(robot, paths, VEL, ACC, penvs, s)
    with_objects = (time.perf_counter() - t0) * 1e3
    k = min(n, args.statement_paths)
    t0 = time.perf_counter()
    stated = [retime_serial.retime(p, VEL, ACC, retime_serial.Settings()) for p in paths[:k]]
    statement_ms = (time.perf_counter() - t0) * 1e3
    equal = all(np.array_equal(a.positions.view(np.uint32), b.positions.view(np.uint32)) and
                np.array_equal(a.velocities.view(np.uint32), b.velocities.view(np.uint32)) for a, b in zip(objects[:k], stated))

    def summary(v):
        med = statistics.median(v)
        return {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "windows_ms": [round(t, 3) for t in v], "us_per_path": round(med * 1e3 / n, 3)}

    status = raw["status"]
    log({"workload": name, "paths": n, "waypoints_mean": round(float(np.mean([len(p) for p in paths])), 2),
         "intervals": {"total": int(raw["intervals"].sum()), "mean": round(float(raw["intervals"].mean()), 1), "max": int(raw["intervals"].max())},
         "samples": {"total": int(raw["samples"].sum()), "mean": round(float(raw["samples"].mean()), 1), "max": int(raw["samples"].max())},
         "duration_s": {"mean": round(float(raw["duration"].mean()), 3), "max": round(float(raw["duration"].max()), 3)},
         "status": {planning.RETIME_STATUS[c]: int((status == c).sum()) for c in range(len(planning.RETIME_STATUS))},
         "questions": raw["questions"], "settings": {"blend": s.blend, "grid_step": s.grid_step, "dt": s.dt},
         "vel_limits": VEL.tolist(), "acc_limits": ACC.tolist(),
         "retime_multi_raw_with_envs": summary(times[True]), "retime_multi_raw_without_envs": summary(times[False]),
         "planning_retime_multi_with_result_objects_ms": round(with_objects, 3),
         "numpy_statement_an_interpreters_time": {"paths": k, "ms_per_path": round(statement_ms / k, 3), "equal_bits": bool(equal)}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--once", action="store_true", help="one retime_multi call per workload and nothing else")
    ap.add_argument("--statement-paths", type=int, default=32)
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=8192)
    ap.add_argument("--out", default=None, help="directory for retime_bench.json")
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
        with open(os.path.join(args.out, "retime_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
