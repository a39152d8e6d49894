#!/usr/bin/env python3
"""Measurement of planning.rrtc_multi_constrained (RRT-Connect inside the band of an end-effector constraint)
against planning.rrtc_multi_goals on the same endpoints without a constraint.

Workloads (tools/bench_rrtc_multi.py's; only files of this tree are read):
  cage   the Panda sphere cage, 1,024 problems that differ in their Halton skip (0 .. 1023).  The cage's own start and goal
         do not survive the projection (upright, they collide), so every problem runs between the first two projected,
         collision-free Halton configurations of tests/constraint_serial.py's set - the cage problem of the GPU test;
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal.
The endpoints are those of the workload projected into the band of EEConstraint.upright(z, 0.2) and collision-checked by
planning.project_goals; a problem whose start or goal does not survive is left out (counted).  Three variants per range:
  constrained   rrtc_multi_constrained under upright(z, 0.2);
  free          rrtc_multi_constrained under a constraint that restricts nothing: rrtc_multi_goals's result, plus the
                extra launch of every round - what that launch costs;
  goals         rrtc_multi_goals on the same endpoints.
All end synchronised with the device (host buffers in, host results out), so every time is a host clock around a window;
the windows alternate between the variants and are warmed first.  Recorded: time per call and per round, rounds, questions,
solved counts, and for `constrained` the share of questions the constraint refused.  No figure is fixed in advance.

    python tools/bench_rrtc_constrained.py [--reps 3] [--workloads cage,mbm] [--ranges 1.0,0.5] [--out FILE.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vamp_mvt_amd as vamp  # noqa: E402
from bench_rrtc_multi import workload_cage, workload_mbm  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402


def measure(name, starts, goals, envs, skips, range_, args):
    robot = vamp.panda
    up, free = vamp.EEConstraint.upright((0, 0, 1), 0.2), vamp.EEConstraint()
    n_all = len(envs)
    ps = planning.project_goals(robot, [s[None] for s in starts], up, list(envs))
    pg = planning.project_goals(robot, [g[None] for g in goals], up, list(envs))
    keep = [p for p in range(n_all) if len(ps[p]) and len(pg[p])]
    a = np.stack([ps[p][0] for p in keep])
    b = np.stack([pg[p][0] for p in keep])
    counts = np.ones(len(keep), np.int64)
    e, sk = [envs[p] for p in keep], [int(skips[p]) for p in keep]
    robot.prepare(e)
    s = planning.RRTCMultiSettings(range=range_, max_iterations=args.max_iterations, max_samples=args.max_samples)
    variants = {"constrained": lambda: robot.rrtc_multi_constrained_raw(a, b, counts, e, up, s, skips=sk),
                "free": lambda: robot.rrtc_multi_constrained_raw(a, b, counts, e, free, s, skips=sk),
                "goals": lambda: robot.rrtc_multi_goals_raw(a, b, counts, e, s, sk)}
    raws = {k: fn() for k, fn in variants.items()}  # warm-up, and the results
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(workload=name, range=range_, problems=n_all, with_endpoints_in_band=len(keep), max_iterations=args.max_iterations,
               max_samples=args.max_samples, free_equals_goals=bool(all(np.array_equal(raws["free"][k], raws["goals"][k])
                                                                      for k in ("status", "iterations", "sizes", "path_lengths", "paths"))))
    for k, raw in raws.items():
        ms = statistics.median(times[k])
        row[k] = dict(ms_per_call=round(ms, 3), windows_ms=[round(t, 3) for t in times[k]], rounds=int(raw["rounds"]),
                      us_per_round=round(ms * 1e3 / max(int(raw["rounds"]), 1), 2), questions=int(raw["questions"]),
                      solved=int((raw["status"] == 0).sum()), max_iterations=int((raw["status"] == 1).sum()),
                      max_samples=int((raw["status"] == 2).sum()), direct=int(((raw["status"] == 0) & (raw["path_lengths"] == 2)).sum()),
                      mean_waypoints_of_solved=round(float(raw["path_lengths"][raw["status"] == 0].mean()) if (raw["status"] == 0).any() else 0.0, 2))
    c = raws["constrained"]
    row["constrained"]["questions_refused_by_the_band"] = int(c["band_refused"].sum())
    row["constrained"]["share_refused"] = round(float(c["band_refused"].sum()) / max(int(c["questions"]), 1), 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="cage,mbm")
    ap.add_argument("--ranges", default="1.0,0.5")
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_rrtc_constrained.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    rows = []
    for name in args.workloads.split(","):
        w = list({"mbm": workload_mbm, "cage": workload_cage}[name]())
        if name == "cage":
            import constraint_serial

            (ends,) = planning.project_goals(vamp.panda, [constraint_serial.configs("panda", 96)],
                                             vamp.EEConstraint.upright((0, 0, 1), 0.2), w[2][0])
            w[0], w[1] = np.tile(ends[0], (len(w[2]), 1)), np.tile(ends[1], (len(w[2]), 1))
        for r in args.ranges.split(","):
            rows.append(measure(name, *w, float(r), args))
    result = {"tool": "tools/bench_rrtc_constrained.py", "constraint": "upright(z, 0.2)", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
