#!/usr/bin/env python3
"""Measurement of planning.retime_multi_constrained (retiming whose blends are repaired corner by corner).

Workloads (only files of this tree are read), the paths as tools/bench_retime.py builds them:
  mbm           the 1,260 simplified MotionBenchMaker Panda plans of tests/golden/mbm_panda.npz, each in its scene;
  cage          the Panda sphere cage x 1,024 (rrtc_multi, simplify_multi);
  cage_upright  the cage x 1,024 under EEConstraint.upright(z, 0.2): rrtc_multi_constrained, simplify_multi_constrained, as
                tools/bench_simplify_constrained.py builds them.
Everything up to the simplified paths is outside the timed region.  Three ways to a trajectory, timed in alternated windows
after one warm-up each (host clock around calls that end synchronised with the device):
  (1) retime_multi alone - and how many of its results are "collision" or leave the band (constraint_check_motion_batch on
      its samples);
  (2) today's remedy: retime_multi, then the failing paths again with stop_at_waypoints=True.  Under a constraint the band
      is checked on both passes' samples inside the window, by this tool's own host code around ONE
      constraint_check_motion_batch per pass - that code's time for the first pass alone is reported beside (2);
  (3) retime_multi_constrained.
For (3): the number complete (and in band by the same check, made outside the window), the distribution of rounds and levels, the duration of every repaired trajectory over its
duration under (2), and the call time over (1) and (2).  There is no time bar: the call has no parent.  --once runs one
retime_multi_constrained call per workload and nothing else (for a kernel trace of its own).

    python tools/bench_retime_constrained.py [--reps 5] [--workloads mbm,cage,cage_upright] [--once] [--out DIR]
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
from bench_retime import ACC, VEL  # noqa: E402
from bench_rrtc_multi import workload_cage, workload_mbm  # noqa: E402


def paths_of(name, args):
    """-> (paths, their environments, the constraint or None)"""
    robot = vamp.panda
    if name == "cage_upright":
        import constraint_serial

        up = vamp.EEConstraint.upright((0, 0, 1), 0.2)
        _, _, envs, skips = workload_cage(1024)
        (ends,) = planning.project_goals(robot, [constraint_serial.configs("panda", 96)], up, envs[0])
        starts, goals = np.tile(ends[0], (len(envs), 1)), np.tile(ends[1], (len(envs), 1))
        robot.prepare(envs)
        plans = planning.rrtc_multi_constrained(robot, starts, [g[None] for g in goals], envs, up, planning.RRTCMultiSettings(
            range=0.5, max_iterations=3000, max_samples=1024), skips=[int(k) for k in skips])
        solved = [i for i, r in enumerate(plans) if r.solved]
        penvs = [envs[i] for i in solved]
        out = planning.simplify_multi_constrained(robot, [np.stack(plans[i].path) for i in solved], penvs, up)
        return [np.stack(r.path) for r in out], penvs, up
    starts, goals, envs, skips = {"mbm": workload_mbm, "cage": workload_cage}[name]()
    robot.prepare(envs)
    plans = planning.rrtc_multi(robot, starts, goals, envs, planning.RRTCMultiSettings(
        range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples), skips)
    solved = [i for i, r in enumerate(plans) if r.solved]
    penvs = [envs[i] for i in solved]
    return [np.stack(r.path) for r in planning.simplify_multi(robot, [plans[i].path for i in solved], penvs)], penvs, None


def run(name, args, log):
    robot = vamp.panda
    paths, penvs, up = paths_of(name, args)
    n = len(paths)
    plain_s, stop_s, new_s = planning.RetimeSettings(), planning.RetimeSettings(stop_at_waypoints=True), planning.RetimeConstrainedSettings()

    def leaves_band(raw):
        """per path: whether some pair of its samples is out of band (one constraint_check_motion_batch over all pairs)"""
        count = len(raw["status"])
        out = np.zeros(count, bool)
        if up is None or count == 0:
            return out
        off, pos = raw["offsets"], raw["positions"]
        first = np.concatenate([np.arange(off[p], off[p + 1] - 1) for p in range(count) if off[p + 1] - off[p] > 1])
        ok = robot.constraint_check_motion_batch(pos[first], pos[first + 1], up)
        owner = np.searchsorted(off, first, side="right") - 1
        np.logical_or.at(out, owner[~ok], True)
        return out

    def alone():
        return robot.retime_multi_raw(paths, VEL, ACC, penvs, plain_s)

    def remedy():
        raw = alone()
        bad = np.flatnonzero((raw["status"] == 1) | leaves_band(raw))
        again = robot.retime_multi_raw([paths[i] for i in bad], VEL, ACC, [penvs[i] for i in bad], stop_s) if len(bad) else None
        return raw, bad, again, None if again is None else leaves_band(again)

    def new():
        return robot.retime_multi_constrained_raw(paths, VEL, ACC, penvs, up, new_s)

    if args.once:
        t0 = time.perf_counter()
        raw = new()
        log({"workload": name, "paths": n, "once_ms": round((time.perf_counter() - t0) * 1e3, 3), "questions": raw["questions"]})
        return
    variants = {"retime_multi": alone, "remedy": remedy, "retime_multi_constrained": new}
    results = {k: f() for k, f in variants.items()}  # warm-up
    times = {k: [] for k in variants}
    for rep in range(args.reps):
        order = list(variants) if rep % 2 == 0 else list(variants)[::-1]
        for k in order:
            t0 = time.perf_counter()
            results[k] = variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)

    def summary(k):
        med = statistics.median(times[k])
        return {"median_ms": round(med, 3), "min_ms": round(min(times[k]), 3), "windows_ms": [round(t, 3) for t in times[k]]}

    raw1 = results["retime_multi"]
    out1 = leaves_band(raw1)
    usable1 = int(((raw1["status"] == 0) & ~out1).sum())
    raw2, bad, again, again_out = results["remedy"]
    duration2 = raw2["duration"].copy()
    usable2 = usable1
    if again is not None:
        duration2[bad] = again["duration"]
        usable2 += int(((again["status"] == 0) & ~again_out).sum())
    raw3 = results["retime_multi_constrained"]
    complete3 = (raw3["status"] == 0) & ~leaves_band(raw3)  # checked as (1) and (2) are, outside the timed window
    t0 = time.perf_counter()
    leaves_band(raw1)
    band_check_ms = (time.perf_counter() - t0) * 1e3  # the tool's own check of one pass, part of every window of (2)
    repaired = np.flatnonzero(complete3 & (raw3["repaired"] > 0))
    ratio = (raw3["duration"][repaired] / duration2[repaired]) if len(repaired) else np.zeros(0)
    levels = raw3["levels"]
    t1, t2, t3 = (statistics.median(times[k]) for k in ("retime_multi", "remedy", "retime_multi_constrained"))
    log({"workload": name, "paths": n, "constraint": None if up is None else "upright(z, 0.2)",
         "settings": {"blend": new_s.blend, "grid_step": new_s.grid_step, "dt": new_s.dt, "blend_halvings": new_s.blend_halvings,
                      "max_rounds": new_s.max_rounds}, "vel_limits": VEL.tolist(), "acc_limits": ACC.tolist(),
         "1_retime_multi": {"status": {planning.RETIME_STATUS[c]: int((raw1["status"] == c).sum()) for c in range(5)},
                            "leave_the_band": int(out1.sum()), "usable": usable1, **summary("retime_multi")},
         "2_remedy": {"retimed_again_with_stops": int(len(bad)), "usable": usable2, "ms_per_usable": round(t2 / max(usable2, 1), 4),
                      "of_which_the_tools_band_check_of_the_first_pass_ms": None if up is None else round(band_check_ms, 3),
                      **summary("remedy")},
         "3_retime_multi_constrained": {
             "status": {planning.RETIME_CONSTRAINED_STATUS[c]: int((raw3["status"] == c).sum()) for c in range(6)},
             "usable": int(complete3.sum()), "complete_but_out_of_band": int(((raw3["status"] == 0) & ~complete3).sum()),
             "ms_per_usable": round(t3 / max(int(complete3.sum()), 1), 4),
             "rounds": {str(r): int((raw3["rounds"] == r).sum()) for r in sorted(set(raw3["rounds"].tolist()))},
             "corner_levels": {str(v): int((levels == v).sum()) for v in sorted(set(levels.tolist()))},
             "paths_repaired": int((raw3["repaired"] > 0).sum()), "paths_with_a_stop": int((raw3["stops"] > 0).sum()),
             "validation_calls": raw3["validation_calls"], "questions": raw3["questions"],
             "repaired_duration_over_remedy": None if not len(ratio) else {
                 "paths": int(len(ratio)), "median": round(float(np.median(ratio)), 4), "mean": round(float(ratio.mean()), 4),
                 "min": round(float(ratio.min()), 4), "max": round(float(ratio.max()), 4), "faster_than_stops": int((ratio < 1).sum()),
                 "slower_than_stops": int((ratio > 1).sum())},
             "time_over_retime_multi": round(t3 / t1, 3), "time_over_remedy": round(t3 / t2, 3), **summary("retime_multi_constrained")}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="mbm,cage,cage_upright")
    ap.add_argument("--once", action="store_true", help="one retime_multi_constrained call per workload and nothing else")
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=8192)
    ap.add_argument("--out", default=None, help="directory for retime_constrained_bench.json")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_retime_constrained.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for name in args.workloads.split(","):
        run(name, args, log)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "retime_constrained_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
