#!/usr/bin/env python3
"""Measurement of planning.aorrtc_multi_constrained (cost-bounded searches inside the band of an end-effector constraint,
DESIGN §5s) against what a constrained caller had before it.

Workloads (tools/bench_rrtc_constrained.py's, Panda under EEConstraint.upright(z, 0.2) with endpoints from
planning.project_goals; only files of this tree are read):
  cage   the sphere cage, 1,024 problems that differ in their Halton skip, between the first two projected, collision-free
         Halton configurations of tests/constraint_serial.py's set;
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: the problems that keep both endpoints (counted).
Three variants, in alternated, warmed windows of one session (host clock around synchronous calls):
  constrained   aorrtc_multi_constrained with `optimize`;
  first         the same call with optimize=False: the first solution, simplified in the band - what a constrained caller
                could get before (rrtc_multi_constrained then simplify_multi_constrained);
  remedy        aorrtc_multi, which does not know the constraint, followed by validate_paths_constrained over what it
                returns: how many of its results are usable at all.
Recorded: time per call and the ratio constrained / first, rounds, questions, how many problems the searches improved, the
sum of final costs over the sum of first costs (solved problems), the questions the band refused; for `remedy` how many of
its solved paths are valid and in band.  No figure is fixed in advance.

    python tools/bench_aorrtc_constrained.py [--reps 3] [--workloads cage,mbm] [--range 0.5] [--out FILE.json]
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


def paths_of(raw):
    ends = np.cumsum(raw["path_lengths"], dtype=np.int64)
    return [raw["paths"][ends[p] - int(raw["path_lengths"][p]):ends[p]] for p in range(len(ends))]


def measure(name, starts, goals, envs, skips, args):
    robot = vamp.panda
    up = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    n_all = len(envs)
    ps = planning.project_goals(robot, [s[None] for s in starts], up, list(envs))
    pg = planning.project_goals(robot, [g[None] for g in goals], up, list(envs))
    keep = [p for p in range(n_all) if len(ps[p]) and len(pg[p])]
    a = np.stack([ps[p][0] for p in keep])
    b = np.stack([pg[p][0] for p in keep])
    e, sk = [envs[p] for p in keep], [int(skips[p]) for p in keep]
    robot.prepare(e)
    common = dict(range=args.range, max_iterations=args.max_iterations, max_internal_iterations=args.max_internal_iterations,
                  max_samples=args.max_samples, max_searches=args.max_searches, max_cost_bound_resamples=args.max_cost_bound_resamples,
                  simplify=planning.SimplifyMultiSettings())
    s_on, s_off = planning.AORRTCMultiSettings(**common), planning.AORRTCMultiSettings(optimize=False, **common)

    def remedy():
        raw = robot.aorrtc_multi_raw(a, b, e, s_on, sk)
        solved = np.flatnonzero(raw["status"] == 0)
        paths = paths_of(raw)
        valid, in_band = planning.validate_paths_constrained(robot, [paths[p] for p in solved], [e[p] for p in solved], up)
        raw["usable"] = int((np.asarray(valid) & np.asarray(in_band)).sum())
        raw["valid"], raw["in_band"] = int(np.asarray(valid).sum()), int(np.asarray(in_band).sum())
        return raw

    variants = {"constrained": lambda: robot.aorrtc_multi_constrained_raw(a, b, e, up, s_on, skips=sk),
                "first": lambda: robot.aorrtc_multi_constrained_raw(a, b, e, up, s_off, skips=sk),
                "remedy": remedy}
    raws = {k: fn() for k, fn in variants.items()}  # warm-up, and the results
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.reps):
        for k in (names if r % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    row = dict(workload=name, problems=n_all, with_endpoints_in_band=len(keep), settings={k: v for k, v in common.items() if k != "simplify"})
    for k, raw in raws.items():
        ms = statistics.median(times[k])
        solved = raw["status"] == 0
        row[k] = dict(ms_per_call=round(ms, 3), windows_ms=[round(t, 3) for t in times[k]], rounds=int(raw["rounds"]),
                      questions=int(raw["questions"]), solved=int(solved.sum()), searches=int(raw["searches"].sum()),
                      improved=int((raw["improvements"] > 0).sum()),
                      first_cost_sum=round(float(raw["first_costs"][solved].astype(np.float64).sum()), 4),
                      cost_sum=round(float(raw["costs"][solved].astype(np.float64).sum()), 4),
                      mean_waypoints_of_solved=round(float(raw["path_lengths"][solved].mean()) if solved.any() else 0.0, 2))
        row[k]["final_over_first_cost"] = round(row[k]["cost_sum"] / row[k]["first_cost_sum"], 4) if row[k]["first_cost_sum"] > 0 else None
        if "band_refused" in raw:
            row[k]["questions_refused_by_the_band"] = int(raw["band_refused"].sum())
    c, f = raws["constrained"], raws["first"]
    row["time_ratio_constrained_over_first"] = round(row["constrained"]["ms_per_call"] / row["first"]["ms_per_call"], 3)
    row["first_stage_agrees"] = bool(np.array_equal(c["first_costs"].view(np.uint32), f["first_costs"].view(np.uint32)))
    valid, in_band = planning.validate_paths_constrained(robot, [p for p, st in zip(paths_of(c), c["status"]) if st == 0],
                                                         [e[p] for p in np.flatnonzero(c["status"] == 0)], up)
    row["constrained"]["resampled_valid_and_in_band"] = int((np.asarray(valid) & np.asarray(in_band)).sum())  # (not promised: DESIGN 5s)
    row["remedy"].update(usable=raws["remedy"]["usable"], valid=raws["remedy"]["valid"], in_band=raws["remedy"]["in_band"])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="cage,mbm")
    ap.add_argument("--range", type=float, default=0.5)
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--max-internal-iterations", type=int, default=500)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--max-searches", type=int, default=4)
    ap.add_argument("--max-cost-bound-resamples", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_aorrtc_constrained.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    rows = []
    for name in args.workloads.split(","):
        w = list({"mbm": workload_mbm, "cage": workload_cage}[name]())
        if name == "cage":
            import constraint_serial

            (ends,) = planning.project_goals(vamp.panda, [constraint_serial.configs("panda", 96)],
                                             vamp.EEConstraint.upright((0, 0, 1), 0.2), w[2][0])
            w[0], w[1] = np.tile(ends[0], (len(w[2]), 1)), np.tile(ends[1], (len(w[2]), 1))
        rows.append(measure(name, *w, args))
    result = {"tool": "tools/bench_aorrtc_constrained.py", "constraint": "upright(z, 0.2)", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
