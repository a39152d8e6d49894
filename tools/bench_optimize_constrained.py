#!/usr/bin/env python3
"""Measurement of planning.optimize_multi_constrained (the lockstep optimiser inside the band of an end-effector
constraint) against what a caller could do before it: planning.optimize_multi on the same paths, followed by
planning.validate_paths_constrained to find out which results are usable.

Workload (only files of this tree are read): DESIGN §5p's - the Panda sphere cage, 1,024 problems that differ in their
Halton skip under EEConstraint.upright(z, 0.2) at range 0.5, planned by planning.rrtc_multi_constrained and simplified by
planning.simplify_multi_constrained; the inputs are the simplified paths with status "ok".  Default optimiser settings.
Variants, timed in alternated windows after one warm-up each:
  simplify      simplify_multi_constrained on the planned paths (timed for comparisons between builds);
  plain         optimize_multi on the simplified paths (for comparisons between builds);
  plain_check   (a) optimize_multi followed by validate_paths_constrained;
  constrained   (b) optimize_multi_constrained.
For (a) and (b): time, results that are usable - status "ok" and (valid, in band) = (1, 1) -, the median smallest waypoint
clearance before and after, plans closer than 1 cm, the cost ratio U / U_first.  For (b) alone: held, the share of the
run's projections that ran more than one evaluation (read off project_batch on the waypoints of one unprojected step,
iterate 0 -> 1, of every path), and how many of the inputs validate_paths_constrained refuses come back "ok".
All end synchronised with the device (host buffers in, host results out), so every time is a host clock around a window.

    python tools/bench_optimize_constrained.py [--reps 5] [--existing-only] [--out FILE.json]

--existing-only times `simplify` and `plain` alone: what a build without the constrained optimiser can run as well.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vamp_mvt_amd as vamp  # noqa: E402
from bench_rrtc_multi import workload_cage  # noqa: E402
from bench_simplify_constrained import timed  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402


def smallest(r, first):
    c = r.clearance_first if first else r.clearance
    return min(float(c[0]), float(c[1]))


def figures(results, usable):
    """the clearance and cost figures of one variant over the paths that iterated"""
    ran = [r for r in results if np.isfinite(smallest(r, True))]
    before, after = np.array([smallest(r, True) for r in ran]), np.array([smallest(r, False) for r in ran])
    return dict(usable=int(usable.sum()), share_usable=round(float(usable.mean()), 4),
                status={st: sum(r.status == st for r in results) for st in planning.OPTIMIZE_CONSTRAINED_STATUS},
                median_smallest_clearance_before_mm=round(float(np.median(before)) * 1e3, 3),
                median_smallest_clearance_after_mm=round(float(np.median(after)) * 1e3, 3),
                closer_than_1cm_before=int((before < 0.01).sum()), closer_than_1cm_after=int((after < 0.01).sum()),
                cost_ratio=round(float(sum(r.cost for r in ran) / max(sum(r.cost_first for r in ran), 1e-30)), 4),
                mean_iterations=round(float(np.mean([r.iterations for r in ran])), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--existing-only", action="store_true", help="time simplify_multi_constrained and optimize_multi alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_optimize_constrained.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    import constraint_serial

    robot = vamp.panda
    up = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    _, _, envs, skips = workload_cage(args.problems)
    (ends,) = planning.project_goals(robot, [constraint_serial.configs("panda", 96)], up, envs[0])
    starts, goals = np.tile(ends[0], (len(envs), 1)), np.tile(ends[1], (len(envs), 1))
    robot.prepare(envs)
    rs = planning.RRTCMultiSettings(range=0.5, max_iterations=3000, max_samples=1024)
    plans = planning.rrtc_multi_constrained(robot, starts, [g[None] for g in goals], envs, up, rs, skips=[int(k) for k in skips])
    solved = [i for i, r in enumerate(plans) if r.solved]
    planned, penvs = [np.stack(plans[i].path) for i in solved], [envs[i] for i in solved]
    ss = planning.SimplifyMultiSettings()

    def simplify():
        return planning.simplify_multi_constrained(robot, planned, penvs, up, ss)

    simple = simplify()
    ok = [i for i, r in enumerate(simple) if r.status == "ok"]
    paths, oenvs = [np.stack(simple[i].path) for i in ok], [penvs[i] for i in ok]
    n = len(paths)
    valid_in, band_in = planning.validate_paths_constrained(robot, paths, oenvs, up)
    refused_in = ~(valid_in & band_in)
    s = planning.OptimizeMultiSettings()

    def plain():
        return planning.optimize_multi(robot, paths, oenvs, s)

    def plain_check():
        out = planning.optimize_multi(robot, paths, oenvs, s)
        return out, planning.validate_paths_constrained(robot, [r.path for r in out], oenvs, up)

    def constrained():
        return planning.optimize_multi_constrained(robot, paths, oenvs, up, s)

    variants = {"simplify": simplify, "plain": plain}
    if not args.existing_only:
        variants.update(plain_check=plain_check, constrained=constrained)
    results, times = timed(variants, args.reps)

    def summary(k):
        return {"median_ms": round(statistics.median(times[k]), 3), "min_ms": round(min(times[k]), 3),
                "windows_ms": [round(t, 3) for t in times[k]]}

    rec = {"tool": "tools/bench_optimize_constrained.py", "constraint": "upright(z, 0.2)", "workload": "cage", "problems": len(envs),
           "simplified_ok_paths": n, "waypoints": int(sum(len(p) for p in paths)), "reps": args.reps,
           "inputs_refused_by_validate_paths_constrained": int(refused_in.sum()),
           "simplify": summary("simplify"), "plain": summary("plain")}
    if not args.existing_only:
        out, (valid, in_band) = results["plain_check"]
        rec["plain_check"] = summary("plain_check")
        rec["plain_check"].update(figures(out, valid & in_band & np.array([r.status == "ok" for r in out])),
                                  paths_left_the_band=int((~in_band).sum()), paths_no_longer_valid=int((~valid).sum()))
        r = results["constrained"]
        valid2, band2 = planning.validate_paths_constrained(robot, [x.path for x in r], oenvs, up)
        is_ok = np.array([x.status == "ok" for x in r])
        rec["constrained"] = summary("constrained")
        rec["constrained"].update(figures(r, valid2 & band2 & is_ok), ok_results_not_1_1=int((is_ok & ~(valid2 & band2)).sum()),
                                  held_total=int(sum(x.held for x in r)), paths_with_held=int(sum(x.held > 0 for x in r)),
                                  refused_inputs_that_come_back_ok=int((refused_in & is_ok).sum()))
        # one unprojected step of every path that iterates, projected by project_batch: how many lanes ran an evaluation, how many more than one
        stepped = planning.optimize_multi(robot, paths, oenvs, planning.OptimizeMultiSettings(max_iterations=1, validate_every=1))
        inner = np.concatenate([np.stack(x.path)[1:-1] for x in stepped if len(x.path) > 2] + [np.zeros((0, robot.dimension()), np.float32)])
        if len(inner):
            _, _, conv, evals = robot.project_batch(inner.astype(np.float32), up)
            evals = np.asarray(evals)
            rec["constrained"].update(one_step_waypoints=int(len(inner)), one_step_share_moved=round(float((evals > 0).mean()), 4),
                                      one_step_share_more_than_one_evaluation=round(float((evals > 1).mean()), 4),
                                      one_step_share_converged=round(float(np.asarray(conv, bool).mean()), 4))
        rec["constrained_over_plain_check"] = round(rec["constrained"]["median_ms"] / rec["plain_check"]["median_ms"], 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
