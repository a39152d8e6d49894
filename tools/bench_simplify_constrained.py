#!/usr/bin/env python3
"""Measurement of planning.simplify_multi_constrained (the lockstep simplifier inside the band of an end-effector
constraint) against what a caller could do before it: planning.simplify_multi on the same paths, followed by
planning.validate_paths_constrained to find out which results left the band.

Workload (only files of this tree are read): tools/bench_rrtc_constrained.py's `cage` - the Panda sphere cage, 1,024
problems that differ in their Halton skip, between the first two projected, collision-free Halton configurations of
tests/constraint_serial.py's set, under EEConstraint.upright(z, 0.2) at range 0.5.  The inputs are the solved paths
planning.rrtc_multi_constrained returns for it.  Variants, timed in alternated windows after one warm-up each:
  plan          rrtc_multi_constrained itself on the cage (the paths' source; timed for comparisons between builds);
  plain         simplify_multi on the paths;
  plain_check   simplify_multi followed by validate_paths_constrained on its results: time, and the share of paths that
                are no longer in band (or no longer valid);
  constrained   simplify_multi_constrained: time, rounds, questions against band_refused, status counts, cost ratio
                final / input.
All end synchronised with the device (host buffers in, host results out), so every time is a host clock around a window.
The share of projected B-spline candidates that converged is not counted on the device: it is read off the serial
statement (tests/simplify_constrained_serial.py, the product answering every question) on an evenly spaced subset of the
paths, whose results are also compared with the device's.  No figure is fixed in advance.

    python tools/bench_simplify_constrained.py [--reps 5] [--serial-paths 8] [--existing-only] [--out FILE.json]

--existing-only times `plan` and `plain` alone: what a build without the constrained simplifier can run as well.
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
from bench_rrtc_multi import workload_cage  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--range", type=float, default=0.5)
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--max-samples", type=int, default=1024)
    ap.add_argument("--serial-paths", type=int, default=8, help="paths re-run through the serial statement (0 = none)")
    ap.add_argument("--existing-only", action="store_true", help="time rrtc_multi_constrained and simplify_multi alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_simplify_constrained.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    import constraint_serial

    robot = vamp.panda
    up = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    _, _, envs, skips = workload_cage(args.problems)
    (ends,) = planning.project_goals(robot, [constraint_serial.configs("panda", 96)], up, envs[0])
    starts, goals = np.tile(ends[0], (len(envs), 1)), np.tile(ends[1], (len(envs), 1))
    robot.prepare(envs)
    rs = planning.RRTCMultiSettings(range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples)

    def plan():
        return planning.rrtc_multi_constrained(robot, starts, [g[None] for g in goals], envs, up, rs, skips=[int(k) for k in skips])

    plans = plan()
    solved = [i for i, r in enumerate(plans) if r.solved]
    paths = [np.stack(plans[i].path) for i in solved]
    penvs = [envs[i] for i in solved]
    n = len(paths)
    s = planning.SimplifyMultiSettings()

    def plain():
        return planning.simplify_multi(robot, paths, penvs, s)

    def plain_check():
        out = planning.simplify_multi(robot, paths, penvs, s)
        return out, planning.validate_paths_constrained(robot, [r.path for r in out], penvs, up)

    def constrained():
        return planning.simplify_multi_constrained(robot, paths, penvs, up, s)

    variants = {"plan": plan, "plain": plain}
    if not args.existing_only:
        variants.update(plain_check=plain_check, constrained=constrained)
    results, times = timed(variants, args.reps)

    def summary(k):
        return {"median_ms": round(statistics.median(times[k]), 3), "min_ms": round(min(times[k]), 3),
                "windows_ms": [round(t, 3) for t in times[k]]}

    cost_in = np.array([planning.path_cost(list(p)) for p in paths], np.float64)
    rec = {"tool": "tools/bench_simplify_constrained.py", "constraint": "upright(z, 0.2)", "workload": "cage", "range": args.range,
           "problems": len(envs), "solved_paths": n, "reps": args.reps,
           "input": {"mean_waypoints": round(float(np.mean([len(p) for p in paths])), 3), "mean_cost": round(float(cost_in.mean()), 4)},
           "plan": summary("plan"), "plain": summary("plain")}
    r = results["plain"]
    rec["plain"].update(rounds=r[0].validity_calls, questions=r[0].edges_checked,
                        mean_waypoints=round(float(np.mean([len(x.path) for x in r])), 3),
                        cost_ratio=round(float(sum(x.cost for x in r) / cost_in.sum()), 4))
    if not args.existing_only:
        out, (valid, in_band) = results["plain_check"]
        rec["plain_check"] = summary("plain_check")
        rec["plain_check"].update(paths_left_the_band=int((~in_band).sum()), share_left_the_band=round(float((~in_band).mean()), 4),
                                  paths_no_longer_valid=int((~valid).sum()),
                                  share_usable=round(float((valid & in_band).mean()), 4))
        r = results["constrained"]
        ok = [i for i, x in enumerate(r) if x.status != "out_of_band"]
        rec["constrained"] = summary("constrained")
        rec["constrained"].update(
            rounds=r[0].validity_calls, questions=r[0].edges_checked, band_refused=int(sum(x.band_refused for x in r)),
            us_per_round=round(rec["constrained"]["median_ms"] * 1e3 / max(r[0].validity_calls, 1), 2),
            status={st: sum(x.status == st for x in r) for st in planning.SIMPLIFY_STATUS},
            mean_iterations=round(float(np.mean([x.iterations for x in r])), 3),
            mean_waypoints=round(float(np.mean([len(x.path) for x in r])), 3),
            cost_ratio=round(float(sum(r[i].cost for i in ok) / cost_in[ok].sum()), 4) if ok else None)
        valid2, band2 = planning.validate_paths_constrained(robot, [x.path for x in r], penvs, up)
        rec["constrained"].update(paths_left_the_band=int((~band2).sum()), paths_no_longer_valid=int((~valid2).sum()))
        rec["constrained_over_plain_check"] = round(rec["constrained"]["median_ms"] / rec["plain_check"]["median_ms"], 3)
        if args.serial_paths > 0 and n > 0:
            from simplify_constrained_serial import product_hooks, simplify_constrained_serial

            sub = np.unique(np.linspace(0, n - 1, min(args.serial_paths, n)).astype(np.int64))
            asked = refused = projected = converged = moved = replaced = 0
            same = True
            for i in sub:
                env = penvs[i]
                w = simplify_constrained_serial(list(paths[i]), lambda a, b, env=env: bool(robot.validate_motion_batch(a[None], b[None], env)[0]),
                                                product_hooks(robot, up), max_waypoints=s.max_waypoints)
                same = same and [q.tobytes() for q in w.path] == [np.asarray(q, np.float32).tobytes() for q in r[i].path] and \
                    w.band_refused == r[i].band_refused
                asked, refused = asked + w.questions, refused + w.band_refused
                projected, converged = projected + len(w.projected), converged + sum(c for _, _, c, _, _ in w.projected)
                moved, replaced = moved + sum(m for *_, m, _ in w.projected), replaced + sum(x for *_, x in w.projected)
            rec["serial_subset"] = dict(paths=len(sub), same_as_device=bool(same), questions_asked_serially=asked, band_refused=refused,
                                        candidates_projected=projected, converged=converged,
                                        share_converged=round(converged / projected, 4) if projected else None,
                                        moved_by_the_projection=moved, replaced_their_waypoint=replaced)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
