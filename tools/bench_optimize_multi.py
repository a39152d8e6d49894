#!/usr/bin/env python3
"""Measurement of planning.optimize_multi (the clearance-aware covariant gradient iteration for many paths in lockstep on
the device, one call) against the same iteration written on the host, which is what a user could write before
it: per iteration ONE clearance_grad_batch_multi call for the waypoints of all unfinished paths and a numpy update per path
(the tridiagonal solve as a product with the cached dense inverse), per validated iterate ONE validate_motion_batch_multi
call.  The host loop follows the same contract but not its operation order, so its figures are close to, not bit for bit,
the device's.

Workloads (only files of this tree are read): the solved paths of planning.rrtc_multi, simplified by
planning.simplify_multi and densified at the robot's resolution, for
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: 1,300 scenes, each with its start and goal;
  cage   the Panda sphere cage, CAGE_START -> CAGE_GOAL, 1,024 problems that differ in their Halton skip (0 .. 1023).

Everything up to the densified paths is outside the timed region.  Both methods end synchronised with the device (host
buffers in, host results out), so every time is a host clock around a window; windows alternate between the methods and
are warmed first.  --once runs one optimize_multi call per workload and nothing else (for a kernel trace of its own).

    python tools/bench_optimize_multi.py [--reps 3] [--workloads mbm,cage] [--once] [--out DIR]
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


def hinge(v, eps):
    with np.errstate(all="ignore"):
        c = np.where(v < 0, -v + 0.5 * eps, np.where(v <= eps, (v - eps) ** 2 / (2 * eps), 0.0))
        d = np.where(v < 0, -1.0, np.where(v <= eps, (v - eps) / eps, 0.0))
    return c.astype(np.float32), d.astype(np.float32)


def host_loop(robot, paths, envs, s):
    """the iteration of vmv_optimize_multi on the host -> (paths, status, cost_first, cost, clearance_first, clearance)"""
    lower, upper = np.asarray(robot.lower_bounds(), np.float32), np.asarray(robot.upper_bounds(), np.float32)
    n = len(paths)
    X = [np.array(p, np.float32) for p in paths]
    best = [x.copy() for x in X]
    has_best = np.zeros(n, bool)
    cost_first, cost = np.zeros(n, np.float32), np.full(n, np.inf, np.float32)
    clr_first, clr = np.full((n, 2), np.nan, np.float32), np.full((n, 2), np.nan, np.float32)
    inverse = {}
    for x in X:
        m = len(x) - 2
        if m >= 1 and m not in inverse:
            inverse[m] = np.linalg.inv(2 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)).astype(np.float32)
    active = [p for p in range(n) if len(X[p]) >= 3]
    change = np.zeros(n, np.float32)
    for k in range(s.max_iterations + 1):
        if not active:
            break
        counts = [len(X[p]) for p in active]
        values, grads = robot.clearance_grad_batch_multi(np.concatenate([X[p] for p in active]), [envs[p] for p in active], counts)
        validated = k % s.validate_every == 0 or k == s.max_iterations
        if validated:
            ok = robot.validate_motion_batch_multi(np.concatenate([X[p][:-1] for p in active]), np.concatenate([X[p][1:] for p in active]),
                                                   [envs[p] for p in active], [c - 1 for c in counts])
        lo = elo = 0
        keep = []
        for p, c in zip(active, counts):
            x, v, g = X[p], values[lo:lo + c], grads[lo:lo + c]
            ce, de = hinge(v[1:-1, 0], np.float32(s.env_margin))
            cs, ds = hinge(v[1:-1, 1], np.float32(s.self_margin))
            u = np.float32(s.smooth_weight * 0.5) * ((x[1:] - x[:-1]) ** 2).sum(dtype=np.float32) + \
                np.float32(s.env_weight) * ce.sum(dtype=np.float32) + np.float32(s.self_weight) * cs.sum(dtype=np.float32)
            if k == 0:
                cost_first[p], clr_first[p] = u, (np.nanmin(v[:, 0]), np.nanmin(v[:, 1]))
            done = False
            if validated:
                if ok[elo:elo + c - 1].all() and (not has_best[p] or u < cost[p]):
                    has_best[p], best[p], cost[p], clr[p] = True, x.copy(), u, (np.nanmin(v[:, 0]), np.nanmin(v[:, 1]))
                done = k >= s.max_iterations or (k > 0 and change[p] < s.min_change)
            if not done:
                G = np.float32(s.smooth_weight) * (2 * x[1:-1] - x[:-2] - x[2:]) + \
                    (np.float32(s.env_weight) * de)[:, None] * g[1:-1, 0] + (np.float32(s.self_weight) * ds)[:, None] * g[1:-1, 1]
                D = np.float32(-s.step) * (inverse[c - 2] @ G)
                m = np.abs(D).max()
                scale = np.float32(s.max_step) / max(m, np.float32(s.max_step))
                change[p] = m * scale
                x = x.copy()
                x[1:-1] = np.clip(x[1:-1] + D * scale, lower, upper)
                X[p] = x
                keep.append(p)
            lo, elo = lo + c, elo + c - 1
        active = keep
    status = np.where(has_best, 0, 1)
    cost = np.where(has_best, cost, cost_first)
    clr[~has_best] = clr_first[~has_best]
    return best, status, cost_first, cost, clr_first, clr


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


def quality(paths_before, paths_after, status, cost_first, cost, clr_first, clr):
    status = np.asarray(status)
    long_enough = np.array([len(p) >= 3 for p in paths_before])
    return {"ok": int((status == 0).sum()), "no_valid": int((status == 1).sum()), "nonfinite": int((status == 2).sum()),
            "improved": int(((np.asarray(cost) < np.asarray(cost_first)) & (status == 0)).sum()),
            "smallest_env_before": float(np.nanmin(clr_first[long_enough, 0])), "smallest_env_after": float(np.nanmin(clr[long_enough, 0])),
            "median_env_before": float(np.nanmedian(clr_first[long_enough, 0])), "median_env_after": float(np.nanmedian(clr[long_enough, 0])),
            "smallest_self_before": float(np.nanmin(clr_first[long_enough, 1])), "smallest_self_after": float(np.nanmin(clr[long_enough, 1])),
            "paths_with_env_below_1cm_before": int((clr_first[long_enough, 0] < 0.01).sum()),
            "paths_with_env_below_1cm_after": int((clr[long_enough, 0] < 0.01).sum()),
            "mean_path_cost_before": round(float(np.mean([planning.path_cost(list(p)) for p in paths_before])), 5),
            "mean_path_cost_after": round(float(np.mean([planning.path_cost(list(p)) for p in paths_after])), 5)}


def run(name, starts, goals, envs, skips, args, log):
    robot = vamp.panda
    robot.prepare(envs)  # finalize + the robot part of every environment, outside the timed region
    plans = planning.rrtc_multi(robot, starts, goals, envs, planning.RRTCMultiSettings(
        range=args.range, max_iterations=args.max_iterations, max_samples=args.max_samples), skips)
    solved = [i for i, r in enumerate(plans) if r.solved]
    penvs = [envs[i] for i in solved]
    simple = planning.simplify_multi(robot, [plans[i].path for i in solved], penvs)
    s = planning.OptimizeMultiSettings()
    dense = [planning.densify_path(np.stack(r.path), float(robot.resolution())) for r in simple]
    fits = [i for i, p in enumerate(dense) if len(p) <= s.max_waypoints]
    paths, penvs = [dense[i] for i in fits], [penvs[i] for i in fits]
    n, lengths = len(paths), [len(p) for p in paths]

    def multi():
        return robot.optimize_multi_raw(paths, penvs, s)

    if args.once:
        t0 = time.perf_counter()
        raw = multi()
        log({"workload": name, "paths": n, "once_ms": round((time.perf_counter() - t0) * 1e3, 3), "clearance_calls": raw["clearance_calls"],
             "validation_calls": raw["validation_calls"]})
        return

    results, times = timed({"multi": multi, "host_loop": lambda: host_loop(robot, paths, penvs, s)}, args.reps)

    def summary(k):
        med = statistics.median(times[k])
        return {"median_ms": round(med, 3), "min_ms": round(min(times[k]), 3), "windows_ms": [round(t, 3) for t in times[k]],
                "us_per_path": round(med * 1e3 / n, 3)}

    raw = results["multi"]
    off = raw["offsets"]
    after = [raw["points"][off[p]:off[p + 1]] for p in range(n)]
    rec = {"workload": name, "paths": n, "left_out_longer_than_max_waypoints": len(dense) - n,
           "waypoints": {"total": int(sum(lengths)), "mean": round(float(np.mean(lengths)), 2), "max": int(max(lengths))},
           "settings": {k: getattr(s, k) for k in ("max_iterations", "validate_every", "step", "max_step", "min_change", "smooth_weight",
                                                   "env_weight", "self_weight", "env_margin", "self_margin", "max_waypoints")},
           "multi": summary("multi"), "host_loop": summary("host_loop")}
    rec["multi"].update(quality(paths, after, raw["status"], raw["cost_first"], raw["cost"], raw["clearance_first"], raw["clearance"]))
    rec["multi"].update({"clearance_calls": raw["clearance_calls"], "validation_calls": raw["validation_calls"],
                         "mean_iterations": round(float(np.mean(raw["iterations"])), 3),
                         "valid_per_validate_paths": int(planning.validate_paths(robot, after, penvs).sum())})
    h = results["host_loop"]
    rec["host_loop"].update(quality(paths, h[0], h[1], h[2], h[3], h[4], h[5]))
    rec["host_loop_over_multi"] = round(rec["host_loop"]["median_ms"] / rec["multi"]["median_ms"], 2)
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="mbm,cage")
    ap.add_argument("--once", action="store_true", help="one optimize_multi call per workload and nothing else")
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--max-iterations", type=int, default=10000)
    ap.add_argument("--max-samples", type=int, default=8192)
    ap.add_argument("--out", default=None, help="directory for optimize_multi_bench.json")
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
        with open(os.path.join(args.out, "optimize_multi_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
