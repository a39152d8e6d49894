#!/usr/bin/env python3
"""Measurement of planning.build_roadmaps / DeviceRoadmaps.query (roadmaps kept on the device: built once per scene,
asked many times) against planning.prm_multi (a roadmap per problem) over the same pairs at the same n_samples and k, in
the same session.

Workloads (only files of this tree are read), Panda:
  scene  one scene (the sphere cage; the `mixed` scene of tests/envs.py), Q random (start, goal) pairs that validate
         accepts, Q in --queries; one roadmap of n samples (--samples) at k = --k; k_connect in --connect.  prm_multi runs
         the same Q pairs in the same scene, every problem over the same Halton samples (skip 0) as the kept roadmap.
  mbm    the MotionBenchMaker fixture tests/golden/mbm_panda.npz: the 1,300 roadmaps built in ONE call and each problem's
         single query answered in ONE call, at every k_connect; the solved counts next to prm_multi's.

Environments are built, finalized and prepared for the robot outside the timed region.  Every method ends synchronised
with the device (host buffers in, host results out), so every time is a host clock around a window; windows alternate
between the variants and are warmed first.  The solve rate and the mean cost are reported next to every time.

    python tools/bench_roadmaps.py [--reps 3] [--workloads cage,mixed,mbm] [--samples 1024,2048,4096] [--k 8]
                                   [--connect 8,16,32] [--queries 1,64,1024,16384] [--prm-max 16384] [--out DIR]
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
from bench_rrtc_multi import environment_from_spec, workload_mbm  # noqa: E402
from vamp_mvt_amd import planning  # noqa: E402


def windows(variants, reps):
    """-> (the results of one warm-up call of each variant, the times of `reps` alternated windows each, in ms)"""
    results = {k: f() for k, f in variants.items()}
    times = {k: [] for k in variants}
    for rep in range(reps):
        for k in (list(variants) if rep % 2 == 0 else list(variants)[::-1]):
            t0 = time.perf_counter()
            variants[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return results, times


def row(res, ms, n):
    solved = [r for r in res if len(r.path) > 0]
    med = statistics.median(ms)
    return {"solved": len(solved), "direct": sum(r.solved and r.iterations == 0 for r in res), "median_ms": round(med, 3),
            "min_ms": round(min(ms), 3), "windows_ms": [round(t, 3) for t in ms], "ms_per_query": round(med / n, 5),
            "mean_cost_of_solved": round(float(np.mean([r.cost for r in solved])), 4) if solved else None,
            "mean_waypoints_of_solved": round(float(np.mean([len(r.path) for r in solved])), 2) if solved else None,
            "status": {st: sum(r.status == st for r in res) for st in planning.PLAN_STATUS},
            "edges_checked": int(sum(r.edges_checked for r in res))}


def valid_pairs(robot, env, n, seed):
    """n (start, goal) pairs of uniform configurations that validate accepts"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(robot.lower_bounds(), np.float32), np.asarray(robot.upper_bounds(), np.float32)
    out = np.zeros((0, len(lo)), np.float32)
    while len(out) < 2 * n:
        q = (lo + (hi - lo) * rng.random((4 * n + 64, len(lo)), dtype=np.float32)).astype(np.float32)
        out = np.vstack([out, q[robot.validate_batch(q, env)]])
    return np.ascontiguousarray(out[0:2 * n:2]), np.ascontiguousarray(out[1:2 * n:2])


def run_scene(name, args, log):
    from envs import spec_for

    robot = vamp.panda
    env = environment_from_spec(spec_for(name))
    robot.prepare([env])
    connects = [int(x) for x in args.connect.split(",")]
    counts = [int(x) for x in args.queries.split(",")]
    starts, goals = valid_pairs(robot, env, max(counts), 17)
    for ns in (int(x) for x in args.samples.split(",")):
        s = planning.RoadmapsSettings(n_samples=ns, k=args.k)
        _, t = windows({"build": lambda: planning.build_roadmaps(robot, [env], s).close()}, args.reps)
        rec = {"workload": name, "n_samples": ns, "k": args.k, "build_median_ms": round(statistics.median(t["build"]), 3),
               "build_windows_ms": [round(x, 3) for x in t["build"]]}
        with planning.build_roadmaps(robot, [env], s) as handle:
            rec["valid_vertices"], rec["candidate_edges"], rec["valid_edges"] = (int(x[0]) for x in handle.summary())
            for n in counts:
                a, b = starts[:n], goals[:n]
                variants = {f"query_kc{kc}": (lambda kc=kc: handle.query(a, b, None, planning.RoadmapQuerySettings(k_connect=kc)))
                            for kc in connects}
                if n <= args.prm_max:
                    ps = planning.PRMMultiSettings(n_samples=ns, k=args.k)
                    variants["prm_multi"] = lambda: planning.prm_multi(robot, a, b, [env] * n, ps)
                results, times = windows(variants, args.reps)
                rec[f"Q{n}"] = {k: row(results[k], times[k], n) for k in variants}
        log(rec)


def run_mbm(args, log):
    robot = vamp.panda
    starts, goals, envs, skips = workload_mbm()
    n = len(envs)
    robot.prepare(envs)
    connects = [int(x) for x in args.connect.split(",")]
    index = np.arange(n)
    for ns in (int(x) for x in args.samples.split(",")):
        s = planning.RoadmapsSettings(n_samples=ns, k=args.k)
        _, t = windows({"build": lambda: planning.build_roadmaps(robot, envs, s, skips).close()}, args.reps)
        rec = {"workload": "mbm", "roadmaps": n, "n_samples": ns, "k": args.k,
               "build_median_ms": round(statistics.median(t["build"]), 3), "build_windows_ms": [round(x, 3) for x in t["build"]]}
        with planning.build_roadmaps(robot, envs, s, skips) as handle:
            v, c, e = handle.summary()
            rec["valid_vertices"], rec["candidate_edges"], rec["valid_edges"] = int(v.sum()), int(c.sum()), int(e.sum())
            variants = {f"query_kc{kc}": (lambda kc=kc: handle.query(starts, goals, index, planning.RoadmapQuerySettings(k_connect=kc)))
                        for kc in connects}
            ps = planning.PRMMultiSettings(n_samples=ns, k=args.k)
            variants["prm_multi"] = lambda: planning.prm_multi(robot, starts, goals, envs, ps, skips)
            results, times = windows(variants, args.reps)
            rec.update({k: row(results[k], times[k], n) for k in variants})
            p_solved = np.array([len(r.path) > 0 for r in results["prm_multi"]])
            for kc in connects:
                q_solved = np.array([len(r.path) > 0 for r in results[f"query_kc{kc}"]])
                rec[f"query_kc{kc}"]["against_prm_multi"] = {
                    "both": int((q_solved & p_solved).sum()), "only_query": int((q_solved & ~p_solved).sum()),
                    "only_prm_multi": int((~q_solved & p_solved).sum()), "neither": int((~q_solved & ~p_solved).sum())}
        log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="cage,mixed,mbm")
    ap.add_argument("--samples", default="1024,2048,4096", help="n_samples of the roadmaps")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--connect", default="8,16,32", help="k_connect of the query variants")
    ap.add_argument("--queries", default="1,64,1024,16384", help="queries per call in the one-scene workloads")
    ap.add_argument("--prm-max", type=int, default=16384, help="prm_multi runs the calls of at most this many pairs")
    ap.add_argument("--out", default=None, help="directory for roadmaps_bench.json")
    args = ap.parse_args()
    vamp.set_device(0)
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for name in args.workloads.split(","):
        if name == "mbm":
            run_mbm(args, log)
        else:
            run_scene(name, args, log)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "roadmaps_bench.json"), "w") as f:
            json.dump({"reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
