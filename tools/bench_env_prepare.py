#!/usr/bin/env python3
"""Measurement of the robot part of many environments (broad-phase grids, reach certificates, static links): built in
one vmv_env_prepare_multi call on the device ("batch") against built by each environment's first use, one by one on the
host ("lazy": one one-configuration vmv_validate_batch per environment; "multi_first": one vmv_validate_batch_multi
over fresh environments, which is how the first-use figures of tools/bench_multi_env.py were taken).

Shapes:
  mbm      the MotionBenchMaker fixture (tests/golden/mbm_<robot>.npz): 1,300 scenes per robot (Panda, UR5, Fetch)
  shell64  64 distinct shell64 scenes (32 spheres + 32 cuboids), Panda
  random   4,096 randomised scenes of 16 mixed primitives, Panda

A robot part is built once per environment, so every repetition constructs and finalizes fresh environments (timed
apart, host clock); the variants alternate within a repetition (A B, B A, ...).  Before the first timed window every
kernel and the first launch of the process are warmed on throwaway environments.  Times are host wall clock around the
call(s), which end synchronised (the calls are synchronous; the lazy loop is followed by a device synchronise).

--package-root DIR imports vamp_mvt_amd from another checkout, e.g. a build of the parent commit, so that its first use
can be measured by the same script in the same session (it has no "batch" variant: use --variants lazy,multi_first).

    python tools/bench_env_prepare.py [--reps 3] [--shapes mbm,shell64,random] [--variants lazy,batch] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VP = ctypes.c_void_p


def load(package_root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(package_root))
    import torch
    import vamp_mvt_amd as vamp

    return torch, vamp


def specs_for(shape, robot, vamp):
    from vamp_mvt_amd.workloads import shell_spec

    if shape == "mbm":
        from test_mbm import problem_primitives

        g = np.load(os.path.join(ROOT, "tests", "golden", f"mbm_{robot}.npz"))
        return [problem_primitives(vamp, g, i) for i in range(len(g["names"]))]
    if shape == "shell64":
        return [shell_spec(s, 32, 32, 0.45, 0.95) for s in range(64)]
    from envs import counted_spec

    return [counted_spec(robot, (4, 3, 3, 3, 3), seed=1000 + s) for s in range(4096)]


def run_shape(torch, vamp, shape, robot, variants, reps, log):
    from vamp_mvt_amd import _lib
    from vamp_mvt_amd._lib import check
    from vamp_mvt_amd.workloads import environment_from_spec

    L = _lib.lib
    mod = getattr(vamp, robot)
    rid, dim = mod._id, mod.dimension()
    specs = specs_for(shape, robot, vamp)
    n = len(specs)
    q = torch.zeros((n, dim), dtype=torch.float32, device="cuda")
    bits = torch.zeros(n, dtype=torch.int64, device="cuda")
    offsets = np.arange(n + 1, dtype=np.uint64)
    stream = VP(torch.cuda.current_stream().cuda_stream)

    def fresh(which=slice(None)):
        t0 = time.perf_counter()
        envs = [environment_from_spec(s) for s in specs[which]]
        handles = (VP * len(envs))(*[e.handle() for e in envs])  # build + finalize (upload)
        return envs, handles, time.perf_counter() - t0

    def lazy(handles, m):
        for k in range(m):
            check(L.vmv_validate_batch(rid, handles[k], VP(q.data_ptr()), 1, VP(bits.data_ptr() + 8 * k), stream),
                  "vmv_validate_batch")

    def multi_first(handles, m):
        check(L.vmv_validate_batch_multi(rid, handles, offsets.ctypes.data_as(_lib.c_size_p), m, VP(q.data_ptr()),
                                         VP(bits.data_ptr()), stream), "vmv_validate_batch_multi")

    def batch(handles, m):
        check(L.vmv_env_prepare_multi(rid, handles, m), "vmv_env_prepare_multi")

    fns = {"lazy": lazy, "multi_first": multi_first, "batch": batch}
    for name in variants:  # warm-up on throwaway environments: first launches, code objects, allocator
        envs, handles, _ = fresh(slice(0, min(n, 8)))
        fns[name](handles, len(envs))
        if name == "batch":
            lazy(handles, len(envs))  # (warms the validate kernels that follow a prepare in real use)
        torch.cuda.synchronize()
    raw = {name: [] for name in variants}
    build = []
    for r in range(reps):
        for name in (variants if r % 2 == 0 else variants[::-1]):
            envs, handles, build_s = fresh()
            build.append(build_s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[name](handles, n)
            torch.cuda.synchronize()
            raw[name].append(time.perf_counter() - t0)
            del envs, handles
    rec = {"shape": shape, "robot": robot, "scenes": n, "reps": reps, "library": _lib.LIB_PATH,
           "build_finalize_s": {"median": round(statistics.median(build), 4), "all": [round(b, 4) for b in build]}}
    for name, v in raw.items():
        rec[name] = {"median_s": statistics.median(v), "min_s": min(v), "per_scene_ms": 1e3 * statistics.median(v) / n,
                     "windows_s": [round(x, 5) for x in v]}
    if "batch" in raw:
        for other in ("lazy", "multi_first"):
            if other in raw:
                rec[f"{other}_over_batch"] = rec[other]["median_s"] / rec["batch"]["median_s"]
    log(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="mbm,shell64,random")
    ap.add_argument("--robots", default="panda,ur5,fetch", help="robots of the mbm shape")
    ap.add_argument("--variants", default="lazy,batch")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None, help="JSON file for the records")
    args = ap.parse_args()
    torch, vamp = load(args.package_root)
    vamp.set_device(0)
    torch.cuda.init()
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    variants = args.variants.split(",")
    for shape in args.shapes.split(","):
        for robot in (args.robots.split(",") if shape == "mbm" else ["panda"]):
            run_shape(torch, vamp, shape, robot, variants, args.reps, log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
