#!/usr/bin/env python3
"""Measurement of vmv_validate_motion_batch_multi (edges against many environments in one call) against one
vmv_validate_motion_batch per environment, on prebuilt, warmed environments, through the C ABI's device entry points on
one torch stream.  The edge counterpart of tools/bench_multi_env.py (same timing rules).

Shapes:
  mbm    the MotionBenchMaker fixture (tests/golden/mbm_<robot>.npz): 1,300 scenes x the start -> goal edge per robot,
         as one multi call vs the loop of 1,300 device calls; the numpy API end to end too.  Environment construction +
         finalize and the first use (the robot part of every environment) are timed separately, once.
  large  64 distinct shell64 scenes x 16,384 roadmap-shaped UR5 edges (workloads.prm_shaped_edges, U[0.2, 1.5] rad,
         generated per scene), as one multi call vs 64 per-scene calls, next to one 1,048,576-edge call on scene 0.
  mixed  one scene per variant class and an attachment (cage, shell64, mixed, capt, clouds, heightfield, attach) x 2,048
         roadmap-shaped UR5 edges: one multi call vs 7 per-scene calls.

Every time is HIP-event time around a window that starts on an idle stream and ends in a synchronise (`inner` calls per
window), after warm-up; the variants of a shape are alternated within each repetition.  The outputs of the variants are
compared bit for bit before timing.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run.

    python tools/bench_multi_env_motion.py [--reps 10] [--out DIR] [--shapes mbm,large,mixed]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_multi_env import ROOT, time_alternating  # noqa: E402  (also puts the repository and tests/ on sys.path)

import torch  # noqa: E402

import vamp_mvt_amd as vamp  # noqa: E402
from vamp_mvt_amd import _lib  # noqa: E402
from vamp_mvt_amd._lib import check  # noqa: E402
from vamp_mvt_amd.workloads import environment_from_spec, prm_shaped_edges, shell_spec  # noqa: E402

L = _lib.lib
VP = ctypes.c_void_p


def _bits(n):
    return torch.zeros(max((n + 63) // 64, 1), dtype=torch.int64, device="cuda")


class Multi:
    """one vmv_validate_motion_batch_multi call with its arguments prebuilt"""

    def __init__(self, rid, envs, counts, a, b):
        self.rid, self.a, self.b, self.bits = rid, a, b, _bits(a.shape[0])
        self.handles = (VP * len(envs))(*[e.handle() for e in envs])
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        self.n_envs = len(envs)

    def __call__(self, stream):
        check(L.vmv_validate_motion_batch_multi(self.rid, self.handles, self.offsets.ctypes.data_as(_lib.c_size_p),
                                                self.n_envs, VP(self.a.data_ptr()), VP(self.b.data_ptr()),
                                                VP(self.bits.data_ptr()), stream), "vmv_validate_motion_batch_multi")

    def result(self, n):
        return vamp.unpack_bits(self.bits.cpu().numpy().view(np.uint64), n)


class Loop:
    """one vmv_validate_motion_batch per environment; segment k's words start at its own word (bits padded per segment)"""

    def __init__(self, rid, envs, counts, a, b):
        dim = a.shape[1]
        words = [(c + 63) // 64 for c in counts]
        self.rid, self.a, self.b, self.bits = rid, a, b, _bits(64 * sum(words))
        self.calls, w0, c0 = [], 0, 0
        for e, c, w in zip(envs, counts, words):
            if c:
                self.calls.append((e.handle(), VP(a.data_ptr() + 4 * dim * c0), VP(b.data_ptr() + 4 * dim * c0), c,
                                   VP(self.bits.data_ptr() + 8 * w0)))
            w0, c0 = w0 + w, c0 + c
        self.counts, self.words = counts, words

    def __call__(self, stream):
        for h, ap, bp, c, out in self.calls:
            check(L.vmv_validate_motion_batch(self.rid, h, ap, bp, c, out, stream), "vmv_validate_motion_batch")

    def result(self, n):
        words = self.bits.cpu().numpy().view(np.uint64)
        out, w0 = [], 0
        for c, w in zip(self.counts, self.words):
            out.append(vamp.unpack_bits(words[w0:w0 + w], c))
            w0 += w
        return np.concatenate(out)[:n]


def shape_mbm(robot, reps, stream, log):
    from test_mbm import problem_primitives

    g = np.load(os.path.join(ROOT, "tests", "golden", f"mbm_{robot}.npz"))
    mod = getattr(vamp, robot)
    rid = mod._id
    n = len(g["names"])
    specs = [problem_primitives(vamp, g, i) for i in range(n)]
    t0 = time.perf_counter()
    envs = [environment_from_spec(s) for s in specs]
    for e in envs:
        e.handle()  # build + finalize (upload)
    build_s = time.perf_counter() - t0
    a_host = np.ascontiguousarray(g["start"], np.float32)
    b_host = np.ascontiguousarray(g["goal"], np.float32)
    a, b = torch.from_numpy(a_host).cuda(), torch.from_numpy(b_host).cuda()
    multi, loop = Multi(rid, envs, [1] * n, a, b), Loop(rid, envs, [1] * n, a, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    multi(stream)  # first use of every environment by this robot: its grids and static links are built here
    torch.cuda.synchronize()
    first_use_s = time.perf_counter() - t0
    loop(stream)
    torch.cuda.synchronize()
    got = multi.result(n)
    assert np.array_equal(got, loop.result(n)), f"{robot}: multi != loop"
    for _ in range(3):
        multi(stream), loop(stream)
    t = time_alternating({"multi": multi, "loop": loop}, reps, 3, stream)
    t0 = time.perf_counter()
    py = mod.validate_motion_batch_multi(a_host, b_host, envs, [1] * n)
    py_multi_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for i, e in enumerate(envs):
        mod.validate_motion_batch(a_host[i:i + 1], b_host[i:i + 1], e)
    py_loop_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(py, got)
    rec = {"shape": "mbm", "robot": robot, "scenes": n, "edges": n, "valid_share": float(got.mean()),
           "build_finalize_s": round(build_s, 3), "first_use_s": round(first_use_s, 3), "multi": t["multi"],
           "loop": t["loop"], "speedup_median": t["loop"]["median_ms"] / t["multi"]["median_ms"],
           "python_numpy_multi_ms": round(py_multi_ms, 3), "python_numpy_loop_ms": round(py_loop_ms, 3)}
    log(rec)
    return rec


def _scene_edges(mod, envs, per, seed):
    parts = [prm_shaped_edges(mod, e, per, 0.2, 1.5, seed + k) for k, e in enumerate(envs)]
    return torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous()


def shape_large(reps, stream, log, scenes=64, per=16384):
    mod = vamp.ur5
    rid = mod._id
    envs = [environment_from_spec(shell_spec(s, 32, 32, 0.45, 0.95)) for s in range(scenes)]
    a, b = _scene_edges(mod, envs, per, 21)
    n = scenes * per
    multi, loop = Multi(rid, envs, [per] * scenes, a, b), Loop(rid, envs, [per] * scenes, a, b)
    one = Loop(rid, envs[:1], [n], a, b)  # one vmv_validate_motion_batch over all n edges against scene 0
    for f in (multi, loop, one):
        f(stream)
    torch.cuda.synchronize()
    got = multi.result(n)
    assert np.array_equal(got, loop.result(n)), "large: multi != loop"
    t = time_alternating({"multi": multi, "loop": loop, "single_1M": one}, reps, 3, stream)
    rec = {"shape": "large", "robot": "ur5", "scenes": scenes, "edges": n, "valid_share": float(got.mean()), **t,
           "loop_over_multi": t["loop"]["median_ms"] / t["multi"]["median_ms"],
           "multi_over_single_1M": t["multi"]["median_ms"] / t["single_1M"]["median_ms"],
           "multi_edges_per_s": n / (t["multi"]["median_ms"] * 1e-3)}
    log(rec)
    return rec


def shape_mixed(reps, stream, log, per=2048):
    from envs import spec_for

    kinds = ["cage", "shell64", "mixed", "capt", "clouds", "heightfield", "attach"]
    mod = vamp.ur5
    rid = mod._id
    envs = [environment_from_spec(spec_for(k, "ur5")) for k in kinds]
    a, b = _scene_edges(mod, envs, per, 31)
    n = per * len(kinds)
    multi, loop = Multi(rid, envs, [per] * len(kinds), a, b), Loop(rid, envs, [per] * len(kinds), a, b)
    for f in (multi, loop):
        f(stream)
    torch.cuda.synchronize()
    got = multi.result(n)
    assert np.array_equal(got, loop.result(n)), "mixed: multi != loop"
    t = time_alternating({"multi": multi, "loop": loop}, reps, 5, stream)
    rec = {"shape": "mixed", "robot": "ur5", "kinds": kinds, "edges": n, "valid_share": float(got.mean()), **t,
           "loop_over_multi": t["loop"]["median_ms"] / t["multi"]["median_ms"]}
    log(rec)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="mbm,large,mixed")
    ap.add_argument("--robots", default="panda,ur5,fetch", help="robots of the mbm shape")
    ap.add_argument("--out", default=None, help="directory for multi_env_motion_bench.json")
    args = ap.parse_args()
    vamp.set_device(0)
    torch.cuda.init()
    stream = VP(torch.cuda.current_stream().cuda_stream)
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    shapes = args.shapes.split(",")
    if "mbm" in shapes:
        for robot in args.robots.split(","):
            shape_mbm(robot, args.reps, stream, log)
    if "large" in shapes:
        shape_large(args.reps, stream, log)
    if "mixed" in shapes:
        shape_mixed(args.reps, stream, log)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "multi_env_motion_bench.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
