#!/usr/bin/env python3
"""Measurement of vmv_validate_batch_multi (many environments in one call) against one vmv_validate_batch per
environment, on prebuilt, warmed environments, through the C ABI's device entry points on one torch stream.

Shapes:
  mbm    the MotionBenchMaker fixture (tests/golden/mbm_<robot>.npz): 1,300 scenes x (start, goal) per robot, as one
         multi call vs the loop of 1,300 device calls.  Environment construction + finalize and the first use (the
         robot part of every environment: grids, static links) are timed separately, once.
  large  64 distinct shell64 scenes x 16,384 uniform Panda configurations (1,048,576), as one multi call vs 64 per-scene
         calls, next to one 1,048,576-configuration call on a single scene.
  mixed  one scene per variant class and an attachment (cage, shell64, mixed, capt, clouds, heightfield, attach) x 16,384
         Panda configurations: one multi call (one launch per class present) vs 7 per-scene calls.

Every time is HIP-event time around a window that starts on an idle stream and ends in a synchronise (`inner` calls per
window), after warm-up; the variants of a shape are alternated within each repetition (A B, B A, ...).  The outputs of
the variants are compared bit for bit before timing.  Kernel times come from a separate rocprofv3 --kernel-trace --stats
run of this script.

    python tools/bench_multi_env.py [--reps 10] [--out DIR] [--shapes mbm,large,mixed]
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import vamp_mvt_amd as vamp  # noqa: E402
from vamp_mvt_amd import _lib  # noqa: E402
from vamp_mvt_amd._lib import check  # noqa: E402
from vamp_mvt_amd.workloads import environment_from_spec, shell_spec  # noqa: E402

L = _lib.lib
VP = ctypes.c_void_p


class Multi:
    """one vmv_validate_batch_multi call with its arguments prebuilt"""

    def __init__(self, rid, envs, counts, q, bits):
        self.rid, self.q, self.bits = rid, q, bits
        self.handles = (VP * len(envs))(*[e.handle() for e in envs])
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        self.n_envs = len(envs)

    def __call__(self, stream):
        check(L.vmv_validate_batch_multi(self.rid, self.handles, self.offsets.ctypes.data_as(_lib.c_size_p), self.n_envs,
                                         VP(self.q.data_ptr()), VP(self.bits.data_ptr()), stream), "vmv_validate_batch_multi")

    def result(self, n):
        return vamp.unpack_bits(self.bits.cpu().numpy().view(np.uint64), n)


class Loop:
    """one vmv_validate_batch per environment; segment k's words start at its own word (bits is padded per segment)"""

    def __init__(self, rid, envs, counts, q, dim):
        self.rid, self.q = rid, q
        words = [(c + 63) // 64 for c in counts]
        self.bits = torch.zeros(max(sum(words), 1), dtype=torch.int64, device="cuda")
        self.calls, w0, c0 = [], 0, 0
        for e, c, w in zip(envs, counts, words):
            if c:
                self.calls.append((e.handle(), VP(q.data_ptr() + 4 * dim * c0), c, VP(self.bits.data_ptr() + 8 * w0)))
            w0, c0 = w0 + w, c0 + c
        self.counts, self.words = counts, words

    def __call__(self, stream):
        for h, qp, c, bp in self.calls:
            check(L.vmv_validate_batch(self.rid, h, qp, c, bp, stream), "vmv_validate_batch")

    def result(self, n):
        words = self.bits.cpu().numpy().view(np.uint64)
        out, w0 = [], 0
        for c, w in zip(self.counts, self.words):
            out.append(vamp.unpack_bits(words[w0:w0 + w], c))
            w0 += w
        return np.concatenate(out)[:n]


class Single:
    """one vmv_validate_batch over the whole batch against one environment"""

    def __init__(self, rid, env, n, q):
        self.rid, self.h, self.n, self.q = rid, env.handle(), n, q
        self.bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")

    def __call__(self, stream):
        check(L.vmv_validate_batch(self.rid, self.h, VP(self.q.data_ptr()), self.n, VP(self.bits.data_ptr()), stream),
              "vmv_validate_batch")


def time_alternating(variants, reps, inner, stream):
    """{name: fn(stream)} -> {name: per-call ms (median, min, every window)}; windows alternate the order per repetition"""
    raw = {k: [] for k in variants}
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    names = list(variants)
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            start.record()
            for _ in range(inner):
                variants[name](stream)
            end.record()
            end.synchronize()
            raw[name].append(start.elapsed_time(end) / inner)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "windows_ms": [round(x, 5) for x in v]}
            for k, v in raw.items()}


def fill_uniform(rid, n, seed, stream):
    dim = L.vmv_robot_dimension(rid)
    q = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    check(L.vmv_fill_uniform_configs(rid, VP(q.data_ptr()), n, seed, stream), "vmv_fill_uniform_configs")
    return q


def shape_mbm(robot, reps, stream, log):
    from test_mbm import problem_primitives

    g = np.load(os.path.join(ROOT, "tests", "golden", f"mbm_{robot}.npz"))
    mod = getattr(vamp, robot)
    rid, dim = mod._id, mod.dimension()
    n_scenes = len(g["names"])
    specs = [problem_primitives(vamp, g, i) for i in range(n_scenes)]
    t0 = time.perf_counter()
    envs = [environment_from_spec(s) for s in specs]
    for e in envs:
        e.handle()  # build + finalize (upload)
    build_s = time.perf_counter() - t0
    q_host = np.stack([np.stack([g["start"][i], g["goal"][i]]) for i in range(n_scenes)]).reshape(-1, dim).astype(np.float32)
    n = len(q_host)
    q = torch.from_numpy(q_host).cuda()
    multi = Multi(rid, envs, [2] * n_scenes, q, torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"))
    loop = Loop(rid, envs, [2] * n_scenes, q, dim)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    multi(stream)  # first use of every environment by this robot: its grids and static links are built here
    torch.cuda.synchronize()
    first_use_s = time.perf_counter() - t0
    loop(stream)
    torch.cuda.synchronize()
    assert np.array_equal(multi.result(n), loop.result(n)), f"{robot}: multi != loop"
    for _ in range(3):
        multi(stream), loop(stream)
    t = time_alternating({"multi": multi, "loop": loop}, reps, 3, stream)
    # the Python API end to end (numpy in, numpy out: staging copies and a synchronise per call), for scale
    t0 = time.perf_counter()
    mod.validate_batch_multi(q_host, envs, [2] * n_scenes)
    py_multi_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for i, e in enumerate(envs):
        mod.validate_batch(q_host[2 * i:2 * i + 2], e)
    py_loop_ms = (time.perf_counter() - t0) * 1e3
    rec = {"shape": "mbm", "robot": robot, "scenes": n_scenes, "configs": n, "build_finalize_s": round(build_s, 3),
           "first_use_s": round(first_use_s, 3), "multi": t["multi"], "loop": t["loop"],
           "speedup_median": t["loop"]["median_ms"] / t["multi"]["median_ms"],
           "python_numpy_multi_ms": round(py_multi_ms, 3), "python_numpy_loop_ms": round(py_loop_ms, 3)}
    log(rec)
    return rec


def shape_large(reps, stream, log, scenes=64, per=16384):
    rid = vamp.panda._id
    envs = [environment_from_spec(shell_spec(s, 32, 32, 0.45, 0.95)) for s in range(scenes)]
    n = scenes * per
    q = fill_uniform(rid, n, 11, stream)
    multi = Multi(rid, envs, [per] * scenes, q, torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"))
    loop = Loop(rid, envs, [per] * scenes, q, 7)
    single = Single(rid, envs[0], n, q)
    for f in (multi, loop, single):
        f(stream)
    torch.cuda.synchronize()
    got = multi.result(n)
    assert np.array_equal(got, loop.result(n)), "large: multi != loop"
    t = time_alternating({"multi": multi, "loop": loop, "single_1M": single}, reps, 5, stream)
    rec = {"shape": "large", "robot": "panda", "scenes": scenes, "configs": n, "valid_share": float(got.mean()),
           **t, "loop_over_multi": t["loop"]["median_ms"] / t["multi"]["median_ms"],
           "multi_over_single_1M": t["multi"]["median_ms"] / t["single_1M"]["median_ms"],
           "multi_checks_per_s": n / (t["multi"]["median_ms"] * 1e-3)}
    log(rec)
    return rec


def shape_mixed(reps, stream, log, per=16384):
    from envs import spec_for

    kinds = ["cage", "shell64", "mixed", "capt", "clouds", "heightfield", "attach"]
    rid = vamp.panda._id
    envs = [environment_from_spec(spec_for(k, "panda")) for k in kinds]
    n = per * len(kinds)
    q = fill_uniform(rid, n, 12, stream)
    multi = Multi(rid, envs, [per] * len(kinds), q, torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda"))
    loop = Loop(rid, envs, [per] * len(kinds), q, 7)
    for f in (multi, loop):
        f(stream)
    torch.cuda.synchronize()
    assert np.array_equal(multi.result(n), loop.result(n)), "mixed: multi != loop"
    t = time_alternating({"multi": multi, "loop": loop}, reps, 5, stream)
    rec = {"shape": "mixed", "robot": "panda", "kinds": kinds, "configs": n, **t,
           "loop_over_multi": t["loop"]["median_ms"] / t["multi"]["median_ms"]}
    log(rec)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="mbm,large,mixed")
    ap.add_argument("--out", default=None, help="directory for multi_env_bench.json")
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
        for robot in ("panda", "ur5", "fetch"):
            shape_mbm(robot, args.reps, stream, log)
    if "large" in shapes:
        shape_large(args.reps, stream, log)
    if "mixed" in shapes:
        shape_mixed(args.reps, stream, log)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "multi_env_bench.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "records": records}, f, indent=1)


if __name__ == "__main__":
    main()
