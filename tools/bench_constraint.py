#!/usr/bin/env python3
"""Measurement of vmv_constraint_project_batch, vmv_constraint_check_batch and vmv_constraint_check_motion_batch through the
C ABI's device entry points on one torch stream.

Inputs per robot: Halton configurations 20,001 .. 52,768 (32,768 lanes) under EEConstraint.upright(z, 0.2), the default
settings; the edges join consecutive PROJECTED configurations cut to a length of 0.5 (10 band samples each), 4,096 of them.
Recorded per robot: each call's time by HIP events, the evaluations the projection made and the time per evaluation, the
share of lanes converged, the share of edges in band, and eefk_batch's time on the same configurations for scale.  There is
no parent to compare against and no target: the figures are reported as they are.

Method: tools/bench_clearance.py's - HIP-event time around windows that start on an idle stream and end in a
synchronise, `inner` calls per window sized for about 50 ms, after warm-up, the variants alternated per repetition.

    python tools/bench_constraint.py [--reps 10] [--out FILE.json] [--robots panda,ur5,fetch,baxter]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import vamp_mvt_amd as vamp  # noqa: E402
from bench_clearance import time_alternating  # noqa: E402
from vamp_mvt_amd import _lib  # noqa: E402
from vamp_mvt_amd._lib import check  # noqa: E402

L = _lib.lib
VP = ctypes.c_void_p
N, N_EDGES, SKIP, EDGE_LENGTH = 32768, 4096, 20000, 0.5


def measure(robot, reps):
    mod = getattr(vamp, robot)
    dim, rid = mod.dimension(), mod._id
    s = vamp.ConstraintSettings()
    cs = s.struct()
    constraint = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    recs = (_lib.EeConstraint * 1)(constraint.struct())
    q = mod.halton_device(N, SKIP)
    out = torch.empty((N, dim), dtype=torch.float32, device="cuda")
    res = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    bits = torch.zeros((N + 63) // 64, dtype=torch.int64, device="cuda")
    frames = torch.empty((N, 16), dtype=torch.float32, device="cuda")
    ok = torch.zeros(N_EDGES, dtype=torch.uint8, device="cuda")
    stream = VP(torch.cuda.current_stream().cuda_stream)

    def project(stream):
        check(L.vmv_constraint_project_batch(rid, VP(q.data_ptr()), N, recs, 1, ctypes.byref(cs), VP(out.data_ptr()), VP(res.data_ptr()),
                                             VP(status.data_ptr()), stream), "vmv_constraint_project_batch")

    project(stream)
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint32)
    conv, evals = (st >> 31).astype(bool), (st & 0x3fffffff).astype(np.int64)
    rows = out[torch.from_numpy(conv).cuda()][:N_EDGES + 1]
    a = rows[:-1].contiguous()
    step = rows[1:] - a
    b = (a + step * (EDGE_LENGTH / step.norm(dim=1, keepdim=True).clamp_min(1e-6)).clamp_max(1.0)).contiguous()
    n_edges = int(a.shape[0])

    def check_configs(stream):
        check(L.vmv_constraint_check_batch(rid, VP(out.data_ptr()), N, recs, 1, ctypes.byref(cs), VP(bits.data_ptr()), VP(res.data_ptr()),
                                           stream), "vmv_constraint_check_batch")

    def check_edges(stream):
        check(L.vmv_constraint_check_motion_batch(rid, VP(a.data_ptr()), VP(b.data_ptr()), n_edges, recs, 1, ctypes.byref(cs),
                                                  VP(ok.data_ptr()), stream), "vmv_constraint_check_motion_batch")

    def eefk(stream):
        check(L.vmv_eefk_batch(rid, VP(q.data_ptr()), N, VP(frames.data_ptr()), stream), "vmv_eefk_batch")

    variants = {"project_batch": project, "check_batch": check_configs, "check_motion_batch": check_edges, "eefk_batch": eefk}
    for fn in variants.values():
        for _ in range(3):
            fn(stream)
    torch.cuda.synchronize()
    in_band = float(ok[:n_edges].float().mean())
    times = {}
    for name, fn in variants.items():  # each variant's windows sized for itself: their times differ by orders of magnitude
        probe = time_alternating({name: fn}, 1, 1, stream)[name]["median_ms"]
        inner = int(max(1, min(200, round(50.0 / max(probe, 1e-3)))))
        times[name] = dict(time_alternating({name: fn}, reps, inner, stream)[name], inner=inner)
    evaluations = int(evals.sum()) + N  # the inputs' included
    t = times["project_batch"]["median_ms"]
    row = {"robot": robot, "dimension": dim, "lanes": N, "edges": n_edges, "edge_length": EDGE_LENGTH, "settings": vars(s),
           "constraint": "upright(z, 0.2)", "project_batch_ms": t, "evaluations": evaluations,
           "mean_evaluations_per_lane": evaluations / N, "ns_per_evaluation": t * 1e6 / evaluations,
           "lanes_converged": float(conv.mean()), "check_batch_ms": times["check_batch"]["median_ms"],
           "check_motion_batch_ms": times["check_motion_batch"]["median_ms"], "edges_in_band": in_band,
           "eefk_batch_ms": times["eefk_batch"]["median_ms"], "times": times}
    print(f"{robot}: project_batch {t:.3f} ms for {N} lanes, {row['mean_evaluations_per_lane']:.1f} evaluations per lane, "
          f"{row['ns_per_evaluation']:.3f} ns per evaluation, converged {row['lanes_converged']:.3f}; check_batch "
          f"{row['check_batch_ms']:.4f} ms (eefk_batch {row['eefk_batch_ms']:.4f} ms); check_motion_batch "
          f"{row['check_motion_batch_ms']:.4f} ms for {n_edges} edges of {EDGE_LENGTH} rad, {in_band:.3f} in band", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--robots", default="panda,ur5,fetch,baxter")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_constraint.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    rows = [measure(r, args.reps) for r in args.robots.split(",")]
    result = {"tool": "tools/bench_constraint.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({r["robot"]: round(r["project_batch_ms"], 3) for r in rows}))


if __name__ == "__main__":
    main()
