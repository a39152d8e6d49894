#!/usr/bin/env python3
"""Measurement of vmv_ik_batch and vmv_eefk_jacobian_batch through the C ABI's device entry points on one torch stream.

Inputs per robot: 1,024 reachable targets - the end-effector frames of Halton configurations 1 .. 1,024 - times 32 Halton
seeds (samples 5,001 .. 5,032: clear of the targets' own configurations), the default settings.  Recorded per robot: the
call's time by HIP events, the time per evaluation (the call's time over the evaluations its lanes made, the seeds'
included), the share of lanes converged and the share of targets with at least one solution; beside them the Jacobian
call's time against eefk_batch's on the same 32,768 configurations, and the operation counts of the end-effector tape
(tools/gen_hip.py).  There is no parent to compare against and no target: the figures are reported as they are.

Method: tools/bench_clearance.py's - HIP-event time around windows that start on an idle stream and end in a
synchronise, `inner` calls per window sized for about 50 ms, after warm-up, the variants alternated per repetition.

    python tools/bench_ik.py [--reps 10] [--out FILE.json] [--robots panda,ur5,fetch,baxter]
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

import gen_code  # noqa: E402
import gen_hip  # noqa: E402
import vamp_mvt_amd as vamp  # noqa: E402
from bench_clearance import time_alternating  # noqa: E402
from vamp_mvt_amd import _lib  # noqa: E402
from vamp_mvt_amd._lib import check  # noqa: E402

L = _lib.lib
VP = ctypes.c_void_p
N_TARGETS, SEED_SKIP = 1024, 5000


def measure(robot, reps):
    mod = getattr(vamp, robot)
    dim, rid = mod.dimension(), mod._id
    s = vamp.IKSettings()
    cs = s.struct()
    n = N_TARGETS * s.n_seeds
    cfg = mod.halton_device(N_TARGETS, 0)
    targets = mod.eefk_batch(cfg).contiguous()
    q = torch.empty((N_TARGETS, s.n_seeds, dim), dtype=torch.float32, device="cuda")
    err = torch.empty((N_TARGETS, s.n_seeds, 2), dtype=torch.float32, device="cuda")
    status = torch.zeros((N_TARGETS, s.n_seeds), dtype=torch.int32, device="cuda")
    many = mod.halton_device(n, 0)  # the Jacobian call and eefk_batch on as many configurations as the IK call has lanes
    frames = torch.empty((n, 16), dtype=torch.float32, device="cuda")
    jac = torch.empty((n, 6, dim), dtype=torch.float32, device="cuda")

    def ik(stream):
        check(L.vmv_ik_batch(rid, VP(targets.data_ptr()), N_TARGETS, None, SEED_SKIP, ctypes.byref(cs), VP(q.data_ptr()),
                             VP(err.data_ptr()), VP(status.data_ptr()), stream), "vmv_ik_batch")

    def jacobian(stream):
        check(L.vmv_eefk_jacobian_batch(rid, VP(many.data_ptr()), n, VP(frames.data_ptr()), VP(jac.data_ptr()), stream),
              "vmv_eefk_jacobian_batch")

    def eefk(stream):
        check(L.vmv_eefk_batch(rid, VP(many.data_ptr()), n, VP(frames.data_ptr()), stream), "vmv_eefk_batch")

    variants = {"ik_batch": ik, "eefk_jacobian_batch": jacobian, "eefk_batch": eefk}
    stream = VP(torch.cuda.current_stream().cuda_stream)
    for fn in variants.values():
        for _ in range(3):
            fn(stream)
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint32)
    conv, evals = (st >> 31).astype(bool), (st & 0x3fffffff).astype(np.int64)
    evaluations = int(evals.sum()) + n  # the seeds' included
    times = {}
    for name, fn in variants.items():  # each variant's windows sized for itself: their times differ by orders of magnitude
        probe = time_alternating({name: fn}, 1, 1, stream)[name]["median_ms"]
        inner = int(max(1, min(200, round(50.0 / max(probe, 1e-3)))))
        times[name] = dict(time_alternating({name: fn}, reps, inner, stream)[name], inner=inner)
    # the two frame calls once more, alternated with each other in windows of one size
    pair = {k: variants[k] for k in ("eefk_jacobian_batch", "eefk_batch")}
    times["alternated"] = time_alternating(pair, reps, times["eefk_jacobian_batch"]["inner"], stream)
    m = gen_code.load(robot)
    em = gen_hip.ee_model(m)
    tt = gen_hip.tangent_tape(em)
    t_ik = times["ik_batch"]["median_ms"]
    row = {"robot": robot, "dimension": dim, "n_targets": N_TARGETS, "n_seeds": s.n_seeds, "lanes": n, "settings": vars(s),
           "ik_batch_ms": t_ik, "evaluations": evaluations, "mean_evaluations_per_lane": evaluations / n,
           "ns_per_evaluation": t_ik * 1e6 / evaluations, "lanes_converged": float(conv.mean()),
           "targets_with_a_solution": float(conv.any(axis=1).mean()),
           "eefk_jacobian_batch_ms": times["alternated"]["eefk_jacobian_batch"]["median_ms"],
           "eefk_batch_ms": times["alternated"]["eefk_batch"]["median_ms"],
           "ee_tape_primal_operations": len(tt["ops"]), "ee_tape_tangent_operations": gen_hip.tangent_op_count(em, tt),
           "ee_joints": bin(gen_hip.ee_joint_mask(m, tt)).count("1"), "times": times}
    print(f"{robot}: ik_batch {t_ik:.3f} ms for {n} lanes, {row['mean_evaluations_per_lane']:.1f} evaluations per lane, "
          f"{row['ns_per_evaluation']:.3f} ns per evaluation; lanes converged {row['lanes_converged']:.3f}, targets with a solution "
          f"{row['targets_with_a_solution']:.3f}; jacobian {row['eefk_jacobian_batch_ms']:.4f} ms against eefk "
          f"{row['eefk_batch_ms']:.4f} ms on {n} configurations; tape {row['ee_tape_primal_operations']} + "
          f"{row['ee_tape_tangent_operations']} operations", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--robots", default="panda,ur5,fetch,baxter")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_ik.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    rows = [measure(r, args.reps) for r in args.robots.split(",")]
    result = {"tool": "tools/bench_ik.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({r["robot"]: round(r["ik_batch_ms"], 3) for r in rows}))


if __name__ == "__main__":
    main()
