#!/usr/bin/env python3
"""Measurement of vmv_clearance_grad_batch against vmv_clearance_batch on the same inputs in the same session, through the
C ABI's device entry points on one torch stream, on prebuilt, warmed environments.

The gradient call is the clearance launch as it is plus one more kernel (one lane per configuration: the tangent tape of
three witness spheres, one record, 2 * dim stores), so the number reported is the RATIO clearance_grad / clearance and,
next to it, the gradient kernel's own time: the gradient call minus the clearance call that writes the same witness.

Shapes: those of tools/bench_clearance.py (profiles/r20_clearance_bench.json) -
  panda_1m, panda_128k   uniform Panda configurations against bench.py's scene (32 spheres + 32 z-aligned cuboids)
  mixed_<robot>          131,072 uniform configurations against the `mixed` scene of tests/envs.py, four robots

Method: bench_clearance.py's - HIP-event time around windows that start on an idle stream and end in a synchronise,
`inner` calls per window sized for about 50 ms, after warm-up, the variants alternated within each repetition.  Before
timing, the values of the gradient call are compared bit for bit with the clearance call's.

    python tools/bench_clearance_grad.py [--reps 10] [--out FILE.json] [--shapes panda_1m,panda_128k,mixed]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import vamp_mvt_amd as vamp  # noqa: E402
from bench_clearance import time_alternating, uniform_configs  # noqa: E402
from vamp_mvt_amd import _lib  # noqa: E402
from vamp_mvt_amd._lib import check  # noqa: E402
from vamp_mvt_amd.workloads import environment_from_spec, shell_spec  # noqa: E402

L = _lib.lib
VP = ctypes.c_void_p


def measure(name, mod, env, n, reps):
    q = uniform_configs(mod, n)
    h = env.handle()
    values = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    values_g = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    grad = torch.empty((n, 2, mod.dimension()), dtype=torch.float32, device="cuda")
    witness = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    rid = mod._id

    def clearance(stream):
        check(L.vmv_clearance_batch(rid, h, VP(q.data_ptr()), n, VP(values.data_ptr()), None, stream), "vmv_clearance_batch")

    def clearance_witness(stream):
        check(L.vmv_clearance_batch(rid, h, VP(q.data_ptr()), n, VP(values.data_ptr()), VP(witness.data_ptr()), stream),
              "vmv_clearance_batch")

    def clearance_grad(stream):
        check(L.vmv_clearance_grad_batch(rid, h, VP(q.data_ptr()), n, VP(values_g.data_ptr()), VP(grad.data_ptr()), None, stream),
              "vmv_clearance_grad_batch")

    variants = {"clearance_batch": clearance, "clearance_batch_witness": clearance_witness, "clearance_grad_batch": clearance_grad}
    stream = VP(torch.cuda.current_stream().cuda_stream)
    for fn in variants.values():  # warm-up: code objects, the robot part of the environment, the LDS attribute, the scratch
        for _ in range(3):
            fn(stream)
    torch.cuda.synchronize()
    same = bool(torch.equal(values.view(torch.int32), values_g.view(torch.int32)))
    g = grad.cpu().numpy()
    probe = time_alternating({"clearance_grad_batch": clearance_grad}, 1, 1, stream)["clearance_grad_batch"]["median_ms"]
    inner = int(max(1, min(200, round(50.0 / max(probe, 1e-3)))))
    times = time_alternating(variants, reps, inner, stream)
    t = {k: v["median_ms"] for k, v in times.items()}
    row = {"shape": name, "robot": mod.__name__.split(".")[-1], "n": n, "inner": inner, "reps": reps,
           "values_bit_identical": same, "gradient_finite": bool(np.isfinite(g).all()),
           "largest_gradient_entry": float(np.abs(g).max()), "gradient_bytes": n * 2 * mod.dimension() * 4,
           "times": times, "ratio_grad_to_clearance": t["clearance_grad_batch"] / t["clearance_batch"],
           "gradient_kernel_ms": t["clearance_grad_batch"] - t["clearance_batch_witness"]}
    print(f"{name}: n = {n}, clearance {t['clearance_batch']:.4f} ms, with witness {t['clearance_batch_witness']:.4f} ms, "
          f"clearance_grad {t['clearance_grad_batch']:.4f} ms (x{row['ratio_grad_to_clearance']:.3f}); gradient kernel "
          f"{row['gradient_kernel_ms']:.4f} ms; values bit-identical: {same}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="panda_1m,panda_128k,mixed")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_clearance_grad.py needs a GPU: there is no CPU path to measure")
    vamp.set_device(0)
    shapes = args.shapes.split(",")
    rows = []
    bench_scene = environment_from_spec(shell_spec(seed=0))
    if "panda_1m" in shapes:
        rows.append(measure("panda_1m", vamp.panda, bench_scene, 1 << 20, args.reps))
    if "panda_128k" in shapes:
        rows.append(measure("panda_128k", vamp.panda, bench_scene, 1 << 17, args.reps))
    if "mixed" in shapes:
        import envs

        for robot in ("panda", "ur5", "fetch", "baxter"):
            env = envs.build_product_env(envs.spec_for("mixed", robot))
            rows.append(measure(f"mixed_{robot}", getattr(vamp, robot), env, 1 << 17, args.reps))
    result = {"tool": "tools/bench_clearance_grad.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({r["shape"]: round(r["ratio_grad_to_clearance"], 3) for r in rows}))


if __name__ == "__main__":
    main()
