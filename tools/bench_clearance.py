#!/usr/bin/env python3
"""Measurement of vmv_clearance_batch against vmv_validate_batch on the same inputs in the same session, through the C
ABI's device entry points on one torch stream, on prebuilt, warmed environments.

Clearance does strictly more arithmetic than validation - every (fine sphere, contact) and every fine self pair, no gate
and no early out - so the number reported is the RATIO clearance / validate, not a speed-up.  Next to it: the bytes
vmv_fk_batch would write for the same batch (n x n_spheres x 16 B, the fine spheres that the clearance kernel keeps in
LDS) and the bytes the clearance call writes (n x 8 B, n x 24 B with the witness).

Shapes:
  panda_1m     1,048,576 uniform Panda configurations (bench.py's generator and seed) against bench.py's scene:
               shell_spec(seed=0), 32 spheres + 32 z-aligned cuboids
  panda_128k   131,072 of the same
  mixed_<robot>  131,072 uniform configurations against the `mixed` scene of tests/envs.py (6 spheres, 6 z-cuboids, 6
               cuboids, 6 capsules, 6 z-capsules), for each of the four robots

Every time is HIP-event time around a window that starts on an idle stream and ends in a synchronise (`inner` calls per
window, sized so that a window lasts tens of milliseconds at least), after warm-up; clearance (with and without the
witness) and validation are alternated within each repetition (A B C, C B A, ...).  Before timing, the sign of the
clearance is compared with the validity bits outside a 1e-4 m band (a sanity check of the inputs, not the test).

    python tools/bench_clearance.py [--reps 10] [--out FILE.json] [--shapes panda_1m,panda_128k,mixed]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

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


def uniform_configs(mod, n, seed=1234):
    q = torch.empty((n, mod.dimension()), dtype=torch.float32, device="cuda")
    stream = VP(torch.cuda.current_stream().cuda_stream)
    check(L.vmv_fill_uniform_configs(mod._id, VP(q.data_ptr()), n, seed, stream), "vmv_fill_uniform_configs")
    torch.cuda.synchronize()
    return q


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


def measure(name, mod, env, n, reps):
    q = uniform_configs(mod, n)
    h = env.handle()
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    values = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    witness = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    rid = mod._id

    def validate(stream):
        check(L.vmv_validate_batch(rid, h, VP(q.data_ptr()), n, VP(bits.data_ptr()), stream), "vmv_validate_batch")

    def clearance(stream):
        check(L.vmv_clearance_batch(rid, h, VP(q.data_ptr()), n, VP(values.data_ptr()), None, stream), "vmv_clearance_batch")

    def clearance_witness(stream):
        check(L.vmv_clearance_batch(rid, h, VP(q.data_ptr()), n, VP(values.data_ptr()), VP(witness.data_ptr()), stream),
              "vmv_clearance_batch")

    variants = {"validate_batch": validate, "clearance_batch": clearance, "clearance_batch_witness": clearance_witness}
    stream = VP(torch.cuda.current_stream().cuda_stream)
    for fn in variants.values():  # warm-up: code objects, the robot part of the environment, the LDS attribute
        for _ in range(3):
            fn(stream)
    torch.cuda.synchronize()
    valid = vamp.unpack_bits(bits.cpu().numpy().view(np.uint64), n)
    least = values.min(dim=1).values.cpu().numpy()
    judged = np.abs(least) >= 1e-4
    agree = bool(np.array_equal(valid[judged], least[judged] > 0))
    # windows of about 50 ms: one probe call sizes `inner`
    probe = time_alternating({"clearance_batch": clearance}, 1, 1, stream)["clearance_batch"]["median_ms"]
    inner = int(max(1, min(200, round(50.0 / max(probe, 1e-3)))))
    times = time_alternating(variants, reps, inner, stream)
    row = {"shape": name, "robot": mod.__name__.split(".")[-1], "n": n, "inner": inner, "reps": reps,
           "valid_fraction": float(valid.mean()), "sign_agrees_outside_band": agree,
           "in_band": int((~judged).sum()),
           "fk_batch_bytes": n * mod.n_spheres() * 16, "clearance_bytes": n * 8, "clearance_witness_bytes": n * 24,
           "times": times,
           "ratio_clearance_to_validate": times["clearance_batch"]["median_ms"] / times["validate_batch"]["median_ms"],
           "ratio_clearance_witness_to_validate":
               times["clearance_batch_witness"]["median_ms"] / times["validate_batch"]["median_ms"]}
    print(f"{name}: n = {n}, validate {times['validate_batch']['median_ms']:.4f} ms, clearance "
          f"{times['clearance_batch']['median_ms']:.4f} ms (x{row['ratio_clearance_to_validate']:.2f}), with witness "
          f"{times['clearance_batch_witness']['median_ms']:.4f} ms (x{row['ratio_clearance_witness_to_validate']:.2f}); "
          f"fk_batch would write {row['fk_batch_bytes'] / 2 ** 20:.0f} MiB, clearance writes {row['clearance_bytes'] / 2 ** 20:.0f} MiB; "
          f"sign agrees: {agree}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="panda_1m,panda_128k,mixed")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("bench_clearance.py needs a GPU: there is no CPU path to measure")
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
    result = {"tool": "tools/bench_clearance.py", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({r["shape"]: round(r["ratio_clearance_to_validate"], 3) for r in rows}))


if __name__ == "__main__":
    main()
