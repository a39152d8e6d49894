#!/usr/bin/env python3
"""Offline study (oracle = test infrastructure): fine-phase calls and rounds of the environment kernel per wave of 64
configurations — one env_fine call per slab chunk (the form the packed phase replaced) vs each link's items packed into
the slab and run in full rounds (vmv::env_fine_flush / env_fine_packed), vs one queue across links (built once and
removed).
Merged gates of gen_hip.merged_groups (what the primitive-only kernels walk), uniform configurations, shell_spec(0).
    python tools/experiments/packed_fine_study.py [waves]"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_hip  # noqa: E402
from envs import build_oracle_env  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from vamp_mvt_amd.workloads import shell_spec  # noqa: E402

waves = int(sys.argv[1]) if len(sys.argv) > 1 else 20
CHUNK = dict(gen_hip.ENV_CHUNK, fetch=gen_hip.DEFAULT_CHUNK)  # fine spheres per slab chunk (kSlabSpheres)
o = Oracle()
env = build_oracle_env(o, shell_spec(0))
f = ctypes.POINTER(ctypes.c_float)


def hit(c, r):
    c = np.ascontiguousarray(c[:3], np.float32)
    return bool(o.L.vo_sphere_environment_in_collision(env.h, c.ctypes.data_as(f), ctypes.c_float(float(r))))


def packed(k, sizes, cap):
    """(calls, rounds) of one link under the generated flush rule: before a chunk of n spheres, if fill + k n > cap, run
    the full rounds staged, or everything if the carried remainder still would not fit; at the end, everything"""
    fill = calls = rounds = 0
    for ci, n in enumerate(sizes):
        if ci > 0 and fill + k * n > cap:
            run = fill // 64 * 64
            if fill - run + k * n > cap:
                run = fill
            calls += 1
            rounds += -(-run // 64)
            fill -= run
        fill += k * n
    return calls + 1, rounds + -(-fill // 64)


for robot in ["panda", "ur5", "fetch", "baxter"]:
    m = json.load(open(os.path.join(ROOT, "vamp_mvt_amd", "robots", f"{robot}.json")))
    groups = gen_hip.merged_groups(m)
    static = set(gen_hip.static_links(m))
    rid = o.robot(robot)
    lob, span = o.bounds(rid)
    rng = np.random.default_rng(0)
    C = min(CHUNK[robot], max(len(g["fine"]) for g in groups))
    cap = C * 64  # kPackSlots
    tot = dict(calls_now=0, calls_packed=0, rounds_now=0, rounds_packed=0, items=0, rounds_queue=0)
    for w in range(waves):
        q = (lob + span * rng.random((64, len(lob)), dtype=np.float32)).astype(np.float32)
        S = np.stack([o.fk_all(rid, c) for c in q])
        bad = np.zeros(64, bool)
        items_wave = 0
        for g in groups:
            if g["link"] in static:
                continue
            gate = np.array([(not bad[i]) and hit(S[i, g["bound"]], g["radius"]) for i in range(64)])
            k = int(gate.sum())
            if k == 0:
                continue
            fine = g["fine"]
            sizes = [len(fine[c0:c0 + C]) for c0 in range(0, len(fine), C)]
            tot["calls_now"] += len(sizes)
            tot["rounds_now"] += sum(-(-k * n // 64) for n in sizes)
            calls, rounds = packed(k, sizes, cap)
            tot["calls_packed"] += calls
            tot["rounds_packed"] += rounds
            items_wave += k * len(fine)
            for i in np.nonzero(gate)[0]:
                if any(hit(S[i, s], S[i, s][3]) for s in fine):
                    bad[i] = True
        tot["items"] += items_wave
        tot["rounds_queue"] += -(-items_wave // 64)
    per = {k: round(v / waves, 2) for k, v in tot.items()}
    print(f"{robot:7s} chunk {C} slots {cap}: env_fine calls {per['calls_now']} -> {per['calls_packed']}, rounds "
          f"{per['rounds_now']} -> {per['rounds_packed']} ({100 * (per['rounds_packed'] / per['rounds_now'] - 1):+.0f} %), "
          f"items {per['items']}, rounds if queued across links {per['rounds_queue']}  (per wave of 64, {waves} waves)",
          flush=True)
