#!/usr/bin/env python3
"""The float64 study behind vmv_optimize_multi's defaults: tests/optimize_serial.py in float64 on the float64
clearances of tests/optimize_cases.py (tests/geom64.py's distance forms, every primitive kind and a heightfield), the CPU
oracle answering the edge questions.  No device.  Per scene a few straight Panda lines that are valid, each at 17, 33 and
65 waypoints, for several values of `step`; per (scene, waypoints, step) the table gives: lines, lines whose cost fell,
mean smallest env clearance before -> after (mm), mean growth of the path length (%), mean best iteration, lines whose
last iterate is not the best (the iteration is not monotone), and iterations until the step falls below min_change.

    python tools/optimize_defaults_study.py [--lines 3] > profiles/r23_optimize_defaults_study.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import envs  # noqa: E402
from optimize_cases import GRAZE_CENTRE, GRAZE_GOAL, Clearance64, graze_line, graze_radius, straight  # noqa: E402
from optimize_serial import OK, optimize_serial  # noqa: E402
from oracle_lib import CAGE_START, Oracle  # noqa: E402

STEPS = (1.0 / 10.0, 1.0 / 40.0, 1.0 / 160.0)


def length(X):
    X = np.asarray(X, np.float64)
    return float(np.sqrt(((X[1:] - X[:-1]) ** 2).sum(1)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=3)
    args = ap.parse_args()
    o = Oracle()
    rid = o.robot("panda")
    lower, span = o.bounds(rid)
    upper = lower + span
    X33 = graze_line(33, np.float64)
    radius = graze_radius(lambda r: Clearance64("panda", [("sphere", np.array([*GRAZE_CENTRE, r], np.float32))])(X33)[0][:, 0].min())
    scenes = {"graze (1 sphere)": [("sphere", np.array([*GRAZE_CENTRE, radius], np.float32))],
              "mixed (spheres, cuboids, capsules, z-capsules)": envs.spec_for("mixed", "panda"),
              "counted (4 of each of the five kinds)": envs.counted_spec("panda", (4, 4, 4, 4, 4), seed=3),
              "heightfield (+ 6 spheres)": envs.spec_for("heightfield", "panda")}
    print("# scene | waypoints | step | lines | improved | env mm before -> after | length growth % | best iteration | "
          "last is not best | mean iterations run")
    for name, spec in scenes.items():
        oenv = envs.build_oracle_env(o, spec)
        clearance = Clearance64("panda", spec)

        def question(a, b):
            return o.validate_motion(rid, oenv, np.asarray(a, np.float32), np.asarray(b, np.float32))

        if name.startswith("graze"):
            ends = [(np.float64(CAGE_START), np.float64(GRAZE_GOAL))]
        else:
            rng = np.random.default_rng(7)
            q = (lower + span * rng.random((4096, 7), dtype=np.float32)).astype(np.float32)
            q = q[o.validate_batch(rid, oenv, q)]
            ends = []
            for a, b in zip(q[0::2], q[1::2]):
                b = a + (b - a) * np.float32(0.35)
                X = straight(a, b, 65)
                v = clearance(straight(a, b, 17, np.float64))[0]
                # valid lines that have something to gain: a waypoint within the margin of an obstacle
                if all(question(u, w) for u, w in zip(X[:-1], X[1:])) and v[:, 0].min() < 0.03:
                    ends.append((a.astype(np.float64), b.astype(np.float64)))
                if len(ends) == args.lines:
                    break
        for N in (17, 33, 65):
            for step in STEPS:
                rows = []
                for a, b in ends:
                    X = straight(a, b, N, np.float64)
                    r = optimize_serial(X, clearance, question, lower, upper, step=step, dtype=np.float64)
                    last = r.history[-1]
                    rows.append((r.status == OK and r.cost < r.cost_first, r.clearance_first[0], r.clearance[0],
                                 100.0 * (length(r.path) / length(X) - 1.0), r.best_iteration,
                                 r.status == OK and not (last[4] and last[0] == r.cost), r.iterations))
                rows = np.array(rows, np.float64)
                print(f"{name} | {N} | 1/{round(1 / step)} | {len(rows)} | {int(rows[:, 0].sum())} | {1e3 * rows[:, 1].mean():.1f} -> "
                      f"{1e3 * rows[:, 2].mean():.1f} | {rows[:, 3].mean():+.2f} | {rows[:, 4].mean():.1f} | {int(rows[:, 5].sum())} | "
                      f"{rows[:, 6].mean():.1f}", flush=True)


if __name__ == "__main__":
    main()
