#!/usr/bin/env python3
"""cartesian_multi against what a user writes without it: per robot 1,024 straight lines of 10 - 20 cm with up to 0.3 rad of
rotation from Halton starts, in the empty environment.

  A  one planning.cartesian_multi call (one tracking launch, two validation calls);
  B  the host loop: per waypoint ONE warm-started ik_batch call (n_seeds = 1, seeds = the previous waypoints) over the lines
     still alive, the convergence and joint-step tests in numpy on whole arrays (the waypoints live in one preallocated
     block; nothing is done line by line), and at the end ONE validate_motion_batch_multi call over all tracked edges.
     The poses of B are computed before its clock starts (cartesian_serial's float64 line, cast to fp32), so B is not
     charged for them.

Both are synchronous host-buffer calls; each window is timed with device events on the default stream around `reps` calls, and
windows of A and B alternate in one process.  Writes one JSON document: per robot the window times, the share of lines
completed and the share of every status.  No ratio is asserted anywhere: this tool records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_lines(robot, n, rng):
    import cartesian_serial as C
    import ik_serial as K

    starts = K.halton32(robot, n, 1000)
    F = K.frames44(robot, starts)
    targets = F.copy()
    for p in range(n):
        d, a = rng.normal(size=3), rng.normal(size=3)
        targets[p, :3, 3] += rng.uniform(0.10, 0.20) * d / np.linalg.norm(d)
        targets[p, :3, :3] = F[p, :3, :3] @ C.rot(a / np.linalg.norm(a), rng.uniform(0.0, 0.3))
    return starts, targets.astype(np.float32)


def host_loop(vamp, mod, starts, lines, poses, s):
    """B: -> (achieved [n], status names [n]); poses[k - 1]: float32 [n][4][4], pose k of every line (the last one repeated)"""
    n = len(starts)
    iks = vamp.IKSettings(n_seeds=1, max_iterations=s.max_iterations, pos_tol=s.pos_tol, rot_tol=s.rot_tol, rot_weight=s.rot_weight,
                          damping=s.damping, max_step=s.max_step, position_only=s.position_only)
    m = np.array([line.m for line in lines])
    prev, live = starts.copy(), np.ones(n, bool)
    achieved, status = np.zeros(n, np.int64), np.array(["complete"] * n, dtype=object)
    way = np.zeros((n, int(m.max()) + 1, starts.shape[1]), np.float32)  # the waypoints, one preallocated block
    way[:, 0] = starts
    for k in range(1, int(m.max()) + 1):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        q, _, conv, _ = mod.ik_batch(poses[k - 1][idx], seeds=prev[idx][:, None, :], settings=iks)
        q, conv = q[:, 0], conv[:, 0]
        ok = conv & (np.abs(q - prev[idx]).max(axis=1) <= np.float32(s.max_joint_step))
        status[idx[~ok]] = np.where(conv[~ok], "joint_jump", "ik_failed")
        live[idx[~ok]] = False
        good = idx[ok]
        prev[good] = q[ok]
        achieved[good] += 1
        way[good, k] = q[ok]
        live[good] = k < m[good]
    edge = np.arange(way.shape[1] - 1)[None, :] < achieved[:, None]  # [n][longest]: the tracked edges, line by line
    if edge.any():
        valid = np.ones(edge.shape, bool)
        valid[edge] = mod.validate_motion_batch_multi(way[:, :-1][edge], way[:, 1:][edge], [None] * n, achieved)
        first_bad = np.where(valid.all(axis=1), achieved, np.argmin(valid, axis=1))
        status[first_bad < achieved] = "collision"
        achieved = first_bad
    return achieved, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps-a", type=int, default=20)
    ap.add_argument("--reps-b", type=int, default=4)
    ap.add_argument("--robots", default="panda,ur5,fetch,baxter")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_cartesian_bench.json"))
    args = ap.parse_args()

    import torch

    import cartesian_serial as C
    import vamp_mvt_amd as vamp

    P = vamp.planning
    s = P.CartesianSettings()
    report = dict(lines=args.lines, windows=args.windows, reps=dict(A=args.reps_a, B=args.reps_b), settings=vars(s).copy(),
                  device=torch.cuda.get_device_name(0), robots={})

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps  # ms per call

    for robot in args.robots.split(","):
        mod = getattr(vamp, robot)
        starts, targets = make_lines(robot, args.lines, np.random.default_rng(25))
        envs = [None] * args.lines
        frames = mod.eefk_batch(starts)
        lines = [C.line(frames[p], targets[p], C.Settings()) for p in range(args.lines)]
        longest = max(line.m for line in lines)
        poses = [np.stack([line.pose(min(k, line.m)) for line in lines]).astype(np.float32) for k in range(1, longest + 1)]

        def run_a():
            return P.cartesian_multi(mod, starts, targets, envs, s)

        def run_b():
            return host_loop(vamp, mod, starts, lines, poses, s)

        got, (b_achieved, b_status) = run_a(), run_b()  # warm-up of every shape, and the answers
        a_ms, b_ms = [], []
        for _ in range(args.windows):
            a_ms.append(timed(run_a, args.reps_a))
            b_ms.append(timed(run_b, args.reps_b))
        status = [r.status for r in got]
        raw = mod.cartesian_multi_raw(starts, targets, envs, s)
        report["robots"][robot] = dict(
            segments=dict(min=int(min(r.segments for r in got)), max=int(longest), total=int(sum(r.segments for r in got))),
            waypoints_returned=int(sum(r.achieved for r in got)), evaluations=int(sum(r.evaluations for r in got)),
            questions=raw["questions"], validation_calls=raw["validation_calls"],
            share={k: status.count(k) / len(status) for k in P.CARTESIAN_STATUS if status.count(k)},
            host_loop_share={k: float((b_status == k).mean()) for k in P.CARTESIAN_STATUS if (b_status == k).any()},
            # (the host loop asks no start: an invalid start shows there as a collision on the first edge)
            same_status_and_achieved_as_host_loop=float(np.mean([(r.status.replace("invalid_start", "collision"), r.achieved) == (st, int(ac))
                                                                 for r, st, ac in zip(got, b_status, b_achieved)])),
            ik_batch_calls_of_host_loop=int(longest),
            cartesian_multi_ms=dict(windows=[round(v, 4) for v in a_ms], median=round(float(np.median(a_ms)), 4)),
            host_loop_ms=dict(windows=[round(v, 4) for v in b_ms], median=round(float(np.median(b_ms)), 4)),
            host_loop_over_cartesian_multi=round(float(np.median(b_ms) / np.median(a_ms)), 2))
        print(robot, json.dumps(report["robots"][robot]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
