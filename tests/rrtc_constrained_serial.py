"""Serial restatement of vmv_rrtc_multi_constrained (include/vamp_mvt_amd.h) — TEST INFRASTRUCTURE ONLY.

The loop is tests/rrtc_goals_serial.py's, imported as it is.  Its one callback `question(a, b)` carries the two hooks of the
constrained planner: where b is a NEW node (every question after the G direct ones: the extension's `new`, a march step's
point) it is first projected and replaced IN PLACE - the loop goes on with the array it handed over, exactly as the device
goes on with the pool element the round kernel rewrote - and then the edge's band test is ANDed into the answer.  Both hooks
are answered through the product's batch calls, one question at a time; that is legitimate because each lane's answer is
its own, bit for bit (tests/test_constraint_gpu.py).  Validity is the caller's `valid(a, b)` (the CPU oracle)."""
from __future__ import annotations

import numpy as np

from rrtc_goals_serial import GoalsResult, rrtc_goals_serial

f32 = np.float32
INVALID_ENDPOINT = 4  # VMV_PLAN_INVALID_ENDPOINT


def _dist(a, b):
    """sqrt of the squares summed in joint order, fp32 (the round kernel's stretch test)"""
    sq = f32(0)
    for j in range(len(a)):
        d = f32(a[j] - b[j])
        sq = f32(d * d) if j == 0 else f32(sq + f32(d * d))
    return f32(np.sqrt(sq))


def rrtc_constrained_serial(mod, start, goals, lower, span, valid, constraint, constraint_settings=None, max_stretch=2.0, range_=1.0,
                            **kw) -> GoalsResult:
    """mod: the product's robot (project_batch, constraint_check_batch, constraint_check_motion_batch); constraint: the
    problem's EEConstraint; kw: rrtc_goals_serial's settings"""
    start, goals = np.array(start, f32), np.array(goals, f32)
    ok = mod.constraint_check_batch(np.concatenate([start[None], goals]), constraint, constraint_settings)
    keep = np.flatnonzero(ok[1:])
    if not ok[0] or len(keep) == 0:  # no path, no question
        res = GoalsResult(status=INVALID_ENDPOINT, size=[0, 0])
        res.band_refused = 0
        return res
    stretch = f32(f32(max_stretch) * f32(range_))
    asked, refused = [0], [0]

    def question(a, b):
        new_node = asked[0] >= len(keep)  # the direct questions come first, one per in-band goal
        asked[0] += 1
        if new_node:
            q, _, converged, _ = mod.project_batch(b[None], constraint, constraint_settings)
            if not converged[0] or not _dist(q[0], a) <= stretch:
                refused[0] += 1
                return False  # the node stays as it was; the answer is 0
            b[:] = q[0]
        in_band = bool(mod.constraint_check_motion_batch(a[None], b[None], constraint, constraint_settings)[0])
        refused[0] += not in_band
        return bool(valid(a, b)) and in_band

    res = rrtc_goals_serial(start, goals[keep], lower, span, question, range_=range_, **kw)
    res.band_refused = refused[0]  # the questions the constraint answered 0, whatever validity said
    if res.goal_index >= 0:
        res.goal_index = int(keep[res.goal_index])  # within the caller's set
    return res
