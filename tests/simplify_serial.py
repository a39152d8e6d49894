"""Serial restatement of the lockstep simplifier's contract — TEST INFRASTRUCTURE ONLY.

simplify() of planning/simplify.hh with the SHORTCUT and BSPLINE routines, one path at a time and ONE QUESTION AT A TIME
in the reference's literal loop order: no windows, the short-circuit `and` kept.  Every quantity is an explicit
np.float32 operation in the written order (one rounding per operation) and `question(a, b) -> bool` is a callback: the
tests pass the CPU oracle's validate_motion, never the library.  Nothing here imports the package.

Because the questions are asked serially, equality with the device for several questions_per_round also shows that
asking a window of candidates at once does not change the answer.  `trace` records what the windowed question count
needs (windowed_questions below): the device asks whole windows and both motions of a B-spline candidate.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

f32 = np.float32
OK, CAPACITY = 0, 1
SHORTCUT, BSPLINE = "SHORTCUT", "BSPLINE"


@dataclass
class SerialSimplifyResult:
    status: int = OK
    path: list = field(default_factory=list)
    iterations: int = 0
    questions: int = 0   # asked serially
    # ("direct",) | ("shortcut", i, candidates, k) with k the 0-based rank (from the far end) of the first valid
    # candidate or None | ("bspline", step, size, passed) with passed = [(index, first valid, second valid or None)]
    trace: list = field(default_factory=list)

    @property
    def erased(self):
        return any(t[0] == "shortcut" and t[3] is not None for t in self.trace)

    @property
    def replaced(self):
        return any(t[0] == "bspline" and any(a and b for _, a, b in t[3]) for t in self.trace)


class _Capacity(Exception):
    pass


def interpolate(a, b, t):
    """a + (b - a) * t per joint (vector/interface.hh:422-425): three roundings"""
    return (a + (b - a) * f32(t)).astype(f32)


def distance(a, b):
    """sqrtf(sum of squares of (b - a) in joint order)"""
    d = (b - a).astype(f32)
    sq = (d * d).astype(f32)
    acc = f32(0)
    for j in range(len(sq)):
        acc = f32(acc + sq[j])
    return f32(np.sqrt(acc))


def cost(path):
    """Path::cost (plan.hh:13-32)"""
    if len(path) < 2:
        return float("inf")
    acc = f32(0)
    for a, b in zip(path[:-1], path[1:]):
        acc = f32(acc + distance(a, b))
    return float(acc)


def _subdivide(path):
    out = []
    for a, b in zip(path[:-1], path[1:]):
        out += [a, interpolate(a, b, 0.5)]
    out.append(path[-1])
    return out


def simplify_serial(path, question, max_iterations=4, operations=(SHORTCUT, BSPLINE), max_steps=5, min_change=0.05,
                    midpoint_interpolation=0.5, max_waypoints=2048) -> SerialSimplifyResult:
    pts = [np.array(q, f32) for q in path]
    res = SerialSimplifyResult()
    min_change = f32(min_change)
    if len(pts) > max_waypoints:
        raise ValueError("max_waypoints is below the input's length")
    for op in operations:
        if op not in (SHORTCUT, BSPLINE):
            raise ValueError(op)

    def ask(a, b):
        res.questions += 1
        return bool(question(a, b))

    def shortcut():
        if len(pts) < 3:
            return False
        result, i = False, 0
        while i < len(pts) - 2:  # re-evaluated after every erase
            candidates, found = len(pts) - i - 2, None
            for j in range(len(pts) - 1, i + 1, -1):
                if ask(pts[i], pts[j]):
                    found = len(pts) - 1 - j
                    del pts[i + 1:j]
                    result = True
                    break
            res.trace.append(("shortcut", i, candidates, found))
            i += 1
        return result

    def bspline():
        if len(pts) < 3:
            return False
        changed = False
        for step in range(max_steps):
            if 2 * len(pts) - 1 > max_waypoints:
                raise _Capacity()  # the subdivide is not performed; the path stays as it stood
            pts[:] = _subdivide(pts)
            updated, passed = False, []
            for index in range(2, len(pts) - 1, 2):
                t1 = interpolate(pts[index], pts[index - 1], midpoint_interpolation)
                t2 = interpolate(pts[index], pts[index + 1], midpoint_interpolation)
                mid = interpolate(t1, t2, 0.5)
                if distance(pts[index], mid) > min_change:  # false for NaN
                    first = ask(pts[index - 1], mid)
                    second = ask(mid, pts[index + 1]) if first else None
                    passed.append((index, first, second))
                    if first and second:
                        pts[index] = mid
                        changed = updated = True
            res.trace.append(("bspline", step, len(pts), passed))
            if not updated:
                break
        return changed

    if len(pts) < 2:
        res.path = pts
        return res
    if len(pts) == 2:
        res.path = [pts[0], pts[1]]
        return res
    res.trace.append(("direct",))
    if ask(pts[0], pts[-1]):
        res.path = [pts[0], pts[-1]]
        return res
    routines = {SHORTCUT: shortcut, BSPLINE: bspline}
    try:
        for _ in range(max_iterations):
            res.iterations += 1
            any_ = False
            for op in operations:
                any_ |= routines[op]()
            if not any_:
                break
    except _Capacity:
        res.status = CAPACITY
    res.path = pts
    return res


def windowed_questions(trace, w):
    """real (non-null) questions the lockstep form asks for this trace with w questions per round: shortcut asks the
    candidates of waypoint i window by window from the far end until a window holds a valid one; a B-spline step asks
    both motions of every candidate that passed the min_change test"""
    total = 0
    for t in trace:
        if t[0] == "direct":
            total += 1
        elif t[0] == "shortcut":
            _, _, candidates, k = t
            total += candidates if k is None else min(candidates, (k // w + 1) * w)
        else:
            total += 2 * len(t[3])
    return total


def windowed_rounds(trace, w):
    """validation rounds this path needs alone (every window is one round)"""
    rounds = 0
    for t in trace:
        if t[0] == "direct":
            rounds += 1
        elif t[0] == "shortcut":
            _, _, candidates, k = t
            rounds += -(-candidates // w) if k is None else k // w + 1
        else:
            rounds += -(-len(t[3]) // (w // 2))
    return rounds
