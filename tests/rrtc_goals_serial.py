"""Serial restatement of the lockstep RRT-Connect contract with goal sets, dynamic domain and start_tree_first
("Goal sets, dynamic domain, start_tree_first") — TEST INFRASTRUCTURE ONLY.

In the style of rrtc_serial.py: one problem at a time, every quantity an explicit np.float32 operation in the written
order (one rounding per operation), and `question(a, b) -> bool` a callback: the tests pass the CPU oracle's
validate_motion, never the library.  The Halton sequence is rrtc_serial's.  Nothing here imports the package.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED, halton

f32 = np.float32
UNSET = np.finfo(np.float32).max  # a node's radius before its first failed extension (FLT_MAX)


@dataclass
class GoalsResult:
    status: int = SOLVED
    path: list = field(default_factory=list)
    iterations: int = 0
    size: list = field(default_factory=list)
    questions: int = 0
    goal_index: int = -1
    # dynamic-domain events: a sample the domain rejected; a radius set on a node's first failed extension; a set radius
    # shrunk by a failed extension, or clamped where max() chose min_radius instead; a set radius grown by a valid one
    events: dict = field(default_factory=lambda: dict(reject=0, set=0, shrink=0, clamp=0, grow=0))

    @property
    def solved(self):
        return self.status == SOLVED


def _nearest(pts: np.ndarray, count: int, t: np.ndarray):
    """(first index with the least distance, that distance) among the nodes whose distance compares below +inf, or None:
    a non-finite node is never the nearest.  The per-joint sum is sequential in fp32."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = pts[:count] - t[None, :]
        sq = diff * diff
        acc = np.zeros(count, f32)
        for j in range(pts.shape[1]):
            acc = acc + sq[:, j]
        d = np.sqrt(acc)
    key = np.where(d < np.inf, d, f32(np.inf))  # NaN and +inf never compare below the running least
    i = int(np.argmin(key))
    return (i, f32(d[i])) if key[i] < np.inf else None


class _Tree:
    def __init__(self, roots, capacity):
        self.pts = np.zeros((capacity, len(roots[0])), f32)
        self.parent = np.zeros(capacity, np.int64)
        self.radius = np.full(capacity, UNSET, f32)
        self.n = 0
        for q in roots:
            self.add(q, self.n)

    def add(self, q, parent):
        self.pts[self.n] = q
        self.parent[self.n] = parent
        self.radius[self.n] = UNSET
        self.n += 1
        return self.n - 1

    def trace(self, i):
        """waypoints i .. root, and the root's index"""
        out = []
        while True:
            out.append(self.pts[i].copy())
            if self.parent[i] == i:
                return out, i
            i = int(self.parent[i])


def rrtc_goals_serial(start, goals, lower, span, question, range_=1.0, balance=True, tree_ratio=1.0, max_iterations=100000,
                      max_samples=8192, skip=0, dynamic_domain=False, radius=4.0, alpha=0.0001, min_radius=1.0,
                      start_tree_first=False) -> GoalsResult:
    start = np.array(start, f32)
    goals = np.array(goals, f32)
    assert goals.ndim == 2 and len(goals) >= 1 and 1 + len(goals) <= max_samples
    lower, span = np.asarray(lower, f32), np.asarray(span, f32)
    R, ratio = f32(range_), f32(tree_ratio)
    radius, alpha, min_radius = f32(radius), f32(alpha), f32(min_radius)
    up, down = f32(f32(1) + alpha), f32(f32(1) - alpha)  # each rounded once, then the products below
    res = GoalsResult()
    ev = res.events

    def ask(a, b):
        res.questions += 1
        return bool(question(a, b))

    for g in range(len(goals)):  # the direct phase: one question per goal, in order
        if ask(start, goals[g]):
            res.path, res.size, res.goal_index = [start, goals[g].copy()], [1, 1], g
            return res
    S, G = _Tree([start], max_samples), _Tree(list(goals), max_samples)
    A, B = (G, S) if start_tree_first else (S, G)
    draws = 0
    while res.iterations < max_iterations and A.n + B.n < max_samples:
        res.iterations += 1
        if (not balance) or f32(np.abs(f32(A.n) - f32(B.n))) / f32(A.n) < ratio:
            A, B = B, A
        draws += 1
        t = halton(skip + draws, lower, span)
        near_a = _nearest(A.pts, A.n, t)
        if near_a is None or not (near_a[1] > 0):
            continue
        ni, d = near_a
        if dynamic_domain and A.radius[ni] < d:
            ev["reject"] += 1
            continue
        s = f32(min(d, R)) / d
        near = A.pts[ni]
        new = (near + (t - near) * s).astype(f32)
        if not ask(near, new):
            if dynamic_domain:
                if A.radius[ni] == UNSET:
                    A.radius[ni] = radius
                    ev["set"] += 1
                else:
                    x = f32(A.radius[ni] * down)
                    if x >= min_radius:
                        ev["shrink"] += 1
                    else:  # fmaxf(x, min_radius) chose min_radius
                        x = min_radius
                        ev["clamp"] += 1
                    A.radius[ni] = x
            continue
        new_i = A.add(new, ni)
        if dynamic_domain and A.radius[ni] != UNSET:
            A.radius[ni] = f32(A.radius[ni] * up)
            ev["grow"] += 1
        near_b = _nearest(B.pts, B.n, new)
        bi, bd = near_b if near_b is not None else (0, f32(np.nan))  # only non-finite roots: one step that cannot be valid
        origin = B.pts[bi].copy()
        c = np.ceil(bd / R)
        n_steps = int(c) if c >= 1 else 1
        prev, frm, connected = bi, origin, True
        for k in range(n_steps):  # the march reads and writes no radius
            if A.n + B.n >= max_samples:
                connected = False
                break
            if bd > 0:
                w = (origin + (new - origin) * (f32(min(f32(k + 1) * R, bd)) / bd)).astype(f32)
            else:
                w = new.copy()
            if not ask(frm, w):
                connected = False
                break
            prev = B.add(w, prev)
            frm = w
        if connected:
            pa, root_a = A.trace(new_i)
            pb, root_b = B.trace(prev)
            pa = pa[::-1]
            path = pa + (pb[1:] if pb[0].tobytes() == new.tobytes() else pb)
            res.path = path if A is S else path[::-1]
            res.goal_index = root_b if A is S else root_a
            res.size = [A.n, B.n]
            return res
    res.status = MAX_ITERATIONS if res.iterations >= max_iterations else MAX_SAMPLES
    res.size = [A.n, B.n]
    return res
