"""Serial restatement of the lockstep RRT-Connect contract — TEST INFRASTRUCTURE ONLY.

One problem at a time, every quantity an explicit np.float32 operation in the written order (one rounding per
operation), Halton by digit reversal, and `question(a, b) -> bool` a callback: the tests pass the CPU oracle's
validate_motion, never the library.  Nothing here imports the package's planning module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

f32 = np.float32
PRIMES = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59)
SOLVED, MAX_ITERATIONS, MAX_SAMPLES = 0, 1, 2


@dataclass
class SerialResult:
    status: int = SOLVED
    path: list = field(default_factory=list)
    iterations: int = 0
    size: list = field(default_factory=list)
    questions: int = 0

    @property
    def solved(self):
        return self.status == SOLVED


def halton(index: int, lower: np.ndarray, span: np.ndarray) -> np.ndarray:
    """sample number `index` (1-based) of the sequence with bases 3, 5, 7, ...: float(n) / float(d), n the
    digit-reversed index and d = b^digits, then u * span + lower (two roundings)"""
    out = np.zeros(len(lower), f32)
    for j in range(len(lower)):
        b, k, n, d = PRIMES[j], int(index), 0, 1
        while k > 0:
            n, d, k = n * b + k % b, d * b, k // b
        u = f32(n) / f32(d)
        out[j] = f32(u * f32(span[j])) + f32(lower[j])
    return out


def _nearest(pts: np.ndarray, count: int, t: np.ndarray):
    """(first index with the least distance, that distance); the per-joint sum is sequential in fp32"""
    diff = pts[:count] - t[None, :]            # fp32 - fp32: one rounding
    sq = diff * diff                           # one rounding
    acc = np.zeros(count, f32)
    for j in range(pts.shape[1]):
        acc = acc + sq[:, j]                   # joints in order, one rounding each
    d = np.sqrt(acc)                           # fp32 sqrt, correctly rounded
    i = int(np.argmin(d))                      # numpy: the first of the least
    return i, f32(d[i])


class _Tree:
    def __init__(self, root, capacity):
        self.pts = np.zeros((capacity, len(root)), f32)
        self.parent = np.zeros(capacity, np.int64)
        self.n = 0
        self.add(root, 0)

    def add(self, q, parent):
        self.pts[self.n] = q
        self.parent[self.n] = parent
        self.n += 1
        return self.n - 1

    def trace(self, i):
        out = []
        while True:
            out.append(self.pts[i].copy())
            if self.parent[i] == i:
                return out
            i = int(self.parent[i])


def rrtc_serial(start, goal, lower, span, question, range_=1.0, balance=True, tree_ratio=1.0, max_iterations=100000,
                max_samples=8192, skip=0) -> SerialResult:
    start, goal = np.array(start, f32), np.array(goal, f32)
    lower, span = np.asarray(lower, f32), np.asarray(span, f32)
    R, ratio = f32(range_), f32(tree_ratio)
    res = SerialResult()

    def ask(a, b):
        res.questions += 1
        return bool(question(a, b))

    if ask(start, goal):
        res.path, res.size = [start, goal], [1, 1]
        return res
    A, B = _Tree(start, max_samples), _Tree(goal, max_samples)
    a_is_start = True
    draws = 0
    while res.iterations < max_iterations and A.n + B.n < max_samples:
        res.iterations += 1
        if (not balance) or f32(np.abs(f32(A.n) - f32(B.n))) / f32(A.n) < ratio:
            A, B = B, A
            a_is_start = not a_is_start
        draws += 1
        t = halton(skip + draws, lower, span)
        ni, d = _nearest(A.pts, A.n, t)
        if not (d > 0):
            continue
        s = f32(min(d, R)) / d
        near = A.pts[ni]
        new = (near + (t - near) * s).astype(f32)  # (t - near): one rounding; * s: one; near + ...: one
        if not ask(near, new):
            continue
        A.add(new, ni)
        new_i = A.n - 1
        bi, bd = _nearest(B.pts, B.n, new)
        origin = B.pts[bi].copy()
        n_steps = max(int(np.ceil(bd / R)), 1)
        prev, frm, connected = bi, origin, True
        for k in range(n_steps):
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
            pa = A.trace(new_i)[::-1]
            pb = B.trace(prev)
            path = pa + (pb[1:] if pb[0].tobytes() == new.tobytes() else pb)
            res.path = path if a_is_start else path[::-1]
            res.size = [A.n, B.n]
            return res
    res.status = MAX_ITERATIONS if res.iterations >= max_iterations else MAX_SAMPLES
    res.size = [A.n, B.n]
    return res
