"""Serial restatement of the lazy complete-graph search's contract — TEST INFRASTRUCTURE ONLY.

One problem at a time, every quantity an explicit np.float32 operation in the written order (one rounding per
operation), and `valid(q) -> bool` / `question(a, b) -> bool` callbacks, asked one at a time: the tests pass the CPU
oracle's validate and validate_motion, never the library.  Nothing here imports the package's planning module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from prm_serial import dist2, halton_samples  # noqa: F401  (halton_samples: for the callers)

f32 = np.float32
INF = f32(np.inf)
SOLVED, MAX_ITERATIONS, NO_PATH, INVALID_ENDPOINT = 0, 1, 3, 4


@dataclass
class SerialResult:
    status: int = NO_PATH
    path: list = field(default_factory=list)
    cost: np.float32 = INF
    iterations: int = 0                                  # searches run
    size: list = field(default_factory=lambda: [0, 0])  # valid vertices, blocked edges
    questions: int = 0                                   # edge questions asked
    known_valid: int = 0                                 # edges answered valid
    ids: list = field(default_factory=list)              # the path's vertex ids
    vertex_valid: np.ndarray = None                      # bool[V]

    @property
    def solved(self):
        return self.status == SOLVED


def weights(verts: np.ndarray, u: int) -> np.ndarray:
    """w(u, v) for every v: sqrtf(d2(u, v)), correctly rounded"""
    with np.errstate(all="ignore"):
        return np.sqrt(dist2(verts, u))


def search(verts: np.ndarray, valid: np.ndarray, blocked: np.ndarray, h: np.ndarray, w_row):
    """One A* search over the complete graph of the valid vertices without the blocked pairs, bounded by V pops: pops
    the open, not-closed vertex least by (fl(g + h), id); a closed vertex is never reopened.
    -> (vertex ids from 0 to 1, g[1]) or (None, inf)"""
    n = len(verts)
    g = np.full(n, INF, f32)
    g[0] = f32(0)
    parent = np.full(n, -1, np.int64)
    is_open, closed = np.zeros(n, bool), np.zeros(n, bool)
    is_open[0] = True
    for _ in range(n):
        cand = np.flatnonzero(is_open & ~closed)
        if len(cand) == 0:
            return None, INF
        with np.errstate(all="ignore"):
            f = g[cand] + h[cand]                        # one rounding
        u = int(cand[np.argmin(f)])                      # the first of the least f: ids ascend in cand
        if u == 1:
            ids = [1]
            while ids[-1] != 0:
                ids.append(int(parent[ids[-1]]))
            return ids[::-1], g[1]
        closed[u] = True
        with np.errstate(all="ignore"):
            c = g[u] + w_row(u)                          # one rounding
        better = valid & ~closed & ~blocked[u] & (c < g)
        g[better], parent[better], is_open[better] = c[better], u, True
    return None, INF


def fcit_serial(start, goal, samples, valid, question, max_iterations=100000) -> SerialResult:
    """samples: [n_samples][dim] (halton_samples(skip, n, lower, span), or the caller's)"""
    verts = np.vstack([np.array(start, f32)[None], np.array(goal, f32)[None], np.asarray(samples, f32)])
    n = len(verts)
    res = SerialResult()
    res.vertex_valid = np.array([bool(np.isfinite(q).all()) and bool(valid(q)) for q in verts])
    res.size = [int(res.vertex_valid.sum()), 0]
    if not (res.vertex_valid[0] and res.vertex_valid[1]):
        res.status = INVALID_ENDPOINT
        return res
    rows = {}

    def w_row(u):
        if u not in rows:
            rows[u] = weights(verts, u)
        return rows[u]

    h = w_row(1)
    blocked = np.zeros((n, n), bool)
    known = set()  # pairs answered valid
    while True:
        if res.iterations == max_iterations:
            res.status = MAX_ITERATIONS
            return res
        res.iterations += 1
        ids, cost = search(verts, res.vertex_valid, blocked, h, w_row)
        if ids is None:
            res.status = NO_PATH
            return res
        for a, b in zip(ids[:-1], ids[1:]):
            a, b = min(a, b), max(a, b)
            if (a, b) in known:
                continue
            res.questions += 1
            if question(verts[a], verts[b]):             # always lower id -> higher id
                known.add((a, b))
                res.known_valid += 1
                continue
            blocked[a, b] = blocked[b, a] = True
            res.size[1] += 1
            break
        else:
            res.status, res.ids, res.path, res.cost = SOLVED, ids, [verts[i].copy() for i in ids], f32(cost)
            return res
