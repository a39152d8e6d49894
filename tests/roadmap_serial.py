"""Serial restatement of the kept-roadmap contract — TEST INFRASTRUCTURE ONLY.

A roadmap is built once over its samples alone (no endpoint takes part, samples 0 and 1 are ordinary vertices) and
then asked any number of (start, goal) queries.  Every quantity is an explicit np.float32 operation in the written
order, and `valid(q) -> bool` / `question(a, b) -> bool` are callbacks asked one at a time: the tests pass the CPU
oracle's validate and validate_motion, never the library.  Nothing here imports the package's planning module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from prm_serial import INF, INVALID_ENDPOINT, NO_PATH, SOLVED, dijkstra_f32, dist2, f32, halton_samples, parent_walk  # noqa: F401


@dataclass
class SerialRoadmap:
    samples: np.ndarray        # [n_samples][dim]
    vertex_valid: np.ndarray   # bool[n_samples]
    pairs: np.ndarray          # int64[m][2] sample ids a < b, in candidate order
    edge_valid: np.ndarray     # bool[m]
    weights: list              # [m] np.float32


@dataclass
class SerialQuery:
    status: int = NO_PATH
    path: list = field(default_factory=list)
    cost: np.float32 = INF
    iterations: int = 0
    size: list = field(default_factory=lambda: [0, 0])  # valid connection edges of the start, of the goal
    questions: int = 0                                   # 1 + |conn(start)| + |conn(goal)|
    conn: list = field(default_factory=lambda: [[], []])  # conn(start), conn(goal): sample ids

    @property
    def solved(self):
        return self.status == SOLVED


def _finite_and_valid(q, valid):
    return bool(np.isfinite(q).all()) and bool(valid(q))


def weight(a, b):
    """w = sqrtf(d2(a, b)), correctly rounded"""
    with np.errstate(all="ignore"):
        return np.sqrt(dist2(np.stack([a, b]), 0)[1])


def nearest_valid(q, samples, valid, k, radius, exclude=None) -> list:
    """the k valid samples u (u != exclude) with 0 < d2(q, u) <= R2 that come first in the order (d2, id)"""
    r2 = f32(radius) * f32(radius)
    d2 = dist2(np.vstack([np.asarray(q, f32)[None], samples]), 0)[1:]
    ids = np.arange(len(samples))
    with np.errstate(invalid="ignore"):
        ok = valid & (d2 > 0) & (d2 <= r2)
    if exclude is not None:
        ok &= ids != exclude
    cand = ids[ok]
    order = np.argsort(d2[cand], kind="stable")[:k]  # stable over ascending ids: the order (d2, id)
    return [int(u) for u in cand[order]]


def neighbours(samples, valid, k, radius) -> list:
    """nbr(v) for every sample (empty for an invalid one); no endpoint rule: every sample is an ordinary vertex"""
    return [nearest_valid(samples[v], samples, valid, k, radius, exclude=v) if valid[v] else [] for v in range(len(samples))]


def candidate_edges(nbr: list) -> list:
    """for v ascending, slot ascending, u = nbr(v)[slot]: {v, u} if v < u or v is not in nbr(u)"""
    return [(min(v, u), max(v, u)) for v, lst in enumerate(nbr) for u in lst if v < u or v not in nbr[u]]


def build_serial(samples, valid, question, k=8, radius=np.inf) -> SerialRoadmap:
    samples = np.asarray(samples, f32)
    vertex_valid = np.array([_finite_and_valid(q, valid) for q in samples])
    edges = candidate_edges(neighbours(samples, vertex_valid, k, radius))
    weights = [weight(samples[a], samples[b]) for a, b in edges]
    ok = np.array([bool(question(samples[a], samples[b])) for a, b in edges], bool)  # always lower id -> higher id
    return SerialRoadmap(samples, vertex_valid, np.array(edges, np.int64).reshape(-1, 2), ok, weights)


def query_serial(rm: SerialRoadmap, start, goal, valid, question, k_connect=8, radius=np.inf) -> SerialQuery:
    ends = [np.array(start, f32), np.array(goal, f32)]
    res = SerialQuery()
    if not (_finite_and_valid(ends[0], valid) and _finite_and_valid(ends[1], valid)):
        res.status = INVALID_ENDPOINT
        return res
    res.conn = [nearest_valid(e, rm.samples, rm.vertex_valid, k_connect, radius) for e in ends]
    res.questions = 1 + len(res.conn[0]) + len(res.conn[1])
    direct = bool(question(ends[0], ends[1]))
    answers = [[bool(question(e, rm.samples[u])) for u in lst] for e, lst in zip(ends, res.conn)]  # endpoint -> sample
    res.size = [sum(answers[0]), sum(answers[1])]
    if direct:
        res.status, res.path, res.cost = SOLVED, [ends[0].copy(), ends[1].copy()], f32(weight(ends[0], ends[1]))
        return res
    res.iterations = len(rm.samples)
    edges = [(2 + int(a), 2 + int(b)) for (a, b), ok in zip(rm.pairs, rm.edge_valid) if ok]
    weights = [w for w, ok in zip(rm.weights, rm.edge_valid) if ok]
    for e in (0, 1):
        for u, ok in zip(res.conn[e], answers[e]):
            if ok:
                edges.append((e, 2 + u))
                weights.append(weight(ends[e], rm.samples[u]))
    g = dijkstra_f32(len(rm.samples) + 2, edges, weights)
    if not np.isfinite(g[1]):
        return res
    ids = parent_walk(g, edges, weights)
    if ids is None:
        return res
    verts = ends + list(rm.samples)
    res.status, res.path, res.cost = SOLVED, [verts[i].copy() for i in ids], f32(g[1])
    return res
