"""Serial restatement of the batched PRM contract — TEST INFRASTRUCTURE ONLY.

One problem at a time, every quantity an explicit np.float32 operation in the written order (one rounding per
operation), and `valid(q) -> bool` / `question(a, b) -> bool` callbacks, asked one at a time: the tests pass the CPU
oracle's validate and validate_motion, never the library.  Nothing here imports the package's planning module.
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass, field

import numpy as np

from rrtc_serial import halton

f32 = np.float32
INF = f32(np.inf)
SOLVED, NO_PATH, INVALID_ENDPOINT = 0, 3, 4


@dataclass
class SerialResult:
    status: int = NO_PATH
    path: list = field(default_factory=list)
    cost: np.float32 = INF
    iterations: int = 0
    size: list = field(default_factory=lambda: [0, 0])  # valid vertices, valid edges
    questions: int = 0                                   # candidate edges asked
    vertex_valid: np.ndarray = None                      # bool[V]
    pairs: np.ndarray = None                             # int64[m][2], a < b, in candidate order
    edge_valid: np.ndarray = None                        # bool[m]

    @property
    def solved(self):
        return self.status == SOLVED


def halton_samples(skip: int, n: int, lower, span) -> np.ndarray:
    return np.stack([halton(skip + 1 + i, lower, span) for i in range(n)])


def dist2(verts: np.ndarray, v: int) -> np.ndarray:
    """d2(v, u) for every u: the sum over the joints in order of (v[j] - u[j])^2, one rounding per operation"""
    with np.errstate(all="ignore"):
        diff = verts[v][None, :] - verts          # one rounding
        sq = diff * diff                          # one rounding
        acc = np.zeros(len(verts), f32)
        for j in range(verts.shape[1]):
            acc = acc + sq[:, j]                  # joints in order, one rounding each
    return acc


def neighbours(verts: np.ndarray, valid: np.ndarray, k: int, radius) -> list:
    """nbr(v) for every vertex (empty for an invalid one): the k valid u != v with 0 < d2 <= R2 first in (d2, id)"""
    r2 = f32(radius) * f32(radius)
    ids = np.arange(len(verts))
    out = []
    for v in range(len(verts)):
        if not valid[v]:
            out.append([])
            continue
        d2 = dist2(verts, v)
        ok = valid & (ids != v) & (d2 > 0) & (d2 <= r2)
        if v < 2:
            ok[:2] = False  # start and goal are never each other's neighbour
        cand = ids[ok]
        order = np.argsort(d2[cand], kind="stable")[:k]  # stable over ascending ids: the order (d2, id)
        out.append([int(u) for u in cand[order]])
    return out


def candidate_edges(nbr: list) -> list:
    """(0, 1) first; then for v ascending, slot ascending, u = nbr(v)[slot]: {v, u} if v < u or v is not in nbr(u)"""
    edges = [(0, 1)]
    for v, lst in enumerate(nbr):
        for u in lst:
            if v < u or v not in nbr[u]:
                edges.append((min(v, u), max(v, u)))
    return edges


def dijkstra_f32(n_vertices: int, edges, weights) -> np.ndarray:
    """g[0] = 0, g[v] = min over the edges {u, v} of fl(g[u] + w), by a heap; w = +inf relaxes nothing"""
    adj = [[] for _ in range(n_vertices)]
    for (a, b), w in zip(edges, weights):
        if np.isfinite(w):
            adj[a].append((b, f32(w)))
            adj[b].append((a, f32(w)))
    g = np.full(n_vertices, INF, f32)
    g[0] = f32(0)
    heap = [(0.0, 0)]
    done = np.zeros(n_vertices, bool)
    while heap:
        _, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v, w in adj[u]:
            c = f32(g[u] + w)
            if c < g[v]:
                g[v] = c
                heapq.heappush(heap, (float(c), v))
    return g


def sweep_fixpoint_f32(n_vertices: int, edges, weights, order=None) -> np.ndarray:
    """the same fixpoint by repeated sweeps over the edges in any order, at most n_vertices of them"""
    g = np.full(n_vertices, INF, f32)
    g[0] = f32(0)
    idx = list(range(len(edges))) if order is None else list(order)
    for _ in range(n_vertices):
        changed = False
        for e in idx:
            (a, b), w = edges[e], f32(weights[e])
            if not np.isfinite(w):
                continue
            for s, t in ((a, b), (b, a)):
                if np.isfinite(g[s]):
                    c = f32(g[s] + w)
                    if c < g[t]:
                        g[t], changed = c, True
        if not changed:
            break
    return g


def parent_walk(g: np.ndarray, edges, weights):
    """vertex ids from 0 to 1: parent(v) = the lowest id u with an edge {u, v}, fl(g[u] + w) == g[v] and g[u] < g[v];
    None where a step finds no parent (only possible below half an ulp of g) — bounded by the vertex count"""
    path, cur = [1], 1
    for _ in range(len(g)):
        if cur == 0:
            return path[::-1]
        best = None
        for (a, b), w in zip(edges, weights):
            if cur not in (a, b) or not np.isfinite(w):
                continue
            u = b if a == cur else a
            if g[u] < g[cur] and f32(g[u] + f32(w)) == g[cur] and (best is None or u < best):
                best = u
        if best is None:
            return None
        cur = best
        path.append(cur)
    return path[::-1] if cur == 0 else None


def prm_serial(start, goal, samples, valid, question, k=8, radius=np.inf) -> SerialResult:
    """samples: [n_samples][dim] (halton_samples(skip, n, lower, span), or the caller's)"""
    verts = np.vstack([np.array(start, f32)[None], np.array(goal, f32)[None], np.asarray(samples, f32)])
    res = SerialResult()
    res.vertex_valid = np.array([bool(np.isfinite(q).all()) and bool(valid(q)) for q in verts])
    res.size = [int(res.vertex_valid.sum()), 0]
    res.pairs, res.edge_valid = np.zeros((0, 2), np.int64), np.zeros(0, bool)
    if not (res.vertex_valid[0] and res.vertex_valid[1]):
        res.status = INVALID_ENDPOINT
        return res
    edges = candidate_edges(neighbours(verts, res.vertex_valid, k, radius))
    with np.errstate(all="ignore"):
        weights = [np.sqrt(dist2(verts[[a, b]], 0)[1]) for a, b in edges]  # w = sqrtf(d2), correctly rounded
    ok = np.array([bool(question(verts[a], verts[b])) for a, b in edges])  # always lower id -> higher id
    res.pairs, res.edge_valid, res.questions = np.array(edges, np.int64), ok, len(edges)
    res.size[1] = int(ok.sum())
    if ok[0]:
        res.status, res.path, res.cost = SOLVED, [verts[0].copy(), verts[1].copy()], f32(weights[0])
        return res
    res.iterations = len(verts) - 2
    kept = [e for e, v in zip(edges, ok) if v]
    kept_w = [w for w, v in zip(weights, ok) if v]
    g = dijkstra_f32(len(verts), kept, kept_w)
    if not np.isfinite(g[1]):
        return res
    ids = parent_walk(g, kept, kept_w)
    if ids is None:
        return res
    res.status, res.path, res.cost = SOLVED, [verts[i].copy() for i in ids], f32(g[1])
    return res
