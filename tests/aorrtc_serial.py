"""Serial restatement of the cost-bounded RRT-Connect contract — TEST INFRASTRUCTURE ONLY.

One problem at a time, every quantity an explicit np.float32 operation in the written order (one rounding per
operation), the counter-based uniform stream, ln32, the polar Gaussian pair and the Householder-reflected PHS sample in
integer and fp32 `+ - * / sqrt` operations only, and `question(a, b) -> bool` a callback: the tests pass the CPU
oracle's validate_motion, never the library.  The first solution is rrtc_serial's, every simplification
simplify_serial's.  Nothing here imports the package's planning module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED, _Tree, rrtc_serial
from simplify_serial import BSPLINE, SHORTCUT, cost, distance, simplify_serial

f32 = np.float32
_M32 = 0xFFFFFFFF
LN2_HI = np.array(0x3F317180, np.uint32).view(f32)[()]  # 0.693138123: 15 bits, exponent * LN2_HI is exact
LN2_LO = np.array(0x3717F7D1, np.uint32).view(f32)[()]  # 9.05800061e-6 = ln 2 - LN2_HI
SQRT2_MANTISSA = 0x3504F3                               # of fl(sqrt(2)) = 0x3FB504F3
_INV = {k: f32(1) / f32(k) for k in (11, 9, 7, 5, 3, 1)}


class Uniform:
    """U = float(hash(c * 0x9E3779B9 + seed) >> 8) * 2^-24, c pre-incremented before every draw (mod 2^32 throughout)"""

    def __init__(self, seed, counter=0):
        self.seed, self.c = int(seed) & _M32, int(counter) & _M32

    def next(self):
        self.c = (self.c + 1) & _M32
        x = (self.c * 0x9E3779B9 + self.seed) & _M32
        x ^= x >> 16
        x = (x * 0x7FEB352D) & _M32
        x ^= x >> 15
        x = (x * 0x846CA68B) & _M32
        x ^= x >> 16
        return f32(x >> 8) * f32(2.0 ** -24)  # both factors exact, the product exact


def ln32(s):
    """natural logarithm of an fp32 0 < s < 1 (normal): the mantissa reduced to (sqrt(1/2), sqrt(2)] by an integer compare,
    2 atanh((m - 1) / (m + 1)) by Horner, and exponent * ln 2 with ln 2 split into a 15-bit head and a tail"""
    bits = int(np.array(s, f32).view(np.uint32))
    e, mant = (bits >> 23) - 127, bits & 0x7FFFFF
    if mant > SQRT2_MANTISSA:
        e, mant = e + 1, mant | 0x3F000000   # m / 2, in (sqrt(1/2), 1)
    else:
        mant |= 0x3F800000                   # m in [1, sqrt(2)]
    m = np.array(mant, np.uint32).view(f32)[()]
    t = f32(m - f32(1)) / f32(m + f32(1))
    t2 = f32(t * t)
    p = _INV[11]
    for k in (9, 7, 5, 3, 1):
        p = f32(f32(p * t2) + _INV[k])
    return f32(f32(f32(e) * LN2_HI) + f32(f32(f32(e) * LN2_LO) + f32(f32(f32(2) * t) * p)))


def gaussian_pair(u: Uniform):
    """Marsaglia's polar method"""
    while True:
        u1 = f32(f32(f32(2) * u.next()) - f32(1))
        u2 = f32(f32(f32(2) * u.next()) - f32(1))
        s = f32(f32(u1 * u1) + f32(u2 * u2))
        if f32(0) < s < f32(1):
            break
    m = f32(np.sqrt(f32(f32(f32(-2) * ln32(s)) / s)))
    return f32(u1 * m), f32(u2 * m)


class PHS:
    """the prolate hyperspheroid with foci start and goal: the per-problem frame and the per-sample draw"""

    def __init__(self, start, goal, lower, span):
        self.n = len(start)
        self.start, self.goal = np.array(start, f32), np.array(goal, f32)
        self.lower = np.asarray(lower, f32)
        self.upper = (self.lower + np.asarray(span, f32)).astype(f32)
        self.dmin = distance(self.start, self.goal)
        self.centre = ((self.start + self.goal).astype(f32) * f32(0.5)).astype(f32)
        a1 = ((self.goal - self.start).astype(f32) / self.dmin).astype(f32)
        self.v = a1.copy()
        self.v[0] = f32(a1[0] + (f32(1) if a1[0] >= 0 else f32(-1)))
        vv = f32(0)
        for j in range(self.n):
            vv = f32(vv + f32(self.v[j] * self.v[j]))
        self.vv = vv

    def sample(self, u: Uniform, max_cost):
        """-> (t, in bounds)"""
        n, max_cost = self.n, f32(max_cost)
        g = []
        for _ in range((n + 3) // 2):  # ceil((n + 2) / 2) pairs
            g += gaussian_pair(u)
        g = g[:n + 2]
        acc = f32(0)
        for x in g:
            acc = f32(acc + f32(x * x))
        norm = f32(np.sqrt(acc))
        r1 = f32(max_cost * f32(0.5))
        rc = f32(f32(np.sqrt(max(f32(f32(max_cost * max_cost) - f32(self.dmin * self.dmin)), f32(0)))) * f32(0.5))
        with np.errstate(all="ignore"):
            y = np.array([f32(f32(g[j] / norm) * (r1 if j == 0 else rc)) for j in range(n)], f32)
            dot = f32(0)
            for j in range(n):
                dot = f32(dot + f32(self.v[j] * y[j]))
            k = f32(f32(f32(2) * dot) / self.vv)
            t = (self.centre + (y - (self.v * k).astype(f32)).astype(f32)).astype(f32)
        ok = bool(np.all((self.lower <= t) & (t <= self.upper)))  # NaN compares false: out of bounds
        return t, ok


class _CostTree(_Tree):
    def __init__(self, root, capacity):
        self.cost = np.zeros(capacity, f32)
        super().__init__(root, capacity)

    def add(self, q, parent, cost_=f32(0)):
        i = super().add(q, parent)
        self.cost[i] = cost_
        return i


def aox_nearest(T: _CostTree, t, c):
    """(first index with the least key among the admissible nodes, its distance), None if no key compares below +inf"""
    c = f32(c)
    diff = T.pts[:T.n] - t[None, :]
    sq = diff * diff
    acc = np.zeros(T.n, f32)
    for j in range(T.pts.shape[1]):
        acc = acc + sq[:, j]
    d = np.sqrt(acc)
    cs = T.cost[:T.n]
    with np.errstate(invalid="ignore"):
        admissible = ~(cs > 0) | ~(c < (cs + d).astype(f32))
        dc = (cs - c).astype(f32)
        key = np.sqrt(((d * d).astype(f32) + (dc * dc).astype(f32)).astype(f32))
        key = np.where(admissible & (key < np.inf), key, np.inf)
    i = int(np.argmin(key))  # numpy: the first of the least
    if not key[i] < np.inf:
        return None, f32(np.nan)
    return i, f32(d[i])


@dataclass
class SearchResult:
    status: int = SOLVED
    path: list = field(default_factory=list)
    iterations: int = 0
    size: list = field(default_factory=list)
    questions: int = 0
    out_of_bounds: int = 0
    reparents: int = 0

    @property
    def solved(self):
        return self.status == SOLVED


def aox_search(start, goal, phs: PHS, u: Uniform, question, max_cost, budget, range_=1.0, balance=True, tree_ratio=1.0,
               max_samples=8192, cost_bound_resample=True, max_cost_bound_resamples=4) -> SearchResult:
    """one cost-bounded RRT-Connect search below max_cost on fresh trees"""
    start, goal = np.array(start, f32), np.array(goal, f32)
    R, ratio, max_cost = f32(range_), f32(tree_ratio), f32(max_cost)
    res = SearchResult()

    def ask(a, b):
        res.questions += 1
        return bool(question(a, b))

    A, B = _CostTree(start, max_samples), _CostTree(goal, max_samples)
    a_is_start = True
    while res.iterations < budget and A.n + B.n < max_samples:
        res.iterations += 1
        if (not balance) or f32(np.abs(f32(A.n) - f32(B.n))) / f32(A.n) < ratio:
            A, B = B, A
            a_is_start = not a_is_start
        t, ok = phs.sample(u, max_cost)
        if not ok:
            res.out_of_bounds += 1
            continue
        g = distance(t, A.pts[0])
        f = f32(g + distance(t, B.pts[0]))
        c_range = max(f32(max_cost - f), f32(0))
        c_rand = f32(f32(u.next() * c_range) + g)
        ni, d = aox_nearest(A, t, c_rand)
        if ni is None or not (d > 0):
            continue
        near = A.pts[ni].copy()
        new = (near + (t - near) * (f32(min(d, R)) / d)).astype(f32)
        if not ask(near, new):
            continue
        new_cost = f32(A.cost[ni] + distance(new, near))
        if cost_bound_resample:
            g2 = distance(new, A.pts[0])
            for _ in range(max_cost_bound_resamples):
                cr = max(f32(new_cost - g2), f32(0))
                mi, md = aox_nearest(A, new, f32(f32(u.next() * cr) + g2))
                if mi is None or mi == ni or not (f32(A.cost[mi] + md) < new_cost) or cr == 0:
                    break
                if not ask(A.pts[mi], new):
                    break
                ni, new_cost = mi, f32(A.cost[mi] + md)
                res.reparents += 1
        new_i = A.add(new, ni, new_cost)
        bi, bd = aox_nearest(B, new, f32(max_cost - new_cost))
        if bi is None or not (f32(f32(new_cost + bd) + B.cost[bi]) < max_cost):
            continue
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
            prev = B.add(w, prev, f32(B.cost[prev] + distance(w, frm)))
            frm = w
        if connected:
            pa = A.trace(new_i)[::-1]
            pb = B.trace(prev)
            path = pa + (pb[1:] if pb[0].tobytes() == new.tobytes() else pb)
            res.path = path if a_is_start else path[::-1]
            res.size = [A.n, B.n]
            return res
    res.status = MAX_ITERATIONS if res.iterations >= budget else MAX_SAMPLES
    res.size = [A.n, B.n]
    return res


@dataclass
class AORRTCResult:
    status: int = SOLVED
    path: list = field(default_factory=list)
    iterations: int = 0
    size: list = field(default_factory=list)
    first_cost: float = float("inf")
    cost: float = float("inf")
    searches: int = 0
    improvements: int = 0
    questions: int = 0                                 # asked serially, all stages
    simplify_questions: int = 0                        # those of them the simplifications asked
    first_path: list = field(default_factory=list)     # after the first stage
    costs: list = field(default_factory=list)          # the bound after every search
    search_status: list = field(default_factory=list)  # status of every search
    out_of_bounds: int = 0
    reparents: int = 0
    tree_sizes: list = field(default_factory=list)     # [|A|, |B|] at the end of every search

    @property
    def solved(self):
        return self.status == SOLVED


def aorrtc_serial(start, goal, lower, span, question, range_=1.0, balance=True, tree_ratio=1.0, max_iterations=100000,
                  max_internal_iterations=100000, max_samples=8192, max_cost_bound_resamples=64, max_searches=0,
                  optimize=True, cost_bound_resample=True, simplify_intermediate=True, skip=0, simplify=None) -> AORRTCResult:
    """the meta loop: first solution, then searches below the best cost until the budget is spent.  `simplify`: keyword
    arguments of simplify_serial (None = its defaults); a path longer than its max_waypoints is kept as it is."""
    start, goal = np.array(start, f32), np.array(goal, f32)
    simplify = dict(simplify or {})
    res = AORRTCResult()

    def simplified(path):
        if not simplify_intermediate or len(path) > simplify.get("max_waypoints", 2048):
            return path
        s = simplify_serial(path, question, **simplify)
        res.questions += s.questions
        res.simplify_questions += s.questions
        return s.path

    first = rrtc_serial(start, goal, lower, span, question, range_=range_, balance=balance, tree_ratio=tree_ratio,
                        max_iterations=max_iterations, max_samples=max_samples, skip=skip)
    res.status, res.iterations, res.size, res.questions = first.status, first.iterations, list(first.size), first.questions
    if not first.solved:
        return res
    res.path = res.first_path = simplified(first.path)
    res.first_cost = res.cost = cost(res.path)
    if not optimize or len(res.path) == 2:
        return res
    phs, u = PHS(start, goal, lower, span), Uniform(skip)
    dmin = distance(start, goal)
    while (res.iterations < max_iterations and f32(f32(res.cost) - dmin) > f32(1e-8)
           and (max_searches == 0 or res.searches < max_searches)):
        budget = min(max_iterations - res.iterations, max_internal_iterations)
        s = aox_search(start, goal, phs, u, question, res.cost, budget, range_=range_, balance=balance,
                       tree_ratio=tree_ratio, max_samples=max_samples, cost_bound_resample=cost_bound_resample,
                       max_cost_bound_resamples=max_cost_bound_resamples)
        res.searches += 1
        res.iterations += s.iterations
        res.size, res.questions = list(s.size), res.questions + s.questions
        res.out_of_bounds, res.reparents = res.out_of_bounds + s.out_of_bounds, res.reparents + s.reparents
        res.search_status.append(s.status)
        res.tree_sizes.append(list(s.size))
        if s.solved:
            path = simplified(s.path)
            c = cost(path)
            if c < res.cost:
                res.path, res.cost = path, c
                res.improvements += 1
        res.costs.append(res.cost)
    return res


__all__ = ["AORRTCResult", "BSPLINE", "MAX_ITERATIONS", "MAX_SAMPLES", "PHS", "SHORTCUT", "SOLVED", "Uniform", "aorrtc_serial",
           "aox_nearest", "aox_search", "gaussian_pair", "ln32"]
