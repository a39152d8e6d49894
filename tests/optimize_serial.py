"""The serial statement of vmv_optimize_multi's contract (include/vamp_mvt_amd.h): one path at a time in numpy,
every operation written once in the order the contract names, in `dtype` arithmetic (float32: what the device must
reproduce bit for bit; float64: the defaults study).  It takes two callbacks and knows nothing of the package:
    clearance_grad(X [N][dim]) -> (values [N][2], grads [N][2][dim])      the two clearances and their gradients
    question(a, b) -> bool                                                 is the motion a -> b valid
The iteration: cost and gradient from the callback's answers, the tridiagonal solve by the Thomas recurrence on
precomputed reciprocals, the step capped in the L-infinity norm over the whole path, clipped to the joint bounds; iterates
0, v, 2v, ... and max_iterations are validated and the cheapest valid one is kept."""
from dataclasses import dataclass, field

import numpy as np

OK, NO_VALID, NONFINITE = 0, 1, 2


@dataclass
class Optimized:
    path: list
    status: int = OK
    iterations: int = 0
    best_iteration: int = 0
    cost_first: float = 0.0
    cost: float = 0.0
    clearance_first: tuple = (np.float32(np.nan), np.float32(np.nan))
    clearance: tuple = (np.float32(np.nan), np.float32(np.nan))
    history: list = field(default_factory=list)  # per iterate: (U, min env, min self, validated, valid)


def reciprocals(n, dtype=np.float32):
    """r_0 = 1 / 2, r_i = 1 / (2 - r_{i-1}): the reciprocals of the Thomas pivots of the n x n tridiagonal (-1, 2, -1)"""
    F = np.dtype(dtype).type
    r = np.zeros(max(n, 1), dtype)
    r[0] = F(0.5)
    for i in range(1, n):
        r[i] = F(1) / (F(2) - r[i - 1])
    return r


def solve(G, r):
    """A z = G per column, A = tridiag(-1, 2, -1): d_0 = G_0, d_i = G_i + r_{i-1} d_{i-1}; z_{n-1} = d_{n-1} r_{n-1},
    z_i = (d_i + z_{i+1}) r_i.  Multiplications and additions only, in G's dtype."""
    z = np.array(G, copy=True)
    n = len(z)
    for i in range(1, n):
        z[i] = z[i] + r[i - 1] * z[i - 1]
    z[n - 1] = z[n - 1] * r[n - 1]
    for i in range(n - 2, -1, -1):
        z[i] = (z[i] + z[i + 1]) * r[i]
    return z


def hinge(v, eps):
    """CHOMP's hinge and its slope; +inf and NaN give 0"""
    F = v.dtype.type
    with np.errstate(all="ignore"):
        d = v - eps
        c = np.where(v < 0, (F(0) - v) + F(0.5) * eps, np.where(v <= eps, (d * d) / (F(2) * eps), F(0)))
        s = np.where(v < 0, F(-1), np.where(v <= eps, d / eps, F(0)))
    return c.astype(v.dtype), s.astype(v.dtype)


def ordered_min(v):
    """the minimum under the total order that puts -0 below +0, NaN left out, +inf if nothing is left"""
    v = np.asarray(v)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return v.dtype.type(np.inf)
    u = np.uint32 if v.dtype == np.float32 else np.uint64
    top = u(1) << u(v.dtype.itemsize * 8 - 1)
    b = v.view(u)
    key = np.where(b & top, ~b, b | top)
    return v[int(np.argmin(key))]


def evaluate(X, values, s):
    """U of iterate X and its waypoint minima; `values` [N][2]"""
    F = X.dtype.type
    d = X[1:] - X[:-1]
    sq = np.zeros(len(X) - 1, X.dtype)
    for j in range(X.shape[1]):
        sq = sq + d[:, j] * d[:, j]
    t = s["w_smooth"] * (F(0.5) * sq)
    ce = hinge(values[1:-1, 0], s["eps_env"])[0]
    cs = hinge(values[1:-1, 1], s["eps_self"])[0]
    t[1:] = t[1:] + (s["w_env"] * ce + s["w_self"] * cs)
    return np.cumsum(t, dtype=X.dtype)[-1], ordered_min(values[:, 0]), ordered_min(values[:, 1])  # (cumsum: ascending, one add each)


def advance(X, values, grads, s, r, lower, upper):
    """the next iterate and the size of the step into it"""
    F = X.dtype.type
    sm = ((F(2) * X[1:-1]) - X[:-2]) - X[2:]
    de = s["w_env"] * hinge(values[1:-1, 0], s["eps_env"])[1]
    ds = s["w_self"] * hinge(values[1:-1, 1], s["eps_self"])[1]
    with np.errstate(all="ignore"):
        G = s["w_smooth"] * sm
        G = G + de[:, None] * grads[1:-1, 0]
        G = G + ds[:, None] * grads[1:-1, 1]
        D = (F(0) - s["step"]) * solve(G, r)
        ad = np.abs(D).ravel()
        ad = ad[~np.isnan(ad)]
        m = ad.max() if len(ad) else F(0)
        scale = s["max_step"] / (m if m > s["max_step"] else s["max_step"])
        v = X[1:-1] + D * scale
        v = np.where(v < lower, lower, np.where(v > upper, upper, v)).astype(X.dtype)
    Xn = X.copy()
    Xn[1:-1] = v
    return Xn, m * scale


def optimize_serial(path, clearance_grad, question, lower, upper, max_iterations=64, validate_every=8, step=1.0 / 40.0,
                    max_step=0.1, min_change=1e-4, smooth_weight=1.0, env_weight=1.0, self_weight=1.0, env_margin=0.05,
                    self_margin=0.01, dtype=np.float32):
    F = np.dtype(dtype).type
    if len(path) == 0:
        return Optimized(path=[])
    X = np.array(path, dtype).reshape(len(path), -1)
    out = Optimized(path=[q.copy() for q in X])
    if not np.isfinite(X).all():
        out.status = NONFINITE
        return out
    N = len(X)
    if N < 3:
        if N == 2:
            out.status = OK if question(X[0], X[1]) else NO_VALID
        return out
    s = dict(step=F(step), max_step=F(max_step), w_smooth=F(smooth_weight), w_env=F(env_weight), w_self=F(self_weight),
             eps_env=F(env_margin), eps_self=F(self_margin))
    lower, upper = np.asarray(lower, dtype), np.asarray(upper, dtype)
    r = reciprocals(N - 2, dtype)
    best = None
    change = F(0)
    for k in range(max_iterations + 1):
        values, grads = clearance_grad(X)
        values, grads = np.asarray(values, dtype), np.asarray(grads, dtype)
        U, env, slf = evaluate(X, values, s)
        if k == 0:
            out.cost_first = out.cost = U
            out.clearance_first = out.clearance = (env, slf)
        validated = k % validate_every == 0 or k == max_iterations
        valid = None
        if validated:
            valid = all(question(a, b) for a, b in zip(X[:-1], X[1:]))
            if valid and (best is None or U < out.cost):  # the first of equal costs stays
                best = X.copy()
                out.best_iteration, out.cost, out.clearance = k, U, (env, slf)
            out.iterations = k
        out.history.append((U, env, slf, validated, valid))
        if validated and (k >= max_iterations or (k > 0 and change < F(min_change))):
            break
        X, change = advance(X, values, grads, s, r, lower, upper)
    if best is None:
        out.status = NO_VALID
    else:
        out.path = [q.copy() for q in best]
    return out
