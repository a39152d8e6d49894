"""The serial statement of vmv_optimize_multi_constrained's contract (include/vamp_mvt_amd.h) — TEST
INFRASTRUCTURE ONLY.  tests/optimize_serial.py's loop, one path at a time in numpy float32, with the changes of the
constrained call: the input's ends are band-tested and its inner waypoints projected before the first iterate; every new
iterate is projected waypoint by waypoint, a waypoint whose projection does not converge keeps its value of the iterate
before (it is HELD); a validated iterate's edge counts where validity AND the band test of the edge say 1.

`reciprocals`, `evaluate`, `advance` and the status values are optimize_serial's own.  The callbacks:
    clearance_grad(X [N][dim]) -> (values [N][2], grads [N][2][dim])
    question(a, b) -> bool                 is the motion a -> b valid
    project(row) -> (row, converged)       the projection of one configuration
    in_band(row) -> bool                   the band test of one configuration
    band_edge(a, b) -> bool                the band test of an edge
The tests without a device pass hand-made callbacks, the device tests `product_hooks`, which asks the product's batch
calls one path at a time; each lane's answer is its own, bit for bit (tests/test_constraint_gpu.py).

`trace` has one entry per projected iterate (iterate 0 first): (moved, held), the inner waypoints' indices the projection
changed and those it could not project."""
from dataclasses import dataclass, field

import numpy as np

from optimize_serial import NO_VALID, NONFINITE, OK, Optimized, advance, evaluate, reciprocals

OUT_OF_BAND = 3  # VMV_OPT_OUT_OF_BAND


@dataclass
class ConstrainedOptimized(Optimized):
    held: int = 0
    trace: list = field(default_factory=list)  # per projected iterate: (indices moved, indices held)


def product_hooks(mod, constraint, constraint_settings=None):
    """-> dict(project=, in_band=, band_edge=) asking the product.  project and band_edge carry `rows = True`: they take
    the rows of one path at once ([n][dim] -> ([n][dim], bool [n]); ([m][dim], [m][dim]) -> bool [m]), one call per path
    and iterate instead of one per waypoint"""
    f32 = np.float32

    def project(rows):
        out, _, converged, _ = mod.project_batch(np.ascontiguousarray(rows, f32), constraint, constraint_settings)
        return np.asarray(out, f32), np.asarray(converged, bool)

    def band_edge(a, b):
        return np.asarray(mod.constraint_check_motion_batch(np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32), constraint,
                                                            constraint_settings), bool)

    def in_band(q):
        return bool(mod.constraint_check_batch(np.ascontiguousarray(q, f32)[None], constraint, constraint_settings)[0])

    project.rows = band_edge.rows = True
    return dict(project=project, in_band=in_band, band_edge=band_edge)


def _project_rows(project, rows):
    """project over the rows of an array -> (rows, converged)"""
    if getattr(project, "rows", False):
        return project(rows)
    pairs = [project(r) for r in rows]
    return np.stack([np.asarray(p[0], rows.dtype) for p in pairs]), np.array([bool(p[1]) for p in pairs])


def _band_edges(band_edge, X):
    """the band test of every consecutive edge of X -> bool array"""
    if getattr(band_edge, "rows", False):
        return band_edge(X[:-1], X[1:])
    return np.array([bool(band_edge(a, b)) for a, b in zip(X[:-1], X[1:])])


def optimize_constrained_serial(path, clearance_grad, question, project, in_band, band_edge, lower, upper, max_iterations=64,
                                validate_every=8, step=1.0 / 40.0, max_step=0.1, min_change=1e-4, smooth_weight=1.0, env_weight=1.0,
                                self_weight=1.0, env_margin=0.05, self_margin=0.01):
    dtype = np.float32
    F = np.float32
    if len(path) == 0:
        return ConstrainedOptimized(path=[])
    X = np.array(path, dtype).reshape(len(path), -1)
    out = ConstrainedOptimized(path=[q.copy() for q in X])
    if not np.isfinite(X).all():
        out.status = NONFINITE
        return out
    N = len(X)
    if N < 2:
        return out
    # change 1: the input is looked at first
    if not (in_band(X[0]) and in_band(X[-1])):
        out.status = OUT_OF_BAND
        return out
    if N == 2:
        out.status = OK if (question(X[0], X[1]) and bool(_band_edges(band_edge, X)[0])) else NO_VALID
        return out
    rows, converged = _project_rows(project, X[1:-1])
    if not converged.all():
        out.status = OUT_OF_BAND
        return out
    moved = [i + 1 for i in range(N - 2) if rows[i].tobytes() != X[i + 1].tobytes()]
    out.trace.append((moved, []))
    X = X.copy()
    X[1:-1] = rows  # iterate 0
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
            # change 3: validity AND the band test of the edge
            valid = bool(_band_edges(band_edge, X).all()) and all(question(a, b) for a, b in zip(X[:-1], X[1:]))
            if valid and (best is None or U < out.cost):  # the first of equal costs stays
                best = X.copy()
                out.best_iteration, out.cost, out.clearance = k, U, (env, slf)
            out.iterations = k
        out.history.append((U, env, slf, validated, valid))
        if validated and (k >= max_iterations or (k > 0 and change < F(min_change))):
            break
        Xs, change = advance(X, values, grads, s, r, lower, upper)  # the step's size is that of the unprojected step
        # change 2: every inner waypoint becomes its projection, or stays as it was in iterate k
        rows, converged = _project_rows(project, Xs[1:-1])
        Xn = X.copy()
        Xn[1:-1] = np.where(converged[:, None], rows, X[1:-1])
        held = [i + 1 for i in range(N - 2) if not converged[i]]
        moved = [i + 1 for i in range(N - 2) if converged[i] and rows[i].tobytes() != Xs[i + 1].tobytes()]
        out.held += len(held)
        out.trace.append((moved, held))
        X = Xn
    if best is None:
        out.status = NO_VALID  # the input's bytes, not iterate 0
    else:
        out.path = [q.copy() for q in best]
    return out
