"""Serial restatement of vmv_aorrtc_multi_constrained (include/vamp_mvt_amd.h) — TEST INFRASTRUCTURE ONLY.

The meta loop is tests/aorrtc_serial.py's with its three parts replaced: the first solution is rrtc_constrained_serial's
(one goal), every simplification simplify_constrained_serial's, and a search is aorrtc_serial.aox_search, imported as it
is, with a `question(a, b)` that carries the constraint.  aox_search computes every quantity it derives from a new node
after the question, from the array it handed over, so the in-place hook of rrtc_constrained_serial carries over: where b
is a NEW node (the extension's `new`, a march step's point) it is projected, refused if the projection fails or lands
farther than max_stretch * range from a, else replaced in place; then the edge's band test is ANDed into the answer.  A
re-parent question A[mi] -> new hands over the very array the accepted extension handed over: it is already projected,
so it is band-checked only, with no stretch test.

The constraint is answered through the product's batch calls one question at a time (`mod`: project_batch,
constraint_check_batch, constraint_check_motion_batch), which is legitimate for the reason rrtc_constrained_serial gives;
validity is the caller's `valid(a, b)` (the CPU oracle).  The tests without a device pass a `mod` that lets everything
through."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from aorrtc_serial import PHS, AORRTCResult, Uniform, aox_search
from rrtc_constrained_serial import INVALID_ENDPOINT, _dist, rrtc_constrained_serial
from simplify_constrained_serial import OUT_OF_BAND, product_hooks, simplify_constrained_serial
from simplify_serial import cost, distance

f32 = np.float32


@dataclass
class ConstrainedAORRTCResult(AORRTCResult):
    band_refused: int = 0        # questions the constraint answered 0, all stages (the simplifier's: its serial count)
    first_refused: int = 0       # of them: the first stage's
    search_refused: int = 0      # of them: the searches'
    simplify_refused: int = 0    # of them: the simplifications'
    out_of_band_simplifications: int = 0  # simplifications that ended OUT_OF_BAND (the path stayed as it was)
    search_refused_each: list = field(default_factory=list)  # per search


def aorrtc_constrained_serial(mod, start, goal, lower, span, valid, constraint, constraint_settings=None, max_stretch=2.0,
                              range_=1.0, balance=True, tree_ratio=1.0, max_iterations=100000, max_internal_iterations=100000,
                              max_samples=8192, max_cost_bound_resamples=64, max_searches=0, optimize=True,
                              cost_bound_resample=True, simplify_intermediate=True, skip=0,
                              simplify=None) -> ConstrainedAORRTCResult:
    """mod: the product's robot; constraint: the problem's EEConstraint; the other arguments are aorrtc_serial's"""
    start, goal = np.array(start, f32), np.array(goal, f32)
    simplify = dict(simplify or {})
    hooks = product_hooks(mod, constraint, constraint_settings)
    res = ConstrainedAORRTCResult()

    def simplified(path):
        if not simplify_intermediate or len(path) > simplify.get("max_waypoints", 2048):
            return path
        s = simplify_constrained_serial(path, valid, hooks, **simplify)
        res.questions += s.questions
        res.simplify_questions += s.questions
        res.band_refused += s.band_refused
        res.simplify_refused += s.band_refused
        if s.status == OUT_OF_BAND:  # the path stays as it is, and so does its cost
            res.out_of_band_simplifications += 1
            return path
        return s.path

    first = rrtc_constrained_serial(mod, start, goal[None], lower, span, valid, constraint, constraint_settings, max_stretch, range_,
                                    balance=balance, tree_ratio=tree_ratio, max_iterations=max_iterations, max_samples=max_samples,
                                    skip=skip)
    res.status, res.iterations, res.size, res.questions = first.status, first.iterations, list(first.size), first.questions
    res.band_refused = res.first_refused = first.band_refused
    if not first.solved:  # INVALID_ENDPOINT among them: no question, no path
        return res
    res.path = res.first_path = simplified(first.path)
    res.first_cost = res.cost = cost(res.path)
    if not optimize or len(res.path) == 2:
        return res

    stretch = f32(f32(max_stretch) * f32(range_))
    projected = [None]  # the array of the last new node the constraint let through
    refused = [0]

    def question(a, b):
        if b is not projected[0]:  # a new node: the extension's `new`, a march step's point
            q, _, converged, _ = mod.project_batch(b[None], constraint, constraint_settings)
            if not converged[0] or not _dist(q[0], a) <= stretch:
                refused[0] += 1
                return False  # the node stays as written; the answer is 0
            b[:] = q[0]
            projected[0] = b
        # (else a re-parent A[mi] -> new: `new` is projected already; the band test alone, no stretch test)
        in_band = bool(mod.constraint_check_motion_batch(a[None], b[None], constraint, constraint_settings)[0])
        refused[0] += not in_band
        return bool(valid(a, b)) and in_band

    phs, u = PHS(start, goal, lower, span), Uniform(skip)  # the sample t itself is never projected
    dmin = distance(start, goal)
    while (res.iterations < max_iterations and f32(f32(res.cost) - dmin) > f32(1e-8)
           and (max_searches == 0 or res.searches < max_searches)):
        budget = min(max_iterations - res.iterations, max_internal_iterations)
        before = refused[0]
        s = aox_search(start, goal, phs, u, question, res.cost, budget, range_=range_, balance=balance, tree_ratio=tree_ratio,
                       max_samples=max_samples, cost_bound_resample=cost_bound_resample,
                       max_cost_bound_resamples=max_cost_bound_resamples)
        res.searches += 1
        res.iterations += s.iterations
        res.size, res.questions = list(s.size), res.questions + s.questions
        res.out_of_bounds, res.reparents = res.out_of_bounds + s.out_of_bounds, res.reparents + s.reparents
        res.search_status.append(s.status)
        res.tree_sizes.append(list(s.size))
        res.search_refused_each.append(refused[0] - before)
        res.search_refused += refused[0] - before
        res.band_refused += refused[0] - before
        if s.solved:
            path = simplified(s.path)
            c = cost(path)
            if c < res.cost:
                res.path, res.cost = path, c
                res.improvements += 1
        res.costs.append(res.cost)
    return res


__all__ = ["ConstrainedAORRTCResult", "INVALID_ENDPOINT", "aorrtc_constrained_serial"]
