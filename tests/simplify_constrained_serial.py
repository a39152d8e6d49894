"""Serial restatement of vmv_simplify_multi_constrained (include/vamp_mvt_amd.h) — TEST INFRASTRUCTURE ONLY.

tests/simplify_serial.py's loop, one path at a time and ONE QUESTION AT A TIME, with the three changes of the constrained
call: every question is validity AND the band test of the edge; a B-spline candidate is projected before it is asked and
replaces its waypoint only if it is farther than min_change from it; the input is band-checked before anything else.

Validity is the caller's `valid(a, b)` (the CPU oracle).  The constraint is answered by a `Hooks` object: the tests without
a device pass hand-made callbacks, the device tests `product_hooks`, which asks the product's project_batch,
constraint_check_batch and constraint_check_motion_batch one question at a time.  That is legitimate for the reason
tests/rrtc_constrained_serial.py gives: each lane's answer is its own, bit for bit (tests/test_constraint_gpu.py).

`trace` has simplify_serial's format, so windowed_questions / windowed_rounds apply; `asked` records per question
(kind, refused by the band, validity's own answer - None where a failed projection left no edge to ask), `projected` per
B-spline candidate (step, index, converged, moved by the projection, replaced its waypoint)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from simplify_serial import BSPLINE, CAPACITY, SHORTCUT, SerialSimplifyResult, _Capacity, _subdivide, distance, interpolate

f32 = np.float32
OUT_OF_BAND = 2  # VMV_SIMPLIFY_OUT_OF_BAND


@dataclass
class Hooks:
    band_point: object  # q -> bool: the band test of one configuration
    band_edge: object   # (a, b) -> bool: the band test of an edge
    project: object     # q -> (q_p, converged)


def product_hooks(mod, constraint, constraint_settings=None) -> Hooks:
    def project(q):
        out, _, converged, _ = mod.project_batch(q[None], constraint, constraint_settings)
        return out[0].astype(f32), bool(converged[0])

    return Hooks(band_point=lambda q: bool(mod.constraint_check_batch(q[None], constraint, constraint_settings)[0]),
                 band_edge=lambda a, b: bool(mod.constraint_check_motion_batch(a[None], b[None], constraint, constraint_settings)[0]),
                 project=project)


@dataclass
class SerialConstrainedResult(SerialSimplifyResult):
    band_refused: int = 0
    asked: list = field(default_factory=list)      # (kind, refused, valid) per serial question
    projected: list = field(default_factory=list)  # (step, index, converged, moved, replaced) per B-spline candidate


def simplify_constrained_serial(path, valid, hooks: Hooks, max_iterations=4, operations=(SHORTCUT, BSPLINE), max_steps=5,
                                min_change=0.05, midpoint_interpolation=0.5, max_waypoints=2048) -> SerialConstrainedResult:
    pts = [np.array(q, f32) for q in path]
    res = SerialConstrainedResult()
    min_change = f32(min_change)
    if len(pts) > max_waypoints:
        raise ValueError("max_waypoints is below the input's length")
    for op in operations:
        if op not in (SHORTCUT, BSPLINE):
            raise ValueError(op)

    def ask(kind, a, b, in_band=None):
        """validity AND band; in_band False: the projection failed, the band's answer is 0 without a test"""
        res.questions += 1
        band = bool(hooks.band_edge(a, b)) if in_band is None else in_band
        ok = bool(valid(a, b)) if in_band is None else None
        res.band_refused += not band
        res.asked.append((kind, not band, ok))
        return bool(ok) and band

    def shortcut():
        if len(pts) < 3:
            return False
        result, i = False, 0
        while i < len(pts) - 2:  # re-evaluated after every erase
            candidates, found = len(pts) - i - 2, None
            for j in range(len(pts) - 1, i + 1, -1):
                if ask("shortcut", pts[i], pts[j]):
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
                if distance(pts[index], mid) > min_change:  # false for NaN; on the unprojected mid
                    mid_p, converged = hooks.project(mid)
                    mid_p = np.array(mid_p, f32)
                    moved = converged and mid_p.tobytes() != mid.tobytes()
                    if not converged:  # both motions are answered 0; the serial loop asks the first only
                        first, second = ask("bspline", pts[index - 1], mid, in_band=False), None
                    else:
                        first = ask("bspline", pts[index - 1], mid_p)
                        second = ask("bspline", mid_p, pts[index + 1]) if first else None
                    passed.append((index, first, second))
                    replaced = bool(first and second and distance(pts[index], mid_p) > min_change)
                    res.projected.append((step, index, converged, moved, replaced))
                    if replaced:
                        pts[index] = mid_p
                        changed = updated = True
            res.trace.append(("bspline", step, len(pts), passed))
            if not updated:
                break
        return changed

    if len(pts) < 3:  # as they are, without any test
        res.path = pts
        return res
    if not hooks.band_point(pts[0]) or not all(hooks.band_edge(a, b) for a, b in zip(pts[:-1], pts[1:])):
        res.status, res.path = OUT_OF_BAND, pts  # the input's bytes, 0 iterations, 0 questions
        return res
    res.trace.append(("direct",))
    if ask("direct", pts[0], pts[-1]):
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
