"""The Python side of the planner and path calls, characterised: what `<robot>.*_raw` and the `planning.*` functions above
them refuse and with which words, which check wins where two apply, what an accepted call hands to the library, and
what it makes of the library's answer.

Table-driven: `_base` gives each wrapper's good arguments, REFUSALS / PLAN_REFUSALS the ways to spoil them, ACCEPTED the
calls that go through.  The expectation of every (wrapper, case) is recorded in tests/golden/planner_call_python.json
(`python tests/test_planner_call_python.py --record` rewrites it) and, for the constrained, cartesian and retime wrappers,
in tests/golden/planner_call_python_paths.json next to it.  No case reaches the real library, so the test
behaves the same with or without a device:

  * a refusal runs against a library that raises on any use; the record is the exception's type and words.  A spoiled
    value the checks let through shows as "AssertionError: library called: <first symbol>", which pins the accepted side
    of every bound as well;
  * an accepted call runs against `_Recorder`, which notes what the entry symbol was given (sizes, the contents of every
    input array, which optional pointers were None, the settings struct's bytes), hands out a fake handle, fills the
    readout buffers with fixed patterns and counts the destroy calls.  The record is that, the returned dict or result
    objects field by field, and for the "fails at" cases the VmvError and that the handle was still destroyed.

The limits on n_problems * (samples, neighbours, questions) products need tens of millions of problems to trip and are
left out.  Environments are fresh `Environment()` objects, given up again while the stand-in is installed, so that no
fake handle ever reaches the real library; the None -> empty-environment path is the existing refusal tests'."""
import ctypes
import hashlib
import json
import os
from dataclasses import fields, is_dataclass, replace

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_call_python.json")
GOLDEN_PATHS = GOLDEN[:-5] + "_paths.json"  # the constrained, cartesian and retime wrappers, characterised later
DIM = 7  # panda
N = 3    # problems or paths of a call
GOAL_COUNTS = (1, 2, 1)
PLANS_HANDLE, ROADMAPS_HANDLE = 0xBEEF, 0x77
WRAPPERS = ("rrtc_multi_raw", "rrtc_multi_goals_raw", "aorrtc_multi_raw", "prm_multi_raw", "fcit_multi_raw",
            "roadmaps_build_raw", "roadmaps_query_raw", "simplify_multi_raw", "optimize_multi_raw",
            "rrtc_multi_constrained_raw", "simplify_multi_constrained_raw", "optimize_multi_constrained_raw",
            "cartesian_multi_raw", "retime_multi_raw", "retime_multi_constrained_raw")
# per wrapper: the symbols an accepted call goes through, the entry first (prm: with keep_roadmaps)
SYMBOLS = {
    "rrtc_multi_raw": ("vmv_rrtc_multi", "vmv_plans_summary", "vmv_plans_paths"),
    "rrtc_multi_goals_raw": ("vmv_rrtc_multi_goals", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_goal_indices"),
    "aorrtc_multi_raw": ("vmv_aorrtc_multi", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_costs"),
    "prm_multi_raw": ("vmv_prm_multi", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_roadmap_summary",
                      "vmv_plans_roadmap_vertices", "vmv_plans_roadmap_edges"),
    "fcit_multi_raw": ("vmv_fcit_multi", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_fcit_summary"),
    "roadmaps_build_raw": ("vmv_roadmaps_build",),
    "roadmaps_query_raw": ("vmv_roadmaps_query", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_query_summary"),
    "simplify_multi_raw": ("vmv_simplify_multi", "vmv_paths_summary", "vmv_paths_points"),
    "optimize_multi_raw": ("vmv_optimize_multi", "vmv_optimized_summary", "vmv_optimized_points"),
    "rrtc_multi_constrained_raw": ("vmv_rrtc_multi_constrained", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_goal_indices",
                                   "vmv_plans_band_refused"),
    "simplify_multi_constrained_raw": ("vmv_simplify_multi_constrained", "vmv_paths_summary", "vmv_paths_points",
                                       "vmv_paths_band_refused"),
    "optimize_multi_constrained_raw": ("vmv_optimize_multi_constrained", "vmv_optimized_held", "vmv_optimized_summary",
                                       "vmv_optimized_points"),
    "cartesian_multi_raw": ("vmv_cartesian_multi", "vmv_cartesian_summary", "vmv_cartesian_points"),
    "retime_multi_raw": ("vmv_retime_multi", "vmv_retime_summary", "vmv_retime_samples"),
    "retime_multi_constrained_raw": ("vmv_retime_multi_constrained", "vmv_retime_summary", "vmv_retime_levels", "vmv_retime_samples"),
}
DESTROY = {w: "vmv_plans_destroy" for w in WRAPPERS}
DESTROY.update(roadmaps_build_raw=None, simplify_multi_raw="vmv_paths_destroy", optimize_multi_raw="vmv_optimized_destroy",
               simplify_multi_constrained_raw="vmv_paths_destroy", optimize_multi_constrained_raw="vmv_optimized_destroy",
               cartesian_multi_raw="vmv_cartesian_destroy", retime_multi_raw="vmv_retime_destroy",
               retime_multi_constrained_raw="vmv_retime_destroy")
# the arguments of every entry symbol, by kind
_PROBLEMS = ("robot", "envs", "n", "starts", "goals", "skips", "settings", "handle")
_SAMPLED = ("robot", "envs", "n", "starts", "goals", "skips", "samples", "settings", "handle")
_PATHS = ("robot", "envs", "n", "points", "offsets", "settings", "handle")
_BAND = ("constraints", "n_constraints", "constraint_settings", "handle")
_TIMED = ("robot", "envs", "n", "points", "offsets", "vel", "acc")
ENTRIES = {
    "vmv_rrtc_multi": _PROBLEMS,
    "vmv_rrtc_multi_goals": ("robot", "envs", "n", "starts", "packed_goals", "goal_offsets", "skips", "settings", "handle"),
    "vmv_aorrtc_multi": _PROBLEMS,
    "vmv_prm_multi": _SAMPLED,
    "vmv_fcit_multi": _SAMPLED,
    "vmv_roadmaps_build": ("robot", "envs", "n", "skips", "samples", "settings", "handle"),
    "vmv_roadmaps_query": ("roadmaps", "n", "index", "starts", "goals", "settings", "handle"),
    "vmv_simplify_multi": _PATHS,
    "vmv_optimize_multi": _PATHS,
    "vmv_rrtc_multi_constrained": ("robot", "envs", "n", "starts", "packed_goals", "goal_offsets", "skips", "settings") + _BAND,
    "vmv_simplify_multi_constrained": _PATHS[:-1] + _BAND,
    "vmv_optimize_multi_constrained": _PATHS[:-1] + _BAND,
    "vmv_cartesian_multi": ("robot", "envs", "n", "starts", "targets", "settings", "handle"),
    "vmv_retime_multi": _TIMED + ("settings", "handle"),
    "vmv_retime_multi_constrained": _TIMED + ("constraints", "n_constraints", "settings", "constraint_settings", "handle"),
}


# ---------------------------------------------------------------------------------------------------------
# the two stand-ins for vamp_mvt_amd.lib
# ---------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def _get(pointer, count):
    if count == 0:
        return np.zeros(0, np.dtype(pointer._type_))
    return np.ctypeslib.as_array(pointer, shape=(count,)).copy()


def _put(pointer, values):
    values = np.asarray(values).reshape(-1)
    if values.size:
        np.ctypeslib.as_array(pointer, shape=(values.size,))[:] = values


class _Recorder:
    """answers every symbol the planner wrappers use; `fail`: the symbol that returns VMV_ERR_INVALID_ARGUMENT"""

    def __init__(self, fail=None):
        self.fail, self.calls, self.entry, self.destroyed = fail, [], None, {}
        self.n = self.ns = self.environments = 0
        self.lengths = np.zeros(0, np.int64)

    def __getattr__(self, name):
        if not name.startswith("vmv_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        if name == "vmv_get_device":
            return 0
        if name == "vmv_env_create":
            self.environments += 1
            args[0]._obj.value = 0x1000 + self.environments
            return 0
        if name in ("vmv_env_finalize", "vmv_env_destroy"):
            return 0
        self.calls.append(name)
        if name.endswith("_destroy"):
            self.destroyed[name] = self.destroyed.get(name, 0) + 1
            return 0
        if name == self.fail:
            return 1
        if name in ENTRIES:
            self.entry = self._entry(name, args)
        else:
            getattr(self, "_" + name)(*args)
        return 0

    def _entry(self, name, args):
        spec = ENTRIES[name]
        assert len(args) == len(spec), name
        a = dict(zip(spec, args))
        n = self.n = int(a["n"])
        cs = a["settings"]._obj
        self.ns = int(getattr(cs, "n_samples", 0))
        offsets = next((a[k] for k in ("goal_offsets", "offsets") if a.get(k) is not None), None)
        total = self.total = n if offsets is None else int(_get(offsets, n + 1)[-1])
        counts = {"starts": n * DIM, "goals": n * DIM, "packed_goals": total * DIM, "points": total * DIM,
                  "goal_offsets": n + 1, "offsets": n + 1, "skips": n, "index": n, "samples": n * self.ns * DIM,
                  "targets": n * 16, "vel": DIM, "acc": DIM}
        rec = {"symbol": name, "settings": [type(cs).__name__, bytes(cs).hex()]}
        for kind, v in a.items():
            if kind in ("robot", "n", "n_constraints"):
                rec[kind] = int(v)
            elif kind == "envs":
                rec[kind] = None if v is None else {"array length": len(v), "handles": list(v)[:n]}
            elif kind == "constraints":  # (the wrapper hands the ctypes array itself)
                rec[kind] = None if v is None else {"array length": len(v), "bytes": bytes(v).hex()}
            elif kind == "constraint_settings":
                rec[kind] = None if v is None else [type(v._obj).__name__, bytes(v._obj).hex()]
            elif kind == "roadmaps":
                rec[kind] = v.value
            elif kind == "handle":
                v._obj.value = PLANS_HANDLE
            elif kind != "settings":
                rec[kind] = None if v is None else _plain(_get(v, counts[kind]))
        return rec

    # -- readouts: fixed patterns ------------------------------------------------------------------------------
    def _vmv_plans_summary(self, plans, status, iterations, sizes, lengths, rounds, questions):
        assert plans.value == PLANS_HANDLE
        k = np.arange(self.n)
        self.lengths = np.array([2, 0, 3])[k % 3]
        _put(status, k % 5)
        _put(iterations, 100 + k)
        _put(sizes, np.stack([10 + k, 20 + k], axis=1))
        _put(lengths, self.lengths)
        rounds._obj.value, questions._obj.value = 11, 22

    def _vmv_plans_paths(self, plans, paths, size):
        assert size == int(self.lengths.sum()) * DIM
        _put(paths, np.arange(size) * 0.5)

    def _vmv_plans_goal_indices(self, plans, indices):
        _put(indices, np.array([0, 0xFFFFFFFF, 1], np.uint32)[np.arange(self.n) % 3])

    def _vmv_plans_costs(self, plans, first, costs, searches, improvements):
        k = np.arange(self.n)
        _put(first, 2.5 + k)
        _put(costs, 1.25 + k)
        _put(searches, 3 + k)
        _put(improvements, k)

    def _vmv_plans_roadmap_summary(self, plans, vertices, candidates, edges, costs):
        self.entry["roadmap_summary pointers None"] = [vertices is None, candidates is None, edges is None, costs is None]
        k = np.arange(self.n)
        _put(candidates, np.array([4, 0, 2])[k % 3])
        _put(costs, 0.5 + 1.5 * k)

    def _vmv_plans_roadmap_vertices(self, plans, p, vertex):
        _put(vertex, (np.arange(self.ns + 2) + p) % 3 == 0)

    def _vmv_plans_roadmap_edges(self, plans, p, pairs, flags, capacity, got):
        _put(pairs, np.arange(2 * capacity) + p)
        _put(flags, np.arange(capacity) % 2)
        got._obj.value = max(capacity - 1, 0)  # one fewer than asked for: the wrapper cuts to what it got

    def _vmv_plans_query_summary(self, plans, costs, asked):
        k = np.arange(self.n)
        _put(costs, 0.75 + k)
        _put(asked, 7 + 2 * k)

    def _vmv_plans_fcit_summary(self, plans, costs, known):
        k = np.arange(self.n)
        _put(costs, 0.25 + k)
        _put(known, 9 + k)

    def _vmv_paths_summary(self, out, status, iterations, lengths, questions, rounds, total):
        assert out.value == PLANS_HANDLE
        k = np.arange(self.n)
        self.lengths = np.array([2, 0, 3])[k % 3]
        _put(status, k % 2)
        _put(iterations, 1 + k)
        _put(lengths, self.lengths)
        _put(questions, 5 + k)
        rounds._obj.value, total._obj.value = 11, 22

    def _vmv_paths_points(self, out, points, size):
        assert size == int(self.lengths.sum()) * DIM
        _put(points, np.arange(size) * 0.5)

    def _vmv_optimized_summary(self, out, status, iterations, best, cost_first, cost, clr_first, clr, calls, validations):
        assert out.value == PLANS_HANDLE
        k = np.arange(self.n)
        _put(status, k % 3)
        _put(iterations, 30 + k)
        _put(best, 20 + k)
        _put(cost_first, 8.5 + k)
        _put(cost, 4.5 + k)
        _put(clr_first, np.stack([0.125 + k, -0.25 - k], axis=1))
        _put(clr, np.stack([0.375 + k, 0.0625 + k], axis=1))
        calls._obj.value, validations._obj.value = 33, 44

    def _vmv_optimized_points(self, out, points, size):
        _put(points, np.arange(size) * 0.25)

    def _vmv_plans_band_refused(self, plans, refused):
        assert plans.value == PLANS_HANDLE
        _put(refused, 40 + np.arange(self.n))

    def _vmv_paths_band_refused(self, out, refused):
        assert out.value == PLANS_HANDLE
        _put(refused, 50 + np.arange(self.n))

    def _vmv_optimized_held(self, out, held):
        assert out.value == PLANS_HANDLE
        _put(held, 60 + np.arange(self.n))

    def _vmv_cartesian_summary(self, out, status, segments, achieved, evaluations, calls, questions):
        assert out.value == PLANS_HANDLE
        k = np.arange(self.n)
        self.lengths = np.array([2, 0, 3])[k % 3] + 1  # achieved + 1 waypoints
        _put(status, k % 7)
        _put(segments, 4 * (k % 2))
        _put(achieved, self.lengths - 1)
        _put(evaluations, 70 + k)
        calls._obj.value, questions._obj.value = 55, 66

    def _vmv_cartesian_points(self, out, points, size):
        assert size == int(self.lengths.sum()) * DIM
        _put(points, np.arange(size) * 0.75)

    def _vmv_retime_summary(self, out, status, intervals, samples, duration, first_invalid, calls, questions):
        assert out.value == PLANS_HANDLE
        k = np.arange(self.n)
        self.lengths = np.array([2, 0, 3])[k % 3]
        _put(status, k % 6)
        _put(intervals, 80 + k)
        _put(samples, self.lengths)
        _put(duration, 1.5 + k)
        _put(first_invalid, np.array([0xFFFFFFFF, 0, 1], np.uint32)[k % 3])
        calls._obj.value, questions._obj.value = 77, 88

    def _vmv_retime_levels(self, out, levels, rounds, repaired, stops):
        k = np.arange(self.n)
        _put(levels, np.arange(self.total) % 5)
        _put(rounds, 1 + k)
        _put(repaired, 2 * k)
        _put(stops, k)

    def _vmv_retime_samples(self, out, times, positions, velocities, accelerations, total):
        assert total == int(self.lengths.sum())
        _put(times, np.arange(total) * 0.01)
        for scale, rows in ((0.5, positions), (0.25, velocities), (0.125, accelerations)):
            _put(rows, np.arange(total * DIM) * scale)


# ---------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------
def _base(vamp, wrapper, n):
    """the good arguments of `wrapper` for n problems or paths"""
    from vamp_mvt_amd import planning as P

    starts = (np.arange(n * DIM).reshape(n, DIM) * 0.01).astype(np.float32)
    a = dict(vamp=vamp, starts=starts, goals=starts + np.float32(1), environments=[vamp.Environment() for _ in range(n)],
             skips=None, samples=None)
    if wrapper in ("rrtc_multi_raw", "rrtc_multi_goals_raw"):
        a["settings"] = P.RRTCMultiSettings(range=0.75, tree_ratio=1.5, max_iterations=1000, max_samples=64, check_every=3)
    if wrapper == "rrtc_multi_goals_raw":
        a["goal_counts"] = np.array([GOAL_COUNTS[p % 3] for p in range(n)], np.int64)
        total = int(a["goal_counts"].sum())
        a["goals"] = (np.arange(total * DIM).reshape(total, DIM) * 0.02).astype(np.float32)
    elif wrapper == "aorrtc_multi_raw":
        a["settings"] = P.AORRTCMultiSettings(range=0.75, tree_ratio=1.5, max_iterations=1000, max_internal_iterations=200,
                                              max_samples=64, max_cost_bound_resamples=8, max_searches=5,
                                              simplify=P.SimplifyMultiSettings(), check_every=3)
    elif wrapper == "prm_multi_raw":
        a["settings"] = P.PRMMultiSettings(n_samples=64, k=4, radius=2.5)
    elif wrapper == "fcit_multi_raw":
        a["settings"] = P.FCITMultiSettings(n_samples=64, max_iterations=50, questions_per_round=2, check_every=1)
    elif wrapper == "roadmaps_build_raw":
        a["settings"] = P.RoadmapsSettings(n_samples=64, k=4, radius=2.5)
    elif wrapper == "roadmaps_query_raw":
        a.update(handle=ctypes.c_void_p(ROADMAPS_HANDLE), n_roadmaps=2, index=None,
                 settings=P.RoadmapQuerySettings(k_connect=3, radius=1.5), environments=[vamp.Environment() for _ in range(2)])
    elif wrapper in ("simplify_multi_raw", "optimize_multi_raw"):
        a["paths"] = [(np.arange(m * DIM).reshape(m, DIM) * 0.125).astype(np.float32) for m in (4, 0, 2)[:n]]
        a["resolution"] = None
        a["settings"] = P.SimplifyMultiSettings(questions_per_round=4) if wrapper == "simplify_multi_raw" else \
            P.OptimizeMultiSettings()
    elif wrapper == "rrtc_multi_constrained_raw":
        a.update(_base(vamp, "rrtc_multi_goals_raw", n), constraints=_constraint(vamp), constraint_settings=None, max_stretch=2.0)
    elif wrapper in ("simplify_multi_constrained_raw", "optimize_multi_constrained_raw"):
        a.update(_base(vamp, wrapper.replace("_constrained", ""), n), constraints=_constraint(vamp), constraint_settings=None)
    elif wrapper == "cartesian_multi_raw":
        a["targets"] = (np.eye(4, dtype=np.float32)[None] + (np.arange(n * 16).reshape(n, 4, 4) * 0.001).astype(np.float32))
        a["settings"] = P.CartesianSettings()
    elif wrapper in ("retime_multi_raw", "retime_multi_constrained_raw"):
        a["paths"] = [(np.arange(m * DIM).reshape(m, DIM) * 0.125).astype(np.float32) for m in (4, 0, 2)[:n]]
        a["vel_limits"], a["acc_limits"] = np.full(DIM, 1.5, np.float32), np.arange(1, DIM + 1) * 0.5
        a["settings"] = P.RetimeSettings() if wrapper == "retime_multi_raw" else P.RetimeConstrainedSettings()
        a.update(constraints=None, constraint_settings=None)
    return a


def _constraint(vamp, k=0):
    return vamp.EEConstraint.box([-1.0, -1.0, 0.25 * k], [1.0, 1.0, 2.0], frame=np.eye(4))


def _replaced(obj, path, value):
    return replace(obj, **{path[0]: value if len(path) == 1 else _replaced(getattr(obj, path[0]), path[1:], value)})


def _args(vamp, wrapper, n, changes):
    """`_base` with `changes` applied: {argument or "settings.<field>": the value, or a function of the good arguments}"""
    a = _base(vamp, wrapper, n)
    good = dict(a)
    for key, value in changes.items():
        if callable(value):
            value = value(good)
        if key.startswith("settings."):
            a["settings"] = _replaced(a["settings"], key.split(".")[1:], value)
        else:
            a[key] = value
    return a


def _raw(vamp, w, a):
    f = getattr(vamp.panda, w)
    if w in ("rrtc_multi_raw", "aorrtc_multi_raw"):
        return f(a["starts"], a["goals"], a["environments"], a["settings"], a["skips"])
    if w == "rrtc_multi_goals_raw":
        return f(a["starts"], a["goals"], a["goal_counts"], a["environments"], a["settings"], a["skips"])
    if w in ("prm_multi_raw", "fcit_multi_raw"):
        return f(a["starts"], a["goals"], a["environments"], a["settings"], a["skips"], a["samples"])
    if w == "roadmaps_build_raw":
        handle, envs = f(a["environments"], a["settings"], a["skips"], a["samples"])
        return {"handle": handle.value, "the environments given": [e is g for e, g in zip(envs, a["environments"])]}
    if w == "roadmaps_query_raw":
        return f(a["handle"], a["n_roadmaps"], a["starts"], a["goals"], a["index"], a["settings"])
    if w == "rrtc_multi_constrained_raw":
        return f(a["starts"], a["goals"], a["goal_counts"], a["environments"], a["constraints"], a["settings"], a["constraint_settings"],
                 a["max_stretch"], a["skips"])
    if w in ("simplify_multi_constrained_raw", "optimize_multi_constrained_raw"):
        return f(a["paths"], a["environments"], a["constraints"], a["settings"], a["constraint_settings"])
    if w == "cartesian_multi_raw":
        return f(a["starts"], a["targets"], a["environments"], a["settings"])
    if w == "retime_multi_raw":
        return f(a["paths"], a["vel_limits"], a["acc_limits"], a["environments"], a["settings"])
    if w == "retime_multi_constrained_raw":
        return f(a["paths"], a["vel_limits"], a["acc_limits"], a["environments"], a["constraints"], a["settings"], a["constraint_settings"])
    return f(a["paths"], a["environments"], a["settings"])


def _plan(vamp, w, a):
    """the planning.* function above wrapper `w`"""
    from vamp_mvt_amd import planning as P

    r = vamp.panda
    if w == "rrtc_multi_raw":
        return P.rrtc_multi(r, a["starts"], a["goals"], a["environments"], a["settings"], a["skips"])
    if w == "rrtc_multi_goals_raw":
        sets = a.get("goal_sets")
        if sets is None:
            counts = np.ones(len(a["goals"]), np.int64) if a["goal_counts"] is None else a["goal_counts"]
            sets = np.split(a["goals"], np.cumsum(counts)[:-1]) if len(counts) else []
        return P.rrtc_multi_goals(r, a["starts"], sets, a["environments"], a["settings"], a["skips"])
    if w == "aorrtc_multi_raw":
        return P.aorrtc_multi(r, a["starts"], a["goals"], a["environments"], a["settings"], a["skips"])
    if w == "prm_multi_raw":
        return P.prm_multi(r, a["starts"], a["goals"], a["environments"], a["settings"], a["skips"], a["samples"])
    if w == "fcit_multi_raw":
        return P.fcit_multi(r, a["starts"], a["goals"], a["environments"], a["settings"], a["skips"], a["samples"])
    if w == "roadmaps_build_raw":
        roadmaps = P.build_roadmaps(r, a["environments"], a["settings"], a["skips"], a["samples"])
        try:
            return {"len": len(roadmaps), "settings": roadmaps.settings, "handle": roadmaps._handle.value}
        finally:
            roadmaps.close()
    if w == "roadmaps_query_raw":
        roadmaps = P.DeviceRoadmaps(r, a["handle"], a["environments"][:a["n_roadmaps"]], P.RoadmapsSettings())
        try:
            return roadmaps.query(a["starts"], a["goals"], a["index"], a["settings"])
        finally:
            roadmaps.close()
    if w == "simplify_multi_raw":
        return P.simplify_multi(r, a["paths"], a["environments"], a["settings"])
    if w == "rrtc_multi_constrained_raw":
        sets = np.split(a["goals"], np.cumsum(a["goal_counts"])[:-1]) if len(a["goal_counts"]) else []
        return P.rrtc_multi_constrained(r, a["starts"], sets, a["environments"], a["constraints"], a["settings"], a["constraint_settings"],
                                        a["skips"], a["max_stretch"])
    if w == "simplify_multi_constrained_raw":
        return P.simplify_multi_constrained(r, a["paths"], a["environments"], a["constraints"], a["settings"], a["constraint_settings"])
    if w == "optimize_multi_constrained_raw":
        return P.optimize_multi_constrained(r, a["paths"], a["environments"], a["constraints"], a["settings"], a["constraint_settings"],
                                            a["resolution"])
    if w == "cartesian_multi_raw":
        return P.cartesian_multi(r, a["starts"], a["targets"], a["environments"], a["settings"])
    if w == "retime_multi_raw":
        return P.retime_multi(r, a["paths"], a["vel_limits"], a["acc_limits"], a["environments"], a["settings"])
    if w == "retime_multi_constrained_raw":
        return P.retime_multi_constrained(r, a["paths"], a["vel_limits"], a["acc_limits"], a["environments"], a["constraints"],
                                          a["settings"], a["constraint_settings"])
    return P.optimize_multi(r, a["paths"], a["environments"], a["settings"], a["resolution"])


def _plain(x):
    """x as JSON: arrays with dtype and shape (a digest beyond 64 elements), dataclasses field by field"""
    if isinstance(x, np.ndarray):
        body = {"sha256": hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()} if x.size > 64 else \
            {"values": x.reshape(-1).tolist()}
        return {"dtype": str(x.dtype), "shape": list(x.shape), **body}
    if isinstance(x, np.generic):
        return {"numpy scalar": str(x.dtype), "value": x.item()}
    if is_dataclass(x):
        return {"class": type(x).__name__, **{f.name: _plain(getattr(x, f.name)) for f in fields(x)}}
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return {"tuple": [_plain(v) for v in x]}
    if isinstance(x, list):
        return [_plain(v) for v in x]
    assert x is None or isinstance(x, (bool, int, float, str)), type(x)
    return x


# ---------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------
def _ints(field, lo, hi):
    """one below, at and one above both ends of the accepted range lo .. hi"""
    return [(f"{field}={v}", {f"settings.{field}": v}) for v in (lo - 1, lo, hi, hi + 1)]


def _floats(field, *values):
    return [(f"{field}={v!r}", {f"settings.{field}": v}) for v in values]


NAN, INF, U32 = float("nan"), float("inf"), 2 ** 32 - 1
_ENVIRONMENTS = [
    ("two environments", {"environments": lambda a: a["environments"][:2]}),
    ("four environments", {"environments": lambda a: a["environments"] + [a["vamp"].Environment()]}),
    ("a string among the environments", {"environments": lambda a: a["environments"][:2] + ["env"]}),
]
_BAD_ENVIRONMENT = {"environments": lambda a: a["environments"][:2] + ["env"]}
_BAD_COUNT = {"environments": lambda a: a["environments"][:2]}
_BAD_SHAPE = {"starts": lambda a: a["starts"][:, :6]}
_BAD_SKIPS = {"skips": [-1, 0, 0]}
_BAD_SAMPLES = {"samples": np.zeros((64, 6), np.float32)}
_ENDPOINTS = [
    ("starts of rank 1", {"starts": lambda a: a["starts"][0]}),
    ("starts of rank 3", {"starts": lambda a: a["starts"][None]}),
    ("starts and goals of dim 6", {"starts": lambda a: a["starts"][:, :6], "goals": lambda a: a["goals"][:, :6]}),
    ("goals of dim 6", {"goals": lambda a: a["goals"][:, :6]}),
    ("two goals for three starts", {"goals": lambda a: a["goals"][:2]}),
    ("goals of rank 1", {"goals": lambda a: a["goals"][0]}),
]
_SKIPS = [
    ("two skips", {"skips": [0, 1]}),
    ("skips of rank 2", {"skips": [[0, 1, 2]]}),
    ("a negative skip", {"skips": [-1, 0, 0]}),
    ("float skips", {"skips": [0.0, 1.0, 2.0]}),
    ("the largest uint64 skip", {"skips": np.array([2 ** 64 - 1, 0, 0], np.uint64)}),
]
_HALTON = [  # n_samples = 64
    ("a skip at the Halton limit", {"skips": [1000000 - 64, 0, 0]}),
    ("a skip beyond the Halton limit", {"skips": [0, 1000000 - 63, 0]}),
    ("a skip beyond the Halton limit, samples given", {"skips": [0, 1000000 - 63, 0], "samples": np.zeros((64, DIM), np.float32)}),
]
_SAMPLES = [
    ("samples of dim 6", {"samples": np.zeros((64, 6), np.float32)}),
    ("samples for two problems", {"samples": np.zeros((2, 64, DIM), np.float32)}),
    ("65 samples", {"samples": np.zeros((65, DIM), np.float32)}),
    ("samples of rank 1", {"samples": np.zeros(64 * DIM, np.float32)}),
]
_RRTC_SETTINGS = (_floats("range", 0.0, -1.0, NAN, INF, 1e-6) + _floats("tree_ratio", NAN) + _ints("max_iterations", 0, U32) +
                  _ints("max_samples", 2, U32) + _ints("check_every", 0, U32))
_ROADMAP_SAMPLING = ([(f"n_samples={v}", {"settings.n_samples": v}) for v in (0, 63, 64, 65, 128, 8128, 8192)] + _ints("k", 1, 16) +
                     _floats("radius", 0.0, -1.0, NAN, INF, 1e-6))
_PATH_CASES = [
    ("a path of dim 6", {"paths": lambda a: [a["paths"][0], a["paths"][1], a["paths"][2][:, :6]]}),
    ("a path of rank 1", {"paths": lambda a: [a["paths"][0][0], a["paths"][1], a["paths"][2]]}),
    ("two environments", _BAD_COUNT),
    ("four environments", _ENVIRONMENTS[1][1]),
    ("a string among the environments", _BAD_ENVIRONMENT),
    ("a string among the environments, a path of dim 6", {**_BAD_ENVIRONMENT, "paths": lambda a: [p[:, :6] for p in a["paths"]]}),
    ("a path of dim 6, two environments", {**_BAD_COUNT, "paths": lambda a: [p[:, :6] for p in a["paths"]]}),
]

REFUSALS = {
    "rrtc_multi_raw": _ENVIRONMENTS + _ENDPOINTS + _SKIPS + _RRTC_SETTINGS + [
        ("a string among the environments, starts of dim 6", {**_BAD_ENVIRONMENT, **_BAD_SHAPE}),
        ("starts of dim 6, two environments", {**_BAD_SHAPE, **_BAD_COUNT}),
        ("two environments, a negative skip", {**_BAD_COUNT, **_BAD_SKIPS}),
        ("a negative skip, range=0", {**_BAD_SKIPS, "settings.range": 0.0}),
        ("range=0, max_samples=1", {"settings.range": 0.0, "settings.max_samples": 1}),
    ],
    "rrtc_multi_goals_raw": _ENVIRONMENTS + _SKIPS + _RRTC_SETTINGS + [
        ("starts of rank 1", {"starts": lambda a: a["starts"][0]}),
        ("starts of dim 6", _BAD_SHAPE),
        ("goals of dim 6", {"goals": lambda a: a["goals"][:, :6]}),
        ("goals of rank 1", {"goals": lambda a: a["goals"][0]}),
        ("goal_counts=None, four goals", {"goal_counts": None}),
        ("two goal counts", {"goal_counts": [2, 2]}),
        ("goal counts of rank 2", {"goal_counts": [[1, 2, 1]]}),
        ("float goal counts", {"goal_counts": [1.0, 2.0, 1.0]}),
        ("a goal count of 0", {"goal_counts": [2, 0, 2]}),
        ("goal counts that sum to 5", {"goal_counts": [1, 2, 2]}),
        ("goal counts that sum to 3", {"goal_counts": [1, 1, 1]}),
        ("a set of 2 goals, max_samples=2", {"settings.max_samples": 2}),
        ("a set of 2 goals, max_samples=3", {"settings.max_samples": 3}),
        ("dynamic_domain off, radius=nan", {"settings.radius": NAN}),
    ] + [(f"dynamic_domain, {name}", {"settings.dynamic_domain": True, **change}) for name, change in
         _floats("radius", 0.0, NAN, INF, 1e-6) + _floats("min_radius", 0.0, NAN, INF, 1e-6) +
         _floats("alpha", -1e-6, 0.0, 0.999, 1.0, NAN)] + [
        ("a string among the environments, starts of dim 6", {**_BAD_ENVIRONMENT, **_BAD_SHAPE}),
        ("starts of dim 6, a goal count of 0", {**_BAD_SHAPE, "goal_counts": [2, 0, 2]}),
        ("a goal count of 0, two environments", {"goal_counts": [2, 0, 2], **_BAD_COUNT}),
        ("two environments, a negative skip", {**_BAD_COUNT, **_BAD_SKIPS}),
        ("a negative skip, range=0", {**_BAD_SKIPS, "settings.range": 0.0}),
        ("max_iterations=-1, a set of 2 goals with max_samples=2", {"settings.max_iterations": -1, "settings.max_samples": 2}),
        ("a set of 2 goals with max_samples=2, dynamic_domain with radius=0",
         {"settings.max_samples": 2, "settings.dynamic_domain": True, "settings.radius": 0.0}),
        ("dynamic_domain, radius=0 and alpha=1", {"settings.dynamic_domain": True, "settings.radius": 0.0, "settings.alpha": 1.0}),
    ],
    "aorrtc_multi_raw": _ENVIRONMENTS + _ENDPOINTS + _SKIPS + _RRTC_SETTINGS + _ints("max_searches", 0, U32) +
    _ints("max_internal_iterations", 1, U32) + _ints("max_cost_bound_resamples", 0, 64) + [
        ("simplify with REDUCE", {"settings.simplify.operations": ["REDUCE"]}),
        ("simplify with max_steps=-1", {"settings.simplify.max_steps": -1}),
        ("a string among the environments, starts of dim 6", {**_BAD_ENVIRONMENT, **_BAD_SHAPE}),
        ("starts of dim 6, two environments", {**_BAD_SHAPE, **_BAD_COUNT}),
        ("two environments, a negative skip", {**_BAD_COUNT, **_BAD_SKIPS}),
        ("a negative skip, range=0", {**_BAD_SKIPS, "settings.range": 0.0}),
        ("range=0, max_searches=-1", {"settings.range": 0.0, "settings.max_searches": -1}),
        ("max_searches=-1, max_internal_iterations=0", {"settings.max_searches": -1, "settings.max_internal_iterations": 0}),
        ("max_internal_iterations=0, max_cost_bound_resamples=65",
         {"settings.max_internal_iterations": 0, "settings.max_cost_bound_resamples": 65}),
        ("max_cost_bound_resamples=65, simplify with REDUCE",
         {"settings.max_cost_bound_resamples": 65, "settings.simplify.operations": ["REDUCE"]}),
    ],
    "prm_multi_raw": _ENVIRONMENTS + _ENDPOINTS + _SKIPS + _HALTON + _SAMPLES + _ROADMAP_SAMPLING + [
        ("a string among the environments, starts of dim 6", {**_BAD_ENVIRONMENT, **_BAD_SHAPE}),
        ("starts of dim 6, two environments", {**_BAD_SHAPE, **_BAD_COUNT}),
        ("two environments, k=0", {**_BAD_COUNT, "settings.k": 0}),
        ("n_samples=65, k=0", {"settings.n_samples": 65, "settings.k": 0}),
        ("k=0, radius=0", {"settings.k": 0, "settings.radius": 0.0}),
        ("radius=0, samples of dim 6", {"settings.radius": 0.0, **_BAD_SAMPLES}),
        ("samples of dim 6, a negative skip", {**_BAD_SAMPLES, **_BAD_SKIPS}),
    ],
    "fcit_multi_raw": _ENVIRONMENTS + _ENDPOINTS + _SKIPS + _HALTON + _SAMPLES +
    [(f"n_samples={v}", {"settings.n_samples": v}) for v in (0, 63, 64, 65, 128, 2048, 2112)] +
    _ints("questions_per_round", 1, 32) + _ints("max_iterations", 1, U32) + _ints("check_every", 0, U32) + [
        ("a string among the environments, starts of dim 6", {**_BAD_ENVIRONMENT, **_BAD_SHAPE}),
        ("starts of dim 6, two environments", {**_BAD_SHAPE, **_BAD_COUNT}),
        ("two environments, n_samples=65", {**_BAD_COUNT, "settings.n_samples": 65}),
        ("n_samples=65, questions_per_round=0", {"settings.n_samples": 65, "settings.questions_per_round": 0}),
        ("questions_per_round=0, max_iterations=0", {"settings.questions_per_round": 0, "settings.max_iterations": 0}),
        ("max_iterations=0, samples of dim 6", {"settings.max_iterations": 0, **_BAD_SAMPLES}),
        ("samples of dim 6, a negative skip", {**_BAD_SAMPLES, **_BAD_SKIPS}),
    ],
    "roadmaps_build_raw": [_ENVIRONMENTS[2]] + _SKIPS + _HALTON + _SAMPLES + _ROADMAP_SAMPLING + [
        ("a string among the environments, k=0", {**_BAD_ENVIRONMENT, "settings.k": 0}),
        ("n_samples=65, k=0", {"settings.n_samples": 65, "settings.k": 0}),
        ("k=0, radius=0", {"settings.k": 0, "settings.radius": 0.0}),
        ("radius=0, samples of dim 6", {"settings.radius": 0.0, **_BAD_SAMPLES}),
        ("samples of dim 6, a negative skip", {**_BAD_SAMPLES, **_BAD_SKIPS}),
    ],
    "roadmaps_query_raw": _ENDPOINTS + _ints("k_connect", 1, 32) + _floats("radius", 0.0, -1.0, NAN, INF, 1e-6) + [
        ("two indices", {"index": [0, 1]}),
        ("indices of rank 2", {"index": [[0, 1, 0]]}),
        ("a negative index", {"index": [0, -1, 0]}),
        ("float indices", {"index": [0.0, 1.0, 0.0]}),
        ("the last roadmap's index", {"index": [0, 1, 1]}),
        ("an index past the last roadmap", {"index": [0, 2, 0]}),
        ("no roadmaps, no index", {"n_roadmaps": 0}),
        ("no roadmaps, an index", {"n_roadmaps": 0, "index": [0, 0, 0]}),
        ("starts of dim 6, k_connect=0", {**_BAD_SHAPE, "settings.k_connect": 0}),
        ("k_connect=0, radius=0", {"settings.k_connect": 0, "settings.radius": 0.0}),
        ("radius=0, an index past the last roadmap", {"settings.radius": 0.0, "index": [0, 2, 0]}),
        ("radius=0, no roadmaps", {"settings.radius": 0.0, "n_roadmaps": 0}),
    ],
    "simplify_multi_raw": _PATH_CASES + _ints("max_iterations", 0, U32) + _ints("max_steps", 0, U32) + _ints("check_every", 0, U32) +
    _ints("max_waypoints", 0, 2 ** 24) + [(f"questions_per_round={v}", {"settings.questions_per_round": v})
                                         for v in (-1, 0, 1, 2, 3, 64, 65, 128)] + _floats("min_change", NAN) + [
        ("an unknown operation", {"settings.operations": ["SHORTCUT", "SMOOTH"]}),
        ("REDUCE", {"settings.operations": ["SHORTCUT", "REDUCE"]}),
        ("PERTURB", {"settings.operations": ["perturb"]}),
        ("8 operations", {"settings.operations": ["SHORTCUT", "BSPLINE"] * 4}),
        ("9 operations", {"settings.operations": ["SHORTCUT"] * 9}),
        ("no operations", {"settings.operations": []}),
        ("interpolate=1", {"settings.interpolate": 1}),
        ("a path of 4 waypoints, max_waypoints=3", {"settings.max_waypoints": 3}),
        ("a path of 4 waypoints, max_waypoints=4", {"settings.max_waypoints": 4}),
        ("a path of 2,048 waypoints, max_waypoints=0", {"settings.max_waypoints": 0, "paths": lambda a: [
            np.zeros((2048, DIM), np.float32)] + a["paths"][1:]}),
        ("a path of 2,049 waypoints, max_waypoints=0", {"settings.max_waypoints": 0, "paths": lambda a: [
            np.zeros((2049, DIM), np.float32)] + a["paths"][1:]}),
        ("two environments, REDUCE", {**_BAD_COUNT, "settings.operations": ["REDUCE"]}),
        ("REDUCE, an unknown operation, 9 operations", {"settings.operations": ["REDUCE"] + ["SMOOTH"] * 8}),
        ("9 operations, interpolate=1", {"settings.operations": ["SHORTCUT"] * 9, "settings.interpolate": 1}),
        ("interpolate=1, max_steps=-1", {"settings.interpolate": 1, "settings.max_steps": -1}),
        ("max_steps=-1, questions_per_round=3", {"settings.max_steps": -1, "settings.questions_per_round": 3}),
        ("questions_per_round=3, max_waypoints=3", {"settings.questions_per_round": 3, "settings.max_waypoints": 3}),
    ],
    "optimize_multi_raw": _PATH_CASES + _ints("max_iterations", 1, U32) + _ints("validate_every", 1, U32) +
    _ints("max_waypoints", 1, 1024) + [case for k in ("step", "max_step", "env_margin", "self_margin")
                                       for case in _floats(k, 0.0, -1.0, NAN, INF, 1e-6)] +
    [case for k in ("smooth_weight", "env_weight", "self_weight") for case in _floats(k, -1e-6, 0.0, NAN, INF)] +
    _floats("min_change", NAN, -1.0, INF) + [
        ("a path of 4 waypoints, max_waypoints=3", {"settings.max_waypoints": 3}),
        ("a path of 4 waypoints, max_waypoints=4", {"settings.max_waypoints": 4}),
        ("two environments, max_iterations=0", {**_BAD_COUNT, "settings.max_iterations": 0}),
        ("max_iterations=0, max_waypoints=0", {"settings.max_iterations": 0, "settings.max_waypoints": 0}),
        ("a path of 4 waypoints with max_waypoints=3, step=0", {"settings.max_waypoints": 3, "settings.step": 0.0}),
        ("step=0, env_margin=0, smooth_weight=-1", {"settings.step": 0.0, "settings.env_margin": 0.0, "settings.smooth_weight": -1.0}),
        ("self_weight=-1, min_change=nan", {"settings.self_weight": -1.0, "settings.min_change": NAN}),
    ],
}

_NO_ENVIRONMENTS = {"environments": None}
_TWO_CONSTRAINTS = {"constraints": lambda a: [_constraint(a["vamp"], k) for k in range(2)]}
_CONSTRAINTS = [
    ("a string as the constraint", {"constraints": "upright"}),
    ("a string among the constraints", {"constraints": lambda a: [_constraint(a["vamp"]), "upright", _constraint(a["vamp"])]}),
    ("no constraints", {"constraints": []}),
    ("two constraints", _TWO_CONSTRAINTS),
    ("four constraints", {"constraints": lambda a: [_constraint(a["vamp"], k) for k in range(4)]}),
    ("a string as the constraint settings", {"constraint_settings": "fine"}),
    ("a string among the environments, two constraints", {**_BAD_ENVIRONMENT, **_TWO_CONSTRAINTS}),
    ("two environments, two constraints", {**_BAD_COUNT, **_TWO_CONSTRAINTS}),
    ("two constraints, a string as the constraint settings", {**_TWO_CONSTRAINTS, "constraint_settings": "fine"}),
]
_LIMITS = [
    ("vel_limits of 6", {"vel_limits": np.ones(6)}),
    ("vel_limits of rank 2", {"vel_limits": np.ones((1, DIM))}),
    ("a vel_limit of 0", {"vel_limits": [1, 1, 1, 0, 1, 1, 1]}),
    ("a vel_limit of inf", {"vel_limits": [1, 1, 1, INF, 1, 1, 1]}),
    ("acc_limits of 8", {"acc_limits": np.ones(8)}),
    ("an acc_limit of nan", {"acc_limits": [1, 1, 1, 1, 1, 1, NAN]}),
    ("a negative acc_limit", {"acc_limits": [-1, 1, 1, 1, 1, 1, 1]}),
]
_RETIME_SETTINGS = (_floats("blend", NAN, INF, 0.0, -1.0) + _floats("grid_step", NAN, 0.0, 1e-7, 1e-6) + _floats("dt", INF, 0.0, 1e-7, 1e-6) +
                    _ints("max_grid", 0, 4096) + _ints("max_samples", 0, U32))
_RETIME = _PATH_CASES + _LIMITS + _RETIME_SETTINGS + [
    ("no environments, a path of dim 6", {**_NO_ENVIRONMENTS, **_PATH_CASES[0][1]}),
    ("no environments, vel_limits of 6", {**_NO_ENVIRONMENTS, "vel_limits": np.ones(6)}),
    ("two environments, vel_limits of 6", {**_BAD_COUNT, "vel_limits": np.ones(6)}),
    ("vel_limits of 6, a negative acc_limit", {"vel_limits": np.ones(6), "acc_limits": [-1, 1, 1, 1, 1, 1, 1]}),
    ("a negative acc_limit, blend=nan", {"acc_limits": [-1, 1, 1, 1, 1, 1, 1], "settings.blend": NAN}),
    ("blend=nan, grid_step=1e-7", {"settings.blend": NAN, "settings.grid_step": 1e-7}),
    ("dt=1e-7, max_grid=4097", {"settings.dt": 1e-7, "settings.max_grid": 4097}),
    ("max_grid=4097, max_samples=-1", {"settings.max_grid": 4097, "settings.max_samples": -1}),
]
REFUSALS.update({
    "rrtc_multi_constrained_raw": _ENVIRONMENTS + _SKIPS + _CONSTRAINTS + [
        ("starts of dim 6", _BAD_SHAPE),
        ("a goal count of 0", {"goal_counts": [2, 0, 2]}),
        ("range=0", {"settings.range": 0.0}),
        ("a set of 2 goals, max_samples=2", {"settings.max_samples": 2}),
        ("dynamic_domain, radius=0", {"settings.dynamic_domain": True, "settings.radius": 0.0}),
    ] + [(f"max_stretch={v!r}", {"max_stretch": v}) for v in (NAN, INF, -1.0, -0.0, 0.0, 1e-6)] + [
        ("a negative skip, two constraints", {**_BAD_SKIPS, **_TWO_CONSTRAINTS}),
        ("range=0, two constraints", {"settings.range": 0.0, **_TWO_CONSTRAINTS}),
        ("dynamic_domain with radius=0, two constraints", {"settings.dynamic_domain": True, "settings.radius": 0.0, **_TWO_CONSTRAINTS}),
        ("two constraints, max_stretch=nan", {**_TWO_CONSTRAINTS, "max_stretch": NAN}),
        ("max_stretch=nan, a string as the constraint settings", {"max_stretch": NAN, "constraint_settings": "fine"}),
    ],
    "simplify_multi_constrained_raw": _PATH_CASES + _CONSTRAINTS + [
        ("REDUCE", {"settings.operations": ["SHORTCUT", "REDUCE"]}),
        ("questions_per_round=3", {"settings.questions_per_round": 3}),
        ("a path of 4 waypoints, max_waypoints=3", {"settings.max_waypoints": 3}),
        ("a path of dim 6, two constraints", {**_PATH_CASES[0][1], **_TWO_CONSTRAINTS}),
        ("REDUCE, two constraints", {"settings.operations": ["REDUCE"], **_TWO_CONSTRAINTS}),
    ],
    "optimize_multi_constrained_raw": _PATH_CASES + _CONSTRAINTS + [
        ("step=0", {"settings.step": 0.0}),
        ("max_iterations=0", {"settings.max_iterations": 0}),
        ("a path of 4 waypoints, max_waypoints=3", {"settings.max_waypoints": 3}),
        ("a path of dim 6, two constraints", {**_PATH_CASES[0][1], **_TWO_CONSTRAINTS}),
        ("step=0, two constraints", {"settings.step": 0.0, **_TWO_CONSTRAINTS}),
    ],
    "cartesian_multi_raw": _ENVIRONMENTS + [
        ("starts of rank 1", {"starts": lambda a: a["starts"][0]}),
        ("starts of dim 6", _BAD_SHAPE),
        ("two targets", {"targets": lambda a: a["targets"][:2]}),
        ("targets as [n][16]", {"targets": lambda a: a["targets"].reshape(N, 16)}),
        ("targets as [n][15]", {"targets": lambda a: a["targets"].reshape(N, 16)[:, :15]}),
        ("targets of rank 1", {"targets": lambda a: a["targets"].reshape(-1)}),
    ] + [case for k in ("pos_step", "rot_step", "pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "max_joint_step")
         for case in _floats(k, NAN, INF, 0.0, -1.0)] + _ints("max_iterations", 0, 2 ** 30 - 1) + _ints("max_waypoints", 0, 1024) + [
        ("no environments, starts of dim 6", {**_NO_ENVIRONMENTS, **_BAD_SHAPE}),
        ("no environments, pos_step=nan", {**_NO_ENVIRONMENTS, "settings.pos_step": NAN}),
        ("starts of dim 6, two targets", {**_BAD_SHAPE, "targets": lambda a: a["targets"][:2]}),
        ("two targets, a string among the environments", {"targets": lambda a: a["targets"][:2], **_BAD_ENVIRONMENT}),
        ("a string among the environments, two environments", {"environments": lambda a: [a["environments"][0], "env"]}),
        ("two environments, pos_step=nan", {**_BAD_COUNT, "settings.pos_step": NAN}),
        ("pos_step=nan, rot_step=inf", {"settings.pos_step": NAN, "settings.rot_step": INF}),
        ("max_joint_step=nan, max_iterations=-1", {"settings.max_joint_step": NAN, "settings.max_iterations": -1}),
        ("max_iterations=-1, max_waypoints=1025", {"settings.max_iterations": -1, "settings.max_waypoints": 1025}),
    ],
    "retime_multi_raw": _RETIME,
    "retime_multi_constrained_raw": _RETIME + _ints("blend_halvings", 0, 8) + _ints("max_rounds", 0, U32) + [
        (name, {"constraints": lambda a: _constraint(a["vamp"]), **changes}) for name, changes in _CONSTRAINTS] + [
        ("constraints=None, a string as the constraint settings", {"constraint_settings": "fine"}),
        ("max_samples=-1, blend_halvings=9", {"settings.max_samples": -1, "settings.blend_halvings": 9}),
        ("blend_halvings=9, max_rounds=-1", {"settings.blend_halvings": 9, "settings.max_rounds": -1}),
        ("max_rounds=-1, two constraints", {"settings.max_rounds": -1, **_TWO_CONSTRAINTS}),
        ("a negative acc_limit, two constraints", {"acc_limits": [-1, 1, 1, 1, 1, 1, 1], **_TWO_CONSTRAINTS}),
        ("no environments, two constraints", {**_NO_ENVIRONMENTS, **_TWO_CONSTRAINTS}),
    ],
})

# refusals of the planning.* functions themselves (their own checks, and the wrapper's words coming through)
PLAN_REFUSALS = {
    "rrtc_multi_raw": [("two environments", _BAD_COUNT), ("range=0 with dynamic_domain", {"settings.range": 0.0,
                                                                                         "settings.dynamic_domain": True})],
    "rrtc_multi_goals_raw": [
        ("a goal set of rank 1", {"goal_sets": lambda a: [a["goals"][:1], a["goals"][1], a["goals"][3:]]}),
        ("an empty goal set", {"goal_sets": lambda a: [a["goals"][:1], a["goals"][1:1], a["goals"][3:]]}),
        ("a goal set of dim 6", {"goal_sets": lambda a: [a["goals"][:1], a["goals"][1:3, :6], a["goals"][3:]]}),
        ("two goal sets", {"goal_sets": lambda a: [a["goals"][:1], a["goals"][1:]]}),
    ],
    "aorrtc_multi_raw": [("simplify=None", {"settings.simplify": None}), ("two environments", _BAD_COUNT)],
    "prm_multi_raw": [("k=0", {"settings.k": 0})],
    "fcit_multi_raw": [("n_samples=65", {"settings.n_samples": 65})],
    "roadmaps_build_raw": [("k=0", {"settings.k": 0})],
    "roadmaps_query_raw": [("an index past the last roadmap", {"index": [0, 2, 0]})],
    "simplify_multi_raw": [("REDUCE", {"settings.operations": ["REDUCE"]}), ("a path of dim 6", _PATH_CASES[0][1])],
    "optimize_multi_raw": [
        ("a path of dim 6", _PATH_CASES[0][1]),
        ("a path of rank 1", _PATH_CASES[1][1]),
        ("a string among the environments, a path of dim 6", _PATH_CASES[5][1]),
        ("a densified path longer than max_waypoints", {"resolution": 8.0, "settings.max_waypoints": 8}),
        ("a densified path as long as max_waypoints", {"resolution": 0.1, "settings.max_waypoints": 4}),
        ("step=0", {"settings.step": 0.0}),
    ],
    "rrtc_multi_constrained_raw": [("two constraints", _TWO_CONSTRAINTS), ("max_stretch=nan", {"max_stretch": NAN}),
                                   ("two environments", _BAD_COUNT)],
    "simplify_multi_constrained_raw": [("REDUCE", {"settings.operations": ["REDUCE"]}), ("two constraints", _TWO_CONSTRAINTS)],
    "optimize_multi_constrained_raw": [
        ("a path of dim 6", _PATH_CASES[0][1]),
        ("a densified path longer than max_waypoints", {"resolution": 8.0, "settings.max_waypoints": 8}),
        ("two constraints", _TWO_CONSTRAINTS),
    ],
    "cartesian_multi_raw": [("two targets", {"targets": lambda a: a["targets"][:2]}), ("pos_step=nan", {"settings.pos_step": NAN})],
    "retime_multi_raw": [("vel_limits of 6", {"vel_limits": np.ones(6)}), ("dt=1e-7", {"settings.dt": 1e-7})],
    "retime_multi_constrained_raw": [("two constraints", _TWO_CONSTRAINTS), ("blend_halvings=9", {"settings.blend_halvings": 9})],
}

# accepted calls: (case name, changes, n, the symbol that fails or None)
_SAMPLES_2D = (np.arange(64 * DIM).reshape(64, DIM) * 0.001).astype(np.float32)
_SAMPLES_3D = (np.arange(N * 64 * DIM).reshape(N, 64, DIM) * 0.002).astype(np.float32)
_GIVEN_SKIPS = {"skips": [5, 0, 7]}
ACCEPTED = {w: [("plain", {}, N, None), ("n = 0", {}, 0, None)] + [(f"fails at {s}", {}, N, s) for s in SYMBOLS[w]] for w in WRAPPERS}
for _w in ("rrtc_multi_raw", "rrtc_multi_goals_raw", "aorrtc_multi_raw", "prm_multi_raw", "fcit_multi_raw", "roadmaps_build_raw"):
    ACCEPTED[_w].append(("skips given", _GIVEN_SKIPS, N, None))
for _w in ("prm_multi_raw", "fcit_multi_raw", "roadmaps_build_raw"):
    ACCEPTED[_w] += [("samples for all", {"samples": _SAMPLES_2D}, N, None), ("samples per problem", {"samples": _SAMPLES_3D}, N, None),
                     ("samples and skips", {"samples": _SAMPLES_2D, **_GIVEN_SKIPS}, N, None)]
_DYNAMIC = {"settings.dynamic_domain": True, "settings.radius": 3.0, "settings.alpha": 0.25, "settings.min_radius": 0.5,
            "settings.start_tree_first": True}
ACCEPTED["rrtc_multi_raw"] += [("dynamic domain and start_tree_first", _DYNAMIC, N, None),
                               ("balance off", {"settings.balance": False}, N, None)]
ACCEPTED["rrtc_multi_goals_raw"] += [
    ("goal_counts=None", {"goal_counts": None, "goals": lambda a: a["goals"][:N]}, N, None),
    ("dynamic domain and start_tree_first", _DYNAMIC, N, None),
    ("a set of 2 goals, max_samples=3", {"settings.max_samples": 3}, N, None)]
ACCEPTED["aorrtc_multi_raw"] += [("flags off, simplify settings of its own", {
    "settings.optimize": False, "settings.cost_bound_resample": False, "settings.simplify_intermediate": False,
    "settings.simplify.operations": ["BSPLINE"], "settings.simplify.max_steps": 2}, N, None)]
_KEEP = {"settings.keep_roadmaps": True}
ACCEPTED["prm_multi_raw"] = [(name, {**changes, **_KEEP} if fail else changes, n, fail) for name, changes, n, fail in
                             ACCEPTED["prm_multi_raw"]] + [("keep_roadmaps", _KEEP, N, None), ("keep_roadmaps, n = 0", _KEEP, 0, None)]
ACCEPTED["roadmaps_query_raw"] += [("index given", {"index": [1, 0, 1]}, N, None)]
ACCEPTED["simplify_multi_raw"] += [("one operation, library defaults", {
    "settings.operations": ["bspline"], "settings.max_waypoints": 0, "settings.questions_per_round": 0}, N, None)]
ACCEPTED["optimize_multi_raw"] += [("densified", {"resolution": 1.0}, N, None)]
_PER_ITEM = {"constraints": lambda a: [_constraint(a["vamp"], k) for k in range(N)]}
_OWN_BAND_SETTINGS = {"constraint_settings": lambda a: a["vamp"].ConstraintSettings(max_iterations=5, pos_tol=0.002, check_step=0.125)}
for _w in ("rrtc_multi_constrained_raw", "simplify_multi_constrained_raw", "optimize_multi_constrained_raw"):
    ACCEPTED[_w] += [("one constraint per item", _PER_ITEM, N, None), ("one constraint per item, n = 0", {"constraints": []}, 0, None),
                     ("constraint settings given", _OWN_BAND_SETTINGS, N, None)]
ACCEPTED["rrtc_multi_constrained_raw"] += [("skips given, max_stretch=3", {**_GIVEN_SKIPS, "max_stretch": 3}, N, None),
                                           ("max_stretch=0", {"max_stretch": 0.0}, N, None)]
ACCEPTED["optimize_multi_constrained_raw"] += [("densified", {"resolution": 1.0}, N, None)]
for _w in ("cartesian_multi_raw", "retime_multi_raw", "retime_multi_constrained_raw"):
    ACCEPTED[_w] += [("no environments", _NO_ENVIRONMENTS, N, None), ("no environments, n = 0", _NO_ENVIRONMENTS, 0, None)] + [
        (f"no environments, fails at {s}", _NO_ENVIRONMENTS, N, s) for s in SYMBOLS[_w]]
ACCEPTED["cartesian_multi_raw"] += [("position_only, library defaults", {
    "settings.position_only": True, "settings.pos_step": 0.0, "settings.max_iterations": 0, "settings.max_waypoints": 0}, N, None),
    ("targets as [n][16]", {"targets": lambda a: a["targets"].reshape(N, 16)}, N, None)]
ACCEPTED["retime_multi_raw"] += [("stop_at_waypoints, library defaults", {
    "settings.stop_at_waypoints": True, "settings.blend": 0.0, "settings.dt": -1.0, "settings.max_grid": 0}, N, None)]
_ONE = {"constraints": lambda a: _constraint(a["vamp"])}
ACCEPTED["retime_multi_constrained_raw"] += [
    ("one constraint", _ONE, N, None), ("one constraint in a list", {"constraints": lambda a: [_constraint(a["vamp"])]}, N, None),
    ("one constraint per path", _PER_ITEM, N, None), ("one constraint, n = 0", _ONE, 0, None),
    ("no environments, one constraint per path", {**_NO_ENVIRONMENTS, **_PER_ITEM}, N, None),
    ("one constraint, constraint settings given", {**_ONE, **_OWN_BAND_SETTINGS}, N, None),
    ("constraints=None, constraint settings given", _OWN_BAND_SETTINGS, N, None),
    ("blend_halvings and max_rounds of its own", {"settings.blend_halvings": 8, "settings.max_rounds": 2}, N, None)] + [
    (f"one constraint per path, fails at {s}", _PER_ITEM, N, s) for s in SYMBOLS["retime_multi_constrained_raw"]]

ALL = ([f"refused / {w} / {name}" for w in WRAPPERS for name, _ in REFUSALS[w]] +
       [f"refused / planning above {w} / {name}" for w in WRAPPERS for name, _ in PLAN_REFUSALS[w]] +
       [f"accepted / {w} / {name}" for w in WRAPPERS for name, _, _, _ in ACCEPTED[w]])


# ---------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------
def _refused(vamp, install, wrapper, changes, call):
    """-> [the exception's type name, its words]"""
    install(_NoLibrary())
    a = _args(vamp, wrapper, N, changes)
    try:
        call(vamp, wrapper, a)
    except Exception as e:  # noqa: BLE001  (whatever it is, is the record)
        return [type(e).__name__, str(e)]
    return None


def _whole(wrapper, name):
    """whether the record of an accepted call is kept as it is; else what the entry was given and what came back are kept
    as digests of their JSON (as exact, a fiftieth of the size): the wrappers added later, but for their "plain" case"""
    return WRAPPERS.index(wrapper) < 9 or name == "plain"


def _accepted(vamp, install, wrapper, changes, n, fail, whole=True):
    """-> {"raw": the wrapper's record, "plan": that of the planning.* function above it}"""
    record = {}
    for level, call in (("raw", _raw), ("plan", _plan)):
        lib = _Recorder(fail)
        install(lib)
        a = _args(vamp, wrapper, n, changes)
        out = {}
        try:
            out["result"] = _plain(call(vamp, wrapper, a))
        except vamp.VmvError as e:
            out["error"] = [type(e).__name__, e.status, str(e).split(" (")[0]]
        finally:
            for e in a["environments"] or ():  # give the fake handles up while the stand-in still answers
                e._dirty()
        out.update(calls=lib.calls, entry=lib.entry, destroyed=lib.destroyed)
        for part in ("entry", "result"):
            if not whole and out.get(part) is not None:
                print(f"{wrapper} / {level} / {part}: {json.dumps(out[part], sort_keys=True)}")  # (what the digest is of)
                out[part] = {"sha256 of the JSON": hashlib.sha256(json.dumps(out[part], sort_keys=True).encode()).hexdigest()}
        if DESTROY[wrapper]:  # whatever the readout did, the handle the entry gave is destroyed once
            assert lib.destroyed.get(DESTROY[wrapper], 0) == (1 if lib.entry is not None else 0), (wrapper, level)
        record[level] = out
    return record


def _same(got, want):
    return json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f, open(GOLDEN_PATHS) as g:
        return {**json.load(f), **json.load(g)}


def test_the_table_covers_every_recorded_case(golden):
    assert len(set(ALL)) == len(ALL)
    assert sorted(golden) == sorted(ALL)


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_refusals(vamp, monkeypatch, golden, wrapper):
    install = lambda lib: monkeypatch.setattr(vamp, "lib", lib)  # noqa: E731
    for prefix, table, call in ((f"refused / {wrapper}", REFUSALS, _raw), (f"refused / planning above {wrapper}", PLAN_REFUSALS, _plan)):
        for name, changes in table[wrapper]:
            got = _refused(vamp, install, wrapper, changes, call)
            print(f"{prefix} / {name}: {got}")
            assert _same(got, golden[f"{prefix} / {name}"]), f"{prefix} / {name}: {got} != {golden[f'{prefix} / {name}']}"


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_accepted_calls(vamp, monkeypatch, golden, wrapper):
    install = lambda lib: monkeypatch.setattr(vamp, "lib", lib)  # noqa: E731
    for name, changes, n, fail in ACCEPTED[wrapper]:
        got = _accepted(vamp, install, wrapper, changes, n, fail, _whole(wrapper, name))
        want = golden[f"accepted / {wrapper} / {name}"]
        for level in ("raw", "plan"):
            for part in sorted(set(got[level]) | set(want[level])):
                assert _same(got[level].get(part), want[level].get(part)), \
                    f"accepted / {wrapper} / {name} / {level} / {part}: {got[level].get(part)} != {want[level].get(part)}"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    assert "--record" in sys.argv
    import vamp_mvt_amd

    real = vamp_mvt_amd.lib
    table = {}
    try:
        put = lambda lib: setattr(vamp_mvt_amd, "lib", lib)  # noqa: E731
        for w in WRAPPERS:
            for case, spoiled in REFUSALS[w]:
                table[f"refused / {w} / {case}"] = _refused(vamp_mvt_amd, put, w, spoiled, _raw)
            for case, spoiled in PLAN_REFUSALS[w]:
                table[f"refused / planning above {w} / {case}"] = _refused(vamp_mvt_amd, put, w, spoiled, _plan)
            for case, changed, count, failing in ACCEPTED[w]:
                table[f"accepted / {w} / {case}"] = _accepted(vamp_mvt_amd, put, w, changed, count, failing, _whole(w, case))
    finally:
        vamp_mvt_amd.lib = real
    assert sorted(table) == sorted(ALL)
    for path, wrappers in ((GOLDEN, WRAPPERS[:9]), (GOLDEN_PATHS, WRAPPERS[9:])):  # one case per line
        keys = sorted(k for k in table if k.split(" / ")[1].replace("planning above ", "") in wrappers)
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(table[k], sort_keys=True)}" for k in keys) + "\n}\n")
    print(len(table), "cases recorded")
