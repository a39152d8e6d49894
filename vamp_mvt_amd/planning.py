"""Host-side planner harness on top of the batched validity API.

The reference's planners are serial C++ templates that call `validate_motion` one edge at a time
(planning/rrtc.hh, prm.hh, fcit.hh).  They are NOT re-implemented here; this module is the small amount of host
logic needed to drive the GPU path the way those planners do:

  * `Halton`            the reference's deterministic sampler (random/halton.hh:75-108), restated in fp32 numpy
                        (bit-exact against the reference's own output, tests/golden/halton_panda.npz);
  * `rrtc`              a minimal RRT-Connect (the `sphere_cage_example.py` plumbing, BASELINE config 1): same
                        ingredients as rrtc.hh (two balanced trees, `range`-limited extension, connect loop), every
                        validity question answered by `validate_motion_batch` — extension and connect candidates of
                        one iteration are checked together;
  * `fcit`              the batch form of the FCIT* loop (fcit.hh:137-349): lazy A* over the complete graph of the valid
                        samples, the unknown edges of each candidate path validated together;
  * `build_roadmap`     the batched form of PRM's inner loops (prm.hh:109-189, roadmap construction :250-266):
                        validate all samples at once, then all k-nearest candidate edges at once, then connect
                        components / search on the host.

Nothing here is on the measured hot path; all collision work goes through vamp_mvt_amd.<robot>.validate_*_batch.
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass, field, replace

import numpy as np

from . import _waypoints

_PRIMES = np.array([3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59], np.float32)


class Halton:
    """vamp::rng::Halton<Robot> (random/halton.hh): default bases = the first `dimension` primes from 3 on."""

    max_iterations = 1000000

    def __init__(self, robot):
        self._lo = robot.lower_bounds()
        self._span = robot._span.copy()  # Robot::s_m
        self._dim = robot.dimension()
        self.reset()

    def reset(self):
        self.b = _PRIMES[: self._dim].copy()
        self.n = np.zeros(self._dim, np.float32)
        self.d = np.ones(self._dim, np.float32)
        self.iterations = 0

    def skip(self, count: int):
        for _ in range(count):
            self.next()

    def next(self) -> np.ndarray:
        f = np.float32
        self.iterations += 1
        if self.iterations > self.max_iterations:
            self.n[:] = 0
            self.d[:] = 1
            self.iterations = 0
            self.b = np.roll(self.b, -1)
        b, n, d = self.b, self.n, self.d
        xf = (d - n).astype(np.float32)
        x_eq_1 = xf == f(1)
        d = np.where(x_eq_1, np.floor((d * b).astype(np.float32)), d).astype(np.float32)
        y = np.where(x_eq_1, f(0), np.floor((d / b).astype(np.float32))).astype(np.float32)
        x_le_y = (~x_eq_1) & (xf <= y)
        while x_le_y.any():
            y = np.where(x_le_y, np.floor((y / b).astype(np.float32)), y).astype(np.float32)
            x_le_y = x_le_y & (xf <= y)
        n = np.where(x_eq_1, f(1), (np.floor(((b + f(1)) * y).astype(np.float32)) - xf)).astype(np.float32)
        self.n, self.d = n, d
        u = (n / d).astype(np.float32)
        return (u * self._span + self._lo).astype(np.float32)  # Robot::scale_configuration (panda.hh:77-80)

    def batch(self, count: int) -> np.ndarray:
        return np.stack([self.next() for _ in range(count)])


@dataclass
class RRTCSettings:
    """subset of planning/rrtc_settings.hh"""
    range: float = 2.0
    balance: bool = True
    tree_ratio: float = 1.0
    max_iterations: int = 100000
    max_samples: int = 100000


@dataclass
class RRTCMultiSettings:
    """settings of `rrtc_multi`: those of RRTCSettings, except that max_samples defaults to 8,192 — every problem of a
    call owns a node pool of max_samples nodes on the device — and check_every (rounds between two looks of the host at
    which problems are finished; 0 = the library's default).  dynamic_domain with radius, alpha, min_radius, and
    start_tree_first are rrtc_settings.hh's; their defaults here are OFF (the reference's are dynamic_domain=True and
    start_tree_first=True), which is `rrtc_multi` as it always was"""
    range: float = 2.0
    balance: bool = True
    tree_ratio: float = 1.0
    max_iterations: int = 100000
    max_samples: int = 8192
    check_every: int = 0
    dynamic_domain: bool = False
    radius: float = 4.0
    alpha: float = 0.0001
    min_radius: float = 1.0
    start_tree_first: bool = False


@dataclass
class PRMMultiSettings:
    """settings of `prm_multi`: n_samples samples per problem (a multiple of 64 from 64 to 8,128), the k nearest
    neighbours per vertex (1 .. 16) within `radius` (inf = no cut), keep_roadmaps = also return every problem's vertex
    flags and candidate edges"""
    n_samples: int = 2048
    k: int = 8
    radius: float = float("inf")
    keep_roadmaps: bool = False


@dataclass
class RoadmapsSettings:
    """settings of `build_roadmaps`: n_samples samples per roadmap (a multiple of 64 from 64 to 8,128) and the k nearest
    neighbours per sample (1 .. 16) within `radius` (inf = no cut)"""
    n_samples: int = 2048
    k: int = 8
    radius: float = float("inf")


@dataclass
class RoadmapQuerySettings:
    """settings of `DeviceRoadmaps.query`: the k_connect nearest valid samples tried per endpoint (1 .. 32, independent of
    the roadmap's k) within `radius` (inf = no cut)"""
    k_connect: int = 8
    radius: float = float("inf")


@dataclass
class FCITMultiSettings:
    """settings of `fcit_multi`: n_samples samples per problem (a multiple of 64 from 64 to 2,048), max_iterations
    searches per problem, questions_per_round (edge questions per problem per round, 1 .. 32: the first is the one the
    search needs next, the others are predictions; 1 is what the measured sweep favours, since a prediction costs a
    search) and check_every (rounds between two looks of the host at which problems are finished; 0 = the library's
    default)"""
    n_samples: int = 1024
    max_iterations: int = 100000
    questions_per_round: int = 1
    check_every: int = 0


@dataclass
class AORRTCMultiSettings:
    """settings of `aorrtc_multi` (planning/aorrtc_settings.hh): range, balance, tree_ratio of the RRT-Connect searches;
    max_iterations of all stages together, max_internal_iterations of one cost-bounded search, max_samples (every problem
    owns a node pool of that many nodes on the device, hence 8,192 and not the reference's 100,000),
    max_cost_bound_resamples (at most 64; the reference's default is 1,000), max_searches (cost-bounded searches per
    problem, 0 = no limit but max_iterations; not in the reference), `simplify` (SimplifyMultiSettings or the
    reference-shaped SimplifySettings) and check_every (0 = the library's default)"""
    range: float = 2.0
    balance: bool = True
    tree_ratio: float = 1.0
    optimize: bool = True
    cost_bound_resample: bool = True
    simplify_intermediate: bool = True
    max_iterations: int = 100000
    max_internal_iterations: int = 100000
    max_samples: int = 8192
    max_cost_bound_resamples: int = 64
    max_searches: int = 0
    simplify: object = None
    check_every: int = 0


PLAN_STATUS = ("solved", "max_iterations", "max_samples", "no_path", "invalid_endpoint")  # VMV_PLAN_*
SIMPLIFY_STATUS = ("ok", "capacity", "out_of_band")  # VMV_SIMPLIFY_* (the last: simplify_multi_constrained only)


@dataclass
class SimplifyMultiSettings:
    """settings of `simplify_multi`: the reference's simplification defaults (max_iterations, operations, and the
    B-spline routine's max_steps, min_change, midpoint_interpolation), then what the lockstep form adds: max_waypoints
    (every path of a call owns that many waypoints on the device, twice), questions_per_round (edge questions per path
    per round: 2, 4, 8, 16, 32 or 64) and check_every (rounds between two looks of the host at which paths are
    finished); 0 = the library's default for each of the three"""
    max_iterations: int = 4
    operations: list = field(default_factory=lambda: ["SHORTCUT", "BSPLINE"])
    max_steps: int = 5
    min_change: float = 0.05
    midpoint_interpolation: float = 0.5
    max_waypoints: int = 2048
    questions_per_round: int = 0
    check_every: int = 0
    interpolate: int = 0  # must stay 0


@dataclass
class PlanningResult:
    """planning/plan.hh:172-179"""
    path: list = field(default_factory=list)
    iterations: int = 0
    size: list = field(default_factory=list)
    validity_calls: int = 0
    cost: float = float("inf")
    edges_checked: int = 0
    samples_drawn: int = 0
    status: str = ""  # rrtc_multi, prm_multi: one of PLAN_STATUS; simplify_multi: one of SIMPLIFY_STATUS
    roadmap: object = None  # prm_multi with keep_roadmaps: (vertex flags, candidate pairs [m][2], their flags)
    first_cost: float = float("inf")  # aorrtc_multi: the cost after the first stage
    searches: int = 0                 # aorrtc_multi: cost-bounded searches run
    improvements: int = 0             # aorrtc_multi: those that gave a cheaper path
    known_valid_edges: int = 0        # fcit_multi: edges the walk found valid
    goal_index: int = -1              # rrtc_multi_goals: the goal of the problem's set the path ends in (-1 = unsolved)

    @property
    def solved(self):
        return len(self.path) > 0


class _Tree:
    def __init__(self, dim):
        self.pts = np.zeros((0, dim), np.float32)
        self.parent = []

    def add(self, q, parent):
        self.pts = np.vstack([self.pts, q[None, :]])
        self.parent.append(parent)
        return len(self.parent) - 1

    def nearest(self, q):
        d = np.linalg.norm(self.pts - q[None, :], axis=1)
        i = int(np.argmin(d))
        return i, float(d[i])

    def trace(self, i):
        out = []
        while True:
            out.append(self.pts[i])
            if self.parent[i] == i:
                return out
            i = self.parent[i]


def rrtc(robot, start, goal, environment, settings: RRTCSettings | None = None, sampler: Halton | None = None):
    """Minimal RRT-Connect on the batched validity API (same structure as planning/rrtc.hh:33-245)."""
    s = settings or RRTCSettings()
    rng = sampler or Halton(robot)
    start = np.asarray(start, np.float32)
    goals = np.asarray(goal, np.float32)
    goals = goals[None] if goals.ndim == 1 else goals  # the reference's multi-goal form: every goal roots the goal tree
    res = PlanningResult()

    def motion(a, b):
        res.validity_calls += 1
        return robot.validate_motion_batch(np.ascontiguousarray(a), np.ascontiguousarray(b), environment)

    direct = motion(np.repeat(start[None], len(goals), 0), goals)  # rrtc.hh:60-73
    if direct.any():
        res.path, res.size = [start, goals[int(np.argmax(direct))]], [1, 1]
        return res
    tree_a, tree_b = _Tree(len(start)), _Tree(len(start))
    tree_a.add(start, 0)
    for g in goals:
        tree_b.add(g, len(tree_b.parent))
    a_is_start = True
    while res.iterations < s.max_iterations and len(tree_a.parent) + len(tree_b.parent) < s.max_samples:
        res.iterations += 1
        asize, bsize = len(tree_a.parent), len(tree_b.parent)
        if (not s.balance) or abs(asize - bsize) / asize < s.tree_ratio:  # rrtc.hh:100-108
            tree_a, tree_b = tree_b, tree_a
            a_is_start = not a_is_start
        target = rng.next()
        ni, dist = tree_a.nearest(target)
        near = tree_a.pts[ni]
        reach = min(dist, s.range)
        if dist <= 0:
            continue
        new = (near + (target - near) * np.float32(reach / dist)).astype(np.float32)
        if not bool(motion(near[None], new[None])[0]):  # extend (rrtc.hh:136-140)
            continue
        new_i = tree_a.add(new, ni)
        # connect (rrtc.hh:160-191): march from tree_b's nearest node towards `new` in `range` steps; all the
        # steps of the march are validated in ONE batch and the first invalid one cuts it
        bi, bdist = tree_b.nearest(new)
        origin = tree_b.pts[bi]
        n_steps = max(int(np.ceil(bdist / s.range)), 1)
        way = np.stack([(origin + (new - origin) * np.float32(min((k + 1) * s.range, bdist) / bdist)).astype(np.float32)
                        for k in range(n_steps)]) if bdist > 0 else new[None]
        froms = np.vstack([origin[None], way[:-1]])
        ok = motion(froms, way)
        n_ok = int(np.argmin(ok)) if not ok.all() else len(ok)
        prev = bi
        for k in range(n_ok):
            prev = tree_b.add(way[k], prev)
        if n_ok == len(ok):  # reached `new`: join the two branches
            pa = tree_a.trace(new_i)[::-1]
            pb = tree_b.trace(prev)
            path = pa + pb[1:] if np.array_equal(pa[-1], pb[0]) else pa + pb
            if not a_is_start:
                path = path[::-1]
            res.path = [np.asarray(p, np.float32) for p in path]
            res.size = [len(tree_a.parent), len(tree_b.parent)]
            return res
    res.size = [len(tree_a.parent), len(tree_b.parent)]
    return res


def rrtc_multi(robot, starts, goals, environments, settings: RRTCMultiSettings | None = None, skips=None):
    """RRT-Connect for many independent problems in lockstep on the device: problem p from starts[p] to goals[p]
    ([n][dim] arrays, one goal each) in environments[p] (None = the empty environment), sampling the Halton samples
    skips[p] + 1, skips[p] + 2, ... (None = 0 for all).  -> list[PlanningResult], one per problem: `path` (waypoints,
    empty if unsolved), `iterations`, `size` = [|A|, |B|] and `status` (one of PLAN_STATUS).

    Per round every unfinished problem asks one edge question and ONE validate_motion_batch_multi launch sequence
    answers all of them; nearest-neighbour search, extension, connect march and bookkeeping run in a device kernel, so
    a round costs a handful of launches however many problems are in flight.

    The decisions are those of `rrtc` (rrtc.hh without dynamic domain), in fp32 with one rounding per operation and
    the first nearest node on ties, so a problem's result is defined bit for bit and does not depend on the other
    problems of the call.  Agreement with `rrtc` itself is NOT pinned: where `range` is not an fp32 number, or numpy's
    float64 intermediates round differently, `rrtc` may take another decision.

    The default max_samples of this call is 8,192 (RRTCMultiSettings), not rrtc's 100,000: the node pool is
    allocated per problem, max_samples * (dim + 1) * 4 bytes each.  skips[p] + max_iterations may not exceed 1,000,000
    (the Halton sequence's validity limit).

    With dynamic_domain or start_tree_first set in the settings (RRTCMultiSettings; both off by default) the call goes
    through `rrtc_multi_goals`' entry point with one goal per problem, and the results carry `goal_index` 0."""
    s = settings or RRTCMultiSettings()
    if _rrtc_additions_off(s):
        return _rrtc_results(robot.rrtc_multi_raw(starts, goals, environments, s, skips))
    return _rrtc_results(robot.rrtc_multi_goals_raw(starts, goals, None, environments, s, skips))


def _rrtc_additions_off(s):
    """whether the five fields RRTCMultiSettings has beyond vmv_rrtc_settings all have their defaults"""
    d = RRTCMultiSettings()
    return all(getattr(s, k, getattr(d, k)) == getattr(d, k)
               for k in ("dynamic_domain", "radius", "alpha", "min_radius", "start_tree_first"))


def _planning_results(raw, lengths="path_lengths", points="paths", **fields):
    """One PlanningResult per problem (or path) of a planner wrapper's dict `raw`: `path` = the rows of raw[points] that
    raw[lengths] gives it, `iterations`, `size` where the dict has sizes, and each attribute named in `fields` as
    (raw key, conversion), left at its default where the dict lacks the key.  status: one of PLAN_STATUS unless given."""
    fields.setdefault("status", ("status", lambda s: PLAN_STATUS[int(s)]))
    ends = np.cumsum(raw[lengths], dtype=np.int64)
    out = []
    for p in range(len(ends)):
        pts = raw[points][ends[p] - int(raw[lengths][p]):ends[p]]
        res = PlanningResult(path=[q.copy() for q in pts], iterations=int(raw["iterations"][p]))
        if "sizes" in raw:
            res.size = [int(raw["sizes"][p, 0]), int(raw["sizes"][p, 1])]
        for name, (key, convert) in fields.items():
            if key in raw:
                setattr(res, name, convert(raw[key][p]))
        out.append(res)
    return out


def _rrtc_results(raw):
    out = _planning_results(raw, goal_index=("goal_indices", int), band_refused=("band_refused", int))  # (the latter: constrained calls)
    if out:  # the call's totals ride on the first result (a round = one validate_motion_batch_multi call)
        out[0].validity_calls, out[0].edges_checked = raw["rounds"], raw["questions"]
    return out


def rrtc_multi_goals(robot, starts, goal_sets, environments, settings: RRTCMultiSettings | None = None, skips=None):
    """`rrtc_multi` with a set of goals per problem (rrtc.hh:33-38): problem p from starts[p] to any goal of goal_sets[p], a
    [G_p][dim] array with G_p >= 1 (the IK solutions of one grasp pose, say; a [dim] vector or an empty set is refused).
    -> list[PlanningResult] as `rrtc_multi`'s, each with `goal_index`: the goal of its own set a solved problem's path
    ends in (-1 = unsolved).

    Per problem the edges start -> goal g are tried first, in order of g and one per round; the first valid one is the
    path.  Otherwise every goal is a root of the goal tree and the search is `rrtc_multi`'s.  The settings'
    dynamic_domain (radius, alpha, min_radius) and start_tree_first work as in rrtc.hh; a sample the dynamic domain
    rejects asks no edge question and so costs no round.  With those off and one goal per problem the results
    are `rrtc_multi`'s bit for bit.  1 + G_p may not exceed max_samples."""
    s = settings or RRTCMultiSettings()
    sets = []
    for g in goal_sets:
        g = np.asarray(g, np.float32)
        if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] != robot.dimension():
            raise TypeError(f"expected every goal set as a [G][{robot.dimension()}] array with G >= 1, got shape {g.shape}")
        sets.append(g)
    packed = np.concatenate(sets) if sets else np.zeros((0, robot.dimension()), np.float32)
    counts = np.array([len(g) for g in sets], np.int64)
    return _rrtc_results(robot.rrtc_multi_goals_raw(starts, packed, counts, environments, s, skips))


def rrtc_multi_constrained(robot, starts, goal_sets, environments, constraints, settings: RRTCMultiSettings | None = None,
                           constraint_settings=None, skips=None, max_stretch=2.0):
    """`rrtc_multi_goals` under end-effector constraints (vmv_rrtc_multi_constrained): constraints is one
    EEConstraint for all problems or one per problem; every tree node is projected into its band and every edge is
    band-checked inside the rounds, one extra launch per round.  Endpoints come from `project_goals`: a problem whose
    start is out of band, or none of whose goals is in band, ends "invalid_endpoint" with no path and no question, and
    out-of-band goals of a set are never used (goal_index still counts within the caller's set).  constraint_settings: a
    ConstraintSettings (its check_step spaces the band samples of an edge); max_stretch: a projected node farther than
    max_stretch * range from the edge's near end is refused.  -> list[PlanningResult] as `rrtc_multi_goals`'s.  The path's
    edges pass `constraint_check_motion_batch`; `simplify_multi_constrained` simplifies it and
    `optimize_multi_constrained` optimises it inside the band and `aorrtc_multi_constrained` searches for a cheaper one
    there, while `simplify_multi`, `optimize_multi` and `aorrtc_multi` do not know the constraint - ask
    `validate_paths_constrained` of what they return.  Each result also carries `band_refused`: the questions the constraint answered 0."""
    s = settings or RRTCMultiSettings()
    sets = []
    for g in goal_sets:
        g = np.asarray(g, np.float32)
        if g.ndim != 2 or g.shape[0] < 1 or g.shape[1] != robot.dimension():
            raise TypeError(f"expected every goal set as a [G][{robot.dimension()}] array with G >= 1, got shape {g.shape}")
        sets.append(g)
    packed = np.concatenate(sets) if sets else np.zeros((0, robot.dimension()), np.float32)
    counts = np.array([len(g) for g in sets], np.int64)
    return _rrtc_results(robot.rrtc_multi_constrained_raw(starts, packed, counts, environments, constraints, s, constraint_settings,
                                                          max_stretch, skips))


def prm_multi(robot, starts, goals, environments, settings: PRMMultiSettings | None = None, skips=None, samples=None):
    """A roadmap per problem for many independent problems in one call on the device: problem p from starts[p] to
    goals[p] ([n][dim] arrays) in environments[p] (None = the empty environment), over the Halton samples skips[p] + 1,
    ... (None = 0 for all) or over `samples` ([n][n_samples][dim]; [n_samples][dim] serves every problem).
    -> list[PlanningResult], one per problem: `path` (waypoints, empty if unsolved), `cost` (inf if unsolved),
    `iterations` (n_samples where the roadmap was searched, 0 for a direct solution or an invalid endpoint), `size` =
    [valid vertices, valid edges], `edges_checked` = candidate edges, `status` (one of PLAN_STATUS: "solved", "no_path",
    "invalid_endpoint") and, with keep_roadmaps, `roadmap`.

    The launches are a fixed sequence whatever the problems are: all vertices of all problems in ONE
    validate_batch_multi call, the k nearest valid neighbours of every valid vertex, all candidate edges in ONE
    validate_motion_batch_multi call, the shortest path per problem.  The result is defined bit for bit —
    fp32 with one rounding per operation, neighbours in the order (squared distance, vertex id), the shortest-path
    cost as the least fixpoint of g[v] = min fl(g[u] + w), the parent with the lowest id — and depends on the problem's
    own inputs alone.  Agreement with the reference's incremental PRM is not claimed."""
    s = settings or PRMMultiSettings()
    raw = robot.prm_multi_raw(starts, goals, environments, s, skips, samples)
    out = _planning_results(raw, cost=("costs", float), edges_checked=("candidate_edges", int),
                            roadmap=("roadmaps", lambda r: r))
    if out:  # the call's validation calls ride on the first result
        out[0].validity_calls = raw["rounds"]
    return out


class DeviceRoadmaps:
    """Roadmaps kept on the device (`build_roadmaps`): `len()` roadmaps, roadmap r built in environments[r].  Holds the
    library's handle and the Environment objects it refers to, so that no environment is collected before its roadmaps;
    the handle is destroyed by `close()` (or `with`), at the latest when the object is collected.  A roadmap answers for
    its environment as it was when the roadmap was built: an Environment changed since (or moved to another device) has
    given up the handle the roadmap refers to, and `query` then raises ValueError."""

    def __init__(self, robot, handle, environments, settings):
        self._robot, self._handle, self._environments, self.settings = robot, handle, environments, settings
        self._generations = [e._generation for e in environments]

    def __len__(self):
        return len(self._environments)

    def _open(self):
        if self._handle is None:
            raise ValueError("the roadmaps are closed")
        return self._handle

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None:
            self._robot.roadmaps_destroy_raw(handle)
        self._environments = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # at interpreter exit the library may be gone first
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def summary(self):
        """-> (valid samples, candidate edges, valid edges) per roadmap, uint32 arrays"""
        return self._robot.roadmaps_summary_raw(self._open(), len(self))

    def roadmap(self, r):
        """roadmap r as kept on the device -> (samples [n_samples][dim], their flags, candidate pairs [m][2] of sample
        ids a < b in candidate order, their flags)"""
        if not 0 <= int(r) < len(self):
            raise IndexError(f"roadmap {r} of {len(self)}")
        return self._robot.roadmaps_roadmap_raw(self._open(), int(r), int(self.settings.n_samples))

    def query(self, starts, goals, index=None, settings: RoadmapQuerySettings | None = None):
        """Query q from starts[q] to goals[q] ([n][dim] arrays) against roadmap index[q] (None = roadmap 0 for all).
        -> list[PlanningResult], one per query: `path` (waypoints, empty if unsolved), `cost` (inf if unsolved),
        `iterations` (n_samples where the roadmap was searched, 0 for a direct solution or an invalid endpoint), `size` =
        [valid connection edges of the start, of the goal], `edges_checked` = 1 + the connections tried for both endpoints
        and `status` ("solved", "no_path", "invalid_endpoint").

        A fixed sequence of launches whatever the queries are: all endpoints in ONE validate_batch_multi call, the
        k_connect nearest valid samples of every endpoint, 1 + 2 k_connect edge questions per query in ONE
        validate_motion_batch_multi call, the shortest path per query over the roadmap's edges and its own connection
        edges.  Defined bit for bit, as `prm_multi` is; a query's result depends on its endpoints, its
        roadmap and the settings alone."""
        s = settings or RoadmapQuerySettings()
        handle = self._open()
        stale = [r for r, (e, g) in enumerate(zip(self._environments, self._generations)) if e._generation != g]
        if stale:
            raise ValueError(f"the environments of roadmaps {stale} changed after the roadmaps were built")
        raw = self._robot.roadmaps_query_raw(handle, len(self), starts, goals, index, s)
        out = _planning_results(raw, cost=("costs", float), edges_checked=("edges_checked", int))
        if out:  # the call's validation calls ride on the first result
            out[0].validity_calls = raw["rounds"]
        return out


def build_roadmaps(robot, environments, settings: RoadmapsSettings | None = None, skips=None, samples=None) -> DeviceRoadmaps:
    """One roadmap per environment (None = the empty environment), built in one call and kept on the device: over the
    Halton samples skips[r] + 1, ... (None = 0 for all) or over `samples` ([n][n_samples][dim]; [n_samples][dim] serves
    every roadmap).  All samples go through ONE validate_batch_multi call and all candidate edges through ONE
    validate_motion_batch_multi call, as in `prm_multi`, but no endpoint takes part: the cost is paid once per scene and
    `DeviceRoadmaps.query` answers any number of (start, goal) pairs against it."""
    s = settings or RoadmapsSettings()
    handle, envs = robot.roadmaps_build_raw(environments, s, skips, samples)
    return DeviceRoadmaps(robot, handle, envs, s)


def fcit_multi(robot, starts, goals, environments, settings: FCITMultiSettings | None = None, skips=None, samples=None):
    """A lazy search of the complete graph over each problem's valid samples, for many independent problems in one call
    on the device; the arguments are those of `prm_multi`.  -> list[PlanningResult], one per problem: `path` (waypoints,
    empty if unsolved), `cost` (inf if unsolved), `iterations` (searches run), `size` = [valid vertices, blocked edges],
    `known_valid_edges` and `status` (one of PLAN_STATUS: "solved", "max_iterations", "no_path", "invalid_endpoint").

    Per problem: A* from the start to the goal over the valid vertices with every unchecked edge taken as free; the
    proposed path's edges are asked from the start, the first invalid one is blocked and the search runs again, until a
    proposed path is valid throughout or none is left.  The complete graph contains every k-nearest graph
    over the same samples, so what `prm_multi` solves this solves, at no higher cost, and it asks only the edges of the
    paths it proposes.  All vertices go through ONE validate_batch_multi call; the searches advance in lockstep rounds
    of questions_per_round questions per problem, the first the one the search needs, the others predictions that only
    fill an answer cache.  The result is defined bit for bit (fp32, one rounding per operation, pops ordered by (g + h,
    vertex id), closed vertices never reopened) and depends on the problem's own inputs and max_iterations alone.
    Agreement with the reference's FCIT* (an edge-queue search) is not claimed."""
    s = settings or FCITMultiSettings()
    raw = robot.fcit_multi_raw(starts, goals, environments, s, skips, samples)
    out = _planning_results(raw, cost=("costs", float), known_valid_edges=("known_valid_edges", int))
    if out:  # the call's totals ride on the first result (validity_calls: the vertices' call and one per round)
        out[0].validity_calls, out[0].edges_checked = raw["rounds"], raw["questions"]
    return out


def aorrtc_multi(robot, starts, goals, environments, settings: AORRTCMultiSettings | None = None, skips=None):
    """AORRTC (planning/aorrtc.hh) for many independent problems on the device, the arguments those of `rrtc_multi`.
    -> list[PlanningResult], one per problem: `path` (the cheapest found, empty if the first stage found none), `cost`
    and `first_cost` (Path::cost of the returned path and of the first stage's; inf if unsolved), `searches`,
    `improvements`, `iterations` (all stages), `size` = [|A|, |B|] of the last search run and `status`.

    Per problem: a first solution by `rrtc_multi`'s contract, simplified by `simplify_multi`'s; then, while the budget
    lasts, RRT-Connect searches under the cost of the best path so far on fresh trees — samples drawn directly from the
    prolate hyperspheroid of that cost, the nearest node by the reference's asymmetric cost-space rule, new nodes
    re-parented under resampled cost bounds — each new solution simplified and kept if it is cheaper.  Search g of
    every still-optimising problem is one lockstep call (one edge question per problem per round); the
    solutions of a generation are simplified in one `simplify_multi` call; the host compares costs.

    Every operation is fp32 with one rounding, the sampler included (a counter-based hash seeded with skips[p], its own
    ln, Marsaglia's polar method, a Householder reflection: + - * / sqrt and integer operations only), so a problem's
    result is defined bit for bit and does not depend on the other problems of the call or on check_every.  Agreement
    with the reference's own random stream is not claimed."""
    return _aorrtc_results(robot.aorrtc_multi_raw(starts, goals, environments, _aorrtc_settings(settings), skips))


def _aorrtc_settings(settings) -> AORRTCMultiSettings:
    s = settings or AORRTCMultiSettings()
    if not isinstance(s.simplify, SimplifyMultiSettings):
        s = replace(s, simplify=_as_simplify_multi_settings(s.simplify))
    return s


def _aorrtc_results(raw):
    out = _planning_results(raw, cost=("costs", float), first_cost=("first_costs", float), searches=("searches", int),
                            improvements=("improvements", int), band_refused=("band_refused", int))  # (the last: the constrained call)
    if out:  # the call's totals over all stages ride on the first result
        out[0].validity_calls, out[0].edges_checked = raw["rounds"], raw["questions"]
    return out


def aorrtc_multi_constrained(robot, starts, goals, environments, constraints, settings: AORRTCMultiSettings | None = None,
                             constraint_settings=None, skips=None, max_stretch=2.0):
    """`aorrtc_multi` under end-effector constraints (vmv_aorrtc_multi_constrained): constraints is one
    EEConstraint for all problems or one per problem.  The first solution is `rrtc_multi_constrained`'s (one goal; a problem
    whose start or goal is out of band ends "invalid_endpoint" with no path, infinite costs and no search), every
    simplification `simplify_multi_constrained`'s (a path it reports "out_of_band" stays as it is), and in every
    cost-bounded search each new node - an extension's, a march step's - is projected into the band, refused beyond
    max_stretch * range, and each edge band-checked, one extra launch per round; a re-parent edge is band-checked only.
    -> list[PlanningResult] as `aorrtc_multi`'s, each with `band_refused`: the questions of all stages the constraint
    answered 0.  A problem's result is its own, bit for bit; with a constraint that restricts nothing it is `aorrtc_multi`'s.

    Not promised: the halves of an edge the simplifier subdivides are not asked again, so `validate_paths_constrained`,
    which samples every returned edge anew, may still answer False for some paths; only the end-effector frame can be
    constrained."""
    return _aorrtc_results(robot.aorrtc_multi_constrained_raw(starts, goals, environments, constraints, _aorrtc_settings(settings),
                                                              constraint_settings, max_stretch, skips))


def _as_simplify_multi_settings(settings) -> SimplifyMultiSettings:
    """SimplifyMultiSettings from the reference-shaped SimplifySettings (api.py: its B-spline numbers sit in .bspline)"""
    if settings is None:
        return SimplifyMultiSettings()
    if isinstance(settings, SimplifyMultiSettings):
        return settings
    b = settings.bspline
    return SimplifyMultiSettings(max_iterations=settings.max_iterations, operations=list(settings.operations),
                                 max_steps=b.max_steps, min_change=b.min_change,
                                 midpoint_interpolation=b.midpoint_interpolation,
                                 max_waypoints=getattr(settings, "max_waypoints", 2048),
                                 questions_per_round=getattr(settings, "questions_per_round", 0),
                                 check_every=getattr(settings, "check_every", 0),
                                 interpolate=getattr(settings, "interpolate", 0))


def path_cost(path) -> float:
    """Path::cost (planning/plan.hh:13-32): the fp32 sum of the segment lengths; inf below 2 waypoints"""
    if len(path) < 2:
        return float("inf")
    p = np.stack(path).astype(np.float32)
    seg = np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1, dtype=np.float32))
    return float(seg.sum(dtype=np.float32))


def simplify_multi(robot, paths, environments, settings=None):
    """The reference's simplify() (planning/simplify.hh) with its SHORTCUT and BSPLINE routines for many independent
    paths in lockstep on the device: paths[p] ([len][dim] array or list of waypoints) in environments[p] (None = the
    empty environment).  -> list[PlanningResult], one per path: `path`, `iterations` (as the reference counts them),
    `cost` (Path::cost) and `status` (one of SIMPLIFY_STATUS).  settings: SimplifyMultiSettings, or the
    reference-shaped SimplifySettings (converted).

    Per round every unfinished path asks questions_per_round edge questions and ONE validate_motion_batch_multi launch
    sequence answers all of them; erasing, subdividing, the min_change test and the bookkeeping run in a device kernel
    (DESIGN §5d).  Shortcut asks the candidates of a waypoint from the far end a window at a time, a B-spline step
    both motions of each candidate; either way the path is the one the reference's one-question-at-a-time loops end
    with, in fp32 with one rounding per operation, so a path's result is defined bit for bit and does not depend on
    questions_per_round, check_every or the other paths of the call.

    REDUCE and PERTURB (they draw random numbers) and `interpolate` raise NotImplementedError.  A path owns
    max_waypoints waypoints; where a B-spline subdivision would need more, the path comes back as it stood, a valid
    path still, with status "capacity"."""
    s = _as_simplify_multi_settings(settings)
    return _simplify_results(robot.simplify_multi_raw(paths, environments, s))


def _simplify_results(raw):
    out = _planning_results(raw, "lengths", "points", edges_checked=("questions", int), band_refused=("band_refused", int),
                            status=("status", lambda k: SIMPLIFY_STATUS[int(k)]))  # (band_refused: the constrained call)
    for res in out:
        res.cost = path_cost(res.path)
    if out:  # the call's totals ride on the first result (a round = one validate_motion_batch_multi call)
        out[0].validity_calls, out[0].edges_checked = raw["rounds"], raw["total_questions"]
    return out


def simplify_multi_constrained(robot, paths, environments, constraints, settings=None, constraint_settings=None):
    """`simplify_multi` inside the band of end-effector constraints (vmv_simplify_multi_constrained):
    constraints is one EEConstraint for all paths or one per path, constraint_settings a ConstraintSettings (its check_step
    spaces the band samples of an edge).  paths takes the paths of `rrtc_multi_constrained`'s results as they are.
    -> list[PlanningResult] as `simplify_multi`'s, each with `band_refused` and `status` "ok", "capacity" or "out_of_band".

    The contract is `simplify_multi`'s with three changes.  Every question is validate_motion AND the band test of the
    edge (`constraint_check_motion_batch`'s answer).  A B-spline candidate is projected into the band before it is asked
    (`project_batch`'s result bit for bit); a projection that does not converge answers both motions 0, and the waypoint
    is replaced by the projected point iff both motions are answered 1 and the projected point is farther than
    min_change from the waypoint.  And the input is looked at first: a path of 3 waypoints or more whose first waypoint
    or one of whose edges is out of band comes back as it is with status "out_of_band", 0 iterations and 0 questions,
    without disturbing the others.  `band_refused` counts, of the questions the one-question-at-a-time loop asks, those
    the constraint answered 0 whatever validity said; it does not depend on questions_per_round.

    As in `simplify_multi` the halves of a subdivided edge are not asked again: every point of a returned path lies on
    an asked in-band edge or on a half of one, so within check_step / 2 of joint-space length of a passing sample.  With
    a constraint that restricts nothing the result is `simplify_multi`'s byte for byte.  One more launch per round than
    `simplify_multi`: one wave per question slot."""
    s = _as_simplify_multi_settings(settings)
    return _simplify_results(robot.simplify_multi_constrained_raw(paths, environments, constraints, s, constraint_settings))


def validate_path(robot, path, environment) -> bool:
    """Path::validate (planning/plan.hh:155-168): every consecutive pair is a valid motion — one batch."""
    if len(path) < 2:
        return True
    p = np.stack(path).astype(np.float32)
    return bool(robot.validate_motion_batch(p[:-1], p[1:], environment).all())


def validate_paths(robot, paths, environments) -> np.ndarray:
    """validate_path for many paths, path p in environments[p] (None = the empty environment) -> bool[len(paths)]: every
    path's consecutive pairs in ONE validate_motion_batch_multi call.  A path of fewer than 2 waypoints is valid."""
    dim = robot.dimension()
    pts = [np.asarray(p, np.float32).reshape(-1, dim) for p in paths]
    counts = [max(len(p) - 1, 0) for p in pts]
    empty = np.zeros((0, dim), np.float32)
    ok = robot.validate_motion_batch_multi(np.concatenate([p[:-1] for p in pts] + [empty]),
                                           np.concatenate([p[1:] for p in pts] + [empty]), environments, counts)
    # path p is valid iff its segment holds no invalid edge (prefix counts: empty segments need no special case)
    bad = np.concatenate([[0], np.cumsum(~ok)])
    ends = np.concatenate([[0], np.cumsum(counts)])
    return bad[ends[1:]] == bad[ends[:-1]]


@dataclass
class PathClearance:
    """path_clearance's answer for one path: the smallest `env` and `self` clearance over its samples (self_: `self` is
    no field name), and the (segment, k) of the sample each was found at (the first such sample; None for a path without
    waypoints)"""
    env: float
    self_: float
    env_at: tuple | None
    self_at: tuple | None


def path_samples(path, resolution):
    """The samples path_clearance takes of one path ([len][dim]) -> (float32 [n][dim], int64 [n][2] = (segment, k)).
    Segment (a, b) is sampled at a + (b - a) * k / m for k = 0..m with m = max(1, ceil(|b - a| * resolution)), computed in
    float64 and cast to fp32; both end points of every segment are samples, so an inner waypoint appears twice.  A path
    of one waypoint is that one sample, at (0, 0)."""
    p = np.asarray(path, np.float64)
    if p.ndim != 2:
        raise TypeError("expected a [len][dim] path")
    if len(p) == 1:
        return p.astype(np.float32), np.zeros((1, 2), np.int64)
    pts, at = [np.zeros((0, p.shape[1]))], [np.zeros((0, 2), np.int64)]
    for i in range(len(p) - 1):
        a, b = p[i], p[i + 1]
        m = max(1, int(np.ceil(np.sqrt(((b - a) ** 2).sum()) * resolution)))
        k = np.arange(m + 1)
        pts.append(a[None, :] + (b - a)[None, :] * (k / m)[:, None])
        at.append(np.stack([np.full(m + 1, i), k], axis=1).astype(np.int64))
    return np.concatenate(pts).astype(np.float32), np.concatenate(at)


def path_clearance(robot, paths, environments, resolution=None):
    """The clearance of finished plans: paths[p] ([len][dim]) in environments[p] (None = the empty environment) ->
    list[PathClearance].  Every segment is sampled as path_samples describes, `resolution` samples per unit of
    configuration-space length (default: robot.resolution()), and the samples of all paths go through ONE
    clearance_batch_multi call.  These samples are NOT the rakes validate_motion walks (those step back from the far end
    in fp32, 8 to a rake): a path's clearance is a measurement at its own, evenly spaced samples, not a replay of the
    validation, and a positive value does not by itself prove validate_motion true."""
    res = float(robot.resolution() if resolution is None else resolution)
    dim = robot.dimension()
    samples = [path_samples(np.asarray(p, np.float64).reshape(-1, dim), res) if len(p) else
               (np.zeros((0, dim), np.float32), np.zeros((0, 2), np.int64)) for p in paths]
    counts = [len(s[0]) for s in samples]
    values = robot.clearance_batch_multi(np.concatenate([s[0] for s in samples] + [np.zeros((0, dim), np.float32)]),
                                         environments, counts)
    out, lo = [], 0
    for (_, at), n in zip(samples, counts):
        v = np.asarray(values[lo:lo + n])
        lo += n
        if n == 0:
            out.append(PathClearance(float("inf"), float("inf"), None, None))
            continue
        ie, js = int(np.argmin(v[:, 0])), int(np.argmin(v[:, 1]))
        out.append(PathClearance(float(v[ie, 0]), float(v[js, 1]), (int(at[ie, 0]), int(at[ie, 1])),
                                 (int(at[js, 0]), int(at[js, 1]))))
    return out


@dataclass
class PushOut:
    """push_out's answer: the configurations ([n][dim] float32), their (env, self) clearances ([n][2] float32, bit for bit
    clearance_batch of those configurations), reached[i] = both clearances of configuration i are at least the margin,
    and the number of clearance_grad_batch calls made"""
    configurations: np.ndarray
    clearances: np.ndarray
    reached: np.ndarray
    calls: int


def push_out(robot, configurations, environment=None, margin=0.01, max_steps=32, max_step=0.05):
    """Moves configurations that are in contact, or closer to it than `margin` (metres), along the clearance gradient
    until both clearances reach `margin` -> PushOut.  A repair for grazing starts and goals, nothing more.

    Every round is ONE robot.clearance_grad_batch call for the configurations still below the margin (the input first,
    then after every step: at most max_steps + 1 calls).  With m the smaller of a configuration's two clearances and g
    that value's gradient, the step is g * (margin - m) / |g|^2 - the first-order step to m = margin - shortened to
    |step|_2 <= max_step (radians; metres for a prismatic joint), and the result is clipped to the joint bounds; host
    arithmetic in float32.  A configuration with g = 0 (a sphere centre inside a cuboid, coincident centres) or a NaN
    value (a non-finite joint) is left where it is and reported as not reached.  Per configuration the best min(env, self)
    seen and the configuration that gave it are kept and returned, so the returned min(env, self) is never below the
    input's, and the returned clearances were computed for exactly the returned configurations.

    There is NO line search, and NO collision checking of the motion between the input and the output: the gradient is
    that of the current witness, a step may bring another contact closer, and the straight line from input to output may
    pass through an obstacle.  Validate the result, and the motion if it matters."""
    dim = robot.dimension()
    q = np.array(configurations, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != dim:
        raise TypeError(f"expected [n][{dim}] configurations")
    if not (max_steps >= 0 and max_step > 0):
        raise ValueError("max_steps must be at least 0 and max_step positive")
    n = len(q)
    margin, max_step = np.float32(margin), np.float32(max_step)
    lower, upper = np.asarray(robot.lower_bounds(), np.float32), np.asarray(robot.upper_bounds(), np.float32)
    best_q, best_v = q.copy(), np.full((n, 2), np.nan, np.float32)
    best_m = np.full(n, -np.inf, np.float32)
    reached = np.zeros(n, bool)
    active = np.arange(n)
    calls = 0
    for step in range(int(max_steps) + 1):
        if len(active) == 0:
            break
        values, grad = robot.clearance_grad_batch(q[active], environment)[:2]
        values, grad = np.asarray(values, np.float32), np.asarray(grad, np.float32)
        calls += 1
        m = np.minimum(values[:, 0], values[:, 1])  # (NaN if either is)
        better = (m > best_m[active]) | (step == 0)
        at = active[better]
        best_q[at], best_v[at], best_m[at] = q[at], values[better], m[better]
        done = m >= margin
        reached[active[done]] = True
        g = np.where((values[:, 0] <= values[:, 1])[:, None], grad[:, 0], grad[:, 1])
        gg = (g * g).sum(axis=1, dtype=np.float32)
        go = ~done & ~np.isnan(m) & (gg > 0) & np.isfinite(gg)
        active, m, g, gg = active[go], m[go], g[go], gg[go]
        if step == int(max_steps) or len(active) == 0:
            break
        delta = g * ((margin - m) / gg)[:, None]
        length = np.sqrt((delta * delta).sum(axis=1, dtype=np.float32))
        delta *= np.where(length > max_step, max_step / np.maximum(length, np.float32(1e-30)), np.float32(1.0))[:, None]
        q[active] = np.clip(q[active] + delta.astype(np.float32), lower, upper)
    return PushOut(best_q, best_v, reached, calls)


OPTIMIZE_STATUS = ("ok", "no_valid", "nonfinite")  # VMV_OPT_*
OPTIMIZE_CONSTRAINED_STATUS = OPTIMIZE_STATUS + ("out_of_band",)  # optimize_multi_constrained: VMV_OPT_OUT_OF_BAND too


@dataclass
class OptimizeMultiSettings:
    """vmv_optimize_settings with the defaults of the float64 study: max_iterations, validate_every
    (iterations between two validated iterates), step, max_step (the largest joint change of one iteration over the whole
    path), min_change (a path ends once a step is smaller), the three weights, the two margins in metres, and
    max_waypoints (at most 1,024)"""
    max_iterations: int = 64
    validate_every: int = 8
    step: float = 1.0 / 40.0
    max_step: float = 0.1
    min_change: float = 1e-4
    smooth_weight: float = 1.0
    env_weight: float = 1.0
    self_weight: float = 1.0
    env_margin: float = 0.05
    self_margin: float = 0.01
    max_waypoints: int = 1024


@dataclass
class OptimizedPath:
    """optimize_multi's answer for one path: the waypoints, `status` (one of OPTIMIZE_STATUS), the iterations run, the
    iteration the returned iterate is from, the cost U of the input and of the returned iterate, and the smallest
    (env, self) clearance over the WAYPOINTS of the input and of the returned iterate"""
    path: list
    status: str
    iterations: int
    best_iteration: int
    cost_first: float
    cost: float
    clearance_first: tuple
    clearance: tuple


@dataclass
class ConstrainedOptimizedPath(OptimizedPath):
    """optimize_multi_constrained's answer for one path: an OptimizedPath whose `status` is one of
    OPTIMIZE_CONSTRAINED_STATUS, with `held`: the projections of the path's iterations that did not converge"""
    held: int = 0


def densify_path(path, resolution):
    """path_samples' rule with the duplicated inner waypoints dropped: segment (a, b) becomes a + (b - a) * k / m, k = 0..m,
    m = max(1, ceil(|b - a| * resolution)), in float64 cast to fp32 - except that every former waypoint is copied, not
    computed, so its bits are the input's.  -> float32 [n][dim]; a path of fewer than 2 waypoints comes back as it is."""
    p32 = np.asarray(path, np.float32)
    if p32.ndim != 2:
        raise TypeError("expected a [len][dim] path")
    if len(p32) < 2:
        return p32.copy()
    p = p32.astype(np.float64)
    out = [p32[:1]]
    for i in range(len(p) - 1):
        a, b = p[i], p[i + 1]
        m = max(1, int(np.ceil(np.sqrt(((b - a) ** 2).sum()) * resolution)))
        seg = (a[None, :] + (b - a)[None, :] * (np.arange(1, m + 1) / m)[:, None]).astype(np.float32)
        seg[-1] = p32[i + 1]
        out.append(seg)
    return np.ascontiguousarray(np.concatenate(out))


def optimize_multi(robot, paths, environments, settings=None, resolution=None):
    """Moves the inner waypoints of many independent paths away from contact, on the device: paths[p] ([len][dim]) in
    environments[p] (None = the empty environment) -> list[OptimizedPath].  A covariant gradient iteration (CHOMP's
    update without its velocity-projection terms) on the cost U = smoothness + hinge(env clearance; env_margin) +
    hinge(self clearance; self_margin) summed over the inner waypoints; include/vamp_mvt_amd.h (vmv_optimize_multi) and
    DESIGN §5l give every operation.  All paths advance in lockstep: ONE clearance_grad_batch_multi call and one step
    kernel per iteration, ONE validate_motion_batch_multi call per validated iterate (every validate_every iterations and
    the last).  What comes back per path is the cheapest validated iterate whose consecutive edges are all valid, so a
    valid input gives a valid output with cost <= cost_first; status "no_valid" and "nonfinite" return the input.

    resolution=None optimises the waypoints as given (the call never adds or removes one).  A number densifies every path
    first with densify_path (the former waypoints stay among the new ones); a densified path longer than
    settings.max_waypoints raises ValueError naming the path.

    What this is and is not: the clearance is that of the WAYPOINTS (clearance / clearance_first are minima over them,
    not over the motion between them); validity is validate_motion's on the consecutive edges; the gradient is the
    current witness's, so a step may bring another contact closer, and the plain iteration does not decrease U
    monotonically - which is why the best validated iterate is kept, not the last."""
    s = settings if settings is not None else OptimizeMultiSettings()
    pts = _optimize_inputs(robot, paths, s, resolution)
    return _optimize_results(robot.optimize_multi_raw(pts, environments, s), len(pts))


def _optimize_inputs(robot, paths, s, resolution):
    """the waypoint arrays of an optimiser call, densified where `resolution` is a number"""
    dim = robot.dimension()
    pts = []
    for k, p in enumerate(paths):
        a = _waypoints(p, dim)
        if resolution is not None:
            a = densify_path(a, float(resolution))
            if len(a) > int(s.max_waypoints):
                raise ValueError(f"path {k} has {len(a)} waypoints at resolution {resolution}: more than max_waypoints "
                                 f"({int(s.max_waypoints)})")
        pts.append(a)
    return pts


def _optimize_results(raw, n, constrained=False):
    """the raw dict of an optimiser call -> one OptimizedPath per path (ConstrainedOptimizedPath with `held`)"""
    off = raw["offsets"]
    out = []
    for p in range(n):
        fields = dict(path=[q.copy() for q in raw["points"][off[p]:off[p + 1]]],
                      status=OPTIMIZE_CONSTRAINED_STATUS[int(raw["status"][p])], iterations=int(raw["iterations"][p]),
                      best_iteration=int(raw["best_iteration"][p]), cost_first=float(raw["cost_first"][p]),
                      cost=float(raw["cost"][p]), clearance_first=tuple(float(v) for v in raw["clearance_first"][p]),
                      clearance=tuple(float(v) for v in raw["clearance"][p]))
        out.append(ConstrainedOptimizedPath(held=int(raw["held"][p]), **fields) if constrained else OptimizedPath(**fields))
    return out


def optimize_multi_constrained(robot, paths, environments, constraints, settings=None, constraint_settings=None, resolution=None):
    """`optimize_multi` inside the band of end-effector constraints (vmv_optimize_multi_constrained):
    constraints is one EEConstraint for all paths or one per path, constraint_settings a ConstraintSettings (None =
    defaults).  -> list[ConstrainedOptimizedPath]: optimize_multi's fields, `held`, and `status` "ok", "no_valid",
    "nonfinite" or "out_of_band".

    Three things change.  The input is looked at first: both ends of a path must pass `constraint_check_batch`, and every
    inner waypoint is replaced by its `project_batch` projection (unchanged where it is in the band already) - which is
    what repairs the points `resolution=` puts on a chord between two in-band waypoints; an end out of band or an inner
    waypoint that cannot be projected gives "out_of_band": the input comes back and nothing is asked.  Every new iterate is
    projected waypoint by waypoint; a waypoint whose projection does not converge keeps its previous value (`held` counts
    these).  And an iterate counts as valid only where every edge passes `validate_motion` AND
    `constraint_check_motion_batch`, so every "ok" result gets (True, True) from `validate_paths_constrained`.
    A constraint that restricts nothing gives `optimize_multi`'s results."""
    s = settings if settings is not None else OptimizeMultiSettings()
    pts = _optimize_inputs(robot, paths, s, resolution)
    return _optimize_results(robot.optimize_multi_constrained_raw(pts, environments, constraints, s, constraint_settings), len(pts), True)


def ik_goals(robot, targets, envs, settings=None, dedup=1e-2):
    """Goal sets for `rrtc_multi_goals` from end-effector targets: targets [P][4][4] frames as `robot.eefk_batch` returns
    them, target p to be reached in envs[p] (an Environment or None; a single environment is broadcast to all targets).
    -> (goal_sets, empty): goal_sets[p] a float32 [G_p][dim] array of collision-free IK solutions of target p, exactly what
    `rrtc_multi_goals` takes; empty = the indices of the targets left with no goal (G_p = 0), which `rrtc_multi_goals`
    refuses - leave those problems out.

    ONE `robot.ik_batch` call (Halton seeds, `settings` = IKSettings), ONE `robot.validate_batch_multi` call over all
    converged rows with target p's rows checked in envs[p], then on the host, per target in seed order, a solution within
    `dedup` (L-infinity, radians; metres for a prismatic joint) of an earlier kept one of the same target is dropped.  No
    checking of the way to a goal: that is the planner's part."""
    targets = np.asarray(targets, np.float32)
    if targets.ndim < 2 or int(np.prod(targets.shape[1:])) != 16:
        raise TypeError("expected targets as [P][4][4] (or [P][16]) frames")
    n = len(targets)
    environments = list(envs) if isinstance(envs, (list, tuple)) else [envs] * n
    if len(environments) != n:
        raise ValueError(f"{n} targets, but {len(environments)} environments")
    q, _, converged, _ = robot.ik_batch(targets, settings=settings)
    q, converged = np.asarray(q, np.float32), np.asarray(converged, bool)
    counts = converged.sum(axis=1).astype(np.int64)
    rows = q[converged]  # target by target, in seed order
    valid = np.asarray(robot.validate_batch_multi(rows, environments, counts), bool) if len(rows) else np.zeros(0, bool)
    goal_sets, at = [], 0
    for p in range(n):
        kept = []
        for g, ok in zip(rows[at:at + counts[p]], valid[at:at + counts[p]]):
            if ok and all(np.abs(g - h).max() > dedup for h in kept):
                kept.append(g)
        at += int(counts[p])
        goal_sets.append(np.array(kept, np.float32).reshape(len(kept), q.shape[2]))
    return goal_sets, [p for p in range(n) if len(goal_sets[p]) == 0]


def _per_problem(items, n, what):
    """a list or tuple of n, or anything else broadcast to the n problems"""
    items = list(items) if isinstance(items, (list, tuple)) else [items] * n
    if len(items) != n:
        raise ValueError(f"{n} problems, but {len(items)} {what}")
    return items


def validate_paths_constrained(robot, paths, envs, constraints, settings=None):
    """-> (valid bool[len(paths)], in_band bool[len(paths)]): path p's consecutive pairs against envs[p] (validate_paths)
    and against the band of constraints[p] (an EEConstraint; one is shared by all paths), in TWO batched calls:
    `robot.validate_motion_batch_multi` and `robot.constraint_check_motion_batch`, the latter with `settings` = a
    ConstraintSettings whose check_step spaces the band samples.  A path of fewer than 2 waypoints is valid and in band.
    What a shortcut, a smoothing or an optimisation returns is to be asked here: none of them knows the constraint."""
    dim = robot.dimension()
    pts = [np.asarray(p, np.float32).reshape(-1, dim) for p in paths]
    n = len(pts)
    environments = _per_problem(envs, n, "environments")
    records = _per_problem(constraints, n, "constraints")
    counts = [max(len(p) - 1, 0) for p in pts]
    empty = np.zeros((0, dim), np.float32)
    a, b = np.concatenate([p[:-1] for p in pts] + [empty]), np.concatenate([p[1:] for p in pts] + [empty])
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, bool)
    per_edge = [records[p] for p in range(n) for _ in range(counts[p])]
    ends = np.concatenate([[0], np.cumsum(counts)])

    def whole(ok):  # path p holds no failing edge (prefix counts: empty segments need no special case)
        bad = np.concatenate([[0], np.cumsum(~np.asarray(ok, bool))])
        return bad[ends[1:]] == bad[ends[:-1]]

    valid = whole(robot.validate_motion_batch_multi(a, b, environments, counts))
    return valid, whole(robot.constraint_check_motion_batch(a, b, per_edge, settings))


def project_goals(robot, goals, constraints, envs, settings=None):
    """Endpoints for planning under a constraint: goals[p] a [G_p][dim] set of configurations of problem p (a start is a
    set of one), projected into the band of constraints[p] (an EEConstraint; one is shared) and checked in envs[p] (an
    Environment or None; one is shared).  ONE `robot.project_batch` call over all rows and ONE `robot.validate_batch_multi`
    call over the converged ones; a row whose projection did not converge or collides is dropped.  -> per problem a
    float32 [G'_p][dim] array, in the rows' order - what `rrtc_multi_goals` takes as goal sets."""
    dim = robot.dimension()
    sets = [np.asarray(g, np.float32).reshape(-1, dim) for g in goals]
    n = len(sets)
    environments = _per_problem(envs, n, "environments")
    records = _per_problem(constraints, n, "constraints")
    if n == 0:
        return []
    rows = np.concatenate(sets)
    owner = np.repeat(np.arange(n), [len(g) for g in sets])
    if len(rows) == 0:
        return [np.zeros((0, dim), np.float32) for _ in sets]
    q, _, converged, _ = robot.project_batch(rows, [records[p] for p in owner], settings)
    q, converged = np.asarray(q, np.float32), np.asarray(converged, bool)
    counts = np.bincount(owner[converged], minlength=n).astype(np.int64)
    valid = np.asarray(robot.validate_batch_multi(q[converged], environments, counts), bool) if converged.any() else np.zeros(0, bool)
    keep = converged.copy()
    keep[converged] = valid
    return [q[keep & (owner == p)].reshape(-1, dim) for p in range(n)]


CARTESIAN_STATUS = ("complete", "ik_failed", "joint_jump", "collision", "invalid_start", "too_long", "non_finite")  # VMV_CART_*


@dataclass
class CartesianSettings:
    """vmv_cartesian_settings with its defaults: pos_step (m) and rot_step (rad) per segment of the line, max_iterations
    evaluations per waypoint, the tolerances and the Levenberg-Marquardt constants of IKSettings (a converged waypoint is
    a solution for ik_batch too), max_joint_step (rad: the largest joint change between two waypoints), max_waypoints (at
    most 1,024) and position_only.  The two steps and max_joint_step are choices, not measurements."""
    pos_step: float = 0.01
    rot_step: float = 0.05
    max_iterations: int = 16
    pos_tol: float = 1e-4
    rot_tol: float = 1e-3
    rot_weight: float = 0.25
    damping: float = 1e-2
    max_step: float = 0.5
    max_joint_step: float = 0.3
    max_waypoints: int = 1024
    position_only: bool = False


@dataclass
class CartesianPath:
    """cartesian_multi's answer for one problem: the waypoints kept (achieved + 1 of them, the first the start's bits),
    `status` (one of CARTESIAN_STATUS), the segments of the line, the segments kept, fraction = achieved / segments (0
    where there is no segment) and the evaluations the tracking made after each waypoint's first"""
    path: np.ndarray
    status: str
    segments: int
    achieved: int
    fraction: float
    evaluations: int

    @property
    def complete(self):
        return self.status == "complete"


def cartesian_multi(robot, starts, targets, environments=None, settings=None):
    """Straight-line end-effector motions for many problems in one call, on the device: problem p leads the end effector
    from the frame of starts[p] ([dim]) to targets[p] ([4][4] or [16], robot.eefk_batch's layout) along a straight line in
    position and a rotation about one fixed axis, in environments[p] (None = the empty environment; environments=None:
    kinematics only, nothing is validated) -> list[CartesianPath].  The line is cut into segments of at most pos_step and
    rot_step; each pose is tracked from the previous waypoint by ik_batch's iteration; the path stops where a pose is not
    reached ("ik_failed"), where a waypoint jumps by more than max_joint_step ("joint_jump"), or in front of the first
    edge validate_motion rejects ("collision").  include/vamp_mvt_amd.h (vmv_cartesian_multi) gives every step."""
    s = settings if settings is not None else CartesianSettings()
    raw = robot.cartesian_multi_raw(starts, targets, environments, s)
    # (plain lists: a thousand results cost a third of the call when every field is converted from its numpy scalar)
    off, points = raw["offsets"].tolist(), raw["points"]
    status, segments = raw["status"].tolist(), raw["segments"].tolist()
    achieved, evaluations = raw["achieved"].tolist(), raw["evaluations"].tolist()
    return [CartesianPath(path=points[off[p]:off[p + 1]].copy(), status=CARTESIAN_STATUS[status[p]], segments=segments[p],
                          achieved=achieved[p], fraction=achieved[p] / segments[p] if segments[p] else 0.0,
                          evaluations=evaluations[p]) for p in range(len(status))]


def approach_poses(targets, distance, axis=(0, 0, 1)):
    """The pre-poses of straight approaches: target . translate(-distance * axis), the axis in the tool frame (its length
    is normalised) -> float32 [P][4][4]"""
    t = np.asarray(targets, np.float64)
    if t.ndim < 2 or int(np.prod(t.shape[1:])) != 16:
        raise TypeError("expected targets as [P][4][4] (or [P][16]) frames")
    t = t.reshape(-1, 4, 4)
    a = np.asarray(axis, np.float64)
    if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
        raise ValueError("axis must be a finite, non-zero 3-vector")
    d = float(distance)
    if not (np.isfinite(d) and d > 0):
        raise ValueError("distance must be positive and finite")
    pre = t.copy()
    pre[:, :3, 3] = t[:, :3, 3] - d * (t[:, :3, :3] @ (a / np.linalg.norm(a)))
    return pre.astype(np.float32)


@dataclass
class Approach:
    """approach_multi's answer for one target: goals [G][dim], the pre-pose configurations whose straight approach is
    complete (what rrtc_multi_goals takes), and paths, one float32 [len][dim] approach path per goal, from the goal to
    the target"""
    goals: np.ndarray
    paths: list


def approach_multi(robot, targets, environments, distance, axis=(0, 0, 1), ik_settings=None, settings=None):
    """Straight tool-frame approaches to many targets: per target the pre-pose is approach_poses' (the target moved back
    by `distance` along `axis` in the tool frame); ONE ik_goals call over the pre-poses (ik_settings) gives each target's
    collision-free pre-pose configurations, ONE cartesian_multi call leads every one of them to its target (settings),
    and a goal is kept if its approach is complete.  environments: one per target, or a single Environment / None for
    all.  -> list[Approach], one per target; Approach.goals goes straight into rrtc_multi_goals (leave out the targets
    whose goals are empty), Approach.paths are the motions that follow the plan.  A retreat is an approach reversed."""
    targets = np.asarray(targets, np.float32)
    pre = approach_poses(targets, distance, axis)
    targets = targets.reshape(-1, 4, 4)
    n = len(targets)
    envs = list(environments) if isinstance(environments, (list, tuple)) else [environments] * n
    if len(envs) != n:
        raise ValueError(f"{n} targets, but {len(envs)} environments")
    goal_sets, _ = ik_goals(robot, pre, envs, settings=ik_settings)
    counts = [len(g) for g in goal_sets]
    dim = robot.dimension()
    starts = np.concatenate(goal_sets + [np.zeros((0, dim), np.float32)])
    which = np.repeat(np.arange(n), counts)
    lines = cartesian_multi(robot, starts, targets[which], [envs[p] for p in which], settings) if len(starts) else []
    out = [Approach(np.zeros((0, dim), np.float32), []) for _ in range(n)]
    for p, line in zip(which, lines):
        if line.complete:
            out[p].goals = np.concatenate([out[p].goals, line.path[:1]])
            out[p].paths.append(line.path)
    return out


RETIME_STATUS = ("complete", "collision", "too_long", "non_finite", "stalled")  # VMV_RETIME_*


@dataclass
class RetimeSettings:
    """vmv_retime_settings with its defaults: blend (the largest blend half-length at a corner, in joint-space distance),
    grid_step (the largest interval of the velocity profile's grid), dt (the sampling period, s), max_grid (intervals per
    path, at most 4,096), max_samples and stop_at_waypoints (no blends: the trajectory rests at every waypoint and stays on
    the polyline).  blend, grid_step and dt are choices, not measurements."""
    blend: float = 0.1
    grid_step: float = 0.02
    dt: float = 0.01
    max_grid: int = 4096
    max_samples: int = 65536
    stop_at_waypoints: bool = False


@dataclass
class Trajectory:
    """retime_multi's answer for one path: times [S], positions / velocities / accelerations [S][dim] sampled every dt
    (the last sample at `duration`), `status` (one of RETIME_STATUS), the intervals of the profile's grid and
    first_invalid, the first sample pair validate_motion rejects (-1: none)"""
    times: np.ndarray
    positions: np.ndarray
    velocities: np.ndarray
    accelerations: np.ndarray
    duration: float
    status: str
    intervals: int
    first_invalid: int

    @property
    def complete(self):
        return self.status == "complete"


def retime_multi(robot, paths, vel_limits, acc_limits, environments=None, settings=None):
    """Time-optimal trajectories along many paths in one call, on the device: path p ([len][dim] waypoints) becomes a C1
    path of straight pieces with parabolic blends at the corners, traversed from rest to rest as fast as |qdot_j| <=
    vel_limits[j] and |qddot_j| <= acc_limits[j] allow, and sampled every dt -> list[Trajectory].  environments[p] (None =
    the empty environment) is where the sampled trajectory is validated, because the blends leave the polyline;
    environments=None: nothing is validated.  A "collision" comes with first_invalid and the whole trajectory: lower
    `blend` or set stop_at_waypoints.  No jerk limits, no torque limits, no non-zero end velocities; velocity is bounded
    at the grid points and acceleration everywhere on the path.  include/vamp_mvt_amd.h (vmv_retime_multi) gives every
    step."""
    s = settings if settings is not None else RetimeSettings()
    raw = robot.retime_multi_raw(paths, vel_limits, acc_limits, environments, s)
    off = raw["offsets"].tolist()
    status, intervals = raw["status"].tolist(), raw["intervals"].tolist()
    duration, bad = raw["duration"].tolist(), raw["first_invalid"].tolist()
    return [Trajectory(times=raw["times"][off[p]:off[p + 1]].copy(), positions=raw["positions"][off[p]:off[p + 1]].copy(),
                       velocities=raw["velocities"][off[p]:off[p + 1]].copy(),
                       accelerations=raw["accelerations"][off[p]:off[p + 1]].copy(), duration=duration[p],
                       status=RETIME_STATUS[status[p]], intervals=intervals[p],
                       first_invalid=-1 if bad[p] == 0xffffffff else bad[p]) for p in range(len(status))]


RETIME_CONSTRAINED_STATUS = RETIME_STATUS + ("out_of_band",)  # VMV_RETIME_*, with VMV_RETIME_OUT_OF_BAND


@dataclass
class RetimeConstrainedSettings(RetimeSettings):
    """vmv_retime_constrained_settings with its defaults: RetimeSettings' fields, blend_halvings (H: how often a corner's
    blend is halved before the corner becomes a stop, at most 8) and max_rounds (after which an unfinished path ends with
    its last round's samples).  3 and 8 are choices, not measurements."""
    blend_halvings: int = 3
    max_rounds: int = 8


@dataclass
class RepairedTrajectory(Trajectory):
    """retime_multi_constrained's answer for one path: a Trajectory (`status` one of RETIME_CONSTRAINED_STATUS) with the
    rounds it took, levels (one per input waypoint: how often that corner's blend was halved, blend_halvings + 1 = a stop,
    0 for the ends and dropped duplicates), repaired (corners with a level above 0) and stops (corners that became stops)"""
    rounds: int = 0
    levels: np.ndarray = None
    repaired: int = 0
    stops: int = 0


def retime_multi_constrained(robot, paths, vel_limits, acc_limits, environments=None, constraints=None, settings=None,
                             constraint_settings=None):
    """`retime_multi` whose blends stay valid and inside the band (vmv_retime_multi_constrained): every
    corner carries a level, 0 at first; a level halves the corner's blend, and above blend_halvings the corner is a stop.
    Per round every unfinished path is set up with its levels, profiled and sampled as `retime_multi` does, every
    consecutive sample pair is put to validate_motion in environments[p] and to the band test of the path's constraint
    (`constraint_check_motion_batch`'s answer; constraints: None, one EEConstraint for all paths or one per path), and
    every corner whose blend a failing pair touches goes up one level.  -> list[RepairedTrajectory].

    "complete" means every returned sample pair passed both tests.  A failing pair that touches no blend - it lies on the
    polyline itself - ends the path at once, "collision" where validate_motion refused it and "out_of_band" otherwise, as
    does round max_rounds.  Where `retime_multi` is complete and no constraint restricts, the result is `retime_multi`'s
    byte for byte, in one round.  Corners are repaired, edges are not; a blend at a lower level is not proven faster than a
    stop (tools/bench_retime_constrained.py measures it); `aorrtc_multi` does not know the constraint,
    `aorrtc_multi_constrained` does."""
    s = settings if settings is not None else RetimeConstrainedSettings()
    raw = robot.retime_multi_constrained_raw(paths, vel_limits, acc_limits, environments, constraints, s, constraint_settings)
    off, lev = raw["offsets"].tolist(), raw["level_offsets"].tolist()
    status, intervals = raw["status"].tolist(), raw["intervals"].tolist()
    duration, bad = raw["duration"].tolist(), raw["first_invalid"].tolist()
    rounds, repaired, stops = raw["rounds"].tolist(), raw["repaired"].tolist(), raw["stops"].tolist()
    return [RepairedTrajectory(times=raw["times"][off[p]:off[p + 1]].copy(), positions=raw["positions"][off[p]:off[p + 1]].copy(),
                               velocities=raw["velocities"][off[p]:off[p + 1]].copy(),
                               accelerations=raw["accelerations"][off[p]:off[p + 1]].copy(), duration=duration[p],
                               status=RETIME_CONSTRAINED_STATUS[status[p]], intervals=intervals[p],
                               first_invalid=-1 if bad[p] == 0xffffffff else bad[p], rounds=rounds[p],
                               levels=raw["levels"][lev[p]:lev[p + 1]].copy(), repaired=repaired[p], stops=stops[p])
            for p in range(len(status))]


@dataclass
class Roadmap:
    vertices: np.ndarray  # [n][dim] valid samples
    edges: np.ndarray     # [m][2] index pairs (valid motions)
    candidate_edges: int = 0
    sampled: int = 0

    def neighbours(self):
        adj = [[] for _ in range(len(self.vertices))]
        for a, b in self.edges:
            w = float(np.linalg.norm(self.vertices[a] - self.vertices[b]))
            adj[a].append((b, w))
            adj[b].append((a, w))
        return adj

    def shortest_path(self, src: int, dst: int):
        """A* with the straight-line heuristic (planning/roadmap.hh style search on the host)."""
        adj = self.neighbours()
        h = lambda i: float(np.linalg.norm(self.vertices[i] - self.vertices[dst]))
        best = {src: 0.0}
        prev = {}
        heap = [(h(src), src)]
        while heap:
            _, u = heapq.heappop(heap)
            if u == dst:
                out = [u]
                while u in prev:
                    u = prev[u]
                    out.append(u)
                return out[::-1]
            for v, w in adj[u]:
                g = best[u] + w
                if g < best.get(v, np.inf):
                    best[v], prev[v] = g, u
                    heapq.heappush(heap, (g + h(v), v))
        return None


def build_roadmap(robot, environment, n_samples=2048, k=8, sampler: Halton | None = None, extra_vertices=()):
    """Batched PRM construction: samples -> validate_batch; k-nearest candidate edges -> validate_motion_batch."""
    rng = sampler or Halton(robot)
    samples = rng.batch(n_samples)
    if len(extra_vertices):
        samples = np.vstack([np.asarray(extra_vertices, np.float32), samples])
    keep = robot.validate_batch(samples, environment)
    v = samples[keep]
    n = len(v)
    if n < 2:
        return Roadmap(v, np.zeros((0, 2), np.int64), 0, len(samples))
    d = np.linalg.norm(v[:, None, :] - v[None, :, :], axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1)[:, : min(k, n - 1)]
    pairs = {(min(i, int(j)), max(i, int(j))) for i in range(n) for j in nn[i]}
    cand = np.array(sorted(pairs), np.int64)
    ok = robot.validate_motion_batch(v[cand[:, 0]], v[cand[:, 1]], environment)
    return Roadmap(v, cand[ok], len(cand), len(samples))


@dataclass
class FCITSettings:
    """the knobs of planning/fcit.hh that matter for a batch driver"""
    batch_size: int = 1000
    max_samples: int = 20000
    max_iterations: int = 64
    optimize: bool = False  # keep adding batches after the first solution (prune with the current cost)


def fcit(robot, start, goal, environment, settings: FCITSettings | None = None, sampler: Halton | None = None):
    """Batch form of the FCIT* loop (planning/fcit.hh:137-349): sample a batch, keep the valid samples
    (`validate_batch`), search the COMPLETE graph over all samples with A* (straight-line heuristic) treating
    unchecked edges as free, then check the unknown edges of the candidate path together (`validate_motion_batch`),
    delete the invalid ones and search again; add another batch when no path remains.  With `optimize`, later
    batches only keep samples inside the current solution's ellipse (the informed set).  Every collision question
    goes through the batched API; the reference asks the same questions one edge at a time (fcit.hh:238,333)."""
    s = settings or FCITSettings()
    rng = sampler or Halton(robot)
    start, goal = np.asarray(start, np.float32), np.asarray(goal, np.float32)
    res = PlanningResult()
    if not robot.validate_batch(np.stack([start, goal]), environment).all():
        return res
    verts = np.stack([start, goal])
    state = {}  # (i, j), i < j -> True valid / False invalid; absent = unchecked
    best_cost, best_path = np.inf, None
    drawn = checked = 0

    def key(a, b):
        return (a, b) if a < b else (b, a)

    def astar():
        n = len(verts)
        h = np.linalg.norm(verts - verts[1], axis=1)
        g = np.full(n, np.inf)
        g[0] = 0.0
        parent = np.full(n, -1)
        closed = np.zeros(n, bool)
        pq = [(float(h[0]), 0)]
        while pq:
            _, u = heapq.heappop(pq)
            if closed[u]:
                continue
            closed[u] = True
            if u == 1:
                path = [1]
                while path[-1] != 0:
                    path.append(int(parent[path[-1]]))
                return path[::-1], float(g[1])
            d = np.linalg.norm(verts - verts[u], axis=1)
            cand = np.flatnonzero(~closed & (g[u] + d + h < best_cost))
            for v in cand:
                if state.get(key(u, int(v))) is False:
                    continue
                ng = g[u] + d[v]
                if ng < g[v]:
                    g[v], parent[v] = ng, u
                    heapq.heappush(pq, (float(ng + h[v]), int(v)))
        return None, np.inf

    for it in range(s.max_iterations):
        res.iterations = it + 1
        while True:
            path, cost = astar()
            if path is None:
                break
            unknown = [key(a, b) for a, b in zip(path[:-1], path[1:]) if key(a, b) not in state]
            if not unknown:
                if cost < best_cost:
                    best_cost, best_path = cost, path
                break
            e = np.array(unknown, np.int64)
            ok = robot.validate_motion_batch(verts[e[:, 0]], verts[e[:, 1]], environment)
            checked += len(e)
            for k, v in zip(unknown, ok):
                state[k] = bool(v)
        if best_path is not None and not s.optimize:
            break
        if drawn >= s.max_samples:
            break
        batch = rng.batch(s.batch_size)
        drawn += len(batch)
        keep = robot.validate_batch(batch, environment)
        new = batch[keep]
        if np.isfinite(best_cost):  # informed set: |x - start| + |x - goal| < current cost
            new = new[np.linalg.norm(new - start, axis=1) + np.linalg.norm(new - goal, axis=1) < best_cost]
        verts = np.vstack([verts, new])
    if best_path is not None:
        res.path = verts[best_path]
        res.cost = best_cost
    res.size = len(verts)
    res.edges_checked = checked
    res.samples_drawn = drawn
    return res
