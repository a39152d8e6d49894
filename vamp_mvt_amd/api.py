"""The reference's planner-facing Python names on top of the batched GPU path.

`import vamp_mvt_amd as vamp` then gives what scripts/sphere_cage_example.py:45-67 uses, under the reference's names
and signatures (bindings/robot_helper.hh:326-597, bindings/settings.cc:13-117, src/vamp/__init__.py:69-139,188-228):

    vamp.configure_robot_and_planner_with_kwargs(robot, planner, **kwargs) -> (module, planner_func, settings, simp_settings)
    vamp.<robot>.halton() -> sampler with next() / skip(n) / reset()          (random/halton.hh, bit-exact)
    vamp.<robot>.rrtc / prm / fcit(start, goal | goals, environment, settings, rng) -> PlanningResult
    vamp.<robot>.roadmap(start, goal, environment, settings, rng) -> Roadmap
    vamp.<robot>.simplify(path, environment, settings, rng) -> PlanningResult
    vamp.<robot>.Path, PlanningResult(solved, path, nanoseconds, iterations, size), space_measure()
    vamp.RRTCSettings, PRMSettings, PRMNeighborParams, FCITSettings, FCITNeighborParams, SimplifySettings, ...
    vamp.results_to_dict(planning_result, simplification_result)

What is NOT the reference's: the planners themselves.  The reference's are serial C++ templates (rrtc.hh, prm.hh,
fcit.hh, simplify.hh) that ask one validity question at a time; these are host-side loops (vamp_mvt_amd/planning.py)
that ask the same kinds of questions in batches of the GPU path, so iteration counts, tree sizes and path costs differ
from the reference's (no reference test pins those).  `simplify` is a greedy shortcutting pass (every shortcut is a
`validate_motion` question answered on the GPU); `<robot>.simplify_multi` runs the reference's SHORTCUT and BSPLINE
routines themselves, for many paths at once on the device (planning.simplify_multi).  `xorshift()` raises, as the reference's does where SIMDxorshift is unavailable (robot_helper.hh:406-409)."""
from __future__ import annotations

import logging
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import planning

DEFAULT_ITERATIONS = 1000000  # src/vamp/constants.py:1
ROBOT_RRT_RANGES = {"sphere": 1, "ur5": 1.5, "panda": 1.0, "fetch": 1.0, "baxter": 0.5}  # constants.py:3-9
# Robot::space_measure() (robots/panda.hh:111-114, ur5.hh:105-108, fetch.hh:117-120, baxter.hh:153-156): model constants
SPACE_MEASURE = {"panda": 57376.4026747593, "ur5": 61528.90796697732, "fetch": 16384.87636281249,
                 "baxter": 590532810.7756369}


# --------------------------------------------------------------------------------------------- settings (settings.cc)
@dataclass
class RRTCSettings:
    """planning/rrtc_settings.hh (dynamic_domain / radius / alpha / min_radius / start_tree_first are accepted and kept;
    the batch driver uses range, balance, tree_ratio, max_iterations, max_samples)"""
    range: float = 2.0
    dynamic_domain: bool = True
    radius: float = 4.0
    alpha: float = 0.0001
    min_radius: float = 1.0
    balance: bool = True
    tree_ratio: float = 1.0
    max_iterations: int = 100000
    max_samples: int = 100000
    start_tree_first: bool = True


def _unit_ball_measure(dim):
    return math.pow(math.sqrt(math.pi), dim) / math.gamma(dim / 2.0 + 1.0)  # planning/roadmap.hh:18-22


class PRMNeighborParams:
    """vp::PRMStarNeighborParams (planning/roadmap.hh:44-81)"""

    def __init__(self, dim, space_measure):
        self.dim, self.space_measure, self.gamma_scale = int(dim), float(space_measure), 2.0

    def max_neighbors(self, num_states):
        return int(math.ceil((math.e + math.e / self.dim) * math.log(float(max(num_states, 1)))))

    def neighbor_radius(self, num_states):
        inv = 1.0 / self.dim
        ratio = self.space_measure / _unit_ball_measure(self.dim)
        c = 2.0 * math.pow(1.0 + inv, inv) * math.pow(ratio, inv)
        n = max(num_states, 2)
        return float(np.float32(self.gamma_scale * c * math.pow(math.log(n) / n, inv)))


class FCITNeighborParams(PRMNeighborParams):
    """vp::FCITStarNeighborParams (roadmap.hh:83-111): all neighbours, infinite radius"""

    def max_neighbors(self, num_states):
        return 2 ** 63 - 1

    def neighbor_radius(self, num_states):
        return float("inf")


class PRMSettings:
    """vp::RoadmapSettings<PRMStarNeighborParams> (settings.cc:54-61)"""

    def __init__(self, neighbor_params):
        self.neighbor_params = neighbor_params
        self.max_iterations = 100000
        self.max_samples = 100000

    def max_neighbors(self, num_states):
        return self.neighbor_params.max_neighbors(num_states)

    def neighbor_radius(self, num_states):
        return self.neighbor_params.neighbor_radius(num_states)


class FCITSettings(PRMSettings):
    """vp::RoadmapSettings<FCITStarNeighborParams> (settings.cc:72-81)"""

    def __init__(self, neighbor_params):
        super().__init__(neighbor_params)
        self.batch_size = 1000
        self.optimize = False


class SimplifyRoutine:
    BSPLINE, REDUCE, SHORTCUT, PERTURB = "BSPLINE", "REDUCE", "SHORTCUT", "PERTURB"


@dataclass
class BSplineSettings:
    max_steps: int = 5
    min_change: float = 0.05
    midpoint_interpolation: float = 0.5


@dataclass
class ReduceSettings:
    max_steps: int = 25
    max_empty_steps: int = 10
    range_ratio: float = 0.33


@dataclass
class ShortcutSettings:
    pass


@dataclass
class PerturbSettings:
    max_steps: int = 25
    max_empty_steps: int = 10
    perturbation_attempts: int = 5
    range_ratio: float = 0.1


@dataclass
class SimplifySettings:
    """vp::SimplifySettings (settings.cc:109-117); `simplify` runs a greedy shortcut pass only, `simplify_multi` the
    SHORTCUT and BSPLINE routines as listed in `operations`"""
    max_iterations: int = 4
    interpolate: int = 0
    operations: list = field(default_factory=lambda: [SimplifyRoutine.SHORTCUT, SimplifyRoutine.BSPLINE])
    reduce: ReduceSettings = field(default_factory=ReduceSettings)
    shortcut: ShortcutSettings = field(default_factory=ShortcutSettings)
    perturb: PerturbSettings = field(default_factory=PerturbSettings)
    bspline: BSplineSettings = field(default_factory=BSplineSettings)


@dataclass
class AORRTCSettings:
    """planning/aorrtc_settings.hh (settings.cc); `<robot>.aorrtc` and `<robot>.aorrtc_multi` run planning.aorrtc_multi:
    max_samples is the node pool every problem owns on the device, max_cost_bound_resamples above 64 is clamped to 64,
    and anytime=True, use_phs=False and rrtc.dynamic_domain=True raise at the call"""
    rrtc: RRTCSettings = field(default_factory=lambda: RRTCSettings(dynamic_domain=False))
    simplify: SimplifySettings = field(default_factory=SimplifySettings)
    optimize: bool = True
    cost_bound_resample: bool = True
    simplify_intermediate: bool = True
    use_phs: bool = True
    anytime: bool = False
    max_iterations: int = 100000
    max_internal_iterations: int = 100000
    max_samples: int = 100000
    max_cost_bound_resamples: int = 1000


# --------------------------------------------------------------------------------------------- per-robot objects
def _cfg(robot, q):
    a = np.ascontiguousarray(q, dtype=np.float32)
    if a.shape != (robot.dimension(),):
        raise TypeError(f"expected a configuration of {robot.dimension()} floats")
    return a


def make_path_class(robot):
    class Path(list):
        """vamp.<robot>.Path (planning/plan.hh:10-169): list of configurations"""

        def append(self, c):
            super().append(_cfg(robot, c))

        def insert(self, i, c):
            super().insert(i, _cfg(robot, c))

        def __setitem__(self, i, c):
            if isinstance(i, slice):
                super().__setitem__(i, [_cfg(robot, q) for q in c])
            else:
                super().__setitem__(i, _cfg(robot, c))

        def cost(self):
            if len(self) < 2:
                return float("inf")
            p = self.numpy()
            return float(np.float32(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1)).sum()))

        def subdivide(self):
            out = []
            for a, b in zip(self[:-1], self[1:]):
                out += [a, (a + (b - a) * np.float32(0.5)).astype(np.float32)]
            out.append(self[-1])
            self[:] = out

        def interpolate_to_resolution(self, resolution):
            if len(self) < 2:
                return
            out = []
            for a, b in zip(list(self[:-1]), list(self[1:])):
                seg = float(np.linalg.norm(b - a))
                n = int(seg * float(resolution))
                out.append(a)
                if seg < 1.0 / float(resolution):
                    continue
                out += [(a + (b - a) * np.float32(i / n)).astype(np.float32) for i in range(1, n)]
            out.append(self[-1])
            self[:] = out

        def interpolate_to_n_states(self, n):
            if len(self) < 2 or n < len(self):
                return
            p = self.numpy()
            seg = np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1))
            if seg.sum() < np.finfo(np.float32).eps:
                return
            t = np.concatenate([[0.0], np.cumsum(seg)]) / seg.sum()
            s = np.linspace(0.0, 1.0, n)
            out = np.stack([np.interp(s, t, p[:, j]) for j in range(p.shape[1])], 1).astype(np.float32)
            self[:] = list(out)

        def validate(self, environment):
            """every consecutive pair is a valid motion (plan.hh:155-168): one batch on the GPU"""
            return planning.validate_path(robot, list(self), environment)

        def numpy(self):
            return np.stack(self).astype(np.float32) if len(self) else np.zeros((0, robot.dimension()), np.float32)

    Path.__qualname__ = f"{robot._name}.Path"
    return Path


class PlanningResult:
    """vamp.<robot>.PlanningResult (robot_helper.hh:486-498, planning/plan.hh:171-179)"""

    def __init__(self, path=None, nanoseconds=0, iterations=0, size=None, cost=0.0):
        self.path = path if path is not None else []
        self.nanoseconds, self.iterations, self.size, self.cost = int(nanoseconds), int(iterations), list(size or []), cost

    @property
    def solved(self):
        return len(self.path) >= 2


class Roadmap:
    """vamp.<robot>.Roadmap (robot_helper.hh:500-517)"""

    def __init__(self, vertices, edges, nanoseconds, iterations):
        self.vertices, self.edges, self.nanoseconds, self.iterations = vertices, edges, nanoseconds, iterations

    def __len__(self):
        return len(self.vertices)

    def __getitem__(self, i):
        return self.vertices[i]


def _goals(robot, goal):
    g = np.asarray(goal, np.float32)
    return [_cfg(robot, g)] if g.ndim == 1 else [_cfg(robot, x) for x in g]


def install(robot):
    """adds the reference's per-robot planner names to a vamp_mvt_amd robot module"""
    Path = make_path_class(robot)
    robot.Path, robot.PlanningResult, robot.Roadmap = Path, PlanningResult, Roadmap
    robot.space_measure = lambda: float(np.float32(SPACE_MEASURE[robot._name]))
    robot.halton = lambda: planning.Halton(robot)

    def xorshift():
        raise RuntimeError("XORShift is not supported by this build (the reference needs SIMDxorshift for it)")

    robot.xorshift = xorshift

    def as_result(res, t0):
        path = Path()
        for q in res.path:
            path.append(q)
        size = res.size if isinstance(res.size, (list, tuple)) else [int(res.size)]
        return PlanningResult(path, time.perf_counter_ns() - t0, res.iterations, size,
                              path.cost() if len(path) >= 2 else 0.0)

    def rrtc(start, goal, environment, settings, rng):
        t0 = time.perf_counter_ns()
        s = planning.RRTCSettings(range=float(settings.range), balance=bool(settings.balance),
                                  tree_ratio=float(settings.tree_ratio), max_iterations=int(settings.max_iterations),
                                  max_samples=int(settings.max_samples))
        return as_result(planning.rrtc(robot, _cfg(robot, start), _goals(robot, goal), environment, s, rng), t0)

    def rrtc_multi(starts, goals, environments, settings, skips=None):
        """planning.rrtc_multi with this robot: many RRT-Connect problems in lockstep on the device ->
        list[PlanningResult] (each with `status`; nanoseconds is the whole call's time divided by the problems).  A
        planning.RRTCMultiSettings is taken as it is, its dynamic_domain and start_tree_first included.  A
        reference-shaped RRTCSettings is reduced to range, balance, tree_ratio, max_iterations and max_samples: its
        dynamic_domain, radius, alpha, min_radius and start_tree_first are NOT used."""
        t0 = time.perf_counter_ns()
        return timed_results(planning.rrtc_multi(robot, starts, goals, environments, multi_settings(settings), skips), t0)

    def multi_settings(settings):
        if isinstance(settings, planning.RRTCMultiSettings):
            return settings
        return planning.RRTCMultiSettings(range=float(settings.range), balance=bool(settings.balance),
                                          tree_ratio=float(settings.tree_ratio), max_iterations=int(settings.max_iterations),
                                          max_samples=int(settings.max_samples), check_every=int(getattr(settings, "check_every", 0)))

    def timed_results(results, t0):
        each = (time.perf_counter_ns() - t0) // max(len(results), 1)
        out = []
        for r in results:
            res = as_result(r, t0)
            res.nanoseconds, res.status, res.goal_index = each, r.status, r.goal_index
            out.append(res)
        return out

    def rrtc_multi_goals(starts, goal_sets, environments, settings, skips=None):
        """planning.rrtc_multi_goals with this robot: rrtc_multi with a [G_p][dim] set of goals per problem ->
        list[PlanningResult] (each with `status` and `goal_index`).  The settings are taken as rrtc_multi takes them."""
        t0 = time.perf_counter_ns()
        return timed_results(planning.rrtc_multi_goals(robot, starts, goal_sets, environments, multi_settings(settings), skips), t0)

    def rrtc_multi_constrained(starts, goal_sets, environments, constraints, settings, constraint_settings=None, skips=None,
                               max_stretch=2.0):
        """planning.rrtc_multi_constrained with this robot: rrtc_multi_goals under end-effector constraints ->
        list[PlanningResult] (each with `status` and `goal_index`).  The settings are taken as rrtc_multi takes them."""
        t0 = time.perf_counter_ns()
        return timed_results(planning.rrtc_multi_constrained(robot, starts, goal_sets, environments, constraints,
                                                             multi_settings(settings), constraint_settings, skips, max_stretch), t0)

    def aorrtc_multi(starts, goals, environments, settings, skips=None):
        """planning.aorrtc_multi with this robot and the reference-shaped AORRTCSettings -> list[PlanningResult] (each
        with `status`, `first_cost`, `searches`, `improvements`; nanoseconds is the whole call's time divided by the
        problems).  A planning.AORRTCMultiSettings is taken as it is."""
        t0 = time.perf_counter_ns()
        return aorrtc_results(planning.aorrtc_multi(robot, starts, goals, environments, aorrtc_settings(settings), skips), t0)

    def aorrtc_multi_constrained(starts, goals, environments, constraints, settings, constraint_settings=None, skips=None,
                                 max_stretch=2.0):
        """planning.aorrtc_multi_constrained with this robot: aorrtc_multi under end-effector constraints ->
        list[PlanningResult] as aorrtc_multi's, each with `band_refused` too.  The settings are taken as aorrtc_multi takes
        them."""
        t0 = time.perf_counter_ns()
        return aorrtc_results(planning.aorrtc_multi_constrained(robot, starts, goals, environments, constraints,
                                                                aorrtc_settings(settings), constraint_settings, skips, max_stretch), t0)

    def aorrtc_settings(settings):
        """planning.AORRTCMultiSettings from the reference-shaped AORRTCSettings; one of the former is taken as it is"""
        if isinstance(settings, planning.AORRTCMultiSettings):
            s = settings
        else:
            if bool(getattr(settings, "anytime", False)):
                raise NotImplementedError("anytime=True (Anytime RRT-Connect) is not part of aorrtc_multi")
            if not bool(getattr(settings, "use_phs", True)):
                raise NotImplementedError("use_phs=False is not part of aorrtc_multi: rejection from the Halton box finds nothing")
            if bool(getattr(settings.rrtc, "dynamic_domain", False)):
                raise NotImplementedError("rrtc.dynamic_domain=True is not part of aorrtc_multi")
            s = planning.AORRTCMultiSettings(
                range=float(settings.rrtc.range), balance=bool(settings.rrtc.balance), tree_ratio=float(settings.rrtc.tree_ratio),
                optimize=bool(settings.optimize), cost_bound_resample=bool(settings.cost_bound_resample),
                simplify_intermediate=bool(settings.simplify_intermediate), max_iterations=int(settings.max_iterations),
                max_internal_iterations=int(settings.max_internal_iterations), max_samples=int(settings.max_samples),
                max_cost_bound_resamples=min(int(settings.max_cost_bound_resamples), 64),
                max_searches=int(getattr(settings, "max_searches", 0)), simplify=settings.simplify,
                check_every=int(getattr(settings, "check_every", 0)))
        return s

    def aorrtc_results(results, t0):
        each = (time.perf_counter_ns() - t0) // max(len(results), 1)
        out = []
        for r in results:
            path = Path()
            for q in r.path:
                path.append(q)
            res = PlanningResult(path, each, r.iterations, r.size, r.cost)
            res.status, res.first_cost, res.searches, res.improvements = r.status, r.first_cost, r.searches, r.improvements
            if hasattr(r, "band_refused"):
                res.band_refused = r.band_refused
            out.append(res)
        return out

    def aorrtc(start, goal, environment, settings, rng=None):
        """one problem of aorrtc_multi (one goal; `rng` is not used: the first stage samples the Halton sequence from its
        start, the searches their own stream)"""
        return aorrtc_multi(_cfg(robot, start)[None], _cfg(robot, goal)[None], [environment], settings)[0]

    def fcit(start, goal, environment, settings, rng):
        t0 = time.perf_counter_ns()
        s = planning.FCITSettings(batch_size=int(settings.batch_size), max_samples=int(settings.max_samples),
                                  max_iterations=min(int(settings.max_iterations), 4096), optimize=bool(settings.optimize))
        best = None
        for g in _goals(robot, goal):  # the reference's multi-goal form searches towards every goal
            r = planning.fcit(robot, _cfg(robot, start), g, environment, s, rng)
            if r.solved and (best is None or r.cost < best.cost):
                best = r
        return as_result(best if best is not None else planning.PlanningResult(), t0)

    def roadmap(start, goal, environment, settings, rng, n_samples=2048):
        t0 = time.perf_counter_ns()
        goals = _goals(robot, goal)
        n = int(min(settings.max_samples, n_samples))
        k = max(1, min(settings.max_neighbors(n), 16))
        rm = planning.build_roadmap(robot, environment, n_samples=n, k=k, sampler=rng,
                                    extra_vertices=[_cfg(robot, start)] + goals)
        return Roadmap(list(rm.vertices), [tuple(map(int, e)) for e in rm.edges], time.perf_counter_ns() - t0, 1), rm

    def prm(start, goal, environment, settings, rng):
        t0 = time.perf_counter_ns()
        start_c, goals = _cfg(robot, start), _goals(robot, goal)
        ok = robot.validate_batch(np.stack([start_c] + goals), environment)
        res = planning.PlanningResult()
        if ok[0] and ok[1:].any():
            n, it = 512, 0
            while n <= min(int(settings.max_samples), 65536) and not res.solved:
                it += 1  # each attempt draws the sampler's NEXT n samples (the caller's sampler is never rewound)
                _, rm = roadmap(start_c, goals, environment, settings, rng, n_samples=n)
                res.iterations, res.size = it, [len(rm.vertices)]
                # the extra vertices survive validation in order: start first, then the valid goals
                n_goal = int(ok[1:].sum())
                best = None
                for gi in range(1, 1 + n_goal):
                    idx = rm.shortest_path(0, gi)
                    if idx is not None:
                        cost = sum(float(np.linalg.norm(rm.vertices[a] - rm.vertices[b])) for a, b in zip(idx[:-1], idx[1:]))
                        if best is None or cost < best[0]:
                            best = (cost, idx)
                if best is not None:
                    res.path = [rm.vertices[i] for i in best[1]]
                n *= 2
        return as_result(res, t0)

    def prm_multi(starts, goals, environments, settings, skips=None, samples=None):
        """planning.prm_multi with this robot and the reference-shaped RoadmapSettings: n_samples = min(max_samples,
        2048) rounded down to a multiple of 64 and at least 64, k = min(max_neighbors(n_samples), 16) and at least 1, as
        roadmap() maps it -> list[PlanningResult] (each with `status`; nanoseconds is the whole call's time divided by the problems)"""
        t0 = time.perf_counter_ns()
        n = max(64, min(int(settings.max_samples), 2048) // 64 * 64)
        s = planning.PRMMultiSettings(n_samples=n, k=max(1, min(settings.max_neighbors(n), 16)))
        results = planning.prm_multi(robot, starts, goals, environments, s, skips, samples)
        each = (time.perf_counter_ns() - t0) // max(len(results), 1)
        out = []
        for r in results:
            path = Path()
            for q in r.path:
                path.append(q)
            res = PlanningResult(path, each, r.iterations, r.size, r.cost)
            res.status = r.status
            out.append(res)
        return out

    def build_roadmaps(environments, settings=None, skips=None, samples=None):
        """planning.build_roadmaps with this robot -> planning.DeviceRoadmaps (`settings`: a planning.RoadmapsSettings)"""
        return planning.build_roadmaps(robot, environments, settings, skips, samples)

    def fcit_multi(starts, goals, environments, settings, skips=None, samples=None):
        """planning.fcit_multi with this robot and the reference-shaped FCITSettings: n_samples = min(max_samples, 2048)
        rounded down to a multiple of 64 and at least 64, max_iterations as given (at least 1) -> list[PlanningResult]
        (each with `status`; nanoseconds is the whole call's time divided by the problems)"""
        t0 = time.perf_counter_ns()
        n = max(64, min(int(settings.max_samples), 2048) // 64 * 64)
        s = planning.FCITMultiSettings(n_samples=n, max_iterations=max(1, min(int(settings.max_iterations), 2 ** 32 - 1)))
        results = planning.fcit_multi(robot, starts, goals, environments, s, skips, samples)
        each = (time.perf_counter_ns() - t0) // max(len(results), 1)
        out = []
        for r in results:
            path = Path()
            for q in r.path:
                path.append(q)
            res = PlanningResult(path, each, r.iterations, r.size, r.cost)
            res.status = r.status
            out.append(res)
        return out

    def simplify(path, environment, settings, rng):
        """greedy shortcutting: for every waypoint the farthest later waypoint it can reach by a valid motion; the
        candidate motions of one pass are validated together (`validate_motion_batch`)"""
        t0 = time.perf_counter_ns()
        pts = [np.asarray(p, np.float32) for p in path]
        for _ in range(max(1, int(settings.max_iterations))):
            if len(pts) < 3:
                break
            n = len(pts)
            pairs = [(i, j) for i in range(n - 2) for j in range(i + 2, n)]
            a = np.stack([pts[i] for i, _ in pairs])
            b = np.stack([pts[j] for _, j in pairs])
            ok = robot.validate_motion_batch(a, b, environment)
            reach = {i: i + 1 for i in range(n - 1)}
            for (i, j), v in zip(pairs, ok):
                if v and j > reach[i]:
                    reach[i] = j
            out, i = [pts[0]], 0
            while i < n - 1:
                i = reach[i]
                out.append(pts[i])
            if len(out) == len(pts):
                break
            pts = out
        res = Path()
        for q in pts:
            res.append(q)
        if int(getattr(settings, "interpolate", 0)) > 0:
            res.interpolate_to_n_states(int(settings.interpolate))
        return PlanningResult(res, time.perf_counter_ns() - t0, 0, [], res.cost() if len(res) >= 2 else 0.0)

    def simplify_multi(paths, environments, settings=None):
        """planning.simplify_multi with this robot: the reference's SHORTCUT and BSPLINE routines for many paths in
        lockstep on the device -> list[PlanningResult] (each with `status`; nanoseconds is the whole call's time
        divided by the paths).  `settings`: a SimplifySettings or a planning.SimplifyMultiSettings."""
        t0 = time.perf_counter_ns()
        results = planning.simplify_multi(robot, paths, environments, settings)
        each = (time.perf_counter_ns() - t0) // max(len(results), 1)
        out = []
        for r in results:
            path = Path()
            for q in r.path:
                path.append(q)
            res = PlanningResult(path, each, r.iterations, [], r.cost)
            res.status = r.status
            out.append(res)
        return out

    def simplify_multi_constrained(paths, environments, constraints, settings=None, constraint_settings=None):
        """planning.simplify_multi_constrained with this robot: `simplify_multi` inside the band of end-effector
        constraints -> list[planning.PlanningResult] (each with `status`, `cost` and `band_refused`)."""
        return planning.simplify_multi_constrained(robot, paths, environments, constraints, settings, constraint_settings)

    def optimize_multi(paths, environments, settings=None, resolution=None):
        """planning.optimize_multi with this robot: the clearance-aware covariant gradient iteration for many paths in
        lockstep on the device -> list[planning.OptimizedPath].  The clearances are those of the waypoints, validity is
        validate_motion's on the consecutive edges, the gradient is the current witness's."""
        return planning.optimize_multi(robot, paths, environments, settings, resolution)

    def optimize_multi_constrained(paths, environments, constraints, settings=None, constraint_settings=None, resolution=None):
        """planning.optimize_multi_constrained with this robot: `optimize_multi` inside the band of end-effector
        constraints -> list[planning.OptimizedPath] (each with `held`; `status` may be "out_of_band")."""
        return planning.optimize_multi_constrained(robot, paths, environments, constraints, settings, constraint_settings, resolution)

    def cartesian_multi(starts, targets, environments=None, settings=None):
        """planning.cartesian_multi with this robot: straight-line end-effector motions for many problems in one call on
        the device -> list[planning.CartesianPath]."""
        return planning.cartesian_multi(robot, starts, targets, environments, settings)

    def retime_multi(paths, vel_limits, acc_limits, environments=None, settings=None):
        """planning.retime_multi with this robot: time-optimal trajectories along many paths in one call on the device
        -> list[planning.Trajectory]."""
        return planning.retime_multi(robot, paths, vel_limits, acc_limits, environments, settings)

    def retime_multi_constrained(paths, vel_limits, acc_limits, environments=None, constraints=None, settings=None,
                                 constraint_settings=None):
        """planning.retime_multi_constrained with this robot: `retime_multi` whose blends are halved, corner by corner,
        until every sample pair is valid and inside the band -> list[planning.RepairedTrajectory]."""
        return planning.retime_multi_constrained(robot, paths, vel_limits, acc_limits, environments, constraints, settings,
                                                 constraint_settings)

    robot.optimize_multi = optimize_multi
    robot.cartesian_multi = cartesian_multi
    robot.retime_multi = retime_multi
    robot.retime_multi_constrained = retime_multi_constrained
    robot.rrtc, robot.fcit, robot.prm, robot.simplify = rrtc, fcit, prm, simplify
    robot.rrtc_multi, robot.simplify_multi, robot.prm_multi = rrtc_multi, simplify_multi, prm_multi
    robot.rrtc_multi_goals = rrtc_multi_goals
    robot.rrtc_multi_constrained = rrtc_multi_constrained
    robot.simplify_multi_constrained = simplify_multi_constrained
    robot.optimize_multi_constrained = optimize_multi_constrained
    robot.aorrtc, robot.aorrtc_multi = aorrtc, aorrtc_multi
    robot.aorrtc_multi_constrained = aorrtc_multi_constrained
    robot.fcit_multi, robot.build_roadmaps = fcit_multi, build_roadmaps
    robot.roadmap = lambda start, goal, environment, settings, rng: roadmap(start, goal, environment, settings, rng)[0]


# ------------------------------------------------------------------- module-level helpers (contract: src/vamp/__init__.py)
_log = logging.getLogger("vamp_mvt_amd")


def _planner_settings(robot_module, robot_name, planner_name):
    """default settings object of a planner (the reference's per-planner defaults, src/vamp/__init__.py:76-95)"""
    makers = {
        "rrtc": lambda: RRTCSettings(range=ROBOT_RRT_RANGES.get(robot_name, RRTCSettings.range)),
        "prm": lambda: PRMSettings(PRMNeighborParams(robot_module.dimension(), robot_module.space_measure())),
        "fcit": lambda: FCITSettings(FCITNeighborParams(robot_module.dimension(), robot_module.space_measure())),
        "aorrtc": lambda: AORRTCSettings(rrtc=RRTCSettings(range=ROBOT_RRT_RANGES.get(robot_name, RRTCSettings.range),
                                                           dynamic_domain=False)),
    }
    if planner_name not in makers:
        raise NotImplementedError(f"no automatic settings for planner '{planner_name}' in this build")
    settings = makers[planner_name]()
    settings.max_iterations = settings.max_samples = DEFAULT_ITERATIONS
    return settings


def _route_kwarg(key, plan_settings, simp_settings):
    """Where a keyword of configure_robot_and_planner_with_kwargs lands: yields (owner, attribute, label).  The rules
    are the reference's (src/vamp/__init__.py:100-134): a planner attribute by its own name; a simplifier attribute
    behind the marker `simplification_`; an attribute of one simplifier routine behind `<routine>_` (markers are
    matched anywhere in the key and removed from it)."""
    yield plan_settings, key, "planner"
    if "simplification_" in key:
        yield simp_settings, key.replace("simplification_", ""), "simplifier"
    for routine in ("reduce", "shortcut", "bspline", "perturb"):
        if routine in key:
            yield getattr(simp_settings, routine), key.replace(routine + "_", ""), f"simplifier.{routine}"


def configure_robot_and_planner_with_kwargs(robots, robot_name: str, planner_name: str, **kwargs):
    """-> (robot module, planner function, planner settings, simplifier settings); same defaults, keyword routing and
    errors as the reference's function of this name (src/vamp/__init__.py:69-139)."""
    robot_module = robots[robot_name]
    if not hasattr(robot_module, planner_name):
        raise ValueError(f"Robot {robot_name} does not support planner {planner_name}!")
    plan_settings = _planner_settings(robot_module, robot_name, planner_name)
    simp_settings = SimplifySettings()
    for key, value in kwargs.items():
        for owner, attribute, label in _route_kwarg(key, plan_settings, simp_settings):
            if not hasattr(owner, attribute):
                continue
            if owner is simp_settings and attribute == "operations":  # routine names -> SimplifyRoutine members
                value = [getattr(SimplifyRoutine, name) for name in value]
            _log.info("%s.%s = %r", label, attribute, value)
            setattr(owner, attribute, value)
    return robot_module, getattr(robot_module, planner_name), plan_settings, simp_settings


def results_to_dict(planning_result, simplification_result=None):
    """One flat record per solved problem, with the column names of the reference's function of this name
    (src/vamp/__init__.py:188-228) so that its evaluation scripts' DataFrames keep their columns."""
    try:
        from pandas import Timedelta
    except ImportError as exc:
        raise RuntimeError("pandas is not installed!") from exc
    plan_path = planning_result.path
    final = simplification_result if simplification_result else None
    final_path = final.path if final is not None else plan_path
    t_plan = Timedelta(nanoseconds=planning_result.nanoseconds)
    t_simp = Timedelta(nanoseconds=final.nanoseconds if final is not None else 0)
    return {
        "planning_time": t_plan,
        "planning_iterations": planning_result.iterations,
        "solved": len(plan_path) > 0,
        "planning_graph_size": sum(planning_result.size),
        "initial_path_vertices": len(plan_path),
        "initial_path_cost": plan_path.cost(),
        "simplification_time": t_simp,
        "simplified_path_vertices": len(final_path),
        "simplified_path_cost": final_path.cost(),
        "total_time": t_plan + t_simp,
    }
