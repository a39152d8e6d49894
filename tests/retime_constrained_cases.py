"""The case set of vmv_retime_multi_constrained's tests (tests/test_retime_constrained.py asserts every class on the CPU,
tests/test_retime_constrained_gpu.py runs the device over it) — TEST INFRASTRUCTURE ONLY.

The corners are constants: per robot one 3-waypoint path whose blends, at every level, carry the end effector farther
along a direction than the polyline ever does, and one whose blends tilt an axis of the tool farther from an axis of the
world (each found once by a random search; free of self-collision).  Everything else
is found here by a CPU search over the serial statement (tests/retime_constrained_serial.py): sphere obstacles against the
CPU oracle, band thresholds against the float64 band of tests/constraint_serial.py, each candidate classified by running
the statement.  A band case is accepted only where every sample the band was asked about is farther than MARGIN from the
band's faces, so that the float64 band and the device's fp32 band (whose frames differ by some 1e-6) give the same class.

Nothing here imports the package."""
from __future__ import annotations

import functools
import json
import os
from dataclasses import dataclass, replace

import numpy as np

import constraint_serial as CS
import ik_serial as K
import retime_constrained_serial as RC
import retime_serial as RS

ROBOTS = ("panda", "baxter")
MARGIN = 5e-5  # metres / difference of cosines; fp32 frames are good to some 1e-6
SETTINGS = RC.Settings(blend=1.0, grid_step=0.041, dt=0.04, max_grid=1200, blend_halvings=3, max_rounds=8)
CS_SETTINGS = CS.Settings()

CORNER = {
    "panda": (np.array([[-2.3390872, 1.7727331, 0.02945706, -1.2033485, -0.8570103, 1.3441123, -0.5211494],
                        [-1.428252, 0.1632464, 0.47266772, -0.69510555, 0.7113121, 1.5878227, -0.54591495],
                        [-1.670965, -0.7407138, 0.7103132, 0.04467913, 1.6964529, 2.4389288, -1.5296987]], np.float32),
              np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)),
    "baxter": (np.array([[-0.07033872, -0.3572622, -1.3884315, 0.00772638, 1.1410215, 0.48856053, -0.4745917, -0.3538959,
                          -1.1496229, -0.6226674, 0.01309102, -0.91163605, -1.4935018, -0.9392806],
                         [-0.07033872, -0.3572622, -1.3884315, 0.00772638, 1.1410215, 0.48856053, -0.4745917, 0.46737728,
                          -0.86931896, -0.81664556, 0.5864408, -0.74013346, 0.53343177, -0.56914246],
                         [-0.07033872, -0.3572622, -1.3884315, 0.00772638, 1.1410215, 0.48856053, -0.4745917, -0.1954592,
                          -0.0057107, -1.5604434, 1.6534047, -0.14174718, 1.6548948, -1.0226619]], np.float32),
               np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)),
}


# per robot a corner of the same kind for the cone: (path, the world's axis, the end effector's axis) - the angle between the
# two is larger inside the corner, at every level, than anywhere on the polyline, and stays below 1.35 rad
CONE_CORNER = {
    "panda": (np.array([[1.9827899, 0.5567233, 1.5587156, -0.7418072, 0.0412538, 1.6066189, 0.7809176],
                        [0.51254785, -0.14874136, 1.236947, -0.8647735, -0.4216449, 1.6650122, -0.788596],
                        [-0.011083258, 0.11746079, 1.4329848, -0.6234029, -2.3958464, 1.697569, -1.6436266]], np.float32),
              np.array([0.478857255, 0.852549393, -0.209416477]), np.array([0.0, 1.0, 0.0])),
    "baxter": (np.array([[-0.7111254, -0.6671826, -0.8218332, 1.018245, 0.14421105, -0.32759643, 0.92812836, -0.27751577,
                          -1.0031627, 0.9476854, 0.099283114, -1.3338028, 0.612015, -0.6095715],
                         [-0.7111254, -0.6671826, -0.8218332, 1.018245, 0.14421105, -0.32759643, 0.92812836, -0.2539229,
                          -0.3660673, 0.9602094, 1.0522054, -1.2046548, -0.41498724, 0.86432946],
                         [-0.7111254, -0.6671826, -0.8218332, 1.018245, 0.14421105, -0.32759643, 0.92812836, 0.6139299,
                          -1.2780865, -0.06967781, 2.046395, -0.5677323, -0.16353543, 2.2400672]], np.float32),
               np.array([-0.889425897, 0.231980272, -0.393835913]), np.array([0.125873469, -0.821071004, -0.556774889])),
}


def limits(robot):
    return RS.limits(robot)


def frame_z(direction):
    """a rigid frame at the origin whose z axis is `direction`, rounded to fp32"""
    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0])
    x = x / np.linalg.norm(x)
    F = np.eye(4)
    F[:3, 0], F[:3, 1], F[:3, 2] = x, np.cross(z, x), z
    return F.astype(np.float32).astype(np.float64)


def blend_points(path, corner, level, S=SETTINGS, n=41):
    """float64 points of the blend at `corner` (an inner waypoint index of a path without duplicates) at `level`"""
    w = np.asarray(path, np.float64)
    L0, L1 = np.linalg.norm(w[corner] - w[corner - 1]), np.linalg.norm(w[corner + 1] - w[corner])
    u0, u1 = (w[corner] - w[corner - 1]) / L0, (w[corner + 1] - w[corner]) / L1
    d = min(S.blend, L0 / 2, L1 / 2) / 2 ** level
    s = np.linspace(0.0, 2 * d, n)[:, None]
    return (w[corner] - d * u0) + u0 * s + 0.5 * (u1 - u0) / (2 * d) * s * s


def polyline_points(path, n=81):
    w = np.asarray(path, np.float64)
    t = np.linspace(0.0, 1.0, n)[:, None]
    return np.concatenate([w[e] + (w[e + 1] - w[e]) * t for e in range(len(w) - 1)])


def along(robot, q, direction):
    """the end effector's position along `direction` (float64)"""
    t, _, _ = K.frame_jac(robot, np.asarray(q, np.float64))
    return t @ (np.asarray(direction) / np.linalg.norm(direction))


def tilt(robot, q, axis, tool=(0.0, 0.0, 1.0)):
    """the angle between the axis `tool` of the end effector and the world's `axis` (float64)"""
    _, R, _ = K.frame_jac(robot, np.asarray(q, np.float64))
    a = R @ (np.asarray(tool, np.float64) / np.linalg.norm(tool))
    return np.arccos(np.clip(a @ (np.asarray(axis) / np.linalg.norm(axis)), -1.0, 1.0))


def box_below(direction, threshold):
    """the end effector stays at or below `threshold` along `direction`"""
    return CS.box((-np.inf, -np.inf, -np.inf), (np.inf, np.inf, float(np.float32(threshold))), frame_z(direction))


def cone_about(axis, max_angle, tool=(0.0, 0.0, 1.0)):
    return CS.upright(tuple(float(np.float32(v)) for v in tool), float(np.float32(max_angle)), frame_z(axis))


@dataclass
class Case:
    name: str
    kind: str            # the class letter of the issue
    robot: str
    path: np.ndarray     # float32 [len][dim]
    spheres: tuple = ()  # ((x, y, z, r), ...): the path's environment; with `validate` False there is none
    constraint: object = None  # a constraint_serial.Constraint
    settings: RC.Settings = SETTINGS
    validate: bool = True      # environments given: every case has one (the empty one checks the robot against itself)
    expect: object = None      # the serial Result on the CPU hooks


class Recorder:
    """the hooks of one case on the CPU: the oracle and the float64 band, keeping the smallest band margin seen"""

    def __init__(self, oracle, case):
        self.o, self.rid, self.case = oracle, oracle.robot(case.robot), case
        self.env = oracle.env()
        for s in case.spheres:
            self.env.add_sphere(*[float(v) for v in s])
        self.margin = np.inf
        self.valid = (lambda a, b: bool(self.o.validate_motion(self.rid, self.env, a, b))) if case.validate else None
        self.band_edge = self._band if case.constraint is not None else None

    def _band(self, a, b):
        q = CS.edge_samples32(a, b, CS_SETTINGS.check_step)
        if q is None:
            return False
        self.margin = min(self.margin, float(CS.band_margin(self.case.robot, q, self.case.constraint, CS_SETTINGS).min()))
        return bool(CS.in_band(self.case.robot, q, self.case.constraint, CS_SETTINGS)[0].all())


def run(oracle, case):
    """-> (the serial Result of the case on the CPU hooks, the smallest band margin)"""
    rec = Recorder(oracle, case)
    V, A = limits(case.robot)
    return RC.retime_constrained(case.path, V, A, case.settings, rec.valid, rec.band_edge), rec.margin


def top_level(res, corner=None):
    lev = res.levels if corner is None else res.levels[corner:corner + 1]
    return int(lev.max()) if len(lev) else 0


def sphere_candidates(oracle, robot, hit, clear, radius=0.01, count=6, seed=0):
    """small spheres (x, y, z, radius) that reach into the robot at some configuration of EVERY list in `hit` and stay
    clear of it at every configuration of `clear`, the deepest first: random centres around where the robot's spheres are
    at the hit configurations, judged by the robot's own spheres (the oracle's forward kinematics)"""
    rid = oracle.robot(robot)
    fk = lambda qs: np.stack([np.asarray(oracle.fk(rid, np.float32(q))) for q in qs])  # [configs][spheres][4]
    hits, free = [fk(h) for h in hit], fk(clear)
    rng = np.random.default_rng(seed)
    middle = hits[-1][len(hits[-1]) // 2]
    moved = np.linalg.norm(middle[:, :3] - free[len(free) // 2][:, :3], axis=1)
    pts = np.concatenate([middle[s, :3] + rng.uniform(-0.15, 0.15, (700, 3)) for s in np.argsort(-moved)[:6]])

    def depth(spheres):  # how far a sphere at each point reaches into the robot, the deepest over configurations
        d = np.linalg.norm(pts[:, None, None, :] - spheres[None, :, :, :3], axis=3)
        return (spheres[None, :, :, 3] + radius - d).max(axis=(1, 2))

    into = np.min([depth(h) for h in hits], axis=0)
    score = np.where(depth(free) < -0.002, into, -np.inf)
    for i in np.argsort(-score)[:count]:
        if score[i] > 0.004:
            yield tuple(float(v) for v in pts[i]) + (radius,)


def find(oracle, candidates, accept):
    for case in candidates:
        res, margin = run(oracle, case)
        if margin > MARGIN and accept(res):
            case.expect = res
            return case
    raise AssertionError("the search found no case of this class")


def thresholds(lo, hi):
    """candidate thresholds strictly between two levels' extremes, the middle first"""
    return [lo + f * (hi - lo) for f in (0.5, 0.35, 0.65)]


def search(robot, oracle):
    """the search itself -> tuple of Case, each with its serial Result on the CPU hooks in `expect`.  Some 20 s per robot:
    `python tests/retime_constrained_cases.py` runs it and writes what it finds to tests/golden, where cases() reads it."""
    path, direction = CORNER[robot]
    H = SETTINGS.blend_halvings
    b = path[1].astype(np.float64)
    mid = lambda level: blend_points(path, 1, level, n=3)[1]
    out = []

    def case(name, kind, **kw):
        return Case(name, kind, robot, kw.pop("path", path), **kw)

    # (a) nothing to repair: the corner in the empty environment
    out.append(find(oracle, [case("clean", "a")], lambda r: r.status == "complete" and r.rounds == 1))
    # (b) a sphere inside the corner's level-0 blend that level 1 or 2 clears; (c) one that only the stop clears
    poly = polyline_points(path)
    out.append(find(oracle, (case("sphere_level", "b", spheres=(s,))
                             for s in sphere_candidates(oracle, robot, [blend_points(path, 1, 0)], np.concatenate([poly, blend_points(path, 1, 2)]))),
                    lambda r: r.status == "complete" and top_level(r) in (1, 2)))
    # (the stop case halves once only: a sphere must reach into every level's blend and stay clear of the polyline, and
    # the blends of levels 0 .. 3 lie too far apart for one small sphere next to this corner)
    once = replace(SETTINGS, blend_halvings=1)
    out.append(find(oracle, (case("sphere_stop", "c", spheres=(s,), settings=once) for s in sphere_candidates(oracle, robot, [blend_points(path, 1, 0), blend_points(path, 1, 1)], poly)),
                    lambda r: r.status == "complete" and top_level(r) == 2 and r.stops == 1))
    # (d) a sphere on a line: the robot's own sphere's place halfway along the first edge
    rid = oracle.robot(robot)
    on_line = np.asarray(oracle.fk(rid, np.float32(0.5 * (path[0].astype(np.float64) + b))))
    far = int(np.argmax(np.linalg.norm(on_line[:, :3] - np.asarray(oracle.fk(rid, path[1]))[:, :3], axis=1)))
    out.append(find(oracle, [case("sphere_line", "d", spheres=(tuple(float(v) for v in on_line[far, :3]) + (0.01,),))],
                    lambda r: r.status == "collision" and r.rounds == 1 and top_level(r) == 0))
    # (e) two corners whose edge is 1.2 <= 2 blend long, so that their blends abut, and a sphere where they meet
    w = path.astype(np.float64)
    u0, u1 = (w[1] - w[0]) / np.linalg.norm(w[1] - w[0]), (w[2] - w[1]) / np.linalg.norm(w[2] - w[1])
    four = np.stack([w[1] - 1.3 * u0, w[1], w[1] + 1.2 * u1, w[1] + 1.2 * u1 - 1.3 * u0]).astype(np.float32)
    meet = np.asarray(oracle.fk(rid, np.float32(w[1] + 0.6 * u1)))
    both = lambda r: any(len(f[3]) == 2 for f in r.history[0][1])
    out.append(find(oracle, (case("abutting", "e", path=four, spheres=(tuple(float(v) for v in meet[s, :3]) + (0.01,),))
                             for s in np.argsort(-np.linalg.norm(meet[:, :3] - np.asarray(oracle.fk(rid, path[1]))[:, :3], axis=1))[:4]), both))
    # (f) the same three classes with bands: the end effector's reach along `direction` under a box, its tilt under a cone
    reach = [along(robot, blend_points(path, 1, lv), direction).max() for lv in range(H + 1)]
    reach_poly = along(robot, polyline_points(path), direction).max()
    out.append(find(oracle, (case("box_level", "fb", constraint=box_below(direction, t)) for t in thresholds(reach[1], reach[0])),
                    lambda r: r.status == "complete" and top_level(r) in (1, 2)))
    out.append(find(oracle, (case("box_stop", "fc", constraint=box_below(direction, t)) for t in thresholds(reach_poly, reach[H])),
                    lambda r: r.status == "complete" and top_level(r) == H + 1))
    line_reach = along(robot, polyline_points(path[:2])[8:33], direction)
    out.append(find(oracle, (case("box_line", "fd", constraint=box_below(direction, t))
                             for t in line_reach.max() - np.array([0.01, 0.013, 0.017, 0.022, 0.03, 0.04])),
                    lambda r: r.status == "out_of_band" and r.rounds == 1))
    # the cone has a corner of its own (CONE_CORNER): under it the tool's tilt from an axis is largest inside the corner
    cone_path, axis, tool = CONE_CORNER[robot]
    unit = lambda v: v / np.linalg.norm(v)
    rot_tol = CS_SETTINGS.rot_tol  # (the band is max_angle + rot_tol wide: the thresholds below are the band's)
    turn = [tilt(robot, blend_points(cone_path, 1, lv), axis, tool).max() for lv in range(H + 1)]
    turn_poly = tilt(robot, polyline_points(cone_path), axis, tool).max()
    out.append(find(oracle, (case("cone_level", "fb", path=cone_path, constraint=cone_about(axis, t - rot_tol, tool))
                             for t in thresholds(turn[1], turn[0])),
                    lambda r: r.status == "complete" and top_level(r) in (1, 2)))
    out.append(find(oracle, (case("cone_stop", "fc", path=cone_path, constraint=cone_about(axis, t - rot_tol, tool))
                             for t in thresholds(turn_poly, turn[H])),
                    lambda r: r.status == "complete" and top_level(r) == H + 1))
    line_turn = tilt(robot, polyline_points(cone_path[:2])[8:33], axis, tool)
    out.append(find(oracle, (case("cone_line", "fd", path=cone_path, constraint=cone_about(axis, t - rot_tol, tool))
                             for t in line_turn.max() - np.array([0.01, 0.013, 0.017, 0.022, 0.03, 0.04])),
                    lambda r: r.status == "out_of_band" and r.rounds == 1))
    # (g) five waypoints: the band fails at corner 1 (the box of "box_level"), a sphere sits in corner 3's blend
    boxed = next(c for c in out if c.name == "box_level")
    ext, mask, limit = np.random.default_rng(3), CS.ee_mask(robot), boxed.constraint.pos_hi[2] - 0.01
    for trial in range(60):  # two more waypoints: free of self-collision and, with their blends, well inside the box
        v = [unit(ext.normal(size=len(u0)) * mask) for _ in range(2)] if trial else [u0, -u1]
        five = np.concatenate([path, np.stack([w[2] + 2.1 * v[0], w[2] + 2.1 * v[0] + 2.1 * v[1]])]).astype(np.float32)
        added = np.concatenate([polyline_points(five[2:]), blend_points(five, 2, 0), blend_points(five, 3, 0)])
        if along(robot, added, direction).max() < limit and run(oracle, case("x", "g", path=five))[0].status == "complete":
            break
    else:
        raise AssertionError("no extension of the corner is free")
    only = lambda r: (r.status == "complete" and [int(x > 0) for x in r.levels] == [0, 1, 0, 1, 0] and
                      all(all(f[3] == [1] for f in fails if not f[2]) and all(f[3] == [3] for f in fails if not f[1])
                          for _, fails, _ in r.history) and
                      any(not f[2] for _, fails, _ in r.history for f in fails) and any(not f[1] for _, fails, _ in r.history for f in fails))
    out.append(find(oracle, (case("two_causes", "g", path=five, spheres=(s,), constraint=boxed.constraint)
                             for s in sphere_candidates(oracle, robot, [blend_points(five, 3, 0)],
                                                        np.concatenate([polyline_points(five), blend_points(five, 3, 2), blend_points(five, 1, 0),
                                                                        blend_points(five, 2, 0)]))), only))
    # (h) a period so long that a sample pair jumps over a whole level-3 blend
    stop = next(c for c in out if c.name == "box_stop")
    for dt in (0.3, 0.4, 0.5, 0.7):
        c = replace(stop, name="long_period", kind="h", settings=replace(SETTINGS, dt=dt), expect=None)
        c.expect, _ = run(oracle, c)
        if jumps(c.expect):
            out.append(c)
            break
    else:
        raise AssertionError("no period makes a pair jump over a level-3 blend")
    # (i) one round only, on the (b) sphere
    level = next(c for c in out if c.name == "sphere_level")
    out.append(find(oracle, [replace(level, name="one_round", kind="i", settings=replace(SETTINGS, max_rounds=1), expect=None)],
                    lambda r: r.status == "collision" and r.rounds == 1))
    # (j) what has no trajectory to repair
    for name, pts in RS.cases(robot):
        if name in ("no_waypoints", "one_waypoint", "one_waypoint_thrice", "duplicates", "nan_waypoint", "line_1mm"):
            out.append(find(oracle, [case(name, "j", path=pts)], lambda r: True))
    return tuple(out)


def jumps(res):
    """whether in some round a failing pair's samples lie on pieces with a whole blend of the last level between them"""
    return any(f[4] for _, fails, _ in res.history for f in fails)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retime_constrained_cases.json")


def _plain(case):
    c = case.constraint
    return dict(name=case.name, kind=case.kind, robot=case.robot, path=np.asarray(case.path, np.float32).tolist(),
                spheres=[list(s) for s in case.spheres], validate=case.validate,
                settings={k: getattr(case.settings, k) for k in ("dt", "blend_halvings", "max_rounds")},
                constraint=None if c is None else dict(frame=np.asarray(c.frame).tolist(), pos_lo=list(c.pos_lo), pos_hi=list(c.pos_hi),
                                                       tool_axis=list(c.tool_axis), ref_axis=list(c.ref_axis), max_angle=c.max_angle))


def _case(d):
    c = d["constraint"]
    return Case(d["name"], d["kind"], d["robot"], np.asarray(d["path"], np.float32).reshape(-1, RS.DIM[d["robot"]]),
                tuple(tuple(s) for s in d["spheres"]),
                None if c is None else CS.Constraint(np.asarray(c["frame"], np.float64), tuple(c["pos_lo"]), tuple(c["pos_hi"]),
                                                     tuple(c["tool_axis"]), tuple(c["ref_axis"]), c["max_angle"]),
                replace(SETTINGS, **d["settings"]), d["validate"])


@functools.lru_cache(maxsize=None)
def cases(robot):
    """-> tuple of Case as the search found them (tests/golden/retime_constrained_cases.json), without `expect`"""
    with open(GOLDEN) as f:
        return tuple(_case(d) for d in json.load(f)[robot])


@functools.lru_cache(maxsize=None)
def expected(robot):
    """-> per case (the serial Result on the CPU hooks, the smallest band margin); computed once per session"""
    from oracle_lib import Oracle
    oracle = Oracle()
    return tuple(run(oracle, c) for c in cases(robot))


if __name__ == "__main__":
    from oracle_lib import Oracle
    with open(GOLDEN, "w") as f:
        json.dump({robot: [_plain(c) for c in search(robot, Oracle())] for robot in ROBOTS}, f, indent=1)
