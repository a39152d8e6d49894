"""planning.cartesian_multi / <robot>.cartesian_multi / planning.approach_multi on the device.

There is no reference for a Cartesian path; the yardsticks are the float64 evaluation of the generator's end-effector tape
(ik_serial.frame_jac) and the float64 statement of the line and its tracking (tests/cartesian_serial.py).  A path is checked
for what it promises: every waypoint's float64 frame against pose k of the float64 line built from eefk_batch's frame, the
joint steps, the counts.  Status and achieved are compared with the statement where tests/test_cartesian.py shows on the
CPU that the statement's answer has a margin (cartesian_serial.robust).  Validation is held against validate_motion_batch
itself, and everything else is bit for bit: a problem against itself alone, in other batches, orders and environments."""
import numpy as np
import pytest

import cartesian_serial as C
import ik_serial as K

pytestmark = pytest.mark.gpu
ROBOTS = C.ROBOTS
# tests/test_ik_gpu.py's FRAME_SLACK, derived there: ten times the fp32 rounding of a frame (DESIGN.md 5i measured 1e-6 m for
# sphere centres), a tenth of the tolerances
FRAME_SLACK = 1e-5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_paths(a, b):
    return len(a) == len(b) and all(x.status == y.status and x.segments == y.segments and x.achieved == y.achieved and
                                    x.evaluations == y.evaluations and np.array_equal(bits(x.path), bits(y.path))
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def sets(vamp):
    """per robot: the shared case set, the device's start frames, and ONE kinematics-only call per value of position_only -
    shared by the tests, left unchanged"""
    out = {}
    for robot in ROBOTS:
        mod = getattr(vamp, robot)
        starts, targets, names = C.cases(robot)
        out[robot] = dict(mod=mod, starts=starts, targets=targets, names=names, frames=mod.eefk_batch(starts),
                          kin={po: vamp.planning.cartesian_multi(mod, starts, targets, None,
                                                                 vamp.planning.CartesianSettings(position_only=po))
                               for po in (False, True)})
    return out


# ---- 1. the contract in float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position_only", (False, True))
@pytest.mark.parametrize("robot", ROBOTS)
def test_every_waypoint_is_on_the_float64_line(sets, robot, position_only):
    case = sets[robot]
    s = C.Settings(position_only=position_only)
    paths = case["kin"][position_only]
    assert len(paths) == len(case["starts"])
    rows, poses = [], []
    for p, r in enumerate(paths):
        line = C.line(case["frames"][p], case["targets"][p], s)
        assert r.segments == line.m, (case["names"][p], r.segments, line.m)
        assert r.achieved <= r.segments and r.path.shape == (r.achieved + 1, case["starts"].shape[1]) and r.path.dtype == np.float32
        assert r.fraction == r.achieved / r.segments
        assert np.array_equal(bits(r.path[0]), bits(case["starts"][p]))  # the start's bits
        assert (r.status == "complete") == (r.achieved == r.segments)
        assert r.status in ("complete", "ik_failed", "joint_jump")  # nothing is validated without environments
        if r.achieved:  # the device's own comparison: fp32 differences against the fp32 setting
            assert np.abs(r.path[1:] - r.path[:-1]).max() <= np.float32(s.max_joint_step)
        for k in range(1, r.achieved + 1):
            rows.append(r.path[k])
            poses.append(line.pose(k))
    t, R, _ = K.frame_jac(robot, np.array(rows, np.float64))
    e_p, e_w, tr = K.errors(t, R, np.array(poses))
    n_p, n_w = np.linalg.norm(e_p, axis=1), np.linalg.norm(e_w, axis=1)
    print(f"{robot} position_only={position_only}: {len(rows)} waypoints, worst |e_p| {n_p.max():.3g}, worst |e_w| {n_w.max():.3g}")
    assert n_p.max() <= s.pos_tol + FRAME_SLACK
    if not position_only:
        assert n_w.max() <= s.rot_tol + FRAME_SLACK and tr.min() > 1.0
    assert sum(r.achieved for r in paths) > 100  # (the set is not one of stillborn lines)


# ---- 2. agreement with the statement where it has a margin -----------------------------------------------------------------
@pytest.mark.parametrize("position_only", (False, True))
@pytest.mark.parametrize("robot", ROBOTS)
def test_status_and_achieved_agree_with_the_statement(sets, robot, position_only):
    paths = sets[robot]["kin"][position_only]
    want = C.tracked(robot, position_only)
    mask = C.robust(robot, position_only)
    assert 2 * int(mask.sum()) >= len(paths)  # the cases left out are at most half of the set
    got = [(r.status, r.achieved) for r in paths]
    print(robot, position_only, [(sets[robot]["names"][p], got[p], (want["status"][p], int(want["achieved"][p])))
                                 for p in range(len(paths)) if got[p] != (want["status"][p], int(want["achieved"][p]))])
    for p in np.flatnonzero(mask):
        assert got[p] == (want["status"][p], int(want["achieved"][p])), (sets[robot]["names"][p], got[p])


# ---- 3. validation -------------------------------------------------------------------------------------------------------
def moving_sphere(vamp, case, paths, fast):
    """-> (problem, k, environment): a completed line that is valid in the empty environment, k = m, and an environment
    with one small sphere on the fine sphere that travels farthest from the start to waypoint k, clear of the start"""
    mod, found = case["mod"], []
    for p in np.flatnonzero(fast):
        w = paths[p].path
        if not (mod.validate_batch(w[:1])[0] and mod.validate_motion_batch(w[:-1], w[1:]).all()):
            continue
        fk = mod.fk_batch(w[[0, -1]])
        d = np.linalg.norm(fk[1, :, :3] - fk[0, :, :3], axis=1)
        j = int(np.argmax(d))
        found.append((float(d[j]), int(p), fk[1, j, :3].copy()))
    for _, p, centre in sorted(found, key=lambda f: -f[0]):
        env = vamp.Environment()
        env.add_sphere(vamp.Sphere(centre, 0.02))
        if mod.validate_batch(paths[p].path[:1], env)[0]:
            return p, len(paths[p].path) - 1, env
    raise AssertionError("no completed line whose start is clear of the obstacle")


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_sphere_on_the_line_cuts_the_path(vamp, sets, robot):
    case, mod = sets[robot], sets[robot]["mod"]
    kin = case["kin"][False]
    p, k, env = moving_sphere(vamp, case, kin, C.fast_complete(robot))
    start, target = case["starts"][p:p + 1], case["targets"][p:p + 1]
    assert bool(mod.validate_batch(start, env)[0])  # the condition: the obstacle is clear of the start
    (r,) = vamp.planning.cartesian_multi(mod, start, target, [env])
    assert r.status == "collision" and r.achieved < k and r.segments == k
    w = kin[p].path
    assert np.array_equal(bits(r.path), bits(w[:r.achieved + 1]))  # the kinematics-only path, cut
    if r.achieved:
        assert mod.validate_motion_batch(r.path[:-1], r.path[1:], env).all()
    assert not bool(mod.validate_motion_batch(w[r.achieved:r.achieved + 1], w[r.achieved + 1:r.achieved + 2], env)[0])
    raw = mod.cartesian_multi_raw(start, target, [env], vamp.planning.CartesianSettings())
    assert raw["validation_calls"] == 2 and raw["questions"] == 1 + k


@pytest.mark.parametrize("robot", ROBOTS)
def test_invalid_start_and_no_environments(vamp, sets, robot):
    case, mod = sets[robot], sets[robot]["mod"]
    kin = case["kin"][False]
    n = len(kin)
    blocked = vamp.Environment()
    blocked.add_sphere(vamp.Sphere(mod.fk_batch(case["starts"][:1])[0, -1, :3], 0.3))
    envs = [blocked] + [None] * (n - 1)
    got = vamp.planning.cartesian_multi(mod, case["starts"], case["targets"], envs)
    assert got[0].status == "invalid_start" and got[0].achieved == 0 and got[0].segments == kin[0].segments
    assert np.array_equal(bits(got[0].path), bits(case["starts"][:1]))
    # in the empty environment only the robot itself can cut a path: what comes back is the kinematics-only path cut where
    # validate_batch and validate_motion_batch say so
    for p in range(1, n):
        g, w = got[p], kin[p]
        assert g.segments == w.segments
        if not mod.validate_batch(case["starts"][p:p + 1])[0]:
            want = ("invalid_start", 0)
        else:
            ok = mod.validate_motion_batch(w.path[:-1], w.path[1:]) if w.achieved else np.zeros(0, bool)
            cut = int(np.argmin(ok)) if not ok.all() else w.achieved
            want = ("collision", cut) if cut < w.achieved else (w.status, w.achieved)
        assert (g.status, g.achieved) == want, (case["names"][p], g.status, g.achieved, want)
        assert np.array_equal(bits(g.path), bits(w.path[:g.achieved + 1])) and g.evaluations == w.evaluations
    assert {"invalid_start"} < {g.status for g in got} and any(g.achieved for g in got)


# ---- 4. batch independence, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_problem_does_not_depend_on_its_batch(vamp, sets, robot):
    case, mod = sets[robot], sets[robot]["mod"]
    P = vamp.planning
    starts, targets = case["starts"], case["targets"]
    n = len(starts)
    far = []
    for _ in range(2):
        e = vamp.Environment()
        e.add_sphere(vamp.Sphere([0.0, 0.0, -5.0], 0.1))
        far.append(e)
    whole = P.cartesian_multi(mod, starts, targets, [far[0]] * n)
    alone = [P.cartesian_multi(mod, starts[p:p + 1], targets[p:p + 1], [far[0]])[0] for p in range(n)]
    assert same_paths(whole, alone)
    assert same_paths(whole, P.cartesian_multi(mod, starts[::-1], targets[::-1], [far[0]] * n)[::-1])
    assert same_paths(whole, P.cartesian_multi(mod, starts, targets, [far[0]] * (n // 2) + [far[1]] * (n - n // 2)))
    # the wave boundary: lines of different m side by side in batches of 1, 63, 64 and 65 lanes
    kin = case["kin"][False]
    for size in (1, 63, 64, 65):
        idx = (np.arange(size) * 7 + 3) % n
        assert same_paths([kin[p] for p in idx], P.cartesian_multi(mod, starts[idx], targets[idx])), size


# ---- 5. non-finite inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_non_finite_start_or_target(vamp, sets, robot):
    case, mod = sets[robot], sets[robot]["mod"]
    kin = case["kin"][False]
    starts, targets = case["starts"].copy(), case["targets"].copy()
    starts[3, 1], targets[5, 1, 3], targets[6, 0, 0] = np.nan, np.inf, np.nan
    got = vamp.planning.cartesian_multi(mod, starts, targets)
    for p in (3, 5, 6):
        assert got[p].status == "non_finite" and got[p].achieved == 0 and got[p].evaluations == 0
        assert np.array_equal(bits(got[p].path), bits(starts[p:p + 1]))
    keep = [p for p in range(len(kin)) if p not in (3, 5, 6)]
    assert same_paths([got[p] for p in keep], [kin[p] for p in keep])
    raw = mod.cartesian_multi_raw(starts[[3, 5]], targets[[3, 5]], [None, None], vamp.planning.CartesianSettings())
    assert raw["validation_calls"] == 0 and raw["questions"] == 0


def test_a_start_without_a_finite_frame_is_non_finite(vamp, sets):
    """a finite start of huge entries: eefk_batch's frame is not finite, so there is no line to set up"""
    case = sets["fetch"]  # (the torso is prismatic: the frame's position is the joint value itself)
    kin = case["kin"][False]
    starts = case["starts"].copy()
    starts[4, :] = 3e38
    assert not np.isfinite(case["mod"].eefk_batch(starts[4:5])).all()
    got = vamp.planning.cartesian_multi(case["mod"], starts, case["targets"], [None] * len(starts))
    assert (got[4].status, got[4].achieved, got[4].segments, got[4].evaluations) == ("non_finite", 0, 0, 0)
    assert np.array_equal(bits(got[4].path), bits(starts[4:5]))
    assert all((g.segments, g.evaluations) == (w.segments, w.evaluations) for p, (g, w) in enumerate(zip(got, kin)) if p != 4)


def test_points_refuses_a_buffer_that_is_too_small(vamp, sets):
    """vmv_cartesian_points on a live, non-empty result: one float short is VMV_ERR_CAPACITY and nothing is written"""
    import ctypes

    from vamp_mvt_amd import _lib

    case, L = sets["panda"], _lib.lib
    starts = np.ascontiguousarray(case["starts"][:5])
    targets = np.ascontiguousarray(case["targets"][:5]).reshape(5, 16)
    cs = _lib.CartesianSettings()  # zeros: every default
    out = ctypes.c_void_p()
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    assert L.vmv_cartesian_multi(vamp.robots.index("panda"), None, 5, fp(starts), fp(targets), ctypes.byref(cs), ctypes.byref(out)) == 0
    try:
        achieved = np.zeros(5, np.uint32)
        assert L.vmv_cartesian_summary(out, None, None, achieved.ctypes.data_as(_lib.c_u32_p), None, None, None) == 0
        size = (int(achieved.sum()) + 5) * 7
        assert size > 5 * 7  # (the result is not one of bare starts)
        sentinel = np.float32(-12345.5)
        buf = np.full(size + 1, sentinel, np.float32)
        for capacity in (0, 1, size - 1):
            assert L.vmv_cartesian_points(out, fp(buf), capacity) == 4  # VMV_ERR_CAPACITY
            assert (buf == sentinel).all()
        assert L.vmv_cartesian_points(out, None, size) == 1  # VMV_ERR_INVALID_ARGUMENT: a NULL buffer for a non-empty result
        assert L.vmv_cartesian_points(out, fp(buf), size) == 0
        want = np.concatenate([r.path for r in case["kin"][False][:5]])
        assert np.array_equal(bits(buf[:size].reshape(-1, 7)), bits(want)) and buf[size] == sentinel
    finally:
        assert L.vmv_cartesian_destroy(out) == 0


@pytest.mark.parametrize("robot", ROBOTS)
def test_too_long(vamp, sets, robot):
    case, mod = sets[robot], sets[robot]["mod"]
    kin = case["kin"][False]
    cap = 12
    got = vamp.planning.cartesian_multi(mod, case["starts"], case["targets"], None, vamp.planning.CartesianSettings(max_waypoints=cap))
    assert any(w.segments + 1 > cap for w in kin) and any(w.segments + 1 <= cap for w in kin)
    for g, w, q in zip(got, kin, case["starts"]):
        if w.segments + 1 > cap:
            assert (g.status, g.achieved, g.segments) == ("too_long", 0, w.segments) and np.array_equal(bits(g.path), bits(q[None]))
        else:
            assert same_paths([g], [w])


# ---- 6. the use: straight approaches ---------------------------------------------------------------------------------------
def test_approach_multi_on_the_panda(vamp):
    mod, P = vamp.panda, vamp.planning
    cfg = K.halton32("panda", 64, 300)
    cfg = cfg[mod.validate_batch(cfg)][:8]
    assert len(cfg) == 8
    targets = mod.eefk_batch(cfg)  # 8 reachable grasp poses in open space
    s = P.CartesianSettings()
    out = P.approach_multi(mod, targets, None, 0.08)
    goal_sets, _ = P.ik_goals(mod, P.approach_poses(targets, 0.08), None)
    print("complete approaches per target:", [len(a.paths) for a in out], "of goals", [len(g) for g in goal_sets])
    assert len(out) == 8 and sum(len(a.paths) for a in out) >= 1  # (the checks below are not vacuous)
    for p, a in enumerate(out):
        assert len(a.goals) == len(a.paths) and a.goals.dtype == np.float32
        for g, w in zip(a.goals, a.paths):
            assert np.array_equal(bits(g), bits(w[0])) and any(np.array_equal(bits(g), bits(h)) for h in goal_sets[p])
            n_p, n_w, tr = K.residuals("panda", w[-1:].astype(np.float64), targets[p:p + 1])
            assert n_p[0] <= s.pos_tol + FRAME_SLACK and n_w[0] <= s.rot_tol + FRAME_SLACK and tr[0] > 1.0
            assert mod.validate_motion_batch(w[:-1], w[1:]).all()
