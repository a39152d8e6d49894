"""vmv_cartesian_multi / planning.cartesian_multi / planning.approach_multi: what holds without a device - the float64
statement (tests/cartesian_serial.py) checked against itself, the conditions on the shared case set that the device tests
(tests/test_cartesian_gpu.py) rest on, the ABI's checks that come before any device query, the Python wrappers' argument
checks and arithmetic, and the host line set-up and cut under sanitizers (tests/native/cartesian_sanitize.cc)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cartesian_serial as C
import ik_serial as K

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE = 0, 1, 2
VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 5, 6
NAMES = ("vmv_cartesian_multi", "vmv_cartesian_summary", "vmv_cartesian_points", "vmv_cartesian_destroy")
SENTINEL = 0x5A5A5A5A
FIELDS = ("pos_step", "rot_step", "max_iterations", "pos_tol", "rot_tol", "rot_weight", "damping", "max_step",
          "max_joint_step", "max_waypoints", "position_only")
DEFAULTS = dict(pos_step=0.01, rot_step=0.05, max_iterations=16, pos_tol=1e-4, rot_tol=1e-3, rot_weight=0.25, damping=1e-2,
                max_step=0.5, max_joint_step=0.3, max_waypoints=1024, position_only=False)


# ---- the serial statement against itself -----------------------------------------------------------------------------------
def test_pose_m_of_a_line_is_the_target():
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = rng.normal(size=3), rng.normal(size=3)
        T0, T1 = np.eye(4), np.eye(4)
        T0[:3, :3], T0[:3, 3] = C.rot(a / np.linalg.norm(a), rng.uniform(0, 3.1)), rng.uniform(-1, 1, 3)
        T1[:3, :3], T1[:3, 3] = C.rot(b / np.linalg.norm(b), rng.uniform(0, 3.1)), rng.uniform(-1, 1, 3)
        line = C.line(T0, T1, C.Settings())
        assert np.abs(line.pose(line.m) - T1).max() <= 1e-12
        assert np.abs(line.pose(0) - T0).max() <= 1e-12
        assert line.m == max(1, int(np.ceil(np.linalg.norm(T1[:3, 3] - T0[:3, 3]) / 0.01)), int(np.ceil(line.theta / 0.05)))
        half = line.pose(line.m // 2 or 1)[:3, :3]
        assert np.abs(half @ half.T - np.eye(3)).max() <= 1e-12  # every pose is a frame


@pytest.mark.parametrize("theta", (0.0, 1e-4, 1.0, 3.0, np.pi))
def test_axis_and_angle_round_trip(theta):
    for axis in ((0, 0, 1), (1, 0, 0), (0.6, 0.0, -0.8), (1 / np.sqrt(3),) * 3, (-0.48, 0.6, 0.64)):
        a, t = C.axis_angle(C.rot(axis, theta))
        assert abs(t - theta) <= 1e-9
        if theta > 0.0:
            d = float(np.dot(a, axis))
            assert (abs(d) if theta == np.pi else d) >= 1.0 - 1e-9
        assert abs(np.linalg.norm(a) - 1.0) <= 1e-12
        assert np.abs(C.rot(a, t) - C.rot(axis, theta)).max() <= 1e-9


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_a_line_to_the_starts_own_frame_is_one_segment_and_completes(robot):
    starts, targets, names = C.cases(robot)
    p = names.index("zero_motion")
    r = C.tracked(robot)
    assert r["lines"][p].m == 1 and r["status"][p] == "complete" and r["achieved"][p] == 1
    p = names.index("pure_rotation")
    assert r["lines"][p].ratios[0] < 1e-3 and r["lines"][p].m == int(np.ceil(0.2613 / 0.05))


# ---- the conditions the device tests rest on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", C.ROBOTS)
def test_conditions_on_the_shared_case_set(robot):
    """At least half of the lines complete with every waypoint within max_iterations / 2 evaluations; at least 3 fail
    ik_failed because the line leaves the reach; no quotient under a ceil is within 1e-3 of an integer.

    "Leaves the reach" is cartesian_serial.left_reach: from the last waypoint, 64 evaluations towards the line's END still
    miss it by more than 5 cm.  The residual AT the failing waypoint cannot reach 5 cm with pos_step = 1 cm - the pose is one
    step from one that was reached and the iteration never accepts a worse state (measured: at most 7 mm over the four
    sets) - so the 5 cm is asked of the line's end instead."""
    starts, targets, names = C.cases(robot)
    n = len(starts)
    assert n == C.N_STARTS + 5 and targets.shape == (n, 4, 4) and targets.dtype == np.float32 and starts.dtype == np.float32
    r = C.tracked(robot)
    fast, left = C.fast_complete(robot), C.left_reach(robot)
    failed = r["status"] == "ik_failed"
    print(robot, "complete within 8:", int(fast.sum()), "of", n, "| left the reach:", int(left.sum()),
          "| largest residual at a failing waypoint:", float(np.nanmax(np.where(failed, r["fail_residual"], np.nan))))
    assert 2 * int(fast.sum()) >= n
    assert int(left.sum()) >= 3
    assert np.nanmax(np.where(failed, r["fail_residual"], np.nan)) <= C.Settings().pos_step + 1e-3
    for p, line in enumerate(r["lines"]):
        for x in line.ratios:
            assert abs(x - round(x)) >= 1e-3 or x < 1e-3, (names[p], x)  # (a zero quotient asks for no segment at all)
    # m from the float64 tape's frames (not rounded to fp32) is the same
    exact = K.frames44(robot, starts)
    assert [C.line(exact[p], targets[p], C.Settings()).m for p in range(n)] == [line.m for line in r["lines"]]
    # the halton lines are 5 - 25 cm long and turn by at most 0.3 rad
    for p in range(C.N_STARTS):
        assert 0.05 <= np.linalg.norm(r["lines"][p].dp) <= 0.26 and r["lines"][p].theta <= 0.32
    assert 2 * int(C.robust(robot, True).sum()) >= n  # the position_only run of the device test has its half as well


# ---- the ABI without a device --------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert vamp.abi_version() == 1  # the change is additive
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.cartesian_multi) and callable(robot.cartesian_multi_raw)
    s = planning.CartesianSettings()
    assert {k: getattr(s, k) for k in DEFAULTS} == DEFAULTS
    assert {k: getattr(C.Settings(), k) for k in DEFAULTS} == DEFAULTS  # the statement's defaults are the call's
    assert planning.CARTESIAN_STATUS == C.STATUS
    assert tuple(f[0] for f in _lib.CartesianSettings._fields_) == FIELDS and ctypes.sizeof(_lib.CartesianSettings) == 44


@pytest.fixture()
def raw(vamp):
    """-> (_lib, make): make() creates an unfinalized C environment (no device needed); all destroyed afterwards"""
    from vamp_mvt_amd import _lib

    handles = []

    def make():
        h = ctypes.c_void_p()
        assert _lib.lib.vmv_env_create(ctypes.byref(h)) == 0
        handles.append(h.value)
        return h.value

    yield _lib, make
    for h in handles:
        _lib.lib.vmv_env_destroy(h)


def _call(_lib, handles, robot=0, n=2, drop=(), **settings):
    """one vmv_cartesian_multi call with two problems; handles None: envs == NULL; `drop` names the pointers passed as NULL
    -> (status, *out)"""
    starts = np.zeros((2, 16), np.float32)
    targets = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (2, 1))
    s = dict.fromkeys(FIELDS, 0)
    s.update(settings)
    cs = _lib.CartesianSettings(*[s[k] for k in FIELDS])
    out = ctypes.c_void_p(SENTINEL)
    ptr = {"envs": None if handles is None else (ctypes.c_void_p * max(len(handles), 1))(*handles),
           "starts": starts.ctypes.data_as(_lib.c_float_p), "targets": targets.ctypes.data_as(_lib.c_float_p),
           "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_cartesian_multi(robot, ptr["envs"], n, ptr["starts"], ptr["targets"], ptr["settings"], ptr["out"])
    return rc, out.value


def test_unknown_robot(raw):
    _lib, make = raw
    for robot in (-1, 4, 7):
        assert _call(_lib, [make(), make()], robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
        assert _call(_lib, None, robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)


@pytest.mark.parametrize("drop", ["starts", "targets", "settings", "out"])
def test_null_pointers(raw, drop):
    _lib, make = raw
    assert _call(_lib, [make(), make()], drop=(drop,)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, None, drop=(drop,)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_null_handle_and_unfinalized_environment(raw):
    _lib, make = raw
    a = make()
    assert _call(_lib, [a, None]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, [None, a]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, [a, make()]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert b"envs[0] is not finalized" in _lib.lib.vmv_last_error()  # the multi-environment prologue's own message
    assert _call(_lib, [a, a]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed


@pytest.mark.parametrize("name", ["pos_step", "rot_step", "pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "max_joint_step"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_settings_are_refused(raw, name, value):
    _lib, _ = raw
    assert _call(_lib, None, **{name: value}) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_out_of_range_settings_are_refused(raw):
    _lib, make = raw
    for kw in (dict(max_waypoints=1025), dict(max_waypoints=2 ** 32 - 1), dict(max_iterations=2 ** 30), dict(position_only=2),
               dict(position_only=-1)):
        assert _call(_lib, None, **kw) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
        assert _call(_lib, [make(), make()], **kw) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # before the handles are looked at
    assert _call(_lib, None, n=2 ** 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_no_problems_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    for handles in (None, []):
        rc, res = _call(_lib, handles, n=0)
        assert rc == VMV_OK and res not in (None, SENTINEL)
        calls, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert L.vmv_cartesian_summary(res, None, None, None, None, ctypes.byref(calls), ctypes.byref(questions)) == VMV_OK
        assert (calls.value, questions.value) == (0, 0)
        assert L.vmv_cartesian_points(res, None, 0) == VMV_OK
        assert L.vmv_cartesian_destroy(res) == VMV_OK
    assert L.vmv_cartesian_summary(None, None, None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_cartesian_points(None, None, 0) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_cartesian_destroy(None) == VMV_ERR_INVALID_ARGUMENT
    assert planning.cartesian_multi(vamp.panda, np.zeros((0, 7)), np.zeros((0, 4, 4))) == []
    assert vamp.panda.cartesian_multi(np.zeros((0, 7)), np.zeros((0, 4, 4)), []) == []
    raw = vamp.panda.cartesian_multi_raw(np.zeros((0, 7)), np.zeros((0, 16)), None, planning.CartesianSettings())
    assert raw["points"].shape == (0, 7) and list(raw["offsets"]) == [0] and raw["questions"] == 0


def test_well_formed_call_fails_loudly_without_a_device(vamp):
    from vamp_mvt_amd import planning

    if vamp.device_count() == 0:  # there is no CPU fallback
        for envs in (None, [None]):
            with pytest.raises(vamp.VmvError) as ei:
                planning.cartesian_multi(vamp.panda, np.zeros((1, 7)), np.eye(4)[None], envs)
            assert ei.value.status == VMV_ERR_NO_DEVICE


# ---- the Python wrappers ---------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    q, T = np.zeros((3, 7), np.float32), np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.CartesianSettings

    def f(*args, **kw):
        return planning.cartesian_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f(q, T, [env, None])  # two environments for three problems
    with pytest.raises(TypeError):
        f(np.zeros((3, 6), np.float32), T)  # wrong dimension
    with pytest.raises(TypeError):
        f(q[0], T[:1])  # one start still is a [1][dim] array
    with pytest.raises(TypeError):
        f(q, T[:2])  # a target per start
    with pytest.raises(TypeError):
        f(q, np.zeros((3, 3, 4), np.float32))  # frames are 4 x 4
    with pytest.raises(TypeError):
        f(q, T, [env, None, "not an environment"])
    for kw in (dict(pos_step=float("nan")), dict(rot_step=float("inf")), dict(max_joint_step=float("-inf")), dict(max_waypoints=1025),
               dict(max_waypoints=-1), dict(max_iterations=2 ** 30), dict(max_iterations=-1), dict(damping=float("nan"))):
        with pytest.raises(ValueError):
            f(q, T, None, S(**kw))
    with pytest.raises(ValueError):
        vamp.panda.cartesian_multi(q, T, [env], S())  # the installed name takes the same road
    with pytest.raises(ValueError):
        planning.approach_multi(vamp.panda, T, None, 0.0)
    with pytest.raises(ValueError):
        planning.approach_multi(vamp.panda, T, None, 0.1, axis=(0, 0, 0))
    with pytest.raises(TypeError):
        planning.approach_multi(vamp.panda, np.zeros((3, 3, 3)), None, 0.1)
    assert env._handle is None  # nothing was built or finalized


class _Recorder:
    """stands in for <robot>: records what planning hands cartesian_multi_raw and answers with a canned result"""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def dimension(self):
        return 7

    def cartesian_multi_raw(self, *args):
        self.calls.append(args)
        return self.answer


def test_results_and_fraction(vamp):
    from vamp_mvt_amd import planning

    raw = dict(status=np.array([0, 1, 5, 6, 3], np.uint8), segments=np.array([3, 4, 2000, 0, 8], np.uint32),
               achieved=np.array([3, 1, 0, 0, 0], np.uint32), evaluations=np.array([9, 20, 0, 0, 17], np.uint32),
               points=np.arange(9 * 7, dtype=np.float32).reshape(9, 7), offsets=np.array([0, 4, 6, 7, 8, 9]),
               validation_calls=2, questions=12)
    robot = _Recorder(raw)
    s = planning.CartesianSettings(pos_step=0.02)
    out = planning.cartesian_multi(robot, "starts", "targets", "envs", s)
    assert robot.calls == [("starts", "targets", "envs", s)]
    assert [r.status for r in out] == ["complete", "ik_failed", "too_long", "non_finite", "collision"]
    assert [r.fraction for r in out] == [1.0, 0.25, 0.0, 0.0, 0.0] and [r.complete for r in out] == [True] + [False] * 4
    assert [len(r.path) for r in out] == [4, 2, 1, 1, 1] and [r.evaluations for r in out] == [9, 20, 0, 0, 17]
    assert np.array_equal(out[1].path, raw["points"][4:6]) and out[1].path.base is not raw["points"]
    planning.cartesian_multi(robot, "a", "b")
    assert robot.calls[-1][2] is None and robot.calls[-1][3] == planning.CartesianSettings()


def test_approach_pre_pose_algebra(vamp):
    from vamp_mvt_amd import planning

    rng = np.random.default_rng(5)
    T = np.tile(np.eye(4), (6, 1, 1))
    for p in range(6):
        a = rng.normal(size=3)
        T[p, :3, :3], T[p, :3, 3] = C.rot(a / np.linalg.norm(a), rng.uniform(0, 3)), rng.uniform(-1, 1, 3)
    for axis, d in (((0, 0, 1), 0.1), ((0, 0, 2), 0.1), ((1, 0, 0), 0.05), ((0.6, 0.0, -0.8), 0.2)):
        u = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        back = np.eye(4)
        back[:3, 3] = -d * u
        pre = planning.approach_poses(T, d, axis)
        assert pre.shape == (6, 4, 4) and pre.dtype == np.float32
        assert np.abs(pre - T @ back).max() <= 1e-6  # target . translate(-distance * axis), rounded to fp32
        assert np.array_equal(pre[:, :3, :3], T[:, :3, :3].astype(np.float32))  # the orientation is the target's
        # the approach is a straight line of `distance` along the tool axis, without rotation
        line = C.line(pre[0], T[0].astype(np.float32), C.Settings())
        assert abs(np.linalg.norm(line.dp) - d) <= 1e-6 and line.theta <= 1e-6
        assert np.abs(line.dp / np.linalg.norm(line.dp) - T[0, :3, :3] @ u).max() <= 1e-5
    assert np.array_equal(planning.approach_poses(T.reshape(6, 16), 0.1), planning.approach_poses(T, 0.1))


def test_approach_multi_composes_ik_goals_and_cartesian_multi(vamp, monkeypatch):
    """one ik_goals call over the pre-poses, one cartesian_multi call from every goal to its target, complete ones kept"""
    from vamp_mvt_amd import planning

    T = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    T[:, 2, 3] = (0.5, 0.6, 0.7)
    goals = [np.full((2, 7), 1.0, np.float32), np.zeros((0, 7), np.float32), np.full((1, 7), 3.0, np.float32)]
    goals[0][1] = 2.0
    seen = {}

    def ik_goals(robot, targets, envs, settings=None):
        seen["ik"] = (targets.copy(), list(envs), settings)
        return goals, [1]

    def cartesian_multi(robot, starts, targets, environments=None, settings=None):
        seen["cart"] = (starts.copy(), targets.copy(), list(environments), settings)
        status = ["complete", "ik_failed", "complete"]
        return [planning.CartesianPath(np.stack([q, q + 1]), st, 1, int(st == "complete"), float(st == "complete"), 2)
                for q, st in zip(starts, status)]

    monkeypatch.setattr(planning, "ik_goals", ik_goals)
    monkeypatch.setattr(planning, "cartesian_multi", cartesian_multi)
    out = planning.approach_multi(vamp.panda, T, ["e0", "e1", "e2"], 0.1, ik_settings="iks", settings="cs")
    assert np.array_equal(seen["ik"][0], planning.approach_poses(T, 0.1)) and seen["ik"][1:] == (["e0", "e1", "e2"], "iks")
    assert np.array_equal(seen["cart"][0], np.concatenate(goals)) and np.array_equal(seen["cart"][1], T[[0, 0, 2]])
    assert seen["cart"][2:] == (["e0", "e0", "e2"], "cs")
    assert [len(a.goals) for a in out] == [1, 0, 1] and [len(a.paths) for a in out] == [1, 0, 1]
    assert np.array_equal(out[0].goals, goals[0][:1]) and np.array_equal(out[2].goals, goals[2])
    assert np.array_equal(out[2].paths[0], np.stack([goals[2][0], goals[2][0] + 1]))
    assert all(a.goals.shape[1] == 7 and a.goals.dtype == np.float32 for a in out)


def test_serial_statement_does_not_import_the_package():
    code = "import sys; sys.path.insert(0, %r); import cartesian_serial; assert 'vamp_mvt_amd' not in sys.modules" % os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call([os.sys.executable, "-c", code])


# ---- the host line set-up and cut under sanitizers ----------------------------------------------------------------------------
def test_host_line_setup_and_cut_under_sanitizers():
    out = os.path.join(ROOT, "build", "cartesian_sanitize")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "cartesian_sanitize.cc"), "-o", out, "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
