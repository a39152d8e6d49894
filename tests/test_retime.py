"""vmv_retime_multi without a device: the statement (tests/retime_serial.py) against closed forms and a linear programme,
the limits it keeps, the conditions on the shared case set that tests/test_retime_gpu.py rests on, the ABI's refusals, the
Python wrappers, and the host set-up under sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import retime_serial as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_CAPACITY, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 4, 5, 6
SENTINEL = 0x5A5A5A5A
NAMES = ("vmv_retime_multi", "vmv_retime_summary", "vmv_retime_samples", "vmv_retime_destroy")
FIELDS = ("blend", "grid_step", "dt", "max_grid", "max_samples", "stop_at_waypoints")
DEFAULTS = dict(blend=0.1, grid_step=0.02, dt=0.01, max_grid=4096, max_samples=65536, stop_at_waypoints=False)
# Measured here on the CPU over the whole case set of all four robots (DESIGN.md 5n records them):
#   the float64 twin's duration of a straight line over the closed form: at most 1 + 5.95e-4 (15 intervals), never below 1;
#   the fp32 statement's |qddot_j| / A_j on 8 sub-samples per interval: at most 1 + 2.06e-6; |qdot_j| / V_j at the grid
#   points: at most 1 + 9.9e-8.
LINE_BAR = 1 + 2 * 5.95e-4  # twice the measured excess
ACC_BAR = 1 + 4 * 2.06e-6   # four times the measured excess, below 1e-4
VEL_BAR = 1 + 4 * 9.9e-8


# ---- the statement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", R.ROBOTS)
def test_straight_lines_take_the_closed_forms_time(robot):
    V, A = R.limits(robot)
    seen = 0
    for (name, w), r in zip(R.cases(robot), R.results(robot, dtype=np.float64)):
        if len(w) != 2 or r.status != "complete" or r.samples < 2:
            continue
        ratio = float(r.duration) / R.line_time(w[0], w[1], V, A)
        print(f"{robot} {name}: {r.intervals} intervals, duration / closed form = {ratio:.7f}")
        assert 1.0 - 1e-12 <= ratio <= LINE_BAR, (name, ratio)
        seen += 1
    assert seen >= 8


def test_controllable_sets_against_a_linear_programme():
    from scipy.optimize import linprog

    V, A = R.limits("panda")
    results = dict(zip((n for n, _ in R.cases("panda")), R.results("panda", dtype=np.float64)))
    checked = 0
    for name in ("right_angle", "bspline_40", "random_4"):
        pr = results[name].profile
        N = len(pr.k)
        for i in np.linspace(0, N - 1, 20).astype(int):
            rows, rhs = [], []  # over (x, u): maximise x
            for s, g in zip(pr.slope[i][pr.line[i]], pr.g[i][pr.line[i]]):
                rows += [[-s, 1.0], [s, -1.0]]  # |u - s x| <= g
                rhs += [g, g]
            rows += [[-1.0, -pr.two_d[i]], [1.0, pr.two_d[i]]]  # 0 <= x + 2 Delta u <= K_{i+1}
            rhs += [0.0, pr.K[i + 1]]
            top = min(float(pr.cap[i].min()), float(pr.xv[i]))
            res = linprog([-1.0, 0.0], A_ub=np.array(rows), b_ub=np.array(rhs), bounds=[(0.0, top if np.isfinite(top) else None), (None, None)],
                          method="highs")
            assert res.status == 0, (name, i, res.message)
            assert abs(pr.K[i] - res.x[0]) <= 1e-9 * max(1.0, abs(res.x[0])), (name, i, pr.K[i], res.x[0])
            checked += 1
    assert checked == 60


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_the_fp32_statement_keeps_the_limits(robot):
    V, A = R.limits(robot)
    worst_v = worst_a = 0.0
    for stop in (False, True):
        for (name, _), r in zip(R.cases(robot), R.results(robot, stop_at_waypoints=stop)):
            if r.status != "complete" or r.samples < 2:
                continue
            rv, ra = R.limit_ratios(r, V, A, sub=8)
            worst_v, worst_a = max(worst_v, rv), max(worst_a, ra)
            assert rv <= VEL_BAR and ra <= ACC_BAR, (name, stop, rv, ra)
    print(f"{robot}: worst |qdot| / V at the grid points {worst_v:.9f}, worst |qddot| / A on 8 sub-samples {worst_a:.9f}")
    assert ACC_BAR - 1 < 1e-4


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_conditions_on_the_shared_case_set(robot):
    V, A = R.limits(robot)
    cases, res, stopped = R.cases(robot), R.results(robot), R.results(robot, stop_at_waypoints=True)
    names = [n for n, _ in cases]
    assert 24 <= len(cases) <= 32 and names != sorted(names)  # shuffled
    by = dict(zip(names, res))
    assert sum(r.profile.vel_binds for r in res if r.profile is not None) >= 6
    assert sum(r.profile.acc_binds for r in res if r.profile is not None) >= 6
    assert not any(r.status == "stalled" for r in res + stopped)
    assert by["at_max_grid"].intervals == R.CASE_SETTINGS.max_grid and by["at_max_grid"].status == "complete"
    assert by["over_max_grid"].intervals == R.CASE_SETTINGS.max_grid + 1 and by["over_max_grid"].status == "too_long"
    assert [by[f"intervals_{k}"].intervals for k in (63, 64, 65)] == [63, 64, 65] and by["line_1mm"].intervals == 2
    assert 950 <= by["intervals_1100"].intervals <= R.CASE_SETTINGS.max_grid and by["intervals_1100"].status == "complete"
    assert by["nan_waypoint"].status == by["inf_waypoint"].status == "non_finite"
    assert (by["no_waypoints"].samples, by["one_waypoint"].samples, by["one_waypoint_thrice"].samples) == (0, 1, 1)
    assert by["line_cap"].profile.vel_binds and not by["line_no_cap"].profile.vel_binds
    assert (by["collinear"].pieces.d > 0).any() and np.abs(by["collinear"].profile.c).max() < 1e-5  # a blend with q'' = 0 up to the waypoints' rounding
    rev = by["reversal"]
    assert np.array_equal(rev.pieces.u_out[rev.pieces.d > 0], -rev.pieces.u_in[rev.pieces.d > 0])  # an exact reversal
    short = by["short_segments"].pieces.d
    assert (short > 0).sum() >= 4 and (short < 0.9 * R.CASE_SETTINGS.blend).all()  # every blend is cut by its segments
    assert (by["bspline_40"].pieces.span < 1e-6).any()  # with slivers of lines between them
    assert np.count_nonzero(by["joint_0_alone"].pieces.u_in[0]) == 1 and by["joint_0_alone"].pieces.u_in[0][0] != 0
    # no quotient under a ceil lies within 1e-3 of an integer (a span below two grid steps has two intervals whatever
    # its quotient, so only quotients from 2 - 1e-3 on can decide anything)
    for (name, _), r, s in zip(cases, res, stopped):
        if r.status != "complete" or r.samples < 2:
            continue
        q = [v for v in r.pieces.quotients + s.pieces.quotients if v > 2 - 1e-3]
        q += [R.sample_quotient(r.duration, dt) for dt in (0.01, 0.001, 0.05)] + [R.sample_quotient(s.duration, 0.01)]
        assert min(abs(v - round(v)) for v in q) > 1e-3, name
        if len(r.pieces.n) > 1 or len(s.pieces.n) > 1:  # blends make every multi-waypoint path faster
            assert r.duration < s.duration, (name, r.duration, s.duration)


def test_serial_statement_does_not_import_the_package():
    code = "import sys; sys.path.insert(0, %r); import retime_serial; assert 'vamp_mvt_amd' not in sys.modules" % os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call([os.sys.executable, "-c", code])


# ---- the ABI without a device ----------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert vamp.abi_version() == 1  # the change is additive
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.retime_multi) and callable(robot.retime_multi_raw)
    s = planning.RetimeSettings()
    assert {k: getattr(s, k) for k in DEFAULTS} == DEFAULTS
    assert {k: getattr(R.Settings(), k) for k in DEFAULTS} == DEFAULTS  # the statement's defaults are the call's
    assert planning.RETIME_STATUS == R.STATUS
    assert tuple(f[0] for f in _lib.RetimeSettings._fields_) == FIELDS and ctypes.sizeof(_lib.RetimeSettings) == 24
    header = open(_lib.HEADER_PATH).read()  # the C struct's defaults are the same
    for text in ("default (0.1)", "default (0.02)", "default (0.01)", "default (4,096)", "default (65,536)"):
        assert text in header


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


def _call(_lib, handles, robot=0, n=2, drop=(), offsets=(0, 2, 4), vel=None, acc=None, **settings):
    """one vmv_retime_multi call with two two-waypoint paths; handles None: envs == NULL; `drop` names the pointers passed
    as NULL -> (status, *out, vmv_last_error())"""
    points = np.zeros((4, 16), np.float32)
    points[1::2] = 0.5
    off = np.array(offsets, np.uintp)
    v = np.ones(16, np.float32) if vel is None else np.asarray(vel, np.float32)
    a = np.ones(16, np.float32) if acc is None else np.asarray(acc, np.float32)
    s = dict.fromkeys(FIELDS, 0)
    s.update(settings)
    cs = _lib.RetimeSettings(*[s[k] for k in FIELDS])
    out = ctypes.c_void_p(SENTINEL)
    ptr = {"envs": None if handles is None else (ctypes.c_void_p * max(len(handles), 1))(*handles),
           "points": points.ctypes.data_as(_lib.c_float_p), "offsets": off.ctypes.data_as(_lib.c_size_p),
           "vel_limits": v.ctypes.data_as(_lib.c_float_p), "acc_limits": a.ctypes.data_as(_lib.c_float_p),
           "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_retime_multi(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["vel_limits"], ptr["acc_limits"],
                                   ptr["settings"], ptr["out"])
    return rc, out.value, _lib.lib.vmv_last_error().decode()


def refused(result, word):
    rc, out, message = result
    return rc == VMV_ERR_INVALID_ARGUMENT and out == SENTINEL and word in message


def test_unknown_robot(raw):
    _lib, make = raw
    for robot in (-1, 4, 7):
        assert _call(_lib, [make(), make()], robot=robot)[:2] == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
        assert _call(_lib, None, robot=robot)[:2] == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)


@pytest.mark.parametrize("drop", ["points", "offsets", "vel_limits", "acc_limits", "settings", "out"])
def test_null_pointers_are_refused_by_name(raw, drop):
    _lib, make = raw
    assert refused(_call(_lib, [make(), make()], drop=(drop,)), drop)
    assert refused(_call(_lib, None, drop=(drop,)), drop)


def test_offsets_are_checked(raw):
    _lib, _ = raw
    assert refused(_call(_lib, None, offsets=(0, 3, 2)), "offsets")
    assert refused(_call(_lib, None, offsets=(1, 2, 4)), "offsets[0]")
    assert refused(_call(_lib, None, n=2 ** 31), "n is")


@pytest.mark.parametrize("which", ["vel_limits", "acc_limits"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), 0.0, -1.0])
def test_limits_must_be_finite_and_positive(raw, which, value):
    _lib, _ = raw
    limits = np.ones(16, np.float32)
    limits[6] = value  # the Panda's last joint
    kw = {"vel" if which == "vel_limits" else "acc": limits}
    assert refused(_call(_lib, None, **kw), which + "[6]")
    limits[6], limits[7] = 1.0, value  # beyond the robot's joints nothing is read
    assert _call(_lib, None, **kw)[0] != VMV_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", ["blend", "grid_step", "dt"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_settings_are_refused_by_name(raw, name, value):
    _lib, _ = raw
    assert refused(_call(_lib, None, **{name: value}), name)


def test_out_of_range_settings_are_refused(raw):
    _lib, make = raw
    for kw, word in ((dict(grid_step=9e-7), "grid_step"), (dict(dt=9e-7), "dt"), (dict(max_grid=4097), "max_grid"),
                     (dict(stop_at_waypoints=2), "stop_at_waypoints"), (dict(stop_at_waypoints=-1), "stop_at_waypoints")):
        assert refused(_call(_lib, None, **kw), word)
        assert refused(_call(_lib, [make(), make()], **kw), word)  # before the handles are looked at
    for kw in (dict(grid_step=1e-6), dict(dt=1e-6), dict(max_grid=4096), dict(blend=-1.0), dict(grid_step=-1.0), dict(dt=-1.0)):
        assert _call(_lib, None, **kw)[0] != VMV_ERR_INVALID_ARGUMENT  # (accepted: fails later for want of a device, or runs)


def test_null_handle_and_unfinalized_environment(raw):
    _lib, make = raw
    a = make()
    assert _call(_lib, [a, None])[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, [None, a])[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    rc, out, message = _call(_lib, [a, make()])
    assert (rc, out) == (VMV_ERR_NOT_FINALIZED, SENTINEL) and "envs[0] is not finalized" in message
    assert _call(_lib, [a, a])[:2] == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed


def test_no_paths_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    for handles in (None, []):
        rc, res, _ = _call(_lib, handles, n=0)
        assert rc == VMV_OK and res not in (None, SENTINEL)
        calls, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert L.vmv_retime_summary(res, None, None, None, None, None, ctypes.byref(calls), ctypes.byref(questions)) == VMV_OK
        assert (calls.value, questions.value) == (0, 0)
        assert L.vmv_retime_samples(res, None, None, None, None, 0) == VMV_OK
        assert L.vmv_retime_destroy(res) == VMV_OK
    assert L.vmv_retime_summary(None, None, None, None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_retime_samples(None, None, None, None, None, 0) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_retime_destroy(None) == VMV_ERR_INVALID_ARGUMENT
    ones = np.ones(7)
    assert planning.retime_multi(vamp.panda, [], ones, ones) == []
    assert vamp.panda.retime_multi([], ones, ones, []) == []
    raw = vamp.panda.retime_multi_raw([], ones, ones, None, planning.RetimeSettings())
    assert raw["positions"].shape == (0, 7) and list(raw["offsets"]) == [0] and raw["questions"] == 0


def test_well_formed_call_fails_loudly_without_a_device(vamp):
    from vamp_mvt_amd import planning

    if vamp.device_count() == 0:  # there is no CPU fallback
        for envs in (None, [None]):
            with pytest.raises(vamp.VmvError) as ei:
                planning.retime_multi(vamp.panda, [np.zeros((2, 7)) + [[0], [1]]], np.ones(7), np.ones(7), envs)
            assert ei.value.status == VMV_ERR_NO_DEVICE


# ---- the Python wrappers ---------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    paths = [np.zeros((3, 7), np.float32), np.ones((2, 7), np.float32), []]
    ones = np.ones(7, np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.RetimeSettings

    def f(*args, **kw):
        return planning.retime_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f(paths, ones, ones, [env, None])  # two environments for three paths
    with pytest.raises(TypeError):
        f([np.zeros((3, 6), np.float32)], ones, ones)  # wrong dimension
    with pytest.raises(TypeError):
        f(paths, np.ones(6), ones)
    with pytest.raises(TypeError):
        f(paths, ones, np.ones((7, 1)))
    with pytest.raises(TypeError):
        f(paths, ones, ones, [env, None, "not an environment"])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        limits = ones.copy()
        limits[3] = bad
        with pytest.raises(ValueError):
            f(paths, limits, ones)
        with pytest.raises(ValueError):
            f(paths, ones, limits)
    for kw in (dict(blend=float("nan")), dict(grid_step=float("inf")), dict(dt=float("-inf")), dict(grid_step=5e-7), dict(dt=5e-7),
               dict(max_grid=4097), dict(max_grid=-1), dict(max_samples=-1), dict(max_samples=2 ** 32)):
        with pytest.raises(ValueError):
            f(paths, ones, ones, None, S(**kw))
    with pytest.raises(ValueError):
        vamp.panda.retime_multi(paths, ones, ones, [env], S())  # the installed name takes the same road
    assert env._handle is None  # nothing was built or finalized


class _Recorder:
    """stands in for <robot>: records what planning hands retime_multi_raw and answers with a canned result"""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def retime_multi_raw(self, *args):
        self.calls.append(args)
        return self.answer


def test_results_are_cut_from_the_packed_arrays(vamp):
    from vamp_mvt_amd import planning

    raw = dict(status=np.array([0, 1, 2, 3, 4, 0], np.uint8), intervals=np.array([5, 9, 5000, 0, 7, 0], np.uint32),
               samples=np.array([4, 3, 0, 0, 0, 1], np.uint32), duration=np.array([0.03, 0.02, 0, 0, 0, 0], np.float32),
               first_invalid=np.array([0xffffffff, 1, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff], np.uint32),
               times=np.arange(8, dtype=np.float32), positions=np.arange(56, dtype=np.float32).reshape(8, 7),
               velocities=np.arange(56, dtype=np.float32).reshape(8, 7) + 100, accelerations=np.arange(56, dtype=np.float32).reshape(8, 7) + 200,
               offsets=np.array([0, 4, 7, 7, 7, 7, 8]), validation_calls=1, questions=5)
    robot = _Recorder(raw)
    s = planning.RetimeSettings(blend=0.05)
    out = planning.retime_multi(robot, "paths", "vel", "acc", "envs", s)
    assert robot.calls == [("paths", "vel", "acc", "envs", s)]
    assert [r.status for r in out] == ["complete", "collision", "too_long", "non_finite", "stalled", "complete"]
    assert [r.first_invalid for r in out] == [-1, 1, -1, -1, -1, -1] and [r.complete for r in out] == [True] + [False] * 4 + [True]
    assert [len(r.times) for r in out] == [4, 3, 0, 0, 0, 1] and [r.intervals for r in out] == [5, 9, 5000, 0, 7, 0]
    assert np.array_equal(out[1].positions, raw["positions"][4:7]) and out[1].positions.base is not raw["positions"]
    assert np.array_equal(out[1].velocities, raw["velocities"][4:7]) and np.array_equal(out[5].accelerations, raw["accelerations"][7:8])
    assert out[0].duration == pytest.approx(0.03) and out[5].positions.shape == (1, 7)
    planning.retime_multi(robot, "a", "v", "c")
    assert robot.calls[-1][3] is None and robot.calls[-1][4] == planning.RetimeSettings()


# ---- the host set-up under sanitizers --------------------------------------------------------------------------------
def test_host_path_setup_under_sanitizers():
    out = os.path.join(ROOT, "build", "retime_sanitize")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "retime_sanitize.cc"), "-o", out, "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
