"""vmv_retime_multi_constrained without a device: the serial statement (tests/retime_constrained_serial.py) against
tests/retime_serial.py where the two must agree, the round loop on hand-made hooks over joint space, the class of every
case of the shared case set on the CPU (the oracle and the float64 band), the ABI's refusals and the Python wrappers."""
import ctypes
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import retime_constrained_cases as C
import retime_constrained_serial as RC
import retime_serial as R

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
SENTINEL = 0x5a5a5a5a
CASE = RC.Settings(grid_step=R.CASE_SETTINGS.grid_step, max_grid=R.CASE_SETTINGS.max_grid)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_trajectory(a, b):
    return (a.status == b.status and a.intervals == b.intervals and a.samples == b.samples and
            np.array_equal(bits(np.float32(a.duration)), bits(np.float32(b.duration))) and
            all(x.shape == y.shape and np.array_equal(bits(x), bits(y))
                for x, y in ((a.times, b.times), (a.positions, b.positions), (a.velocities, b.velocities), (a.accelerations, b.accelerations))))


# ---- the statement against retime_serial -----------------------------------------------------------------------------
@pytest.mark.parametrize("robot", R.ROBOTS)
def test_without_refusals_the_statement_is_retime_serials(robot):
    V, A = R.limits(robot)
    yes = lambda a, b: True
    for (name, w), want in zip(R.cases(robot), R.results(robot)):
        for hooks in ((None, None), (yes, yes)):
            got = RC.retime_constrained(w, V, A, CASE, *hooks)
            assert same_trajectory(got, want), name
            assert got.rounds == 1 and not got.levels.any() and got.repaired == 0 and got.stops == 0 and got.first_invalid == RC.NONE
            assert got.levels.shape == (len(w),)


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_all_corners_stopped_is_stop_at_waypoints(robot):
    V, A = R.limits(robot)
    corners = 0
    for (name, w), want in zip(R.cases(robot), R.results(robot, stop_at_waypoints=True)):
        got = RC.retime_constrained(w, V, A, replace(CASE, stop_at_waypoints=True))
        assert same_trajectory(got, want), name
        assert got.stops == got.repaired and set(got.levels.tolist()) <= {0, CASE.blend_halvings + 1}
        corners += got.stops
    assert corners > 40


def test_serial_statement_does_not_import_the_package():
    code = ("import sys; sys.path.insert(0, %r); import retime_constrained_serial, retime_constrained_cases; "
            "assert 'vamp_mvt_amd' not in sys.modules" % os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([os.sys.executable, "-c", code])


# ---- the round loop on hand-made hooks over joint space --------------------------------------------------------------
S2 = RC.Settings(blend=0.2, grid_step=0.019, dt=0.01)
V2, A2 = np.array([1.0, 1.2], np.float32), np.array([2.0, 2.3], np.float32)
CORNER2 = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], np.float32)
INSIDE = lambda depth: np.array([1.0 - depth, depth])  # a point on the corner's bisector, inside it


def near(point, eps):
    """refuses a pair whose second sample comes within eps of `point`"""
    return lambda a, b: float(np.linalg.norm(np.asarray(b, np.float64) - point)) > eps


def test_a_point_just_inside_the_corner_is_cleared_by_a_level():
    # the level-0 blend of half-length 0.2 passes the bisector at depth 0.05; level 1 at 0.025
    r = RC.retime_constrained(CORNER2, V2, A2, S2, valid=near(INSIDE(0.05), 0.01))
    assert r.status == "complete" and r.levels.tolist() == [0, 1, 0] and r.rounds == 2 and (r.repaired, r.stops) == (1, 0)
    assert len(r.history) == 2 and r.history[0][2] == [1] and all(f[3] == [1] and not f[1] and f[2] for f in r.history[0][1])
    assert all(np.linalg.norm(r.positions - INSIDE(0.05), axis=1) > 0.01)
    plain = R.retime(CORNER2, V2, A2, S2)
    assert r.duration > plain.duration  # (here the smaller blend is slower)


off_the_polyline = lambda a, b: not (1.0 - float(b[0]) > 1e-4 and float(b[1]) > 1e-4)  # refuses every sample inside the corner


def test_a_point_at_the_corner_needs_the_stop_and_one_on_the_line_ends_the_path():
    H = S2.blend_halvings
    r = RC.retime_constrained(CORNER2, V2, A2, S2, band_edge=off_the_polyline)
    assert r.status == "complete" and r.levels.tolist() == [0, H + 1, 0] and r.rounds == H + 2 and (r.repaired, r.stops) == (1, 1)
    stop = R.retime(CORNER2, V2, A2, replace(S2, stop_at_waypoints=True))
    assert same_trajectory(r, stop)
    for hook, status in (("valid", "collision"), ("band_edge", "out_of_band")):
        r = RC.retime_constrained(CORNER2, V2, A2, S2, **{hook: near(np.array([0.5, 0.0]), 0.02)})
        assert r.status == status and r.rounds == 1 and not r.levels.any() and r.first_invalid == r.history[0][1][0][0]
        assert same_trajectory(replace(r, status="complete"), R.retime(CORNER2, V2, A2, S2))  # the samples come back whole
    both = RC.retime_constrained(CORNER2, V2, A2, S2, valid=near(np.array([0.5, 0.0]), 0.02), band_edge=near(np.array([0.3, 0.0]), 0.02))
    assert both.status == "out_of_band" and both.first_invalid < r.first_invalid  # the FIRST failing pair names the status


def test_max_rounds_ends_with_the_last_rounds_samples():
    r = RC.retime_constrained(CORNER2, V2, A2, replace(S2, max_rounds=1), valid=near(INSIDE(0.05), 0.01))
    assert r.status == "collision" and r.rounds == 1 and not r.levels.any() and r.first_invalid >= 0
    assert same_trajectory(replace(r, status="complete"), R.retime(CORNER2, V2, A2, S2))
    r = RC.retime_constrained(CORNER2, V2, A2, replace(S2, max_rounds=3), band_edge=off_the_polyline)
    assert r.status == "out_of_band" and r.rounds == 3 and r.levels.tolist() == [0, 2, 0]  # (the levels of the last set-up)


def test_abutting_blends_are_blamed_together_and_only_the_blamed_corners_move():
    zig = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.3], [2.0, 0.3], [2.0, 1.3]], np.float32)  # corners 1 and 2 abut (0.3 <= 2 blend)
    across = lambda a, b: not (a[1] < 0.15 <= b[1] and b[0] < 1.5)  # refuses the pair that crosses the blends' junction (1, 0.15)
    r = RC.retime_constrained(zig, V2, A2, S2, valid=across)
    assert [f[3] for f in r.history[0][1]] == [[1, 2]]  # one pair, both corners
    assert r.history[0][0].tolist() == [0, 0, 0, 0, 0] and r.history[1][0].tolist() == [0, 1, 1, 0, 0]
    assert r.status == "collision" and r.rounds == 2 and r.levels.tolist() == [0, 1, 1, 0, 0]  # then a line carries the junction
    only_three = RC.retime_constrained(zig, V2, A2, S2, valid=near(np.array([2.0 - 0.05, 0.3 + 0.05]), 0.01))
    assert only_three.status == "complete" and only_three.levels.tolist() == [0, 0, 0, 1, 0]


def test_a_long_period_jumps_over_a_whole_blend_and_still_blames_it():
    H = S2.blend_halvings
    coarse = replace(S2, dt=0.2, blend=0.05)  # the level-3 blend is 0.0125 long

    def chord(a, b):  # refuses a pair whose chord's middle lies inside the corner
        m = 0.5 * (np.asarray(a, np.float64) + np.asarray(b, np.float64))
        return not (1.0 - m[0] > 1e-4 and m[1] > 1e-4)

    r = RC.retime_constrained(CORNER2, V2, A2, coarse, valid=chord)
    jumped = [(levels.tolist(), f) for levels, fails, _ in r.history for f in fails if f[4]]
    assert jumped and all(levels[1] == H and f[3] == [1] for levels, f in jumped)  # neither sample on the blend, and it is blamed
    assert r.levels[1] == H + 1 and r.status == "collision" and r.rounds == H + 2  # (the chord across a stop is on no blend)


def test_duplicates_and_trivial_paths_report_levels_per_input_waypoint():
    w = np.array([[0, 0], [0, 0], [1, 0], [1, 0], [1, 0], [1, 1]], np.float32)
    r = RC.retime_constrained(w, V2, A2, S2, valid=near(INSIDE(0.05), 0.01))
    assert r.levels.tolist() == [0, 0, 1, 0, 0, 0] and r.status == "complete"  # the kept copy of the corner carries it
    for w, samples in ((np.zeros((0, 2)), 0), (np.ones((1, 2)), 1), (np.ones((3, 2)), 1)):
        r = RC.retime_constrained(w, V2, A2, S2, valid=lambda a, b: False)
        assert (r.status, r.samples, r.rounds, r.questions) == ("complete", samples, 1, 0) and r.levels.tolist() == [0] * len(w)
    bad = CORNER2.copy()
    bad[1, 0] = np.nan
    r = RC.retime_constrained(bad, V2, A2, S2, valid=lambda a, b: False)
    assert (r.status, r.samples, r.rounds) == ("non_finite", 0, 1)
    two = RC.retime_constrained(CORNER2[:2], V2, A2, S2, valid=lambda a, b: False)
    assert two.status == "collision" and two.first_invalid == 0 and two.rounds == 1


def test_a_later_round_can_end_too_long():
    # halving the blend changes the interval count - 75 intervals at level 0, 76 at level 1 with this grid_step - so a
    # max_grid that level 0 meets can refuse a later round
    S = replace(S2, blend=0.3, grid_step=0.027)
    n = [RC.setup(CORNER2, S, [0, lv, 0])[2] for lv in range(3)]
    assert len(set(n)) > 1
    worst = int(np.argmax(n))
    assert worst > 0 and n[worst] > n[0]
    r = RC.retime_constrained(CORNER2, V2, A2, replace(S, max_grid=n[worst] - 1), valid=off_the_polyline)
    assert r.status == "too_long" and r.rounds == worst + 1 and r.samples == 0 and r.intervals == n[worst] and r.levels[1] == worst


# ---- the shared case set: every class, on the CPU --------------------------------------------------------------------
CLASSES = ("a", "b", "c", "d", "e", "fb", "fc", "fd", "g", "h", "i", "j")


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_every_case_has_its_class_on_the_cpu(robot):
    cases, results = C.cases(robot), C.expected(robot)
    assert {c.kind for c in cases} == set(CLASSES)
    assert len(cases) <= 40 and max(len(c.path) for c in cases) <= 12
    H = C.SETTINGS.blend_halvings
    bands = set()  # (the band's kind, the class) of every band case
    for c, (r, margin) in zip(cases, results):
        top = int(r.levels.max()) if len(r.levels) else 0
        if c.constraint is not None:
            assert margin > C.MARGIN, (c.name, margin)  # the fp32 band gives the same class
            bands.add(("cone" if c.constraint.max_angle > 0 else "box", c.kind))
        if c.kind == "a":
            assert (r.status, r.rounds, top) == ("complete", 1, 0)
        elif c.kind in ("b", "fb"):
            assert r.status == "complete" and 1 <= top <= H and r.stops == 0 and r.repaired == 1, c.name
        elif c.kind in ("c", "fc"):
            assert r.status == "complete" and top == c.settings.blend_halvings + 1 and r.stops == 1, c.name
            assert r.rounds == c.settings.blend_halvings + 2
        elif c.kind in ("d", "fd"):
            assert r.status == ("collision" if c.kind == "d" else "out_of_band") and r.rounds == 1 and top == 0, c.name
            assert any(not f[3] for f in r.history[0][1])
        elif c.kind == "e":
            assert any(len(f[3]) == 2 for f in r.history[0][1]), c.name
            w = c.path.astype(np.float64)
            assert np.linalg.norm(w[2] - w[1]) <= 2 * c.settings.blend
        elif c.kind == "g":
            assert r.status == "complete" and [int(x > 0) for x in r.levels] == [0, 1, 0, 1, 0]
            fails = [f for _, fs, _ in r.history for f in fs]
            assert {tuple(f[3]) for f in fails if not f[2]} == {(1,)} and {tuple(f[3]) for f in fails if not f[1]} == {(3,)}
        elif c.kind == "h":
            assert C.jumps(r) and c.settings.blend_halvings == 3 and c.settings.dt > C.SETTINGS.dt
        elif c.kind == "i":
            assert (r.status, r.rounds, top, c.settings.max_rounds) == ("collision", 1, 0, 1) and r.samples > 0
            twin = next(k for k, b in enumerate(cases) if b.kind == "b" and b.spheres == c.spheres)
            assert results[twin][0].rounds > 1
    assert bands >= {(band, kind) for band in ("box", "cone") for kind in ("fb", "fc", "fd")}  # (b) to (d) under both bands
    names = {c.name for c in cases}
    assert {"no_waypoints", "one_waypoint", "one_waypoint_thrice", "duplicates", "nan_waypoint"} <= names
    assert {"box_level", "box_stop", "box_line", "cone_level", "cone_stop", "cone_line"} <= names


# ---- the ABI without a device ----------------------------------------------------------------------------------------
NAMES = ("vmv_retime_multi_constrained", "vmv_retime_levels")
FIELDS = ("blend", "grid_step", "dt", "max_grid", "max_samples", "stop_at_waypoints")


def test_symbols_settings_and_statuses(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name) and getattr(_lib.lib, name).argtypes is not None
    assert "vmv_retime_band_pairs_host" not in names and hasattr(dll, "vmv_retime_band_pairs_host")  # the tests' aid is no interface
    assert not hasattr(vamp.panda, "retime_band_pairs")
    assert vamp.abi_version() == 1  # the change is additive
    assert planning.RETIME_STATUS == R.STATUS == ("complete", "collision", "too_long", "non_finite", "stalled")
    assert planning.RETIME_CONSTRAINED_STATUS == RC.STATUS == planning.RETIME_STATUS + ("out_of_band",)
    s = planning.RetimeConstrainedSettings()
    assert (s.blend_halvings, s.max_rounds) == (3, 8) == (RC.Settings().blend_halvings, RC.Settings().max_rounds)
    assert all(getattr(s, k) == getattr(planning.RetimeSettings(), k) for k in FIELDS)
    assert ctypes.sizeof(_lib.RetimeConstrainedSettings) == 32
    assert tuple(f[0] for f in _lib.RetimeConstrainedSettings._fields_) == ("base", "blend_halvings", "max_rounds")
    header = open(_lib.HEADER_PATH).read()
    assert "VMV_RETIME_OUT_OF_BAND = 5" in header and "default (3); at most 8" in header and "default (8)" in header
    assert "choices, not measurements" in header
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.retime_multi_constrained) and callable(robot.retime_multi_constrained_raw)


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


def _call(_lib, handles, robot=0, n=2, drop=(), offsets=(0, 2, 4), vel=None, acc=None, constraints=0, halvings=0, max_rounds=0,
          constraint=None, constraint_settings=None, **settings):
    """one vmv_retime_multi_constrained call with two two-waypoint paths -> (status, *out, vmv_last_error())"""
    points = np.zeros((4, 16), np.float32)
    points[1::2] = 0.5
    off = np.array(offsets, np.uintp)
    v = np.ones(16, np.float32) if vel is None else np.asarray(vel, np.float32)
    a = np.ones(16, np.float32) if acc is None else np.asarray(acc, np.float32)
    s = dict.fromkeys(FIELDS, 0)
    s.update(settings)
    cs = _lib.RetimeConstrainedSettings(_lib.RetimeSettings(*[s[k] for k in FIELDS]), halvings, max_rounds)
    import vamp_mvt_amd as vamp
    one = (constraint or vamp.EEConstraint.upright((0, 0, 1), 0.2)).struct()
    records = (_lib.EeConstraint * max(constraints, 1))(*[one] * max(constraints, 1))
    ps = (constraint_settings or vamp.ConstraintSettings()).struct()
    out = ctypes.c_void_p(SENTINEL)
    ptr = {"envs": None if handles is None else (ctypes.c_void_p * max(len(handles), 1))(*handles),
           "points": points.ctypes.data_as(_lib.c_float_p), "offsets": off.ctypes.data_as(_lib.c_size_p),
           "vel_limits": v.ctypes.data_as(_lib.c_float_p), "acc_limits": a.ctypes.data_as(_lib.c_float_p),
           "constraints": records if constraints else None, "settings": ctypes.byref(cs),
           "constraint_settings": ctypes.byref(ps) if constraints else None, "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_retime_multi_constrained(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["vel_limits"],
                                               ptr["acc_limits"], ptr["constraints"], constraints, ptr["settings"],
                                               ptr["constraint_settings"], ptr["out"])
    return rc, out.value, _lib.lib.vmv_last_error().decode()


def refused(result, word):
    rc, out, message = result
    return rc == VMV_ERR_INVALID_ARGUMENT and out == SENTINEL and word in message and "vmv_retime_multi_constrained" in message


def test_every_refusal_of_retime_multi_is_made_under_the_new_name(raw):
    _lib, make = raw
    assert _call(_lib, None, robot=99)[:2] == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    for drop in ("settings", "out", "vel_limits", "acc_limits", "offsets", "points"):
        assert refused(_call(_lib, [make(), make()], drop=(drop,)), drop)
        assert refused(_call(_lib, None, drop=(drop,), constraints=1), drop)
    assert refused(_call(_lib, None, offsets=(0, 3, 2)), "offsets") and refused(_call(_lib, None, offsets=(1, 2, 4)), "offsets[0]")
    assert refused(_call(_lib, None, n=2 ** 31), "n is")
    for which in ("vel", "acc"):
        for value in (0.0, -1.0, float("nan"), float("inf")):
            limits = np.ones(16, np.float32)
            limits[6] = value
            assert refused(_call(_lib, None, **{which: limits}), which + "_limits[6]")
    for name in ("blend", "grid_step", "dt"):
        for value in (float("nan"), float("inf"), float("-inf")):
            assert refused(_call(_lib, None, **{name: value}), name)
    for kw, word in ((dict(grid_step=9e-7), "grid_step"), (dict(dt=9e-7), "dt"), (dict(max_grid=4097), "max_grid"),
                     (dict(stop_at_waypoints=2), "stop_at_waypoints"), (dict(stop_at_waypoints=-1), "stop_at_waypoints")):
        assert refused(_call(_lib, None, **kw), word)
        assert refused(_call(_lib, [make(), make()], **kw), word)  # before the handles are looked at
    a = make()
    assert _call(_lib, [a, None])[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    rc, out, message = _call(_lib, [a, make()])
    assert (rc, out) == (VMV_ERR_NOT_FINALIZED, SENTINEL) and "envs[0] is not finalized" in message


def test_the_calls_own_refusals(raw, vamp):
    _lib, _ = raw
    assert refused(_call(_lib, None, halvings=9), "blend_halvings")
    assert _call(_lib, None, halvings=8)[0] != VMV_ERR_INVALID_ARGUMENT
    assert refused(_call(_lib, None, n=2, constraints=3), "n_constraints")
    assert refused(_call(_lib, None, n=2, constraints=2, offsets=(0, 2, 4), drop=("constraints",)), "constraints is NULL")
    assert refused(_call(_lib, None, constraints=1, drop=("constraint_settings",)), "constraint_settings is NULL")
    assert refused(_call(_lib, None, constraints=1, constraint_settings=vamp.ConstraintSettings(check_step=float("nan"))), "check_step")
    flat = vamp.EEConstraint.upright((0, 0, 0), 0.2)
    assert refused(_call(_lib, None, constraints=2, constraint=flat), "constraints[0]: tool_axis")
    lopsided = vamp.EEConstraint.box((0.5, 0, 0), (0.0, 1, 1))
    assert refused(_call(_lib, None, constraints=1, constraint=lopsided), "pos_lo must not exceed pos_hi")
    for constraints in (0, 1, 2):  # accepted: fails later for want of a device, or runs
        assert _call(_lib, None, constraints=constraints)[0] != VMV_ERR_INVALID_ARGUMENT


def test_no_paths_and_the_levels_accessor(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, res, _ = _call(_lib, None, n=0)
    assert rc == VMV_OK and res not in (None, SENTINEL)
    assert L.vmv_retime_levels(res, None, None, None, None) == VMV_OK
    assert L.vmv_retime_samples(res, None, None, None, None, 0) == VMV_OK and L.vmv_retime_destroy(res) == VMV_OK
    assert L.vmv_retime_levels(None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    # a result of plain vmv_retime_multi is refused
    cs = _lib.RetimeSettings(0, 0, 0, 0, 0, 0)
    out = ctypes.c_void_p()
    ones = np.ones(16, np.float32)
    assert L.vmv_retime_multi(0, None, 0, None, None, ones.ctypes.data_as(_lib.c_float_p), ones.ctypes.data_as(_lib.c_float_p),
                              ctypes.byref(cs), ctypes.byref(out)) == VMV_OK
    assert L.vmv_retime_levels(out, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT and b"vmv_retime_levels" in L.vmv_last_error()
    assert L.vmv_retime_destroy(out) == VMV_OK
    ones = np.ones(7)
    assert planning.retime_multi_constrained(vamp.panda, [], ones, ones) == []
    assert vamp.panda.retime_multi_constrained([], ones, ones, [], vamp.EEConstraint.upright((0, 0, 1), 0.2)) == []
    raw = vamp.panda.retime_multi_constrained_raw([], ones, ones, None, None, planning.RetimeConstrainedSettings())
    assert raw["positions"].shape == (0, 7) and raw["levels"].shape == (0,) and list(raw["level_offsets"]) == [0]


def test_well_formed_call_fails_loudly_without_a_device(vamp):
    from vamp_mvt_amd import planning

    if vamp.device_count() == 0:  # there is no CPU fallback
        for envs, cons in ((None, None), ([None], None), (None, vamp.EEConstraint.upright((0, 0, 1), 0.2))):
            with pytest.raises(vamp.VmvError) as ei:
                planning.retime_multi_constrained(vamp.panda, [np.zeros((2, 7)) + [[0], [1]]], np.ones(7), np.ones(7), envs, cons)
            assert ei.value.status == VMV_ERR_NO_DEVICE


# ---- the Python wrappers ---------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    paths = [np.zeros((3, 7), np.float32), np.ones((2, 7), np.float32)]
    ones = np.ones(7, np.float32)
    up = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.RetimeConstrainedSettings
    f = lambda **kw: planning.retime_multi_constrained(vamp.panda, kw.pop("paths", paths), kw.pop("vel", ones), ones, **kw)
    for kw, error in ((dict(settings=S(blend_halvings=9)), ValueError), (dict(settings=S(blend_halvings=-1)), ValueError),
                      (dict(settings=S(max_rounds=2 ** 32)), ValueError), (dict(settings=S(dt=float("nan"))), ValueError),
                      (dict(settings=S(max_grid=5000)), ValueError), (dict(constraints=[up, up, up]), ValueError),
                      (dict(constraints="upright"), TypeError), (dict(environments=[None]), ValueError),
                      (dict(vel=np.ones(6)), (TypeError, ValueError)), (dict(paths=[np.zeros((3, 6))]), (TypeError, ValueError))):
        with pytest.raises(error):
            f(**kw)


def test_results_are_cut_from_the_packed_arrays(vamp):
    from vamp_mvt_amd import planning

    class Robot:
        def retime_multi_constrained_raw(self, *args):
            self.args = args
            pos = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
            return dict(status=np.array([0, 5, 1], np.uint8), intervals=np.array([4, 6, 8], np.uint32), samples=np.array([2, 0, 3], np.uint32),
                        duration=np.array([0.5, 0.0, 1.5], np.float32), first_invalid=np.array([0xffffffff, 7, 1], np.uint32),
                        times=np.arange(5, dtype=np.float32), positions=pos, velocities=pos + 100, accelerations=pos + 200,
                        offsets=np.array([0, 2, 2, 5]), validation_calls=2, questions=9, rounds=np.array([1, 3, 2], np.uint32),
                        repaired=np.array([0, 2, 1], np.uint32), stops=np.array([0, 1, 0], np.uint32),
                        levels=np.array([0, 0, 0, 4, 1, 0, 0, 2, 0], np.uint8), level_offsets=np.array([0, 2, 6, 9]))

    robot = Robot()
    got = planning.retime_multi_constrained(robot, "paths", "v", "a", "envs", "cons", None, "cs")
    assert robot.args[:5] == ("paths", "v", "a", "envs", "cons") and robot.args[5] == planning.RetimeConstrainedSettings() and robot.args[6] == "cs"
    assert [t.status for t in got] == ["complete", "out_of_band", "collision"] and [t.first_invalid for t in got] == [-1, 7, 1]
    assert [t.rounds for t in got] == [1, 3, 2] and [t.repaired for t in got] == [0, 2, 1] and [t.stops for t in got] == [0, 1, 0]
    assert [t.levels.tolist() for t in got] == [[0, 0], [0, 4, 1, 0], [0, 2, 0]]
    assert got[2].positions.shape == (3, 7) and got[2].positions[0, 0] == 14 and len(got[1].times) == 0 and got[0].complete
    assert isinstance(got[0], planning.Trajectory)
