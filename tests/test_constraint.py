"""vmv_constraint_project_batch / _check_batch / _check_motion_batch (and their _host forms), vamp.EEConstraint,
<robot>.project_batch / constraint_check_batch / constraint_check_motion_batch, planning.validate_paths_constrained and
planning.project_goals: what needs no device.  Every argument check of the entry points (they all run before any device
query), the wrappers' shape checks, the float64 statement (tests/constraint_serial.py) against its own promises, and the
host set-up under sanitizers (tests/native/constraint_sanitize.cc)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import constraint_serial as S

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 6
SYMBOLS = ("vmv_constraint_project_batch", "vmv_constraint_project_batch_host", "vmv_constraint_check_batch",
           "vmv_constraint_check_batch_host", "vmv_constraint_check_motion_batch", "vmv_constraint_check_motion_batch_host")
KINDS = ("project", "check", "motion")
FILL = np.float32(-123.0)
MARK = 0xa5


def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib

    declared = _lib.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and hasattr(_lib.lib, s)
        assert getattr(_lib.lib, s).argtypes is not None and getattr(_lib.lib, s).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.EeConstraint) == 29 * 4 and ctypes.sizeof(_lib.ConstraintSettings) == 28
    d = vamp.ConstraintSettings()
    k = S.Settings()
    assert vars(d) == {f: getattr(k, f) for f in vars(d)}  # the serial statement runs the same defaults
    for r in S.ROBOTS:
        mod = getattr(vamp, r)
        assert callable(mod.project_batch) and callable(mod.constraint_check_batch) and callable(mod.constraint_check_motion_batch)


def _constraint(_lib, **kw):
    c = _lib.EeConstraint()
    c.frame[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
    c.pos_lo[:], c.pos_hi[:] = [-np.inf] * 3, [np.inf] * 3
    c.tool_axis[:], c.ref_axis[:] = [0, 0, 1], [0, 0, 1]
    c.max_angle = 0.2
    for name, value in kw.items():
        if isinstance(value, dict):
            for i, v in value.items():
                getattr(c, name)[i] = v
        else:
            setattr(c, name, value)
    return c


def _call(_lib, kind, host, robot=0, n=3, arrays=True, second=True, out=True, extra=True, constraints=True, settings=True,
          n_constraints=1, record=None, bad_at=0, **fields):
    """one refused (or empty) call with its outputs pre-filled -> (status, message); the outputs are untouched.  `arrays`,
    `second`, `out`, `extra`: whether the input array, the second input (motion), the required output and the optional
    output (the residuals) are passed; record: keyword changes to constraint number bad_at; fields: the settings"""
    base = dict(max_iterations=0, pos_tol=0.0, rot_tol=0.0, rot_weight=0.0, damping=0.0, max_step=0.0, check_step=0.0)
    base.update(fields)
    s = _lib.ConstraintSettings(*[base[f] for f, _ in _lib.ConstraintSettings._fields_])
    count = max(n_constraints, 1)
    recs = (_lib.EeConstraint * count)(*[_constraint(_lib, **(record or {})) if k == bad_at else _constraint(_lib) for k in range(count)])
    A, B = np.zeros((3, 7), np.float32), np.zeros((3, 7), np.float32)
    Q = np.full((3, 7), FILL, np.float32)
    E = np.full((3, 2), FILL, np.float32)
    st = np.full(3, MARK, np.uint32)
    bits = np.full(1, MARK, np.uint64)
    ok = np.full(3, MARK, np.uint8)
    if host:
        p = lambda a, t=None: a.ctypes.data_as(t or _lib.c_float_p)  # noqa: E731
    else:  # (the device entry points: refused before any pointer is used, so host addresses do for the test)
        p = lambda a, t=None: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    tail = [] if host else [None]
    fn = getattr(_lib.lib, f"vmv_constraint_{ {'project': 'project', 'check': 'check', 'motion': 'check_motion'}[kind] }_batch" + ("_host" if host else ""))
    common = [recs if constraints else None, n_constraints, ctypes.byref(s) if settings else None]
    if kind == "project":
        rc = fn(robot, p(A) if arrays else None, n, *common, p(Q) if out else None, p(E) if extra else None,
                p(st, _lib.c_u32_p) if second else None, *tail)
    elif kind == "check":
        rc = fn(robot, p(A) if arrays else None, n, *common, p(bits, _lib.c_u64_p) if out else None, p(E) if extra else None, *tail)
    else:
        rc = fn(robot, p(A) if arrays else None, p(B) if second else None, n, *common, p(ok, _lib.c_u8_p) if out else None, *tail)
    assert (Q == FILL).all() and (E == FILL).all() and (st == MARK).all() and (bits == MARK).all() and (ok == MARK).all()
    return rc, _lib.lib.vmv_last_error().decode()


@pytest.mark.parametrize("host", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_argument_checks(vamp, kind, host):
    from vamp_mvt_amd import _lib

    call = lambda **kw: _call(_lib, kind, host, **kw)  # noqa: E731
    assert call(robot=99)[0] == VMV_ERR_UNKNOWN_ROBOT
    assert call(robot=-1, arrays=False)[0] == VMV_ERR_UNKNOWN_ROBOT  # the robot wins over a NULL pointer
    missing = ["arrays", "out", "constraints", "settings"] + (["second"] if kind != "check" else [])
    for m in missing:
        assert call(**{m: False}) == (VMV_ERR_INVALID_ARGUMENT, "null pointer"), m
    assert call(arrays=False, n=0)[0] == VMV_ERR_INVALID_ARGUMENT  # a NULL array wins over the empty batch
    assert call(constraints=False, n_constraints=2) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")  # ... over the count
    for bad in (0, 2, 4):
        assert call(n_constraints=bad) == (VMV_ERR_INVALID_ARGUMENT, "n_constraints must be 1 or n")
    assert call(n_constraints=2, pos_tol=-1.0)[1].startswith("n_constraints")  # the count before the settings
    for f in ("pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "check_step"):
        for v in (-1.0, float("nan"), float("inf")):
            rc, msg = call(**{f: v})
            assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith(f + " must be"), (f, v, msg)
    assert call(max_iterations=1 << 30)[1].startswith("max_iterations")
    assert call(pos_tol=-1.0, check_step=-1.0)[1].startswith("pos_tol")  # the struct's order
    assert call(pos_tol=-1.0, record=dict(max_angle=9.0))[1].startswith("pos_tol")  # the settings before the constraints
    assert call(n=1 << 31, n_constraints=1) == (VMV_ERR_INVALID_ARGUMENT, "n must be below 2^31")
    nan, inf = float("nan"), float("inf")
    refused = [(dict(pos_lo={1: nan}), "must not be NaN"), (dict(pos_hi={0: nan}), "must not be NaN"),
               (dict(pos_lo={2: 0.5}, pos_hi={2: 0.25}), "pos_lo must not exceed pos_hi"), (dict(pos_lo={0: inf}), "pos_lo must be below +inf"),
               (dict(tool_axis={2: 0.0}), "must not be zero"), (dict(ref_axis={2: 0.0}), "must not be zero"),
               (dict(tool_axis={0: nan}), "must be finite"), (dict(max_angle=1.6), "max_angle must be in [0, pi/2]"),
               (dict(max_angle=-0.5), "max_angle must be in"), (dict(max_angle=nan), "max_angle must not be NaN"),
               (dict(frame={0: 1.01}), "frame must be rigid"), (dict(frame={0: -1.0}), "frame must be rigid"),
               (dict(frame={15: 0.0}), "frame must be rigid"), (dict(frame={7: nan}), "frame must be finite")]
    for record, words in refused:
        rc, msg = call(record=record)
        assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith("constraints[0]: ") and words in msg, (record, msg)
        rc, msg = call(record=record, n_constraints=3, bad_at=2)  # per-lane records: the index is named
        assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith("constraints[2]: ") and words in msg, (record, msg)
        assert call(record=record, n=0, n_constraints=1)[0] == VMV_ERR_INVALID_ARGUMENT  # a refusal wins over the empty batch
    # an empty batch needs no device; the optional output may be NULL; a zero axis is fine while the orientation is free
    assert call(n=0)[0] == VMV_OK and call(n=0, extra=False)[0] == VMV_OK and call(n=0, n_constraints=0)[0] == VMV_OK
    assert call(n=0, record=dict(max_angle=0.0, tool_axis={2: 0.0}))[0] == VMV_OK
    assert call(n=0, record=dict(max_angle=float(np.float32(np.pi / 2))))[0] == VMV_OK


def test_wrapper_shape_errors(vamp):
    from vamp_mvt_amd import planning

    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    assert np.array_equal(c.frame, np.eye(4)) and np.isinf(c.pos_lo).all() and np.isinf(c.pos_hi).all() and c.max_angle == 0.2
    b = vamp.EEConstraint.box((-1, -2, -3), (1, 2, 3), frame=np.eye(4))
    assert b.max_angle == 0.0 and b.pos_lo.tolist() == [-1, -2, -3] and b.pos_hi.tolist() == [1, 2, 3]
    with pytest.raises(TypeError):
        vamp.EEConstraint(frame=np.eye(3))
    with pytest.raises(TypeError):
        vamp.EEConstraint(pos_lo=(0, 0))
    with pytest.raises(TypeError):
        vamp.EEConstraint.upright((0, 1), 0.2)
    for call in (vamp.panda.project_batch, vamp.panda.constraint_check_batch):
        with pytest.raises(TypeError):
            call(np.zeros((2, 6), np.float32), c)
        with pytest.raises(TypeError):
            call(np.zeros((2, 7), np.float32), "upright")
        with pytest.raises(ValueError):
            call(np.zeros((3, 7), np.float32), [c, c])
    with pytest.raises(TypeError):
        vamp.panda.constraint_check_motion_batch(np.zeros((2, 7), np.float32), np.zeros((3, 7), np.float32), c)
    with pytest.raises(ValueError):
        vamp.panda.constraint_check_motion_batch(np.zeros((3, 7), np.float32), np.zeros((3, 7), np.float32), [c, c])
    with pytest.raises(vamp.VmvError, match="max_angle"):  # the library's own refusal comes through, before any device
        vamp.panda.project_batch(np.zeros((0, 7), np.float32), vamp.EEConstraint.upright((0, 0, 1), 2.0))
    # empty batches need no device
    q, res, conv, evals = vamp.panda.project_batch(np.zeros((0, 7), np.float32), c)
    assert q.shape == (0, 7) and res.shape == (0, 2) and conv.shape == (0,) and evals.shape == (0,)
    assert vamp.panda.constraint_check_batch(np.zeros((0, 7), np.float32), c).shape == (0,)
    assert vamp.panda.constraint_check_motion_batch(np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), []).shape == (0,)
    valid, band = planning.validate_paths_constrained(vamp.panda, [], None, c)
    assert valid.shape == (0,) and band.shape == (0,)
    assert planning.project_goals(vamp.panda, [], c, None) == []
    with pytest.raises(ValueError):
        planning.validate_paths_constrained(vamp.panda, [np.zeros((2, 7))], None, [c, c])
    with pytest.raises(ValueError):
        planning.project_goals(vamp.panda, [np.zeros((2, 7))], [c, c], None)


class FakeRobot:
    """records what planning hands the robot and answers from tables"""

    def __init__(self):
        self.calls = []

    def dimension(self):
        return 2

    def validate_motion_batch_multi(self, a, b, environments, counts):
        self.calls.append(("motion", np.array(a), np.array(b), list(environments), list(counts)))
        return np.asarray(a)[:, 0] >= 0

    def constraint_check_motion_batch(self, a, b, constraints, settings=None):
        self.calls.append(("band", np.array(a), np.array(b), list(constraints), settings))
        return np.asarray(b)[:, 1] >= 0

    def project_batch(self, q, constraints, settings=None):
        self.calls.append(("project", np.array(q), list(constraints), settings))
        q = np.asarray(q, np.float32) + 1
        return q, np.zeros((len(q), 2), np.float32), q[:, 1] != 3, np.zeros(len(q), np.int32)

    def validate_batch_multi(self, rows, environments, counts):
        self.calls.append(("validate", np.array(rows), list(environments), list(counts)))
        return np.asarray(rows)[:, 0] != 5


def test_validate_paths_constrained_makes_two_batched_calls(vamp):
    from vamp_mvt_amd import planning

    robot = FakeRobot()
    paths = [np.array([[0, 0], [1, 1], [2, 2]]), np.array([[-1, 0], [1, 1]]), np.array([[0, 0], [1, -1], [2, 2]]), np.array([[3, 3]])]
    cons = ["c0", "c1", "c2", "c3"]
    valid, band = planning.validate_paths_constrained(robot, paths, ["e0", "e1", "e2", "e3"], cons, settings="s")
    assert [c[0] for c in robot.calls] == ["motion", "band"]
    _, a, b, envs, counts = robot.calls[0]
    assert counts == [2, 1, 2, 0] and envs == ["e0", "e1", "e2", "e3"] and len(a) == 5
    assert robot.calls[1][3] == ["c0", "c0", "c1", "c2", "c2"] and robot.calls[1][4] == "s"  # one record per edge
    assert valid.tolist() == [True, False, True, True] and band.tolist() == [True, True, False, True]
    robot = FakeRobot()
    planning.validate_paths_constrained(robot, paths, "env", "shared")
    assert robot.calls[0][3] == ["env"] * 4 and robot.calls[1][3] == ["shared"] * 5


def test_project_goals_projects_validates_and_drops(vamp):
    from vamp_mvt_amd import planning

    robot = FakeRobot()
    goals = [np.array([[0, 0], [4, 4], [1, 2]]), np.zeros((0, 2)), np.array([[4, 1]])]
    out = planning.project_goals(robot, goals, ["c0", "c1", "c2"], ["e0", "e1", "e2"], settings="s")
    assert [c[0] for c in robot.calls] == ["project", "validate"]
    assert robot.calls[0][2] == ["c0", "c0", "c0", "c2"] and robot.calls[0][3] == "s"
    _, rows, envs, counts = robot.calls[1]
    assert counts == [2, 0, 1] and envs == ["e0", "e1", "e2"]  # the row that did not converge is not validated
    assert [g.tolist() for g in out] == [[[1, 1]], [], []]  # (4, 4) -> (5, 5) collides; (1, 2) -> (2, 3) did not converge; (4, 1) -> (5, 2) collides
    assert all(g.dtype == np.float32 and g.shape[1] == 2 for g in out)


def test_serial_statement_does_not_import_the_package():
    code = "import sys; sys.path.insert(0, %r); import constraint_serial; assert 'vamp_mvt_amd' not in sys.modules" % os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call([os.sys.executable, "-c", code])


# ---- the float64 statement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", S.ROBOTS)
def test_float64_statement_keeps_its_promises(robot):
    """64 Halton configurations per robot and the three constraints of the device tests: every converged projection is in
    the band, inside the joint bounds, and moved only joints that move the end effector; an in-band input comes back
    unchanged with 0 evaluations; a non-finite row comes back as given"""
    q = S.configs(robot, 64).astype(np.float64)
    lo, hi = S.K.bounds(robot)
    moves = S.ee_mask(robot)
    for name, c in S.cases(robot).items():
        r = S.project(robot, q, c)
        conv = r["converged"]
        ok, _ = S.in_band(robot, r["q"], c)
        print(f"{robot} {name}: converged {conv.mean():.3f}, mean evaluations {r['evaluations'].mean():.1f}")
        assert conv.any() and ok[conv].all() and not ok[~conv].any()
        assert ((r["q"] >= lo) & (r["q"] <= hi)).all()
        assert np.array_equal(r["q"][:, ~moves], q[:, ~moves])
        assert (r["evaluations"][~conv] == S.Settings().max_iterations).all()
        again = S.project(robot, r["q"][conv], c)
        assert np.array_equal(again["q"], r["q"][conv]) and again["converged"].all() and (again["evaluations"] == 0).all()
        bad = q[:3].copy()
        bad[1, 0] = np.nan
        rb = S.project(robot, bad, c)
        assert np.array_equal(rb["q"][1], bad[1], equal_nan=True) and np.isnan(rb["res"][1]).all() and not rb["converged"][1]
        assert np.array_equal(rb["q"][[0, 2]], r["q"][[0, 2]]) and not S.in_band(robot, bad, c)[0][1]


def test_edge_samples_of_the_statement():
    a = np.zeros(7, np.float32)
    b = a.copy()
    assert len(S.edge_samples32(a, b)) == 1 and np.array_equal(S.edge_samples32(a, b)[0], a)  # a zero-length edge: one sample
    b[0] = np.float32(0.05)
    assert len(S.edge_samples32(a, b)) == 1  # exactly check_step
    b[0] = np.float32(0.0500001)
    assert len(S.edge_samples32(a, b)) == 2
    b[0] = np.float32(64 * 0.05 + 0.01)
    assert len(S.edge_samples32(a, b)) == 65
    b[0] = np.float32(1024 * 0.05 + 0.01)
    assert S.edge_samples32(a, b) is None
    b[0] = np.nan
    assert S.edge_samples32(a, b) is None


# ---- the host set-up under sanitizers ------------------------------------------------------------------------------------
def test_host_constraint_setup_under_sanitizers():
    out = os.path.join(ROOT, "build", "constraint_sanitize")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "constraint_sanitize.cc"), "-o", out, "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


# ---- vmv_rrtc_multi_constrained: the checks that come before any device query --------------------------------------------
def _plan(_lib, vamp, robot=0, n=2, constraints=True, csettings=True, settings=True, n_constraints=1, record=None, max_stretch=0.0,
          drop_out=False, **fields):
    """one refused (or empty) vmv_rrtc_multi_constrained call -> (status, message); *out stays as it was"""
    made = []
    for _ in range(2):  # created, unfinalized C environments: no device needed
        h = ctypes.c_void_p()
        assert _lib.lib.vmv_env_create(ctypes.byref(h)) == VMV_OK
        made.append(h.value)
    handles = (ctypes.c_void_p * 2)(*made)
    starts, goals = np.zeros((2, 7), np.float32), np.ones((2, 7), np.float32)
    base = _lib.RrtcSettings(1.0, 1, 1.0, 100, 64, 0)
    gs = _lib.RrtcGoalsSettings(base, 0, 4.0, 0.0001, 1.0, 0)
    cfields = dict(max_iterations=0, pos_tol=0.0, rot_tol=0.0, rot_weight=0.0, damping=0.0, max_step=0.0, check_step=0.0)
    cfields.update(fields)
    ps = _lib.ConstraintPlanSettings(_lib.ConstraintSettings(*[cfields[f] for f, _ in _lib.ConstraintSettings._fields_]), max_stretch)
    count = max(n_constraints, 1)
    recs = (_lib.EeConstraint * count)(*[_constraint(_lib, **(record or {})) if k == count - 1 else _constraint(_lib) for k in range(count)])
    out = ctypes.c_void_p(0x5A5A5A5A)
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    rc = _lib.lib.vmv_rrtc_multi_constrained(robot, handles, n, fp(starts), fp(goals), None, None, ctypes.byref(gs) if settings else None,
                                             recs if constraints else None, n_constraints, ctypes.byref(ps) if csettings else None,
                                             None if drop_out else ctypes.byref(out))
    for h in made:
        _lib.lib.vmv_env_destroy(h)
    if rc != VMV_OK:
        assert out.value == 0x5A5A5A5A  # a refused call writes nothing
    elif not drop_out:
        assert _lib.lib.vmv_plans_destroy(out) == VMV_OK
    return rc, _lib.lib.vmv_last_error().decode()


def test_constrained_planner_argument_checks(vamp):
    from vamp_mvt_amd import _lib, planning

    assert "vmv_rrtc_multi_constrained" in _lib.declared_symbols() and ctypes.sizeof(_lib.ConstraintPlanSettings) == 32
    call = lambda **kw: _plan(_lib, vamp, **kw)  # noqa: E731
    assert call(robot=99)[0] == VMV_ERR_UNKNOWN_ROBOT and call(robot=-1, constraints=False)[0] == VMV_ERR_UNKNOWN_ROBOT
    assert call(settings=False)[0] == VMV_ERR_INVALID_ARGUMENT and call(drop_out=True)[0] == VMV_ERR_INVALID_ARGUMENT
    assert call(constraints=False) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")
    assert call(csettings=False) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")
    assert call(settings=False, constraints=False)[0] == VMV_ERR_INVALID_ARGUMENT  # vmv_rrtc_multi_goals's checks come first
    for bad in (0, 3):
        assert call(n_constraints=bad) == (VMV_ERR_INVALID_ARGUMENT, "n_constraints must be 1 or n_problems")
    assert call(check_step=-1.0)[1].startswith("check_step must be") and call(pos_tol=float("nan"))[1].startswith("pos_tol must be")
    for v in (-1.0, float("nan"), float("inf")):
        assert call(max_stretch=v)[1].startswith("max_stretch must be")
    assert call(pos_tol=-1.0, max_stretch=-1.0)[1].startswith("pos_tol")  # the struct's order
    rc, msg = call(record=dict(max_angle=2.0))
    assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith("constraints[0]: max_angle")
    rc, msg = call(record=dict(pos_lo={0: 1.0}, pos_hi={0: 0.0}), n_constraints=2)
    assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith("constraints[1]: pos_lo must not exceed")
    assert call(n=0)[0] == VMV_OK and call(n=0, n_constraints=0)[0] == VMV_OK  # no problems: an empty result, no device
    assert call(n=0, record=dict(max_angle=2.0))[0] == VMV_ERR_INVALID_ARGUMENT  # a refusal wins over the empty batch
    # the Python layers: shape errors before any library call, an empty call without a device
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    assert planning.rrtc_multi_constrained(vamp.panda, np.zeros((0, 7)), [], [], c) == []
    assert callable(vamp.panda.rrtc_multi_constrained_raw)
    with pytest.raises(TypeError):
        planning.rrtc_multi_constrained(vamp.panda, np.zeros((1, 7)), [np.zeros(7)], [None], c)
    with pytest.raises(ValueError):
        planning.rrtc_multi_constrained(vamp.panda, np.zeros((2, 7)), [np.zeros((1, 7))] * 2, [None, None], [c, c, c])
    with pytest.raises(ValueError):
        planning.rrtc_multi_constrained(vamp.panda, np.zeros((1, 7)), [np.zeros((1, 7))], [None], c, max_stretch=-1.0)
