"""vmv_optimize_multi_constrained / planning.optimize_multi_constrained: what holds without a device — every refusal of
the entry point in the header's order with *out untouched, vmv_optimized_held on results of either call, the Python
layers' own checks, and the serial statement (tests/optimize_constrained_serial.py) against hand-made clearance, band and
projection callbacks on a planar toy problem."""
import ctypes

import numpy as np
import pytest

from optimize_constrained_serial import OUT_OF_BAND, optimize_constrained_serial
from optimize_serial import NO_VALID, NONFINITE, OK, optimize_serial

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 5, 6
SENTINEL = 0x5A5A5A5A
DEFAULTS = dict(max_iterations=64, validate_every=8, step=1.0 / 40.0, max_step=0.1, min_change=1e-4, smooth_weight=1.0,
                env_weight=1.0, self_weight=1.0, env_margin=0.05, self_margin=0.01, max_waypoints=0)
f32 = np.float32


# ---- the entry point's checks ---------------------------------------------------------------------------------------------
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


@pytest.fixture()
def raw(vamp):
    """two created, unfinalized C environments (no device needed), destroyed afterwards"""
    from vamp_mvt_amd import _lib

    handles = []
    for _ in range(2):
        h = ctypes.c_void_p()
        assert _lib.lib.vmv_env_create(ctypes.byref(h)) == 0
        handles.append(h.value)
    yield _lib, handles
    for h in handles:
        _lib.lib.vmv_env_destroy(h)


def _call(_lib, handles, robot=0, n=None, drop=(), offsets=(0, 4, 7), n_constraints=1, record=None, cfields=None, keep=False,
          **settings):
    """one vmv_optimize_multi_constrained call with two paths (4 and 3 waypoints); `drop` names the pointers passed as NULL;
    record: fields of the last constraint; cfields: fields of the constraint settings -> (status, *out, vmv_last_error())"""
    n = len(handles) if n is None else n
    pts = np.linspace(0.0, 1.0, 7 * 7, dtype=np.float32).reshape(7, 7)
    s = dict(DEFAULTS)
    s.update(settings)
    cs = _lib.OptimizeSettings(*[s[k] for k in DEFAULTS])
    cf = dict(max_iterations=0, pos_tol=0.0, rot_tol=0.0, rot_weight=0.0, damping=0.0, max_step=0.0, check_step=0.0)
    cf.update(cfields or {})
    ps = _lib.ConstraintSettings(*[cf[f] for f, _ in _lib.ConstraintSettings._fields_])
    count = max(n_constraints, 1)
    recs = (_lib.EeConstraint * count)(*[_constraint(_lib, **(record or {})) if k == count - 1 else _constraint(_lib) for k in range(count)])
    out = ctypes.c_void_p(SENTINEL)
    off = np.ascontiguousarray(offsets, np.uintp)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "points": pts.ctypes.data_as(_lib.c_float_p),
           "offsets": off.ctypes.data_as(_lib.c_size_p), "settings": ctypes.byref(cs), "constraints": recs,
           "constraint_settings": ctypes.byref(ps), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_optimize_multi_constrained(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["settings"],
                                                 ptr["constraints"], n_constraints, ptr["constraint_settings"], ptr["out"])
    message = _lib.lib.vmv_last_error().decode()
    if rc == VMV_OK and not keep and "out" not in drop:
        assert _lib.lib.vmv_optimized_destroy(out) == VMV_OK
        return rc, None, message
    return rc, out.value, message


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmv_optimize_multi_constrained", "vmv_optimized_held"):
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert vamp.abi_version() == 1  # the change is additive
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.optimize_multi_constrained) and callable(robot.optimize_multi_constrained_raw)
    assert planning.OPTIMIZE_CONSTRAINED_STATUS == ("ok", "no_valid", "nonfinite", "out_of_band")
    assert planning.OPTIMIZE_CONSTRAINED_STATUS[:3] == planning.OPTIMIZE_STATUS
    assert ctypes.sizeof(_lib.OptimizeSettings) == 44 and ctypes.sizeof(_lib.ConstraintSettings) == 28  # both layouts stay


def test_refusals_in_the_headers_order(raw):
    """vmv_optimize_multi's checks in its order, then the constraint's own; each pair below spoils two things and the
    earlier check's answer comes back; *out stays as it was"""
    _lib, handles = raw
    refused = lambda **kw: _call(_lib, handles, **kw)[:2]  # noqa: E731
    bad = (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    # ---- vmv_optimize_multi's own, in its order
    for robot in (-1, 4, 7):
        assert refused(robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    assert refused(robot=9, drop=("settings", "constraints")) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    for drop in ("envs", "points", "offsets", "settings", "out"):
        assert refused(drop=(drop,)) == bad, drop
    assert refused(n=1 << 31) == bad
    assert refused(max_waypoints=3) == bad and refused(max_waypoints=1025) == bad
    for offsets in ((0, 5, 4), (1, 4, 7), (3, 2, 7)):
        assert refused(offsets=offsets) == bad
    assert _call(_lib, [handles[0], None])[:2] == bad
    for name in ("step", "max_step", "env_margin", "self_margin"):
        for value in (0.0, -1.0, float("inf"), float("nan")):
            assert refused(**{name: value}) == bad, (name, value)
    for name in ("smooth_weight", "env_weight", "self_weight"):
        for value in (-1e-3, float("inf"), float("nan")):
            assert refused(**{name: value}) == bad, (name, value)
    assert refused(min_change=float("nan")) == bad and refused(validate_every=0) == bad
    # ---- then the constraint's own, in vmv_constraint_project_batch's order, with their words
    assert _call(_lib, handles, drop=("constraints",)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "null pointer")
    assert _call(_lib, handles, drop=("constraint_settings",)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "null pointer")
    for count in (0, 3):
        assert _call(_lib, handles, n_constraints=count) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "n_constraints must be 1 or n_paths")
    for field in ("pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "check_step"):
        for v in (-1.0, float("nan"), float("inf")):
            rc, out, msg = _call(_lib, handles, cfields={field: v})
            assert (rc, out) == bad and msg.startswith(field + " must be"), (field, v, msg)
    rc, out, msg = _call(_lib, handles, cfields=dict(max_iterations=1 << 30))
    assert (rc, out) == bad and msg.startswith("max_iterations must be")
    rc, out, msg = _call(_lib, handles, record=dict(max_angle=2.0))
    assert (rc, out) == bad and msg.startswith("constraints[0]: max_angle")
    rc, out, msg = _call(_lib, handles, record=dict(pos_lo={0: 1.0}, pos_hi={0: 0.0}), n_constraints=2)
    assert (rc, out) == bad and msg.startswith("constraints[1]: pos_lo must not exceed")
    rc, out, msg = _call(_lib, handles, record=dict(frame={3: float("nan")}))
    assert (rc, out) == bad and msg.startswith("constraints[0]: frame must be finite")
    # ---- which check wins where two apply
    assert refused(step=0.0, drop=("constraints",)) == bad
    assert _call(_lib, handles, validate_every=0, n_constraints=3)[2] != "n_constraints must be 1 or n_paths"
    assert _call(_lib, handles, drop=("constraints",), n_constraints=3)[2] == "null pointer"
    assert _call(_lib, handles, n_constraints=3, cfields=dict(pos_tol=-1.0))[2] == "n_constraints must be 1 or n_paths"
    assert _call(_lib, handles, cfields=dict(pos_tol=-1.0, check_step=-1.0), record=dict(max_angle=2.0))[2].startswith("pos_tol")
    assert _call(_lib, handles, cfields=dict(check_step=-1.0), record=dict(max_angle=2.0))[2].startswith("check_step")
    # ---- a well-formed call reaches the environments' own checks, which need no device either
    assert refused() == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(n_constraints=2) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(record=dict(max_angle=2.0)) == bad  # a refusal wins over the environments' state
    assert refused(validate_every=1000, min_change=-1.0, max_iterations=0, smooth_weight=0.0) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_a_refused_environment_kind_comes_after_the_constraints_checks(raw):
    """a point cloud or an attachment stays refused as in vmv_optimize_multi, in vmv_clearance_batch_multi's words, before
    the finalized check; the argument checks of both layers come first"""
    _lib, handles = raw
    tf = np.eye(4, dtype=np.float32)
    sp = np.array([[0, 0, 0.1, 0.03]], np.float32)
    assert _lib.lib.vmv_env_attach(handles[1], tf.ctypes.data_as(_lib.c_float_p), sp.ctypes.data_as(_lib.c_float_p), 1) == 0
    rc, out, msg = _call(_lib, handles)
    assert (rc, out) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL) and "attachment" in msg and "envs[1]" in msg, msg
    assert _call(_lib, handles, n_constraints=2)[2] == msg
    assert _call(_lib, handles, drop=("constraints",))[2] == "null pointer"
    assert _call(_lib, handles, record=dict(max_angle=2.0))[2].startswith("constraints[0]: max_angle")
    assert _call(_lib, handles, step=0.0)[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL) and _call(_lib, handles, step=0.0)[2] != msg


def test_no_paths_is_ok_and_held_knows_its_results(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, res, _ = _call(_lib, [], n=0, keep=True)
    assert rc == VMV_OK and res not in (None, SENTINEL)
    calls, validations = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_optimized_summary(res, None, None, None, None, None, None, None, ctypes.byref(calls),
                                   ctypes.byref(validations)) == VMV_OK
    assert (calls.value, validations.value) == (0, 0)
    assert L.vmv_optimized_held(res, None) == VMV_OK
    held = (ctypes.c_uint32 * 1)(77)
    assert L.vmv_optimized_held(res, held) == VMV_OK and held[0] == 77  # no path: nothing is written
    assert L.vmv_optimized_points(res, None, 0) == VMV_OK
    assert L.vmv_optimized_destroy(res) == VMV_OK
    assert _call(_lib, [], n=0, n_constraints=0)[0] == VMV_OK
    assert _call(_lib, [], n=0, record=dict(max_angle=2.0))[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # a refusal wins over the empty batch
    # a result of the unconstrained call carries no such count
    cs = _lib.OptimizeSettings(*[DEFAULTS[k] for k in DEFAULTS])
    plain = ctypes.c_void_p()
    assert L.vmv_optimize_multi(0, None, 0, None, None, ctypes.byref(cs), ctypes.byref(plain)) == VMV_OK
    assert L.vmv_optimized_held(plain, held) == VMV_ERR_INVALID_ARGUMENT and held[0] == 77
    assert L.vmv_optimized_destroy(plain) == VMV_OK
    assert L.vmv_optimized_held(None, None) == VMV_ERR_INVALID_ARGUMENT
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    assert planning.optimize_multi_constrained(vamp.panda, [], [], c) == []
    assert vamp.panda.optimize_multi_constrained([], [], c) == []
    empty = vamp.panda.optimize_multi_constrained_raw([], [], c, planning.OptimizeMultiSettings())
    assert empty["held"].shape == (0,) and empty["held"].dtype == np.uint32
    assert "held" not in vamp.panda.optimize_multi_raw([], [], planning.OptimizeMultiSettings())


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a = np.zeros((4, 7), np.float32)
    env = vamp.Environment()
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.OptimizeMultiSettings

    def f(*args, **kw):
        return planning.optimize_multi_constrained(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f([a, a, a], [env, None], c)  # two environments for three paths
    with pytest.raises(TypeError):
        f([np.zeros((4, 6), np.float32)], [env], c)  # wrong dimension
    with pytest.raises(TypeError):
        f([a, a], [env, "not an environment"], c)
    for kw in (dict(step=0.0), dict(validate_every=0), dict(max_iterations=0), dict(max_waypoints=1025), dict(max_waypoints=3),
               dict(min_change=float("nan")), dict(env_weight=-1.0)):
        with pytest.raises(ValueError):
            f([a], [env], c, S(**kw))
    with pytest.raises(TypeError):
        f([a], [env], "upright")  # not an EEConstraint
    with pytest.raises(TypeError):
        f([a, a], [env, env], [c, None])
    with pytest.raises(ValueError):
        f([a, a, a], [env] * 3, [c, c])  # 1 constraint or one per path
    with pytest.raises(ValueError):
        f([a, a], [env, env], [])
    with pytest.raises(ValueError):
        vamp.panda.optimize_multi_constrained([a, a, a], [env] * 3, [c, c])  # the installed name takes the same road
    with pytest.raises(ValueError):
        f([a, a, a], [env, None], [c, c])  # optimize_multi's checks come first
    long_line = np.stack([np.zeros(7, np.float32), np.full(7, 2.0, np.float32)])
    with pytest.raises(ValueError, match="path 1"):  # densified beyond max_waypoints
        f([a, long_line], [env, env], c, resolution=400.0)
    assert env._handle is None  # nothing was built or finalized


class _FakeRobot:
    """stands where planning expects a robot: records what the raw call was given and answers a fixed dict"""

    def __init__(self):
        self.calls = []

    def dimension(self):
        return 2

    def optimize_multi_constrained_raw(self, paths, environments, constraints, settings, constraint_settings=None):
        self.calls.append((paths, environments, constraints, settings, constraint_settings))
        off = np.cumsum([0] + [len(p) for p in paths])
        pts = np.arange(off[-1] * 2, dtype=np.float32).reshape(-1, 2)
        n = len(paths)
        k = np.arange(n)
        return dict(status=np.array([0, 3, 1, 2], np.uint8)[k % 4], iterations=(3 + k).astype(np.uint32),
                    best_iteration=(1 + k).astype(np.uint32), cost_first=(8.5 + k).astype(np.float32), cost=(4.5 + k).astype(np.float32),
                    clearance_first=np.stack([0.125 + k, -0.25 - k], axis=1).astype(np.float32),
                    clearance=np.stack([0.375 + k, 0.5 + k], axis=1).astype(np.float32), points=pts, offsets=off.astype(np.int64),
                    clearance_calls=5, validation_calls=2, held=np.array([4, 0, 1, 0], np.uint32)[k % 4])


def test_planning_function_on_a_fake_robot(vamp):
    from vamp_mvt_amd import planning

    robot = _FakeRobot()
    paths = [np.zeros((m, 2), np.float32) for m in (3, 4, 2, 1)]
    s = planning.OptimizeMultiSettings(max_iterations=5)
    got = planning.optimize_multi_constrained(robot, paths, ["e0", "e1", "e2", "e3"], "c", s, "cs")
    (given, envs, cons, gs, cs), = robot.calls
    assert (envs, cons, cs) == (["e0", "e1", "e2", "e3"], "c", "cs") and gs is s
    assert [p.tobytes() for p in given] == [p.tobytes() for p in paths]
    assert all(type(r) is planning.ConstrainedOptimizedPath and isinstance(r, planning.OptimizedPath) for r in got)
    assert [r.status for r in got] == ["ok", "out_of_band", "no_valid", "nonfinite"]
    assert [r.held for r in got] == [4, 0, 1, 0] and all(type(r.held) is int for r in got)
    assert [len(r.path) for r in got] == [3, 4, 2, 1] and [r.iterations for r in got] == [3, 4, 5, 6]
    assert np.array_equal(np.stack(got[1].path), np.arange(6, 14, dtype=np.float32).reshape(4, 2))
    assert (got[0].cost_first, got[0].cost, got[0].best_iteration) == (8.5, 4.5, 1) and got[2].clearance == (2.375, 2.5)
    # resolution= densifies first, as optimize_multi does; defaults where nothing is given
    line = np.array([[0.0, 0.0], [1.0, 0.0]], np.float32)
    planning.optimize_multi_constrained(robot, [line], ["e"], "c", resolution=4.0)
    given, _, _, gs, cs = robot.calls[1]
    assert given[0].tobytes() == planning.densify_path(line, 4.0).tobytes() and len(given[0]) == 5
    assert gs == planning.OptimizeMultiSettings() and cs is None
    assert planning.optimize_multi_constrained(robot, [], [], "c") == []


# ---- the serial statement on a planar toy: a disc to keep away from -------------------------------------------------------
CENTRE, RADIUS = np.array([0.5, -0.2], np.float32), f32(0.25)
LOWER, UPPER = np.array([-1.0, -1.0], f32), np.array([2.0, 2.0], f32)
LINE = np.stack([np.linspace(0.0, 1.0, 9), np.full(9, 0.08)], axis=1).astype(f32)  # 3 cm above the disc at x = 0.5
KW = dict(max_iterations=12, validate_every=4, env_margin=0.1)


def _clearance(X):
    X = np.asarray(X, f32)
    d = X - CENTRE[None]
    L = np.sqrt((d * d).sum(1)).astype(f32)
    values = np.stack([L - RADIUS, np.full(len(X), np.inf, f32)], axis=1).astype(f32)
    grads = np.zeros((len(X), 2, 2), f32)
    grads[:, 0] = d / L[:, None]
    return values, grads


def _valid(a, b):
    t = np.linspace(0.0, 1.0, 33)[:, None]
    p = np.asarray(a, np.float64)[None] * (1 - t) + np.asarray(b, np.float64)[None] * t
    return bool((np.linalg.norm(p - CENTRE[None].astype(np.float64), axis=1) > RADIUS).all())


def _free():
    return dict(project=lambda q: (q.copy(), True), in_band=lambda q: True, band_edge=lambda a, b: True)


def _bytes(path):
    return [np.asarray(q, f32).tobytes() for q in path]


def _key(r):
    return (r.status, r.iterations, r.best_iteration, f32(r.cost_first).tobytes(), f32(r.cost).tobytes(),
            np.array(r.clearance_first, f32).tobytes(), np.array(r.clearance, f32).tobytes(), _bytes(r.path))


def test_a_band_that_refuses_nothing_is_the_unconstrained_statement():
    for kw in (KW, dict(KW, validate_every=1), dict(KW, validate_every=100), dict(KW, min_change=0.05), dict(KW, max_step=0.01)):
        want = optimize_serial(LINE, _clearance, _valid, LOWER, UPPER, **kw)
        got = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **_free(), **kw)
        assert _key(got) == _key(want), kw
        assert [tuple(map(repr, h)) for h in got.history] == [tuple(map(repr, h)) for h in want.history]
        assert got.held == 0 and all(t == ([], []) for t in got.trace) and len(got.trace) == got.iterations + 1
    assert want.status == OK and want.best_iteration > 0 and want.cost < want.cost_first  # the toy is no trivial case
    for short in (LINE[:0], LINE[:1], LINE[:2]):
        want = optimize_serial(short, _clearance, _valid, LOWER, UPPER, **KW)
        got = optimize_constrained_serial(short, _clearance, _valid, lower=LOWER, upper=UPPER, **_free(), **KW)
        assert _key(got) == _key(want)


def test_a_projection_that_never_converges_holds_every_waypoint():
    hooks = _free()
    inner = len(LINE) - 2
    asked = []

    def project(q):  # the input's own rows converge (unchanged); later nothing does, and what comes back then is dropped
        asked.append(q.tobytes())
        return (q.copy(), True) if len(asked) <= inner else (q + f32(1.0), False)

    hooks["project"] = project
    got = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert (got.status, got.iterations, got.best_iteration) == (OK, 12, 0)  # iterate 0, validated again and again
    assert _bytes(got.path) == _bytes(LINE) and got.cost == got.cost_first
    assert got.held == got.iterations * inner == 12 * inner
    assert got.trace[0] == ([], []) and all(t == ([], list(range(1, inner + 1))) for t in got.trace[1:]) and len(got.trace) == 13
    assert len({repr(h[0]) for h in got.history}) == 1  # every iterate is iterate 0
    # with min_change so large that the path stops at the first validated iterate: held counts the iterations that ran
    hooks["project"] = lambda q: (q.copy(), False)
    none = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert (none.status, none.iterations, none.held, none.trace) == (OUT_OF_BAND, 0, 0, [])  # the input itself cannot be projected
    calls = []
    hooks["project"] = lambda q: (q.copy(), not calls.append(1) and len(calls) <= inner)
    early = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **dict(KW, min_change=10.0))
    assert (early.status, early.iterations, early.held) == (OK, 4, 4 * inner)


def test_out_of_band_inputs_come_back_as_they_are():
    def never(*a):
        raise AssertionError("a question was asked")

    for end in (0, len(LINE) - 1):
        hooks = dict(project=never, band_edge=never, in_band=lambda q, end=end: q.tobytes() != LINE[end].tobytes())
        got = optimize_constrained_serial(LINE, never, never, lower=LOWER, upper=UPPER, **hooks, **KW)
        assert (got.status, got.iterations, got.best_iteration, got.held, got.history, got.trace) == (OUT_OF_BAND, 0, 0, 0, [], [])
        assert _bytes(got.path) == _bytes(LINE) and got.cost == 0.0 and np.isnan(got.clearance_first[0])
        two = optimize_constrained_serial(LINE[[0, -1]], never, never, lower=LOWER, upper=UPPER, **hooks, **KW)
        assert two.status == OUT_OF_BAND and _bytes(two.path) == _bytes(LINE[[0, -1]])
    # one inner waypoint that cannot be projected
    hooks = dict(_free(), band_edge=never, project=lambda q: (q.copy(), q.tobytes() != LINE[3].tobytes()))
    got = optimize_constrained_serial(LINE, never, never, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert got.status == OUT_OF_BAND and _bytes(got.path) == _bytes(LINE) and got.iterations == 0
    # a non-finite waypoint is looked at before the band; fewer than 2 waypoints: as they are, without any test
    bad = LINE.copy()
    bad[2, 1] = np.nan
    none = dict(project=never, in_band=never, band_edge=never)
    assert optimize_constrained_serial(bad, never, never, lower=LOWER, upper=UPPER, **none, **KW).status == NONFINITE
    for short in (LINE[:0], LINE[:1]):
        got = optimize_constrained_serial(short, never, never, lower=LOWER, upper=UPPER, **none, **KW)
        assert got.status == OK and _bytes(got.path) == _bytes(short)
    # two waypoints in band: the one edge is asked both ways
    hooks = _free()
    assert optimize_constrained_serial(LINE[:2], never, _valid, lower=LOWER, upper=UPPER, **hooks, **KW).status == OK
    hooks["band_edge"] = lambda a, b: False
    assert optimize_constrained_serial(LINE[:2], never, _valid, lower=LOWER, upper=UPPER, **hooks, **KW).status == NO_VALID
    assert optimize_constrained_serial(LINE[:2], never, lambda a, b: False, lower=LOWER, upper=UPPER, **_free(), **KW).status == NO_VALID


def test_a_band_edge_that_fails_at_one_validated_iterate_makes_the_best_skip_it():
    free = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **_free(), **KW)
    validated = [k for k, h in enumerate(free.history) if h[3]]
    assert validated == [0, 4, 8, 12] and all(free.history[k][4] for k in validated)
    best = free.best_iteration
    assert best in (4, 8, 12)
    # the band refuses one edge of exactly that iterate, named by its bits from a run that records every edge asked
    iterates = []
    hooks = _free()
    hooks["band_edge"] = lambda a, b: iterates.append((a.tobytes(), b.tobytes())) or True
    optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    per = len(LINE) - 1
    assert len(iterates) == per * len(validated)
    named = iterates[per * validated.index(best) + 3]  # edge 3 of the best iterate
    hooks["band_edge"] = lambda a, b: (a.tobytes(), b.tobytes()) != named
    got = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert got.status == OK and got.best_iteration != best and got.best_iteration in validated
    assert got.history[best][3:] == (True, False) and [h[0] for h in got.history] == [h[0] for h in free.history]
    others = [free.history[k][0] for k in validated if k != best]
    assert got.cost == min(others) and got.cost >= free.cost and got.iterations == free.iterations
    assert _bytes(got.path) != _bytes(free.path) and got.held == 0
    # a band that refuses every edge of every iterate: the input's bytes, not iterate 0
    hooks["band_edge"] = lambda a, b: False
    hooks["project"] = lambda q: (q + f32(1e-3), True)  # iterate 0 differs from the input
    none = optimize_constrained_serial(LINE, _clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert (none.status, none.iterations, none.best_iteration) == (NO_VALID, 12, 0) and _bytes(none.path) == _bytes(LINE)
    assert none.trace[0][0] == list(range(1, len(LINE) - 1)) and none.cost == none.cost_first


def test_a_projection_that_moves_waypoints_is_what_the_next_iterate_is_computed_from():
    """the projection pulls every inner waypoint onto the line y = 0.1: all later costs are those of points on it"""
    hooks = _free()
    hooks["project"] = lambda q: (np.array([q[0], 0.1], f32), True)
    hooks["in_band"] = lambda q: True
    clearances = []

    def clearance(X):
        clearances.append(np.asarray(X, f32).copy())
        return _clearance(X)

    got = optimize_constrained_serial(LINE, clearance, _valid, lower=LOWER, upper=UPPER, **hooks, **KW)
    assert got.status == OK and got.held == 0 and got.trace[0][0] == list(range(1, len(LINE) - 1))
    assert all((X[1:-1, 1] == f32(0.1)).all() and X[0].tobytes() == LINE[0].tobytes() and X[-1].tobytes() == LINE[-1].tobytes()
               for X in clearances)
    assert all((np.array(got.path)[1:-1, 1] == f32(0.1)))
    assert any(t[0] for t in got.trace[1:])  # a step left the line and was brought back


def test_serial_statement_does_not_import_the_package():
    import os
    import optimize_constrained_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text
