"""vmv_simplify_multi_constrained / planning.simplify_multi_constrained: what holds without a device — every refusal of
the entry point in the header's order with *out untouched, vmv_paths_band_refused on results of either call, the Python
layers' own checks, and the serial statement (tests/simplify_constrained_serial.py) against hand-made band and projection
callbacks on a planar toy problem."""
import ctypes

import numpy as np
import pytest

from simplify_constrained_serial import OUT_OF_BAND, Hooks, simplify_constrained_serial
from simplify_serial import OK, simplify_serial

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 5, 6
OP_BSPLINE, OP_REDUCE, OP_SHORTCUT = 0, 1, 2
SENTINEL = 0x5A5A5A5A
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


def _call(_lib, handles, robot=0, n=None, drop=(), offsets=(0, 4, 7), operations=(OP_SHORTCUT, OP_BSPLINE), n_constraints=1,
          record=None, cfields=None, keep=False, **settings):
    """one vmv_simplify_multi_constrained call with two paths (4 and 3 waypoints); `drop` names the pointers passed as NULL;
    record: fields of the last constraint; cfields: fields of the constraint settings -> (status, *out, vmv_last_error())"""
    n = len(handles) if n is None else n
    pts = np.linspace(0.0, 1.0, 7 * 7, dtype=np.float32).reshape(7, 7)
    s = dict(max_iterations=4, interpolate=0, n_operations=len(operations), bspline_max_steps=5, bspline_min_change=0.05,
             bspline_midpoint_interpolation=0.5, max_waypoints=0, questions_per_round=0, check_every=0)
    s.update(settings)
    ops = (ctypes.c_uint32 * 8)(*(list(operations) + [OP_SHORTCUT] * 8)[:8])
    cs = _lib.SimplifySettings(s["max_iterations"], s["interpolate"], s["n_operations"], ops, s["bspline_max_steps"],
                               s["bspline_min_change"], s["bspline_midpoint_interpolation"], s["max_waypoints"],
                               s["questions_per_round"], s["check_every"])
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
    rc = _lib.lib.vmv_simplify_multi_constrained(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["settings"],
                                                 ptr["constraints"], n_constraints, ptr["constraint_settings"], ptr["out"])
    message = _lib.lib.vmv_last_error().decode()
    if rc == VMV_OK and not keep and "out" not in drop:
        assert _lib.lib.vmv_paths_destroy(out) == VMV_OK
        return rc, None, message
    return rc, out.value, message


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmv_simplify_multi_constrained", "vmv_paths_band_refused"):
        assert name in names and hasattr(dll, name)
    assert vamp.abi_version() == 1  # the change is additive
    assert callable(vamp.panda.simplify_multi_constrained) and callable(vamp.panda.simplify_multi_constrained_raw)
    assert planning.SIMPLIFY_STATUS == ("ok", "capacity", "out_of_band")


def test_refusals_in_the_headers_order(raw):
    """vmv_simplify_multi's checks in its order, then the constraint's own; each pair below spoils two things and the
    earlier check's answer comes back; *out stays as it was"""
    _lib, handles = raw
    refused = lambda **kw: _call(_lib, handles, **kw)[:2]  # noqa: E731
    bad = (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    # ---- vmv_simplify_multi's own, in its order
    for robot in (-1, 4, 7):
        assert refused(robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    assert refused(robot=9, drop=("settings", "constraints")) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    for drop in ("envs", "points", "offsets", "settings", "out"):
        assert refused(drop=(drop,)) == bad, drop
    for w in (1, 3, 12, 65, 128):
        assert refused(questions_per_round=w) == bad
    assert refused(interpolate=64) == bad and refused(n_operations=9) == bad
    assert refused(operations=(OP_REDUCE,)) == bad and refused(operations=(OP_SHORTCUT, 4)) == bad
    assert refused(n=1 << 31) == bad and refused(n=1 << 27, questions_per_round=16) == bad
    assert refused(max_waypoints=3) == bad and refused(max_waypoints=(1 << 24) + 1) == bad
    for offsets in ((0, 5, 4), (1, 4, 7), (3, 2, 7)):
        assert refused(offsets=offsets) == bad
    assert _call(_lib, [handles[0], None])[:2] == bad
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
    assert refused(questions_per_round=3, drop=("constraints",)) == bad
    assert _call(_lib, handles, questions_per_round=3, n_constraints=3)[2] != "n_constraints must be 1 or n_paths"
    assert _call(_lib, handles, drop=("constraints",), n_constraints=3)[2] == "null pointer"
    assert _call(_lib, handles, n_constraints=3, cfields=dict(pos_tol=-1.0))[2] == "n_constraints must be 1 or n_paths"
    assert _call(_lib, handles, cfields=dict(pos_tol=-1.0, check_step=-1.0), record=dict(max_angle=2.0))[2].startswith("pos_tol")
    assert _call(_lib, handles, cfields=dict(check_step=-1.0), record=dict(max_angle=2.0))[2].startswith("check_step")
    # ---- a well-formed call reaches the environments' own checks, which need no device either
    assert refused() == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(n_constraints=2) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(record=dict(max_angle=2.0)) == bad  # a refusal wins over the environments' state
    for w in (0, 2, 4, 8, 16, 32, 64):
        assert refused(questions_per_round=w) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_no_paths_is_ok_and_band_refused_knows_its_results(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, paths, _ = _call(_lib, [], n=0, keep=True)
    assert rc == VMV_OK and paths not in (None, SENTINEL)
    rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_paths_summary(paths, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
    assert (rounds.value, questions.value) == (0, 0)
    assert L.vmv_paths_band_refused(paths, None) == VMV_OK
    assert L.vmv_paths_destroy(paths) == VMV_OK
    assert _call(_lib, [], n=0, n_constraints=0)[0] == VMV_OK
    assert _call(_lib, [], n=0, record=dict(max_angle=2.0))[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # a refusal wins over the empty batch
    # a result of the unconstrained call carries no such count
    cs = _lib.SimplifySettings(4, 0, 0, (ctypes.c_uint32 * 8)(), 5, 0.05, 0.5, 0, 0, 0)
    plain = ctypes.c_void_p()
    assert L.vmv_simplify_multi(0, None, 0, None, None, ctypes.byref(cs), ctypes.byref(plain)) == VMV_OK
    refused = (ctypes.c_uint32 * 1)(77)
    assert L.vmv_paths_band_refused(plain, refused) == VMV_ERR_INVALID_ARGUMENT and refused[0] == 77
    assert L.vmv_paths_destroy(plain) == VMV_OK
    assert L.vmv_paths_band_refused(None, None) == VMV_ERR_INVALID_ARGUMENT
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    assert planning.simplify_multi_constrained(vamp.panda, [], [], c) == []
    assert vamp.panda.simplify_multi_constrained([], [], c) == []
    empty = vamp.panda.simplify_multi_constrained_raw([], [], c, planning.SimplifyMultiSettings())
    assert empty["band_refused"].shape == (0,) and empty["band_refused"].dtype == np.uint32


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a = np.zeros((4, 7), np.float32)
    env = vamp.Environment()
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.SimplifyMultiSettings

    def f(*args, **kw):
        return planning.simplify_multi_constrained(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f([a, a, a], [env, None], c)  # two environments for three paths
    with pytest.raises(TypeError):
        f([np.zeros((4, 6), np.float32)], [env], c)  # wrong dimension
    with pytest.raises(TypeError):
        f([a, a], [env, "not an environment"], c)
    with pytest.raises(NotImplementedError):
        f([a], [env], c, S(operations=["SHORTCUT", "REDUCE"]))
    with pytest.raises(ValueError):
        f([a], [env], c, S(questions_per_round=3))
    with pytest.raises(ValueError):
        f([a], [env], c, S(max_waypoints=3))
    with pytest.raises(TypeError):
        f([a], [env], "upright")  # not an EEConstraint
    with pytest.raises(TypeError):
        f([a, a], [env, env], [c, None])
    with pytest.raises(ValueError):
        f([a, a, a], [env] * 3, [c, c])  # 1 constraint or one per path
    with pytest.raises(ValueError):
        f([a, a], [env, env], [])
    with pytest.raises(ValueError):
        vamp.panda.simplify_multi_constrained([a, a, a], [env] * 3, [c, c])  # the installed name takes the same road
    with pytest.raises(ValueError):
        f([a, a, a], [env, None], [c, c])  # simplify_multi's checks come first
    assert env._handle is None  # nothing was built or finalized


class _FakeRobot:
    """stands where planning expects a robot: records what the raw call was given and answers a fixed dict"""

    def __init__(self):
        self.calls = []

    def simplify_multi_constrained_raw(self, paths, environments, constraints, settings, constraint_settings=None):
        self.calls.append((paths, environments, constraints, settings, constraint_settings))
        pts = np.arange(6 * 2, dtype=np.float32).reshape(6, 2)
        return dict(status=np.array([0, 2, 1], np.uint8), iterations=np.array([3, 0, 1], np.uint32), lengths=np.array([2, 3, 1], np.uint32),
                    questions=np.array([9, 0, 4], np.uint32), points=pts, rounds=5, total_questions=13,
                    band_refused=np.array([4, 0, 1], np.uint32))


def test_planning_function_on_a_fake_robot(vamp):
    from vamp_mvt_amd import planning

    robot = _FakeRobot()
    ref = vamp.SimplifySettings()  # the reference-shaped settings are converted as simplify_multi converts them
    got = planning.simplify_multi_constrained(robot, ["p0", "p1", "p2"], ["e0", "e1", "e2"], "c", ref, "cs")
    (paths, envs, cons, s, cs), = robot.calls
    assert (paths, envs, cons, cs) == (["p0", "p1", "p2"], ["e0", "e1", "e2"], "c", "cs")
    assert isinstance(s, planning.SimplifyMultiSettings) and s == planning._as_simplify_multi_settings(ref)
    assert [r.status for r in got] == ["ok", "out_of_band", "capacity"]
    assert [r.band_refused for r in got] == [4, 0, 1] and all(type(r.band_refused) is int for r in got)
    assert [len(r.path) for r in got] == [2, 3, 1] and [r.iterations for r in got] == [3, 0, 1]
    assert np.array_equal(np.stack(got[1].path), np.arange(4, 10, dtype=np.float32).reshape(3, 2))
    assert got[0].cost == planning.path_cost(got[0].path) and got[2].cost == float("inf")
    assert (got[0].validity_calls, got[0].edges_checked) == (5, 13) and got[1].edges_checked == 0 and got[2].edges_checked == 4
    planning.simplify_multi_constrained(robot, [], [], "c")
    assert robot.calls[1][3] == planning.SimplifyMultiSettings() and robot.calls[1][4] is None


# ---- the serial statement on a planar toy: a disc to go around ------------------------------------------------------------
CENTRE, RADIUS = np.array([0.5, 0.0]), 0.3
ZIGZAG = [(0.0, 0.0), (0.1, 0.3), (0.3, 0.5), (0.5, 0.55), (0.7, 0.5), (0.9, 0.3), (1.0, 0.0)]


def _valid(a, b):
    t = np.linspace(0.0, 1.0, 129)[:, None]
    p = np.asarray(a, np.float64)[None] * (1 - t) + np.asarray(b, np.float64)[None] * t
    return bool((np.linalg.norm(p - CENTRE[None], axis=1) > RADIUS).all())


def _free():
    return Hooks(band_point=lambda q: True, band_edge=lambda a, b: True, project=lambda q: (q.copy(), True))


def _bytes(path):
    return [np.asarray(q, f32).tobytes() for q in path]


def test_a_band_that_refuses_nothing_is_the_unconstrained_statement():
    for kw in (dict(), dict(max_waypoints=16), dict(operations=("BSPLINE", "SHORTCUT"), max_iterations=2), dict(min_change=0.01)):
        want = simplify_serial(ZIGZAG, _valid, **kw)
        got = simplify_constrained_serial(ZIGZAG, _valid, _free(), **kw)
        assert (got.status, got.iterations, got.questions) == (want.status, want.iterations, want.questions), kw
        assert _bytes(got.path) == _bytes(want.path) and got.trace == want.trace
        assert got.band_refused == 0 and len(got.asked) == got.questions and not any(r for _, r, _ in got.asked)
        assert got.projected and not any(moved for _, _, _, moved, _ in got.projected) and all(c for _, _, c, _, _ in got.projected)
        assert sum(r for *_, r in got.projected) == sum(1 for t in want.trace if t[0] == "bspline" for _, a, b in t[3] if a and b)
    assert want.erased and want.replaced and len(want.path) > 2  # the toy is no trivial case


def test_a_band_that_refuses_one_named_shortcut_edge():
    log = []

    def logged(a, b):
        log.append((a.tobytes(), b.tobytes(), _valid(a, b)))
        return log[-1][2]

    plain = simplify_serial(ZIGZAG, logged)
    assert plain.trace[0] == ("direct",) and not log[0][2] and plain.trace[1][0] == "shortcut" and plain.trace[1][3] is not None
    named = next((a, b) for a, b, ok in log[1:] if ok)  # the first shortcut the unconstrained loop takes
    hooks = _free()
    hooks.band_edge = lambda a, b: (a.tobytes(), b.tobytes()) != named
    got = simplify_constrained_serial(ZIGZAG, _valid, hooks)
    assert got.status == OK and got.band_refused >= 1
    assert got.band_refused == sum(r for _, r, _ in got.asked) and all(kind == "shortcut" and ok for kind, r, ok in got.asked if r)
    # waypoint 0 goes on to the next candidate: found one rank later than without the band
    assert got.trace[1][:3] == plain.trace[1][:3] and got.trace[1][3] == plain.trace[1][3] + 1
    edges = set(zip(_bytes(got.path)[:-1], _bytes(got.path)[1:]))
    assert named not in edges and _bytes(got.path) != _bytes(plain.path)
    assert got.path[0].tobytes() == plain.path[0].tobytes() and got.path[-1].tobytes() == plain.path[-1].tobytes()
    assert all(_valid(a, b) for a, b in zip(got.path[:-1], got.path[1:]))


def test_a_projection_back_onto_the_waypoint_is_refused_by_the_second_min_change_test():
    path = [np.array(p, f32) for p in ((0.0, 0.0), (0.5, 0.6), (1.0, 0.0))]  # around the disc by one corner
    assert not _valid(path[0], path[2])
    free = simplify_constrained_serial(path, _valid, _free(), operations=("BSPLINE",), max_iterations=1, max_steps=1)
    assert free.trace[1] == ("bspline", 0, 5, [(2, True, True)]) and free.path[2].tobytes() != path[1].tobytes()
    hooks = _free()
    hooks.project = lambda q: (path[1].copy(), True)  # every midpoint is moved back onto the corner
    got = simplify_constrained_serial(path, _valid, hooks, operations=("BSPLINE",), max_iterations=1, max_steps=1)
    assert got.trace[1] == ("bspline", 0, 5, [(2, True, True)])  # both motions were asked and answered 1 ...
    assert free.projected == [(0, 2, True, False, True)]
    assert got.projected == [(0, 2, True, True, False)] and got.band_refused == 0 and got.questions == 3
    assert got.path[2].tobytes() == path[1].tobytes() and len(got.path) == 5  # ... and the waypoint stays
    assert got.iterations == 1 and got.status == OK
    # a projection that does not converge: the first motion is asked and refused, the second is not asked
    hooks.project = lambda q: (q.copy(), False)
    lost = simplify_constrained_serial(path, _valid, hooks, operations=("BSPLINE",), max_iterations=1, max_steps=1)
    assert lost.trace[1] == ("bspline", 0, 5, [(2, False, None)]) and lost.band_refused == 1 and lost.questions == 2
    assert lost.asked == [("direct", False, False), ("bspline", True, None)] and lost.path[2].tobytes() == path[1].tobytes()
    assert lost.projected == [(0, 2, False, False, False)]


def test_an_out_of_band_input_comes_back_as_it_is():
    def never(a, b):
        raise AssertionError("a validity question was asked")

    pts = [np.array(p, f32) for p in ZIGZAG]
    hooks = _free()
    hooks.band_edge = lambda a, b: (a.tobytes(), b.tobytes()) != (pts[3].tobytes(), pts[4].tobytes())  # an interior edge
    got = simplify_constrained_serial(ZIGZAG, never, hooks)
    assert (got.status, got.iterations, got.questions, got.band_refused, got.trace) == (OUT_OF_BAND, 0, 0, 0, [])
    assert _bytes(got.path) == _bytes(pts)
    hooks = _free()
    hooks.band_point = lambda q: False  # the first waypoint is the one the edge tests do not sample
    got = simplify_constrained_serial(ZIGZAG, never, hooks)
    assert got.status == OUT_OF_BAND and _bytes(got.path) == _bytes(pts)
    # fewer than 3 waypoints: as they are, without any test
    none = Hooks(band_point=never, band_edge=never, project=never)
    for short in (ZIGZAG[:0], ZIGZAG[:1], ZIGZAG[:2]):
        got = simplify_constrained_serial(short, never, none)
        assert got.status == OK and _bytes(got.path) == _bytes(short) and got.questions == 0
