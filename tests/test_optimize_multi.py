"""vmv_optimize_multi / planning.optimize_multi: what holds without a device — the ABI surface, the checks that come before
any device query, the Python wrapper's argument checks, and the serial statement's (tests/optimize_serial.py) own
properties with float64 CPU clearances (tests/optimize_cases.py) and the CPU oracle answering the edge questions."""
import ctypes

import numpy as np
import pytest

import envs
from optimize_cases import GRAZE_CENTRE, Clearance64, graze_line, graze_radius, straight
from optimize_serial import NO_VALID, NONFINITE, OK, optimize_serial, reciprocals, solve
from oracle_lib import CAGE_GOAL, CAGE_START

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_CAPACITY = 0, 1, 2, 4
VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 5, 6
NAMES = ("vmv_optimize_multi", "vmv_optimized_summary", "vmv_optimized_points", "vmv_optimized_destroy")
SENTINEL = 0x5A5A5A5A
DEFAULTS = dict(max_iterations=64, validate_every=8, step=1.0 / 40.0, max_step=0.1, min_change=1e-4, smooth_weight=1.0,
                env_weight=1.0, self_weight=1.0, env_margin=0.05, self_margin=0.01, max_waypoints=0)


def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None
    assert vamp.abi_version() == 1  # the change is additive
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.optimize_multi) and callable(robot.optimize_multi_raw)
    s = planning.OptimizeMultiSettings()
    assert {k: getattr(s, k) for k in DEFAULTS} == dict(DEFAULTS, max_waypoints=1024)
    assert planning.OPTIMIZE_STATUS == ("ok", "no_valid", "nonfinite")
    assert ctypes.sizeof(_lib.OptimizeSettings) == 44


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


def _call(_lib, handles, robot=0, n=None, drop=(), offsets=(0, 4, 7), **settings):
    """one vmv_optimize_multi call with two paths (4 and 3 waypoints); `drop` names the pointers passed as NULL ->
    (status, *out, vmv_last_error())"""
    n = len(handles) if n is None else n
    pts = np.linspace(0.0, 1.0, 7 * 7, dtype=np.float32).reshape(7, 7)
    s = dict(DEFAULTS)
    s.update(settings)
    cs = _lib.OptimizeSettings(*[s[k] for k in DEFAULTS])
    out = ctypes.c_void_p(SENTINEL)
    off = np.ascontiguousarray(offsets, np.uintp)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "points": pts.ctypes.data_as(_lib.c_float_p),
           "offsets": off.ctypes.data_as(_lib.c_size_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_optimize_multi(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["settings"], ptr["out"])
    return rc, out.value, _lib.lib.vmv_last_error()


def _refused(result, status=VMV_ERR_INVALID_ARGUMENT):
    return result[:2] == (status, SENTINEL)


def test_unknown_robot(raw):
    _lib, make = raw
    handles = [make(), make()]
    for robot in (-1, 4, 7):
        assert _refused(_call(_lib, handles, robot=robot), VMV_ERR_UNKNOWN_ROBOT)


@pytest.mark.parametrize("drop", ["envs", "points", "offsets", "settings", "out"])
def test_null_pointers(raw, drop):
    _lib, make = raw
    assert _refused(_call(_lib, [make(), make()], drop=(drop,)))


def test_null_handle(raw):
    _lib, make = raw
    assert _refused(_call(_lib, [make(), None]))
    assert _refused(_call(_lib, [None, make()]))


@pytest.mark.parametrize("offsets", [(0, 5, 4), (1, 4, 7), (3, 2, 7)])
def test_offsets_must_start_at_zero_and_not_decrease(raw, offsets):
    _lib, make = raw
    assert _refused(_call(_lib, [make(), make()], offsets=offsets))


def test_max_waypoints(raw):
    _lib, make = raw
    handles = [make(), make()]
    assert _refused(_call(_lib, handles, max_waypoints=3))  # below the longer path
    assert _refused(_call(_lib, handles, max_waypoints=4), VMV_ERR_NOT_FINALIZED)
    assert _refused(_call(_lib, handles, max_waypoints=1024), VMV_ERR_NOT_FINALIZED)
    assert _refused(_call(_lib, handles, max_waypoints=1025))  # the cap
    assert _refused(_call(_lib, handles, offsets=(0, 1025, 1028)))  # longer than the default (no waypoint is read)


@pytest.mark.parametrize("name", ["step", "max_step", "env_margin", "self_margin"])
@pytest.mark.parametrize("value", [0.0, -1.0, float("inf"), float("nan")])
def test_steps_and_margins_must_be_positive_and_finite(raw, name, value):
    _lib, make = raw
    assert _refused(_call(_lib, [make(), make()], **{name: value}))


@pytest.mark.parametrize("name", ["smooth_weight", "env_weight", "self_weight"])
def test_weights_must_be_finite_and_not_negative(raw, name):
    _lib, make = raw
    handles = [make(), make()]
    for value in (-1e-3, float("inf"), float("nan")):
        assert _refused(_call(_lib, handles, **{name: value}))
    assert _refused(_call(_lib, handles, **{name: 0.0}), VMV_ERR_NOT_FINALIZED)  # a zero weight is a setting


def test_validate_every_and_min_change(raw):
    _lib, make = raw
    handles = [make(), make()]
    assert _refused(_call(_lib, handles, validate_every=0))
    assert _refused(_call(_lib, handles, min_change=float("nan")))
    assert _refused(_call(_lib, handles, validate_every=1000, min_change=-1.0, max_iterations=0), VMV_ERR_NOT_FINALIZED)


def test_count_limits(raw):
    _lib, make = raw
    h = make()
    assert _refused(_call(_lib, [h, h], n=1 << 31))  # (no array is read)
    n = 1 << 21  # 2^21 paths of 1,024 waypoints: 2^31 waypoints in all (no waypoint is read)
    from vamp_mvt_amd import _lib as L

    offsets = np.arange(n + 1, dtype=np.uintp) * 1024
    handles = (ctypes.c_void_p * n)(*([h] * n))
    cs = L.OptimizeSettings(*[DEFAULTS[k] for k in DEFAULTS])
    out = ctypes.c_void_p(SENTINEL)
    pts = np.zeros((1, 7), np.float32)
    rc = L.lib.vmv_optimize_multi(0, handles, n, pts.ctypes.data_as(L.c_float_p), offsets.ctypes.data_as(L.c_size_p),
                                  ctypes.byref(cs), ctypes.byref(out))
    assert (rc, out.value) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    offsets[-1] -= 1  # one waypoint fewer passes this check and reaches the environments'
    rc = L.lib.vmv_optimize_multi(0, handles, n, pts.ctypes.data_as(L.c_float_p), offsets.ctypes.data_as(L.c_size_p),
                                  ctypes.byref(cs), ctypes.byref(out))
    assert (rc, out.value) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def _fp(a):
    from vamp_mvt_amd import _lib

    return a.ctypes.data_as(_lib.c_float_p)


def _add_cloud(_lib, h, kind):
    pts = np.random.default_rng(3).uniform(0.3, 0.9, (64, 3)).astype(np.float32)
    if kind == "capt":
        rc = _lib.lib.vmv_env_add_capt_pointcloud(h, _fp(pts), len(pts), 0.01, 0.1, 0.005, None)
    else:
        lo, hi = np.full(3, -2.0, np.float32), np.full(3, 2.0, np.float32)
        rc = _lib.lib.vmv_env_add_mvt_pointcloud(h, _fp(pts), len(pts), 0.01, 0.1, _fp(lo), _fp(hi), 0.005, None, None)
    assert rc == 0, _lib.lib.vmv_last_error()


def _attach(_lib, h):
    tf = np.eye(4, dtype=np.float32)
    sp = np.array([[0, 0, 0.1, 0.03]], np.float32)
    assert _lib.lib.vmv_env_attach(h, _fp(tf), _fp(sp), 1) == 0


@pytest.mark.parametrize("kind, word", [("capt", b"CAPT"), ("mvt", b"MVT"), ("attach", b"attachment")])
def test_out_of_scope_kinds_are_refused_as_the_clearance_calls_refuse_them(raw, kind, word):
    """a point cloud or an attachment: the status and the message of vmv_clearance_batch_multi, naming the kind and the
    index, before the finalized check (both environments are unfinalized) and before any device query"""
    _lib, make = raw
    h, plain = make(), make()
    _attach(_lib, h) if kind == "attach" else _add_cloud(_lib, h, kind)
    rc, out, msg = _call(_lib, [plain, h])
    assert (rc, out) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL) and word in msg and b"envs[1]" in msg, msg
    # word for word the clearance call's own refusal
    qa, values = np.zeros((8, 7), np.float32), np.zeros((8, 2), np.float32)
    offs = np.array([0, 4, 8], np.uintp)
    rc2 = _lib.lib.vmv_clearance_batch_multi(0, (ctypes.c_void_p * 2)(plain, h), offs.ctypes.data_as(_lib.c_size_p), 2,
                                             ctypes.c_void_p(qa.ctypes.data), ctypes.c_void_p(values.ctypes.data), None, None)
    assert rc2 == rc and _lib.lib.vmv_last_error() == msg
    rc, out, msg = _call(_lib, [h, plain])
    assert (rc, out) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL) and word in msg and b"envs[0]" in msg, msg
    # the settings' checks come first
    assert _refused(_call(_lib, [plain, h], step=0.0))


def test_unfinalized_environment_is_reported_without_a_device(raw):
    _lib, make = raw
    a = make()
    assert _refused(_call(_lib, [a, make()]), VMV_ERR_NOT_FINALIZED)
    assert _refused(_call(_lib, [a, a]), VMV_ERR_NOT_FINALIZED)  # repeated handles are allowed


def test_no_paths_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, res, _ = _call(_lib, [], n=0)
    assert rc == VMV_OK and res not in (None, SENTINEL)
    calls, validations = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_optimized_summary(res, None, None, None, None, None, None, None, ctypes.byref(calls),
                                   ctypes.byref(validations)) == VMV_OK
    assert (calls.value, validations.value) == (0, 0)
    assert L.vmv_optimized_points(res, None, 0) == VMV_OK
    assert L.vmv_optimized_destroy(res) == VMV_OK
    assert L.vmv_optimized_summary(None, None, None, None, None, None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_optimized_points(None, None, 0) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_optimized_destroy(None) == VMV_ERR_INVALID_ARGUMENT
    assert planning.optimize_multi(vamp.panda, [], []) == []
    assert vamp.panda.optimize_multi([], []) == []


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.optimize_multi(vamp.panda, [straight(CAGE_START, CAGE_GOAL, 9)], [None])
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a = np.zeros((4, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.OptimizeMultiSettings

    def f(*args, **kw):
        return planning.optimize_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f([a, a, a], [env, None])  # two environments for three paths
    with pytest.raises(TypeError):
        f([np.zeros((4, 6), np.float32)], [env])  # wrong dimension
    with pytest.raises(TypeError):
        f([a[0]], [env])  # one waypoint still is a [1][dim] array
    with pytest.raises(TypeError):
        f([a, a], [env, "not an environment"])
    for kw in (dict(step=0.0), dict(max_step=-1.0), dict(env_margin=float("nan")), dict(self_margin=float("inf")),
               dict(smooth_weight=-1.0), dict(env_weight=float("nan")), dict(validate_every=0), dict(max_iterations=0),
               dict(max_waypoints=1025), dict(max_waypoints=3), dict(min_change=float("nan")), dict(max_iterations=2 ** 32)):
        with pytest.raises(ValueError):
            f([a], [env], S(**kw))
    long_line = np.stack([np.zeros(7, np.float32), np.full(7, 2.0, np.float32)])
    with pytest.raises(ValueError, match="path 1"):  # 2 * sqrt(7) * 400 samples: beyond max_waypoints
        f([a, long_line], [env, env], resolution=400.0)
    with pytest.raises(ValueError):
        vamp.panda.optimize_multi([a, a, a], [env, None], S())  # the installed name takes the same road
    assert env._handle is None  # nothing was built or finalized


def test_densification_keeps_the_waypoints_and_follows_path_samples(vamp):
    from vamp_mvt_amd import planning

    rng = np.random.default_rng(5)
    p = rng.uniform(-2, 2, (6, 7)).astype(np.float32)
    p[3] = p[2]  # a repeated waypoint: a segment of length 0 still yields its end
    for res in (1.0, 8.0, 32.0):
        d = planning.densify_path(p, res)
        samples, at = planning.path_samples(p, res)
        first = np.concatenate([[True], at[1:, 1] != 0])  # drop k = 0 of every segment but the first
        assert d.dtype == np.float32 and len(d) == int(first.sum())
        # every former waypoint is among the new ones, bit for bit and in order
        ends = np.cumsum([0] + [int((at[:, 0] == i).sum()) - 1 for i in range(len(p) - 1)])
        assert [d[e].tobytes() for e in ends] == [q.tobytes() for q in p]
        # and the samples between them are path_samples' own
        inner = np.ones(len(d), bool)
        inner[ends] = False
        assert np.array_equal(d[inner], samples[first][inner])
    assert len(planning.densify_path(p[:1], 8.0)) == 1 and len(planning.densify_path(p[:0], 8.0)) == 0


# ---- the serial statement's own properties ------------------------------------------------------------------------

# Bound on |Thomas solve in fp32 - float64 dense solve|_inf / |float64 solution|_inf.  A = tridiag(-1, 2, -1) is a
# symmetric M-matrix: its LU factors have the sign pattern of A, so |L||U| = |A| and the recurrence is componentwise
# backward stable: (A + dA) z^ = G with |dA| <= g |A| (Higham, Accuracy and Stability, 9.13 / 9.14: g = 4u + O(u^2) for
# the tridiagonal solve with divisions; the reciprocals r_i are rounded once more and multiplied instead, one further
# rounding per pivot, and G itself is rounded to fp32 on input: g <= 8u with u = 2^-24).  Hence |z^ - z|_inf <=
# g cond_inf(A) |z^|_inf with cond_inf(A) = |A|_inf |A^-1|_inf = 4 * (n + 1)^2 / 8 for odd n (the row sums of A^-1 are
# i (n + 1 - i) / 2), at most (n + 1)^2 / 2.  Derived, not fitted.
def solve_bound(n):
    return 8.0 * 2.0 ** -24 * (n + 1) ** 2 / 2.0


@pytest.mark.parametrize("n", [1, 2, 63, 1022])
def test_solve_agrees_with_the_dense_solve(n):
    rng = np.random.default_rng(n)
    G = rng.normal(0, 1, (n, 7)).astype(np.float32)
    A = 2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    want = np.linalg.solve(A, G.astype(np.float64))
    r = reciprocals(n)
    assert r.dtype == np.float32 and r[0] == np.float32(0.5)
    assert np.abs(r.astype(np.float64) - np.arange(1, n + 1) / np.arange(2, n + 2)).max() <= (n + 1) * 2.0 ** -24  # i / (i + 1)
    got = solve(G, r)
    assert got.dtype == np.float32 and got.shape == G.shape
    err = np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)
    print(f"n = {n}: relative error {err.max():.3g}, bound {solve_bound(n):.3g}")
    assert (err <= solve_bound(n)).all()
    # and the float64 form of the same recurrence is the dense solve to float64's own bound
    got64 = solve(G.astype(np.float64), reciprocals(n, np.float64))
    assert (np.abs(got64 - want).max(axis=0) / np.abs(want).max(axis=0) <= 8.0 * 2.0 ** -53 * (n + 1) ** 2 / 2.0).all()


@pytest.fixture(scope="module")
def panda(oracle):
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return rid, lower, (lower + span).astype(np.float32)


@pytest.fixture(scope="module")
def graze(oracle, panda):
    """the grazing case at 17 waypoints: one sphere 5 mm from the straight line's waypoints"""
    rid, lower, upper = panda
    X = graze_line(17, np.float64)
    radius = graze_radius(lambda r: Clearance64("panda", [("sphere", np.array([*GRAZE_CENTRE, r], np.float32))])(X)[0][:, 0].min())
    spec = [("sphere", np.array([*GRAZE_CENTRE, radius], np.float32))]
    oenv = envs.build_oracle_env(oracle, spec)
    return X, Clearance64("panda", spec), lambda a, b: oracle.validate_motion(rid, oenv, np.asarray(a, np.float32),
                                                                             np.asarray(b, np.float32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_serial_statement_on_the_grazing_case(panda, graze, dtype):
    _, lower, upper = panda
    X, clearance, question = graze
    assert all(question(a, b) for a, b in zip(X[:-1], X[1:]))  # the input is valid
    before = X.copy()
    r = optimize_serial(X.astype(dtype), clearance, question, lower, upper, dtype=dtype)
    assert np.array_equal(X, before)
    assert r.status == OK and r.iterations == 64 and len(r.path) == len(X)
    assert r.path[0].tobytes() == X[0].astype(dtype).tobytes() and r.path[-1].tobytes() == X[-1].astype(dtype).tobytes()
    assert abs(r.clearance_first[0] - 0.005) < 1e-5 and abs(r.clearance_first[1] - 0.0152) < 1e-4
    assert r.cost <= r.cost_first and r.clearance[0] >= 0.045  # (the float64 prototype: 0.048 at 17 waypoints)
    assert all(question(a, b) for a, b in zip(r.path[:-1], r.path[1:]))
    validated = [k for k, h in enumerate(r.history) if h[3]]
    assert validated == [0, 8, 16, 24, 32, 40, 48, 56, 64]
    valid_costs = [r.history[k][0] for k in validated if r.history[k][4]]
    assert r.cost == min(valid_costs) and r.history[r.best_iteration][0] == r.cost


def test_serial_statement_entry_cases_and_stopping(panda, graze):
    _, lower, upper = panda
    X, clearance, question = graze
    X = X.astype(np.float32)

    def never(*a):
        raise AssertionError("a question was asked")

    assert optimize_serial(X[:0], never, never, lower, upper).path == []
    one = optimize_serial(X[:1], never, never, lower, upper)
    assert (one.status, one.iterations, len(one.path)) == (OK, 0, 1) and one.path[0].tobytes() == X[0].tobytes()
    two = optimize_serial(X[:2], never, question, lower, upper)
    assert (two.status, two.iterations) == (OK, 0) and [q.tobytes() for q in two.path] == [X[0].tobytes(), X[1].tobytes()]
    assert optimize_serial(X[:2], never, lambda a, b: False, lower, upper).status == NO_VALID
    bad = X.copy()
    bad[5, 2] = np.nan
    r = optimize_serial(bad, never, never, lower, upper)
    assert r.status == NONFINITE and np.array(r.path).tobytes() == bad.tobytes()
    # no valid iterate: the input comes back
    r = optimize_serial(X, clearance, lambda a, b: False, lower, upper, max_iterations=8, validate_every=4)
    assert (r.status, r.iterations, r.best_iteration) == (NO_VALID, 8, 0) and np.array(r.path).tobytes() == X.tobytes()
    assert r.cost == r.cost_first
    # a large min_change stops at the first validated iterate after 0; validate_every above max_iterations: 0 and the last
    r = optimize_serial(X, clearance, question, lower, upper, min_change=10.0, validate_every=3)
    assert r.iterations == 3 and [k for k, h in enumerate(r.history) if h[3]] == [0, 3]
    r = optimize_serial(X, clearance, question, lower, upper, max_iterations=5, validate_every=100)
    assert r.iterations == 5 and [k for k, h in enumerate(r.history) if h[3]] == [0, 5]
    # the iterates do not depend on validate_every
    a = optimize_serial(X, clearance, question, lower, upper, max_iterations=6, validate_every=1)
    b = optimize_serial(X, clearance, question, lower, upper, max_iterations=6, validate_every=6)
    assert [h[0] for h in a.history] == [h[0] for h in b.history]


def test_serial_statement_never_returns_worse_than_a_valid_input(oracle, panda):
    """a scene of rotated cuboids and capsules: straight lines between valid configurations; where the input is valid the
    output is valid with U <= U_0, where it collides the result is a repair or the input"""
    rid, lower, upper = panda
    spec = envs.spec_for("mixed", "panda")
    oenv = envs.build_oracle_env(oracle, spec)
    clearance = Clearance64("panda", spec)

    def question(a, b):
        return oracle.validate_motion(rid, oenv, np.asarray(a, np.float32), np.asarray(b, np.float32))

    rng = np.random.default_rng(2)
    q = (lower + (upper - lower) * rng.random((256, 7), dtype=np.float32)).astype(np.float32)
    q = q[oracle.validate_batch(rid, oenv, q)]
    seen = set()
    for a, b in zip(q[0:12:2], q[1:12:2]):
        X = straight(a, a + (b - a) * np.float32(0.3), 9)
        valid = all(question(u, v) for u, v in zip(X[:-1], X[1:]))
        r = optimize_serial(X, clearance, question, lower, upper, max_iterations=16, validate_every=4)
        assert r.path[0].tobytes() == X[0].tobytes() and r.path[-1].tobytes() == X[-1].tobytes()
        if valid:
            assert r.status == OK and r.cost <= r.cost_first
        if r.status == OK:
            assert all(question(u, v) for u, v in zip(r.path[:-1], r.path[1:]))
        else:
            assert r.status == NO_VALID and np.array(r.path).tobytes() == X.tobytes()
        seen.add((valid, r.status))
    assert (True, OK) in seen


def test_serial_statement_does_not_import_the_package():
    import os
    import optimize_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text
