"""vmv_simplify_multi / planning.simplify_multi: what holds without a device — the serial comparator's own figures (the
contract of DESIGN §5d restated in tests/simplify_serial.py, with the CPU oracle answering every question), the ABI
surface, the checks that come before any device query, and the Python wrapper's argument checks."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE
from rrtc_serial import rrtc_serial
from simplify_serial import BSPLINE, CAPACITY, OK, SHORTCUT, simplify_serial, windowed_questions

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_CAPACITY = 0, 1, 2, 4
VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 5, 6
OP_BSPLINE, OP_REDUCE, OP_SHORTCUT, OP_PERTURB = 0, 1, 2, 3
NAMES = ("vmv_simplify_multi", "vmv_paths_summary", "vmv_paths_points", "vmv_paths_destroy")
SENTINEL = 0x5A5A5A5A

# skip of the RRT-Connect path (range 1.0) -> input length, status, iterations, output length, questions (asked
# serially), first 16 hex digits of sha256 over the output waypoints' bytes; default settings
CAGE_FIGURES = [
    (0, 14, OK, 4, 9, 159, "1325830f2a33a8a1"),
    (2000, 11, OK, 4, 9, 131, "bbb07aeac624719e"),
    (5000, 14, OK, 4, 11, 272, "8fe82d54af96828e"),
]


def path_hash(path):
    return hashlib.sha256(b"".join(np.asarray(q, np.float32).tobytes() for q in path)).hexdigest()[:16]


@pytest.fixture(scope="module")
def cage(oracle):
    env = oracle.env()
    for c in SPHERE_CAGE:
        env.add_sphere(*c, 0.2)
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return rid, env, lower, span


@pytest.fixture(scope="module")
def cage_paths(oracle, cage):
    rid, env, lower, span = cage
    return {skip: rrtc_serial(CAGE_START, CAGE_GOAL, lower, span, lambda a, b: oracle.validate_motion(rid, env, a, b),
                              range_=1.0, skip=skip).path for skip in (0, 2000, 5000)}


@pytest.mark.parametrize("skip, n_in, status, iterations, n_out, questions, digest", CAGE_FIGURES)
def test_comparator_figures_on_the_sphere_cage(oracle, cage, cage_paths, skip, n_in, status, iterations, n_out, questions, digest):
    rid, env, _, _ = cage
    asked = []

    def question(a, b):
        asked.append((a.copy(), b.copy()))
        return oracle.validate_motion(rid, env, a, b)

    path = cage_paths[skip]
    before = [q.copy() for q in path]
    r = simplify_serial(path, question)
    assert len(path) == n_in and all(np.array_equal(a, b) for a, b in zip(path, before))  # the input is left alone
    assert (r.status, r.iterations, len(r.path), r.questions) == (status, iterations, n_out, questions)
    assert r.questions == len(asked) and path_hash(r.path) == digest
    assert r.path[0].tobytes() == path[0].tobytes() and r.path[-1].tobytes() == path[-1].tobytes()
    assert all(oracle.validate_motion(rid, env, a, b) for a, b in zip(r.path[:-1], r.path[1:]))
    assert r.erased and r.replaced
    # the windowed form asks whole windows and both motions of a candidate: never fewer questions than the serial one
    assert all(windowed_questions(r.trace, w) >= r.questions for w in (2, 4, 8, 16, 32, 64))


def test_comparator_entry_cases(oracle, cage, cage_paths):
    rid, env, _, _ = cage

    def never(a, b):
        raise AssertionError("a question was asked")

    path = cage_paths[0]
    assert simplify_serial([], never).path == []
    one = simplify_serial(path[:1], never)
    assert len(one.path) == 1 and one.path[0].tobytes() == path[0].tobytes() and one.iterations == 0
    two = simplify_serial([path[0], path[-1]], never)  # (front, back) without a question, valid or not
    assert [q.tobytes() for q in two.path] == [path[0].tobytes(), path[-1].tobytes()] and two.questions == 0
    free = oracle.env()
    direct = simplify_serial(path, lambda a, b: oracle.validate_motion(rid, free, a, b))
    assert (len(direct.path), direct.iterations, direct.questions) == (2, 0, 1)
    assert [q.tobytes() for q in direct.path] == [path[0].tobytes(), path[-1].tobytes()]


def test_comparator_capacity_and_operation_lists(oracle, cage, cage_paths):
    rid, env, _, _ = cage
    q = lambda a, b: oracle.validate_motion(rid, env, a, b)  # noqa: E731
    path = cage_paths[0]
    # shortcut leaves 4 waypoints, two subdivisions make 7 and 13 of them, the third would need 25
    r = simplify_serial(path, q, max_waypoints=len(path))
    assert (r.status, r.iterations, len(r.path)) == (CAPACITY, 1, 13)
    assert r.path[0].tobytes() == path[0].tobytes() and r.path[-1].tobytes() == path[-1].tobytes()
    assert all(q(a, b) for a, b in zip(r.path[:-1], r.path[1:]))
    s = simplify_serial(path, q, operations=(SHORTCUT,))
    assert (s.status, s.iterations, len(s.path)) == (OK, 2, 4)  # the second iteration changes nothing
    b = simplify_serial(path, q, operations=(BSPLINE, SHORTCUT, SHORTCUT), max_iterations=1)
    assert b.status == OK and b.iterations == 1 and b.trace[1][:3] == ("bspline", 0, 2 * len(path) - 1)
    assert simplify_serial(path, q, max_iterations=0).iterations == 0
    assert simplify_serial(path, q, operations=()).iterations == 1  # an iteration in which nothing changed
    with pytest.raises(ValueError):
        simplify_serial(path, q, max_waypoints=len(path) - 1)


def test_comparator_does_not_import_the_package():
    import os
    import simplify_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
    assert vamp.abi_version() == 1  # the change is additive
    assert callable(vamp.panda.simplify_multi) and callable(vamp.panda.simplify_multi_raw)
    s = planning.SimplifyMultiSettings()
    assert (s.max_iterations, list(s.operations), s.max_steps, s.min_change, s.midpoint_interpolation, s.max_waypoints) == \
        (4, ["SHORTCUT", "BSPLINE"], 5, 0.05, 0.5, 2048)


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


def _call(_lib, handles, robot=0, n=None, drop=(), offsets=(0, 4, 7), operations=(OP_SHORTCUT, OP_BSPLINE), **settings):
    """one vmv_simplify_multi call with two paths (4 and 3 waypoints); `drop` names the pointers passed as NULL ->
    (status, *out)"""
    n = len(handles) if n is None else n
    pts = np.linspace(0.0, 1.0, 7 * 7, dtype=np.float32).reshape(7, 7)
    s = dict(max_iterations=4, interpolate=0, n_operations=len(operations), bspline_max_steps=5, bspline_min_change=0.05,
             bspline_midpoint_interpolation=0.5, max_waypoints=0, questions_per_round=0, check_every=0)
    s.update(settings)
    ops = (ctypes.c_uint32 * 8)(*(list(operations) + [OP_SHORTCUT] * 8)[:8])
    cs = _lib.SimplifySettings(s["max_iterations"], s["interpolate"], s["n_operations"], ops, s["bspline_max_steps"],
                               s["bspline_min_change"], s["bspline_midpoint_interpolation"], s["max_waypoints"],
                               s["questions_per_round"], s["check_every"])
    out = ctypes.c_void_p(SENTINEL)
    off = np.ascontiguousarray(offsets, np.uintp)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "points": pts.ctypes.data_as(_lib.c_float_p),
           "offsets": off.ctypes.data_as(_lib.c_size_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_simplify_multi(robot, ptr["envs"], n, ptr["points"], ptr["offsets"], ptr["settings"], ptr["out"])
    return rc, out.value


def test_unknown_robot(raw):
    _lib, handles = raw
    for robot in (-1, 4, 7):
        assert _call(_lib, handles, robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)


@pytest.mark.parametrize("drop", ["envs", "points", "offsets", "settings", "out"])
def test_null_pointers(raw, drop):
    _lib, handles = raw
    assert _call(_lib, handles, drop=(drop,)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_null_handle(raw):
    _lib, handles = raw
    assert _call(_lib, [handles[0], None]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("offsets", [(0, 5, 4), (1, 4, 7), (3, 2, 7)])
def test_offsets_must_start_at_zero_and_not_decrease(raw, offsets):
    _lib, handles = raw
    assert _call(_lib, handles, offsets=offsets) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("w", [1, 3, 6, 12, 24, 48, 65, 128, 2 ** 31])
def test_questions_per_round_must_be_in_the_set(raw, w):
    _lib, handles = raw
    assert _call(_lib, handles, questions_per_round=w) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("w", [0, 2, 4, 8, 16, 32, 64])
def test_questions_per_round_in_the_set_reaches_the_next_check(raw, w):
    _lib, handles = raw
    assert _call(_lib, handles, questions_per_round=w) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_max_waypoints_below_the_longest_path(raw):
    _lib, handles = raw
    assert _call(_lib, handles, max_waypoints=3) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, max_waypoints=4) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, handles, max_waypoints=(1 << 24) + 1) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_path_count_limit(raw):
    _lib, handles = raw
    assert _call(_lib, handles, n=1 << 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # (no array is read)
    assert _call(_lib, handles, n=1 << 27, questions_per_round=16) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, n=1 << 25, questions_per_round=64) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("kw", [dict(operations=(OP_REDUCE,)), dict(operations=(OP_SHORTCUT, OP_PERTURB)),
                                dict(operations=(OP_SHORTCUT, 4)), dict(interpolate=64), dict(n_operations=9)])
def test_out_of_scope_settings(raw, kw):
    _lib, handles = raw
    assert _call(_lib, handles, **kw) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_operation_lists_that_are_allowed(raw):
    _lib, handles = raw
    for ops in ((), (OP_BSPLINE,), (OP_BSPLINE, OP_SHORTCUT), (OP_SHORTCUT,) * 8, (OP_BSPLINE, OP_BSPLINE, OP_SHORTCUT)):
        assert _call(_lib, handles, operations=ops) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_unfinalized_environment_is_reported_without_a_device(raw):
    _lib, handles = raw
    assert _call(_lib, handles) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, [handles[0], handles[0]]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed


def test_no_paths_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, paths = _call(_lib, [], n=0)
    assert rc == VMV_OK and paths not in (None, SENTINEL)
    rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_paths_summary(paths, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
    assert (rounds.value, questions.value) == (0, 0)
    assert L.vmv_paths_points(paths, None, 0) == VMV_OK
    assert L.vmv_paths_destroy(paths) == VMV_OK
    assert L.vmv_paths_summary(None, None, None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_paths_points(None, None, 0) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_paths_destroy(None) == VMV_ERR_INVALID_ARGUMENT
    assert planning.simplify_multi(vamp.panda, [], []) == []
    assert vamp.panda.simplify_multi([], []) == []


def test_well_formed_call_fails_loudly_without_gpu(vamp, cage_paths):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.simplify_multi(vamp.panda, [cage_paths[0]], [None])
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
    S = planning.SimplifyMultiSettings

    def f(*args, **kw):
        return planning.simplify_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f([a, a, a], [env, None])  # two environments for three paths
    with pytest.raises(TypeError):
        f([np.zeros((4, 6), np.float32)], [env])  # wrong dimension
    with pytest.raises(TypeError):
        f([a[0]], [env])  # one waypoint still is a [1][dim] array
    with pytest.raises(TypeError):
        f([a, a], [env, "not an environment"])
    for routine in ("REDUCE", "PERTURB", vamp.SimplifyRoutine.REDUCE, vamp.SimplifyRoutine.PERTURB):
        with pytest.raises(NotImplementedError):
            f([a], [env], S(operations=["SHORTCUT", routine]))
    with pytest.raises(ValueError):
        f([a], [env], S(operations=["SMOOTH"]))
    with pytest.raises(ValueError):
        f([a], [env], S(operations=["SHORTCUT"] * 9))
    with pytest.raises(NotImplementedError):
        f([a], [env], S(interpolate=64))
    with pytest.raises(NotImplementedError):
        f([a], [env], vamp.SimplifySettings(interpolate=64))  # the reference-shaped settings are converted, then checked
    with pytest.raises(NotImplementedError):
        f([a], [env], vamp.SimplifySettings(operations=[vamp.SimplifyRoutine.SHORTCUT, vamp.SimplifyRoutine.REDUCE]))
    for w in (1, 3, 12, 128, -2):
        with pytest.raises(ValueError):
            f([a], [env], S(questions_per_round=w))
    with pytest.raises(ValueError):
        f([a], [env], S(max_waypoints=3))
    with pytest.raises(ValueError):
        f([a], [env], S(max_iterations=-1))
    with pytest.raises(ValueError):
        f([a], [env], S(check_every=2 ** 32))
    with pytest.raises(ValueError):
        vamp.panda.simplify_multi([a, a, a], [env, None], S())  # the installed name takes the same road
    assert env._handle is None  # nothing was built or finalized
