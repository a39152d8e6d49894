"""vmv_rrtc_multi / planning.rrtc_multi: what holds without a device — the serial comparator's own figures (the contract of
DESIGN §5c restated in tests/rrtc_serial.py, with the CPU oracle answering every question), the ABI surface, the checks
that come before any device query, and the Python wrapper's argument checks."""
import ctypes

import numpy as np
import pytest

from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE
from rrtc_serial import MAX_ITERATIONS, SOLVED, rrtc_serial

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
NAMES = ("vmv_rrtc_multi", "vmv_plans_summary", "vmv_plans_paths", "vmv_plans_destroy")
SENTINEL = 0x5A5A5A5A

# range, skip, max_iterations -> status, iterations, size, questions (None = not recorded)
CAGE_FIGURES = [
    (1.0, 0, 100000, SOLVED, 605, [37, 22], 662),
    (1.0, 1000, 100000, SOLVED, 663, [44, 24], None),
    (1.0, 2000, 100000, SOLVED, 219, [18, 13], None),
    (1.0, 3000, 100000, SOLVED, 338, [27, 17], None),
    (1.0, 4000, 100000, SOLVED, 398, [23, 43], None),
    (1.0, 5000, 100000, SOLVED, 208, [15, 23], None),
    (0.25, 0, 100000, SOLVED, 1442, [283, 155], 1878),
    (0.25, 1000, 100000, SOLVED, 3274, [640, 331], None),
    (1.0, 0, 100, MAX_ITERATIONS, 100, [4, 8], None),
]


@pytest.fixture(scope="module")
def cage(oracle):
    env = oracle.env()
    for c in SPHERE_CAGE:
        env.add_sphere(*c, 0.2)
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return rid, env, lower, span


@pytest.mark.parametrize("range_, skip, max_iterations, status, iterations, size, questions", CAGE_FIGURES)
def test_comparator_figures_on_the_sphere_cage(oracle, cage, range_, skip, max_iterations, status, iterations, size, questions):
    rid, env, lower, span = cage
    asked = []

    def question(a, b):
        asked.append((a.copy(), b.copy()))
        return oracle.validate_motion(rid, env, a, b)

    r = rrtc_serial(CAGE_START, CAGE_GOAL, lower, span, question, range_=range_, balance=True, tree_ratio=1.0,
                    max_iterations=max_iterations, max_samples=8192, skip=skip)
    assert (r.status, r.iterations, r.size) == (status, iterations, size)
    assert r.questions == len(asked) and (questions is None or r.questions == questions)
    if status == SOLVED:
        assert r.path[0].tobytes() == np.array(CAGE_START, np.float32).tobytes()
        assert r.path[-1].tobytes() == np.array(CAGE_GOAL, np.float32).tobytes()
        assert all(oracle.validate_motion(rid, env, a, b) for a, b in zip(r.path[:-1], r.path[1:]))
    else:
        assert r.path == []


def test_comparator_stops_at_the_node_pool_bound(oracle, cage):
    rid, env, lower, span = cage
    r = rrtc_serial(CAGE_START, CAGE_GOAL, lower, span, lambda a, b: oracle.validate_motion(rid, env, a, b), range_=1.0,
                    max_samples=30)
    assert not r.solved and sum(r.size) == 30 and r.iterations < 605


def test_comparator_does_not_import_the_package_planner():
    import os
    import rrtc_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text  # neither the planner nor the library


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
    assert vamp.abi_version() == 1  # the change is additive


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


def _call(_lib, handles, robot=0, n=None, drop=(), skips=None, **settings):
    """one vmv_rrtc_multi call with two problems; `drop` names the pointers passed as NULL -> (status, *out)"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((max(len(handles), 1), 7), 0.5, np.float32)
    s = dict(range=1.0, balance=1, tree_ratio=1.0, max_iterations=1000, max_samples=64, check_every=0)
    s.update(settings)
    cs = _lib.RrtcSettings(s["range"], s["balance"], s["tree_ratio"], s["max_iterations"], s["max_samples"], s["check_every"])
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_rrtc_multi(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
                                 None if sk is None else sk.ctypes.data_as(_lib.c_u64_p), ptr["settings"], ptr["out"])
    return rc, out.value


def test_unknown_robot(raw):
    _lib, handles = raw
    for robot in (-1, 4, 7):
        assert _call(_lib, handles, robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)


@pytest.mark.parametrize("drop", ["envs", "starts", "goals", "settings", "out"])
def test_null_pointers(raw, drop):
    _lib, handles = raw
    assert _call(_lib, handles, drop=(drop,)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_null_handle(raw):
    _lib, handles = raw
    assert _call(_lib, [handles[0], None]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("settings", [dict(range=0.0), dict(range=-1.0), dict(range=float("inf")), dict(range=float("nan")),
                                      dict(max_samples=1), dict(max_samples=0)])
def test_bad_settings(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_halton_validity_limit(raw):
    """skip + max_iterations may not pass 1,000,000, with and without a skips array; at the limit the next check speaks"""
    _lib, handles = raw
    assert _call(_lib, handles, max_iterations=1000001) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999001], max_iterations=1000) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 2 ** 63], max_iterations=1000) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999000], max_iterations=1000) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, handles, max_iterations=1000000) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_problem_count_limit(raw):
    _lib, handles = raw
    assert _call(_lib, handles, n=1 << 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # (no array is read)


def test_unfinalized_environment_is_reported_without_a_device(raw):
    _lib, handles = raw
    assert _call(_lib, handles) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, [handles[0], handles[0]]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed


def test_no_problems_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib

    L = _lib.lib
    rc, plans = _call(_lib, [], n=0)
    assert rc == VMV_OK and plans not in (None, SENTINEL)
    rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_plans_summary(plans, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
    assert (rounds.value, questions.value) == (0, 0)
    assert L.vmv_plans_paths(plans, None, 0) == VMV_OK
    assert L.vmv_plans_destroy(plans) == VMV_OK
    assert L.vmv_plans_summary(None, None, None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_paths(None, None, 0) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_destroy(None) == VMV_ERR_INVALID_ARGUMENT
    from vamp_mvt_amd import planning

    assert planning.rrtc_multi(vamp.panda, np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), []) == []


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.rrtc_multi(vamp.panda, [CAGE_START], [CAGE_GOAL], [None])
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a = np.zeros((3, 7), np.float32)
    b = np.ones((3, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.RRTCMultiSettings
    assert S().max_samples == 8192

    def f(*args, **kw):
        return planning.rrtc_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f(a, b, [env, None])  # two environments for three problems
    with pytest.raises(TypeError):
        f(a, b[:2], [env] * 3)  # starts and goals of different shapes
    with pytest.raises(TypeError):
        f(np.zeros((3, 6), np.float32), np.zeros((3, 6), np.float32), [env] * 3)  # wrong dimension
    with pytest.raises(TypeError):
        f(a[0], b[0], [env])  # one problem still is a [1][dim] array
    with pytest.raises(TypeError):
        f(a, b, [env, "not an environment", None])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1, -1])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, S(range=0.0))
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, S(range=float("nan")))
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, S(max_samples=1))
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, S(max_iterations=-1))
    with pytest.raises(ValueError):
        vamp.panda.rrtc_multi(a, b, [env, None], S())  # the installed name takes the same road
    assert env._handle is None  # nothing was built or finalized
