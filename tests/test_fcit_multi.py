"""vmv_fcit_multi / planning.fcit_multi: what holds without a device — the ABI surface, the checks that come before any
device query, the accessor's refusal, the Python wrapper's argument checks, and the serial statement's own properties
(the contract of DESIGN §5g restated in tests/fcit_serial.py) on the sphere cage and three scenes of tests/envs.py.

Two groups.  The tests down to test_python_checks_its_arguments_before_any_library_call pin the LIBRARY and the package:
they fail where vmv_fcit_multi does not exist.  The tests below "the serial statement's own properties" pin the
STATEMENT alone, the yardstick the device tests compare against: they never touch the library."""
import ctypes

import numpy as np
import pytest

import envs
import fcit_serial as fs
import prm_serial as ps
from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
NAMES = ("vmv_fcit_multi", "vmv_plans_fcit_summary")
SENTINEL = 0x5A5A5A5A
f32 = np.float32


def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None  # the _lib.py table has the entry
    assert vamp.abi_version() == 1  # the change is additive
    s = planning.FCITMultiSettings()
    assert (s.n_samples, s.max_iterations, s.questions_per_round, s.check_every) == (1024, 100000, 1, 0)
    assert ctypes.sizeof(_lib.FcitSettings) == 16
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.fcit_multi) and callable(robot.fcit_multi_raw) and callable(robot.fcit)


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


def _call(_lib, handles, robot=0, n=None, drop=(), skips=None, samples=False, **settings):
    """one vmv_fcit_multi call with two problems; `drop` names the pointers passed as NULL -> (status, *out)"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((max(len(handles), 1), 7), 0.5, np.float32)
    s = dict(n_samples=64, max_iterations=100, questions_per_round=8, check_every=0)
    s.update(settings)
    cs = _lib.FcitSettings(s["n_samples"], s["max_iterations"], s["questions_per_round"], s["check_every"])
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    sm = np.zeros((max(len(handles), 1), min(s["n_samples"], 2048), 7), np.float32) if samples else None
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_fcit_multi(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
                                 None if sk is None else sk.ctypes.data_as(_lib.c_u64_p),
                                 None if sm is None else sm.ctypes.data_as(_lib.c_float_p), ptr["settings"], ptr["out"])
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


@pytest.mark.parametrize("settings", [dict(n_samples=0), dict(n_samples=63), dict(n_samples=65), dict(n_samples=100),
                                      dict(n_samples=2112), dict(n_samples=8128), dict(n_samples=1 << 20),
                                      dict(questions_per_round=0), dict(questions_per_round=33),
                                      dict(questions_per_round=1 << 31), dict(max_iterations=0)])
def test_bad_settings(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("settings", [dict(n_samples=64, questions_per_round=1), dict(n_samples=2048, questions_per_round=32),
                                      dict(max_iterations=1), dict(max_iterations=2 ** 32 - 1), dict(check_every=1),
                                      dict(check_every=2 ** 32 - 1)])
def test_settings_at_their_limits_pass_to_the_next_check(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_halton_validity_limit(raw):
    """skip + n_samples may not pass 1,000,000 where the samples are the Halton sequence's; the caller's own have no skip"""
    _lib, handles = raw
    assert _call(_lib, handles, skips=[0, 999937]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 2 ** 63]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[2 ** 64 - 32, 0]) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999936]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, handles, skips=[0, 2 ** 63], samples=True) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_pair_state_and_question_limits(raw):
    """n_problems * V * ceil(V / 32) (the words of one pair-state matrix) and n_problems * questions_per_round stay below
    2^31 (no array is read)"""
    _lib, handles = raw
    assert _call(_lib, handles, n=1 << 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    h = [handles[0]] * 16117  # 2,050 * 65 = 133,250 words per problem; 16,117 * 133,250 = 2^31 + 106,602
    assert _call(_lib, h, n_samples=2048) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, h[:16116], n_samples=2048) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # 2^31 - 26,648
    # (a problem has at least 66 * 3 words of pair state and at most 32 questions per round, so the first bound refuses a
    # call before the second can: the second is stated for the day the first is loosened)


def test_unfinalized_environment_is_reported_without_a_device(raw):
    _lib, handles = raw
    assert _call(_lib, handles) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, [handles[0], handles[0]]) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed


def test_no_problems_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, plans = _call(_lib, [], n=0)
    assert rc == VMV_OK and plans not in (None, SENTINEL)
    rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_plans_summary(plans, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
    assert (rounds.value, questions.value) == (0, 0)
    assert L.vmv_plans_paths(plans, None, 0) == VMV_OK
    assert L.vmv_plans_fcit_summary(plans, None, None) == VMV_OK
    assert L.vmv_plans_roadmap_summary(plans, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT  # not a PRM result
    assert L.vmv_plans_costs(plans, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT            # nor an AORRTC result
    assert L.vmv_plans_destroy(plans) == VMV_OK
    assert L.vmv_plans_fcit_summary(None, None, None) == VMV_ERR_INVALID_ARGUMENT
    empty = np.zeros((0, 7), np.float32)
    assert planning.fcit_multi(vamp.panda, empty, empty, []) == []
    assert vamp.panda.fcit_multi(empty, empty, [], vamp.FCITSettings(vamp.FCITNeighborParams(7, 1.0))) == []


def test_accessor_refuses_plans_of_another_origin(vamp):
    """an rrtc_multi or a prm_multi result has no pair state: the accessor says so and writes nothing"""
    from vamp_mvt_amd import _lib

    L = _lib.lib
    rrtc, prm = ctypes.c_void_p(), ctypes.c_void_p()
    cs = _lib.RrtcSettings(1.0, 1, 1.0, 10, 64, 0)
    assert L.vmv_rrtc_multi(0, None, 0, None, None, None, ctypes.byref(cs), ctypes.byref(rrtc)) == VMV_OK
    cp = _lib.PrmSettings(64, 4, float("inf"), 0)
    assert L.vmv_prm_multi(0, None, 0, None, None, None, None, ctypes.byref(cp), ctypes.byref(prm)) == VMV_OK
    for plans in (rrtc, prm):
        costs, counts = np.full(4, 7, np.float32), np.full(4, 7, np.uint32)
        assert L.vmv_plans_fcit_summary(plans, costs.ctypes.data_as(_lib.c_float_p),
                                        counts.ctypes.data_as(_lib.c_u32_p)) == VMV_ERR_INVALID_ARGUMENT
        assert (costs == 7).all() and (counts == 7).all()
        assert L.vmv_plans_destroy(plans) == VMV_OK


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.fcit_multi(vamp.panda, [CAGE_START], [CAGE_GOAL], [None], planning.FCITMultiSettings(n_samples=64))
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
    S = planning.FCITMultiSettings

    def f(*args, **kw):
        return planning.fcit_multi(vamp.panda, *args, **kw)

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
    for bad in (S(n_samples=100), S(n_samples=0), S(n_samples=2112), S(questions_per_round=0), S(questions_per_round=33),
                S(max_iterations=0), S(max_iterations=2 ** 32), S(check_every=-1)):
        with pytest.raises(ValueError):
            f(a, b, [env] * 3, bad)
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1, -1])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, S(n_samples=64), skips=[0, 1, 999937])
    with pytest.raises(TypeError):
        f(a, b, [env] * 3, S(n_samples=64), samples=np.zeros((63, 7), np.float32))
    with pytest.raises(TypeError):
        f(a, b, [env] * 3, S(n_samples=64), samples=np.zeros((2, 64, 7), np.float32))
    with pytest.raises(TypeError):
        f(a, b, [env] * 3, S(n_samples=64), samples=np.zeros((64, 6), np.float32))
    with pytest.raises(ValueError):
        vamp.panda.fcit_multi(a, b, [env, None], vamp.FCITSettings(vamp.FCITNeighborParams(7, 1.0)))  # the installed name too
    assert env._handle is None  # nothing was built or finalized


# ---- the serial statement's own properties ---------------------------------------------------------------------------
class Scene:
    def __init__(self, oracle, kind):
        self.o, self.rid = oracle, oracle.robot("panda")
        self.lower, self.span = oracle.bounds(self.rid)
        self.env = envs.build_oracle_env(oracle, envs.spec_for(kind, "panda"))

    def valid(self, q):
        return self.o.validate(self.rid, self.env, q)

    def question(self, a, b):
        return self.o.validate_motion(self.rid, self.env, a, b)

    def samples(self, n, skip=0):
        return fs.halton_samples(skip, n, self.lower, self.span)


@pytest.fixture(scope="module")
def cage(oracle):
    return Scene(oracle, "cage")


def path_cost(path):
    """the left-to-right fp32 sum of the segment lengths"""
    total = f32(0)
    for a, b in zip(path[:-1], path[1:]):
        total = f32(total + np.sqrt(ps.dist2(np.stack([a, b]), 0)[1]))
    return total


# n_samples -> status, valid vertices, searches, questions, cost, waypoints (skip 0).  The solved case's cost was recorded
# as 10.90768, five decimals of a print; the statement's value is the fp32 number 10.9076805, one ulp above f32(10.90768),
# and it is the left-to-right fp32 sum along the path (asserted below), so the bits are pinned and the print is checked.
CAGE_FIGURES = [
    (64, fs.NO_PATH, 14, 51, 54, np.inf, 0),
    (128, fs.NO_PATH, 22, 145, 154, np.inf, 0),
    (1024, fs.SOLVED, 179, 586, 656, 10.9076805, 4),
]


@pytest.fixture(scope="module")
def cage_results(cage):
    """fcit_serial and prm_serial (k = 8) on the three cage problems, computed once"""
    out = {}
    for n, *_ in CAGE_FIGURES:
        samples = cage.samples(n)
        out[n] = (fs.fcit_serial(CAGE_START, CAGE_GOAL, samples, cage.valid, cage.question),
                  ps.prm_serial(CAGE_START, CAGE_GOAL, samples, cage.valid, cage.question, k=8))
    return out


@pytest.mark.parametrize("n_samples, status, vertices, searches, questions, cost, waypoints", CAGE_FIGURES)
def test_serial_figures_on_the_sphere_cage(cage, cage_results, n_samples, status, vertices, searches, questions, cost, waypoints):
    r = cage_results[n_samples][0]
    assert (r.status, r.size[0], r.iterations, r.questions, r.cost, len(r.path)) == \
        (status, vertices, searches, questions, f32(cost), waypoints)
    assert r.questions == r.known_valid + r.size[1]  # every question ends as a remembered edge or a blocked one
    if status == fs.NO_PATH:
        assert r.iterations == r.size[1] + 1  # every search but the last blocked one edge
    else:
        assert r.path[0].tobytes() == np.array(CAGE_START, f32).tobytes()
        assert r.path[-1].tobytes() == np.array(CAGE_GOAL, f32).tobytes()
        assert all(cage.question(a, b) for a, b in zip(r.path[:-1], r.path[1:]))
        assert path_cost(r.path) == r.cost and "%.5f" % r.cost == "10.90768"


def test_serial_endpoints(cage):
    samples = cage.samples(64)
    inside = np.array(CAGE_START, f32)
    inside[1] = 0.9  # the arm leans into the cage's spheres
    assert not cage.valid(inside)
    for start in (inside, np.array([np.nan] + CAGE_START[1:], f32)):
        r = fs.fcit_serial(start, CAGE_GOAL, samples, cage.valid, cage.question)
        assert (r.status, r.path, r.questions, r.iterations, r.size) == (fs.INVALID_ENDPOINT, [], 0, 0, [14 - 1, 0])
        assert np.isinf(r.cost)
    near = (np.array(CAGE_START, f32) + f32(0.01)).astype(f32)
    r = fs.fcit_serial(CAGE_START, near, samples, cage.valid, cage.question)
    assert (r.status, len(r.path), r.iterations, r.questions, r.size[1]) == (fs.SOLVED, 2, 1, 1, 0)
    assert r.cost == np.sqrt(ps.dist2(np.stack([np.array(CAGE_START, f32), near]), 0)[1])


def test_serial_max_iterations(cage):
    samples = cage.samples(64)
    r = fs.fcit_serial(CAGE_START, CAGE_GOAL, samples, cage.valid, cage.question, max_iterations=5)
    assert (r.status, r.iterations, r.path, r.size[1]) == (fs.MAX_ITERATIONS, 5, [], 5) and np.isinf(r.cost)
    r = fs.fcit_serial(CAGE_START, CAGE_GOAL, samples, cage.valid, cage.question, max_iterations=1)
    assert (r.status, r.iterations, r.questions) == (fs.MAX_ITERATIONS, 1, 1)  # the straight edge, asked and blocked


def check_inclusion(fcit, prm):
    """what prm_serial solves, fcit_serial solves, at no higher cost but a handful of fp32 roundings per hop"""
    if prm.solved:
        assert fcit.solved
        assert float(fcit.cost) <= float(prm.cost) * (1 + 1e-4)


@pytest.mark.parametrize("n_samples", [64, 128, 1024])
def test_inclusion_on_the_cage(cage_results, n_samples):
    fcit, prm = cage_results[n_samples]
    check_inclusion(fcit, prm)
    if n_samples == 1024:
        assert prm.solved and fcit.cost < prm.cost and fcit.questions < prm.questions  # 10.9077 in 656 against 12.6186 in 933


@pytest.mark.parametrize("kind", ["mixed", "shell64", "many"])
def test_inclusion_on_other_scenes(oracle, kind):
    scene = Scene(oracle, kind)
    rng = np.random.default_rng(5)
    q = (scene.lower + scene.span * rng.random((256, 7), dtype=np.float32)).astype(np.float32)
    q = q[oracle.validate_batch(scene.rid, scene.env, q)]
    solved = 0
    for k in range(4):
        samples = scene.samples(64, 100 * k)
        fcit = fs.fcit_serial(q[2 * k], q[2 * k + 1], samples, scene.valid, scene.question)
        prm = ps.prm_serial(q[2 * k], q[2 * k + 1], samples, scene.valid, scene.question, k=8)
        check_inclusion(fcit, prm)
        solved += prm.solved
        if fcit.solved:
            assert path_cost(fcit.path) == fcit.cost
            assert all(scene.question(a, b) for a, b in zip(fcit.path[:-1], fcit.path[1:]))
    assert solved >= 1  # the property was exercised


def test_serial_statement_does_not_import_the_package_planner():
    import os

    with open(os.path.abspath(fs.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text  # neither the planner nor the library
