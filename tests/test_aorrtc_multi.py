"""vmv_aorrtc_multi / planning.aorrtc_multi: what holds without a device — the ABI surface, the checks that come before any
device query, the settings mapping, the Python wrapper's argument checks, and the serial statement's own properties (the
contract of DESIGN §5f restated in tests/aorrtc_serial.py, with the CPU oracle answering every question)."""
import ctypes

import numpy as np
import pytest

from aorrtc_serial import PHS, Uniform, aorrtc_serial, ln32
from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE
from rrtc_serial import rrtc_serial
from simplify_serial import cost, simplify_serial

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
NAMES = ("vmv_aorrtc_multi", "vmv_plans_costs", "vmv_phs_samples")
SENTINEL = 0x5A5A5A5A


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


def _settings(_lib, **kw):
    s = dict(range=1.0, balance=1, tree_ratio=1.0, check_every=0, optimize=1, cost_bound_resample=1, simplify_intermediate=1,
             max_iterations=1000, max_internal_iterations=100, max_samples=64, max_cost_bound_resamples=4, max_searches=0,
             simplify_iterations=4, interpolate=0, operations=(2, 0), max_waypoints=0, questions_per_round=0)
    s.update(kw)
    ops = tuple(s["operations"])
    simp = _lib.SimplifySettings(s["simplify_iterations"], s["interpolate"], s.get("n_operations", len(ops)),
                                 (ctypes.c_uint32 * 8)(*ops[:8]), 5, 0.05, 0.5, s["max_waypoints"], s["questions_per_round"], 0)
    rrtc = _lib.RrtcSettings(s["range"], s["balance"], s["tree_ratio"], 7, 7, s["check_every"])  # its maxima are not read
    return _lib.AorrtcSettings(rrtc, simp, s["optimize"], s["cost_bound_resample"], s["simplify_intermediate"],
                               s["max_iterations"], s["max_internal_iterations"], s["max_samples"],
                               s["max_cost_bound_resamples"], s["max_searches"])


def _call(_lib, handles, robot=0, n=None, drop=(), skips=None, **settings):
    """one vmv_aorrtc_multi call with two problems; `drop` names the pointers passed as NULL -> (status, *out)"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((max(len(handles), 1), 7), 0.5, np.float32)
    cs = _settings(_lib, **settings)
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_aorrtc_multi(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
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


@pytest.mark.parametrize("settings", [
    dict(range=0.0), dict(range=-1.0), dict(range=float("inf")), dict(range=float("nan")), dict(max_samples=1),
    dict(max_samples=0), dict(max_internal_iterations=0), dict(max_cost_bound_resamples=65),
    dict(questions_per_round=3), dict(interpolate=1), dict(operations=(2, 1)), dict(operations=(3,)), dict(n_operations=9),
    dict(max_waypoints=(1 << 24) + 1)])
def test_bad_settings(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_accepted_settings_reach_the_environment_check(raw):
    _lib, handles = raw
    for settings in (dict(max_cost_bound_resamples=64), dict(max_cost_bound_resamples=0), dict(max_searches=3),
                     dict(optimize=0), dict(questions_per_round=64), dict(operations=())):
        assert _call(_lib, handles, **settings) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_halton_validity_limit(raw):
    """skip + max_iterations (the AORRTC settings', not rrtc's own) may not pass 1,000,000"""
    _lib, handles = raw
    assert _call(_lib, handles, max_iterations=1000001) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999001], max_iterations=1000) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999000], max_iterations=1000) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_problem_count_limit(raw):
    _lib, handles = raw
    assert _call(_lib, handles, n=1 << 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # (no array is read)
    assert _call(_lib, handles, n=1 << 25) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


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
    assert L.vmv_plans_costs(plans, None, None, None, None) == VMV_OK
    assert L.vmv_plans_paths(plans, None, 0) == VMV_OK
    assert L.vmv_plans_destroy(plans) == VMV_OK
    assert L.vmv_plans_costs(None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    # the plans of vmv_rrtc_multi carry no costs
    cs = _lib.RrtcSettings(1.0, 1, 1.0, 10, 64, 0)
    other = ctypes.c_void_p()
    assert L.vmv_rrtc_multi(0, None, 0, None, None, None, ctypes.byref(cs), ctypes.byref(other)) == VMV_OK
    assert L.vmv_plans_costs(other, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_destroy(other) == VMV_OK
    assert planning.aorrtc_multi(vamp.panda, np.zeros((0, 7), np.float32), np.zeros((0, 7), np.float32), []) == []


def test_sampler_entry_point_checks_its_arguments(vamp):
    from vamp_mvt_amd import _lib

    a, b = np.zeros(7, np.float32), np.ones(7, np.float32)
    c = ctypes.c_uint32(SENTINEL)
    fp = lambda x: x.ctypes.data_as(_lib.c_float_p)
    f = _lib.lib.vmv_phs_samples
    assert f(9, fp(a), fp(b), 3.0, 0, 0, 0, None, None, ctypes.byref(c)) == VMV_ERR_UNKNOWN_ROBOT
    assert f(0, None, fp(b), 3.0, 0, 0, 0, None, None, ctypes.byref(c)) == VMV_ERR_INVALID_ARGUMENT
    assert f(0, fp(a), fp(b), 3.0, 0, 0, 0, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert f(0, fp(a), fp(b), 3.0, 0, 0, 4, None, None, ctypes.byref(c)) == VMV_ERR_INVALID_ARGUMENT
    assert c.value == SENTINEL


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.aorrtc_multi(vamp.panda, [CAGE_START], [CAGE_GOAL], [None])
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback


# ------------------------------------------------------------------------------------------------------- Python layer
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a, b = np.zeros((3, 7), np.float32), np.ones((3, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.AORRTCMultiSettings
    assert S().max_samples == 8192 and S().max_cost_bound_resamples == 64

    def f(*args, **kw):
        return planning.aorrtc_multi(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f(a, b, [env, None])  # two environments for three problems
    with pytest.raises(TypeError):
        f(a, b[:2], [env] * 3)
    with pytest.raises(TypeError):
        f(a[0], b[0], [env])
    with pytest.raises(TypeError):
        f(a, b, [env, "not an environment", None])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, skips=[0, 1, -1])
    for bad in (dict(range=0.0), dict(range=float("nan")), dict(max_samples=1), dict(max_iterations=-1),
                dict(max_internal_iterations=0), dict(max_cost_bound_resamples=65), dict(max_searches=-1),
                dict(simplify=planning.SimplifyMultiSettings(questions_per_round=3))):
        with pytest.raises(ValueError):
            f(a, b, [env] * 3, S(**bad))
    with pytest.raises(NotImplementedError):
        f(a, b, [env] * 3, S(simplify=planning.SimplifyMultiSettings(operations=["REDUCE"])))
    assert env._handle is None  # nothing was built or finalized


def test_settings_mapping(vamp, monkeypatch):
    """the reference-shaped AORRTCSettings reach planning.aorrtc_multi field by field; what is not built raises at the call"""
    from vamp_mvt_amd import planning

    s = vamp.AORRTCSettings()
    assert (s.optimize, s.cost_bound_resample, s.simplify_intermediate, s.use_phs, s.anytime) == (True, True, True, True, False)
    assert (s.max_iterations, s.max_internal_iterations, s.max_samples, s.max_cost_bound_resamples) == (100000,) * 3 + (1000,)
    assert isinstance(s.rrtc, vamp.RRTCSettings) and isinstance(s.simplify, vamp.SimplifySettings)
    seen = []
    monkeypatch.setattr(planning, "aorrtc_multi", lambda robot, a, b, envs, settings, skips=None: seen.append((settings, skips)) or [])
    s.rrtc.range, s.rrtc.balance, s.rrtc.tree_ratio = 0.75, False, 2.0
    s.optimize, s.cost_bound_resample, s.simplify_intermediate = False, False, False
    s.max_iterations, s.max_internal_iterations, s.max_samples, s.max_cost_bound_resamples = 5000, 700, 4096, 9
    s.simplify.max_iterations = 2
    a, b = np.zeros((2, 7), np.float32), np.ones((2, 7), np.float32)
    assert vamp.panda.aorrtc_multi(a, b, [None, None], s, skips=[5, 6]) == []
    m, skips = seen[0]
    assert isinstance(m, planning.AORRTCMultiSettings) and skips == [5, 6]
    assert (m.range, m.balance, m.tree_ratio, m.optimize, m.cost_bound_resample, m.simplify_intermediate) == \
        (0.75, False, 2.0, False, False, False)
    assert (m.max_iterations, m.max_internal_iterations, m.max_samples, m.max_cost_bound_resamples, m.max_searches) == \
        (5000, 700, 4096, 9, 0)
    assert m.simplify is s.simplify and planning._as_simplify_multi_settings(m.simplify).max_iterations == 2
    s.max_cost_bound_resamples = 1000
    vamp.panda.aorrtc_multi(a, b, [None, None], s)
    assert seen[1][0].max_cost_bound_resamples == 64  # the library's limit
    own = planning.AORRTCMultiSettings(max_searches=3)
    vamp.panda.aorrtc_multi(a, b, [None, None], own)
    assert seen[2][0] is own
    for change in (dict(anytime=True), dict(use_phs=False)):
        bad = vamp.AORRTCSettings(**change)
        with pytest.raises(NotImplementedError):
            vamp.panda.aorrtc(a[0], b[0], None, bad)
    bad = vamp.AORRTCSettings()
    bad.rrtc.dynamic_domain = True
    with pytest.raises(NotImplementedError):
        vamp.panda.aorrtc(a[0], b[0], None, bad)
    assert len(seen) == 3
    module, planner, settings, simp = vamp.configure_robot_and_planner_with_kwargs("panda", "aorrtc", optimize=False)
    assert planner is vamp.panda.aorrtc and isinstance(settings, vamp.AORRTCSettings)
    assert settings.rrtc.range == 1.0 and settings.optimize is False


# ------------------------------------------------------------------------------------------------- the serial statement
def test_serial_statement_does_not_import_the_package_planner():
    import os
    import aorrtc_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text


def _ln32_errors(s):
    """-> (|ln32(x) - log(x)|, half an ulp of the fp32 result) per value, the logarithm in float64"""
    true = np.log(s.astype(np.float64))
    got = np.array([ln32(x) for x in s], np.float32)
    half_ulp = np.maximum(np.spacing(np.abs(got)), np.spacing(np.abs(true).astype(np.float32))).astype(np.float64) / 2
    return np.abs(got.astype(np.float64) - true), half_ulp


def test_ln32_against_log():
    """|ln32(s) - log(s)| <= 2e-7 on 10,000 values: 8,000 uniform over exp(-4) < s < 1, the 1,000 fp32 numbers just below 1
    and 1,000 at that domain's lower end.  The domain follows from the format alone: the bound is absolute, and half an ulp
    of an fp32 result is 1.19e-7 for 2 <= |ln s| < 4 but 2.38e-7 from |ln s| = 4 on, so below exp(-4) = 0.0183 not even the
    correctly rounded logarithm stays within 2e-7.  What the computation may add: t carries two roundings and (2 t) p two
    more, at most 2.4e-7 relative on |ln m| <= ln(2) / 2 = 0.347, so 8.1e-8; the inner sum half an ulp of 0.35, 1.5e-8;
    the series' remainder 2e-11: together below 1e-7, whatever the exponent (its product with ln 2's head is exact).

    Nearer 0 the same statement is asserted in the only form fp32 admits, error <= half an ulp of the result + 1e-7: on the
    1,000 smallest values the polar method's s = u1 u1 + u2 u2 can take (the multiples of 2^-46), and on every exponent from
    -46 to -1 at the mantissas around the reduction's branch (1, just below, at and just above fl(sqrt 2), just below 2),
    so that a wrong exponent term or a wrong e + 1 branch for small s shows."""
    rng = np.random.default_rng(0)
    lo = np.float32(np.exp(-4.0)) + np.float32(2.0 ** -29)  # the first fp32 numbers above exp(-4)
    s = np.concatenate([(lo + (np.float32(1) - lo) * rng.random(8000, dtype=np.float32)).astype(np.float32),
                        np.float32(1) - np.arange(1, 1001, dtype=np.float32) * np.float32(2.0 ** -24),
                        lo + np.arange(1000, dtype=np.float32) * np.float32(2.0 ** -29)]).astype(np.float32)
    assert len(s) == 10000 and bool(((s > np.exp(-4.0)) & (s < 1)).all())
    err, half_ulp = _ln32_errors(s)
    print("ln32 on (exp(-4), 1): max error", err.max(), "at the lower end", err[9000:].max(), "just below 1", err[8000:9000].max())
    assert err.max() <= 2e-7
    assert bool((err <= half_ulp + 1e-7).all())

    tiny = (np.arange(1, 1001, dtype=np.float32) * np.float32(2.0 ** -46)).astype(np.float32)
    mantissas = (0x000000, 0x000001, 0x3504F2, 0x3504F3, 0x3504F4, 0x400000, 0x7FFFFF)
    sweep = np.array([((e + 127) << 23) | m for e in range(-46, 0) for m in mantissas], np.uint32).view(np.float32)
    assert tiny[0] == np.float32(2.0 ** -46) and sweep[0] == tiny[0] and bool(((sweep > 0) & (sweep < 1)).all())
    for name, values in (("multiples of 2^-46", tiny), ("exponent sweep", sweep)):
        err, half_ulp = _ln32_errors(values)
        excess = err - half_ulp
        print("ln32 on the", name, ": max error", err.max(), "max error beyond half an ulp of the result", excess.max())
        assert bool((excess <= 1e-7).all()), (name, values[int(np.argmax(excess))], excess.max())


@pytest.fixture(scope="module")
def cage(oracle):
    env = oracle.env()
    for c in SPHERE_CAGE:
        env.add_sphere(*c, 0.2)
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return lambda a, b: oracle.validate_motion(rid, env, a, b), lower, span


def test_in_bounds_phs_samples_lie_in_the_informed_set(cage):
    """dist(t, start) + dist(t, goal) <= max_cost (1 + 1e-5), in float64, for bounds from just above the straight line to
    three times it; and a loose bound does throw samples out of the joint bounds"""
    _, lower, span = cage
    a, b = np.array(CAGE_START, np.float32), np.array(CAGE_GOAL, np.float32)
    phs, u = PHS(a, b, lower, span), Uniform(1000)
    kept = {}
    for factor in (1.0001, 1.05, 1.3, 2.0, 3.0):
        max_cost = np.float32(np.float32(factor) * phs.dmin)
        for _ in range(600):
            t, ok = phs.sample(u, max_cost)
            if ok:
                kept[factor] = kept.get(factor, 0) + 1
                f = np.linalg.norm(t.astype(np.float64) - a) + np.linalg.norm(t.astype(np.float64) - b)
                assert f <= float(max_cost) * (1 + 1e-5), (factor, f, max_cost)
    assert kept[1.0001] == 600 and 0 < kept[3.0] < 600
    assert u.c > 5 * 600 * 10  # at least 5 pairs of uniforms per sample


@pytest.fixture(scope="module")
def serial_results(cage):
    """skip -> the serial statement's result between the cage's start and goal (500-iteration searches, at most 3)"""
    question, lower, span = cage
    return {skip: aorrtc_serial(CAGE_START, CAGE_GOAL, lower, span, question, range_=1.0, max_iterations=4000,
                                max_internal_iterations=500, max_searches=3, max_cost_bound_resamples=4, skip=skip)
            for skip in (1000, 2000)}


def test_first_stage_is_rrtc_serial_then_simplify_serial(cage, serial_results):
    question, lower, span = cage
    for skip, w in serial_results.items():
        r = rrtc_serial(CAGE_START, CAGE_GOAL, lower, span, question, range_=1.0, max_iterations=4000, max_samples=8192, skip=skip)
        first = simplify_serial(r.path, question).path
        assert [q.tobytes() for q in w.first_path] == [q.tobytes() for q in first]
        assert w.first_cost == cost(first) and w.searches == 3
        assert w.iterations == r.iterations + 3 * 500 or w.improvements > 0
    off = aorrtc_serial(CAGE_START, CAGE_GOAL, lower, span, question, range_=1.0, max_iterations=4000, skip=1000, optimize=False)
    assert [q.tobytes() for q in off.path] == [q.tobytes() for q in serial_results[1000].first_path] and off.searches == 0


def test_costs_never_increase_and_paths_are_valid(cage, serial_results):
    question, _, _ = cage
    assert serial_results[1000].improvements >= 1  # 6.762 -> 4.479 in its first search
    for w in serial_results.values():
        bounds = [w.first_cost] + w.costs
        assert all(later <= earlier for earlier, later in zip(bounds[:-1], bounds[1:])) and w.cost == bounds[-1]
        assert sum(later < earlier for earlier, later in zip(bounds[:-1], bounds[1:])) == w.improvements
        assert w.path[0].tobytes() == np.array(CAGE_START, np.float32).tobytes()
        assert w.path[-1].tobytes() == np.array(CAGE_GOAL, np.float32).tobytes()
        assert all(question(a, b) for a, b in zip(w.path[:-1], w.path[1:]))
        assert w.cost == cost(w.path)
