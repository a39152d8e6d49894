"""vmv_aorrtc_multi_constrained / planning.aorrtc_multi_constrained: what holds without a device — every refusal of the
entry point in the header's order with *out untouched, vmv_plans_costs and vmv_plans_band_refused on its plans and on
another call's, the Python layers' own checks and field mapping, and the serial statement
(tests/aorrtc_constrained_serial.py) with a constraint that lets everything through against tests/aorrtc_serial.py."""
import ctypes

import numpy as np
import pytest

from aorrtc_constrained_serial import INVALID_ENDPOINT, aorrtc_constrained_serial
from aorrtc_serial import aorrtc_serial
from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
SENTINEL = 0x5A5A5A5A


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


def _call(_lib, handles, robot=0, n=None, drop=(), skips=None, n_constraints=1, record=None, cfields=None, max_stretch=0.0, keep=False,
          **settings):
    """one vmv_aorrtc_multi_constrained call with two problems; `drop` names the pointers passed as NULL; record: fields of the
    last constraint; cfields: fields of the constraint settings -> (status, *out, vmv_last_error())"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((max(len(handles), 1), 7), 0.5, np.float32)
    cs = _settings(_lib, **settings)
    cf = dict(max_iterations=0, pos_tol=0.0, rot_tol=0.0, rot_weight=0.0, damping=0.0, max_step=0.0, check_step=0.0)
    cf.update(cfields or {})
    ps = _lib.ConstraintPlanSettings(_lib.ConstraintSettings(*[cf[f] for f, _ in _lib.ConstraintSettings._fields_]), max_stretch)
    count = max(n_constraints, 1)
    recs = (_lib.EeConstraint * count)(*[_constraint(_lib, **(record or {})) if k == count - 1 else _constraint(_lib) for k in range(count)])
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "constraints": recs,
           "constraint_settings": ctypes.byref(ps), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_aorrtc_multi_constrained(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
                                               None if sk is None else sk.ctypes.data_as(_lib.c_u64_p), ptr["settings"],
                                               ptr["constraints"], n_constraints, ptr["constraint_settings"], ptr["out"])
    message = _lib.lib.vmv_last_error().decode()
    if rc == VMV_OK and not keep and "out" not in drop:
        assert _lib.lib.vmv_plans_destroy(out) == VMV_OK
        return rc, None, message
    return rc, out.value, message


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib, planning

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vmv_aorrtc_multi_constrained", "vmv_plans_costs", "vmv_plans_band_refused"):
        assert name in names and hasattr(dll, name)
    assert vamp.abi_version() == 1  # the change is additive
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.aorrtc_multi_constrained) and callable(robot.aorrtc_multi_constrained_raw)
    assert callable(planning.aorrtc_multi_constrained) and "invalid_endpoint" in planning.PLAN_STATUS


def test_refusals_in_the_headers_order(raw):
    """vmv_aorrtc_multi's checks in its order, then vmv_rrtc_multi's remaining ones and the constraint's own as
    vmv_rrtc_multi_constrained makes them; where two things are spoiled the earlier check's answer comes back; *out stays"""
    _lib, handles = raw
    refused = lambda **kw: _call(_lib, handles, **kw)[:2]  # noqa: E731
    bad = (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    # ---- vmv_aorrtc_multi's own, in its order
    for robot in (-1, 4, 7):
        assert refused(robot=robot) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    assert refused(robot=9, drop=("settings", "constraints")) == (VMV_ERR_UNKNOWN_ROBOT, SENTINEL)
    for drop in ("envs", "starts", "goals", "settings", "out"):
        assert refused(drop=(drop,)) == bad, drop
    assert refused(n=1 << 31) == bad and refused(n=1 << 25) == bad  # (no array is read)
    for settings in (dict(max_internal_iterations=0), dict(max_cost_bound_resamples=65), dict(questions_per_round=3),
                     dict(interpolate=1), dict(operations=(2, 1)), dict(operations=(3,)), dict(n_operations=9),
                     dict(max_waypoints=(1 << 24) + 1)):
        assert refused(**settings) == bad, settings
    # ---- then vmv_rrtc_multi's: the NULL handles, range, max_samples, the Halton sequence's limit
    assert _call(_lib, [handles[0], None])[:2] == bad
    for settings in (dict(range=0.0), dict(range=-1.0), dict(range=float("inf")), dict(range=float("nan")), dict(max_samples=1),
                     dict(max_samples=0), dict(max_iterations=1000001)):
        assert refused(**settings) == bad, settings
    assert refused(skips=[0, 999001], max_iterations=1000) == bad
    # ---- then the constraint's own, in vmv_rrtc_multi_constrained's order, with their words
    assert _call(_lib, handles, drop=("constraints",)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "null pointer")
    assert _call(_lib, handles, drop=("constraint_settings",)) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "null pointer")
    for count in (0, 3):
        assert _call(_lib, handles, n_constraints=count) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "n_constraints must be 1 or n_problems")
    for field in ("pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "check_step"):
        for v in (-1.0, float("nan"), float("inf")):
            rc, out, msg = _call(_lib, handles, cfields={field: v})
            assert (rc, out) == bad and msg.startswith(field + " must be"), (field, v, msg)
    rc, out, msg = _call(_lib, handles, cfields=dict(max_iterations=1 << 30))
    assert (rc, out) == bad and msg.startswith("max_iterations must be")
    for v in (-1.0, float("nan"), float("inf")):
        rc, out, msg = _call(_lib, handles, max_stretch=v)
        assert (rc, out) == bad and msg.startswith("max_stretch must be"), v
    rc, out, msg = _call(_lib, handles, record=dict(max_angle=2.0))
    assert (rc, out) == bad and msg.startswith("constraints[0]: max_angle")
    rc, out, msg = _call(_lib, handles, record=dict(pos_lo={0: 1.0}, pos_hi={0: 0.0}), n_constraints=2)
    assert (rc, out) == bad and msg.startswith("constraints[1]: pos_lo must not exceed")
    rc, out, msg = _call(_lib, handles, record=dict(frame={3: float("nan")}))
    assert (rc, out) == bad and msg.startswith("constraints[0]: frame must be finite")
    # ---- which check wins where two apply
    assert refused(max_internal_iterations=0, drop=("constraints",)) == bad
    assert _call(_lib, handles, questions_per_round=3, n_constraints=3)[2] != "n_constraints must be 1 or n_problems"
    assert _call(_lib, handles, range=0.0, n_constraints=3)[2] != "n_constraints must be 1 or n_problems"
    assert _call(_lib, handles, drop=("constraints",), n_constraints=3)[2] == "null pointer"
    assert _call(_lib, handles, n_constraints=3, cfields=dict(pos_tol=-1.0))[2] == "n_constraints must be 1 or n_problems"
    assert _call(_lib, handles, cfields=dict(pos_tol=-1.0), max_stretch=-1.0, record=dict(max_angle=2.0))[2].startswith("pos_tol")
    assert _call(_lib, handles, max_stretch=-1.0, record=dict(max_angle=2.0))[2].startswith("max_stretch")
    # ---- a well-formed call reaches the environments' own checks, which need no device either
    assert refused() == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(n_constraints=2) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(max_stretch=3.0, optimize=0, max_searches=3) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert refused(skips=[0, 999000], max_iterations=1000) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, [handles[0], handles[0]])[:2] == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # repeated handles are allowed
    assert refused(record=dict(max_angle=2.0)) == bad  # a refusal wins over the environments' state


def test_no_problems_is_ok_and_the_readouts_know_their_results(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    rc, plans, _ = _call(_lib, [], n=0, keep=True)
    assert rc == VMV_OK and plans not in (None, SENTINEL)
    rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.vmv_plans_summary(plans, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
    assert (rounds.value, questions.value) == (0, 0)
    assert L.vmv_plans_costs(plans, None, None, None, None) == VMV_OK  # both readouts accept the new plans
    assert L.vmv_plans_band_refused(plans, None) == VMV_OK
    assert L.vmv_plans_paths(plans, None, 0) == VMV_OK
    assert L.vmv_plans_destroy(plans) == VMV_OK
    # n_constraints neither 1 nor n_problems (0 here), and a refusal wins over the empty batch
    assert _call(_lib, [], n=0, n_constraints=0)[0] == VMV_OK
    assert _call(_lib, [], n=0, n_constraints=2) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL, "n_constraints must be 1 or n_problems")
    assert _call(_lib, [], n=0, record=dict(max_angle=2.0))[:2] == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    # vmv_aorrtc_multi's plans carry costs and no band count; vmv_rrtc_multi_constrained's a band count and no costs
    cs = _settings(_lib)
    plain = ctypes.c_void_p()
    assert L.vmv_aorrtc_multi(0, None, 0, None, None, None, ctypes.byref(cs), ctypes.byref(plain)) == VMV_OK
    word = (ctypes.c_uint32 * 1)(77)
    assert L.vmv_plans_costs(plain, None, None, None, None) == VMV_OK
    assert L.vmv_plans_band_refused(plain, word) == VMV_ERR_INVALID_ARGUMENT and word[0] == 77
    assert L.vmv_plans_destroy(plain) == VMV_OK
    gs = _lib.RrtcGoalsSettings(_lib.RrtcSettings(1.0, 1, 1.0, 10, 64, 0), 0, 4.0, 0.0001, 1.0, 0)
    ps = _lib.ConstraintPlanSettings(_lib.ConstraintSettings(), 0.0)
    recs = (_lib.EeConstraint * 1)(_constraint(_lib))
    first = ctypes.c_void_p()
    assert L.vmv_rrtc_multi_constrained(0, None, 0, None, None, None, None, ctypes.byref(gs), recs, 1, ctypes.byref(ps),
                                        ctypes.byref(first)) == VMV_OK
    assert L.vmv_plans_band_refused(first, None) == VMV_OK
    assert L.vmv_plans_costs(first, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_destroy(first) == VMV_OK
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    none = np.zeros((0, 7), np.float32)
    assert planning.aorrtc_multi_constrained(vamp.panda, none, none, [], c) == []
    assert vamp.panda.aorrtc_multi_constrained(none, none, [], c, planning.AORRTCMultiSettings()) == []
    empty = vamp.panda.aorrtc_multi_constrained_raw(none, none, [], c, planning._aorrtc_settings(None))
    assert empty["band_refused"].shape == (0,) and empty["band_refused"].dtype == np.uint32 and empty["costs"].shape == (0,)


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.aorrtc_multi_constrained(vamp.panda, [CAGE_START], [CAGE_GOAL], [None], vamp.EEConstraint())
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback


# ---- the Python layers ----------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a, b = np.zeros((3, 7), np.float32), np.ones((3, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    c = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.AORRTCMultiSettings

    def f(*args, **kw):
        return planning.aorrtc_multi_constrained(vamp.panda, *args, **kw)

    with pytest.raises(ValueError):
        f(a, b, [env, None], c)  # two environments for three problems
    with pytest.raises(TypeError):
        f(a, b[:2], [env] * 3, c)
    with pytest.raises(TypeError):
        f(a[0], b[0], [env], c)
    with pytest.raises(TypeError):
        f(a, b, [env, "not an environment", None], c)
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, c, skips=[0, 1])
    for bad in (dict(range=0.0), dict(max_samples=1), dict(max_internal_iterations=0), dict(max_cost_bound_resamples=65),
                dict(simplify=planning.SimplifyMultiSettings(questions_per_round=3))):
        with pytest.raises(ValueError):
            f(a, b, [env] * 3, c, S(**bad))
    with pytest.raises(TypeError):
        f(a, b, [env] * 3, "upright")  # not an EEConstraint
    with pytest.raises(TypeError):
        f(a, b, [env] * 3, [c, None, c])
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, [c, c])  # 1 constraint or one per problem
    with pytest.raises(ValueError):
        f(a, b, [env] * 3, [])
    for stretch in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            f(a, b, [env] * 3, c, max_stretch=stretch)
    with pytest.raises(ValueError):
        vamp.panda.aorrtc_multi_constrained(a, b, [env] * 3, [c, c], S())  # the installed name takes the same road
    with pytest.raises(ValueError):
        f(a, b, [env, None], [c, c])  # aorrtc_multi's checks come first
    assert env._handle is None  # nothing was built or finalized


class _FakeRobot:
    """stands where planning expects a robot: records what the raw call was given and answers a fixed dict"""

    def __init__(self):
        self.calls = []

    def aorrtc_multi_constrained_raw(self, starts, goals, environments, constraints, settings, constraint_settings=None,
                                     max_stretch=2.0, skips=None):
        self.calls.append((starts, goals, environments, constraints, settings, constraint_settings, max_stretch, skips))
        pts = np.arange(5 * 2, dtype=np.float32).reshape(5, 2)
        inf = np.float32(np.inf)
        return dict(status=np.array([0, 4, 0, 1], np.uint8), iterations=np.array([30, 0, 1, 1200], np.uint32),
                    sizes=np.array([[5, 4], [0, 0], [1, 1], [90, 88]], np.uint32), path_lengths=np.array([3, 0, 2, 0], np.uint32),
                    paths=pts, rounds=41, questions=97, first_costs=np.array([2.5, inf, 1.25, inf], np.float32),
                    costs=np.array([2.0, inf, 1.25, inf], np.float32), searches=np.array([3, 0, 0, 0], np.uint32),
                    improvements=np.array([1, 0, 0, 0], np.uint32), band_refused=np.array([7, 0, 0, 12], np.uint32))


def test_planning_function_on_a_fake_robot(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    robot = _FakeRobot()
    ref = vamp.SimplifySettings()  # reference-shaped simplifier settings are converted as aorrtc_multi converts them
    s = planning.AORRTCMultiSettings(range=0.5, max_searches=3, simplify=ref)
    got = planning.aorrtc_multi_constrained(robot, "a", "b", ["e"] * 4, "c", s, "cs", [1, 2, 3, 4], 3.0)
    (starts, goals, envs, cons, given, cs, stretch, skips), = robot.calls
    assert (starts, goals, envs, cons, cs, stretch, skips) == ("a", "b", ["e"] * 4, "c", "cs", 3.0, [1, 2, 3, 4])
    assert isinstance(given.simplify, planning.SimplifyMultiSettings) and given.simplify == planning._as_simplify_multi_settings(ref)
    assert (given.range, given.max_searches) == (0.5, 3)
    assert [r.status for r in got] == ["solved", "invalid_endpoint", "solved", "max_iterations"]
    assert [r.band_refused for r in got] == [7, 0, 0, 12] and all(type(r.band_refused) is int for r in got)
    assert [len(r.path) for r in got] == [3, 0, 2, 0] and [r.iterations for r in got] == [30, 0, 1, 1200]
    assert [r.size for r in got] == [[5, 4], [0, 0], [1, 1], [90, 88]]
    assert [(r.first_cost, r.cost, r.searches, r.improvements) for r in got] == \
        [(2.5, 2.0, 3, 1), (float("inf"), float("inf"), 0, 0), (1.25, 1.25, 0, 0), (float("inf"), float("inf"), 0, 0)]
    assert np.array_equal(np.stack(got[2].path), np.arange(6, 10, dtype=np.float32).reshape(2, 2))
    assert (got[0].validity_calls, got[0].edges_checked) == (41, 97)
    planning.aorrtc_multi_constrained(robot, "a", "b", [], "c")
    assert robot.calls[1][4] == planning._aorrtc_settings(None) and robot.calls[1][5] is None and robot.calls[1][6] == 2.0
    # <robot>.aorrtc_multi_constrained maps the reference-shaped AORRTCSettings as <robot>.aorrtc_multi does
    seen = []
    monkeypatch.setattr(planning, "aorrtc_multi_constrained",
                        lambda r, a, b, envs, c, settings, cs=None, skips=None, max_stretch=2.0: seen.append((c, settings, cs, skips, max_stretch)) or [])
    rs = vamp.AORRTCSettings()
    rs.rrtc.range, rs.max_iterations, rs.max_cost_bound_resamples = 0.75, 5000, 1000
    z = np.zeros((2, 7), np.float32)
    assert vamp.panda.aorrtc_multi_constrained(z, z, [None, None], "c", rs, "cs", skips=[5, 6], max_stretch=1.5) == []
    c, m, cs, skips, stretch = seen[0]
    assert (c, cs, skips, stretch) == ("c", "cs", [5, 6], 1.5) and isinstance(m, planning.AORRTCMultiSettings)
    assert (m.range, m.max_iterations, m.max_cost_bound_resamples) == (0.75, 5000, 64)
    bad = vamp.AORRTCSettings(anytime=True)
    with pytest.raises(NotImplementedError):
        vamp.panda.aorrtc_multi_constrained(z, z, [None, None], "c", bad)


# ---- the serial statement ---------------------------------------------------------------------------------------------------
class _LetsEverythingThrough:
    """stands where the statement expects the product's robot: every projection converges where it stands, every
    configuration and every edge is in band"""

    def __init__(self):
        self.projected = self.edges = 0

    def project_batch(self, q, constraint, settings=None):
        self.projected += len(q)
        return q.copy(), None, np.ones(len(q), bool), None

    def constraint_check_batch(self, q, constraint, settings=None):
        return np.ones(len(q), bool)

    def constraint_check_motion_batch(self, a, b, constraint, settings=None):
        self.edges += len(a)
        return np.ones(len(a), bool)


@pytest.fixture(scope="module")
def cage(oracle):
    env = oracle.env()
    for c in SPHERE_CAGE:
        env.add_sphere(*c, 0.2)
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return lambda a, b: oracle.validate_motion(rid, env, a, b), lower, span


@pytest.mark.parametrize("skip,kw", [(1000, dict()), (2000, dict(simplify_intermediate=False)), (1000, dict(optimize=False)),
                                     (2000, dict(max_samples=64, max_searches=2))])
def test_a_constraint_that_lets_everything_through_is_the_unconstrained_statement(cage, skip, kw):
    question, lower, span = cage
    settings = dict(range_=1.0, max_iterations=3000, max_internal_iterations=400, max_searches=3, max_cost_bound_resamples=4, skip=skip)
    settings.update(kw)
    want = aorrtc_serial(CAGE_START, CAGE_GOAL, lower, span, question, **settings)
    mod = _LetsEverythingThrough()
    got = aorrtc_constrained_serial(mod, CAGE_START, CAGE_GOAL, lower, span, question, "constraint", **settings)
    for name in ("status", "iterations", "size", "searches", "improvements", "questions", "simplify_questions", "reparents",
                 "out_of_bounds", "search_status", "tree_sizes"):
        assert getattr(got, name) == getattr(want, name), name
    assert np.float32(got.first_cost).tobytes() == np.float32(want.first_cost).tobytes()
    assert np.float32(got.cost).tobytes() == np.float32(want.cost).tobytes() and got.costs == want.costs
    assert [q.tobytes() for q in got.path] == [q.tobytes() for q in want.path] and want.solved
    assert (got.band_refused, got.first_refused, got.search_refused, got.simplify_refused) == (0, 0, 0, 0)
    if kw.get("optimize", True):
        assert want.searches >= 2


def test_the_reparent_question_is_told_from_the_other_two(cage):
    """max_stretch 1.001: an extension and a march step are at most `range` long and pass, a re-parent edge - its near end
    is a nearest node in cost space - may be longer.  Were the stretch rule applied to it, the statement could not equal
    aorrtc_serial here; it is band-checked only, so the re-parents happen as they do unconstrained."""
    valid, lower, span = cage
    settings = dict(range_=1.0, max_iterations=3000, max_internal_iterations=400, max_searches=3, max_cost_bound_resamples=4, skip=1000,
                    simplify_intermediate=False)  # (so that every question is the first stage's or a search's)
    want = aorrtc_serial(CAGE_START, CAGE_GOAL, lower, span, valid, **settings)
    asked = []

    def question(a, b):
        asked.append(float(np.linalg.norm(np.asarray(b, np.float64) - np.asarray(a, np.float64))))
        return valid(a, b)

    got = aorrtc_constrained_serial(_LetsEverythingThrough(), CAGE_START, CAGE_GOAL, lower, span, question, "constraint", max_stretch=1.001,
                                    **settings)
    print("re-parents", want.reparents, "longest edge asked after the direct one", max(asked[1:]))
    assert want.reparents > 0 and max(asked[1:]) > 1.001  # only a re-parent edge can be that long
    assert got.reparents == want.reparents and got.questions == want.questions == len(asked)
    assert [q.tobytes() for q in got.path] == [q.tobytes() for q in want.path]


def test_an_out_of_band_endpoint_asks_nothing(cage):
    question, lower, span = cage

    class _StartOut(_LetsEverythingThrough):
        def constraint_check_batch(self, q, constraint, settings=None):
            ok = np.ones(len(q), bool)
            ok[0] = False
            return ok

    got = aorrtc_constrained_serial(_StartOut(), CAGE_START, CAGE_GOAL, lower, span, question, "constraint", range_=1.0, max_iterations=100)
    assert got.status == INVALID_ENDPOINT and got.path == [] and got.questions == 0 and got.searches == 0
    assert got.first_cost == float("inf") and got.cost == float("inf") and got.band_refused == 0
