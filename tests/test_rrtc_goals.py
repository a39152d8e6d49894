"""vmv_rrtc_multi_goals / planning.rrtc_multi_goals: what holds without a device — the serial statement's own figures
(DESIGN §5c "Goal sets, dynamic domain, start_tree_first" restated in tests/rrtc_goals_serial.py, with the CPU oracle
answering every question), the ABI surface, the checks that come before any device query, and the Python wrapper's
argument checks."""
import ctypes

import numpy as np
import pytest

from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_goals_cases import (DOMAIN_EVENTS, DOMAIN_TABLE, GOAL_SET_SETTINGS, Problem, Scene, check_path, classes_of,
                              domain_problem, goal_set_problems, settings_dict)
from rrtc_goals_serial import rrtc_goals_serial
from rrtc_serial import MAX_ITERATIONS, SOLVED, rrtc_serial
from test_rrtc_multi import CAGE_FIGURES

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
NAMES = ("vmv_rrtc_multi_goals", "vmv_plans_goal_indices")
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def cage(oracle):
    return Scene(oracle, "panda", "cage")


@pytest.mark.parametrize("range_, skip, max_iterations", [row[:3] for row in CAGE_FIGURES])
def test_additions_off_and_one_goal_is_the_old_comparator(cage, range_, skip, max_iterations):
    old = rrtc_serial(CAGE_START, CAGE_GOAL, cage.lower, cage.span, cage.question, range_=range_, max_iterations=max_iterations,
                      skip=skip)
    new = rrtc_goals_serial(CAGE_START, [CAGE_GOAL], cage.lower, cage.span, cage.question, range_=range_,
                            max_iterations=max_iterations, skip=skip)
    assert (new.status, new.iterations, new.size, new.questions) == (old.status, old.iterations, old.size, old.questions)
    assert [q.tobytes() for q in new.path] == [q.tobytes() for q in old.path]
    assert new.goal_index == (0 if old.solved else -1) and not any(new.events.values())


@pytest.mark.parametrize("row", range(len(DOMAIN_TABLE)))
def test_dynamic_domain_figures_on_the_sphere_cage(cage, row):
    status, iterations, size, questions = DOMAIN_TABLE[row][4:]
    p, s = domain_problem(cage, row)
    r = p.expected(s)
    assert (r.status, r.iterations, r.size, r.questions) == (status, iterations, size, questions)
    if row in DOMAIN_EVENTS:
        assert r.events == DOMAIN_EVENTS[row]
    # an iteration either is rejected, asks its extension (set, shrink, clamp: invalid; else valid) or has d == 0
    invalid = r.events["set"] + r.events["shrink"] + r.events["clamp"]
    assert r.events["reject"] + invalid <= r.iterations and r.events["grow"] <= sum(r.size) - 2
    check_path(p, r)
    assert r.goal_index == (0 if status == SOLVED else -1)


def test_start_tree_first_with_one_goal_changes_the_search(cage):
    p = Problem(cage, CAGE_START, [CAGE_GOAL], 0)
    default, first = p.expected(settings_dict(max_iterations=100000)), p.expected(settings_dict(max_iterations=100000, start_tree_first=True))
    assert (default.iterations, default.size, default.questions) == (605, [37, 22], 662)
    assert first.solved and (first.iterations, first.size) != (default.iterations, default.size)
    assert [q.tobytes() for q in first.path] != [q.tobytes() for q in default.path]
    check_path(p, first)


def test_start_tree_first_with_two_goals_changes_nothing(cage):
    """sizes 1 and G >= 2 never balance on the first iteration (tree_ratio 1): A is the start tree either way"""
    p = next(q for q in goal_set_problems(cage) if len(q.goals) == 2)
    a, b = p.expected(settings_dict()), p.expected(settings_dict(start_tree_first=True))
    assert a.iterations > 0 and (a.status, a.iterations, a.size, a.questions, a.goal_index) == (b.status, b.iterations, b.size, b.questions, b.goal_index)
    assert [q.tobytes() for q in a.path] == [q.tobytes() for q in b.path]


def test_goal_set_batch_holds_every_case(cage):
    problems = goal_set_problems(cage)
    want = [p.expected(GOAL_SET_SETTINGS) for p in problems]
    classes = classes_of(problems, want)
    for needed in ("direct_later", "tree_later", "tree_first", "unsolved"):
        assert needed in classes, classes
    assert {len(p.goals) for p in problems} == {2, 3, 4, 5}
    for i, (p, w) in enumerate(zip(problems, want)):
        check_path(p, w, i)
        if classes[i].startswith("direct"):  # one question per goal up to the first valid one, and nothing else
            assert (w.questions, w.size, len(w.path)) == (w.goal_index + 1, [1, 1], 2)
        else:
            assert w.questions > len(p.goals)
        if classes[i] == "unsolved":
            assert (w.status, w.iterations) == (MAX_ITERATIONS, 3000)


def test_comparator_does_not_import_the_package():
    import os
    import rrtc_goals_serial as m

    with open(os.path.abspath(m.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text


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


def _call(_lib, handles, robot=0, n=None, drop=(), skips=None, offsets=(0, 2, 3), **settings):
    """one vmv_rrtc_multi_goals call with two problems of 2 and 1 goals; `drop` names the pointers passed as NULL,
    offsets=None passes goal_offsets as NULL -> (status, *out)"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((4, 7), 0.5, np.float32)
    s = dict(range=1.0, balance=1, tree_ratio=1.0, max_iterations=1000, max_samples=64, check_every=0, dynamic_domain=0, radius=4.0,
             alpha=0.0001, min_radius=1.0, start_tree_first=0)
    s.update(settings)
    cs = _lib.RrtcGoalsSettings(_lib.RrtcSettings(s["range"], s["balance"], s["tree_ratio"], s["max_iterations"], s["max_samples"],
                                                  s["check_every"]),
                                s["dynamic_domain"], s["radius"], s["alpha"], s["min_radius"], s["start_tree_first"])
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_rrtc_multi_goals(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
                                       None if off is None else off.ctypes.data_as(_lib.c_size_p),
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


@pytest.mark.parametrize("offsets", [(1, 2, 3), (0, 2, 1), (0, 0, 2), (0, 2, 2), (0, 1, 2 ** 31), (0, 2 ** 40, 2 ** 40 + 1)])
def test_bad_offsets_and_empty_sets(raw, offsets):
    """offsets that do not start at 0, decrease, leave a set empty, or count 2^31 goals or more (no goal is read)"""
    _lib, handles = raw
    assert _call(_lib, handles, offsets=offsets) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_a_goal_set_must_fit_the_node_pool(raw):
    """1 + G <= max_samples; at the bound the next check speaks"""
    _lib, handles = raw
    assert _call(_lib, handles, max_samples=2) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)  # G = 2
    assert _call(_lib, handles, max_samples=3) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, handles, max_samples=2, offsets=None) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # one goal each
    assert _call(_lib, handles, max_samples=1, offsets=None) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


BAD_DOMAIN = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(min_radius=0.0),
              dict(min_radius=float("nan")), dict(min_radius=float("inf")), dict(alpha=-0.01), dict(alpha=1.0), dict(alpha=float("nan")),
              dict(alpha=float("inf"))]


@pytest.mark.parametrize("values", BAD_DOMAIN)
def test_domain_values_are_checked_only_when_the_domain_is_on(raw, values):
    _lib, handles = raw
    assert _call(_lib, handles, dynamic_domain=1, **values) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, dynamic_domain=0, **values) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # accepted as they are


@pytest.mark.parametrize("settings", [dict(range=0.0), dict(range=float("nan")), dict(max_samples=1), dict(max_samples=0)])
def test_bad_base_settings(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


def test_halton_validity_limit(raw):
    _lib, handles = raw
    assert _call(_lib, handles, max_iterations=1000001) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999001], max_iterations=1000) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, handles, skips=[0, 999000], max_iterations=1000) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, handles, max_iterations=1000000, dynamic_domain=1, start_tree_first=1) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_unfinalized_environment_is_reported_without_a_device(raw):
    _lib, handles = raw
    assert _call(_lib, handles) == (VMV_ERR_NOT_FINALIZED, SENTINEL)
    assert _call(_lib, [handles[0], handles[0]], dynamic_domain=1) == (VMV_ERR_NOT_FINALIZED, SENTINEL)


def test_no_problems_is_ok_and_empty(vamp):
    from vamp_mvt_amd import _lib, planning

    L = _lib.lib
    for offsets in (None, (0,)):
        rc, plans = _call(_lib, [], n=0, offsets=offsets)
        assert rc == VMV_OK and plans not in (None, SENTINEL)
        rounds, questions = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert L.vmv_plans_summary(plans, None, None, None, None, ctypes.byref(rounds), ctypes.byref(questions)) == VMV_OK
        assert (rounds.value, questions.value) == (0, 0)
        assert L.vmv_plans_paths(plans, None, 0) == VMV_OK
        assert L.vmv_plans_goal_indices(plans, None) == VMV_OK
        assert L.vmv_plans_destroy(plans) == VMV_OK
    assert L.vmv_plans_goal_indices(None, None) == VMV_ERR_INVALID_ARGUMENT
    assert planning.rrtc_multi_goals(vamp.panda, np.zeros((0, 7), np.float32), [], []) == []


def test_goal_indices_refuses_the_plans_of_another_call(vamp):
    from test_rrtc_multi import _call as call_rrtc_multi
    from vamp_mvt_amd import _lib

    rc, plans = call_rrtc_multi(_lib, [], n=0)
    assert rc == VMV_OK
    assert _lib.lib.vmv_plans_goal_indices(plans, None) == VMV_ERR_INVALID_ARGUMENT
    assert _lib.lib.vmv_plans_destroy(plans) == VMV_OK


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.rrtc_multi_goals(vamp.panda, [CAGE_START], [[CAGE_GOAL, CAGE_START]], [None])
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback
    with pytest.raises(vamp.VmvError) as ei:
        planning.rrtc_multi(vamp.panda, [CAGE_START], [CAGE_GOAL], [None], planning.RRTCMultiSettings(dynamic_domain=True))
    assert ei.value.status == VMV_ERR_NO_DEVICE


def test_rrtc_multi_takes_the_old_entry_point_while_the_additions_are_off(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    calls = []
    empty = dict(status=np.zeros(0, np.uint8), iterations=np.zeros(0, np.uint32), sizes=np.zeros((0, 2), np.uint32),
                 path_lengths=np.zeros(0, np.uint32), paths=np.zeros((0, 7), np.float32), rounds=0, questions=0)
    monkeypatch.setattr(vamp.panda, "rrtc_multi_raw", lambda *a: calls.append("rrtc_multi") or empty, raising=False)
    monkeypatch.setattr(vamp.panda, "rrtc_multi_goals_raw", lambda *a: calls.append("rrtc_multi_goals") or empty, raising=False)
    S = planning.RRTCMultiSettings
    for s in (None, S(), S(range=0.5, check_every=3), S(radius=4.0, alpha=0.0001, min_radius=1.0)):
        planning.rrtc_multi(vamp.panda, [], [], [], s)
    assert calls == ["rrtc_multi"] * 4
    for s in (S(dynamic_domain=True), S(start_tree_first=True), S(radius=2.0), S(alpha=0.05), S(min_radius=1.5)):
        planning.rrtc_multi(vamp.panda, [], [], [], s)
    assert calls[4:] == ["rrtc_multi_goals"] * 5


def test_settings_and_result_gained_their_fields_at_the_end(vamp):
    from vamp_mvt_amd import planning

    s = planning.RRTCMultiSettings(1.0, False, 0.5, 10, 20, 3)  # positional construction up to check_every is unchanged
    assert (s.range, s.balance, s.tree_ratio, s.max_iterations, s.max_samples, s.check_every) == (1.0, False, 0.5, 10, 20, 3)
    assert (s.dynamic_domain, s.radius, s.alpha, s.min_radius, s.start_tree_first) == (False, 4.0, 0.0001, 1.0, False)
    assert planning.PlanningResult().goal_index == -1
    assert callable(vamp.panda.rrtc_multi_goals) and callable(vamp.baxter.rrtc_multi_goals)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    a = np.zeros((3, 7), np.float32)
    sets = [np.ones((2, 7), np.float32), np.ones((1, 7), np.float32), np.ones((4, 7), np.float32)]
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    S = planning.RRTCMultiSettings

    def f(*args, **kw):
        return planning.rrtc_multi_goals(vamp.panda, *args, **kw)

    with pytest.raises(TypeError):
        f(a, [sets[0], np.ones(7, np.float32), sets[2]], [env] * 3)  # a [dim] vector is no goal set
    with pytest.raises(TypeError):
        f(a, [sets[0], np.zeros((0, 7), np.float32), sets[2]], [env] * 3)  # an empty set
    with pytest.raises(TypeError):
        f(a, [sets[0], np.ones((2, 6), np.float32), sets[2]], [env] * 3)  # wrong dimension
    with pytest.raises(TypeError):
        f(a, np.ones((3, 7), np.float32), [env] * 3)  # an [n][dim] array is n vectors, not n sets
    with pytest.raises(TypeError):
        f(a, sets[:2], [env] * 3)  # two sets for three starts
    with pytest.raises(TypeError):
        f(a[0], sets[:1], [env])  # one problem still is a [1][dim] array of starts
    with pytest.raises(ValueError):
        f(a, sets, [env, None])  # two environments for three problems
    with pytest.raises(TypeError):
        f(a, sets, [env, "not an environment", None])
    with pytest.raises(ValueError):
        f(a, sets, [env] * 3, skips=[0, 1])
    with pytest.raises(ValueError):
        f(a, sets, [env] * 3, skips=[0, 1, -1])
    with pytest.raises(ValueError):
        f(a, sets, [env] * 3, S(range=0.0))
    with pytest.raises(ValueError):
        f(a, sets, [env] * 3, S(max_samples=1))
    with pytest.raises(ValueError):
        f(a, sets, [env] * 3, S(max_samples=4))  # 1 + 4 goals
    for bad in (dict(radius=0.0), dict(radius=float("nan")), dict(min_radius=-1.0), dict(alpha=1.0), dict(alpha=-0.5)):
        with pytest.raises(ValueError):
            f(a, sets, [env] * 3, S(dynamic_domain=True, **bad))
    with pytest.raises(ValueError):
        vamp.panda.rrtc_multi_goals(a, sets, [env, None], S())  # the installed name takes the same road
    # rrtc_multi with an addition on takes the new entry point: the same checks in front of it
    b = np.ones((3, 7), np.float32)
    on = S(start_tree_first=True)
    with pytest.raises(ValueError):
        planning.rrtc_multi(vamp.panda, a, b, [env, None], on)
    with pytest.raises(TypeError):
        planning.rrtc_multi(vamp.panda, a, b[:2], [env] * 3, on)
    with pytest.raises(TypeError):
        planning.rrtc_multi(vamp.panda, a[0], b[0], [env], on)
    with pytest.raises(ValueError):
        planning.rrtc_multi(vamp.panda, a, b, [env] * 3, S(dynamic_domain=True, alpha=2.0))
    with pytest.raises(ValueError):
        vamp.panda.rrtc_multi(a, b, [env] * 3, S(dynamic_domain=True, radius=-1.0))  # a RRTCMultiSettings is taken as it is
    assert env._handle is None  # nothing was built or finalized
