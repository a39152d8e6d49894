"""planning.rrtc_multi_goals (goal sets, dynamic domain, start_tree_first) on the device against the serial statement
(tests/rrtc_goals_serial.py) with the CPU oracle answering every question: per problem the status, the iterations, the
tree sizes, the goal index and every waypoint bit for bit; and every returned path runs from its start to the goal it
names and is valid under the oracle edge by edge.  The problems are picked on the CPU (tests/rrtc_goals_cases.py)."""
import numpy as np
import pytest

import test_rrtc_multi_gpu as old
from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_goals_cases import (DOMAIN_TABLE, GOAL_SET_SETTINGS, REFERENCE_DOMAIN, TIGHT_DOMAIN, Problem, Scene, check, classes_of,
                              domain_problem, goal_set_problems, key, settings_dict)
from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED

pytestmark = pytest.mark.gpu
GPU_MAX_ITERATIONS = 6000  # a launch may run as many nearest searches as iterations are left: kept small


def run(vamp, problems, settings):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, problems[0].scene.robot)
    return planning.rrtc_multi_goals(robot, np.stack([p.start for p in problems]), [p.goals for p in problems],
                                     [p.scene.env for p in problems], planning.RRTCMultiSettings(**settings),
                                     [p.skip for p in problems])


def capped(settings):
    """the table's settings with max_iterations within the GPU tests' limit (no solved row needs more)"""
    return dict(settings, max_iterations=min(settings["max_iterations"], GPU_MAX_ITERATIONS))


@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "empty")}


def direct_problem(scene, n_goals, seed):
    """a problem of the empty environment: valid endpoints, so that the first goal is direct"""
    a, b = scene.valid_pairs(n_goals, seed)
    return Problem(scene, a[0], b, 7 * seed)


@pytest.fixture(scope="module")
def mixed_batch(vamp, scenes):
    """27 Panda problems in four settings groups, one call each, every group in permuted order: the dynamic-domain rows 1 - 3
    of the table; row 6; 17 goal-set problems of 2 .. 5 goals; start_tree_first with one goal and with two; and an
    empty-environment problem that is direct in each of the first three.  -> per group (settings, problems, want, got)"""
    cage, empty = scenes["cage"], scenes["empty"]
    groups = []
    rows = [domain_problem(cage, r) for r in (0, 1, 2)]
    groups.append((capped(rows[0][1]), [p for p, _ in rows] + [direct_problem(empty, 3, 1)]))
    p6, s6 = domain_problem(cage, 5)
    groups.append((s6, [p6, direct_problem(empty, 1, 2)]))
    groups.append((GOAL_SET_SETTINGS, goal_set_problems(cage) + [direct_problem(empty, 2, 3)]))
    two_goals = next(q for q in goal_set_problems(cage) if len(q.goals) == 2)
    groups.append((settings_dict(start_tree_first=True), [Problem(cage, CAGE_START, [CAGE_GOAL], 0),
                                                          Problem(cage, CAGE_START, [CAGE_GOAL], 1000), two_goals]))
    out = []
    for g, (s, problems) in enumerate(groups):
        problems = [problems[i] for i in np.random.default_rng(g).permutation(len(problems))]
        out.append((s, problems, [p.expected(s) for p in problems], run(vamp, problems, s)))
    return out


def test_mixed_batch(mixed_batch):
    for s, problems, want, got in mixed_batch:
        check(problems, got, want)
        assert got[0].edges_checked == sum(w.questions for w in want)  # the call's question total
        assert got[0].validity_calls >= max(w.questions for w in want)  # rounds: one question per problem per round
    # the groups are what the test needs: the table's rows with their pinned figures, every goal-set case, direct problems
    figures = {}
    for s, problems, want, got in mixed_batch[:2]:
        for p, g in zip(problems, got):
            if p.scene.kind == "cage":
                figures[(s["radius"], p.skip)] = (old.STATUS[g.status], g.iterations, g.size)
    assert figures == {(DOMAIN_TABLE[r][0]["radius"], DOMAIN_TABLE[r][2]): tuple(DOMAIN_TABLE[r][4:7]) for r in (0, 1, 2, 5)}
    _, problems, want, _ = mixed_batch[2]
    classes = classes_of(problems, want)
    assert {"direct_first", "direct_later", "tree_first", "tree_later", "unsolved"} <= set(classes)
    assert {len(p.goals) for p in problems} == {2, 3, 4, 5}
    assert sum(p.scene.kind == "empty" and w.solved and w.iterations == 0 for _, ps, ws, _ in mixed_batch for p, w in zip(ps, ws)) == 3
    _, problems, want, _ = mixed_batch[3]  # start_tree_first changed the one-goal searches (605 iterations without it)
    assert all(w.solved for w in want) and 605 not in [w.iterations for w in want]


@pytest.mark.parametrize("row", [3, 4])
def test_large_trees_under_dynamic_domain(vamp, scenes, row):
    p, s = domain_problem(scenes["cage"], row)
    s = capped(s)
    want = [p.expected(s)]
    assert (want[0].status, want[0].iterations, want[0].size) == tuple(DOMAIN_TABLE[row][4:7]) and sum(want[0].size) > 256
    check([p], run(vamp, [p], s), want)


def test_additions_off_is_rrtc_multi(vamp, scenes):
    problems = [old.Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in old.CAGE_TABLE]
    base = old.run(vamp, problems, old.settings_of())
    assert [(g.iterations, g.size) for g in base] == [old.CAGE_TABLE[p.skip] for p in problems]
    got = run(vamp, [Problem(p.scene, p.start, [p.goal], p.skip) for p in problems], settings_dict())
    assert [old.key(g) for g in got] == [old.key(g) for g in base]
    assert [g.goal_index for g in got] == [0] * len(problems)
    assert (got[0].validity_calls, got[0].edges_checked) == (base[0].validity_calls, base[0].edges_checked)


def test_independence(vamp, mixed_batch):
    """a problem's result depends on nothing but its own inputs: not on the batch, its order, or how often the host looks"""
    s, problems, want, got = mixed_batch[2]
    base = [key(g) for g in got]
    assert [key(g) for g in run(vamp, problems[::-1], s)][::-1] == base
    assert [key(g) for g in run(vamp, problems, dict(s, check_every=1))] == base
    classes = classes_of(problems, want)
    for i in (classes.index("tree_later"), classes.index("direct_later")):  # a goal-set problem and a direct one
        assert key(run(vamp, [problems[i]], s)[0]) == base[i]
    s, problems, _, got = mixed_batch[0]  # and a dynamic-domain problem of the table
    i = next(i for i, p in enumerate(problems) if p.scene.kind == "cage" and p.skip == 1000)
    assert key(run(vamp, [problems[i]], s)[0]) == key(got[i])


@pytest.mark.parametrize("robot, seed", [("ur5", 5), ("baxter", 5)])
def test_other_dimensions(vamp, oracle, robot, seed):
    """6 and 14 joints, 4 problems of 3 goals each among rotated cuboids and capsules, dynamic domain on"""
    scene = Scene(oracle, robot, "mixed")
    a, b = scene.valid_pairs(8, seed)
    goals = np.concatenate([a[4:], b])
    problems = [Problem(scene, a[k], goals[3 * k:3 * k + 3], 100 * k) for k in range(4)]
    s = settings_dict(max_iterations=500, **REFERENCE_DOMAIN)
    want = [p.expected(s) for p in problems]
    assert any(w.solved and w.iterations > 0 for w in want)
    check(problems, run(vamp, problems, s), want)


def test_max_samples_boundary(vamp, scenes):
    problems = [p for p in goal_set_problems(scenes["cage"]) if len(p.goals) == 3][:3]
    s = settings_dict(max_samples=4, **TIGHT_DOMAIN)  # 1 + G: the roots fill the pool
    want = [p.expected(s) for p in problems]
    tree = [i for i, w in enumerate(want) if not w.solved]
    assert tree and all((want[i].status, want[i].iterations, sum(want[i].size)) == (MAX_SAMPLES, 0, 4) for i in tree)
    got = run(vamp, problems, s)
    check(problems, got, want)
    assert all((got[i].status, got[i].iterations, sum(got[i].size)) == ("max_samples", 0, 4) for i in tree)
    problems = goal_set_problems(scenes["cage"])[:12]
    s = settings_dict(max_samples=30)  # (without the domain the trees of this batch grow beyond 30 nodes)
    want = [p.expected(s) for p in problems]
    assert any(w.status == MAX_SAMPLES and w.iterations > 0 for w in want)
    got = run(vamp, problems, s)
    check(problems, got, want)
    assert all(sum(g.size) <= 30 for g in got)


def test_a_non_finite_goal_inside_a_set(vamp, scenes):
    """the goal is never the nearest node and no edge to it is valid: the problem is solved through another goal of its set"""
    problems = goal_set_problems(scenes["cage"])[3:9]
    at = next(i for i, p in enumerate(problems) if len(p.goals) == 3)
    before = [p.expected(GOAL_SET_SETTINGS) for p in problems]
    problems[at].goals[0, 3] = np.nan
    want = list(before)
    want[at] = problems[at].expected(GOAL_SET_SETTINGS)
    assert want[at].solved and want[at].iterations > 0 and want[at].goal_index > 0
    assert any(w.solved and w.iterations > 0 for i, w in enumerate(want) if i != at)
    check(problems, run(vamp, problems, GOAL_SET_SETTINGS), want)


def test_rrtc_multi_with_an_addition_on(vamp, scenes):
    """planning.rrtc_multi and <robot>.rrtc_multi take a RRTCMultiSettings with dynamic domain to the new entry point"""
    from vamp_mvt_amd import planning

    p, s = domain_problem(scenes["cage"], 1)
    s = capped(s)
    want = p.expected(s)
    args = (p.start[None], p.goals, [p.scene.env], planning.RRTCMultiSettings(**s), [p.skip])
    check([p], planning.rrtc_multi(vamp.panda, *args), [want])
    got = vamp.panda.rrtc_multi(*args)[0]
    assert (got.status, got.iterations, got.size, got.goal_index) == ("solved", want.iterations, want.size, 0)
    assert [np.asarray(q, np.float32).tobytes() for q in got.path] == [q.tobytes() for q in want.path]
