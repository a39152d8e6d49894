"""planning.rrtc_multi on the device against the serial comparator (tests/rrtc_serial.py) with the CPU oracle answering
every question: per problem the status, the iterations, the tree sizes and every waypoint bit for bit; and every returned
path runs from its start to its goal and is valid under the oracle edge by edge.  The problems are picked on the CPU."""
import numpy as np
import pytest

import envs
from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED, rrtc_serial

pytestmark = pytest.mark.gpu
STATUS = {"solved": SOLVED, "max_iterations": MAX_ITERATIONS, "max_samples": MAX_SAMPLES}
CAGE_TABLE = {0: (605, [37, 22]), 1000: (663, [44, 24]), 2000: (219, [18, 13]), 3000: (338, [27, 17]),
              4000: (398, [23, 43]), 5000: (208, [15, 23])}  # skip -> iterations, size at range 1.0 (all solved)


class Scene:
    """one environment, built alike for the product and the oracle"""

    def __init__(self, oracle, robot, kind):
        self.robot, self.kind = robot, kind
        self.rid = oracle.robot(robot)
        self.lower, self.span = oracle.bounds(self.rid)
        spec = envs.spec_for(kind, robot)
        self.oenv = envs.build_oracle_env(oracle, spec)
        self.env = envs.build_product_env(spec) if spec else None  # None = the empty environment
        self.o = oracle

    def question(self, a, b):
        return self.o.validate_motion(self.rid, self.oenv, a, b)

    def valid_pairs(self, n, seed):
        """n (start, goal) pairs of uniform configurations that are valid by the oracle"""
        rng = np.random.default_rng(seed)
        q = (self.lower + self.span * rng.random((64 * n, len(self.lower)), dtype=np.float32)).astype(np.float32)
        q = q[self.o.validate_batch(self.rid, self.oenv, q)][: 2 * n]
        assert len(q) == 2 * n
        return q[0::2], q[1::2]


class Problem:
    def __init__(self, scene, start, goal, skip):
        self.scene, self.skip = scene, int(skip)
        self.start, self.goal = np.array(start, np.float32), np.array(goal, np.float32)

    def expected(self, settings):
        return rrtc_serial(self.start, self.goal, self.scene.lower, self.scene.span, self.scene.question,
                           range_=settings.range, balance=settings.balance, tree_ratio=settings.tree_ratio,
                           max_iterations=settings.max_iterations, max_samples=settings.max_samples, skip=self.skip)


def run(vamp, problems, settings):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, problems[0].scene.robot)
    return planning.rrtc_multi(robot, np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                               [p.scene.env for p in problems], settings, [p.skip for p in problems])


def key(result):
    """what must not depend on the rest of the batch: status, iterations, size and the waypoints' bits"""
    return (result.status if isinstance(result.status, int) else STATUS[result.status], int(result.iterations),
            list(result.size), [np.asarray(q, np.float32).tobytes() for q in result.path])


def check(problems, got, want):
    assert len(got) == len(want) == len(problems)
    for i, (p, g, w) in enumerate(zip(problems, got, want)):
        assert key(g) == key(w), (i, p.scene.kind, p.skip, key(g)[:3], key(w)[:3])
        if w.solved:
            assert g.path[0].tobytes() == p.start.tobytes() and g.path[-1].tobytes() == p.goal.tobytes()
            assert all(p.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), i
        else:
            assert len(g.path) == 0


def settings_of(**kw):
    from vamp_mvt_amd import planning

    s = dict(range=1.0, balance=True, tree_ratio=1.0, max_iterations=3000, max_samples=8192, check_every=0)
    s.update(kw)
    return planning.RRTCMultiSettings(**s)


@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "empty", "mixed")}  # mixed: rotated cuboids and capsules


@pytest.fixture(scope="module")
def mixed_batch(vamp, scenes):
    """40 Panda problems in interleaved order: 20 in the sphere cage (skips 0, 1000, ...), 8 in the empty environment, 12
    among rotated cuboids and capsules; with the comparator's results and the device's for the default check_every"""
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, 1000 * k) for k in range(20)]
    problems += [Problem(scenes["empty"], a, b, 7 * k) for k, (a, b) in enumerate(zip(*scenes["empty"].valid_pairs(8, 3)))]
    problems += [Problem(scenes["mixed"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(12, 5)))]
    order = np.random.default_rng(1).permutation(len(problems))
    problems = [problems[i] for i in order]
    s = settings_of()
    want = [p.expected(s) for p in problems]
    # the batch is what the test needs: direct solutions in the empty environment, blocked direct edges elsewhere
    assert sum(p.scene.kind == "empty" and w.solved and w.iterations == 0 for p, w in zip(problems, want)) >= 6
    assert sum(p.scene.kind == "mixed" for p in problems) >= 6
    assert any(p.scene.kind == "mixed" and w.iterations > 0 for p, w in zip(problems, want))
    return problems, want, run(vamp, problems, s)


def test_mixed_batch(mixed_batch):
    problems, want, got = mixed_batch
    check(problems, got, want)
    seen = {}
    for p, g in zip(problems, got):
        if p.scene.kind == "cage" and p.skip in CAGE_TABLE:
            seen[p.skip] = (g.status, g.iterations, g.size)
    assert seen == {k: ("solved", it, size) for k, (it, size) in CAGE_TABLE.items()}
    assert got[0].edges_checked == sum(w.questions for w in want)  # the call's question total
    assert got[0].validity_calls >= max(w.questions for w in want)  # rounds: one question per problem per round


def test_large_trees(vamp, scenes):
    """trees beyond one wave's and one workgroup's lanes: the strided search and the cross-wave argmin"""
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in (0, 1000)]
    s = settings_of(range=0.25, max_iterations=4000)
    want = [p.expected(s) for p in problems]
    assert [w.size for w in want] == [[283, 155], [640, 331]] and [w.iterations for w in want] == [1442, 3274]
    check(problems, run(vamp, problems, s), want)


@pytest.mark.parametrize("limit", [dict(max_iterations=100), dict(max_samples=30)])
def test_limits(vamp, scenes, limit):
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, 1000 * k) for k in range(6)]
    problems.insert(3, Problem(scenes["empty"], CAGE_START, CAGE_GOAL, 0))  # (a direct solution is no limit case)
    s = settings_of(**limit)
    want = [p.expected(s) for p in problems]
    reason = MAX_ITERATIONS if "max_iterations" in limit else MAX_SAMPLES
    assert sum(w.status == reason for w in want) >= 4
    if "max_iterations" in limit:
        assert (want[0].status, want[0].iterations, want[0].size) == (MAX_ITERATIONS, 100, [4, 8])
    got = run(vamp, problems, s)
    check(problems, got, want)
    assert all(sum(g.size) <= s.max_samples for g in got)


def test_independence(vamp, mixed_batch):
    """a problem's result depends on nothing but its own inputs: not on the batch, its order, or how often the host looks"""
    problems, _, got = mixed_batch
    base = [key(g) for g in got]
    s = settings_of()
    assert [key(g) for g in run(vamp, problems[::-1], s)][::-1] == base
    assert [key(g) for g in run(vamp, problems, settings_of(check_every=1))] == base
    alone = [next(i for i, p in enumerate(problems) if p.scene.kind == kind and base[i][1] > lo)
             for kind, lo in (("cage", 0), ("mixed", 0), ("empty", -1))]
    for i in alone:
        assert key(run(vamp, [problems[i]], s)[0]) == base[i]


@pytest.mark.parametrize("robot, kind, seed", [("ur5", "mixed", 5), ("fetch", "mixed", 5), ("baxter", "mixed", 5)])
def test_other_dimensions(vamp, oracle, robot, kind, seed):
    """6, 8 and 14 joints, 8 problems each, endpoints valid by the oracle"""
    scene = Scene(oracle, robot, kind)
    problems = [Problem(scene, a, b, 100 * k) for k, (a, b) in enumerate(zip(*scene.valid_pairs(8, seed)))]
    s = settings_of(max_iterations=500)
    want = [p.expected(s) for p in problems]
    assert any(w.iterations > 0 for w in want) and any(w.solved and w.iterations > 0 for w in want)
    check(problems, run(vamp, problems, s), want)


def test_non_finite_endpoints_end_unsolved_and_leave_the_others_alone(vamp, scenes):
    s = settings_of(max_iterations=300)
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in (2000, 0, 5000, 0, 1000)]
    problems.append(Problem(scenes["empty"], CAGE_START, CAGE_GOAL, 0))
    want = [p.expected(s) for p in problems]
    problems[1].start[3] = np.nan
    problems[3].goal[0] = np.inf
    got = run(vamp, problems, s)
    for i in (1, 3):
        assert got[i].status != "solved" and len(got[i].path) == 0 and sum(got[i].size) <= s.max_samples
    rest = [0, 2, 4, 5]
    assert any(want[i].solved and want[i].iterations > 0 for i in rest)
    check([problems[i] for i in rest], [got[i] for i in rest], [want[i] for i in rest])


@pytest.fixture(scope="module")
def staggered(vamp, mixed_batch):
    """five problems of the mixed batch that finish in different rounds: two the direct question solves (finished in round
    2), the two shortest of the cage and one among the cuboids that needs iterations; run with the default check_every"""
    problems, want, _ = mixed_batch
    by_questions = sorted(range(len(problems)), key=lambda i: want[i].questions)
    pick = [i for i in by_questions if want[i].questions == 1][:2]
    pick += [i for i in by_questions if problems[i].scene.kind == "cage"][:2]
    pick.append(next(i for i in by_questions if problems[i].scene.kind == "mixed" and want[i].iterations > 0))
    assert len(pick) == 5 and len({want[i].questions for i in pick}) >= 4
    pick.sort()  # the batch's interleaved order
    some = [problems[i] for i in pick]
    return some, [want[i] for i in pick], run(vamp, some, settings_of())


@pytest.mark.parametrize("every", [1, 3])
def test_the_host_looks_every_check_every_rounds_and_changes_no_bit(vamp, staggered, every):
    """a problem asks one question per round and ends in the round after its last, so the call ends at the first look at
    or after round max(questions) + 1"""
    problems, want, base = staggered
    check(problems, base, want)
    got = run(vamp, problems, settings_of(check_every=every))
    assert [key(g) for g in got] == [key(g) for g in base]
    rounds, questions = got[0].validity_calls, got[0].edges_checked
    assert questions == base[0].edges_checked == sum(w.questions for w in want)
    assert rounds > 0 and rounds % every == 0
    assert rounds * len(problems) >= questions
    assert rounds == every * -(-(max(w.questions for w in want) + 1) // every)
    assert base[0].validity_calls == 16 * -(-(max(w.questions for w in want) + 1) // 16)
