"""planning.aorrtc_multi on the device against the serial statement (tests/aorrtc_serial.py) with the CPU oracle answering
every question: per problem the status, the iterations, the searches, the improvements, the first cost, the cost, the tree
sizes and every waypoint bit for bit, and every returned path runs from its start to its goal; the device sampler alone
against the serial sampler.  The paths of the mixed batch, of the NaN-start batch and of the searches themselves
(intermediate simplification off) are also re-validated by the oracle edge by edge; the other tests compare bits only
(check(valid=False) says why).  The problems are picked on the CPU."""
import numpy as np
import pytest

import envs
from aorrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, PHS, SOLVED, Uniform, aorrtc_serial
from oracle_lib import CAGE_GOAL, CAGE_START
from simplify_serial import cost, distance

pytestmark = pytest.mark.gpu
STATUS = {"solved": SOLVED, "max_iterations": MAX_ITERATIONS, "max_samples": MAX_SAMPLES}


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

    def expected(self, s):
        return aorrtc_serial(self.start, self.goal, self.scene.lower, self.scene.span, self.scene.question, range_=s.range,
                             balance=s.balance, tree_ratio=s.tree_ratio, max_iterations=s.max_iterations,
                             max_internal_iterations=s.max_internal_iterations, max_samples=s.max_samples,
                             max_cost_bound_resamples=s.max_cost_bound_resamples, max_searches=s.max_searches,
                             optimize=s.optimize, cost_bound_resample=s.cost_bound_resample,
                             simplify_intermediate=s.simplify_intermediate, skip=self.skip)


def settings_of(**kw):
    from vamp_mvt_amd import planning

    s = dict(range=1.0, max_iterations=4000, max_internal_iterations=500, max_searches=6, max_cost_bound_resamples=4,
             max_samples=8192)
    s.update(kw)
    return planning.AORRTCMultiSettings(**s)


def run(vamp, problems, settings):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, problems[0].scene.robot)
    return planning.aorrtc_multi(robot, np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                                 [p.scene.env for p in problems], settings, [p.skip for p in problems])


def key(r):
    """what must not depend on the rest of the batch"""
    return (r.status if isinstance(r.status, int) else STATUS[r.status], int(r.iterations), int(r.searches), int(r.improvements),
            np.float32(r.first_cost).tobytes(), np.float32(r.cost).tobytes(), list(r.size),
            [np.asarray(q, np.float32).tobytes() for q in r.path])


def check(problems, got, want, valid=True):
    """valid = False: bit for bit only.  simplify() subdivides without asking whether the halves of a valid edge are valid
    motions themselves, and the oracle rejects such a half in a good part of the simplified paths of these
    scenes; the paths of the searches themselves are re-validated where simplify_intermediate is off."""
    assert len(got) == len(want) == len(problems)
    for i, (p, g, w) in enumerate(zip(problems, got, want)):
        kg, kw = key(g), key(w)
        print(i, p.scene.kind, p.skip, "device", kg[:4], g.first_cost, g.cost, kg[6], "serial", kw[:4], w.first_cost, w.cost, kw[6])
        assert kg == kw, (i, p.scene.kind, p.skip)
        if w.solved:
            assert g.path[0].tobytes() == p.start.tobytes() and g.path[-1].tobytes() == p.goal.tobytes()
            assert not valid or all(p.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), i
            assert g.cost <= g.first_cost
        else:
            assert len(g.path) == 0 and g.cost == float("inf")


# --------------------------------------------------------------------------------------------------- the sampler alone
@pytest.mark.parametrize("robot, seed, counter", [("panda", 0, 0), ("ur5", 1000, 12345), ("baxter", 999999, 2 ** 32 - 40)])
def test_sampler(vamp, oracle, robot, seed, counter):
    """4,096 successive samples of the device sampler, bit for bit, with the counter (7 joints; 6: n + 2 even, no surplus
    Gaussian; 14); the last case wraps the 32-bit counter"""
    scene = Scene(oracle, robot, "empty")
    a, b = (x[0] for x in scene.valid_pairs(1, 3))
    max_cost = np.float32(np.float32(1.25) * distance(a, b))
    q, ok, c = getattr(vamp, robot).phs_samples(a, b, max_cost, seed, counter, 4096)
    phs, u = PHS(a, b, scene.lower, scene.span), Uniform(seed, counter)
    want = [phs.sample(u, max_cost) for _ in range(4096)]
    assert c == u.c
    assert [x.tobytes() for x in q] == [t.tobytes() for t, _ in want]
    assert list(ok) == [w for _, w in want]
    assert 0 < sum(ok)


# ------------------------------------------------------------------------------------------------------ the mixed batch
@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "mixed")}


@pytest.fixture(scope="module")
def mixed_batch(vamp, scenes):
    """20 Panda problems in interleaved order: 8 among rotated cuboids and capsules and 8 in the sphere cage between
    random valid configurations (skips 100 k), 4 between the cage's own start and goal; with the serial results and the
    device's.  The seeds are the first for which the serial results meet what is asserted below; the last assertion lets
    this batch be re-validated edge by edge (see check())."""
    problems = [Problem(scenes["mixed"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(8, 31)))]
    problems += [Problem(scenes["cage"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["cage"].valid_pairs(8, 22)))]
    problems += [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in (0, 1000, 2000, 6000)]
    order = np.random.default_rng(1).permutation(len(problems))
    problems = [problems[i] for i in order]
    s = settings_of()
    want = [p.expected(s) for p in problems]
    trees = [n for w in want for size in w.tree_sizes for n in size]
    assert sum(w.improvements > 0 for w in want) >= 2
    assert sum(w.improvements >= 2 for w in want) >= 1
    assert sum(w.reparents for w in want) >= 1
    assert sum(w.out_of_bounds for w in want) >= 1
    assert sum(w.solved and w.iterations == 0 for w in want) >= 2
    assert sum(not w.solved for w in want) >= 1
    assert max(trees) > 256
    assert min(trees) < 64
    assert all(p.scene.question(a, b) for p, w in zip(problems, want) for a, b in zip(w.path[:-1], w.path[1:]))
    return problems, want, run(vamp, problems, s)


def test_mixed_batch(mixed_batch):
    problems, want, got = mixed_batch
    check(problems, got, want)
    # the call's totals over all stages: at least the first stage's and the searches' questions (the simplifier asks whole windows)
    assert got[0].edges_checked >= sum(w.questions - w.simplify_questions for w in want) and got[0].validity_calls > 0


def _some(want, count=4):
    """problems of the mixed batch that ran searches, the improved ones first"""
    ranked = sorted(range(len(want)), key=lambda i: (-want[i].improvements, -want[i].searches, i))
    pick = sorted(ranked[:count])
    assert all(want[i].searches > 0 for i in pick) and any(want[i].improvements > 0 for i in pick)
    return pick


def test_independence(vamp, mixed_batch):
    """a problem's result depends on nothing but its own inputs: not on the batch, its order, or how often the host looks"""
    problems, want, got = mixed_batch
    base = [key(g) for g in got]
    s = settings_of()
    for i in _some(want):
        assert key(run(vamp, [problems[i]], s)[0]) == base[i]
    order = np.random.default_rng(2).permutation(len(problems))
    permuted = run(vamp, [problems[i] for i in order], s)
    assert [key(g) for g in permuted] == [base[i] for i in order]
    assert [key(g) for g in run(vamp, problems, settings_of(check_every=1))] == base


@pytest.mark.parametrize("change", [dict(cost_bound_resample=False), dict(max_cost_bound_resamples=1),
                                    dict(simplify_intermediate=False)])
def test_switches_against_the_serial_statement(vamp, mixed_batch, change):
    problems, want, _ = mixed_batch
    some = [problems[i] for i in _some(want)]
    s = settings_of(**change)
    expected = [p.expected(s) for p in some]
    assert any(w.searches > 0 for w in expected)
    check(some, run(vamp, some, s), expected, valid=not s.simplify_intermediate)


def test_small_pool(vamp, mixed_batch):
    """64 nodes per problem: searches that end because the pool is full"""
    problems, want, _ = mixed_batch
    some = [problems[i] for i in _some(want)]
    s = settings_of(max_samples=64)
    expected = [p.expected(s) for p in some]
    assert any(MAX_SAMPLES in w.search_status for w in expected)
    got = run(vamp, some, s)
    check(some, got, expected, valid=False)
    assert all(sum(g.size) <= 64 for g in got)


def test_without_optimize_it_is_rrtc_multi_then_simplify_multi(vamp, mixed_batch):
    from vamp_mvt_amd import planning

    problems, _, _ = mixed_batch
    s = settings_of(optimize=False)
    got = run(vamp, problems, s)
    robot = vamp.panda
    first = planning.rrtc_multi(robot, np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                                [p.scene.env for p in problems],
                                planning.RRTCMultiSettings(range=1.0, max_iterations=4000, max_samples=8192),
                                [p.skip for p in problems])
    solved = [i for i, r in enumerate(first) if r.solved]
    simplified = planning.simplify_multi(robot, [first[i].path for i in solved], [problems[i].scene.env for i in solved])
    assert len(solved) >= 2 and len(solved) < len(problems)
    for i, r in enumerate(first):
        assert (got[i].status, got[i].iterations, got[i].size, got[i].searches) == (r.status, r.iterations, r.size, 0)
        if i not in solved:
            assert len(got[i].path) == 0
    for i, r in zip(solved, simplified):
        assert [q.tobytes() for q in got[i].path] == [q.tobytes() for q in r.path]
        # (Path::cost as the contract states it, the sequential fp32 sum; planning.path_cost sums with numpy)
        assert np.float32(got[i].cost).tobytes() == np.float32(cost(r.path)).tobytes() == np.float32(got[i].first_cost).tobytes()


@pytest.mark.parametrize("robot", ["ur5", "baxter"])
def test_other_dimensions(vamp, oracle, robot):
    """6 and 14 joints, 4 problems each, endpoints valid by the oracle"""
    scene = Scene(oracle, robot, "mixed")
    problems = [Problem(scene, a, b, 100 * k) for k, (a, b) in enumerate(zip(*scene.valid_pairs(4, 5)))]
    s = settings_of(max_iterations=1500, max_internal_iterations=300, max_searches=3)
    want = [p.expected(s) for p in problems]
    assert any(w.searches > 0 for w in want)
    check(problems, run(vamp, problems, s), want, valid=False)


def test_a_non_finite_start_ends_unsolved_and_leaves_the_others_alone(vamp, scenes):
    s = settings_of(max_iterations=1500, max_searches=2)
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in (1000, 0, 2000)]
    want = [p.expected(s) for p in problems]
    problems[1].start[3] = np.nan
    got = run(vamp, problems, s)
    assert got[1].status != "solved" and len(got[1].path) == 0 and got[1].cost == float("inf") and got[1].searches == 0
    assert any(want[i].searches > 0 for i in (0, 2))
    check([problems[0], problems[2]], [got[0], got[2]], [want[0], want[2]])


def test_reference_shaped_entry_points(vamp, mixed_batch):
    """<robot>.aorrtc_multi and <robot>.aorrtc with a vamp.AORRTCSettings, end to end: the same bits as the batch, in the
    robot module's own PlanningResult and Path"""
    problems, want, got = mixed_batch
    pick = _some(want, 3)
    s = vamp.AORRTCSettings()
    s.rrtc.range, s.max_iterations, s.max_internal_iterations, s.max_samples, s.max_cost_bound_resamples = 1.0, 4000, 500, 8192, 4
    s.max_searches = 6  # (not a reference field: read where present)
    some = [problems[i] for i in pick]
    results = vamp.panda.aorrtc_multi(np.stack([p.start for p in some]), np.stack([p.goal for p in some]),
                                      [p.scene.env for p in some], s, [p.skip for p in some])
    for i, r in zip(pick, results):
        assert isinstance(r, vamp.panda.PlanningResult) and isinstance(r.path, vamp.panda.Path) and r.solved
        assert key(r) == key(got[i]) and r.nanoseconds > 0
        assert np.float32(r.path.numpy()).tobytes() == np.stack(got[i].path).tobytes()
    zero = Problem(some[0].scene, some[0].start, some[0].goal, 0)  # aorrtc() takes no skip: the Halton sequence from its start
    one = vamp.panda.aorrtc(zero.start, zero.goal, zero.scene.env, s, None)
    assert isinstance(one.path, vamp.panda.Path) and key(one) == key(run(vamp, [zero], settings_of())[0])
