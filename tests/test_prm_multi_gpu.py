"""planning.prm_multi on the device against the serial comparator (tests/prm_serial.py) with the CPU oracle answering
every question.  Every assertion is bit for bit: per problem the status, the iterations, the valid-vertex, candidate-edge
and valid-edge counts, the cost's bits and every waypoint's bits; and every returned path runs from its start to its goal
and is valid under the oracle edge by edge.  The problems are picked on the CPU."""
import numpy as np
import pytest

import envs
from oracle_lib import CAGE_GOAL, CAGE_START
from prm_serial import INVALID_ENDPOINT, NO_PATH, SOLVED, halton_samples, prm_serial

pytestmark = pytest.mark.gpu
STATUS = {"solved": SOLVED, "no_path": NO_PATH, "invalid_endpoint": INVALID_ENDPOINT}
f32 = np.float32


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

    def valid(self, q):
        return self.o.validate(self.rid, self.oenv, q)

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
    def __init__(self, scene, start, goal, skip=0, samples=None):
        self.scene, self.skip, self.samples = scene, int(skip), samples
        self.start, self.goal = np.array(start, np.float32), np.array(goal, np.float32)
        self._want = {}

    def expected(self, s):
        key = (s.n_samples, s.k, s.radius)
        if key not in self._want:  # the comparator's answer is computed once and never changed
            samples = self.samples if self.samples is not None else halton_samples(self.skip, s.n_samples, self.scene.lower,
                                                                                   self.scene.span)
            self._want[key] = prm_serial(self.start, self.goal, samples, self.scene.valid, self.scene.question, k=s.k,
                                         radius=s.radius)
        return self._want[key]


def settings_of(**kw):
    from vamp_mvt_amd import planning

    s = dict(n_samples=256, k=6, radius=float("inf"), keep_roadmaps=False)
    s.update(kw)
    return planning.PRMMultiSettings(**s)


def run(vamp, problems, settings):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, problems[0].scene.robot)
    samples = None if problems[0].samples is None else np.stack([p.samples for p in problems])
    return planning.prm_multi(robot, np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                              [p.scene.env for p in problems], settings, [p.skip for p in problems], samples)


def key(result):
    """everything a problem returns, in bits: status, iterations, valid vertices and edges, candidate edges, cost, waypoints"""
    questions = result.questions if hasattr(result, "questions") else result.edges_checked
    return (result.status if isinstance(result.status, int) else STATUS[result.status], int(result.iterations),
            [int(x) for x in result.size], int(questions), f32(result.cost).tobytes(),
            [np.asarray(q, np.float32).tobytes() for q in result.path])


def check(problems, got, want):
    assert len(got) == len(want) == len(problems)
    for i, (p, g, w) in enumerate(zip(problems, got, want)):
        assert key(g) == key(w), (i, p.scene.kind, p.skip, key(g)[:4], key(w)[:4], float(g.cost), float(w.cost))
        if w.solved:
            assert g.path[0].tobytes() == p.start.tobytes() and g.path[-1].tobytes() == p.goal.tobytes()
            assert all(p.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), i
        else:
            assert len(g.path) == 0 and np.isinf(g.cost)


def check_roadmap(g, w):
    """the kept roadmap: vertex flags and the whole candidate list, pair by pair and flag by flag"""
    vertex, pairs, flags = g.roadmap
    assert vertex.tolist() == w.vertex_valid.tolist()
    assert pairs.tolist() == w.pairs.tolist()
    assert flags.tolist() == w.edge_valid.tolist()


@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "empty", "mixed")}  # mixed: rotated cuboids and capsules


def inside_cage_obstacle(scene):
    q = np.array(CAGE_START, np.float32)
    q[1] = 0.9  # the arm leans into the cage's spheres
    assert np.isfinite(q).all() and not scene.valid(q)
    return q


@pytest.fixture(scope="module")
def mixed_batch(vamp, scenes):
    """24 Panda problems in shuffled order: 14 among rotated cuboids and capsules, 4 in the empty environment, 6 in the
    sphere cage (one with its start inside an obstacle, one with a NaN in its start, one with an infinite goal joint);
    with the comparator's results and the device's"""
    problems = [Problem(scenes["mixed"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(14, 5)))]
    problems += [Problem(scenes["empty"], a, b, 7 * k) for k, (a, b) in enumerate(zip(*scenes["empty"].valid_pairs(4, 3)))]
    problems += [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, 1000 * k) for k in range(6)]
    problems[-1].start = inside_cage_obstacle(scenes["cage"])
    problems[-2].start[3] = np.nan
    problems[-3].goal[0] = np.inf
    order = np.random.default_rng(1).permutation(len(problems))
    inside, nan_start, inf_goal = (int(np.flatnonzero(order == len(problems) - j)[0]) for j in (1, 2, 3))
    problems = [problems[i] for i in order]
    s = settings_of()
    want = [p.expected(s) for p in problems]
    # the batch is what the test needs
    assert sum(w.solved and len(w.path) == 2 and w.iterations == 0 for w in want) >= 4                  # direct solutions
    assert sum(w.solved and len(w.path) >= 5 and w.iterations == s.n_samples for w in want) >= 3         # roadmap solutions
    assert sum(w.status == NO_PATH and w.questions > 1 for w in want) >= 2
    assert [want[i].status for i in (inside, nan_start, inf_goal)] == [INVALID_ENDPOINT] * 3
    assert want[inside].size[0] > 0 and want[inside].questions == 0
    return problems, want, run(vamp, problems, s)


def test_mixed_batch(mixed_batch):
    problems, want, got = mixed_batch
    check(problems, got, want)
    assert got[0].validity_calls == 2  # one call for all vertices, one for all candidate edges


def test_cage_at_1024_samples(vamp, scenes):
    """V beyond one workgroup of the neighbour search and of the shortest-path sweeps; the figures recorded for the cage"""
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, skip) for skip in (0, 5000, 1000)]
    s = settings_of(n_samples=1024, k=8)
    want = [p.expected(s) for p in problems]
    assert (want[0].status, len(want[0].path), want[0].cost, want[0].size, want[0].questions) == \
        (SOLVED, 6, f32(12.618573), [179, 357], 933)
    assert want[1].status == NO_PATH
    check(problems, run(vamp, problems, s), want)


@pytest.mark.parametrize("shape", [dict(n_samples=64, k=1), dict(n_samples=64, k=16), dict(n_samples=320, k=6),
                                   dict(n_samples=256, k=8, radius=3.0)])
def test_smallest_shapes(vamp, scenes, shape):
    """one neighbour; more neighbours asked for than valid vertices exist (14 of 66 in the cage); V = 322, no multiple of
    any tile; a radius that cuts the lists short"""
    problems = [Problem(scenes["cage"], CAGE_START, CAGE_GOAL, 0)]
    problems += [Problem(scenes["mixed"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(3, 5)))]
    problems += [Problem(scenes["empty"], a, b, 7 * k) for k, (a, b) in enumerate(zip(*scenes["empty"].valid_pairs(1, 3)))]
    s = settings_of(keep_roadmaps=True, **shape)
    want = [p.expected(s) for p in problems]
    if shape == dict(n_samples=64, k=16):
        assert want[0].size[0] == 14 and want[0].questions < 14 * 13 // 2 + 2
    if "radius" in shape:
        full = [p.expected(settings_of(**{**shape, "radius": float("inf")})) for p in problems]
        assert all(1 < w.questions < f.questions for w, f in zip(want[:4], full[:4]))  # cut short, not cut to nothing
    got = run(vamp, problems, s)
    check(problems, got, want)
    for g, w in zip(got, want):
        check_roadmap(g, w)


def lattice_samples(with_nan):
    """a 4 x 4 x 4 lattice of exactly representable values on joints 0, 2, 4, the other joints at the cage start's values:
    ties everywhere; sample 1 is a copy of sample 0, sample 2 a copy of the start; optionally a row with a NaN"""
    vals = np.array([-0.5, 0.0, 0.5, 1.0], f32)
    grid = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    samples = np.repeat(np.array(CAGE_START, f32)[None], 64, 0)
    samples[:, 0], samples[:, 2], samples[:, 4] = grid[:, 0], grid[:, 1], grid[:, 2]
    samples[1] = samples[0]
    samples[2] = np.array(CAGE_START, f32)
    if with_nan:
        samples[37, 3] = np.nan
    return samples


@pytest.mark.parametrize("k, candidates", [(3, 154), (6, 249), (16, 665)])
def test_ties_and_duplicates(vamp, scenes, k, candidates):
    problems = [Problem(scenes[kind], CAGE_START, CAGE_GOAL, samples=lattice_samples(with_nan))
                for kind in ("empty", "cage") for with_nan in (False, True)]
    s = settings_of(n_samples=64, k=k, keep_roadmaps=True)
    want = [p.expected(s) for p in problems]
    # in the empty environment every vertex is valid but the NaN row, and the direct edge is valid
    assert (want[0].size[0], want[0].questions, bool(want[0].edge_valid[0])) == (66, candidates, True)
    assert want[1].size[0] == 65 and want[1].questions < candidates
    assert 2 < want[2].size[0] < 66 and not want[2].edge_valid[0]
    got = run(vamp, problems, s)
    check(problems, got, want)
    for g, w in zip(got, want):
        check_roadmap(g, w)


def test_independence(vamp, mixed_batch):
    """a problem's result depends on nothing but its own inputs: not on the batch, its order or its size; the batch's
    problems share three environments, so handles repeat throughout"""
    problems, want, got = mixed_batch
    base = [key(g) for g in got]
    s = settings_of()
    assert [key(g) for g in run(vamp, problems[::-1], s)][::-1] == base
    for i in range(len(problems)):  # every problem alone: one problem, its endpoints' segment alone in its validity word
        assert key(run(vamp, [problems[i]], s)[0]) == base[i], i
    assert [key(g) for g in run(vamp, problems * 2, s)] == base * 2  # the same problems and handles twice in one call


def test_more_problems_than_one_launch_holds(vamp, scenes):
    """40,000 problems of 64 samples: the per-problem kernels are launched in chunks of 32,768 workgroups, and a problem
    beyond the first chunk gets what it gets in a call of four (which is compared with the comparator)"""
    four = [Problem(scenes["mixed"], a, b, 100 * k) for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(3, 5)))]
    four.append(Problem(scenes["cage"], inside_cage_obstacle(scenes["cage"]), CAGE_GOAL, 0))
    s = settings_of(n_samples=64, k=2)
    want = [p.expected(s) for p in four]
    assert {w.status for w in want} >= {INVALID_ENDPOINT} and any(w.questions > 1 for w in want)
    base = run(vamp, four, s)
    check(four, base, want)
    many = run(vamp, four * 10000, s)
    keys = [key(g) for g in base]
    assert all(key(many[i]) == keys[i % 4] for i in (0, 1, 2, 3, 32766, 32767, 32768, 32769, 32770, 32771, 39996, 39997, 39998, 39999))
    assert [(g.status, g.iterations, g.size, g.edges_checked, len(g.path)) for g in many] == \
        [(g.status, g.iterations, g.size, g.edges_checked, len(g.path)) for g in base] * 10000


@pytest.mark.parametrize("robot", ["ur5", "fetch", "baxter"])
def test_other_dimensions(vamp, oracle, robot):
    """6, 8 and 14 joints (the padded 8- and 16-joint instances of the neighbour kernel), four problems each, endpoints
    valid by the oracle; Fetch's first problem runs against a point cloud"""
    scene = Scene(oracle, robot, "mixed")
    problems = [Problem(scene, a, b, 100 * k) for k, (a, b) in enumerate(zip(*scene.valid_pairs(4, 5)))]
    if robot == "fetch":
        cloud = Scene(oracle, robot, "capt")
        a, b = cloud.valid_pairs(4, 5)
        problems[0] = Problem(cloud, a[2], b[2], 200)
    s = settings_of(n_samples=128, k=4)
    want = [p.expected(s) for p in problems]
    assert any(w.solved and len(w.path) >= 4 for w in want) and any(w.questions > 1 for w in want)
    check(problems, run(vamp, problems, s), want)


@pytest.mark.parametrize("max_samples, n_samples", [(300, 256), (10, 64)])
def test_reference_shaped_settings(vamp, scenes, max_samples, n_samples):
    """<robot>.prm_multi: n_samples = min(max_samples, 2048) rounded down to a multiple of 64, at least 64; k =
    min(max_neighbors(n_samples), 16)"""
    settings = vamp.PRMSettings(vamp.PRMNeighborParams(7, vamp.panda.space_measure()))
    settings.max_samples = max_samples
    k = min(settings.max_neighbors(n_samples), 16)
    assert k == 16 if n_samples == 256 else 1 <= k <= 16
    problems = [Problem(scenes["mixed"], a, b, 100 * j) for j, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(3, 5)))]
    want = [p.expected(settings_of(n_samples=n_samples, k=k)) for p in problems]
    got = vamp.panda.prm_multi(np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                               [p.scene.env for p in problems], settings, [p.skip for p in problems])
    for g, w, p in zip(got, want, problems):
        assert (STATUS[g.status], g.iterations, g.size, f32(g.cost).tobytes()) == (w.status, w.iterations, w.size, w.cost.tobytes())
        assert [q.tobytes() for q in g.path] == [q.tobytes() for q in w.path]
        assert isinstance(g.path, vamp.panda.Path) and (not w.solved or g.path.validate(p.scene.env))


def test_plans_summary_totals(vamp, mixed_batch, scenes):
    """rounds = validation calls made, questions = candidate edges asked; a call whose endpoints are all invalid asks none"""
    problems, want, _ = mixed_batch
    s = settings_of()
    raw = vamp.panda.prm_multi_raw(np.stack([p.start for p in problems]), np.stack([p.goal for p in problems]),
                                   [p.scene.env for p in problems], s, [p.skip for p in problems])
    assert raw["rounds"] == 2 and raw["questions"] == int(raw["candidate_edges"].sum()) == sum(w.questions for w in want)
    assert raw["sizes"].tolist() == [w.size for w in want]
    assert raw["path_lengths"].tolist() == [len(w.path) for w in want] and len(raw["paths"]) == sum(len(w.path) for w in want)
    bad = inside_cage_obstacle(scenes["cage"])
    raw = vamp.panda.prm_multi_raw(np.stack([bad, bad]), np.stack([CAGE_GOAL, CAGE_GOAL]).astype(f32), [scenes["cage"].env] * 2, s)
    assert raw["status"].tolist() == [INVALID_ENDPOINT] * 2 and (raw["rounds"], raw["questions"]) == (1, 0)
    assert raw["sizes"][:, 1].tolist() == [0, 0] and raw["sizes"][0, 0] == raw["sizes"][1, 0] > 0 and np.isinf(raw["costs"]).all()


def test_paths_go_straight_into_simplify_multi(vamp, mixed_batch):
    from vamp_mvt_amd import planning

    problems, want, got = mixed_batch
    solved = [i for i, w in enumerate(want) if w.solved and len(w.path) >= 5]
    assert len(solved) >= 3
    shortcut = planning.SimplifyMultiSettings(operations=["SHORTCUT"])  # (every edge shortcut keeps was asked: valid results)
    out = planning.simplify_multi(vamp.panda, [got[i].path for i in solved], [problems[i].scene.env for i in solved], shortcut)
    for i, r in zip(solved, out):
        p = problems[i]
        assert r.status == "ok" and 2 <= len(r.path) <= len(got[i].path) and r.cost <= got[i].cost
        assert r.path[0].tobytes() == p.start.tobytes() and r.path[-1].tobytes() == p.goal.tobytes()
        assert all(p.scene.question(a, b) for a, b in zip(r.path[:-1], r.path[1:]))
