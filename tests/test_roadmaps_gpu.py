"""planning.build_roadmaps / DeviceRoadmaps.query on the device against the serial comparator (tests/roadmap_serial.py)
with the CPU oracle answering every question.  Every assertion is bit for bit: the kept roadmaps pair by pair and flag
by flag, and per query the status, the iterations, the valid connection edges, the questions asked, the cost's bits and
every waypoint's bits; every returned path runs from its start to its goal and is valid under the oracle edge by edge.
The roadmaps and queries are picked on the CPU."""
import numpy as np
import pytest

from oracle_lib import CAGE_GOAL, CAGE_START
from roadmap_serial import INVALID_ENDPOINT, NO_PATH, SOLVED, build_serial, halton_samples, query_serial
from test_prm_multi_gpu import STATUS, Scene, inside_cage_obstacle, lattice_samples

pytestmark = pytest.mark.gpu
f32 = np.float32


class Map:
    """one roadmap to build: a scene and its samples (the Halton samples after `skip`, or the caller's)"""

    def __init__(self, scene, skip=0, samples=None):
        self.scene, self.skip, self.samples = scene, int(skip), samples
        self._want = {}

    def expected(self, s):
        key = (s.n_samples, s.k, s.radius)
        if key not in self._want:  # the comparator's roadmap is computed once and never changed
            samples = self.samples if self.samples is not None else halton_samples(self.skip, s.n_samples, self.scene.lower,
                                                                                   self.scene.span)
            self._want[key] = build_serial(samples, self.scene.valid, self.scene.question, k=s.k, radius=s.radius)
        return self._want[key]


class Query:
    def __init__(self, m, start, goal):
        self.map = m
        self.start, self.goal = np.array(start, np.float32), np.array(goal, np.float32)
        self._want = {}

    def expected(self, s, q):
        key = (s.n_samples, s.k, s.radius, q.k_connect, q.radius)
        if key not in self._want:
            self._want[key] = query_serial(self.map.expected(s), self.start, self.goal, self.map.scene.valid,
                                           self.map.scene.question, k_connect=q.k_connect, radius=q.radius)
        return self._want[key]


def settings_of(**kw):
    from vamp_mvt_amd import planning

    s = dict(n_samples=256, k=6, radius=float("inf"))
    s.update(kw)
    return planning.RoadmapsSettings(**s)


def query_settings_of(**kw):
    from vamp_mvt_amd import planning

    return planning.RoadmapQuerySettings(**kw)


def build(vamp, maps, settings):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, maps[0].scene.robot)
    samples = None if maps[0].samples is None else np.stack([m.samples for m in maps])
    return planning.build_roadmaps(robot, [m.scene.env for m in maps], settings, [m.skip for m in maps], samples)


def ask(handle, maps, queries, q):
    if not queries:
        return []
    index = [next(i for i, m in enumerate(maps) if m is x.map) for x in queries]
    return handle.query(np.stack([x.start for x in queries]), np.stack([x.goal for x in queries]), index, q)


def key(result):
    """everything a query returns, in bits: status, iterations, valid connection edges, questions, cost, waypoints"""
    questions = result.questions if hasattr(result, "questions") else result.edges_checked
    return (result.status if isinstance(result.status, int) else STATUS[result.status], int(result.iterations),
            [int(x) for x in result.size], int(questions), f32(result.cost).tobytes(),
            [np.asarray(p, np.float32).tobytes() for p in result.path])


def check(queries, got, want):
    assert len(got) == len(want) == len(queries)
    for i, (x, g, w) in enumerate(zip(queries, got, want)):
        assert key(g) == key(w), (i, x.map.scene.kind, key(g)[:4], key(w)[:4], float(g.cost), float(w.cost))
        if w.solved:
            assert g.path[0].tobytes() == x.start.tobytes() and g.path[-1].tobytes() == x.goal.tobytes()
            assert all(x.map.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), i
        else:
            assert len(g.path) == 0 and np.isinf(g.cost)


def check_roadmaps(handle, maps, s):
    """the kept roadmaps: samples, vertex flags and the whole candidate list, pair by pair and flag by flag"""
    vertices, candidates, valid_edges = handle.summary()
    for r, m in enumerate(maps):
        w = m.expected(s)
        samples, vertex, pairs, flags = handle.roadmap(r)
        assert samples.tobytes() == np.ascontiguousarray(w.samples, np.float32).tobytes()
        assert vertex.tolist() == w.vertex_valid.tolist()
        assert pairs.tolist() == w.pairs.tolist()
        assert flags.tolist() == w.edge_valid.tolist()
        assert (int(vertices[r]), int(candidates[r]), int(valid_edges[r])) == \
            (int(w.vertex_valid.sum()), len(w.pairs), int(w.edge_valid.sum()))


def run(vamp, maps, queries, s, q, roadmaps_too=True):
    """build, compare the kept roadmaps, query, compare -> the device's results"""
    with build(vamp, maps, s) as handle:
        if roadmaps_too:
            check_roadmaps(handle, maps, s)
        got = ask(handle, maps, queries, q)
    check(queries, got, [x.expected(s, q) for x in queries])
    return got


@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "empty", "mixed")}  # mixed: rotated cuboids and capsules


def invalid_configuration(scene, seed):
    """a uniform configuration with finite joints that the oracle rejects"""
    rng = np.random.default_rng(seed)
    q = (scene.lower + scene.span * rng.random((256, len(scene.lower)), dtype=np.float32)).astype(np.float32)
    return q[~scene.o.validate_batch(scene.rid, scene.oenv, q)][0]


def mixed_maps_and_queries(scenes):
    """three roadmaps (cage, mixed, empty) and 24 queries over them in shuffled order: 6 in the cage (one with its start
    inside an obstacle, one with a NaN in its start, one with an infinite goal joint), 14 among rotated cuboids and
    capsules, 4 in the empty environment -> (maps, queries, the positions of the three invalid ones)"""
    maps = [Map(scenes["cage"], 0), Map(scenes["mixed"], 100), Map(scenes["empty"], 7)]
    queries = [Query(maps[0], CAGE_START, CAGE_GOAL)] + [Query(maps[0], a, b) for a, b in zip(*scenes["cage"].valid_pairs(5, 11))]
    queries += [Query(maps[1], a, b) for a, b in zip(*scenes["mixed"].valid_pairs(14, 5))]
    queries += [Query(maps[2], a, b) for a, b in zip(*scenes["empty"].valid_pairs(4, 3))]
    queries[3].start = inside_cage_obstacle(scenes["cage"])
    queries[4].start[3] = np.nan
    queries[5].goal[0] = np.inf
    order = np.random.default_rng(1).permutation(len(queries))
    invalid = [int(np.flatnonzero(order == j)[0]) for j in (3, 4, 5)]
    return maps, [queries[i] for i in order], invalid


@pytest.fixture(scope="module")
def mixed(vamp, scenes):
    """the mixed batch with the comparator's results, the handle (kept open for the module) and the device's results"""
    maps, queries, invalid = mixed_maps_and_queries(scenes)
    s, q = settings_of(), query_settings_of()
    want = [x.expected(s, q) for x in queries]
    # the batch is what the test needs
    assert sum(w.solved and len(w.path) == 2 and w.iterations == 0 for w in want) >= 4                  # direct solutions
    assert sum(w.solved and len(w.path) >= 4 and w.iterations == s.n_samples for w in want) >= 3         # through the roadmap
    assert sum(w.status == NO_PATH and w.questions > 1 for w in want) >= 2
    assert [want[i].status for i in invalid] == [INVALID_ENDPOINT] * 3 and all(want[i].questions == 0 for i in invalid)
    handle = build(vamp, maps, s)
    yield maps, queries, want, handle, ask(handle, maps, queries, q)
    handle.close()


def test_mixed_build_and_query(mixed):
    maps, queries, want, handle, got = mixed
    assert len(handle) == 3
    check_roadmaps(handle, maps, settings_of())
    check(queries, got, want)
    assert got[0].validity_calls == 2  # one call for all endpoints, one for all questions


def test_a_roadmap_without_queries_and_invalid_endpoints_alone(mixed):
    """a call that leaves the mixed roadmap out gives the others' queries what they got; a call of invalid endpoints
    alone makes one counted validation call and asks nothing"""
    maps, queries, want, handle, got = mixed
    some = [i for i, x in enumerate(queries) if x.map is not maps[1]]
    assert 0 < len(some) < len(queries)
    again = ask(handle, maps, [queries[i] for i in some], query_settings_of())
    assert [key(g) for g in again] == [key(got[i]) for i in some]
    bad = [x for x, w in zip(queries, want) if w.status == INVALID_ENDPOINT]
    out = ask(handle, maps, bad, query_settings_of())
    assert [STATUS[g.status] for g in out] == [INVALID_ENDPOINT] * 3 and out[0].validity_calls == 1
    assert all((g.size, g.edges_checked, g.iterations, len(g.path)) == ([0, 0], 0, 0, 0) and np.isinf(g.cost) for g in out)


@pytest.mark.parametrize("shape", [dict(n_samples=64, k=1), dict(n_samples=64, k=16), dict(n_samples=320, k=6),
                                   dict(n_samples=256, k=8, radius=3.0)])
def test_smallest_build_shapes(vamp, scenes, shape):
    """one neighbour; more neighbours asked for than valid samples exist (12 of 64 in the cage); 320 samples, no multiple
    of a 256 tile; a radius that cuts the lists short"""
    maps = [Map(scenes["cage"], 0), Map(scenes["mixed"], 100), Map(scenes["empty"], 7)]
    queries = [Query(maps[0], CAGE_START, CAGE_GOAL)] + [Query(maps[1], a, b) for a, b in zip(*scenes["mixed"].valid_pairs(3, 5))]
    queries += [Query(maps[2], a, b) for a, b in zip(*scenes["empty"].valid_pairs(1, 3))]
    s = settings_of(**shape)
    if shape == dict(n_samples=64, k=16):
        w = maps[0].expected(s)
        assert int(w.vertex_valid.sum()) == 12 and len(w.pairs) == 12 * 11 // 2  # every pair of the 12, once
    if "radius" in shape:
        full = [m.expected(settings_of(**{**shape, "radius": float("inf")})) for m in maps]
        assert all(0 < len(m.expected(s).pairs) < len(f.pairs) for m, f in zip(maps, full))  # cut short, not cut to nothing
    run(vamp, maps, queries, s, query_settings_of())


@pytest.mark.parametrize("connect", [dict(k_connect=1), dict(k_connect=32), dict(k_connect=16, radius=2.5)])
def test_smallest_query_shapes(mixed, connect):
    """one connection per endpoint; 32 at 64 samples would be more than a roadmap's valid samples, and is here more than a
    query's block of 17 held before; a query radius that cuts conn short"""
    maps, queries, _, handle, _ = mixed
    s, q = settings_of(), query_settings_of(**connect)
    want = [x.expected(s, q) for x in queries]
    if "radius" in connect:
        full = [x.expected(s, query_settings_of(k_connect=16)) for x in queries]
        assert sum(1 < w.questions < f.questions for w, f in zip(want, full)) >= 6  # cut short, not cut to nothing
    check(queries, ask(handle, maps, queries, q), want)


def test_more_connections_than_valid_samples(vamp, scenes):
    """k_connect = 32 against the 12 valid samples of the cage's 64: every list ends early and the rest of the block is
    null questions"""
    maps = [Map(scenes["cage"], 0)]
    queries = [Query(maps[0], CAGE_START, CAGE_GOAL)] + [Query(maps[0], a, b) for a, b in zip(*scenes["cage"].valid_pairs(3, 11))]
    s, q = settings_of(n_samples=64, k=8), query_settings_of(k_connect=32)
    want = [x.expected(s, q) for x in queries]
    assert all(w.questions == 25 for w in want)
    run(vamp, maps, queries, s, q)


def test_cage_at_1024_samples(vamp, scenes):
    """V beyond one workgroup of the neighbour search and of the shortest-path sweeps; the figures recorded for the cage"""
    maps = [Map(scenes["cage"], 0), Map(scenes["cage"], 5000)]
    queries = [Query(m, CAGE_START, CAGE_GOAL) for m in maps]
    queries += [Query(maps[0], a, b) for a, b in zip(*scenes["cage"].valid_pairs(3, 11))]
    s, q = settings_of(n_samples=1024, k=8), query_settings_of(k_connect=8)
    w = queries[0].expected(s, q)
    assert (w.status, len(w.path), int(f32(w.cost).view(np.uint32)), w.size, w.questions) == (SOLVED, 7, 1097692643, [6, 3], 17)
    m = maps[0].expected(s)
    assert (int(m.vertex_valid.sum()), len(m.pairs), int(m.edge_valid.sum())) == (177, 914, 344)
    run(vamp, maps, queries, s, q)


@pytest.mark.parametrize("k", [3, 16])
def test_ties_and_duplicates(vamp, scenes, k):
    """the 4 x 4 x 4 lattice: ties everywhere; sample 1 is a copy of sample 0, sample 2 a copy of the queries' start
    (d2 = 0: no connection); one roadmap per scene has a row with a NaN; a query with start == goal has a direct edge of
    weight 0"""
    maps = [Map(scenes[kind], samples=lattice_samples(with_nan)) for kind in ("empty", "cage") for with_nan in (False, True)]
    queries = [Query(m, CAGE_START, CAGE_GOAL) for m in maps] + [Query(m, CAGE_START, CAGE_START) for m in maps[:3:2]]
    s, q = settings_of(n_samples=64, k=k), query_settings_of(k_connect=k)
    want = [x.expected(s, q) for x in queries]
    assert int(maps[0].expected(s).vertex_valid.sum()) == 64 and int(maps[1].expected(s).vertex_valid.sum()) == 63
    assert all(2 not in w.conn[0] for w in want[:4]) and all(len(w.conn[0]) == k for w in want[:2])
    assert want[0].solved and len(want[0].path) == 2 and not (want[2].solved and len(want[2].path) == 2)
    for w in want[4:]:
        assert (w.status, len(w.path), w.iterations) == (SOLVED, 2, 0) and w.cost == 0 and w.cost.tobytes() == f32(0).tobytes()
    run(vamp, maps, queries, s, q)


def test_a_roadmap_with_no_valid_vertex(vamp, scenes):
    """every sample is the same invalid configuration: no neighbour, no edge, no connection; queries reduce to the direct edge"""
    bad = inside_cage_obstacle(scenes["cage"])
    maps = [Map(scenes["cage"], samples=np.repeat(bad[None], 64, 0))]
    near = (np.array(CAGE_START, f32) + f32(0.01)).astype(f32)
    queries = [Query(maps[0], CAGE_START, CAGE_GOAL), Query(maps[0], CAGE_START, near), Query(maps[0], bad, CAGE_GOAL)]
    s, q = settings_of(n_samples=64, k=4), query_settings_of(k_connect=4)
    want = [x.expected(s, q) for x in queries]
    assert not maps[0].expected(s).vertex_valid.any() and len(maps[0].expected(s).pairs) == 0
    assert [(w.status, w.questions, w.size) for w in want] == [(NO_PATH, 1, [0, 0]), (SOLVED, 1, [0, 0]), (INVALID_ENDPOINT, 0, [0, 0])]
    run(vamp, maps, queries, s, q)


def test_independence_of_the_batch(mixed):
    """a query's result depends on nothing but its endpoints, its roadmap and the settings: not on the batch, its order
    or its size"""
    maps, queries, _, handle, got = mixed
    base = [key(g) for g in got]
    q = query_settings_of()
    assert [key(g) for g in ask(handle, maps, queries[::-1], q)][::-1] == base
    for i in range(len(queries)):  # every query alone
        assert key(ask(handle, maps, [queries[i]], q)[0]) == base[i], i
    assert [key(g) for g in ask(handle, maps, queries * 2, q)] == base * 2  # the same queries twice in one call


def test_independence_of_the_handle(vamp, mixed):
    """each roadmap built alone is the roadmap built with the others, and answers its queries alike"""
    maps, queries, _, _, got = mixed
    s, q = settings_of(), query_settings_of()
    for m in maps:
        mine = [i for i, x in enumerate(queries) if x.map is m]
        with build(vamp, [m], s) as alone:
            check_roadmaps(alone, [m], s)
            out = ask(alone, [m], [queries[i] for i in mine], q)
        assert [key(g) for g in out] == [key(got[i]) for i in mine]


def test_more_queries_than_one_launch_holds(vamp, scenes):
    """40,000 queries against one 64-sample roadmap: the per-query kernels are launched in chunks of 32,768 workgroups, and
    a query beyond the first chunk gets what it gets in a call of four (which is compared with the comparator)"""
    maps = [Map(scenes["mixed"], 100)]
    four = [Query(maps[0], a, b) for a, b in zip(*scenes["mixed"].valid_pairs(3, 5))]
    four.append(Query(maps[0], invalid_configuration(scenes["mixed"], 2), four[0].goal))
    s, q = settings_of(n_samples=64, k=8), query_settings_of(k_connect=8)
    want = [x.expected(s, q) for x in four]
    assert want[3].status == INVALID_ENDPOINT and any(w.solved and w.iterations for w in want[:3])
    with build(vamp, maps, s) as handle:
        base = ask(handle, maps, four, q)
        check(four, base, want)
        many = handle.query(np.tile(np.stack([x.start for x in four]), (10000, 1)),
                            np.tile(np.stack([x.goal for x in four]), (10000, 1)), None, q)
    keys = [key(g) for g in base]
    assert all(key(many[i]) == keys[i % 4] for i in (0, 1, 2, 3, 16382, 16383, 16384, 16385, 32766, 32767, 32768, 32769, 32770,
                                                     32771, 39996, 39997, 39998, 39999))
    assert [(g.status, g.iterations, g.size, g.edges_checked, len(g.path)) for g in many] == \
        [(g.status, g.iterations, g.size, g.edges_checked, len(g.path)) for g in base] * 10000


@pytest.mark.parametrize("robot", ["ur5", "fetch", "baxter"])
def test_other_dimensions(vamp, oracle, robot):
    """6, 8 and 14 joints (the padded 8- and 16-joint instances of both searches), four queries each, endpoints valid by
    the oracle; Fetch's second roadmap is built against a point cloud"""
    scene = Scene(oracle, robot, "mixed")
    maps = [Map(scene, 100)]
    queries = [Query(maps[0], a, b) for a, b in zip(*scene.valid_pairs(4, 5))]
    if robot == "fetch":
        cloud = Scene(oracle, robot, "capt")
        maps.append(Map(cloud, 200))
        a, b = cloud.valid_pairs(4, 5)
        queries[0] = Query(maps[1], a[2], b[2])
    s, q = settings_of(n_samples=128, k=4), query_settings_of(k_connect=4)
    want = [x.expected(s, q) for x in queries]
    assert any(w.questions > 1 for w in want)
    run(vamp, maps, queries, s, q)


def test_handle_lifetime(vamp, scenes, mixed):
    """the same handle asked twice answers alike; after close() a fresh build works and answers alike; a handle whose
    environment changed refuses the query"""
    maps, queries, _, handle, got = mixed
    s, q = settings_of(), query_settings_of()
    base = [key(g) for g in got]
    assert [key(g) for g in ask(handle, maps, queries, q)] == base
    other = build(vamp, maps, s)
    other.close()
    with pytest.raises(ValueError):
        ask(other, maps, queries, q)
    with build(vamp, maps, s) as fresh:
        assert [key(g) for g in ask(fresh, maps, queries, q)] == base
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    with vamp.panda.build_roadmaps([env], settings_of(n_samples=64)) as mine:
        assert len(mine.query(queries[0].start[None], queries[0].goal[None])) == 1
        env.add_sphere(vamp.Sphere([0.5, 0.3, 0.5], 0.1))  # the environment gives up the handle the roadmap refers to
        with pytest.raises(ValueError):
            mine.query(queries[0].start[None], queries[0].goal[None])


def test_paths_go_straight_into_simplify_multi(vamp, mixed):
    from vamp_mvt_amd import planning

    maps, queries, want, _, got = mixed
    solved = [i for i, w in enumerate(want) if w.solved and len(w.path) >= 4]
    assert len(solved) >= 3
    shortcut = planning.SimplifyMultiSettings(operations=["SHORTCUT"])  # (every edge shortcut keeps was asked: valid results)
    out = planning.simplify_multi(vamp.panda, [got[i].path for i in solved], [queries[i].map.scene.env for i in solved], shortcut)
    for i, r in zip(solved, out):
        x = queries[i]
        assert r.status == "ok" and 2 <= len(r.path) <= len(got[i].path) and r.cost <= got[i].cost
        assert r.path[0].tobytes() == x.start.tobytes() and r.path[-1].tobytes() == x.goal.tobytes()
        assert all(x.map.scene.question(a, b) for a, b in zip(r.path[:-1], r.path[1:]))
