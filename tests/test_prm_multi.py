"""vmv_prm_multi / planning.prm_multi: what holds without a device — the ABI surface, the checks that come before any
device query, the accessors' refusals, the Python wrapper's argument checks, and the serial comparator's own properties
(the contract of DESIGN §5e restated in tests/prm_serial.py) on random graphs, lattices and the sphere cage.

Two groups.  The tests down to test_python_checks_its_arguments_before_any_library_call pin the LIBRARY and the package:
they fail where vmv_prm_multi does not exist.  The tests below "the comparator's own properties" pin the COMPARATOR
alone, the yardstick the device tests compare against: they never touch the library and pass without it."""
import ctypes

import numpy as np
import pytest

import prm_serial as ps
from oracle_lib import CAGE_GOAL, CAGE_START, SPHERE_CAGE

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 5, 6
NAMES = ("vmv_prm_multi", "vmv_plans_roadmap_summary", "vmv_plans_roadmap_vertices", "vmv_plans_roadmap_edges")
SENTINEL = 0x5A5A5A5A
f32 = np.float32


def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in names and hasattr(dll, name)
        assert getattr(_lib.lib, name).argtypes is not None  # the _lib.py table has the entry
    assert vamp.abi_version() == 1  # the change is additive
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert "VMV_PLAN_NO_PATH = 3" in text and "VMV_PLAN_INVALID_ENDPOINT = 4" in text
    from vamp_mvt_amd import planning

    assert planning.PLAN_STATUS[3:5] == ("no_path", "invalid_endpoint")
    assert planning.PLAN_STATUS[:3] == ("solved", "max_iterations", "max_samples")
    s = planning.PRMMultiSettings()
    assert (s.n_samples, s.k, s.radius, s.keep_roadmaps) == (2048, 8, float("inf"), False)
    for robot in (vamp.panda, vamp.ur5, vamp.fetch, vamp.baxter):
        assert callable(robot.prm_multi) and callable(robot.prm_multi_raw)


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
    """one vmv_prm_multi call with two problems; `drop` names the pointers passed as NULL -> (status, *out)"""
    n = len(handles) if n is None else n
    a = np.zeros((max(len(handles), 1), 7), np.float32)
    b = np.full((max(len(handles), 1), 7), 0.5, np.float32)
    s = dict(n_samples=64, k=4, radius=float("inf"), keep_roadmaps=0)
    s.update(settings)
    cs = _lib.PrmSettings(s["n_samples"], s["k"], s["radius"], s["keep_roadmaps"])
    out = ctypes.c_void_p(SENTINEL)
    sk = None if skips is None else np.ascontiguousarray(skips, np.uint64)
    sm = np.zeros((max(len(handles), 1), min(s["n_samples"], 8192), 7), np.float32) if samples else None
    ptr = {"envs": (ctypes.c_void_p * max(len(handles), 1))(*handles), "starts": a.ctypes.data_as(_lib.c_float_p),
           "goals": b.ctypes.data_as(_lib.c_float_p), "settings": ctypes.byref(cs), "out": ctypes.byref(out)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_prm_multi(robot, ptr["envs"], n, ptr["starts"], ptr["goals"],
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
                                      dict(n_samples=8192), dict(n_samples=1 << 20), dict(k=0), dict(k=17),
                                      dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
                                      dict(radius=float("-inf"))])
def test_bad_settings(raw, settings):
    _lib, handles = raw
    assert _call(_lib, handles, **settings) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)


@pytest.mark.parametrize("settings", [dict(n_samples=64, k=1), dict(n_samples=8128, k=16), dict(radius=1e-3),
                                      dict(radius=float("inf")), dict(keep_roadmaps=1)])
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


def test_edge_batch_limit(raw):
    """n_problems * (n_samples + 2) * k stays below 2^31 (no array is read)"""
    _lib, handles = raw
    assert _call(_lib, handles, n=1 << 31) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    h = [handles[0]] * 16512  # 16,512 * 8,130 * 16 = 2^31 + 393,216
    assert _call(_lib, h, n_samples=8128, k=16) == (VMV_ERR_INVALID_ARGUMENT, SENTINEL)
    assert _call(_lib, h[:16508], n_samples=8128, k=16) == (VMV_ERR_NOT_FINALIZED, SENTINEL)  # 2^31 - 127,104


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
    assert L.vmv_plans_roadmap_summary(plans, None, None, None, None) == VMV_OK
    flag, n = ctypes.c_uint8(0), ctypes.c_size_t(7)
    assert L.vmv_plans_roadmap_vertices(plans, 0, ctypes.byref(flag)) == VMV_ERR_INVALID_ARGUMENT  # no problem 0, not kept
    assert L.vmv_plans_roadmap_edges(plans, 0, None, None, 0, ctypes.byref(n)) == VMV_ERR_INVALID_ARGUMENT and n.value == 7
    assert L.vmv_plans_destroy(plans) == VMV_OK
    assert L.vmv_plans_roadmap_summary(None, None, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_roadmap_vertices(None, 0, ctypes.byref(flag)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_roadmap_edges(None, 0, None, None, 0, ctypes.byref(n)) == VMV_ERR_INVALID_ARGUMENT
    empty = np.zeros((0, 7), np.float32)
    assert planning.prm_multi(vamp.panda, empty, empty, []) == []
    assert vamp.panda.prm_multi(empty, empty, [], vamp.PRMSettings(vamp.PRMNeighborParams(7, 1.0))) == []


def test_accessors_refuse_plans_of_another_origin(vamp):
    """an rrtc_multi result has no roadmap: the three accessors say so and write nothing"""
    from vamp_mvt_amd import _lib

    L = _lib.lib
    cs = _lib.RrtcSettings(1.0, 1, 1.0, 10, 64, 0)
    plans = ctypes.c_void_p()
    assert L.vmv_rrtc_multi(0, None, 0, None, None, None, ctypes.byref(cs), ctypes.byref(plans)) == VMV_OK
    counts = np.full(4, 7, np.uint32)
    assert L.vmv_plans_roadmap_summary(plans, counts.ctypes.data_as(_lib.c_u32_p), None, None, None) == VMV_ERR_INVALID_ARGUMENT
    flag, n = ctypes.c_uint8(9), ctypes.c_size_t(7)
    assert L.vmv_plans_roadmap_vertices(plans, 0, ctypes.byref(flag)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_plans_roadmap_edges(plans, 0, None, None, 0, ctypes.byref(n)) == VMV_ERR_INVALID_ARGUMENT
    assert (counts == 7).all() and flag.value == 9 and n.value == 7
    assert L.vmv_plans_destroy(plans) == VMV_OK


def test_well_formed_call_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    from vamp_mvt_amd import planning

    with pytest.raises(vamp.VmvError) as ei:
        planning.prm_multi(vamp.panda, [CAGE_START], [CAGE_GOAL], [None], planning.PRMMultiSettings(n_samples=64))
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
    S = planning.PRMMultiSettings

    def f(*args, **kw):
        return planning.prm_multi(vamp.panda, *args, **kw)

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
    for bad in (S(n_samples=100), S(n_samples=0), S(n_samples=8192), S(k=0), S(k=17), S(radius=0.0), S(radius=float("nan")),
                S(radius=-2.0)):
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
        vamp.panda.prm_multi(a, b, [env, None], vamp.PRMSettings(vamp.PRMNeighborParams(7, 1.0)))  # the installed name too
    assert env._handle is None  # nothing was built or finalized


# ---- the comparator's own properties ---------------------------------------------------------------------------------
def _random_graph(rng, n_vertices, n_edges, lattice_weights, connected=False):
    chain = [0, *range(2, n_vertices), 1]  # 0 - 2 - 3 - ... - 1: every vertex is reached, the goal last
    pairs = {(min(a, b), max(a, b)) for a, b in zip(chain[:-1], chain[1:])} if connected else set()
    while len(pairs) < n_edges:
        a, b = (int(x) for x in rng.integers(0, n_vertices, 2))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    edges = sorted(pairs)
    if lattice_weights:  # many equal path sums: ties everywhere
        w = rng.choice(np.array([0.5, 1.0, 1.5], f32), len(edges))
    else:
        w = rng.uniform(0.01, 3.0, len(edges)).astype(f32)
    return edges, [f32(x) for x in w]


@pytest.mark.parametrize("seed", range(6))
def test_heap_dijkstra_equals_the_sweep_fixpoint_in_any_order(seed):
    rng = np.random.default_rng(seed)
    n = 40
    edges, w = _random_graph(rng, n, 30 if seed == 5 else 90, lattice_weights=seed % 2 == 0)  # (seed 5: not connected)
    w[3] = f32(np.inf)  # an overflowed weight relaxes nothing
    g = ps.dijkstra_f32(n, edges, w)
    assert g[0] == 0 and (seed != 5 or np.isinf(g).any())
    for order in (None, rng.permutation(len(edges)), range(len(edges) - 1, -1, -1)):
        assert ps.sweep_fixpoint_f32(n, edges, w, order).tobytes() == g.tobytes()
    for (a, b), x in zip(edges, w):  # a fixpoint: no edge relaxes anything
        if np.isfinite(x):
            assert not f32(g[a] + x) < g[b] and not f32(g[b] + x) < g[a]


@pytest.mark.parametrize("seed", range(6))
def test_parent_rule_reproduces_the_cost_as_the_left_to_right_sum(seed):
    rng = np.random.default_rng(100 + seed)
    n = 40
    edges, w = _random_graph(rng, n, 100, lattice_weights=seed % 2 == 0, connected=True)
    g = ps.dijkstra_f32(n, edges, w)
    assert np.isfinite(g[1])
    ids = ps.parent_walk(g, edges, w)
    assert ids[0] == 0 and ids[-1] == 1 and len(set(ids)) == len(ids) <= n
    weight = {e: x for e, x in zip(edges, w)}
    total = f32(0)
    for a, b in zip(ids[:-1], ids[1:]):
        total = f32(total + weight[(min(a, b), max(a, b))])
        assert total == g[b]
    assert total == g[1]


def _lattice(dim=3):
    vals = np.array([-0.5, 0.0, 0.5, 1.0], f32)
    grid = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(grid[:, :dim])


@pytest.mark.parametrize("k", [1, 3, 6, 16])
def test_candidate_list_holds_every_pair_once(k):
    """ties everywhere (a lattice), a duplicate, invalid vertices: every unordered neighbour pair is listed once, in order"""
    rng = np.random.default_rng(k)
    verts = np.vstack([[[0.25, 0.25, 0.25]], [[0.75, 0.5, 0.25]], _lattice()]).astype(f32)
    verts[5] = verts[4]  # a duplicate: never its twin's neighbour
    valid = rng.random(len(verts)) < 0.8
    valid[:2] = True
    nbr = ps.neighbours(verts, valid, k, np.inf)
    edges = ps.candidate_edges(nbr)
    assert edges[0] == (0, 1) and len(set(edges)) == len(edges) and all(a < b for a, b in edges)
    want = {(min(v, u), max(v, u)) for v, lst in enumerate(nbr) for u in lst} | {(0, 1)}
    assert set(edges) == want
    for v, lst in enumerate(nbr):
        assert len(lst) <= k and (valid[v] or lst == []) and v not in lst
        assert all(valid[u] for u in lst) and not (v < 2 and any(u < 2 for u in lst))
        d2 = ps.dist2(verts, v)
        assert all(d2[u] > 0 for u in lst)
        keys = [(float(d2[u]), u) for u in lst]
        assert keys == sorted(keys)
        others = [(float(d2[u]), u) for u in range(len(verts))
                  if valid[u] and u != v and d2[u] > 0 and not (v < 2 and u < 2)]
        assert not valid[v] or keys == sorted(others)[:k]
    assert (4 not in nbr[5]) and (5 not in nbr[4])


def test_radius_cuts_the_lists():
    verts = np.vstack([[[0.25, 0.25, 0.25]], [[0.75, 0.5, 0.25]], _lattice()]).astype(f32)
    valid = np.ones(len(verts), bool)
    nbr = ps.neighbours(verts, valid, 16, 0.5)  # lattice neighbours at exactly 0.5 are kept (d2 <= R2)
    assert nbr[2] == [3, 6, 18] and max(len(x) for x in nbr) <= 8
    assert all(ps.dist2(verts, v)[u] <= f32(0.25) for v, lst in enumerate(nbr) for u in lst)


@pytest.fixture(scope="module")
def cage(oracle):
    env = oracle.env()
    for c in SPHERE_CAGE:
        env.add_sphere(*c, 0.2)
    rid = oracle.robot("panda")
    lower, span = oracle.bounds(rid)
    return rid, env, lower, span


# n_samples, skip, k -> status, waypoints, cost, valid vertices, candidate edges, valid edges (None = not recorded)
CAGE_FIGURES = [
    (1024, 0, 8, ps.SOLVED, 6, 12.618573, 179, 933, 357),
    (1024, 5000, 8, ps.NO_PATH, 0, np.inf, None, None, None),
    (512, 0, 8, ps.NO_PATH, 0, np.inf, None, None, None),
    (64, 0, 16, ps.NO_PATH, 0, np.inf, 14, None, None),
]


@pytest.mark.parametrize("n_samples, skip, k, status, waypoints, cost, vertices, candidates, valid_edges", CAGE_FIGURES)
def test_comparator_figures_on_the_sphere_cage(oracle, cage, n_samples, skip, k, status, waypoints, cost, vertices, candidates,
                                               valid_edges):
    rid, env, lower, span = cage
    r = ps.prm_serial(CAGE_START, CAGE_GOAL, ps.halton_samples(skip, n_samples, lower, span),
                      lambda q: oracle.validate(rid, env, q), lambda a, b: oracle.validate_motion(rid, env, a, b), k=k)
    assert (r.status, len(r.path), r.cost, r.iterations) == (status, waypoints, f32(cost), n_samples)
    assert vertices is None or r.size[0] == vertices
    assert candidates is None or (r.questions, r.size[1]) == (candidates, valid_edges)
    assert r.questions == len(r.pairs) == len(r.edge_valid) and r.size[1] == int(r.edge_valid.sum())
    if status == ps.SOLVED:
        assert r.path[0].tobytes() == np.array(CAGE_START, f32).tobytes()
        assert r.path[-1].tobytes() == np.array(CAGE_GOAL, f32).tobytes()
        assert all(oracle.validate_motion(rid, env, a, b) for a, b in zip(r.path[:-1], r.path[1:]))
        p = np.stack(r.path)
        total = f32(0)
        for a, b in zip(p[:-1], p[1:]):
            total = f32(total + np.sqrt(ps.dist2(np.stack([a, b]), 0)[1]))
        assert total == r.cost


def test_comparator_endpoints(oracle, cage):
    rid, env, lower, span = cage
    samples = ps.halton_samples(0, 64, lower, span)
    valid, question = (lambda q: oracle.validate(rid, env, q)), (lambda a, b: oracle.validate_motion(rid, env, a, b))
    inside = np.array(CAGE_START, f32)
    inside[1] = 0.9  # the arm leans into the cage's spheres
    assert not valid(inside)
    for start in (inside, np.array([np.nan] + CAGE_START[1:], f32)):
        r = ps.prm_serial(start, CAGE_GOAL, samples, valid, question, k=4)
        assert (r.status, r.path, r.questions, r.iterations, r.size[1]) == (ps.INVALID_ENDPOINT, [], 0, 0, 0) and np.isinf(r.cost)
    near = (np.array(CAGE_START, f32) + f32(0.01)).astype(f32)
    r = ps.prm_serial(CAGE_START, near, samples, valid, question, k=4)
    assert (r.status, len(r.path), r.iterations) == (ps.SOLVED, 2, 0) and bool(r.edge_valid[0])
    assert r.cost == np.sqrt(ps.dist2(np.stack([np.array(CAGE_START, f32), near]), 0)[1])


def test_comparator_does_not_import_the_package_planner():
    import os

    with open(os.path.abspath(ps.__file__)) as f:
        text = f.read()
    assert "import vamp_mvt_amd" not in text and "from vamp_mvt_amd" not in text  # neither the planner nor the library
