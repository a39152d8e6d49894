"""vmv_optimize_multi on the device against the serial statement (tests/optimize_serial.py in float32), with the device's
own clearance_grad_batch - pinned by its own tests - as the clearance callback and the CPU oracle answering every edge
question: per path the status, the iterations, the best iteration, both costs' bits, the four clearance minima's bits and
every waypoint's bits.  Every returned path with status OK is valid under the oracle edge by edge; every other path equals
its input's bytes.  Then the grazing case of DESIGN §5l and the Python layer."""
import numpy as np
import pytest

import envs
from optimize_cases import GRAZE_CENTRE, graze_line, graze_radius, straight
from optimize_serial import NO_VALID, NONFINITE, OK, optimize_serial
from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_serial import rrtc_serial

pytestmark = pytest.mark.gpu
KEYS = ("max_iterations", "validate_every", "step", "max_step", "min_change", "smooth_weight", "env_weight", "self_weight",
        "env_margin", "self_margin")


class Scene:
    """one environment, built alike for the product and the oracle"""

    def __init__(self, oracle, vamp, robot, kind):
        self.robot, self.kind, self.o = robot, kind, oracle
        self.module = getattr(vamp, robot)
        self.rid = oracle.robot(robot)
        self.lower, span = oracle.bounds(self.rid)
        self.upper = (self.lower + span).astype(np.float32)
        spec = envs.spec_for(kind, robot)
        self.oenv = envs.build_oracle_env(oracle, spec)
        self.env = envs.build_product_env(spec) if spec else None  # None = the empty environment

    def question(self, a, b):
        return self.o.validate_motion(self.rid, self.oenv, a, b)

    def clearance_grad(self, X):
        return self.module.clearance_grad_batch(np.ascontiguousarray(X, np.float32), self.env)

    def valid_configs(self, n, seed):
        rng = np.random.default_rng(seed)
        q = (self.lower + (self.upper - self.lower) * rng.random((64 * n, len(self.lower)), dtype=np.float32)).astype(np.float32)
        q = q[self.o.validate_batch(self.rid, self.oenv, q)][:n]
        assert len(q) == n
        return q


class Item:
    def __init__(self, scene, path, tag):
        self.scene, self.tag = scene, tag
        self.path = np.ascontiguousarray(path, np.float32).reshape(len(path), len(scene.lower))

    def expected(self, s):
        return optimize_serial(self.path, self.scene.clearance_grad, self.scene.question, self.scene.lower, self.scene.upper,
                               **{k: getattr(s, k) for k in KEYS})

    def input_is_valid(self):
        return bool(np.isfinite(self.path).all()) and all(self.scene.question(a, b) for a, b in zip(self.path[:-1], self.path[1:]))


def settings_of(**kw):
    from vamp_mvt_amd import planning

    return planning.OptimizeMultiSettings(**kw)


def run(items, s):
    """-> per item (status, iterations, best_iteration, bits of cost_first, cost, clearance_first, clearance, waypoints)"""
    raw = items[0].scene.module.optimize_multi_raw([i.path for i in items], [i.scene.env for i in items], s)
    off = raw["offsets"]
    return [(int(raw["status"][p]), int(raw["iterations"][p]), int(raw["best_iteration"][p]), raw["cost_first"][p].tobytes(),
             raw["cost"][p].tobytes(), raw["clearance_first"][p].tobytes(), raw["clearance"][p].tobytes(),
             raw["points"][off[p]:off[p + 1]].tobytes()) for p in range(len(items))]


def key_of(w):
    f = np.float32
    return (w.status, w.iterations, w.best_iteration, f(w.cost_first).tobytes(), f(w.cost).tobytes(),
            np.array(w.clearance_first, f).tobytes(), np.array(w.clearance, f).tobytes(),
            np.array(w.path, f).tobytes())


def check(items, got, want):
    assert len(got) == len(want) == len(items)
    for i, (it, g, w) in enumerate(zip(items, got, want)):
        k = key_of(w)
        assert g[:3] == k[:3], (i, it.tag, g[:3], k[:3])
        for name, a, b in zip(("cost_first", "cost", "clearance_first", "clearance"), g[3:7], k[3:7]):
            assert a == b, (i, it.tag, name, np.frombuffer(a, np.float32), np.frombuffer(b, np.float32))
        assert g[7] == k[7], (i, it.tag, "waypoints")
        path = np.frombuffer(g[7], np.float32).reshape(it.path.shape)
        if len(path):
            assert path[0].tobytes() == it.path[0].tobytes() and path[-1].tobytes() == it.path[-1].tobytes(), (i, it.tag)
        if g[0] == OK:
            assert all(it.scene.question(a, b) for a, b in zip(path[:-1], path[1:])), (i, it.tag)
            assert np.frombuffer(g[4], np.float32)[0] <= np.frombuffer(g[3], np.float32)[0]
        else:
            assert g[0] in (NO_VALID, NONFINITE) and g[7] == it.path.tobytes(), (i, it.tag)
        if it.input_is_valid():
            assert g[0] == OK, (i, it.tag)


@pytest.fixture(scope="module")
def scenes(oracle, vamp):
    return {k: Scene(oracle, vamp, "panda", k) for k in ("cage", "empty", "mixed")}  # mixed: rotated cuboids and capsules


@pytest.fixture(scope="module")
def panda_items(scenes, vamp):
    """a shuffled batch: straight lines between valid configurations at the lengths where the kernels change path (2, 3,
    4; 64, 65, 66 around a wave in the waypoint stride and the edge words; 130; max_waypoints), some of them colliding;
    raw RRT-Connect paths, densified; a NaN waypoint; none and one waypoint"""
    from vamp_mvt_amd import planning

    cage, empty, mixed = scenes["cage"], scenes["empty"], scenes["mixed"]
    qc, qm = cage.valid_configs(10, 1), mixed.valid_configs(8, 2)
    near = lambda a, b, t: (a + (b - a) * np.float32(t)).astype(np.float32)  # noqa: E731
    fa, fb = next((a, b) for a in qc for b in qc if not cage.question(a, b))  # a straight line the cage blocks
    items = [Item(cage, straight(fa, fb, 2), "cage 2 far"), Item(cage, straight(qc[0], near(qc[0], qc[1], 0.02), 2), "cage 2 near"),
             Item(cage, straight(qc[4], near(qc[4], qc[5], 0.1), 3), "cage 3"), Item(cage, straight(qc[3], near(qc[3], qc[4], 0.2), 4), "cage 4"),
             Item(cage, straight(CAGE_START, near(np.float32(CAGE_START), np.float32(CAGE_GOAL), 0.3), 64), "cage 64"),
             Item(cage, straight(qc[5], qc[6], 65), "cage 65 far"), Item(mixed, straight(qm[0], near(qm[0], qm[1], 0.4), 66), "mixed 66"),
             Item(mixed, straight(qm[2], qm[3], 130), "mixed 130 far"), Item(cage, straight(qc[7], near(qc[7], qc[8], 0.05), 1024), "cage 1024"),
             Item(empty, straight(qc[8], qc[9], 33), "empty 33"), Item(mixed, straight(qm[4], near(qm[4], qm[5], 0.3), 17), "mixed 17"),
             Item(cage, straight(qc[0], qc[1], 1), "one"), Item(cage, np.zeros((0, 7), np.float32), "none")]
    bad = straight(qc[1], near(qc[1], qc[2], 0.2), 9)
    bad[4, 3] = np.nan
    items.append(Item(cage, bad, "nan"))
    for k, (scene, a, b) in enumerate(((cage, CAGE_START, CAGE_GOAL), (mixed, qm[6], qm[7]))):
        p = rrtc_serial(a, b, scene.lower, scene.upper - scene.lower, scene.question, range_=1.0, max_iterations=3000, skip=1000 * k).path
        assert len(p) >= 3
        items.append(Item(scene, planning.densify_path(np.stack(p), 8.0), f"rrtc {scene.kind}"))
    order = np.random.default_rng(1).permutation(len(items))
    return [items[i] for i in order]


@pytest.fixture(scope="module")
def panda_runs(panda_items):
    """per validate_every: the settings, the serial statement's results, the device's"""
    out = {}
    for v in (1, 8, 100):
        s = settings_of(max_iterations=12, validate_every=v)
        out[v] = (s, [it.expected(s) for it in panda_items], run(panda_items, s))
    return out


@pytest.mark.parametrize("v", [1, 8, 100])
def test_batch_matches_the_serial_statement(panda_items, panda_runs, v):
    s, want, got = panda_runs[v]
    check(panda_items, got, want)
    by_tag = {it.tag: w for it, w in zip(panda_items, want)}
    # the batch is what the test needs: repairs or refusals among the colliding lines, improved valid ones, every status
    assert {w.status for w in want} == {OK, NO_VALID, NONFINITE}
    assert by_tag["nan"].status == NONFINITE and by_tag["one"].status == OK and by_tag["none"].status == OK
    assert by_tag["cage 2 near"].status == OK and by_tag["cage 2 far"].status == NO_VALID
    assert sum(w.status == OK and w.best_iteration > 0 for w in want) >= 4
    assert any(not it.input_is_valid() and len(it.path) > 2 for it in panda_items)
    assert any(w.iterations == 12 for w in want)


def test_reversed_alone_and_twice(panda_items, panda_runs):
    s, want, got = panda_runs[8]
    assert run(panda_items[::-1], s) == got[::-1]
    for it, g in zip(panda_items, got):
        assert run([it], s) == [g], it.tag
    assert run(panda_items + panda_items, s) == got + got


def test_paths_that_stop_early_are_compacted_away(panda_items):
    """min_change so large that the paths whose steps have become small stop at their first validated iterate, while the
    paths still being repaired or pushed by the cap run on"""
    s = settings_of(max_iterations=12, validate_every=4, min_change=0.05)
    want = [it.expected(s) for it in panda_items]
    check(panda_items, run(panda_items, s), want)
    its = {w.iterations for it, w in zip(panda_items, want) if len(it.path) > 2 and w.status != NONFINITE}
    assert 4 in its and 12 in its, its


@pytest.mark.parametrize("robot", ["ur5", "fetch", "baxter"])  # fetch: a prismatic joint, dim 8; baxter: dim 14
def test_other_robots(oracle, vamp, robot):
    scene, free = Scene(oracle, vamp, robot, "cage"), Scene(oracle, vamp, robot, "empty")
    q = scene.valid_configs(6, 4)
    near = lambda a, b, t: (a + (b - a) * np.float32(t)).astype(np.float32)  # noqa: E731
    items = [Item(scene, straight(q[0], near(q[0], q[1], 0.1), 3), "3"), Item(scene, straight(q[2], near(q[2], q[3], 0.3), 33), "33"),
             Item(scene, straight(q[4], q[5], 65), "65 far"), Item(free, straight(q[1], q[2], 20), "empty 20")]
    if robot == "baxter":  # the largest gradient a shipped robot keeps in LDS: 1,022 x 14 floats
        items.append(Item(scene, straight(q[0], near(q[0], q[1], 0.2), 1024), "1024"))
    s = settings_of(max_iterations=10, validate_every=5)
    check(items, run(items, s), [it.expected(s) for it in items])


def test_grazing_case(oracle, vamp):
    """33 waypoints on a straight line, 5 mm from one sphere; the float64 study reaches 48 - 50 mm of waypoint
    clearance for 0.4 % more path length.  Bounds: env >= 0.04 (8 mm left for fp32 and the kernels' sine), path_cost grows by
    less than 2 %."""
    from vamp_mvt_amd import planning

    X = graze_line(33)
    env_of = lambda r: envs.build_product_env([("sphere", np.array([*GRAZE_CENTRE, r], np.float32))])  # noqa: E731
    radius = np.float32(graze_radius(lambda r: vamp.panda.clearance_batch(X, env_of(r))[:, 0].min()))
    spec = [("sphere", np.array([*GRAZE_CENTRE, radius], np.float32))]
    env, oenv = envs.build_product_env(spec), envs.build_oracle_env(oracle, spec)
    rid = oracle.robot("panda")
    first = vamp.panda.clearance_batch(X, env)
    print(f"radius {radius:.6f}, input clearances env {first[:, 0].min():.6f} self {first[:, 1].min():.6f}")
    assert abs(radius - 0.0044) < 5e-4 and abs(first[:, 0].min() - 0.005) < 1e-5
    assert all(oracle.validate_motion(rid, oenv, a, b) for a, b in zip(X[:-1], X[1:]))  # the input is valid
    s = settings_of(max_iterations=64, validate_every=8, step=1.0 / 40.0, max_step=0.1, min_change=1e-4, smooth_weight=1.0,
                    env_weight=1.0, self_weight=1.0, env_margin=0.05, self_margin=0.01)
    r = planning.optimize_multi(vamp.panda, [X], [env], s)[0]
    before, after = planning.path_cost(list(X)), planning.path_cost(r.path)
    print(f"status {r.status}, iterations {r.iterations}, best {r.best_iteration}, U {r.cost_first:.6f} -> {r.cost:.6f}, "
          f"clearance {r.clearance_first} -> {r.clearance}, path_cost {before:.6f} -> {after:.6f}")
    assert r.status == "ok"
    assert r.clearance[0] >= 0.04
    assert after < 1.02 * before
    assert r.cost <= r.cost_first
    assert all(oracle.validate_motion(rid, oenv, a, b) for a, b in zip(r.path[:-1], r.path[1:]))


def test_python_layer_on_planned_and_simplified_paths(vamp):
    from vamp_mvt_amd import planning

    env = envs.build_product_env(envs.spec_for("cage", "panda"))
    plans = planning.rrtc_multi(vamp.panda, [CAGE_START] * 2, [CAGE_GOAL] * 2, [env] * 2, skips=[0, 1000])
    assert all(p.solved for p in plans)
    simple = planning.simplify_multi(vamp.panda, [p.path for p in plans], [env] * 2)
    res = 8.0
    got = planning.optimize_multi(vamp.panda, [p.path for p in simple], [env] * 2, resolution=res)
    assert [r.status for r in got] == ["ok", "ok"]
    assert planning.validate_paths(vamp.panda, [r.path for r in got], [env] * 2).all()
    for r, p in zip(got, simple):
        dense = planning.densify_path(np.stack(p.path), res)
        assert len(r.path) == len(dense) > len(p.path)
        assert r.path[0].tobytes() == p.path[0].tobytes() and r.path[-1].tobytes() == p.path[-1].tobytes()
        values = vamp.panda.clearance_batch(np.stack(r.path), env)
        assert np.float32(r.clearance[0]).tobytes() == values[:, 0].min().tobytes()
        assert np.float32(r.clearance[1]).tobytes() == values[:, 1].min().tobytes()
        first = vamp.panda.clearance_batch(dense, env)
        assert np.float32(r.clearance_first[0]).tobytes() == first[:, 0].min().tobytes()
        assert r.cost <= r.cost_first
