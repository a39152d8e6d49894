"""planning.simplify_multi on the device against the serial comparator (tests/simplify_serial.py) with the CPU oracle
answering every question: per path the status, the iterations, the length and every waypoint bit for bit; and every
returned path keeps its endpoints' bits and is valid under the oracle edge by edge.  The comparator asks one question at
a time, so equality for several questions_per_round also checks the windows.  The paths are picked on the CPU."""
import numpy as np
import pytest

import envs
from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_serial import rrtc_serial
from simplify_serial import CAPACITY, OK, simplify_serial, windowed_questions, windowed_rounds

pytestmark = pytest.mark.gpu
STATUS = {"ok": OK, "capacity": CAPACITY}


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
        rng = np.random.default_rng(seed)
        q = (self.lower + self.span * rng.random((64 * n, len(self.lower)), dtype=np.float32)).astype(np.float32)
        q = q[self.o.validate_batch(self.rid, self.oenv, q)][: 2 * n]
        assert len(q) == 2 * n
        return q[0::2], q[1::2]

    def plan(self, start, goal, skip, max_iterations=3000):
        """a raw RRT-Connect path (the serial planner of tests/rrtc_serial.py); [] if unsolved"""
        return rrtc_serial(start, goal, self.lower, self.span, self.question, range_=1.0, max_iterations=max_iterations,
                           skip=skip).path


class Item:
    """one path to simplify in one scene"""

    def __init__(self, scene, path, tag=""):
        self.scene, self.tag = scene, tag
        self.path = [np.array(q, np.float32) for q in path]

    def expected(self, s):
        return simplify_serial(self.path, self.scene.question, max_iterations=s.max_iterations, operations=tuple(s.operations),
                               max_steps=s.max_steps, min_change=s.min_change,
                               midpoint_interpolation=s.midpoint_interpolation, max_waypoints=s.max_waypoints)

    def input_is_valid(self):
        return all(self.scene.question(a, b) for a, b in zip(self.path[:-1], self.path[1:]))


def settings_of(**kw):
    from vamp_mvt_amd import planning

    return planning.SimplifyMultiSettings(**kw)


def run(vamp, items, settings=None):
    from vamp_mvt_amd import planning

    robot = getattr(vamp, items[0].scene.robot)
    return planning.simplify_multi(robot, [i.path for i in items], [i.scene.env for i in items], settings)


def key(result):
    """what must not depend on the rest of the batch or on how it is asked: status, iterations and the waypoints' bits"""
    return (result.status if isinstance(result.status, int) else STATUS[result.status], int(result.iterations),
            [np.asarray(q, np.float32).tobytes() for q in result.path])


def check(items, got, want, valid=True):
    assert len(got) == len(want) == len(items)
    for i, (it, g, w) in enumerate(zip(items, got, want)):
        assert key(g)[:2] == key(w)[:2] and len(g.path) == len(w.path), (i, it.tag, key(g)[:2], len(g.path), key(w)[:2], len(w.path))
        assert key(g)[2] == key(w)[2], (i, it.tag)
        if len(it.path) >= 1:
            assert g.path[0].tobytes() == it.path[0].tobytes() and g.path[-1].tobytes() == it.path[-1].tobytes(), (i, it.tag)
        if valid and it.input_is_valid():  # then so is what came back, edge by edge
            assert all(it.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), (i, it.tag)


@pytest.fixture(scope="module")
def scenes(oracle):
    return {k: Scene(oracle, "panda", k) for k in ("cage", "empty", "mixed")}  # mixed: rotated cuboids and capsules


@pytest.fixture(scope="module")
def cage_plans(scenes):
    return [scenes["cage"].plan(CAGE_START, CAGE_GOAL, 1000 * k) for k in range(8)]


@pytest.fixture(scope="module")
def interleaved(scenes, cage_plans):
    """raw RRT-Connect paths in shuffled order: 8 in the sphere cage, 4 of those again in the empty environment (their
    straight line is free there), the solved ones of 12 problems among rotated cuboids and capsules, 3 in the empty
    environment"""
    items = [Item(scenes["cage"], p, f"cage{k}") for k, p in enumerate(cage_plans)]
    items += [Item(scenes["empty"], p, f"cage{k} in empty") for k, p in enumerate(cage_plans[:4])]
    for k, (a, b) in enumerate(zip(*scenes["mixed"].valid_pairs(12, 5))):
        p = scenes["mixed"].plan(a, b, 100 * k)
        if len(p) >= 2:
            items.append(Item(scenes["mixed"], p, f"mixed{k}"))
    items += [Item(scenes["empty"], scenes["empty"].plan(a, b, 7 * k), f"empty{k}")
              for k, (a, b) in enumerate(zip(*scenes["empty"].valid_pairs(3, 3)))]
    order = np.random.default_rng(1).permutation(len(items))
    return [items[i] for i in order]


@pytest.fixture(scope="module")
def edge_lengths(scenes, cage_plans):
    """0, 1, 2 and 3 waypoints, and 3 waypoints whose straight line is blocked"""
    cage, p = scenes["cage"], cage_plans[0]
    three_free = Item(scenes["empty"], p[:3], "three, free")
    blocked = next(Item(cage, q[s:s + 3], "three, blocked") for q in cage_plans for s in range(len(q) - 2)
                   if not cage.question(q[s], q[s + 2]))
    return [Item(cage, [], "none"), Item(cage, p[:1], "one"), Item(cage, [p[0], p[-1]], "two, blocked"),
            Item(scenes["empty"], p[:2], "two"), three_free, blocked]


@pytest.fixture(scope="module")
def window_paths(scenes, cage_plans):
    """candidate counts size - i - 2 of 3, 4 and 5 for waypoint 0 (W - 1, W, W + 1 at 4 questions per round): the first 5,
    6 and 7 waypoints of a planned path, and a hand-built zig-zag over its first waypoints, P0 P1 P1 P2 P3 P2 P3 and its
    first 6 and 5 waypoints — from P0 only P1 can be reached, the last candidate of the scan"""
    cage = scenes["cage"]
    items = [Item(cage, cage_plans[6][:n], f"slice{n}") for n in (5, 6, 7)]
    p = cage_plans[7]
    assert not any(cage.question(p[0], p[k]) for k in (2, 3))
    zig = [p[0], p[1], p[1], p[2], p[3], p[2], p[3]]
    items += [Item(cage, zig[:n], f"zigzag{n}") for n in (5, 6, 7)]
    assert all(it.input_is_valid() for it in items)
    return items


@pytest.fixture(scope="module")
def batch(vamp, interleaved, edge_lengths, window_paths):
    """the whole batch with the comparator's results and the device's for the default settings"""
    items = interleaved + edge_lengths + window_paths
    s = settings_of()
    want = [it.expected(s) for it in items]
    tagged = {it.tag: w for it, w in zip(items, want)}
    # the batch is what the tests need
    assert len(interleaved) >= 20 and all(it.input_is_valid() for it in interleaved)
    direct = [w for it, w in zip(items, want) if len(it.path) > 2 and len(w.path) == 2 and w.questions == 1]
    assert len(direct) >= 4 and all(w.iterations == 0 for w in direct)
    assert sum(w.erased for w in want) >= 8 and sum(w.replaced for w in want) >= 8
    assert sum(w.iterations > 1 for w in want) >= 8
    assert any(it.scene.kind == "mixed" and w.replaced for it, w in zip(items, want))
    assert [len(tagged[t].path) for t in ("none", "one", "two, blocked", "two", "three, free")] == [0, 1, 2, 2, 2]
    assert [tagged[t].questions for t in ("none", "one", "two, blocked", "two", "three, free")] == [0, 0, 0, 0, 1]
    assert tagged["three, blocked"].iterations >= 1 and len(tagged["three, blocked"].path) >= 3
    for n, count in ((5, 3), (6, 4), (7, 5)):  # W - 1, W, W + 1 candidates for the input's waypoint 0
        for name in ("slice", "zigzag"):
            first = next(t for t in tagged[f"{name}{n}"].trace if t[0] == "shortcut")
            assert first[1:3] == (0, count), (name, n, first)
    # the first valid j lies in a later window than the first (rank 4 or more from the far end, 4 questions per round)
    assert next(t for t in tagged["zigzag7"].trace if t[0] == "shortcut")[3] == 4
    assert next(t for t in tagged["slice7"].trace if t[0] == "shortcut")[3] == 4
    assert sum(any(t[0] == "shortcut" and t[3] is not None and t[3] >= 4 for t in w.trace) for w in want) >= 6
    return items, want, run(vamp, items, s)


def test_batch_matches_the_comparator(batch):
    items, want, got = batch
    check(items, got, want)
    assert all(g.status == "ok" for g in got)
    for g in got:  # Path::cost of what came back
        if len(g.path) >= 2:
            p = np.stack(g.path).astype(np.float64)
            assert g.cost == pytest.approx(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(1)).sum(), rel=1e-5)
        else:
            assert g.cost == float("inf")


@pytest.mark.parametrize("w", [2, 4, 64])
def test_questions_per_round_changes_no_bit_and_the_totals_are_the_windowed_counts(vamp, batch, w):
    items, want, base = batch
    got = run(vamp, items, settings_of(questions_per_round=w))
    assert [key(g) for g in got] == [key(g) for g in base]
    counts = [windowed_questions(x.trace, w) for x in want]
    assert got[0].edges_checked == sum(counts)  # the call's total rides on the first result
    assert [g.edges_checked for g in got[1:]] == counts[1:]
    rounds = max(windowed_rounds(x.trace, w) for x in want)
    assert rounds <= got[0].validity_calls <= rounds + 16 + 1  # the host looks every 16 rounds by default


def test_check_every_changes_no_bit(vamp, batch):
    items, want, base = batch
    got = run(vamp, items, settings_of(check_every=1, questions_per_round=4))
    assert [key(g) for g in got] == [key(g) for g in base]
    rounds = max(windowed_rounds(x.trace, 4) for x in want)
    assert rounds <= got[0].validity_calls <= rounds + 2


def test_batch_independence(vamp, batch):
    """a path's result depends on nothing but its own waypoints, environment and settings"""
    items, want, base = batch
    keys = [key(g) for g in base]
    assert [key(g) for g in run(vamp, items[::-1])][::-1] == keys
    alone = [next(i for i, (it, w) in enumerate(zip(items, want)) if it.scene.kind == kind and w.replaced) for kind in ("cage", "mixed")]
    alone.append(next(i for i, w in enumerate(want) if len(items[i].path) > 2 and w.questions == 1))
    for i in alone:
        assert key(run(vamp, [items[i]])[0]) == keys[i]


def test_capacity(vamp, batch):
    items = batch[0]
    longest = max(len(it.path) for it in items)
    s = settings_of(max_waypoints=longest + 1)
    want = [it.expected(s) for it in items]
    assert sum(w.status == CAPACITY for w in want) >= 4 and sum(w.status == OK and w.iterations > 0 for w in want) >= 4
    got = run(vamp, items, s)
    check(items, got, want)  # capacity results are still valid paths between the same ends
    assert [g.status for g in got] == ["capacity" if w.status == CAPACITY else "ok" for w in want]
    assert all(len(g.path) <= longest + 1 for g in got)


def test_other_operation_lists(vamp, batch):
    """bit for bit only: like the reference, a subdivision does not ask whether the two halves of a valid edge are valid
    motions themselves (their samples lie elsewhere), and with these settings one of them is not"""
    items = batch[0][:12]
    for ops, kw in ((["SHORTCUT"], {}), (["BSPLINE", "SHORTCUT"], {}), (["BSPLINE", "BSPLINE", "SHORTCUT", "SHORTCUT"], dict(max_iterations=2)),
                    (["SHORTCUT", "BSPLINE"], dict(max_steps=2, min_change=0.01, midpoint_interpolation=0.25)), ([], {}),
                    (["SHORTCUT", "BSPLINE"], dict(max_iterations=0))):
        s = settings_of(operations=ops, **kw)
        want = [it.expected(s) for it in items]
        check(items, run(vamp, items, s), want, valid=False)


def test_non_finite_waypoint(vamp, batch, scenes, cage_plans):
    """every question that touches the NaN waypoint is invalid and its distance passes no min_change test: the path ends;
    under SHORTCUT alone it comes back with its input bytes, and its neighbours in the batch are not affected"""
    items, want, base = batch
    blocked = next(it for it in items if it.tag == "three, blocked")
    bad = Item(blocked.scene, blocked.path, "nan")
    bad.path[1][3] = np.nan
    neighbours = [i for i, it in enumerate(items) if it.tag in ("cage0", "cage5", "mixed8")]
    assert len(neighbours) == 3
    mixed = [items[neighbours[0]], bad, items[neighbours[1]], bad, items[neighbours[2]]]
    s = settings_of(operations=["SHORTCUT"])
    got = run(vamp, mixed, s)
    for g in (got[1], got[3]):
        assert g.status == "ok" and [q.tobytes() for q in g.path] == [q.tobytes() for q in bad.path]
    rest = [mixed[0], mixed[2], mixed[4]]
    check(rest, [got[0], got[2], got[4]], [it.expected(s) for it in rest])
    # default operations: the B-spline step subdivides, then no candidate passes (the NaN waypoint's neighbours are NaN)
    got = run(vamp, mixed)
    w = bad.expected(settings_of())
    for g in (got[1], got[3]):
        assert (g.status, g.iterations, len(g.path)) == ("ok", w.iterations, len(w.path)) and len(g.path) == 5
        a, b = np.stack(g.path), np.stack(w.path)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))
        assert [q.tobytes() for q in g.path[::2]] == [q.tobytes() for q in bad.path]  # the input's waypoints, untouched
    assert [key(got[i]) for i in (0, 2, 4)] == [key(base[i]) for i in neighbours]
    # a NaN waypoint that a shortcut can jump over is erased like any other
    long_bad = Item(scenes["cage"], cage_plans[0], "nan in a long path")
    long_bad.path[5][2] = np.nan
    w = long_bad.expected(settings_of(operations=["SHORTCUT"]))
    g = run(vamp, [long_bad], settings_of(operations=["SHORTCUT"]))[0]
    assert key(g) == key(w)


@pytest.mark.parametrize("robot", ["ur5", "fetch", "baxter"])
def test_other_robots(vamp, oracle, robot):
    """6, 8 and 14 joints: one planned path in the sphere cage, and the same path in the empty environment"""
    cage, empty = Scene(oracle, robot, "cage"), Scene(oracle, robot, "empty")
    s = settings_of()
    for k, (a, b) in enumerate(zip(*cage.valid_pairs(4, 5))):
        path = cage.plan(a, b, 100 * k, max_iterations=500)
        if len(path) > 2:
            items = [Item(cage, path, f"{robot} cage"), Item(empty, path, f"{robot} empty")]
            want = [it.expected(s) for it in items]
            if want[0].erased and want[0].replaced:
                break
    else:
        raise AssertionError("no path that exercises both routines")
    check(items, run(vamp, items, s), want)  # (in the empty environment only self-collision can block the straight line)


def test_installed_name_and_reference_settings_take_the_same_road(vamp, batch):
    items, want, base = batch
    some = items[:10]
    got = vamp.panda.simplify_multi([it.path for it in some], [it.scene.env for it in some], vamp.SimplifySettings())
    assert [(STATUS[g.status], int(g.iterations), [np.asarray(q, np.float32).tobytes() for q in g.path]) for g in got] == \
        [key(g) for g in base[:10]]
    assert all(g.cost == b.cost or (len(g.path) < 2) for g, b in zip(got, base[:10]))
    s = vamp.SimplifySettings(max_iterations=2, operations=[vamp.SimplifyRoutine.BSPLINE, vamp.SimplifyRoutine.SHORTCUT])
    s.bspline.max_steps, s.bspline.min_change = 3, 0.02
    want2 = [it.expected(settings_of(max_iterations=2, operations=["BSPLINE", "SHORTCUT"], max_steps=3, min_change=0.02)) for it in some]
    got2 = vamp.panda.simplify_multi([it.path for it in some], [it.scene.env for it in some], s)
    assert [(STATUS[g.status], int(g.iterations), [np.asarray(q, np.float32).tobytes() for q in g.path]) for g in got2] == \
        [key(w) for w in want2]


@pytest.fixture(scope="module")
def staggered(vamp, batch):
    """six paths of the batch that finish in different rounds: two whose straight line is valid (finished in round 2), one
    too short to ask anything, and the three of the others that need the fewest rounds alone; run with the default
    check_every at 4 questions per round"""
    items, want, _ = batch
    rounds = [windowed_rounds(w.trace, 4) for w in want]
    by_rounds = sorted(range(len(items)), key=lambda i: rounds[i])
    pick = [i for i in by_rounds if len(items[i].path) > 2 and want[i].questions == 1][:2]
    pick.append(next(i for i, it in enumerate(items) if it.tag == "two"))
    pick += [i for i in by_rounds if want[i].iterations > 0 and (want[i].erased or want[i].replaced)][:3]
    assert len(pick) == 6 and len({rounds[i] for i in pick}) >= 3
    pick.sort()
    some = [items[i] for i in pick]
    return some, [want[i] for i in pick], run(vamp, some, settings_of(questions_per_round=4))


@pytest.mark.parametrize("every", [1, 3])
def test_the_host_looks_every_check_every_rounds_and_changes_no_bit(vamp, staggered, every):
    """the call ends at the first look after the last path has ended, within the bounds the tests above use: the rounds
    the slowest path needs alone, the one that consumes its last answers, and at most check_every more"""
    items, want, base = staggered
    check(items, base, want)
    got = run(vamp, items, settings_of(check_every=every, questions_per_round=4))
    assert [key(g) for g in got] == [key(g) for g in base]
    counts = [windowed_questions(w.trace, 4) for w in want]
    assert [g.edges_checked for g in got[1:]] == counts[1:] and got[0].edges_checked == sum(counts)
    rounds, need = got[0].validity_calls, max(windowed_rounds(w.trace, 4) for w in want)
    assert rounds > 0 and rounds % every == 0
    assert rounds * 4 >= max(counts)
    assert need <= rounds <= need + every + 1


def test_a_call_of_short_paths_runs_no_round(vamp, scenes, cage_plans):
    """0, 1 and 2 waypoints only, in real environments and the empty one (None): nothing is asked, every path comes back
    with its input bytes"""
    cage, empty, p = scenes["cage"], scenes["empty"], cage_plans[0]
    assert cage.env is not None and empty.env is None and not cage.question(p[0], p[-1])
    items = [Item(cage, [p[0], p[-1]], "two, blocked"), Item(empty, [], "none"), Item(empty, p[:2], "two"),
             Item(cage, p[:1], "one"), Item(empty, p[3:4], "one"), Item(scenes["mixed"], p[1:3], "two")]
    for s in (settings_of(), settings_of(check_every=1, questions_per_round=2)):
        got = run(vamp, items, s)
        assert [[q.tobytes() for q in g.path] for g in got] == [[q.tobytes() for q in it.path] for it in items]
        assert all(g.status == "ok" and g.iterations == 0 for g in got)
        assert [g.validity_calls for g in got] == [0] * len(items) and [g.edges_checked for g in got] == [0] * len(items)
