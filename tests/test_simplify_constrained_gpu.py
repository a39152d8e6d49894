"""planning.simplify_multi_constrained / <robot>.simplify_multi_constrained_raw / vmv_simplify_multi_constrained on the device.

Expected results come from tests/simplify_constrained_serial.py: simplify_serial's loop with the three changes of the
constrained call, the CPU oracle answering validity and the product's batch calls answering the band tests and the
projection one question at a time.  Per path the status, the iterations, the length, every waypoint bit and band_refused
are compared.  The inputs: the solved paths of tests/test_rrtc_constrained_gpu.py's twelve Panda problems under
upright(z, 0.2), and hand-built paths - runs of projected Halton configurations whose consecutive edges are in band and
collision-free - for the window boundary, the 64-lane ballot, the out-of-band and the non-finite input.  max_waypoints is
256 throughout."""
import numpy as np
import pytest

import constraint_serial as S
from simplify_constrained_serial import OUT_OF_BAND, product_hooks, simplify_constrained_serial
from simplify_serial import CAPACITY, OK, cost, windowed_questions
from test_constraint_gpu import frame_slack, to_vamp
from test_rrtc_constrained_gpu import ANGLE, OTHERS, PANDA, Case

pytestmark = pytest.mark.gpu
STATUS = {"ok": OK, "capacity": CAPACITY, "out_of_band": OUT_OF_BAND}
MAX_WAYPOINTS = 256
W_DEFAULT = 16  # the library's questions_per_round
LONG = 67       # waypoints: a B-spline step over it looks at 65 indices, one more than a wave's ballot holds


class Item:
    """one path to simplify in one scene under one constraint"""

    def __init__(self, scene, constraint, path, tag):
        self.scene, self.constraint, self.tag = scene, constraint, tag
        self.path = [np.array(q, np.float32) for q in path]

    def expected(self, mod, **kw):
        kw.setdefault("max_waypoints", MAX_WAYPOINTS)
        return simplify_constrained_serial(self.path, self.scene.question, product_hooks(mod, self.constraint), **kw)


def key(r):
    """what must not depend on the rest of the batch or on how it is asked"""
    return (r.status if isinstance(r.status, int) else STATUS[r.status], int(r.iterations),
            [np.asarray(q, np.float32).tobytes() for q in r.path], int(r.band_refused))


def same(got, want, items):
    for i, (g, w) in enumerate(zip(got, want)):
        assert key(g)[:2] == key(w)[:2] and len(g.path) == len(w.path), (i, items[i].tag, key(g)[:2], len(g.path), key(w)[:2], len(w.path))
        assert key(g)[2] == key(w)[2], (i, items[i].tag)
        assert key(g)[3] == key(w)[3], (i, items[i].tag, g.band_refused, w.band_refused)


def run(vamp, mod, items, constraints=None, **kw):
    s = vamp.planning.SimplifyMultiSettings(max_waypoints=kw.pop("max_waypoints", MAX_WAYPOINTS), **kw)
    cons = [it.constraint for it in items] if constraints is None else constraints
    return vamp.planning.simplify_multi_constrained(mod, [it.path for it in items], [it.scene.env for it in items], cons, s)


def chain(mod, scene, constraint, rows, length, avoid=None, at_least=None):
    """a run of `length` of the rows (of at_least where no row is left to go on with): from rows[0] on always the first row
    not yet used whose edge from the run's end is in band and collision-free; avoid: from the third waypoint on the edge
    from `avoid` must be OUT of band as well"""
    path, unused = [rows[0]], np.ones(len(rows), bool)
    unused[0] = False
    while len(path) < length:
        idx = np.flatnonzero(unused)
        rest = rows[idx]
        ok = np.asarray(mod.constraint_check_motion_batch(np.repeat(path[-1][None], len(rest), 0), rest, constraint), bool)
        if avoid is not None and len(path) >= 2:
            ok = ok & ~np.asarray(mod.constraint_check_motion_batch(np.repeat(avoid[None], len(rest), 0), rest, constraint), bool)
        k = next((int(k) for k in np.flatnonzero(ok) if scene.question(path[-1], rest[k])), None)
        if k is None:
            assert at_least is not None and len(path) >= at_least, (len(path), length)
            break
        unused[idx[k]] = False
        path.append(rest[k])
    return path


def walk(mod, scene, constraint, start, robot, length, step=0.045):
    """a zig-zag of short steps, each projected again: `length` waypoints whose consecutive edges are in band and
    collision-free (a step that fails either is left out)"""
    moves = S.ee_mask(robot).astype(np.float32)
    rng = np.random.default_rng(11)
    dirs = [d * moves / np.linalg.norm(d * moves) for d in rng.normal(size=(2, len(moves)))]
    path, k = [np.array(start, np.float32)], 0
    while len(path) < length and k < 8 * length:
        q, _, converged, _ = mod.project_batch((path[-1] + np.float32(step) * dirs[k % 2].astype(np.float32))[None].astype(np.float32), constraint)
        k += 1
        q = np.asarray(q, np.float32)[0]
        if converged[0] and mod.constraint_check_motion_batch(path[-1][None], q[None], constraint)[0] and scene.question(path[-1], q):
            path.append(q)
    assert len(path) == length
    return path


def hand_built(mod, scene, constraint, rows, raw):
    """the hand-built inputs in one scene: dict tag -> Item.  rows: projected, collision-free configurations; raw:
    unprojected ones"""
    out_row = next(q for q in raw if not mod.constraint_check_batch(q[None], constraint)[0])
    long = chain(mod, scene, constraint, rows, LONG)
    # from its first waypoint only the second is reachable inside the band: W + 2 candidates, none of them in band
    window = chain(mod, scene, constraint, rows[1:], W_DEFAULT + 4, avoid=rows[1])
    outside = [q.copy() for q in long[:5]]
    outside[2] = out_row
    nan = [q.copy() for q in long[:5]]
    nan[2][3] = np.nan
    paths = {"two": long[:2], "three": long[:3], "window": window, "long": long, "outside": outside, "nan": nan}
    return {tag: Item(scene, constraint, p, tag) for tag, p in paths.items()}


class Batch:
    def __init__(self, vamp, oracle):
        self.vamp, self.case = vamp, Case(vamp, oracle, "panda", PANDA)
        self.mod, self.constraint = self.case.mod, self.case.constraint
        plans = self.case.run(list(range(len(PANDA))))
        self.items = [Item(p["scene"], self.constraint, g.path, f"plan{i}")
                      for i, (p, g) in enumerate(zip(self.case.problems, plans)) if len(g.path) >= 2]
        self.empty = self.case.scenes["empty"]
        (rows,) = vamp.planning.project_goals(self.mod, [S.configs("panda", 768)], self.constraint, self.empty.env)
        self.rows = rows
        self.hand = hand_built(self.mod, self.empty, self.constraint, rows, S.configs("panda", 8))
        self.items += list(self.hand.values())
        self.want = [it.expected(self.mod) for it in self.items]
        self.got = run(vamp, self.mod, self.items)
        self.finite = [i for i, it in enumerate(self.items) if it.tag != "nan"]

    def index(self, tag):
        return next(i for i, it in enumerate(self.items) if it.tag == tag)


@pytest.fixture(scope="module")
def batch(vamp, oracle):
    return Batch(vamp, oracle)


def report(items, got, want):
    for i, (it, g, w) in enumerate(zip(items, got, want)):
        print(f"{i} {it.tag}: {len(it.path)} -> {len(g.path)} waypoints, status {g.status}, iterations {g.iterations}, questions "
              f"{w.questions} asked serially of which the band refused {w.band_refused} ({sum(1 for _, r, ok in w.asked if r and ok)} "
              f"of them valid); {len(w.projected)} candidates projected, {sum(m for *_, m, _ in w.projected)} moved, "
              f"{sum(m and r for *_, m, r in w.projected)} moved and accepted, {sum(not c for _, _, c, _, _ in w.projected)} did not "
              f"converge; cost {cost(it.path):.4f} -> {cost(w.path):.4f}")


def test_batch_equals_the_serial_statement(batch):
    items, want, got = batch.items, batch.want, batch.got
    report(items, got, want)
    same(got, want, items)
    counts = [windowed_questions(w.trace, W_DEFAULT) for w in want]
    assert [g.edges_checked for g in got[1:]] == counts[1:] and got[0].edges_checked == sum(counts)  # the total rides on the first
    # ---- what the inputs must exercise: conditions of the test, read off the serial trace
    tag = {it.tag: w for it, w in zip(items, want)}
    assert sum(len(it.path) > 2 for it in items if it.tag.startswith("plan")) >= 4  # tree-solved plans went in
    assert len(tag["two"].path) == 2 and tag["two"].questions == 0 and tag["three"].questions >= 1
    first = next(t for t in tag["window"].trace if t[0] == "shortcut")
    assert first[1] == 0 and first[2] > W_DEFAULT and (first[3] is None or first[3] >= W_DEFAULT), first  # a window boundary is crossed
    for name in ("outside", "nan"):
        w, g, it = tag[name], got[batch.index(name)], batch.hand[name]
        assert (w.status, w.iterations, w.questions, w.band_refused) == (OUT_OF_BAND, 0, 0, 0) and g.status == "out_of_band"
        assert [q.tobytes() for q in g.path] == [q.tobytes() for q in it.path] and g.edges_checked == 0
    assert all(w.status == OK for name, w in tag.items() if name not in ("outside", "nan"))
    assert any(kind == "shortcut" and r and ok for w in want for kind, r, ok in w.asked)  # a valid shortcut the band refused
    assert any(m and r for w in want for *_, m, r in w.projected)  # a projected midpoint that moved and was accepted
    assert any(cost(w.path) < cost(it.path) for it, w in zip(items, want) if len(it.path) > 2)  # a path got shorter
    print("projections that did not converge:", sum(not c for w in want for _, _, c, _, _ in w.projected))


def test_bspline_first_looks_at_more_indices_than_a_wave_has_lanes(vamp, batch):
    """BSPLINE before SHORTCUT: the first step subdivides the 67-waypoint path as it is and its min_change ballot runs over
    65 indices"""
    items = [batch.hand["long"], batch.hand["window"], batch.items[0]]
    kw = dict(operations=["BSPLINE", "SHORTCUT"], max_iterations=2, max_steps=1, min_change=0.01)
    want = [it.expected(batch.mod, operations=("BSPLINE", "SHORTCUT"), max_iterations=2, max_steps=1, min_change=0.01) for it in items]
    step = want[0].trace[1]
    assert step[:3] == ("bspline", 0, 2 * LONG - 1) and any(index > 2 * 64 for index, _, _ in step[3]), step[:3]  # a candidate of the second ballot
    for w in (W_DEFAULT, 2):
        same(run(vamp, batch.mod, items, questions_per_round=w, **kw), want, items)


@pytest.mark.parametrize("w", [2, 4, 64])
def test_no_bit_depends_on_questions_per_round(vamp, batch, w):
    got = run(vamp, batch.mod, batch.items, questions_per_round=w)
    assert [key(g) for g in got] == [key(g) for g in batch.got]
    counts = [windowed_questions(x.trace, w) for x in batch.want]
    assert [g.edges_checked for g in got[1:]] == counts[1:] and got[0].edges_checked == sum(counts)


@pytest.mark.parametrize("every", [1, 3])
def test_no_bit_depends_on_check_every(vamp, batch, every):
    got = run(vamp, batch.mod, batch.items, check_every=every, questions_per_round=4)
    assert [key(g) for g in got] == [key(g) for g in batch.got]


def test_no_bit_depends_on_the_batch(vamp, batch):
    items, base = batch.items, [key(g) for g in batch.got]
    assert [key(g) for g in run(vamp, batch.mod, items[::-1])][::-1] == base
    assert [key(g) for g in run(vamp, batch.mod, items, constraints=batch.constraint)] == base  # one shared record
    for tag in ("three", "window", "outside", "nan", "two", next(it.tag for it, w in zip(items, batch.want) if w.projected)):
        i = batch.index(tag)
        assert key(run(vamp, batch.mod, [items[i]])[0]) == base[i], tag
        assert key(run(vamp, batch.mod, [items[i]], constraints=batch.constraint)[0]) == base[i], tag


def test_three_constraints_mixed_in_one_call(vamp, batch):
    """upright, the plane and the box with a cone of tests/constraint_serial.py in one call, one record per path: every
    path as in a call of its own with its constraint shared, and as the serial statement has it.  Under the plane only
    short edges stay in band, so the inputs there are projected zig-zag walks and min_change is small."""
    mod, scene, P = batch.mod, batch.empty, vamp.planning
    kw = dict(min_change=0.005, questions_per_round=4)
    items = [batch.hand["three"], batch.items[0]]
    plane, box = (to_vamp(vamp, S.cases("panda")[name]) for name in ("plane", "box_cone"))
    (rows,) = P.project_goals(mod, [S.configs("panda", 16)], plane, scene.env)
    items += [Item(scene, plane, walk(mod, scene, plane, rows[k], "panda", 6), f"plane{k}") for k in (0, 1)]
    (rows,) = P.project_goals(mod, [S.configs("panda", 96)], box, scene.env)
    run_ = chain(mod, scene, box, rows, 6)  # (the box and the cone leave room for edges between projected configurations)
    items += [Item(scene, box, run_, "box_cone0"), Item(scene, box, run_[:4], "box_cone1")]
    items = [items[i] for i in (2, 0, 4, 3, 1, 5)]
    want = [it.expected(mod, min_change=0.005) for it in items]
    got = run(vamp, mod, items, **kw)
    report(items, got, want)
    same(got, want, items)
    assert all(w.status == OK for w in want)
    mixed = [w for it, w in zip(items, want) if it.tag[:5] in ("plane", "box_c")]
    assert sum(len(w.projected) for w in mixed) >= 1 and sum(w.band_refused for w in mixed) >= 1 and any(w.iterations > 0 for w in mixed)
    for i, it in enumerate(items):
        assert key(run(vamp, mod, [it], constraints=it.constraint, **kw)[0]) == key(got[i]), it.tag


def test_a_constraint_that_restricts_nothing_is_simplify_multi(vamp, batch):
    P = vamp.planning
    items = [batch.items[i] for i in batch.finite]  # (a non-finite waypoint is out of every band)
    free = vamp.EEConstraint()  # infinite bounds, max_angle 0
    for w in (0, 2):
        s = P.SimplifyMultiSettings(max_waypoints=MAX_WAYPOINTS, questions_per_round=w)
        got = P.simplify_multi_constrained(batch.mod, [it.path for it in items], [it.scene.env for it in items], free, s)
        want = P.simplify_multi(batch.mod, [it.path for it in items], [it.scene.env for it in items], s)
        assert [key(g)[:3] for g in got] == [(STATUS[x.status], int(x.iterations), [q.tobytes() for q in x.path]) for x in want]
        assert [g.edges_checked for g in got] == [x.edges_checked for x in want] and got[0].validity_calls == want[0].validity_calls
        assert all(g.band_refused == 0 for g in got)
    assert any(x.iterations > 0 and len(x.path) > 2 for x in want) and any(len(x.path) == 2 for x in want)


def test_capacity(vamp, batch):
    """max_waypoints just below one path's first subdivision: that path ends `capacity` as it stood, the others of the call
    are what they are alone under the same settings.  Once with the default operations (SHORTCUT has run before the first
    subdivision), once with BSPLINE first (the input itself is what would be subdivided)."""
    items, want = batch.items, batch.want
    first = {i: next(t for t in w.trace if t[0] == "bspline")[2] for i, w in enumerate(want) if any(t[0] == "bspline" for t in w.trace)}
    fits = [i for i in first if len(items[i].path) <= first[i] - 1]  # (max_waypoints may not be below the input's length)
    plan = next(i for i, it in enumerate(items) if it.tag.startswith("plan") and 8 <= len(it.path) <= 20)
    for ops, chosen, m in ((("SHORTCUT", "BSPLINE"), max(fits, key=lambda i: first[i]), None), (("BSPLINE", "SHORTCUT"), plan, 2 * len(items[plan].path) - 2)):
        m = first[chosen] - 1 if m is None else m  # 2 n - 1 = m + 1 waypoints would be needed
        some = [i for i in range(len(items)) if len(items[i].path) <= m]
        assert chosen in some and len(some) >= 4
        sub = [items[i] for i in some]
        expect = [it.expected(batch.mod, max_waypoints=m, operations=ops) for it in sub]
        got = run(vamp, batch.mod, sub, max_waypoints=m, operations=list(ops))
        same(got, expect, sub)
        g, w = got[some.index(chosen)], expect[some.index(chosen)]
        assert g.status == "capacity" and w.status == CAPACITY and 2 * len(g.path) - 1 == m + 1, (ops, len(g.path), m)
        print(ops, "max_waypoints", m, "statuses", [x.status for x in got])
        if ops[0] == "SHORTCUT":  # the paths that never needed more room are what they were in the large call
            unchanged = [k for k, i in enumerate(some) if key(expect[k]) == key(want[i])]
            assert len(unchanged) >= 2 and all(key(got[k]) == key(batch.got[some[k]]) for k in unchanged)
        else:
            assert [q.tobytes() for q in g.path] == [q.tobytes() for q in items[chosen].path] and g.iterations == 1
            assert any(x.status == "ok" for x in got) or any(len(x.path) > len(it.path) for x, it in zip(got, sub))


def test_every_returned_path_keeps_its_promises(vamp, batch):
    """from the input's first waypoint to its last, no dearer than the input, every edge collision-free, and no point of
    it farther beyond the band than the spacing of the band samples allows"""
    P, mod = vamp.planning, batch.mod
    band = ANGLE + 1e-3
    moves = S.ee_mask("panda")
    c64 = S.upright((0.0, 0.0, 1.0), ANGLE)
    step = 0.05  # check_step
    worst, checked = -np.inf, 0
    for it, g in zip(batch.items, batch.got):
        if g.status == "out_of_band" or len(it.path) < 2:
            continue
        path = np.stack(g.path).astype(np.float32)
        assert path[0].tobytes() == it.path[0].tobytes() and path[-1].tobytes() == it.path[-1].tobytes(), it.tag
        assert g.cost <= P.path_cost(it.path), (it.tag, g.cost, P.path_cost(it.path))
        assert P.validate_paths(mod, [path], [it.scene.env])[0], it.tag
        assert all(it.scene.question(a, b) for a, b in zip(path[:-1], path[1:])), it.tag
        # Every edge is an asked in-band edge or a piece of one (a subdivision does not ask the halves): its points lie
        # within h / 2 <= check_step / 2 of a passing sample, so the tool axis is at most sum_j |u_j| check_step / 2 beyond the
        # band (u the edge's unit direction), plus what the frames differ by: the passing samples passed in fp32, the
        # float64 cosine differs by at most 1.5 slack, the angle by that over sin(band).  At 4x finer float64 samples.
        tol = 1.5 * frame_slack(mod, "panda", path) / np.sin(band)
        for x, y in zip(path[:-1].astype(np.float64), path[1:].astype(np.float64)):
            length = np.linalg.norm(y - x)
            n_c = max(1, int(np.ceil(length / step)))
            t = np.arange(0, 4 * n_c + 1) / (4.0 * n_c)
            cs = S.in_band("panda", x[None, :] + (y - x)[None, :] * t[:, None], c64)[1]["cs"]
            excess = float((np.arccos(np.clip(cs, -1.0, 1.0)) - band).max())
            bound = (np.abs(y - x)[moves].sum() / length if length > 0 else 0.0) * step / 2
            worst, checked = max(worst, excess), checked + 1
            assert excess <= bound + tol, (it.tag, excess, bound, tol)
    print(f"{checked} edges; largest angle beyond the band at 4x finer float64 samples {worst:.3e} rad")
    assert checked >= 50


@pytest.mark.parametrize("robot", sorted(OTHERS))
def test_other_robots(vamp, oracle, robot):
    """the solved plans of the robot's four problems and hand-built runs, four paths in all (Baxter: the constraint acts on
    the arm kEeJointMask moves)"""
    c = Case(vamp, oracle, robot, OTHERS[robot])
    plans = c.run(list(range(len(OTHERS[robot]))))
    items = [Item(p["scene"], c.constraint, g.path, f"plan{i}") for i, (p, g) in enumerate(zip(c.problems, plans)) if len(g.path) > 2][:2]
    scene = c.scenes["empty"]
    (rows,) = vamp.planning.project_goals(c.mod, [S.configs(robot, 256)], c.constraint, scene.env)
    k = 0
    while len(items) < 4:  # (Baxter's other arm is in the way of many chords: its runs may end early)
        items.append(Item(scene, c.constraint, chain(c.mod, scene, c.constraint, rows[8 * k:], 7, at_least=3), f"run{k}"))
        k += 1
    want = [it.expected(c.mod) for it in items]
    for w in (0, 2):
        got = run(vamp, c.mod, items, questions_per_round=w)
        same(got, want, items)
    report(items, got, want)
    assert any(w.iterations > 0 for w in want) and sum(w.band_refused for w in want) > 0
