"""planning.optimize_multi_constrained / <robot>.optimize_multi_constrained_raw / vmv_optimize_multi_constrained on the device.

Expected results come from tests/optimize_constrained_serial.py: optimize_serial's loop with the changes of the constrained
call, the device's own clearance_grad_batch, project_batch, constraint_check_batch and constraint_check_motion_batch asked
per path (a lane's result is its own: tests/test_constraint_gpu.py) and the CPU oracle answering validity.  Per path the
status, the iterations, the best iteration, both costs, the four minima, held and every waypoint are compared bit for bit.
The inputs are built as tests/test_simplify_constrained_gpu.py builds its runs: projected Halton configurations whose
consecutive edges are in band and collision-free (in the empty environment; between the cage's spheres such chords are
too rare), and projected zig-zag walks, over the sphere cage and the empty environment, under upright(z, 0.2).
max_iterations 12 and validate_every 4 throughout unless a test says otherwise."""
import numpy as np
import pytest

import constraint_serial as S
from lm_pins import antiparallel
from optimize_constrained_serial import OUT_OF_BAND, optimize_constrained_serial, product_hooks
from optimize_serial import NO_VALID, NONFINITE, OK
from test_constraint_gpu import frame_slack, to_vamp
from test_rrtc_constrained_gpu import ANGLE, OTHERS, PANDA, Case
from test_simplify_constrained_gpu import chain, walk

pytestmark = pytest.mark.gpu
KEYS = ("max_iterations", "validate_every", "step", "max_step", "min_change", "smooth_weight", "env_weight", "self_weight",
        "env_margin", "self_margin")
STATUS = ("ok", "no_valid", "nonfinite", "out_of_band")


class Item:
    """one path to optimise in one scene under one constraint"""

    def __init__(self, mod, scene, constraint, path, tag):
        self.mod, self.scene, self.constraint, self.tag = mod, scene, constraint, tag
        self.path = np.ascontiguousarray(np.array(path, np.float32).reshape(len(path), len(scene.lower)))
        self.upper = (scene.lower + scene.span).astype(np.float32)

    def clearance_grad(self, X):
        return self.mod.clearance_grad_batch(np.ascontiguousarray(X, np.float32), self.scene.env)

    def expected(self, s, cs=None):
        return optimize_constrained_serial(self.path, self.clearance_grad, self.scene.question, lower=self.scene.lower, upper=self.upper,
                                           **product_hooks(self.mod, self.constraint, cs), **{k: getattr(s, k) for k in KEYS})


def settings_of(vamp, **kw):
    kw.setdefault("max_iterations", 12)
    kw.setdefault("validate_every", 4)
    return vamp.planning.OptimizeMultiSettings(**kw)


def run(items, s, cs=None, constraints=None):
    """-> per item (status, iterations, best_iteration, held, bits of cost_first, cost, clearance_first, clearance, waypoints)"""
    cons = [it.constraint for it in items] if constraints is None else constraints
    raw = items[0].mod.optimize_multi_constrained_raw([it.path for it in items], [it.scene.env for it in items], cons, s, cs)
    off = raw["offsets"]
    return [(int(raw["status"][p]), int(raw["iterations"][p]), int(raw["best_iteration"][p]), int(raw["held"][p]),
             raw["cost_first"][p].tobytes(), raw["cost"][p].tobytes(), raw["clearance_first"][p].tobytes(), raw["clearance"][p].tobytes(),
             raw["points"][off[p]:off[p + 1]].tobytes()) for p in range(len(items))], raw


def key_of(w):
    f = np.float32
    return (w.status, w.iterations, w.best_iteration, w.held, f(w.cost_first).tobytes(), f(w.cost).tobytes(),
            np.array(w.clearance_first, f).tobytes(), np.array(w.clearance, f).tobytes(), np.array(w.path, f).tobytes())


def same(items, got, want):
    assert len(got) == len(want) == len(items)
    for i, (it, g, w) in enumerate(zip(items, got, want)):
        k = key_of(w)
        assert g[:4] == k[:4], (i, it.tag, g[:4], k[:4])
        for name, a, b in zip(("cost_first", "cost", "clearance_first", "clearance"), g[4:8], k[4:8]):
            assert a == b, (i, it.tag, name, np.frombuffer(a, np.float32), np.frombuffer(b, np.float32))
        assert g[8] == k[8], (i, it.tag, "waypoints")
        if g[0] != OK:
            assert g[8] == it.path.tobytes(), (i, it.tag)  # every other status returns the input's bytes


def report(items, want):
    for i, (it, w) in enumerate(zip(items, want)):
        moved = sum(len(m) for m, _ in w.trace[1:])
        print(f"{i} {it.tag}: {len(it.path)} waypoints, status {STATUS[w.status]}, iterations {w.iterations}, best {w.best_iteration}, "
              f"U {w.cost_first:.5f} -> {w.cost:.5f}, held {w.held}, repaired at iterate 0 {len(w.trace[0][0]) if w.trace else 0}, "
              f"moved by later projections {moved}, validated {[(k, h[4]) for k, h in enumerate(w.history) if h[3]]}")


def zigzag(mod, scene, constraint, start, robot, length, at_least=None, step=0.045):
    """test_simplify_constrained_gpu.walk's zig-zag of short projected steps, whose edges are in band and collision-free; a
    walk that gets stuck (a joint at its bound, a sphere in the way) may end with at_least waypoints"""
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
    assert len(path) >= (length if at_least is None else at_least), (len(path), length)
    return path


class Batch:
    def __init__(self, vamp, oracle):
        P = vamp.planning
        self.vamp, self.case = vamp, Case(vamp, oracle, "panda", PANDA)
        mod, c = self.case.mod, self.case.constraint
        self.mod, self.constraint = mod, c
        empty, cage = self.case.scenes["empty"], self.case.scenes["cage"]
        raw = S.configs("panda", 768)
        (rows,) = P.project_goals(mod, [raw], c, empty.env)
        (crow,) = P.project_goals(mod, [raw[:256]], c, cage.env)
        long = chain(mod, empty, c, rows, 66)
        item = lambda scene, path, tag, con=c: Item(mod, scene, con, path, tag)  # noqa: E731
        items = [item(empty, long[:0], "none"), item(empty, long[:1], "one"), item(empty, long[:2], "two"),
                 item(empty, long[:3], "three"), item(cage, zigzag(mod, cage, c, crow[0], "panda", 4), "four cage"),
                 item(empty, long[::-1][:65], "65"), item(empty, long, "66"),
                 item(cage, zigzag(mod, cage, c, crow[20], "panda", 3), "three cage"), item(empty, chain(mod, empty, c, rows[100:], 5), "five"),
                 item(empty, zigzag(mod, empty, c, rows[3], "panda", 9, at_least=5), "walk 9"), item(cage, zigzag(mod, cage, c, crow[5], "panda", 12, at_least=5), "walk cage")]
        # one unprojected interior waypoint, a short way out of the band: repaired at iterate 0
        rep = [q.copy() for q in zigzag(mod, empty, c, rows[7], "panda", 6, at_least=4)]
        out = next(q for q in (rep[2] + np.float32(t) * S.ee_mask("panda").astype(np.float32) for t in (0.02, 0.04, 0.08, 0.16))
                   if not mod.constraint_check_batch(q[None], c)[0])
        rep[2] = out.astype(np.float32)
        items.append(item(empty, rep, "repaired"))
        nan = [q.copy() for q in long[:5]]
        nan[2][3] = np.nan
        items.append(item(empty, nan, "nan"))
        outside = next(q for q in raw if not mod.constraint_check_batch(q[None], c)[0])
        items.append(item(empty, [q.copy() for q in long[:4]] + [outside], "end outside"))
        # an interior waypoint whose tool axis is antiparallel to its constraint's reference axis: no direction to turn in
        row, anti64 = antiparallel(vamp, "panda", raw)
        assert row is not None
        anti = to_vamp(vamp, anti64)
        ends, _, conv, _ = mod.project_batch(raw[200:232], anti)
        ends = np.asarray(ends, np.float32)[np.asarray(conv, bool)]
        assert len(ends) >= 2
        items.append(item(empty, [ends[0], raw[row], ends[1]], "antiparallel", anti))
        self.anti_row = raw[row]
        # a two-waypoint in-band edge, densified: the points on the chord may leave the band and are repaired at iterate 0
        items.append(item(empty, P.densify_path(np.stack(long[:2]), 4.0), "densified"))
        order = np.random.default_rng(4).permutation(len(items))
        self.items = [items[i] for i in order]
        self.main = [i for i, it in enumerate(self.items) if it.constraint is c]
        self.runs = {}

    def get(self, v=4, cs=None, **kw):
        """the settings, the serial statement's results and the device's for one choice of settings, computed once"""
        k = (v, None if cs is None else cs.max_iterations, tuple(sorted(kw.items())))
        if k not in self.runs:
            s = settings_of(self.vamp, validate_every=v, **kw)
            self.runs[k] = (s, [it.expected(s, cs) for it in self.items], *run(self.items, s, cs))
        return self.runs[k]

    def tag(self, name):
        return next(i for i, it in enumerate(self.items) if it.tag == name)


@pytest.fixture(scope="module")
def batch(vamp, oracle):
    return Batch(vamp, oracle)


@pytest.mark.parametrize("v", [1, 4, 100])
def test_batch_equals_the_serial_statement(batch, v):
    s, want, got, raw = batch.get(v)
    report(batch.items, want)
    same(batch.items, got, want)
    by = {it.tag: w for it, w in zip(batch.items, want)}
    # ---- what the inputs must exercise: conditions of the test, read off the statement's trace
    assert sorted(len(it.path) for it in batch.items)[:5] == [0, 1, 2, 3, 3] and {65, 66} <= {len(it.path) for it in batch.items}
    assert by["nan"].status == NONFINITE and by["end outside"].status == OUT_OF_BAND and by["antiparallel"].status == OUT_OF_BAND
    q, _, conv, evals = batch.mod.project_batch(batch.anti_row[None], batch.items[batch.tag("antiparallel")].constraint)
    assert not conv[0] and evals[0] == 0 and q[0].tobytes() == batch.anti_row.tobytes()  # back as given, unconverged
    assert by["none"].status == by["one"].status == OK and by["two"].status == OK
    assert by["repaired"].status == OK and by["repaired"].trace[0][0] == [2]  # the one waypoint out of band, moved at iterate 0
    assert by["densified"].status == OK and len(batch.items[batch.tag("densified")].path) > 3
    for name in ("nan", "end outside", "antiparallel"):
        assert (by[name].iterations, by[name].held, by[name].history) == (0, 0, [])
    # at least one waypoint moved by a projection and kept; at least one path cheaper than its input
    assert any(w.status == OK and any(m for m, _ in w.trace[1:w.best_iteration + 1]) for w in want)
    assert any(w.status == OK and w.cost < w.cost_first for w in want)
    assert any(w.iterations == 12 for w in want)
    assert raw["clearance_calls"] == 13 and raw["validation_calls"] == len([k for k in range(13) if k % v == 0 or k == 12])


def test_projections_that_fail_during_the_run_hold_their_waypoints(batch):
    """constraint_settings.max_iterations = 1: one evaluation after the first is often not enough to come back into the band"""
    cs = batch.vamp.ConstraintSettings(max_iterations=1)
    s, want, got, raw = batch.get(4, cs)
    report(batch.items, want)
    same(batch.items, got, want)
    assert any(w.held > 0 for w in want)
    assert any(w.held > 0 and w.status == OK for w in want)
    assert all(w.held == sum(len(h) for _, h in w.trace) for w in want)
    # held does not depend on validate_every's compaction points nor on the batch
    held = [g[3] for g in got]
    for v in (1, 100):
        s2 = settings_of(batch.vamp, validate_every=v)
        assert [g[3] for g in run(batch.items, s2, cs)[0]] == held
    i = max(range(len(want)), key=lambda k: want[k].held)
    assert run([batch.items[i]], s, cs)[0] == [got[i]]


def test_reversed_alone_twice_and_one_shared_record(batch):
    s, want, got, _ = batch.get(4)
    items = batch.items
    assert run(items[::-1], s)[0] == got[::-1]
    for it, g in zip(items, got):
        assert run([it], s)[0] == [g], it.tag
    assert run(items + items, s)[0] == got + got
    main = [items[i] for i in batch.main]
    assert run(main, s, constraints=batch.constraint)[0] == [got[i] for i in batch.main]  # one shared record
    assert run(main[:1], s, constraints=batch.constraint)[0] == [got[batch.main[0]]]


def test_three_constraints_mixed_in_one_call(batch):
    """upright, the plane and the box with a cone of tests/constraint_serial.py in one call, one record per path: every
    path as the serial statement has it, and as in a call of its own with its constraint shared"""
    vamp, mod, scene, P = batch.vamp, batch.mod, batch.case.scenes["empty"], batch.vamp.planning
    items = [batch.items[batch.tag("three")], batch.items[batch.tag("walk 9")]]
    plane, box = (to_vamp(vamp, S.cases("panda")[name]) for name in ("plane", "box_cone"))
    (rows,) = P.project_goals(mod, [S.configs("panda", 16)], plane, scene.env)
    items += [Item(mod, scene, plane, walk(mod, scene, plane, rows[k], "panda", 6), f"plane{k}") for k in (0, 1)]
    (rows,) = P.project_goals(mod, [S.configs("panda", 96)], box, scene.env)
    run_ = chain(mod, scene, box, rows, 6)
    items += [Item(mod, scene, box, run_, "box_cone0"), Item(mod, scene, box, run_[:4], "box_cone1")]
    items = [items[i] for i in (2, 0, 4, 3, 1, 5)]
    s = settings_of(vamp)
    want = [it.expected(s) for it in items]
    got, _ = run(items, s)
    report(items, want)
    same(items, got, want)
    assert all(w.status in (OK, NO_VALID) for w in want) and any(w.status == OK and w.iterations == 12 for w in want)
    for i, it in enumerate(items):
        assert run([it], s, constraints=it.constraint)[0] == [got[i]], it.tag


def test_every_ok_result_keeps_its_promises(batch):
    """from the input's first bits to its last, (1, 1) from validate_paths_constrained, valid edge by edge per the oracle, every
    waypoint in the band, and no point of it farther beyond the band than the spacing of the band samples allows"""
    P, mod = batch.vamp.planning, batch.mod
    band = ANGLE + 1e-3
    moves = S.ee_mask("panda")
    c64 = S.upright((0.0, 0.0, 1.0), ANGLE)
    step = 0.05  # check_step
    worst, checked = -np.inf, 0
    for v in (1, 4):
        s, want, got, _ = batch.get(v)
        for i in batch.main:
            it, g = batch.items[i], got[i]
            if g[0] != OK or len(it.path) < 2:
                continue
            path = np.frombuffer(g[8], np.float32).reshape(it.path.shape)
            assert path[0].tobytes() == it.path[0].tobytes() and path[-1].tobytes() == it.path[-1].tobytes(), it.tag
            valid, in_band = P.validate_paths_constrained(mod, [path], it.scene.env, it.constraint)
            assert valid[0] and in_band[0], it.tag
            assert all(it.scene.question(a, b) for a, b in zip(path[:-1], path[1:])), it.tag
            assert mod.constraint_check_batch(path, it.constraint).all(), it.tag
            assert np.frombuffer(g[5], np.float32)[0] <= np.frombuffer(g[4], np.float32)[0]
            # Every edge has been asked afresh: its points lie within check_step / 2 of a passing sample, so the tool axis is at
            # most sum_j |u_j| check_step / 2 beyond the band (u the edge's unit direction), plus what the frames differ by: the
            # passing samples passed in fp32, the float64 cosine differs by at most 1.5 slack, the angle by that over sin(band).
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


def test_a_constraint_that_restricts_nothing_is_optimize_multi(batch):
    vamp = batch.vamp
    items = [it for it in batch.items if np.isfinite(it.path).all()]  # (a non-finite path is the same in both calls too)
    items.append(batch.items[batch.tag("nan")])
    free = vamp.EEConstraint()  # infinite bounds, max_angle 0
    for v in (4, 100):
        s = settings_of(vamp, validate_every=v)
        got, raw = run(items, s, constraints=free)
        plain = batch.mod.optimize_multi_raw([it.path for it in items], [it.scene.env for it in items], s)
        for name in ("status", "iterations", "best_iteration", "cost_first", "cost", "clearance_first", "clearance", "points"):
            assert raw[name].tobytes() == plain[name].tobytes(), name
        assert (raw["clearance_calls"], raw["validation_calls"]) == (plain["clearance_calls"], plain["validation_calls"])
        assert not raw["held"].any()
    assert any(g[0] == OK and g[2] > 0 for g in got) and any(g[0] == NONFINITE for g in got)


def test_paths_that_stop_early_are_compacted_away(batch):
    """min_change so large that some paths stop at their first validated iterate while the others run on"""
    s, want, got, _ = batch.get(4, min_change=0.05)
    same(batch.items, got, want)
    its = {w.iterations for it, w in zip(batch.items, want) if len(it.path) > 2 and w.status in (OK, NO_VALID)}
    assert 4 in its and 12 in its, its
    full = batch.get(4)[2]
    late = [i for i, w in enumerate(want) if w.iterations == 12]
    assert all(got[i][8] == full[i][8] and got[i][3] == full[i][3] for i in late)  # the rest: bit for bit what they are without it


@pytest.mark.parametrize("robot", sorted(OTHERS))
def test_other_robots(vamp, oracle, robot):
    """four paths per robot (Baxter: the constraint acts on the arm kEeJointMask moves)"""
    c = Case(vamp, oracle, robot, OTHERS[robot])
    scene, cage = c.scenes["empty"], c.scenes["cage"]
    (rows,) = vamp.planning.project_goals(c.mod, [S.configs(robot, 256)], c.constraint, scene.env)
    items = [Item(c.mod, scene, c.constraint, chain(c.mod, scene, c.constraint, rows[8 * k:], 5, at_least=3), f"run{k}") for k in (0, 1)]
    items.append(Item(c.mod, scene, c.constraint, zigzag(c.mod, scene, c.constraint, rows[2], robot, 7, at_least=3), "walk"))
    (crow,) = vamp.planning.project_goals(c.mod, [S.configs(robot, 96)], c.constraint, cage.env)
    items.append(Item(c.mod, cage, c.constraint, zigzag(c.mod, cage, c.constraint, crow[0], robot, 4, at_least=3), "cage"))
    s = settings_of(vamp)
    want = [it.expected(s) for it in items]
    got, _ = run(items, s)
    report(items, want)
    same(items, got, want)
    assert run(items, s, constraints=c.constraint)[0] == got
    assert any(w.iterations == 12 for w in want) and any(w.status == OK and w.cost < w.cost_first for w in want)


def test_python_layer_densifies_and_names_its_statuses(batch):
    P, mod = batch.vamp.planning, batch.mod
    it = batch.items[batch.tag("two")]
    far = batch.items[batch.tag("end outside")]
    got = P.optimize_multi_constrained(mod, [it.path, far.path], [it.scene.env, far.scene.env], batch.constraint, settings_of(batch.vamp),
                                       resolution=4.0)
    dense = batch.items[batch.tag("densified")]
    assert len(got[0].path) == len(dense.path) and got[0].status == "ok" and got[1].status == "out_of_band" and got[1].held == 0
    want = batch.get(4)[2][batch.tag("densified")]
    assert np.stack(got[0].path).tobytes() == want[8] and got[0].held == want[3]
    assert batch.mod.optimize_multi_constrained(
        [it.path], [it.scene.env], batch.constraint, settings_of(batch.vamp), resolution=4.0)[0].path[1].tobytes() == got[0].path[1].tobytes()
