"""planning.retime_multi_constrained / <robot>.retime_multi_constrained on the device.

The yardstick is tests/retime_constrained_serial.py with the product's own validate_motion_batch and
constraint_check_motion_batch as hooks: the device's answer equals it bit for bit - status, first_invalid, rounds, levels,
repaired, stops, intervals, the duration and every sample.  The case set is tests/retime_constrained_cases.py's, whose
classes tests/test_retime_constrained.py asserts on the CPU; here every case must land in the same class.  Then the
consequences of the definition: a path's answer is its own whatever the batch, complete results pass both checks on every
returned pair, and the identities against retime_multi.  Every comparison is of bytes or of booleans."""
import numpy as np
import pytest

import retime_constrained_cases as C
import retime_constrained_serial as RC
import retime_serial as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """two results of the product, byte for byte"""
    return (a.status == b.status and a.intervals == b.intervals and a.first_invalid == b.first_invalid and
            np.array_equal(bits(np.float32(a.duration)), bits(np.float32(b.duration))) and
            (a.rounds, a.repaired, a.stops) == (b.rounds, b.repaired, b.stops) and np.array_equal(a.levels, b.levels) and
            same_samples(a, b))


def same_samples(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y))
               for x, y in ((a.times, b.times), (a.positions, b.positions), (a.velocities, b.velocities), (a.accelerations, b.accelerations)))


def settings_of(vamp, S):
    return vamp.planning.RetimeConstrainedSettings(blend=S.blend, grid_step=S.grid_step, dt=S.dt, max_grid=S.max_grid,
                                                   max_samples=S.max_samples, stop_at_waypoints=S.stop_at_waypoints,
                                                   blend_halvings=S.blend_halvings, max_rounds=S.max_rounds)


def constraint_of(vamp, c):
    """the product's constraint of a constraint_serial.Constraint; None: one that restricts nothing"""
    if c is None:
        return vamp.EEConstraint()
    return vamp.EEConstraint(frame=c.frame, pos_lo=c.pos_lo, pos_hi=c.pos_hi, tool_axis=c.tool_axis, ref_axis=c.ref_axis, max_angle=c.max_angle)


def environment_of(vamp, case):
    if not case.spheres:
        return None
    env = vamp.Environment()
    for s in case.spheres:
        env.add_sphere(vamp.Sphere([float(v) for v in s[:3]], float(s[3])))
    return env


class Hook:
    """a product call as a hook of the serial statement: one pair at a time, or all pairs of a round in one batch"""

    def __init__(self, batch):
        self.batch = batch

    def __call__(self, a, b):
        return bool(self.batch(a[None], b[None])[0])


def hooks_of(mod, env, constraint):
    valid = Hook(lambda a, b: mod.validate_motion_batch(a, b, env))
    band = None if constraint is None else Hook(lambda a, b: mod.constraint_check_motion_batch(a, b, constraint))
    return valid, band


def statement(mod, case, env, constraint, S=None, one_at_a_time=False):
    valid, band = hooks_of(mod, env, constraint)
    if one_at_a_time:
        valid, band = valid.__call__, None if band is None else band.__call__
    V, A = C.limits(case.robot)
    return RC.retime_constrained(case.path, V, A, S or case.settings, valid, band)


def against_statement(name, g, w):
    assert g.status == w.status, (name, g.status, w.status)
    assert g.first_invalid == (-1 if w.first_invalid == RC.NONE else w.first_invalid), (name, g.first_invalid, w.first_invalid)
    assert (g.rounds, g.repaired, g.stops) == (w.rounds, w.repaired, w.stops), (name, g.rounds, w.rounds)
    assert g.levels.dtype == np.uint8 and np.array_equal(g.levels, w.levels), (name, g.levels, w.levels)
    assert g.intervals == w.intervals and len(g.times) == w.samples, (name, g.intervals, w.intervals, len(g.times), w.samples)
    assert np.array_equal(bits(np.float32(g.duration)), bits(w.duration)), (name, g.duration, w.duration)
    for what, x, y in (("times", g.times, w.times), ("positions", g.positions, w.positions),
                       ("velocities", g.velocities, w.velocities), ("accelerations", g.accelerations, w.accelerations)):
        assert x.dtype == np.float32 and x.shape == y.shape, (name, what)
        differ = np.flatnonzero((bits(x) != bits(y)).reshape(len(x), max(x[:1].size, 1)).any(axis=1))
        assert differ.size == 0, (name, what, differ[:5])


@pytest.fixture(scope="module")
def sets(vamp):
    """per robot: the cases with their environments and constraints, ONE call per group of cases that share their settings,
    and the statement's result of every case on the product's hooks - shared by the tests, left unchanged"""
    out = {}
    for robot in C.ROBOTS:
        mod = getattr(vamp, robot)
        cases = C.cases(robot)
        V, A = C.limits(robot)
        envs = [environment_of(vamp, c) for c in cases]
        cons = [constraint_of(vamp, c.constraint) for c in cases]
        got, groups = [None] * len(cases), {}
        for k, c in enumerate(cases):
            groups.setdefault(c.settings, []).append(k)
        for S, members in groups.items():
            res = vamp.planning.retime_multi_constrained(mod, [cases[k].path for k in members], V, A, [envs[k] for k in members],
                                                         [cons[k] for k in members], settings_of(vamp, S))
            for k, r in zip(members, res):
                got[k] = r
        want = [statement(mod, c, envs[k], cons[k] if c.constraint is not None else None) for k, c in enumerate(cases)]
        out[robot] = dict(mod=mod, cases=cases, V=V, A=A, envs=envs, cons=cons, groups=groups, got=got, want=want)
    return out


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_the_case_set_equals_the_statement_bit_for_bit(sets, robot):
    s = sets[robot]
    assert len(s["groups"]) >= 4  # the main group, one halving, a long period, one round
    for c, g, w in zip(s["cases"], s["got"], s["want"]):
        against_statement(c.name, g, w)
    assert sum(len(g.times) for g in s["got"]) > 400  # (the set is not one of stillborn paths: 10 paths of 40 samples)


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_every_case_lands_in_the_class_the_cpu_found(sets, robot):
    """the oracle is the device's validate_motion and the float64 band agrees with the fp32 one beyond its margin: status,
    rounds and levels are those tests/test_retime_constrained.py classified, so no class is empty here"""
    s = sets[robot]
    for c, g, (e, _) in zip(s["cases"], s["got"], C.expected(robot)):
        assert (g.status, g.rounds, g.levels.tolist()) == (e.status, e.rounds, e.levels.tolist()), c.name
        assert g.first_invalid == (-1 if e.first_invalid == RC.NONE else e.first_invalid), c.name
    kinds = {c.kind: g for c, g in zip(s["cases"], s["got"])}
    H = C.SETTINGS.blend_halvings
    assert kinds["b"].status == "complete" and 0 < kinds["b"].levels.max() <= H and kinds["c"].stops == 1 and kinds["fc"].levels.max() == H + 1
    assert kinds["d"].status == "collision" and kinds["fd"].status == "out_of_band" and kinds["i"].status == "collision"
    assert [int(x > 0) for x in kinds["g"].levels] == [0, 1, 0, 1, 0] and kinds["g"].repaired == 2
    # (b) to (d) under both kinds of band, each on the device: a level clears, only the stop clears, a line ends the path
    named = {c.name: g for c, g in zip(s["cases"], s["got"])}
    for band in ("box", "cone"):
        level, stop, line = named[band + "_level"], named[band + "_stop"], named[band + "_line"]
        assert level.status == "complete" and 0 < level.levels.max() <= H and level.stops == 0, band
        assert stop.status == "complete" and stop.levels.max() == H + 1 and stop.stops == 1 and stop.rounds == H + 2, band
        assert line.status == "out_of_band" and line.rounds == 1 and not line.levels.any() and line.first_invalid >= 0, band


def test_hooks_asked_one_pair_at_a_time_give_the_same_statement(sets):
    s = sets["panda"]
    k = next(k for k, c in enumerate(s["cases"]) if c.kind == "g")
    c = s["cases"][k]
    w = statement(s["mod"], c, s["envs"][k], s["cons"][k], one_at_a_time=True)
    against_statement(c.name, s["got"][k], w)
    assert w.rounds >= 2


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_a_paths_answer_does_not_depend_on_the_batch(vamp, sets, robot):
    s = sets[robot]
    mod, V, A = s["mod"], s["V"], s["A"]
    S, members = max(s["groups"].items(), key=lambda kv: len(kv[1]))
    paths, envs, cons = ([s["cases"][k].path for k in members], [s["envs"][k] for k in members], [s["cons"][k] for k in members])
    got = [s["got"][k] for k in members]
    f = lambda p, e, c: vamp.planning.retime_multi_constrained(mod, p, V, A, e, c, settings_of(vamp, S))
    back = f(paths[::-1], envs[::-1], cons[::-1])[::-1]
    twice = f(paths + paths, envs + envs, cons + cons)
    assert all(same(a, b) for a, b in zip(got, back))
    assert len(twice) == 2 * len(got) and all(same(a, b) for a, b in zip(got + got, twice))
    assert len({g.rounds for g in got}) >= 3  # the paths of the batch end in different rounds
    for k, g in zip(members, got):
        alone = f([s["cases"][k].path], [s["envs"][k]], s["cons"][k])  # (one constraint: shared)
        assert len(alone) == 1 and same(alone[0], g), s["cases"][k].name


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_complete_results_pass_both_checks_on_every_returned_pair(sets, robot):
    s = sets[robot]
    complete = 0
    for k, (c, g) in enumerate(zip(s["cases"], s["got"])):
        if g.status != "complete" or len(g.times) < 2:
            continue
        complete += 1
        assert s["mod"].validate_motion_batch(g.positions[:-1], g.positions[1:], s["envs"][k]).all(), c.name
        assert s["mod"].constraint_check_motion_batch(g.positions[:-1], g.positions[1:], s["cons"][k]).all(), c.name
        assert np.array_equal(bits(g.positions[0]), bits(c.path[0])) and np.array_equal(bits(g.positions[-1]), bits(c.path[-1]))
        assert not g.velocities[0].any() and not g.velocities[-1].any()
    assert complete >= 6


@pytest.mark.parametrize("robot", C.ROBOTS)
def test_the_band_kernel_answers_as_constraint_check_motion_batch(sets, robot):
    """one round's pairs: the plain retime_multi samples of every case, each list under its case's constraint (the cases
    without one under the box of "box_level", which their corner leaves)"""
    s = sets[robot]
    mod, cases = s["mod"], s["cases"]
    box = s["cons"][next(k for k, c in enumerate(cases) if c.name == "box_level")]
    lists, cons = [], []
    for k, c in enumerate(cases):
        t = sets[robot]["got"][k]
        if len(t.times) >= 1:
            lists.append(t.positions)
            cons.append(s["cons"][k] if c.constraint is not None else box)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in lists])])
    got = mod._retime_band_pairs(np.concatenate(lists), offsets, cons)
    zeros = 0
    for a, (p, con) in enumerate(zip(lists, cons)):
        mine = got[offsets[a]:offsets[a + 1]]
        assert mine[-1] == 1  # a list's last row has no pair
        if len(p) > 1:
            want = mod.constraint_check_motion_batch(p[:-1], p[1:], con)
            assert np.array_equal(mine[:-1].astype(bool), want), a
            zeros += int((~want).sum())
    assert zeros > 20 and int(got.sum()) > 500
    shared = mod._retime_band_pairs(np.concatenate(lists), offsets, box)
    want = np.concatenate([np.append(mod.constraint_check_motion_batch(p[:-1], p[1:], box), True) if len(p) > 1 else [True] for p in lists])
    assert np.array_equal(shared.astype(bool), want)


def test_the_sphere_on_a_line_is_retime_multis_collision(vamp, sets):
    for robot in C.ROBOTS:
        s = sets[robot]
        k = next(k for k, c in enumerate(s["cases"]) if c.kind == "d")
        c, g = s["cases"][k], s["got"][k]
        S = settings_of(vamp, c.settings)
        plain = vamp.planning.retime_multi(s["mod"], [c.path], s["V"], s["A"], [s["envs"][k]], S)[0]
        assert plain.status == "collision" == g.status and plain.first_invalid == g.first_invalid and g.rounds == 1
        assert plain.intervals == g.intervals and same_samples(plain, g) and bits(np.float32(plain.duration)) == bits(np.float32(g.duration))
        # without constraints at all, and with one per path that restricts nothing: the same bytes
        bare = vamp.planning.retime_multi_constrained(s["mod"], [c.path], s["V"], s["A"], [s["envs"][k]], None, S)[0]
        assert same(bare, g)


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_the_identities_against_retime_multi_on_the_clean_cases(vamp, robot):
    """retime_serial's case set for all four robots, nothing to repair: without environments and constraints, in the empty
    environment, under a constraint that restricts nothing, and with every corner stopped"""
    mod = getattr(vamp, robot)
    paths = [w for _, w in R.cases(robot)]
    names = [n for n, _ in R.cases(robot)]
    V, A = R.limits(robot)
    P = vamp.planning
    base = dict(blend=R.CASE_SETTINGS.blend, grid_step=R.CASE_SETTINGS.grid_step, dt=R.CASE_SETTINGS.dt, max_grid=R.CASE_SETTINGS.max_grid)
    n = len(paths)
    for stop in (False, True):
        plain = P.retime_multi(mod, paths, V, A, None, P.RetimeSettings(stop_at_waypoints=stop, **base))
        S = P.RetimeConstrainedSettings(stop_at_waypoints=stop, **base)
        for envs, cons in ((None, None), (None, vamp.EEConstraint()), (None, [vamp.EEConstraint()] * n)):
            got = P.retime_multi_constrained(mod, paths, V, A, envs, cons, S)
            for name, g, p, w in zip(names, got, plain, paths):
                assert (g.status, g.intervals, g.first_invalid, g.rounds) == (p.status, p.intervals, p.first_invalid, 1), name
                assert same_samples(g, p) and np.array_equal(bits(np.float32(g.duration)), bits(np.float32(p.duration))), name
                assert len(g.levels) == len(w) and set(g.levels.tolist()) <= ({0, S.blend_halvings + 1} if stop else {0}), name
                assert g.stops == g.repaired == int((g.levels > 0).sum())
    # in the empty environment (the robot against itself): where retime_multi is complete the same bytes in one round; where
    # its first invalid pair lies on lines only, its collision, first_invalid and bytes; else the levels rose
    free = P.retime_multi(mod, paths, V, A, [None] * n, P.RetimeSettings(**base))
    raw = mod.retime_multi_constrained_raw(paths, V, A, [None] * n, None, P.RetimeConstrainedSettings(**base))
    got = P.retime_multi_constrained(mod, paths, V, A, [None] * n, None, P.RetimeConstrainedSettings(**base))
    seen = set()
    for name, g, p in zip(names, got, free):
        if p.status != "collision":
            assert (g.status, g.rounds, g.first_invalid) == (p.status, 1, p.first_invalid) and same_samples(g, p) and not g.levels.any(), name
            seen.add("same")
        elif g.rounds == 1:
            assert (g.status, g.first_invalid) == ("collision", p.first_invalid) and same_samples(g, p) and not g.levels.any(), name
            seen.add("line")
        else:
            assert g.levels.any(), name
            seen.add("repaired")
    assert "same" in seen
    assert 1 <= raw["validation_calls"] <= int(raw["rounds"].max())  # one call per round that has samples to ask about
    first_round = sum(len(p.times) - 1 for p in free if len(p.times) > 1)
    assert raw["questions"] >= first_round and (raw["rounds"].max() > 1 or raw["questions"] == first_round)


def test_every_corner_stopped_has_the_samples_of_stop_at_waypoints(vamp, sets):
    """the case whose corner only the stop clears: its samples are retime_multi's with stop_at_waypoints"""
    for robot in C.ROBOTS:
        s = sets[robot]
        stopped = [k for k, c in enumerate(s["cases"]) if c.kind in ("c", "fc")]
        assert len(stopped) == 3  # the sphere, the box, the cone
        for k in stopped:
            c, g = s["cases"][k], s["got"][k]
            assert g.stops == 1 == g.repaired and len(c.path) == 3
            S = settings_of(vamp, c.settings)
            stop = vamp.planning.retime_multi(s["mod"], [c.path], s["V"], s["A"], None,
                                              vamp.planning.RetimeSettings(blend=S.blend, grid_step=S.grid_step, dt=S.dt, max_grid=S.max_grid,
                                                                           max_samples=S.max_samples, stop_at_waypoints=True))[0]
            assert same_samples(g, stop) and g.intervals == stop.intervals


def test_one_constraint_for_all_paths_equals_the_same_constraint_per_path(vamp):
    """panda, paths of 4, 3 and 5 waypoints, one obstacle sphere: the smallest call in which the band kernel reads its
    record both ways (one for all; one per path, found through the sampled path's index) over paths of uneven length"""
    import constraint_serial as S

    mod, P = vamp.panda, vamp.planning
    constraint = vamp.EEConstraint.upright((0, 0, 1), 0.2)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.55, 0.0, 0.6], 0.08))
    (rows,) = P.project_goals(mod, [S.configs("panda", 96)], constraint, env)
    assert len(rows) >= 12
    paths = [rows[0:4], rows[4:7], rows[7:12]]
    V, A = C.limits("panda")
    s = P.RetimeConstrainedSettings()
    once = mod.retime_multi_constrained_raw(paths, V, A, [env] * 3, constraint, s)
    each = mod.retime_multi_constrained_raw(paths, V, A, [env] * 3, [constraint] * 3, s)
    print("status", once["status"], "rounds", once["rounds"], "samples", once["samples"], "questions", once["questions"])
    assert once["questions"] > 0 and (once["samples"] > 1).all()  # every path was sampled and its pairs were asked
    assert sorted(once) == sorted(each)
    for k in once:
        a, b = np.asarray(once[k]), np.asarray(each[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
