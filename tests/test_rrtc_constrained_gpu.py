"""planning.rrtc_multi_constrained / <robot>.rrtc_multi_constrained_raw / vmv_rrtc_multi_constrained on the device.

Expected results come from tests/rrtc_constrained_serial.py: rrtc_goals_serial's loop with the CPU oracle answering validity
and the product's batch calls answering the two constraint hooks one question at a time.  Every problem's status,
iterations, sizes, waypoint bits and goal are compared; a solved path is checked for what it promises - from the start's
bits to the named goal's, every edge valid and in band - and the result must not depend on the batch, its order or
check_every.  Endpoints come from planning.project_goals under upright(z, 0.2)."""
import numpy as np
import pytest

import constraint_serial as S
import ik_serial as K
from rrtc_constrained_serial import INVALID_ENDPOINT, rrtc_constrained_serial
from rrtc_goals_cases import key
from rrtc_serial import SOLVED
from test_rrtc_multi_gpu import Scene

pytestmark = pytest.mark.gpu
ANGLE = 0.2
RANGE = 0.5
# (scene, start row, goal rows, Halton skip, max_samples): rows index the projected, collision-free Halton configurations
# of the robot; a goal set made of the start's own neighbours (negative rows: start + a small step, projected again) is
# solved by a direct edge.  The skips are pinned: DESIGN.md 5o records what each problem does on the MI355X.
PANDA = [("empty", 0, (1,), 0, 256), ("empty", 2, (3, 4), 1000, 256), ("empty", 5, (6,), 2000, 256), ("empty", 7, (-1,), 0, 256),
         ("empty", 8, (9, 10), 3000, 600), ("empty", 11, (-1, 12), 4000, 256),
         ("cage", 0, (1,), 0, 256), ("cage", 2, (3,), 500, 256), ("cage", 4, (-1,), 0, 256), ("cage", 5, (6, 7), 1500, 256),
         ("cage", 8, (9,), 2500, 256), ("cage", 10, (11,), 3500, 256)]
OTHERS = {"ur5": [("empty", 0, (1,), 0, 256), ("empty", 2, (-1,), 0, 256), ("cage", 0, (1, 2), 1000, 256), ("cage", 3, (4,), 2000, 256)],
          "baxter": [("empty", 0, (1,), 0, 256), ("empty", 2, (-1,), 0, 256), ("cage", 0, (1, 2), 1000, 256), ("cage", 3, (4,), 2000, 256)]}


class Case:
    def __init__(self, vamp, oracle, robot, table):
        P = vamp.planning
        self.vamp, self.robot, self.mod = vamp, robot, getattr(vamp, robot)
        self.constraint = vamp.EEConstraint.upright((0, 0, 1), ANGLE)
        self.scenes = {k: Scene(oracle, robot, k) for k in ("empty", "cage")}
        raw = S.configs(robot, 96)
        self.problems = []
        for kind, s, goals, skip, max_samples in table:
            scene = self.scenes[kind]
            (rows,) = P.project_goals(self.mod, [raw], self.constraint, scene.env)
            start = rows[s]
            near = (start + np.float32(0.05) * S.ee_mask(robot)).astype(np.float32)  # a short step from the start, projected below
            (near,) = P.project_goals(self.mod, [near[None]], self.constraint, scene.env)
            gs = np.stack([near[0] if g < 0 else rows[g] for g in goals])
            self.problems.append(dict(scene=scene, start=start, goals=gs, skip=skip, max_samples=max_samples))

    def settings(self, p, **kw):
        return self.vamp.planning.RRTCMultiSettings(range=RANGE, max_iterations=1500, max_samples=p["max_samples"], **kw)

    def run(self, idx, constraint=None, **kw):
        """one call per max_samples value (a setting of the call), results in the order of idx"""
        P, out = self.vamp.planning, {}
        for m in sorted({self.problems[i]["max_samples"] for i in idx}):
            sub = [i for i in idx if self.problems[i]["max_samples"] == m]
            ps = [self.problems[i] for i in sub]
            got = P.rrtc_multi_constrained(self.mod, np.stack([p["start"] for p in ps]), [p["goals"] for p in ps],
                                           [p["scene"].env for p in ps], constraint or self.constraint, self.settings(ps[0], **kw),
                                           skips=[p["skip"] for p in ps])
            out.update(zip(sub, got))
        return [out[i] for i in idx]

    def expected(self, p):
        sc = p["scene"]
        return rrtc_constrained_serial(self.mod, p["start"], p["goals"], sc.lower, sc.span, sc.question, self.constraint, range_=RANGE,
                                       max_iterations=1500, max_samples=p["max_samples"], skip=p["skip"])

    def check_paths(self, got):
        """what a solved path promises; -> (tree-solved, direct) counts and the largest angle beyond the band at finer samples"""
        P, mod = self.vamp.planning, self.mod
        trees = direct = 0
        worst = -np.inf
        band = ANGLE + 1e-3
        moves = S.ee_mask(self.robot)
        c64 = S.upright((0.0, 0.0, 1.0), ANGLE)
        for p, g in zip(self.problems, got):
            if key(g)[0] != SOLVED:
                assert len(g.path) == 0 and g.goal_index == -1
                continue
            path = np.stack(g.path).astype(np.float32)
            assert path[0].tobytes() == p["start"].tobytes() and path[-1].tobytes() == p["goals"][g.goal_index].tobytes()
            trees, direct = trees + (len(path) > 2), direct + (len(path) == 2)
            valid, in_band = P.validate_paths_constrained(mod, [path], p["scene"].env, self.constraint)
            assert valid[0] and in_band[0] and P.validate_paths(mod, [path], [p["scene"].env])[0]
            assert mod.constraint_check_motion_batch(path[:-1], path[1:], self.constraint).all()
            assert all(p["scene"].question(a, b) for a, b in zip(path[:-1], path[1:]))
            # 4x finer float64 samples: between two passing samples h apart the tool axis turns by at most sum_j |u_j| h / 2
            # (u the edge's unit direction); the passing samples passed in fp32, 1.5 slack / sin(band) of angle away at most
            tol = 1.5 * 2.0 * float(np.abs(mod.eefk_batch(path).astype(np.float64) - K.frames44(self.robot, path.astype(np.float64))).max()) / np.sin(band)
            for x, y in zip(path[:-1].astype(np.float64), path[1:].astype(np.float64)):
                n_c = len(S.edge_samples32(x.astype(np.float32), y.astype(np.float32)))
                t = np.arange(4, 4 * n_c + 1) / (4.0 * n_c)
                cs = S.in_band(self.robot, x[None, :] + (y - x)[None, :] * t[:, None], c64)[1]["cs"]
                excess = float((np.arccos(np.clip(cs, -1.0, 1.0)) - band).max())
                length = np.linalg.norm(y - x)
                bound = (np.abs(y - x)[moves].sum() / length if length > 0 else 0.0) * (length / n_c) / 2
                worst = max(worst, excess)
                assert excess <= bound + tol, (excess, bound, tol)
        return trees, direct, worst


@pytest.fixture(scope="module")
def panda(vamp, oracle):
    c = Case(vamp, oracle, "panda", PANDA)
    c.got = c.run(list(range(len(PANDA))))
    return c


def test_panda_batch_equals_the_serial_statement(panda):
    want = [panda.expected(p) for p in panda.problems]
    for i, (g, w) in enumerate(zip(panda.got, want)):
        print(i, PANDA[i][0], "status", key(g)[0], "iterations", g.iterations, "size", g.size, "waypoints", len(g.path), "goal", g.goal_index)
        assert key(g) == key(w), (i, key(g)[:3], key(g)[4], key(w)[:3], key(w)[4])
        assert g.band_refused == w.band_refused, (i, g.band_refused, w.band_refused)
    print("questions", [w.questions for w in want], "of which the constraint refused", [w.band_refused for w in want])
    assert sum(w.band_refused for w in want) > 0
    # the call's totals ride on its first result: the questions of the eleven problems that share max_samples 256
    assert panda.got[0].edges_checked == sum(w.questions for i, w in enumerate(want) if PANDA[i][4] == 256)


def test_panda_paths_keep_their_promises(panda):
    trees, direct, worst = panda.check_paths(panda.got)
    print(f"panda: {trees} problems solved through the trees, {direct} by a direct edge; largest angle beyond the band at 4x finer "
          f"float64 samples {worst:.3e} rad")
    assert trees >= 4 and direct >= 2  # the floors: the test cannot pass on an empty set


def test_result_does_not_depend_on_the_batch_its_order_or_check_every(panda):
    n = len(PANDA)
    whole = [key(g) for g in panda.got]
    order = list(range(n))[::-1]
    assert [key(g) for g in panda.run(order)] == [whole[i] for i in order]
    for idx in ([3], [0, 6, 9], [4]):
        assert [key(g) for g in panda.run(idx)] == [whole[i] for i in idx]
    for every in (1, 3, 16):
        assert [key(g) for g in panda.run(list(range(n)), check_every=every)] == whole, every


def test_a_constraint_that_restricts_nothing_is_rrtc_multi_goals(panda):
    P, vamp = panda.vamp.planning, panda.vamp
    idx = [i for i in range(len(PANDA)) if PANDA[i][4] == 256]
    ps = [panda.problems[i] for i in idx]
    free = vamp.EEConstraint()  # infinite bounds, max_angle 0
    got = panda.run(idx, constraint=free)
    want = P.rrtc_multi_goals(panda.mod, np.stack([p["start"] for p in ps]), [p["goals"] for p in ps], [p["scene"].env for p in ps],
                              panda.settings(ps[0]), [p["skip"] for p in ps])
    assert [key(g) for g in got] == [key(w) for w in want]
    assert (got[0].validity_calls, got[0].edges_checked) == (want[0].validity_calls, want[0].edges_checked)
    assert any(len(w.path) > 2 for w in want)


def test_out_of_band_start_is_an_invalid_endpoint(panda):
    P = panda.vamp.planning
    ps = [panda.problems[i] for i in (0, 3, 6)]
    starts = np.stack([p["start"] for p in ps])
    raw = S.configs("panda", 4)
    assert not panda.mod.constraint_check_batch(raw[:1], panda.constraint)[0]
    starts[1] = raw[0]
    got = P.rrtc_multi_constrained(panda.mod, starts, [p["goals"] for p in ps], [p["scene"].env for p in ps], panda.constraint,
                                   panda.settings(ps[0]), skips=[p["skip"] for p in ps])
    assert got[1].status == "invalid_endpoint" and len(got[1].path) == 0 and got[1].goal_index == -1 and got[1].iterations == 0
    assert key(got[0]) == key(panda.got[0]) and key(got[2]) == key(panda.got[6])  # the others untouched
    alone = P.rrtc_multi_constrained(panda.mod, starts[1:2], [ps[1]["goals"]], [ps[1]["scene"].env], panda.constraint, panda.settings(ps[0]))
    assert alone[0].status == "invalid_endpoint" and alone[0].edges_checked == 0 and alone[0].validity_calls == 0  # 0 questions
    # out-of-band goals of a set are never used: the goal index still counts within the caller's set
    mixed = np.stack([raw[1], ps[1]["goals"][0]])
    (r,) = P.rrtc_multi_constrained(panda.mod, ps[1]["start"][None], [mixed], [ps[1]["scene"].env], panda.constraint, panda.settings(ps[0]))
    assert r.status == "solved" and r.goal_index == 1 and np.stack(r.path)[-1].tobytes() == mixed[1].tobytes()
    want = rrtc_constrained_serial(panda.mod, ps[1]["start"], mixed, ps[1]["scene"].lower, ps[1]["scene"].span, ps[1]["scene"].question,
                                   panda.constraint, range_=RANGE, max_iterations=1500, max_samples=256)
    assert key(r) == key(want) and want.status != INVALID_ENDPOINT


@pytest.mark.parametrize("robot", sorted(OTHERS))
def test_other_robots(vamp, oracle, robot):
    c = Case(vamp, oracle, robot, OTHERS[robot])
    got = c.run(list(range(len(OTHERS[robot]))))
    for i, (p, g) in enumerate(zip(c.problems, got)):
        w = c.expected(p)
        print(robot, i, "status", key(g)[0], "iterations", g.iterations, "size", g.size, "waypoints", len(g.path))
        assert key(g) == key(w) and g.band_refused == w.band_refused, (i, key(g)[:3], key(w)[:3])
    trees, direct, worst = c.check_paths(got)
    print(f"{robot}: {trees} through the trees, {direct} direct; largest angle beyond the band {worst:.3e} rad")
    assert trees + direct >= 1


def test_one_constraint_for_all_problems_equals_the_same_constraint_per_problem(vamp):
    """panda, three problems with 1, 2 and 1 goals, one obstacle sphere: the smallest call in which the endpoint test
    and the rounds read the records both ways (one for all; one per lane, expanded over goal sets of uneven size)"""
    mod, P = vamp.panda, vamp.planning
    constraint = vamp.EEConstraint.upright((0, 0, 1), ANGLE)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.55, 0.0, 0.6], 0.08))
    (rows,) = P.project_goals(mod, [S.configs("panda", 96)], constraint, env)
    assert len(rows) >= 7
    starts, goals, counts = rows[[0, 2, 5]], rows[[1, 3, 4, 6]], [1, 2, 1]
    s = P.RRTCMultiSettings(range=RANGE, max_iterations=1500, max_samples=256)
    once = mod.rrtc_multi_constrained_raw(starts, goals, counts, [env] * 3, constraint, s, skips=[0, 1000, 2000])
    each = mod.rrtc_multi_constrained_raw(starts, goals, counts, [env] * 3, [constraint] * 3, s, skips=[0, 1000, 2000])
    print("status", once["status"], "iterations", once["iterations"], "rounds", once["rounds"], "band_refused", once["band_refused"])
    assert (once["status"] != INVALID_ENDPOINT).all() and once["iterations"].max() > 0  # all take part, one grows its trees
    assert sorted(once) == sorted(each)
    for k in once:
        a, b = np.asarray(once[k]), np.asarray(each[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
