"""planning.aorrtc_multi_constrained / vmv_aorrtc_multi_constrained on the device.

Expected results come from tests/aorrtc_constrained_serial.py: aorrtc_serial's meta loop and search with
rrtc_constrained_serial for the first solution, simplify_constrained_serial for every simplification, the CPU oracle
answering validity and the product's batch calls answering the constraint one question at a time.  Per problem the status,
iterations, searches, improvements, the bytes of first_cost and cost, the tree sizes, every waypoint bit and band_refused
are compared; the result must not depend on the batch, its order or check_every; a constraint that restricts nothing gives
aorrtc_multi's bytes; without `optimize` the call is rrtc_multi_constrained then simplify_multi_constrained.  Endpoints come
from planning.project_goals under upright(z, 0.2).  The statement asks the device one question at a time, so the budgets are
small: a problem asks about 1,500 questions in all."""
import numpy as np
import pytest

import constraint_serial as S
from aorrtc_constrained_serial import INVALID_ENDPOINT, aorrtc_constrained_serial
from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED
from simplify_serial import cost
from test_rrtc_multi_gpu import Scene

pytestmark = pytest.mark.gpu
ANGLE = 0.2
BASE = dict(range=0.5, max_samples=256, max_iterations=1200, max_internal_iterations=200, max_searches=3, max_cost_bound_resamples=2)
STATUS = {"solved": SOLVED, "max_iterations": MAX_ITERATIONS, "max_samples": MAX_SAMPLES, "invalid_endpoint": INVALID_ENDPOINT}
# (scene, start row, goal row, skip, settings of the problem's own): rows index the projected, collision-free Halton
# configurations of the robot; goal row -1 = a short step from the start, projected again (solved by a direct edge).  The
# pairs and skips are pinned: DESIGN.md 5s records what each problem does on the MI355X.
PANDA = [("empty", 0, 1, 0, {}), ("empty", 2, 3, 1000, {}), ("empty", 2, 4, 1000, {}), ("empty", 7, -1, 0, {}),
         ("cage", 8, 9, 2500, {}), ("cage", 5, 7, 1500, {}), ("cage", 2, 3, 500, {}), ("cage", 5, 6, 1500, {})]
OTHERS = {"ur5": [("empty", 0, 1, 0, {}), ("empty", 1, 2, 500, {}), ("cage", 3, 4, 2000, {})],
          "baxter": [("empty", 0, 1, 0, {}), ("cage", 0, 1, 1000, {}), ("cage", 0, 2, 1000, {})]}
FULL_POOL = ("empty", 2, 3, 1000, dict(max_samples=64, max_internal_iterations=600, max_searches=2))


def key(r):
    """what must not depend on the rest of the batch; a device result and a serial one give the same tuple"""
    return (r.status if isinstance(r.status, int) else STATUS[r.status], int(r.iterations), int(r.searches), int(r.improvements),
            np.float32(r.first_cost).tobytes(), np.float32(r.cost).tobytes(), list(r.size),
            [np.asarray(q, np.float32).tobytes() for q in r.path], int(getattr(r, "band_refused", 0)))  # (aorrtc_multi's: none)


class Case:
    def __init__(self, vamp, oracle, robot, table):
        P = vamp.planning
        self.vamp, self.robot, self.mod = vamp, robot, getattr(vamp, robot)
        self.constraint = vamp.EEConstraint.upright((0, 0, 1), ANGLE)
        self.scenes = {k: Scene(oracle, robot, k) for k in sorted({row[0] for row in table})}
        raw = S.configs(robot, 96)
        self.problems = []
        for kind, s, g, skip, own in table:
            scene = self.scenes[kind]
            (rows,) = P.project_goals(self.mod, [raw], self.constraint, scene.env)
            start = rows[s]
            if g < 0:  # a short step from the start, projected
                near = (start + np.float32(0.05) * S.ee_mask(robot)).astype(np.float32)
                (near,) = P.project_goals(self.mod, [near[None]], self.constraint, scene.env)
                goal = near[0]
            else:
                goal = rows[g]
            self.problems.append(dict(scene=scene, start=start, goal=goal, skip=skip, own=dict(own)))

    def settings(self, p, **kw):
        return self.vamp.planning.AORRTCMultiSettings(**{**BASE, **p["own"], **kw})

    def run(self, idx, constraint=None, starts=None, unconstrained=False, **kw):
        """one call per distinct set of a problem's own settings (they are settings of the call), results in the order of idx;
        self.totals: (rounds, questions) summed over those calls"""
        P, out = self.vamp.planning, {}
        self.totals = [0, 0]
        for own in sorted({tuple(sorted(self.problems[i]["own"].items())) for i in idx}):
            sub = [i for i in idx if tuple(sorted(self.problems[i]["own"].items())) == own]
            ps = [self.problems[i] for i in sub]
            a = np.stack([p["start"] if starts is None else starts[i] for i, p in zip(sub, ps)])
            b, es, sk = np.stack([p["goal"] for p in ps]), [p["scene"].env for p in ps], [p["skip"] for p in ps]
            if unconstrained:
                got = P.aorrtc_multi(self.mod, a, b, es, self.settings(ps[0], **kw), sk)
            else:
                got = P.aorrtc_multi_constrained(self.mod, a, b, es, constraint or self.constraint, self.settings(ps[0], **kw), skips=sk)
            self.totals[0] += got[0].validity_calls
            self.totals[1] += got[0].edges_checked
            out.update(zip(sub, got))
        return [out[i] for i in idx]

    def expected(self, p, **kw):
        sc, s = p["scene"], self.settings(p, **kw)
        return aorrtc_constrained_serial(self.mod, p["start"], p["goal"], sc.lower, sc.span, sc.question, self.constraint,
                                         range_=s.range, balance=s.balance, tree_ratio=s.tree_ratio, max_iterations=s.max_iterations,
                                         max_internal_iterations=s.max_internal_iterations, max_samples=s.max_samples,
                                         max_cost_bound_resamples=s.max_cost_bound_resamples, max_searches=s.max_searches,
                                         optimize=s.optimize, cost_bound_resample=s.cost_bound_resample,
                                         simplify_intermediate=s.simplify_intermediate, skip=p["skip"])

    def check(self, got, want, revalidate=False):
        """test 1's checks.  revalidate: every edge of every path also by the oracle and by constraint_check_motion_batch -
        only where simplify_intermediate is off: simplify() subdivides without asking the halves of an edge again
        (test_aorrtc_multi_gpu.check gives the reason for validity, DESIGN 5p for the band)"""
        assert len(got) == len(want) == len(self.problems)
        for i, (p, g, w) in enumerate(zip(self.problems, got, want)):
            kg, kw = key(g), key(w)
            print(self.robot, i, p["scene"].kind, p["skip"], "device", kg[:4], g.first_cost, g.cost, kg[6], kg[8], "waypoints", len(g.path),
                  "| serial", kw[:4], w.first_cost, w.cost, kw[6], kw[8], "searches", w.search_status, "refused in them", w.search_refused_each,
                  "re-parents", w.reparents, "questions", w.questions)
            assert kg == kw, (self.robot, i, kg[:7], kg[8], kw[:7], kw[8])
            if w.solved:
                path = np.stack(g.path).astype(np.float32)
                assert path[0].tobytes() == p["start"].tobytes() and path[-1].tobytes() == p["goal"].tobytes()
                assert g.cost <= g.first_cost and np.float32(g.cost).tobytes() == np.float32(cost(list(path))).tobytes()
                if revalidate:
                    assert all(p["scene"].question(a, b) for a, b in zip(path[:-1], path[1:])), i
                    assert self.mod.constraint_check_motion_batch(path[:-1], path[1:], self.constraint).all(), i
            else:
                assert len(g.path) == 0 and g.cost == float("inf") and g.first_cost == float("inf") and g.searches == 0


@pytest.fixture(scope="module")
def panda(vamp, oracle):
    c = Case(vamp, oracle, "panda", PANDA)
    c.got = c.run(list(range(len(PANDA))))
    c.got_totals = tuple(c.totals)
    c.want = [c.expected(p) for p in c.problems]
    return c


def test_panda_batch_equals_the_serial_statement(panda):
    panda.check(panda.got, panda.want)
    want = panda.want
    # coverage, on the statement's own counters: the test cannot pass on problems that never reach the new code
    # (the floors above 1: half of what the statement shows on the MI355X - 5, 121, 7 and 1,663)
    assert sum(w.improvements > 0 for w in want) >= 2                          # searches solved and kept
    assert sum(w.reparents for w in want) >= 60                                # accepted re-parents
    assert sum(st == MAX_ITERATIONS for w in want for st in w.search_status) >= 3  # searches that ended at their budget
    assert sum(w.search_refused for w in want) >= 831                          # searches' questions refused by the band
    assert sum(w.solved and w.searches == 0 and len(w.first_path) == 2 for w in want) >= 1  # ends after stage 1 on 2 waypoints
    # the call's totals: at least the first stage's and the searches' questions (the simplifier asks whole windows)
    assert panda.got_totals[1] >= sum(w.questions - w.simplify_questions for w in want) and panda.got_totals[0] > 0


def test_search_paths_are_valid_and_in_band(panda):
    """simplify_intermediate off: what the searches themselves return, re-validated edge by edge"""
    got = panda.run(list(range(len(PANDA))), simplify_intermediate=False)
    want = [panda.expected(p, simplify_intermediate=False) for p in panda.problems]
    panda.check(got, want, revalidate=True)
    assert sum(w.searches > 0 for w in want) >= 1 and sum(len(w.path) > 2 for w in want) >= 1


def test_result_does_not_depend_on_the_batch_its_order_or_check_every(panda):
    n = len(PANDA)
    whole = [key(g) for g in panda.got]
    order = list(range(n))[::-1]
    assert [key(g) for g in panda.run(order)] == [whole[i] for i in order]
    for idx in ([0, 4, 6], [1, 5], *[[i] for i in range(n)]):
        assert [key(g) for g in panda.run(idx)] == [whole[i] for i in idx], idx
    for every in (1, 3, 16):
        assert [key(g) for g in panda.run(list(range(n)), check_every=every)] == whole, every


def test_a_constraint_that_restricts_nothing_is_aorrtc_multi(panda):
    idx = list(range(len(PANDA)))
    free = panda.vamp.EEConstraint()  # infinite bounds, max_angle 0
    got = panda.run(idx, constraint=free)
    totals = tuple(panda.totals)
    want = panda.run(idx, unconstrained=True)
    assert totals == tuple(panda.totals)  # rounds and questions
    for g, w in zip(got, want):
        assert g.band_refused == 0 and key(g) == key(w)
    assert any(w.searches > 0 for w in want) and any(len(w.path) > 2 for w in want)


def test_without_optimize_it_is_rrtc_multi_constrained_then_simplify_multi_constrained(panda):
    P, mod = panda.vamp.planning, panda.mod
    ps = panda.problems
    got = panda.run(list(range(len(ps))), optimize=False)
    first = P.rrtc_multi_constrained(mod, np.stack([p["start"] for p in ps]), [p["goal"][None] for p in ps], [p["scene"].env for p in ps],
                                     panda.constraint, P.RRTCMultiSettings(range=BASE["range"], max_iterations=BASE["max_iterations"],
                                                                           max_samples=BASE["max_samples"]),
                                     skips=[p["skip"] for p in ps])
    solved = [i for i, r in enumerate(first) if r.solved]
    simplified = P.simplify_multi_constrained(mod, [first[i].path for i in solved], [ps[i]["scene"].env for i in solved], panda.constraint)
    assert len(solved) >= 2
    refused = [r.band_refused for r in first]
    for i, r in zip(solved, simplified):
        path = first[i].path if r.status == "out_of_band" else r.path
        assert [q.tobytes() for q in got[i].path] == [np.asarray(q, np.float32).tobytes() for q in path]
        assert np.float32(got[i].cost).tobytes() == np.float32(cost(list(path))).tobytes() == np.float32(got[i].first_cost).tobytes()
        refused[i] += r.band_refused
    for i, r in enumerate(first):
        assert (got[i].status, got[i].iterations, got[i].size, got[i].searches, got[i].improvements) == (r.status, r.iterations, r.size, 0, 0)
        assert got[i].band_refused == refused[i]
        if i not in solved:
            assert len(got[i].path) == 0 and got[i].cost == float("inf")


def test_out_of_band_start_is_an_invalid_endpoint(panda):
    idx = [0, 4, 5]
    raw = S.configs("panda", 4)
    assert not panda.mod.constraint_check_batch(raw[:1], panda.constraint)[0]
    starts = {i: panda.problems[i]["start"] for i in idx}
    starts[4] = raw[0]
    got = panda.run(idx, starts=starts)
    bad = got[1]
    assert bad.status == "invalid_endpoint" and len(bad.path) == 0 and bad.iterations == 0 and bad.searches == 0 and bad.band_refused == 0
    assert bad.cost == float("inf") and bad.first_cost == float("inf")
    assert key(got[0]) == key(panda.got[0]) and key(got[2]) == key(panda.got[5])  # the others untouched
    alone = panda.run([4], starts=starts)
    assert alone[0].status == "invalid_endpoint" and tuple(panda.totals) == (0, 0)  # no round, no question


@pytest.mark.parametrize("robot", sorted(OTHERS))
def test_other_robots(vamp, oracle, robot):
    """6 joints (n + 2 even: no surplus Gaussian) and 14.  Baxter's three problems run 9 searches in the statement (floor 4).
    UR5's do not reach a search under this constraint: of 16 pairs tried on the MI355X, at max_samples 256 and 1,024, every
    one is solved by its direct edge or fills the pool in the first stage (DESIGN.md 5o saw the same of rrtc_multi_constrained),
    so UR5 checks the first stage's hand-over and the 2-waypoint end only."""
    c = Case(vamp, oracle, robot, OTHERS[robot])
    got = c.run(list(range(len(OTHERS[robot]))))
    want = [c.expected(p) for p in c.problems]
    c.check(got, want)
    assert sum(w.searches for w in want) >= {"baxter": 4, "ur5": 0}[robot]


def test_full_pool(vamp, oracle):
    """64 nodes: a march meets the full pool"""
    c = Case(vamp, oracle, "panda", [FULL_POOL])
    got = c.run([0])
    want = [c.expected(p) for p in c.problems]
    c.check(got, want)
    assert MAX_SAMPLES in want[0].search_status and sum(want[0].size) == 64  # a search ended on the full pool
