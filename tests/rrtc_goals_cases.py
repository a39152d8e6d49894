"""The problems, settings and comparisons tests/test_rrtc_goals.py (no device) and tests/test_rrtc_goals_gpu.py share —
TEST INFRASTRUCTURE ONLY.  Expected results come from the serial statement (tests/rrtc_goals_serial.py) with the CPU
oracle answering every question; `Scene` is test_rrtc_multi_gpu.py's."""
from __future__ import annotations

import numpy as np

from oracle_lib import CAGE_GOAL, CAGE_START
from rrtc_goals_serial import rrtc_goals_serial
from rrtc_serial import MAX_ITERATIONS, MAX_SAMPLES, SOLVED
from test_rrtc_multi_gpu import Scene  # noqa: F401  (re-exported)

STATUS = {"solved": SOLVED, "max_iterations": MAX_ITERATIONS, "max_samples": MAX_SAMPLES}
REFERENCE_DOMAIN = dict(dynamic_domain=True, radius=4.0, alpha=0.0001, min_radius=1.0)  # rrtc_settings.hh
TIGHT_DOMAIN = dict(dynamic_domain=True, radius=2.0, alpha=0.05, min_radius=1.5)        # every event occurs, the clamp included
# the sphere cage, CAGE_START -> CAGE_GOAL, max_samples 8192, balance on, ratio 1:
# domain, range, skip, max_iterations -> status, iterations, size, questions
DOMAIN_TABLE = [
    (REFERENCE_DOMAIN, 1.0, 0, 100000, SOLVED, 1486, [54, 108], 1289),
    (REFERENCE_DOMAIN, 1.0, 1000, 100000, SOLVED, 433, [26, 18], 326),
    (REFERENCE_DOMAIN, 1.0, 3000, 100000, SOLVED, 476, [30, 21], 376),
    (REFERENCE_DOMAIN, 0.25, 1000, 100000, SOLVED, 784, [164, 103], 898),
    (TIGHT_DOMAIN, 0.25, 2000, 6000, SOLVED, 4252, [146, 168], 880),
    (TIGHT_DOMAIN, 1.0, 1000, 6000, MAX_ITERATIONS, 6000, [82, 42], 566),
]
DOMAIN_EVENTS = {0: dict(reject=357, grow=121, set=130, shrink=843, clamp=0),
                 5: dict(reject=5557, grow=89, set=113, shrink=207, clamp=4)}
SERIAL_KEYS = ("range", "balance", "tree_ratio", "max_iterations", "max_samples", "dynamic_domain", "radius", "alpha", "min_radius",
               "start_tree_first")


def settings_dict(**kw):
    s = dict(range=1.0, balance=True, tree_ratio=1.0, max_iterations=3000, max_samples=8192, check_every=0, dynamic_domain=False,
             radius=4.0, alpha=0.0001, min_radius=1.0, start_tree_first=False)
    s.update(kw)
    return s


class Problem:
    def __init__(self, scene, start, goals, skip):
        self.scene, self.skip = scene, int(skip)
        self.start, self.goals = np.array(start, np.float32), np.array(goals, np.float32)
        assert self.goals.ndim == 2

    def expected(self, settings):
        s = {k: settings[k] for k in SERIAL_KEYS}
        return rrtc_goals_serial(self.start, self.goals, self.scene.lower, self.scene.span, self.scene.question,
                                 range_=s.pop("range"), skip=self.skip, **s)


def key(result):
    """what must not depend on the rest of the batch: status, iterations, size, the waypoints' bits and the goal"""
    return (result.status if isinstance(result.status, int) else STATUS[result.status], int(result.iterations),
            list(result.size), [np.asarray(q, np.float32).tobytes() for q in result.path], int(result.goal_index))


def check(problems, got, want):
    assert len(got) == len(want) == len(problems)
    for i, (p, g, w) in enumerate(zip(problems, got, want)):
        assert key(g) == key(w), (i, p.scene.kind, p.skip, key(g)[:3], key(g)[4], key(w)[:3], key(w)[4])
        check_path(p, g, i)


def check_path(p, g, i=0):
    """a solved result runs from the start's bits to the bits of the goal it names, valid under the oracle edge by edge"""
    if len(g.path) == 0:
        assert g.goal_index == -1, i
        return
    assert 0 <= g.goal_index < len(p.goals), i
    assert np.asarray(g.path[0], np.float32).tobytes() == p.start.tobytes(), i
    assert np.asarray(g.path[-1], np.float32).tobytes() == p.goals[g.goal_index].tobytes(), i
    assert all(p.scene.question(a, b) for a, b in zip(g.path[:-1], g.path[1:])), i


def domain_problem(scene, row):
    """(the problem, its settings) of a DOMAIN_TABLE row"""
    domain, range_, skip, max_iterations = DOMAIN_TABLE[row][:4]
    return Problem(scene, CAGE_START, [CAGE_GOAL], skip), settings_dict(range=range_, max_iterations=max_iterations, **domain)


GOAL_SET_SETTINGS = settings_dict(max_iterations=3000, **TIGHT_DOMAIN)


def goal_set_problems(cage, n=17):
    """n problems from CAGE_START in the sphere cage with 2 .. 5 goals each (unequal within the batch): valid
    configurations drawn as Scene.valid_pairs draws them, and the cage's own goal appended to every other set"""
    a, b = cage.valid_pairs(40, 23)
    pool, at, out = np.concatenate([a, b]), 0, []
    for k in range(n):
        count = 2 + k % 4
        drawn = count - 1 if k % 2 == 0 else count
        goals = list(pool[at:at + drawn])
        at += drawn
        if k % 2 == 0:
            goals.append(np.array(CAGE_GOAL, np.float32))
        out.append(Problem(cage, CAGE_START, goals, 100 * k))
    return out


def classes_of(problems, want):
    """which of the cases the goal-set batch must hold each problem is"""
    out = []
    for p, w in zip(problems, want):
        if w.solved and w.iterations == 0:
            out.append("direct_later" if w.goal_index > 0 else "direct_first")
        elif w.solved:
            out.append("tree_later" if w.goal_index > 0 else "tree_first")
        else:
            out.append("unsolved")
    return out
