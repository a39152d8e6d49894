"""The reach rule of tools/experiments/fine_reach_study.py (a fine sphere is tested against a candidate only if the
candidate's surface lies within the sphere's reach from the gate's centre), the parts its count rests on.  The rule is
studied, not built ("pruning by reach"); these tests keep the study's figures honest.

Certificate: for Panda and UR5, every gate of the primitive-only walk and every fine sphere, the oracle's fp32 FK keeps
|c_s - c_gate| + r_s at least 1e-6 m below the tabulated reach, over 2,000 configurations of which a third lie 2.5 x
outside the joint bounds; the spheres stand in non-increasing reach; the class sizes are what the thresholds imply.
Count: on 32 waves of 64 uniform configurations against shell64, no rule (one threshold, three, exact per entry)
drops an (item, primitive) pair whose exact predicate is negative, of more than 1,000 such pairs."""
import importlib.util
import os

import numpy as np
import pytest

import self_gates

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ROBOTS = ["panda", "ur5"]


def _study():
    spec = importlib.util.spec_from_file_location("fine_reach_study", os.path.join(ROOT, "tools", "experiments", "fine_reach_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("robot", ROBOTS)
def test_reach_holds_under_fp32_fk_and_orders_the_spheres(oracle, robot):
    study = _study()
    g, m = self_gates.gen_hip(), self_gates.model(robot)
    gates = study.fine_reach(g, m)
    assert [x["link"] for x in gates] == [x["link"] for x in g.merged_groups(m)]
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    q = (lo + span * np.random.default_rng(2024).random((2000, len(lo)), dtype=np.float32)).astype(np.float32)
    q[::3] *= np.float32(2.5)
    S = np.stack([oracle.fk_all(rid, c) for c in q]).astype(np.float64)  # fp32 centres, exact in float64
    R = np.array(m["radii"], np.float64)
    for gate, grp in zip(gates, g.merged_groups(m)):
        assert sorted(gate["order"]) == sorted(grp["fine"]) and gate["bound"] == grp["bound"]
        reach = np.array(gate["reach"])
        assert np.all(np.diff(reach) <= 0)
        assert reach[0] <= grp["radius"] + 1e-5  # the gate's own radius encloses the farthest sphere
        d = np.linalg.norm(S[:, gate["order"], :3] - S[:, [gate["bound"]], :3], axis=2) + R[gate["order"]][None, :]
        worst = (d - reach[None, :]).max()
        assert worst <= -1e-6, (robot, gate["link"], worst)


def test_class_sizes_are_what_the_thresholds_imply():
    study = _study()
    reach = [0.176, 0.176, 0.171, 0.121, 0.109, 0.109, 0.086, 0.086, 0.078, 0.078, 0.074, 0.074]
    taus, S = study.reach_classes(reach, (6, 4, 3))
    assert taus == [0.086 + study.MARGIN, 0.109 + study.MARGIN, 0.121 + study.MARGIN] and S == [12, 6, 4, 3]
    assert study.reach_classes(reach, ()) == ([], [12])
    taus, S = study.reach_classes(reach, (5,))  # a cut inside a tie excludes the whole tie
    assert S == [12, 4]
    for t, s in zip(taus, S[1:]):
        assert s == sum(1 for r in reach if r + study.MARGIN > t)
    d = np.array([0.05, 0.0860, 0.0863, 0.1090, 0.1093, 0.15])
    taus, S = study.reach_classes(reach, (6, 4, 3))
    assert study.candidate_class(taus, d).tolist() == [0, 0, 1, 1, 2, 3]
    with pytest.raises(AssertionError):
        study.reach_classes(reach, (3, 4))  # thresholds must ascend


def test_no_rule_drops_a_hit_on_the_bench_scene(oracle):
    study = _study()
    waves = 32
    _, _, gates, units, chunk = study.sample("panda", waves)
    slots = chunk * study.WAVE
    rules = {"exact": lambda gi: (lambda d, r=np.array(gates[gi]["reach"]): (r[None, :] + study.MARGIN > np.asarray(d)[:, None]).sum(1)
                                  if len(d) else np.zeros(0, int))}
    for n_thr in (1, 3):
        cuts = [study.choose_cuts(units[gi], g["reach"], n_thr, chunk, slots) for gi, g in enumerate(gates)]
        assert any(cuts), "no gate takes a class"

        def rule(gi, cuts=cuts):
            taus, S = study.reach_classes(gates[gi]["reach"], cuts[gi])
            S = np.array(S)
            return lambda d: S[study.candidate_class(taus, d)]
        rules[f"{n_thr} thresholds"] = rule
    today, _ = study.evaluate(gates, units, lambda gi: (lambda d, n=len(gates[gi]["order"]): np.full(len(d), n, int)), chunk)
    print("today: hits per wave", today["hits"] / waves, "pairs", today["pairs"] / waves, "rounds", today["rounds"] / waves)
    assert today["hits"] > 1000 and today["lost"] == 0
    for name, rule in rules.items():
        tot, _ = study.evaluate(gates, units, rule, chunk)
        print(name, "pairs per wave", tot["pairs"] / waves, "rounds", tot["rounds"] / waves, "hits lost", tot["lost"], "of", tot["hits"])
        assert tot["hits"] == today["hits"] and tot["lost"] == 0, name
        assert tot["pairs"] < today["pairs"] and tot["rounds"] < today["rounds"], name
