"""The generated prescreen of the self-collision half (tools/gen_hip.py: fkcc_self_prescreen, tape_error, prescreen_margin;
text in vamp_mvt_amd/csrc/gen/<robot>_dev.inc): the exact screen's groups, centres and table bits on bare trigonometry, with
every threshold widened by the margin the generator computes, and the Q_MAX rule in front.  The exact screen itself stays
the gates' own text.  The running-error bound the margins come from is checked as a bound, in float64."""
import os
import re

import numpy as np
import pytest

import self_gates

SCREENED = ["panda", "fetch"]
TERM = re.compile(r"any \|= (vmv::neg\(vmv::sql2_3\((.*?)\) - (\S+?)f\))(.*?);  // (\S+) vs\. (\S+?)(?:: (.*))?\n")
PROFILE = os.path.join(self_gates.ROOT, "profiles", "r33_bare_trig_error.txt")


def _body(text, start, end):
    s = text.index(start)
    return text[s:text.index(end, s)]


def _normalise(term):
    """op-tape values carry the prefix of the walk that emitted them (t12, p1_12, s12, f12): -> v12"""
    return re.sub(r"\b(?:p\d+_|t|s|f)(\d+)\b", r"v\1", term)


def _screens(robot):
    text = self_gates.generated_text(robot)
    exact = _body(text, "bool fkcc_self_screen(const float (&q)[kDim])", "return any;")
    fast = _body(text, "bool fkcc_self_prescreen(const float (&q)[kDim])", "return any;")
    return text, exact, fast


@pytest.mark.parametrize("robot", SCREENED)
def test_prescreen_has_the_exact_screens_terms_on_wider_thresholds(robot):
    g = self_gates.gen_hip()
    m = self_gates.model(robot)
    text, exact, fast = _screens(robot)
    e_terms, f_terms = TERM.findall(exact), TERM.findall(fast)
    assert len(e_terms) == len(f_terms) == len(m["self_groups"])
    assert fast.count("sql2_3") == len(m["self_groups"])
    assert "vsin" not in fast and "vcos" not in fast and "bare_sin" in fast and "bare_cos" in fast
    assert "slab" not in fast and "bad" not in fast
    _, centre_err = g.tape_error(m)
    by_pair = {(sg["a"], sg["b"]): sg for sg in m["self_groups"]}
    for (_, e_xyz, e_thr, e_bit, ea, eb, _), (_, f_xyz, f_thr, f_bit, fa, fb, note) in zip(e_terms, f_terms):
        assert (ea, eb) == (fa, fb), "same groups in the same order"
        assert _normalise(e_xyz) == _normalise(f_xyz), "the same bounding centres"
        assert e_bit == f_bit, "the same table-bit term"
        thr, thr_f = float.fromhex(e_thr), float.fromhex(f_thr)
        assert thr_f >= thr
        rs, delta = (float(v) for v in re.match(r"rs = (\S+), delta = (\S+) ", note).groups())
        assert f"BARE_TRIG_EPS = {g.BARE_TRIG_EPS!r}" in note
        # the reported margin is the generator's, and the threshold is its square rounded up
        want_rs, want_delta, want_thr = g.prescreen_margin(m, by_pair[(fa, fb)], centre_err)
        assert (rs, delta, thr_f) == (want_rs, want_delta, want_thr)
        assert float(np.float32(np.float32(rs) * np.float32(rs))) == thr, "rs is the gate's own sum of radii"
        t = (rs + delta) ** 2
        up = np.float32(t) if float(np.float32(t)) >= t else np.nextafter(np.float32(t), np.float32(np.inf))
        assert thr_f == float(up) and thr_f >= t
        env_bound = {x["link"]: x["bound"] for x in m["env_groups"]}
        sg = by_pair[(fa, fb)]
        e_sum = centre_err[sg["bound_a"]] + centre_err[env_bound[sg["b"]]]
        assert delta >= max(2.0 * e_sum, g.SELF_MARGIN)
    # every table word a term reads is loaded in the prescreen
    for name in set(re.findall(r"\b(tb\d+|tm)\b", " ".join(t[3] for t in f_terms))):
        assert re.search(rf"unsigned {name} = ", fast), name
    assert f"return {robot}::fkcc_self_prescreen(q);" in text


@pytest.mark.parametrize("robot", SCREENED)
def test_q_max_rule_once_per_joint(robot):
    g = self_gates.gen_hip()
    m = self_gates.model(robot)
    _, _, fast = _screens(robot)
    assert g.Q_MAX >= 4.0 * np.pi and float(np.float32(g.Q_MAX)) == g.Q_MAX
    rules = re.findall(r"any \|= !\(__builtin_fabsf\(q\[(\d+)\]\) <= (\S+)f\);", fast)
    assert [int(j) for j, _ in rules] == list(range(m["dimension"]))
    assert all(float.fromhex(v) == g.Q_MAX for _, v in rules)
    for lo, span in zip(m["lower"], m["span"]):
        assert max(abs(lo), abs(lo + span)) + np.pi / 2 <= g.Q_MAX
    # the rules stand before the first use of the bare trigonometry
    assert fast.rindex("__builtin_fabsf") < fast.index("bare_")


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch", "baxter"])
def test_exact_screen_is_still_the_gates_own_text(robot):
    """as tests/test_self_screen.py compares them: term by term against fkcc_self's gates, nothing of the prescreen in it"""
    text = self_gates.generated_text(robot)
    exact = _body(text, "bool fkcc_self_screen(const float (&q)[kDim])", "return any;")
    full = _body(text, "    fkcc_self(const float (&q)[kDim], vmv::lds_ptr slab, const vmv::lds_cptr radii_, const bool skip)",
                 "constexpr int kSelfPasses")
    gates = {(a, b): term for term, a, b in
             re.findall(r"const bool gate_\w+ = vmv::group_any<G>\((.*)\) && !bad(?: && VMV_ABLATE_SELF != 8)?;  // (\S+) vs\. (\S+)\n", full)}
    terms = re.findall(r"any \|= (.*);  // (\S+) vs\. (\S+)\n", exact)
    assert len(terms) == len(gates)
    for term, a, b in terms:
        assert _normalise(term) == _normalise(gates[(a, b)]), (a, b)
    assert "bare_" not in exact and "fmaf" not in exact and "fabsf" not in exact
    assert exact.count("vmv::vsin(") + exact.count("vmv::vcos(") > 0
    if robot not in SCREENED:
        assert "bool fkcc_self_prescreen(const float (&q)[kDim])\n    {\n        bool" not in text
        assert f"return {robot}::fkcc_self_screen(q);  // (no kSelfScreen" in text


@pytest.mark.parametrize("robot", SCREENED)
def test_running_error_bound_is_a_bound(robot):
    """4,096 configurations uniform in bounds, the tape in float64 with every sin / cos displaced by +-BARE_TRIG_EPS (random
    signs per operation and configuration, 8 draws): no bounding centre moves by more than its E_c"""
    g = self_gates.gen_hip()
    m = self_gates.model(robot)
    per_op, centre_err = g.tape_error(m)
    rng = np.random.default_rng(33)
    q = np.array(m["lower"]) + np.array(m["span"]) * rng.random((4096, m["dimension"]))
    base = g.eval_tape(m, q)
    trig = [i for i, (op, _, _) in enumerate(m["ops"]) if op in ("sin", "cos")]
    assert trig
    env_bound = {x["link"]: x["bound"] for x in m["env_groups"]}
    centres = sorted({sg["bound_a"] for sg in m["self_groups"]} | {env_bound[sg["b"]] for sg in m["self_groups"]})
    worst = np.zeros(len(centres))
    for _ in range(8):
        off = {i: g.BARE_TRIG_EPS * rng.choice([-1.0, 1.0], size=len(q)) for i in trig}
        moved = g.eval_tape(m, q, trig_offset=off)
        worst = np.maximum(worst, np.linalg.norm(moved[:, centres] - base[:, centres], axis=2).max(axis=0))
    for s, w in zip(centres, worst):
        print(robot, "centre", s, "moved", w, "bound", centre_err[s])
        assert w <= centre_err[s]
    assert worst.max() > 0.0
    assert all(M >= 0.0 and E >= 0.0 for M, E in per_op)


def test_bare_trig_eps_is_twice_the_measured_maximum_rounded_up():
    """profiles/r33_bare_trig_error.txt holds what vmv_bare_trig_error measured (tests/test_self_prescreen_gpu.py writes it)"""
    g = self_gates.gen_hip()
    with open(PROFILE) as f:
        rec = dict(re.findall(r"^(max_abs_\w+) (\S+)$", f.read(), re.M))
    worst = max(float(rec["max_abs_sin_diff"]), float(rec["max_abs_cos_diff"]))
    assert worst > 0.0
    assert g.BARE_TRIG_EPS >= 2.0 * worst
    digit, exp = f"{g.BARE_TRIG_EPS:.0e}".split("e")
    assert float(f"{digit}e{exp}") == g.BARE_TRIG_EPS, "one significant digit"
    step = 10.0 ** int(exp)
    assert g.BARE_TRIG_EPS - step < 2.0 * worst, "rounded up, not further"
