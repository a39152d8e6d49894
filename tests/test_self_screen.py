"""The generated screen of the self-collision half (tools/gen_hip.py: fkcc_self_screen, kSelfScreen; text in
vamp_mvt_amd/csrc/gen/<robot>_dev.inc): one gate term per self-collision group, each the very text of that group's gate in
fkcc_self (so, built with -ffp-contract=off, the same bits) including its table-bit term, and kSelfScreen as decided by the
sampled any-gate rate with the generated tables applied."""
import re

import pytest

import self_gates

ROBOTS = ["panda", "ur5", "fetch", "baxter"]


def _body(text, start, end):
    s = text.index(start)
    return text[s:text.index(end, s)]


def _normalise(term):
    """op-tape values carry the prefix of the walk that emitted them (t12, p1_12, s12): -> v12"""
    return re.sub(r"\b(?:p\d+_|t|s)(\d+)\b", r"v\1", term)


@pytest.mark.parametrize("robot", ROBOTS)
def test_screen_has_every_groups_gate_once(robot):
    m = self_gates.model(robot)
    text = self_gates.generated_text(robot)
    two, multi = self_gates.tables(robot, m, text)
    screen = _body(text, "bool fkcc_self_screen(const float (&q)[kDim])", "return any;")
    terms = re.findall(r"any \|= (.*);  // (\S+) vs\. (\S+)\n", screen)
    assert len(terms) == len(m["self_groups"])
    assert sorted((a, b) for _, a, b in terms) == sorted((g["a"], g["b"]) for g in m["self_groups"])
    assert screen.count("sql2_3") == len(m["self_groups"])  # no second formula next to the terms
    assert "bad" not in screen and "slab" not in screen

    # the gates of fkcc_self, by group
    full = _body(text, "    fkcc_self(const float (&q)[kDim], vmv::lds_ptr slab, const vmv::lds_cptr radii_, const bool skip)",
                 "constexpr int kSelfPasses")
    gates = {(a, b): term for term, a, b in
             re.findall(r"const bool gate_\w+ = vmv::group_any<G>\((.*)\) && !bad(?: && VMV_ABLATE_SELF != 8)?;  // (\S+) vs\. (\S+)\n", full)}
    assert len(gates) == len(m["self_groups"])
    # the table-bit term each group must carry: the multi-joint bits ride above the 8 bits of the first two-joint word
    want_bit = {}
    for ti, t in enumerate(two):
        for bit, gi in enumerate(t["groups"]):
            want_bit[gi] = f" && ((tb{ti} >> {bit}) & 1u) != 0u"
    for k, t in enumerate(multi):
        want_bit[t["group"]] = f" && ((tb0 >> {8 + k}) & 1u) != 0u" if two else f" && ((tm >> {k}) & 1u) != 0u"
    for term, a, b in terms:
        assert _normalise(term) == _normalise(gates[(a, b)]), (a, b)
        (gi,) = [i for i, g in enumerate(m["self_groups"]) if (g["a"], g["b"]) == (a, b)]
        if gi in want_bit:
            assert term.endswith(want_bit[gi]), (a, b, term)
        else:
            assert ">>" not in term and term.endswith(")") and "&&" not in term, (a, b, term)
    # every table word a term reads is loaded in the screen
    for name in set(re.findall(r"\b(tb\d+|tm)\b", " ".join(t for t, _, _ in terms))):
        assert re.search(rf"unsigned {name} = ", screen), name


@pytest.mark.parametrize("robot", ROBOTS)
def test_screen_is_on_where_few_configurations_fire_a_gate(robot):
    g = self_gates.gen_hip()
    m = self_gates.model(robot)
    text = self_gates.generated_text(robot)
    two, multi = self_gates.tables(robot, m, text)
    _, rate = g.gate_rates(m, tables=two, multi=multi, any_rate=True)  # the generator's sample, the generated tables
    on = re.search(r"constexpr bool kSelfScreen = (true|false);", text).group(1) == "true"
    print(robot, "some gate fires for", rate, "of uniform configurations; screen", on)
    assert on == (rate < g.SELF_SCREEN_MAX_RATE)
    assert abs(rate - g.SELF_SCREEN_MAX_RATE) > 0.05, "too close to the threshold for a sampled rate to decide"
    assert f"static constexpr bool kSelfScreen = {robot}::kSelfScreen;" in text
    if robot in ("panda", "fetch"):
        assert on
    if robot == "ur5":
        assert not on
