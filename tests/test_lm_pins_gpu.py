"""The four device kernels that run the damped least-squares iteration - ik_batch, cartesian_multi, project_batch and the
constraint round of rrtc_multi_constrained - against tests/golden/lm_parent.json, recorded on the MI355X from the commit before
the iteration was stated once (tools/make_lm_golden.py; the header names the commit): every small integer output and the
SHA-256 of every float output's bytes, bit for bit.  tests/lm_pins.py holds the cases.  A clear-text field that differs is
printed before the digests, so a failure reads as "ik_batch/full evaluations: lane 17: 9, parent 8"."""
import pytest

import lm_pins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    doc = lm_pins.load()
    assert doc["header"]["recorded_from"] and sorted(doc["robots"]) == sorted(lm_pins.ROBOTS)
    return doc["robots"]


@pytest.mark.parametrize("robot", lm_pins.ROBOTS)
def test_the_loops_give_the_parents_bits(vamp, golden, robot):
    want = golden[robot]
    got = lm_pins.compute(vamp, robot)
    # the pin is not vacuous: lanes that converge and lanes that do not, a rejected step's schedule (ik_failed after two
    # evaluations), the non-finite rows, and the round kernel reached by problems that go through the trees
    full = want["ik_batch/full"]
    assert "1" in full["converged"] and "0" in full["converged"] and len(full["converged"]) == 32 * lm_pins.IK_TARGETS
    spoiled = 32 * lm_pins.IK_SPOILED[0] + lm_pins.IK_SPOILED[1]
    assert want["ik_batch/spoiled_seed"]["converged"][spoiled] == "0" and want["ik_batch/spoiled_seed"]["evaluations"][spoiled] == 0
    assert "ik_failed" in want["cartesian_multi/two_iterations"]["status"] and "complete" in want["cartesian_multi/full"]["status"]
    for name in lm_pins.NAMES:
        for layout in ("shared", "per_lane"):
            call = want[f"project_batch/{name}/{layout}"]
            assert call["converged"][lm_pins.NONFINITE_ROW] == "0" and call["evaluations"][lm_pins.NONFINITE_ROW] == 0
            assert max(call["evaluations"]) > 1 and "1" in call["converged"]
    assert max(want["rrtc_multi_constrained"]["iterations"]) > 0
    bad = lm_pins.differences(want, got)
    print("\n".join(bad))
    assert not bad, f"{robot}: {len(bad)} fields differ from the parent's; the first: {bad[0]}"
