#!/usr/bin/env python3
"""Records tests/golden/lm_parent.json: the outputs of ik_batch, cartesian_multi, project_batch and rrtc_multi_constrained
on the cases of tests/lm_pins.py, from the library that is loaded (the in-tree one, or VMV_LIBRARY), on the GPU.  The small
integer outputs stand in clear, every float output as the SHA-256 of its raw bytes.  Public Python API only, so it runs on
any commit that has the four calls: the fixture is recorded from the commit BEFORE a change to the shared iteration
(csrc/vmv_robot_tu.inc: lm_start, lm_accept, lm_step) and then holds the changed build to it (tests/test_lm_pins_gpu.py).
A digest that differs means an operation changed: find it, do not record again.

usage: tools/make_lm_golden.py --recorded-from "commit 8d0713d" [--out FILE]     write the fixture
       tools/make_lm_golden.py --check                                           compare the loaded library with it"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
MAX_FIXTURE_BYTES = 64 * 1024


def dumps(doc):
    """one line per call: the file reads and diffs by call"""
    lines = ["{", ' "header": ' + json.dumps(doc["header"]) + ",", ' "robots": {']
    robots = list(doc["robots"])
    for robot in robots:
        lines.append(f'  "{robot}": {{')
        calls = doc["robots"][robot]
        lines += [f'   "{call}": ' + json.dumps(calls[call], separators=(",", ":")) + ("," if i + 1 < len(calls) else "")
                  for i, call in enumerate(calls)]
        lines.append("  }" + ("," if robot != robots[-1] else ""))
    return "\n".join(lines + [" }", "}"]) + "\n"


def main():
    import lm_pins
    import vamp_mvt_amd as vamp

    ap = argparse.ArgumentParser()
    ap.add_argument("--recorded-from", default=None, help="the commit whose build is loaded, as the header states it")
    ap.add_argument("--out", default=lm_pins.FIXTURE)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if vamp.device_count() < 1:
        raise SystemExit("make_lm_golden.py needs a GPU: the calls have no CPU path")
    vamp.set_device(0)
    robots = {robot: lm_pins.compute(vamp, robot) for robot in lm_pins.ROBOTS}
    if args.check:
        want = lm_pins.load()["robots"]
        bad = [f"{robot}: {line}" for robot in lm_pins.ROBOTS for line in lm_pins.differences(want[robot], robots[robot])]
        print("\n".join(bad) if bad else "the loaded library gives the fixture bit for bit")
        sys.exit(1 if bad else 0)
    if not args.recorded_from:
        raise SystemExit("--recorded-from is required: the header states which commit's build the fixture holds")
    header = dict(tool="tools/make_lm_golden.py", recorded_from=args.recorded_from, cases="tests/lm_pins.py", floats="SHA-256 of the raw little-endian bytes")
    text = dumps(dict(header=header, robots=robots))
    assert json.loads(text)["robots"] == robots and len(text) <= MAX_FIXTURE_BYTES, len(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(f"{args.out}: {len(text)} bytes")
    for robot, calls in robots.items():
        rows = [c["antiparallel_row"] for k, c in calls.items() if k.endswith("per_lane")]
        stuck = [calls[k]["converged"][r] == "0" and calls[k]["evaluations"][r] == 0 for k, r in
                 zip([k for k in calls if k.endswith("per_lane")], rows) if r >= 0]
        print(f"{robot}: antiparallel row {rows[0]} (came back as given, 0 evaluations: {stuck}); cartesian statuses "
              f"{sorted(set(calls['cartesian_multi/two_iterations']['status']))}; rrtc {calls['rrtc_multi_constrained']['status']}")


if __name__ == "__main__":
    main()
