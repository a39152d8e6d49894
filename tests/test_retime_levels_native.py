"""The host steps of vmv_retime_multi_constrained as a stand-alone program (tests/native/retime_levels_sanitize.cc) under
AddressSanitizer + UBSan, and its levelled set-up against the serial statement's, piece by piece and bit for bit.  CPU only:
the program has its own main, nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import retime_constrained_serial as RC
import retime_serial as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def program():
    out = os.path.join(ROOT, "build", "retime_levels_sanitize")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "retime_levels_sanitize.cc"), "-o", out, "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    return lambda args, text="": subprocess.run([out, *args], input=text, capture_output=True, text=True, env=env, timeout=600)


def test_levelled_setup_and_blame_rule_under_sanitizers(program):
    r = program([])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("robot", ("panda", "baxter"))
def test_the_levelled_setup_is_the_serial_statements(program, robot):
    """retime_path with levels against retime_constrained_serial.setup over the shared case set, with the levels 0, H,
    H + 1 and a mix of them: the same outcome, the same corners, the same fp32 piece records"""
    S = RC.Settings(grid_step=R.CASE_SETTINGS.grid_step, max_grid=R.CASE_SETTINGS.max_grid)
    H = S.blend_halvings
    rng = np.random.default_rng(5)
    what_code = {"ok": 0, "trivial": 1, "too_long": 2, "non_finite": 3}
    blends = 0
    for name, w in R.cases(robot):
        dim = R.DIM[robot]
        for levels in (np.zeros(len(w), int), np.full(len(w), H), np.full(len(w), H + 1), rng.integers(0, H + 2, len(w))):
            text = f"{dim} {len(w)} {float(np.float32(S.blend))!r} {float(np.float32(S.grid_step))!r} {S.max_grid} {H}\n"
            text += " ".join(str(int(v)) for v in levels) + "\n" + " ".join(f"{v:08x}" for v in bits(w).reshape(-1)) + "\n"
            r = program(["dump"], text)
            assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-2000:])
            lines = r.stdout.strip().split("\n")
            what, distinct, N, P, corner, _ = RC.setup(w, S, levels)
            head = [int(v) for v in lines[0].split()]
            assert head[0] == what_code[what] and head[2] == N and head[3] == (len(corner) if what == "ok" else 0), (name, head, what)
            if what != "ok":
                continue
            assert head[1] == distinct
            for a, line in enumerate(lines[1:]):
                f = line.split()
                assert [int(v) for v in f[:4]] == [corner[a], P.n[a], P.first[a], int(P.stop[a])], (name, a)
                got = np.array([int(v, 16) for v in f[4:]], np.uint32)
                want = np.concatenate([bits([P.d[a], P.span[a]]), np.stack([bits(P.base[a]), bits(P.u_in[a]), bits(P.u_out[a])], axis=1).reshape(-1)])
                assert np.array_equal(got, want), (name, a)
                blends += corner[a] != 0
    assert blends > 50
