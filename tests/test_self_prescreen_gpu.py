"""The prescreen of the self-collision kernel on the GPU (validate_self_kernel<kSelfPrescreen>, fkcc_self_prescreen):
  * the error of the hardware's sine and cosine against vsin / vcos, the arithmetic the gates use, over every fp32 value
    of the domain |x| <= Q_MAX (vmv_bare_trig_error): at most BARE_TRIG_EPS / 2;
  * the prescreen's flags are a superset of the exact screen's, word for word (vmv_self_screen_flags), on uniform
    configurations, on configurations bisected onto each gate's boundary, and on rows at and beyond the domain;
  * the validity words are the same with the prescreen (default), the exact screen (VMV_SELF_SCREEN=2) and no screen (0).
With VMV_RECORD_PROFILES=1 the measurements are written to profiles/r33_bare_trig_error.txt and r33_prescreen_rate.txt."""
import ctypes
import os

import numpy as np
import pytest

import self_gates
from envs import make_env

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "fetch"]
PROFILES = os.path.join(self_gates.ROOT, "profiles")
RECORD = os.environ.get("VMV_RECORD_PROFILES") == "1"


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _trig_error(vamp, lo_bits, hi_bits):
    out = np.full(2, -1.0, np.float32)
    rc = vamp.lib.vmv_bare_trig_error(lo_bits, hi_bits, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)
    assert rc == 0
    return float(out[0]), float(out[1])


def test_bare_trig_error_over_the_whole_domain(vamp):
    g = self_gates.gen_hip()
    lo, hi = _bits(2.0 ** -20), _bits(g.Q_MAX)
    assert 2 * (hi - lo + 1) > 3.9e8  # about 4e8 values: 1.98e8 patterns, each with both signs
    s_main, c_main = _trig_error(vamp, lo, hi)
    # below 2^-20: every pattern (0, the denormals and the smallest normal among them), a superset of any sample
    s_low, c_low = _trig_error(vamp, 0, lo - 1)
    assert _bits(np.finfo(np.float32).tiny) < lo
    print(f"main range: sin {s_main!r} cos {c_main!r}; below 2^-20: sin {s_low!r} cos {c_low!r}; BARE_TRIG_EPS {g.BARE_TRIG_EPS!r}")
    if RECORD:
        with open(os.path.join(PROFILES, "r33_bare_trig_error.txt"), "w") as f:
            f.write("vmv_bare_trig_error: max |bare_sin - vsin| and max |bare_cos - vcos|, both signs of every fp32 pattern\n"
                    f"domain 0 .. Q_MAX = {g.Q_MAX!r} (bits 0x00000000 .. 0x{hi:08x}); main range from 2^-20 (0x{lo:08x})\n"
                    f"main_range_sin {s_main!r}\nmain_range_cos {c_main!r}\nbelow_2^-20_sin {s_low!r}\nbelow_2^-20_cos {c_low!r}\n"
                    f"max_abs_sin_diff {max(s_main, s_low)!r}\nmax_abs_cos_diff {max(c_main, c_low)!r}\n")
    for v in (s_main, c_main, s_low, c_low):
        assert 0.0 <= v <= g.BARE_TRIG_EPS / 2.0
    assert s_main > 0.0 and c_main > 0.0  # the kernel did compare two different things


def _flags(vamp, name, q, mode):
    """bool per row: vmv_self_screen_flags"""
    torch = pytest.importorskip("torch")
    n = q.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    tw = torch.full(((n + 63) // 64,), -1, dtype=torch.int64).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = vamp.lib.vmv_self_screen_flags(vamp.lib.vmv_robot_id(name.encode()), ctypes.c_void_p(tq.data_ptr()), n, mode,
                                        ctypes.c_void_p(tw.data_ptr()), stream)
    assert rc == 0
    torch.cuda.synchronize()
    bits = np.unpackbits(tw.cpu().numpy().view(np.uint8), bitorder="little").astype(bool)
    assert not bits[n:].any()
    return bits[:n]


def _uniform(m, n, seed):
    lo, span = np.array(m["lower"], np.float32), np.array(m["span"], np.float32)
    return (lo + span * np.random.default_rng(seed).random((n, len(lo)), dtype=np.float32)).astype(np.float32)


def _assert_superset(exact, fast, what):
    missed = np.nonzero(exact & ~fast)[0]
    assert len(missed) == 0, (what, "rows the exact screen flags and the prescreen does not", missed[:10])


@pytest.mark.parametrize("name", ROBOTS)
def test_superset_on_uniform_configurations(vamp, name):
    m = self_gates.model(name)
    q = _uniform(m, 65536, 3301)
    exact, fast = _flags(vamp, name, q, 0), _flags(vamp, name, q, 1)
    _assert_superset(exact, fast, name)
    ne, nf = int(exact.sum()), int(fast.sum())
    assert 0 < ne < len(q)
    line = f"{name}: 65,536 uniform configurations, exact screen flags {ne}, prescreen {nf} (+{nf - ne}, +{(nf - ne) / ne * 100:.3f} %)"
    print(line)
    if RECORD:
        path = os.path.join(PROFILES, "r33_prescreen_rate.txt")
        old = [ln for ln in (open(path).read().splitlines() if os.path.exists(path) else []) if not ln.startswith(name + ":")]
        with open(path, "w") as f:
            f.write("\n".join(old + [line]) + "\n")


def _thresholds(m):
    """per group: the exact gate's threshold, rs * rs with the gate's own two fp32 roundings"""
    r = np.array(m["radii"])
    rs = [np.float32(np.float32(r[g["bound_a"]]) + np.float32(r[g["bound_b"]])) for g in m["self_groups"]]
    return np.array([float(np.float32(v * v)) for v in rs])


def _d2(m, q64):
    c = self_gates.gen_hip().eval_tape(m, q64)
    return np.stack([((c[:, g["bound_a"]] - c[:, g["bound_b"]]) ** 2).sum(axis=1) for g in m["self_groups"]], axis=1)


def boundary_cases(m, per_group=64, sample=16384, seed=3302):
    """-> (float32 rows on the gates' boundaries, groups covered, groups left out).  A group is covered if the uniform
    sample holds a row its gate fires for and one it does not; per covered group, per_group segments between such rows
    are bisected in float64 until |d^2 - thr| <= 1e-6 thr."""
    q = _uniform(m, sample, seed).astype(np.float64)
    thr = _thresholds(m)
    fires = _d2(m, q) < thr[None, :]
    rng = np.random.default_rng(seed + 1)
    a, b, col = [], [], []
    covered, left_out = [], []
    for gi in range(len(m["self_groups"])):
        on, off = np.nonzero(fires[:, gi])[0], np.nonzero(~fires[:, gi])[0]
        if len(on) == 0 or len(off) == 0:
            left_out.append(gi)
            continue
        covered.append(gi)
        a.append(q[rng.choice(on, per_group)])
        b.append(q[rng.choice(off, per_group)])
        col += [gi] * per_group
    a, b, col = np.concatenate(a), np.concatenate(b), np.array(col)
    rows = np.arange(len(col))
    f = lambda x: _d2(m, x)[rows, col] - thr[col]  # noqa: E731  (a: negative, b: non-negative)
    mid = 0.5 * (a + b)
    for _ in range(80):
        fm = f(mid)
        if (np.abs(fm) <= 1e-6 * thr[col]).all():
            break
        inside = fm < 0
        a[inside], b[~inside] = mid[inside], mid[~inside]
        mid = 0.5 * (a + b)
    assert (np.abs(f(mid)) <= 1e-6 * thr[col]).all()
    return mid.astype(np.float32), covered, left_out


@pytest.mark.parametrize("name", ROBOTS)
def test_superset_on_the_gates_boundaries(vamp, name):
    m = self_gates.model(name)
    cases, covered, left_out = boundary_cases(m)
    names = [f"{m['self_groups'][gi]['a']} vs. {m['self_groups'][gi]['b']}" for gi in left_out]
    print(f"{name}: boundary cases for {len(covered)} of {len(m['self_groups'])} groups; left out: {names}")
    assert 2 * len(covered) >= len(m["self_groups"])
    n = len(cases) + (1000 - len(cases)) % 64  # ragged: the same tail as n = 1,000
    assert n % 64 == 1000 % 64
    q = np.concatenate([cases, _uniform(m, n - len(cases), 3303)])
    exact, fast = _flags(vamp, name, q, 0), _flags(vamp, name, q, 1)
    _assert_superset(exact, fast, name)
    on_boundary = exact[:len(cases)]
    print(f"{name}: {int(on_boundary.sum())} of {len(cases)} boundary rows flagged by the exact screen, {int(fast[:len(cases)].sum())} by the prescreen")
    assert on_boundary.any() and not on_boundary.all()


@pytest.mark.parametrize("name", ROBOTS)
def test_rows_at_and_beyond_the_domain(vamp, name):
    g = self_gates.gen_hip()
    m = self_gates.model(name)
    qmax = np.float32(g.Q_MAX)
    beyond = np.nextafter(qmax, np.float32(np.inf))
    inside = [qmax, -qmax, np.float32(2 * np.pi), np.float32(-2 * np.pi), np.float32(4 * np.pi), np.float32(-4 * np.pi)]
    outside = [beyond, -beyond, np.float32(1e6), np.float32(-1e6), np.float32(1e30), np.float32(-1e30), np.float32(np.inf),
               np.float32(-np.inf), np.float32(np.nan)]
    assert all(abs(v) <= qmax for v in inside)
    base = _uniform(m, 8, 3304)
    rows, is_out = [], []
    for b in base:
        for j in range(m["dimension"]):
            for v in inside + outside:
                r = b.copy()
                r[j] = v
                rows.append(r)
                is_out.append(not abs(v) <= qmax)
    q, is_out = np.array(rows, np.float32), np.array(is_out)
    exact, fast = _flags(vamp, name, q, 0), _flags(vamp, name, q, 1)
    assert fast[is_out].all(), "a row beyond the domain is not flagged"
    _assert_superset(exact, fast, name)
    assert not fast[~is_out].all()  # inside the domain the prescreen still decides


# ---- end to end: the words with the prescreen, the exact screen and no screen ------------------------------------------
def _self_stage(vamp, name, q, words):
    """vmv_validate_batch_self over caller words (ANDs into them); returns the words after the call"""
    torch = pytest.importorskip("torch")
    tq = torch.from_numpy(q).cuda()
    tw = torch.from_numpy(words.view(np.int64).copy()).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = vamp.lib.vmv_validate_batch_self(vamp.lib.vmv_robot_id(name.encode()), ctypes.c_void_p(tq.data_ptr()), q.shape[0],
                                          ctypes.c_void_p(tw.data_ptr()), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return tw.cpu().numpy().view(np.uint64)


def _three_modes(monkeypatch, run):
    out = []
    for mode in (None, "2", "0"):
        if mode is None:
            monkeypatch.delenv("VMV_SELF_SCREEN", raising=False)
        else:
            monkeypatch.setenv("VMV_SELF_SCREEN", mode)
        out.append(run())
    monkeypatch.delenv("VMV_SELF_SCREEN", raising=False)
    return out


@pytest.mark.parametrize("name", ROBOTS)
def test_words_are_the_same_in_every_mode(vamp, oracle, monkeypatch, name):
    m = self_gates.model(name)
    env, oenv = make_env("shell64", oracle, name)
    rid = oracle.robot(name)
    robot = getattr(vamp, name)
    for n in [1, 63, 64, 65, 1023, 1024, 1025, 4097]:
        q = _uniform(m, n, 3400 + n)
        q[::13] = (q[::13] * np.float32(1.6)).astype(np.float32)  # some joints out of range: more self-collisions
        fast, exact, plain = _three_modes(monkeypatch, lambda: robot.validate_batch(q, env))
        assert np.array_equal(fast, exact) and np.array_equal(fast, plain), n
        assert np.array_equal(fast, oracle.validate_batch(rid, oenv, q, threads=8)), n
        caller = np.random.default_rng(n).random((n + 63) // 64 * 64) < 0.625  # bits at and beyond n are set too
        words = np.packbits(caller, bitorder="little").view(np.uint64)
        fast, exact, plain = _three_modes(monkeypatch, lambda: _self_stage(vamp, name, q, words))
        assert np.array_equal(fast, exact) and np.array_equal(fast, plain), n
        want = np.zeros(len(caller), bool)
        want[:n] = caller[:n] & oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
        assert np.array_equal(fast, np.packbits(want, bitorder="little").view(np.uint64)), n


@pytest.mark.parametrize("name", ROBOTS)
def test_flagged_rows_in_the_last_word_only(vamp, oracle, monkeypatch, name):
    """every row but some of the last word's is one no screen flags; those are flagged, half of them colliding"""
    m = self_gates.model(name)
    q0 = _uniform(m, 4096, 3500)
    exact, fast = _flags(vamp, name, q0, 0), _flags(vamp, name, q0, 1)
    rid = oracle.robot(name)
    valid = oracle.validate_batch(rid, oracle.env(), q0, threads=8).astype(bool)
    quiet, flagged_ok, colliding = q0[~fast][0], q0[exact & valid][0], q0[~valid][0]
    n = 4097 - 27
    assert n % 64 >= 37
    q = np.tile(quiet, (n, 1))
    rows = n - 37 + np.random.default_rng(7).permutation(37)[:20]
    q[rows[:10]], q[rows[10:]] = flagged_ok, colliding
    assert not _flags(vamp, name, q, 1)[:n - 37].any()
    words = np.full((n + 63) // 64, np.uint64(0xFFFFFFFFFFFFFFFF))
    fast_w, exact_w, plain_w = _three_modes(monkeypatch, lambda: _self_stage(vamp, name, q, words))
    assert np.array_equal(fast_w, exact_w) and np.array_equal(fast_w, plain_w)
    want = np.zeros(len(words) * 64, bool)
    want[:n] = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
    assert np.array_equal(fast_w, np.packbits(want, bitorder="little").view(np.uint64))
    assert not want[rows[10:]].any() and want[rows[:10]].all()
