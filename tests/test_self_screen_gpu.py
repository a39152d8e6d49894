"""The screened self-collision kernel (validate_self_kernel<true>: fkcc_self_screen on every valid configuration, fkcc_self
on the flagged ones only) against the oracle and against the unscreened instance (VMV_SELF_SCREEN=0), word for word.
The inputs put configurations of three classes, picked on the CPU from the generator's float64 tape, where the second
round's passes begin and end:
  G0  every gate clear by more than 1 cm or switched off by its table bit (never flagged), valid
  F   some gate fires by more than 1 cm with its table bit set (flagged), valid
  C   self-colliding
Panda and Fetch are screened; for UR5 (not screened) the switch must change nothing.  UR5's forearm / wrist_2 bounding
pair is never clear by more than 5.8 mm (200,000 uniform draws), so no UR5 configuration has every gate clear by 1 cm: its
G0 asks for 2 mm, still three orders of magnitude above fp32 effects."""
import ctypes

import numpy as np
import pytest

import self_gates
from envs import make_env

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "fetch", "ur5"]
MARGIN = 0.01  # metres: far from anything fp32 (~1e-6 m) or the float64 tape could decide differently
G0_MARGIN = {"ur5": 0.002}  # (see above)


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


_CLASSES = {}


def _classes(oracle, name):
    """one configuration of each class: dict(G0=q, F=q, C=q)"""
    if name in _CLASSES:
        return _CLASSES[name]
    m = self_gates.model(name)
    two, multi = self_gates.tables(name, m, self_gates.generated_text(name))
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    q = (lo + span * np.random.default_rng(1010).random((2000, len(lo)), dtype=np.float32)).astype(np.float32)
    clear = self_gates.gate_clearance(m, q)
    bits = self_gates.table_bits(m, two, multi, q)
    valid = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)  # empty environment: self-collision alone
    unflagged = ((clear > G0_MARGIN.get(name, MARGIN)) | ~bits).all(axis=1)
    g0 = unflagged & valid
    f = ((clear < -MARGIN) & bits).any(axis=1) & valid
    assert not (unflagged & ~valid).any(), "a configuration no gate fires for collides"
    found = {"G0": g0, "F": f, "C": ~valid}
    for k, mask in found.items():
        assert mask.any(), f"{name}: no configuration of class {k} among {len(q)} draws"
    _CLASSES[name] = {k: q[np.nonzero(mask)[0][0]].copy() for k, mask in found.items()}
    return _CLASSES[name]


def _self_stage(vamp, name, q, words):
    """vmv_validate_batch_self over caller words (ANDs into them); returns the words after the call"""
    torch = pytest.importorskip("torch")
    n = q.shape[0]
    tq = torch.from_numpy(q).cuda()
    tw = torch.from_numpy(words.view(np.int64).copy()).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = vamp.lib.vmv_validate_batch_self(vamp.lib.vmv_robot_id(name.encode()), ctypes.c_void_p(tq.data_ptr()), n,
                                          ctypes.c_void_p(tw.data_ptr()), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return tw.cpu().numpy().view(np.uint64)


def _check(vamp, oracle, monkeypatch, name, q, caller, what):
    """the self stage over `caller` (bool per bit of the words, bits beyond n included), screen on and off"""
    n = q.shape[0]
    n_words = (n + 63) // 64
    assert caller.shape == (n_words * 64,)
    rid = oracle.robot(name)
    self_valid = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
    want = np.zeros(n_words * 64, bool)
    want[:n] = caller[:n] & self_valid
    want_words = np.packbits(want, bitorder="little").view(np.uint64)
    words = np.packbits(caller, bitorder="little").view(np.uint64)
    monkeypatch.delenv("VMV_SELF_SCREEN", raising=False)
    got = _self_stage(vamp, name, q, words)
    monkeypatch.setenv("VMV_SELF_SCREEN", "0")
    plain = _self_stage(vamp, name, q, words)
    monkeypatch.delenv("VMV_SELF_SCREEN", raising=False)
    assert np.array_equal(plain, want_words), ("unscreened", what)
    assert np.array_equal(got, want_words), ("screened", what)
    assert np.array_equal(got, plain), what


def _set_group(monkeypatch, group):
    if group is None:
        monkeypatch.delenv("VMV_SELF_GROUP", raising=False)
    else:
        monkeypatch.setenv("VMV_SELF_GROUP", group)


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("group", [None, "1", "8"])
def test_flagged_rows_at_the_pass_boundaries(vamp, oracle, monkeypatch, name, group):
    """n = 1,024, all bits set; G0 rows except k rows (half F, half C) at seeded positions; k spans 0, one lane, one
    pass less / exactly / plus one lane, two passes, every row"""
    cls = _classes(oracle, name)
    _set_group(monkeypatch, group)
    n = 1024
    for k in [0, 1, 63, 64, 65, 128, 1024]:
        rng = np.random.default_rng(k)
        q = np.tile(cls["G0"], (n, 1))
        rows = rng.permutation(n)[:k]
        q[rows[: k // 2]] = cls["F"]
        q[rows[k // 2:]] = cls["C"]
        _check(vamp, oracle, monkeypatch, name, q, np.ones(n, bool), (k, group))


@pytest.mark.parametrize("name", ROBOTS)
def test_ragged_batches(vamp, oracle, monkeypatch, name):
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    for n in [1, 63, 65, 1000, 4097]:
        rng = np.random.default_rng(4000 + n)
        q = (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)
        q[::13] = (q[::13] * np.float32(1.6)).astype(np.float32)  # some joints out of range: more self-collisions
        caller = rng.random((n + 63) // 64 * 64) < 0.625  # bits at and beyond n are set too
        _check(vamp, oracle, monkeypatch, name, q, caller, n)


@pytest.mark.parametrize("name", ROBOTS)
def test_flags_in_the_tail_word_only(vamp, oracle, monkeypatch, name):
    cls = _classes(oracle, name)
    n = 4097 - 27
    assert n % 64 >= 37
    q = np.tile(cls["G0"], (n, 1))
    rng = np.random.default_rng(7)
    rows = n - 37 + rng.permutation(37)[:20]
    q[rows[:10]] = cls["F"]
    q[rows[10:]] = cls["C"]
    _check(vamp, oracle, monkeypatch, name, q, np.ones((n + 63) // 64 * 64, bool), "tail")


@pytest.mark.parametrize("name", ROBOTS)
def test_validate_batch_with_and_without_the_screen(vamp, oracle, monkeypatch, name):
    env, oenv = make_env("shell64", oracle, name)
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    n = 20000 - 27
    q = (lo + span * np.random.default_rng(99).random((n, len(lo)), dtype=np.float32)).astype(np.float32)
    q[::13] = (q[::13] * np.float32(1.6)).astype(np.float32)
    want = oracle.validate_batch(rid, oenv, q, threads=8)
    monkeypatch.delenv("VMV_SELF_SCREEN", raising=False)
    assert np.array_equal(getattr(vamp, name).validate_batch(q, env), want)
    monkeypatch.setenv("VMV_SELF_SCREEN", "0")
    assert np.array_equal(getattr(vamp, name).validate_batch(q, env), want)
