"""The self-collision kernel with passes shared by the waves of a workgroup against the oracle, word for word, at every
share size (VMV_SELF_GROUP)."""
import ctypes

import numpy as np
import pytest

from envs import make_env
from workmix import case_seed

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "ur5", "fetch", "baxter"]
# ragged sizes: below one wave, not a multiple of 64, below one workgroup's share of words (4 x group words), several
# workgroups with a ragged last share
SIZES = [1, 37, 63, 64, 65, 100, 1000, 4097, 20000]
# share of the caller's bits that is set: none, Baxter-like 3 %, the flagship's 62.5 %, all (bits beyond n included)
FRACTIONS = [0.0, 0.03, 0.625, 1.0]


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


def _configs(oracle, name, n, seed):
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(seed)
    q = (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)
    q[::13] = (q[::13] * np.float32(1.6)).astype(np.float32)  # some joints out of range: more self-collisions
    return rid, q


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


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("fraction", FRACTIONS)
def test_shared_passes_match_oracle_and_per_wave_kernel(vamp, oracle, monkeypatch, name, fraction):
    for n in SIZES:
        rid, q = _configs(oracle, name, n, seed=case_seed(name, "self_balance", n) % 100000)
        self_valid = oracle.validate_batch(rid, oracle.env(), q, threads=8)  # empty environment: self-collision alone
        n_words = (n + 63) // 64
        rng = np.random.default_rng(n)
        caller = rng.random(n_words * 64) < fraction  # bits beyond n are set too (at 100 %: all-ones words)
        words = np.packbits(caller, bitorder="little").view(np.uint64)
        want = np.zeros(n_words * 64, bool)
        want[:n] = caller[:n] & self_valid
        want_words = np.packbits(want, bitorder="little").view(np.uint64)
        for group in [None] + [str(g) for g in range(1, 9)]:
            if group is None:
                monkeypatch.delenv("VMV_SELF_GROUP", raising=False)
            else:
                monkeypatch.setenv("VMV_SELF_GROUP", group)
            got = _self_stage(vamp, name, q, words)
            assert np.array_equal(got, want_words), (n, group)


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("kind", ["shell64", "cage"])
def test_validate_batch_same_with_either_self_kernel(vamp, oracle, name, kind):
    env, oenv = make_env(kind, oracle, name)
    n = 20000 - 27
    rid, q = _configs(oracle, name, n, seed=case_seed(name, kind, "self_balance_batch") % 100000)
    want = oracle.validate_batch(rid, oenv, q, threads=8)
    assert np.array_equal(getattr(vamp, name).validate_batch(q, env), want)
