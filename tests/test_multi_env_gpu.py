"""<robot>.validate_batch_multi / vmv_validate_batch_multi on the GPU: bit-identical to one validate_batch per
environment, concatenated, and equal to the oracle; for every environment kind (so every kernel variant class and the
attachment kernel), segment boundaries inside validity words, repeated handles, empty segments and non-finite rows."""
import ctypes
import os

import numpy as np
import pytest

from envs import build_oracle_env, build_product_env, spec_for

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "ur5", "fetch", "baxter"]
KINDS = ["empty", "cage", "shell64", "mixed", "many", "capt", "clouds", "mvt", "heightfield", "attach"]
SIZES = [0, 1, 63, 64, 65, 300, 5000]


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


def _ill_formed_spec(robot):
    """test_gpu_parity.test_ill_formed_primitives_take_the_full_loops' scene: stretched / sheared cuboid axes and a capsule
    whose rdv is not 1 / |v|^2 (EnvDev::ill_formed: the full-loop variant)"""
    out = []
    for k, (kind, p) in enumerate(spec_for("mixed", robot, seed=5)):
        p = np.array(p, np.float32)
        if kind == "cuboid" and k % 2 == 0:
            p[3:6] *= np.float32(1.7)
            p[6:9] += np.float32(0.4) * p[9:12]
        if kind == "capsule" and k % 3 == 0:
            p[7] *= np.float32(0.45)
        out.append((kind, p))
    return out


def _scene_set(oracle, robot):
    specs = [spec_for(k, robot) for k in KINDS] + [_ill_formed_spec(robot)]
    return [build_product_env(s) for s in specs], [build_oracle_env(oracle, s) for s in specs]


def _segments(rng, n_scenes):
    """(scene index, count) per segment: every scene once, two handles repeated; sizes drawn from SIZES (each at least
    once), shuffled, so boundary words straddle segments of different classes"""
    scenes = list(range(n_scenes)) + [1, 9]
    sizes = SIZES + list(rng.choice(SIZES, len(scenes) - len(SIZES)))
    rng.shuffle(sizes)
    order = rng.permutation(len(scenes))
    return [(scenes[i], int(c)) for i, c in zip(order, sizes)]


def _configs(oracle, robot, n, rng, offsets):
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    q = (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)
    out_of_range = rng.random(n) < 0.05  # beyond the joint limits: still evaluated exactly
    q[out_of_range] = (lo - 0.3 * span + 1.6 * span * rng.random((int(out_of_range.sum()), len(lo)))).astype(np.float32)
    bad = []
    for a, b in zip(offsets[:-1], offsets[1:]):  # non-finite rows at segment edges
        if b > a:
            bad += [a, b - 1]
    bad = np.array(sorted(set(bad)), np.int64)[::2]
    specials = np.array([np.nan, np.inf, -np.inf], np.float32)
    q[bad, rng.integers(len(lo), size=len(bad))] = specials[np.arange(len(bad)) % 3]
    return rid, q, bad


@pytest.mark.parametrize("robot", ROBOTS)
def test_multi_is_bit_identical_to_per_environment_calls_and_the_oracle(vamp, oracle, robot):
    mod = getattr(vamp, robot)
    envs, oenvs = _scene_set(oracle, robot)
    rng = np.random.default_rng(sum(map(ord, robot)))
    segs = _segments(rng, len(envs))
    counts = [c for _, c in segs]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(offsets[-1])
    rid, q, bad = _configs(oracle, robot, n, rng, offsets)
    got = mod.validate_batch_multi(q, [envs[s] for s, _ in segs], counts)
    assert got.dtype == bool and got.shape == (n,)
    want = np.concatenate([mod.validate_batch(q[a:b], envs[s]) if b > a else np.zeros(0, bool)
                           for (s, _), a, b in zip(segs, offsets[:-1], offsets[1:])])
    assert np.array_equal(got, want), f"{robot}: {int((got != want).sum())} of {n} differ from per-environment calls"
    assert not got[bad].any()  # non-finite rows are invalid
    assert got.any() and not got.all(), "degenerate workload"
    for (s, _), a, b in zip(segs, offsets[:-1], offsets[1:]):  # oracle on a subsample of every segment
        idx = np.arange(a, b)
        idx = idx[np.isfinite(q[idx]).all(axis=1)]
        idx = idx if len(idx) <= 96 else np.sort(rng.choice(idx, 96, replace=False))
        if len(idx):
            assert np.array_equal(got[idx], oracle.validate_batch(rid, oenvs[s], q[idx], threads=8)), (robot, (KINDS + ["ill-formed"])[s])


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch"])
def test_mbm_scenes_in_one_call_match_the_oracle(vamp, oracle, golden_dir, robot):
    """all 1,300 MotionBenchMaker scenes x (start, goal) in ONE call (tests/test_mbm.py checks them one call each)"""
    from test_mbm import HERE, STANDARD, problem_primitives

    g = np.load(os.path.join(golden_dir, f"mbm_{robot}.npz"))
    rid = oracle.robot(robot)
    names = [str(x) for x in g["names"]]
    specs = [problem_primitives(vamp, g, i) for i in range(len(names))]
    q = np.stack([np.stack([g["start"][i], g["goal"][i]]) for i in range(len(names))]).reshape(-1, g["start"].shape[1])
    q = q.astype(np.float32)
    got = getattr(vamp, robot).validate_batch_multi(q, [build_product_env(s) for s in specs], [2] * len(names))
    for i, spec in enumerate(specs):
        want = oracle.validate_batch(rid, build_oracle_env(oracle, spec), q[2 * i:2 * i + 2])
        assert np.array_equal(got[2 * i:2 * i + 2], want), f"{robot} problem {names[i]}/{g['index'][i]}"
    both = got.reshape(-1, 2).all(axis=1)
    assert int(sum(b for b, name in zip(both, names) if name in STANDARD)) == HERE[robot]


def test_torch_input_on_a_side_stream_and_back_to_back_tables(vamp, oracle):
    torch = pytest.importorskip("torch")
    envs, _ = _scene_set(oracle, "panda")
    rng = np.random.default_rng(7)
    segs_a, segs_b = _segments(rng, len(envs)), _segments(rng, len(envs))[::-1]
    qa = _configs(oracle, "panda", sum(c for _, c in segs_a), rng, np.cumsum([0] + [c for _, c in segs_a]))[1]
    qb = _configs(oracle, "panda", sum(c for _, c in segs_b), rng, np.cumsum([0] + [c for _, c in segs_b]))[1]
    want_a = vamp.panda.validate_batch_multi(qa, [envs[s] for s, _ in segs_a], [c for _, c in segs_a])
    want_b = vamp.panda.validate_batch_multi(qb, [envs[s] for s, _ in segs_b], [c for _, c in segs_b])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ta, tb = torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda()
        # two calls back to back on one stream with different tile tables (the per-stream scratch is reused)
        got_a = vamp.panda.validate_batch_multi(ta, [envs[s] for s, _ in segs_a], [c for _, c in segs_a])
        got_b = vamp.panda.validate_batch_multi(tb, [envs[s] for s, _ in segs_b], [c for _, c in segs_b])
        got_a2 = vamp.panda.validate_batch_multi(ta, [envs[s] for s, _ in segs_a], [c for _, c in segs_a])
    side.synchronize()
    assert got_a.dtype == torch.bool and got_a.is_cuda
    assert np.array_equal(got_a.cpu().numpy(), want_a) and np.array_equal(got_a2.cpu().numpy(), want_a)
    assert np.array_equal(got_b.cpu().numpy(), want_b)
    vamp._lib.lib.vmv_release_staging()  # frees the per-stream tables; later calls allocate them again
    got = vamp.panda.validate_batch_multi(qa, [envs[s] for s, _ in segs_a], [c for _, c in segs_a])
    assert np.array_equal(got, want_a)


def test_device_call_with_a_bad_argument_writes_nothing(vamp, oracle):
    torch = pytest.importorskip("torch")
    from vamp_mvt_amd import _lib

    envs, _ = _scene_set(oracle, "panda")
    q = torch.zeros((200, 7), dtype=torch.float32, device="cuda")
    bits = torch.full((4,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    handles = (ctypes.c_void_p * 3)(envs[1].handle(), envs[2].handle(), envs[5].handle())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for offsets in ([0, 100, 50, 200], [3, 100, 150, 200]):
        offs = np.array(offsets, np.uint64)
        rc = _lib.lib.vmv_validate_batch_multi(0, handles, offs.ctypes.data_as(_lib.c_size_p), 3,
                                               ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(bits.data_ptr()), stream)
        assert rc == 1
    torch.cuda.synchronize()
    assert (bits == 0x5A5A5A5A).all()


def test_environment_of_another_device_is_refused(vamp, oracle):
    if vamp.device_count() < 2:
        pytest.skip("needs two GPUs")
    torch = pytest.importorskip("torch")
    from vamp_mvt_amd import _lib

    vamp.set_device(1)
    try:
        other = build_product_env(spec_for("cage", "panda"))
        h1 = other.handle()
    finally:
        vamp.set_device(0)
    here = build_product_env(spec_for("shell64", "panda"))
    handles = (ctypes.c_void_p * 2)(here.handle(), h1)
    q = torch.zeros((128, 7), dtype=torch.float32, device="cuda:0")
    bits = torch.full((2,), 7, dtype=torch.int64, device="cuda:0")
    offs = np.array([0, 64, 128], np.uint64)
    rc = _lib.lib.vmv_validate_batch_multi(0, handles, offs.ctypes.data_as(_lib.c_size_p), 2, ctypes.c_void_p(q.data_ptr()),
                                           ctypes.c_void_p(bits.data_ptr()), None)
    assert rc == 1 and b"device" in _lib.lib.vmv_last_error()
    torch.cuda.synchronize()
    assert (bits == 7).all()
