"""<robot>.validate_motion_batch_multi / vmv_validate_motion_batch_multi on the GPU: bit-identical to one
validate_motion_batch per environment, concatenated, and equal to the oracle; for every environment kind (so every
variant class of the task kernels and the attachment walk), segment boundaries inside validity bytes and words,
repeated handles, empty segments, non-finite endpoints, later passes with no or very unequal work, the 2^20-edge slice
boundary, torch streams, and planning.validate_paths."""
import ctypes
import os

import numpy as np
import pytest

from envs import build_oracle_env, build_product_env, spec_for
from workmix import case_seed, mixed_edges

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "ur5", "fetch", "baxter"]
KINDS = ["empty", "cage", "shell64", "mixed", "many", "capt", "clouds", "mvt", "heightfield", "attach"]
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 300, 2000]
POOL = 400  # oracle-checked edges per scene (segments draw from them)
_SCENES = {}


def _ill_formed_spec(robot):
    """the mixed scene with stretched / sheared cuboid axes and capsules whose rdv is not 1 / |v|^2 (EnvDev::ill_formed:
    the full-loop variant), as test_multi_env_gpu.py builds it"""
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


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


def _scenes(oracle, robot):
    """(product environments, oracle environments, edge pools) of every kind plus the ill-formed scene; built once"""
    if robot not in _SCENES:
        specs = [spec_for(k, robot) for k in KINDS] + [_ill_formed_spec(robot)]
        oenvs = [build_oracle_env(oracle, s) for s in specs]
        pools = []
        for i, o in enumerate(oenvs):
            try:
                pools.append(mixed_edges(oracle, robot, o, POOL, case_seed("motion-multi", robot, i), zero_every=11)[1:])
            except AssertionError:  # no valid configuration in this scene: the empty scene's edges, all answered here
                a, b = pools[0][0], pools[0][1]
                pools.append((a, b, oracle.validate_motion_batch(oracle.robot(robot), o, a, b, threads=8)))
        _SCENES[robot] = ([build_product_env(s) for s in specs], oenvs, pools)
    return _SCENES[robot]


def _segments(rng, n_scenes):
    """(scene index, count) per segment: every scene once, two handles repeated; sizes drawn from SIZES (each at least
    once), shuffled, so boundary bytes and words straddle segments of different classes"""
    scenes = list(range(n_scenes)) + [1, 9]
    sizes = SIZES + list(rng.choice(SIZES, len(scenes) - len(SIZES)))
    rng.shuffle(sizes)
    order = rng.permutation(len(scenes))
    return [(scenes[i], int(c)) for i, c in zip(order, sizes)]


def _edges(rng, pools, segs):
    """edges drawn from each segment's scene pool -> (a, b, oracle answers, offsets, indices of non-finite edges)"""
    parts = []
    for s, c in segs:
        a, b, v = pools[s]
        idx = rng.integers(len(a), size=c)
        parts.append((a[idx], b[idx], v[idx]))
    a = np.concatenate([p[0] for p in parts]).astype(np.float32)
    b = np.concatenate([p[1] for p in parts]).astype(np.float32)
    v = np.concatenate([p[2] for p in parts])
    offsets = np.concatenate([[0], np.cumsum([c for _, c in segs])]).astype(np.int64)
    bad = []
    for k, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):  # non-finite endpoints at segment edges
        if hi > lo:
            bad.append(lo if k % 2 else hi - 1)
    bad = np.array(sorted(set(bad)), np.int64)
    specials = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j, i in enumerate(bad):
        (a if j % 2 else b)[i, j % a.shape[1]] = specials[j % 3]
    return a, b, v, offsets, bad


def _per_environment(mod, a, b, envs, offsets):
    return np.concatenate([mod.validate_motion_batch(a[lo:hi], b[lo:hi], e) if hi > lo else np.zeros(0, bool)
                           for e, lo, hi in zip(envs, offsets[:-1], offsets[1:])])


@pytest.mark.parametrize("robot", ROBOTS)
def test_multi_is_bit_identical_to_per_environment_calls_and_the_oracle(vamp, oracle, robot):
    mod = getattr(vamp, robot)
    envs, oenvs, pools = _scenes(oracle, robot)
    rng = np.random.default_rng(case_seed("motion-multi-segments", robot))
    segs = _segments(rng, len(envs))
    a, b, v, offsets, bad = _edges(rng, pools, segs)
    seg_envs = [envs[s] for s, _ in segs]
    got = mod.validate_motion_batch_multi(a, b, seg_envs, [c for _, c in segs])
    n = int(offsets[-1])
    assert got.dtype == bool and got.shape == (n,)
    want = _per_environment(mod, a, b, seg_envs, offsets)
    assert np.array_equal(got, want), f"{robot}: {int((got != want).sum())} of {n} differ from per-environment calls"
    assert not got[bad].any()  # an edge with a non-finite endpoint is invalid
    finite = np.ones(n, bool)
    finite[bad] = False
    assert np.array_equal(got[finite], v[finite]), f"{robot}: differs from the oracle"
    assert got.any() and not got.all(), "degenerate workload"
    for (s, _), lo, hi in zip(segs, offsets[:-1], offsets[1:]):  # and the oracle itself on a subsample per segment
        idx = np.arange(lo, hi)[finite[lo:hi]]
        idx = idx if len(idx) <= 64 else np.sort(rng.choice(idx, 64, replace=False))
        if len(idx):
            want_o = oracle.validate_motion_batch(oracle.robot(robot), oenvs[s], a[idx], b[idx], threads=8)
            assert np.array_equal(got[idx], want_o), (robot, (KINDS + ["ill-formed"])[s])


def test_later_pass_with_no_work_and_with_very_unequal_work(vamp, oracle):
    mod = vamp.ur5
    envs, oenvs, pools = _scenes(oracle, "ur5")
    rid = oracle.robot("ur5")
    rng = np.random.default_rng(case_seed("motion-multi-unequal"))
    kinds = [1, 2, 5, 9, 3]  # cage, shell64, capt, attach, mixed
    # (1) every edge is one rake (zero length): the later pass has no task at all
    counts = [9, 65, 7, 300, 64]
    starts = np.concatenate([pools[s][0][rng.integers(POOL, size=c)] for s, c in zip(kinds, counts)])
    got = mod.validate_motion_batch_multi(starts, starts.copy(), [envs[s] for s in kinds], counts)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(got, _per_environment(mod, starts, starts, [envs[s] for s in kinds], offsets))
    assert np.array_equal(got, np.concatenate([oracle.validate_batch(rid, oenvs[s], starts[lo:hi])
                                               for s, lo, hi in zip(kinds, offsets[:-1], offsets[1:])]))
    # (2) segments that are entirely invalid after rake 0 (every goal collides; every goal is non-finite), and one edge
    # of hundreds of rakes (a start from the pool, the last joint turned by 16 whole turns: rake 0 sees the start's pose)
    # between segments of short edges
    lo_b, span = oracle.bounds(rid)
    q = (lo_b + span * rng.random((20000, len(lo_b)), dtype=np.float32)).astype(np.float32)
    hit = q[~oracle.validate_batch(rid, oenvs[2], q, threads=8)][:130]
    a_short = pools[1][0]
    a_long = pools[2][0][:1].copy()
    b_long = a_long.copy()
    b_long[0, -1] += np.float32(32.0 * np.pi)
    a_dead = pools[2][0][rng.integers(POOL, size=len(hit))]
    a_nan = pools[9][0][:16]
    b_nan = np.full_like(a_nan, np.nan)
    a = np.concatenate([a_short[:9], a_dead, a_short[9:40], a_long, a_nan, a_short[40:105]]).astype(np.float32)
    b = np.concatenate([a_short[:9] + 0.01, hit, a_short[9:40] + 0.01, b_long, b_nan, a_short[40:105] + 0.01]).astype(np.float32)
    kinds = [1, 2, 1, 2, 9, 9]
    counts = [9, len(hit), 31, 1, 16, 65]
    seg = [envs[s] for s in kinds]
    got = mod.validate_motion_batch_multi(a, b, seg, counts)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(got, _per_environment(mod, a, b, seg, offsets))
    assert not got[offsets[4]:offsets[5]].any()
    want = np.concatenate([oracle.validate_motion_batch(rid, oenvs[s], a[lo:hi], b[lo:hi], threads=8)
                           for s, lo, hi in zip(kinds[:4], offsets[:4], offsets[1:5])])
    assert np.array_equal(got[:offsets[4]], want)
    assert np.array_equal(got[offsets[5]:], oracle.validate_motion_batch(rid, oenvs[9], a[offsets[5]:], b[offsets[5]:]))


@pytest.fixture(scope="module")
def mbm_envs(vamp, golden_dir):
    """each robot's 1,300 MotionBenchMaker environments, built once per module"""
    from test_mbm import problem_primitives

    cache = {}

    def get(robot):
        if robot not in cache:
            g = np.load(os.path.join(golden_dir, f"mbm_{robot}.npz"))
            specs = [problem_primitives(vamp, g, i) for i in range(len(g["names"]))]
            cache[robot] = (g, specs, [build_product_env(s) for s in specs])
        return cache[robot]

    return get


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch"])
def test_mbm_start_goal_edges_in_one_call_match_the_oracle(vamp, oracle, mbm_envs, robot):
    g, specs, envs = mbm_envs(robot)
    rid = oracle.robot(robot)
    a = np.ascontiguousarray(g["start"], np.float32)
    b = np.ascontiguousarray(g["goal"], np.float32)
    got = getattr(vamp, robot).validate_motion_batch_multi(a, b, envs, [1] * len(envs))
    want = np.array([oracle.validate_motion(rid, build_oracle_env(oracle, s), a[i], b[i]) for i, s in enumerate(specs)])
    assert np.array_equal(got, want), f"{robot}: problems {np.flatnonzero(got != want)[:10]} differ"
    assert not got.all()  # (Fetch: no straight start -> goal edge of the archive is free)


def test_slice_boundary(vamp, oracle):
    """2^20 + 4,160 short UR5 edges in five segments; the fourth straddles edge 2^20 (the slice boundary)"""
    mod = vamp.ur5
    envs, oenvs, _ = _scenes(oracle, "ur5")
    rid = oracle.robot("ur5")
    kinds = [2, 1, 3, 9, 5]  # shell64, cage, mixed, attach, capt
    counts = [262_147, 524_288, 262_000, 301, 4_000]
    n = sum(counts)
    assert n == (1 << 20) + 4160
    rng = np.random.default_rng(case_seed("motion-multi-slices"))
    lo_b, span = oracle.bounds(rid)
    a = (lo_b + span * rng.random((n, len(lo_b)), dtype=np.float32)).astype(np.float32)
    b = (a + rng.normal(0.0, 0.05, a.shape)).astype(np.float32)
    seg = [envs[s] for s in kinds]
    got = mod.validate_motion_batch_multi(a, b, seg, counts)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert offsets[3] < (1 << 20) < offsets[4]
    assert np.array_equal(got, _per_environment(mod, a, b, seg, offsets))
    assert got.any() and not got.all()
    for s, lo, hi in zip(kinds, offsets[:-1], offsets[1:]):
        idx = np.sort(rng.choice(np.arange(lo, hi), min(64, hi - lo), replace=False))
        if s == 9:  # and the edges on both sides of the slice boundary
            idx = np.union1d(idx, np.arange(max(lo, (1 << 20) - 8), min(hi, (1 << 20) + 8)))
        assert np.array_equal(got[idx], oracle.validate_motion_batch(rid, oenvs[s], a[idx], b[idx], threads=8))


def test_torch_input_on_a_side_stream_and_back_to_back_tables(vamp, oracle):
    torch = pytest.importorskip("torch")
    envs, _, pools = _scenes(oracle, "panda")
    rng = np.random.default_rng(case_seed("motion-multi-torch"))
    segs_a, segs_b = _segments(rng, len(envs)), _segments(rng, len(envs))[::-1]
    aa, ba = _edges(rng, pools, segs_a)[:2]
    ab, bb = _edges(rng, pools, segs_b)[:2]
    ea, ca = [envs[s] for s, _ in segs_a], [c for _, c in segs_a]
    eb, cb = [envs[s] for s, _ in segs_b], [c for _, c in segs_b]
    want_a = vamp.panda.validate_motion_batch_multi(aa, ba, ea, ca)
    want_b = vamp.panda.validate_motion_batch_multi(ab, bb, eb, cb)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ta, tb = torch.from_numpy(aa).cuda(), torch.from_numpy(ba).cuda()
        tc, td = torch.from_numpy(ab).cuda(), torch.from_numpy(bb).cuda()
        # two calls back to back on one stream with different tables (the per-stream tables and scratch are reused)
        got_a = vamp.panda.validate_motion_batch_multi(ta, tb, ea, ca)
        got_b = vamp.panda.validate_motion_batch_multi(tc, td, eb, cb)
        got_a2 = vamp.panda.validate_motion_batch_multi(ta, tb, ea, ca)
    side.synchronize()
    assert got_a.dtype == torch.bool and got_a.is_cuda
    assert np.array_equal(got_a.cpu().numpy(), want_a) and np.array_equal(got_a2.cpu().numpy(), want_a)
    assert np.array_equal(got_b.cpu().numpy(), want_b)
    vamp._lib.lib.vmv_release_staging()  # frees the per-stream tables and scratch; later calls allocate them again
    with torch.cuda.stream(side):
        got_side = vamp.panda.validate_motion_batch_multi(ta, tb, ea, ca)  # the side stream's, again
    side.synchronize()
    assert np.array_equal(got_side.cpu().numpy(), want_a)
    got = vamp.panda.validate_motion_batch_multi(aa, ba, ea, ca)
    assert np.array_equal(got, want_a)


def test_device_call_with_bad_offsets_writes_nothing(vamp, oracle):
    torch = pytest.importorskip("torch")
    from vamp_mvt_amd import _lib

    envs = _scenes(oracle, "panda")[0]
    a = torch.zeros((200, 7), dtype=torch.float32, device="cuda")
    bits = torch.full((4,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    handles = (ctypes.c_void_p * 3)(envs[1].handle(), envs[2].handle(), envs[5].handle())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for offsets in ([0, 100, 50, 200], [3, 100, 150, 200]):
        offs = np.array(offsets, np.uint64)
        rc = _lib.lib.vmv_validate_motion_batch_multi(0, handles, offs.ctypes.data_as(_lib.c_size_p), 3,
                                                      ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(a.data_ptr()),
                                                      ctypes.c_void_p(bits.data_ptr()), stream)
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
    a = torch.zeros((128, 7), dtype=torch.float32, device="cuda:0")
    bits = torch.full((2,), 7, dtype=torch.int64, device="cuda:0")
    offs = np.array([0, 64, 128], np.uint64)
    rc = _lib.lib.vmv_validate_motion_batch_multi(0, handles, offs.ctypes.data_as(_lib.c_size_p), 2,
                                                  ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(a.data_ptr()),
                                                  ctypes.c_void_p(bits.data_ptr()), None)
    assert rc == 1 and b"device" in _lib.lib.vmv_last_error()
    torch.cuda.synchronize()
    assert (bits == 7).all()


def test_validate_paths_equals_path_validate_per_path(vamp, oracle):
    from vamp_mvt_amd import planning

    envs, _, pools = _scenes(oracle, "fetch")
    rng = np.random.default_rng(case_seed("motion-multi-paths"))
    paths, scenes = [], []
    for k, length in enumerate([0, 1, 2, 5, 0, 30, 1, 12, 2, 3, 60, 7]):
        s = [1, 2, 3, 5, 9, 0, 10][k % 7]
        a = pools[s][0]
        start = a[rng.integers(len(a))]
        steps = rng.normal(0.0, 0.08, (max(length - 1, 0), len(start))).astype(np.float32)
        path = np.concatenate([start[None, :], start[None, :] + np.cumsum(steps, axis=0)]).astype(np.float32)[:length]
        paths.append([p for p in path])
        scenes.append(envs[s])
    scenes[4] = None  # the empty environment
    got = planning.validate_paths(vamp.fetch, paths, scenes)
    want = np.array([planning.validate_path(vamp.fetch, p, e if e is not None else vamp.Environment())
                     for p, e in zip(paths, scenes)])
    assert got.dtype == bool and got.shape == (len(paths),)
    assert np.array_equal(got, want)
    assert got[[0, 1, 4, 6]].all()  # fewer than 2 waypoints: valid
    assert not got.all(), "degenerate workload"
    Path = vamp.fetch.Path
    for p, e, g in zip(paths, scenes, got):
        if e is not None and len(p):
            assert Path(p).validate(e) == g
