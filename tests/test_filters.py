"""Point-cloud filters: vamp.filter_pointcloud with filter_type "scdf" (collision/filter.hh:175-275)
and "centervox" (collision/filter_centervox.hh).

Oracle = oracle/vamp_oracle.c (vo_filter_scdf / vo_filter_centervox).  Both filters are pinned against the reference's
own headers compiled in place (tests/test_ref_cloud_pins.py and its GPU twin, tests/golden/ref_{scdf,centervox}.npz)
wherever the answer is independent of tie order; the restatement keeps equal Morton codes in their current order (the
reference's pdqsort leaves that order open).  The tests here pin the oracle against an independent slow Python
restatement and against the filters' defining properties, and compare the HIP implementation with the oracle point for
point, in order, at the larger sizes."""
import numpy as np
import pytest

from pins import scene_cloud

ORIGIN = np.array([0.0, 0.0, 0.333], np.float32)  # Panda first joint (reference src/vamp/constants.py)
RANGE = np.float32(1.19)
LO, HI = ORIGIN - RANGE, ORIGIN + RANGE


def slow_scdf(pc, min_dist, max_range, origin, lo, hi, cull):
    """independent restatement of filter.hh:175-275 in numpy/Python (fp32 arithmetic, stable sort), small n only"""
    f = np.float32
    n = len(pc)
    sqdist, sqrange = f(min_dist) * f(min_dist), f(max_range) * f(max_range)
    mn = min(f(origin[k]) - f(max_range) for k in range(3))
    mx = min(f(origin[k]) + f(max_range) for k in range(3))
    first = []
    for i in range(n):
        d = pc[i] - origin
        sq = f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2]))
        if not cull or (sq < sqrange and all(lo[k] <= pc[i, k] <= hi[k] for k in range(3))):
            first.append(i)
    first += [0] * (n - len(first))

    def remap(x):
        v = f(f(f(x - mn) / f(mx - mn)) * f(1000.0))
        return int(np.int64(np.trunc(v))) & 0xffffffff if np.isfinite(v) and abs(v) < 2.0 ** 63 else 0

    def pdep(src, mask):
        out, bit = 0, 0
        for pos in range(32):
            if (mask >> pos) & 1:
                out |= ((src >> bit) & 1) << pos
                bit += 1
        return out

    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        pts = pc[first]
        new_min, new_max = min(mx, f(pts.min())), max(mn, f(pts.max()))
        codes = [pdep(remap(p[perm[0]]), 0x49249249) | pdep(remap(p[perm[1]]), 0x92492492) |
                 pdep(remap(p[perm[2]]), 0x24924924) for p in pts]
        order = np.argsort(np.array(codes, np.uint64), kind="stable")
        first = [first[j] for j in order]
        kept = [first[0]]
        for i in first[1:]:
            d = pc[i] - pc[kept[-1]]
            if f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2])) > sqdist:
                kept.append(i)
        first = kept
        mx = f((np.float64(f(new_max + mx))) / 2.0)
        mn = f((np.float64(f(new_min + mn))) / 2.0)
    return pc[first]


@pytest.mark.parametrize("cull", [True, False])
def test_oracle_scdf_matches_slow_restatement(oracle, cull):
    pc = scene_cloud(700, 3)
    want = slow_scdf(pc, 0.03, RANGE, ORIGIN, LO, HI, cull)
    got = oracle.filter_scdf(pc, 0.03, RANGE, ORIGIN, LO, HI, cull)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert 20 < len(got) < len(pc)


def test_oracle_scdf_properties(oracle):
    pc = scene_cloud(20000, 5)
    out = oracle.filter_scdf(pc, 0.02, RANGE, ORIGIN, LO, HI, True)
    keys = {tuple(p) for p in pc.view(np.uint32).reshape(-1, 3).tolist()}
    assert all(tuple(p) in keys for p in out.view(np.uint32).reshape(-1, 3).tolist())  # a subset of the input
    d = np.linalg.norm(out[1:] - out[:-1], axis=1)
    assert (d > 0.02 * 0.999).all()  # neighbours on the last curve are farther than min_dist apart
    inside = (np.linalg.norm(out - ORIGIN, axis=1) < RANGE)
    assert inside.sum() >= len(out) - 1  # only the reference's stray copy of point 0 may lie outside
    assert 500 < len(out) < 8000


def test_oracle_centervox_properties(oracle):
    pc = scene_cloud(30000, 7)
    vs = 0.03
    out = oracle.filter_centervox(pc, vs, RANGE, ORIGIN, LO, HI)
    width = float((HI - LO).max())
    gw = min(255, int(np.ceil(width / vs)))
    isf = np.float32(gw) / np.float32(width)
    vox = np.clip(((out - LO) * isf).astype(np.int32), 0, 254)
    assert len({tuple(v) for v in vox.tolist()}) == len(out)  # one point per voxel
    # every retained point is the closest to its voxel centre among the inputs of that voxel
    ok = (np.linalg.norm(pc - ORIGIN, axis=1) < RANGE) & ((pc >= LO) & (pc <= HI)).all(1)
    cand = pc[ok]
    cvox = np.clip(((cand - LO) * isf).astype(np.int32), 0, 254)
    centre = LO + (cvox.astype(np.float32) + np.float32(0.5)) * np.float32(vs)
    dsq = ((cand - centre) ** 2).sum(1)
    best = {}
    for v, d, p in zip(map(tuple, cvox.tolist()), dsq, cand):
        if v not in best or d < best[v][0]:
            best[v] = (d, p)
    assert len(best) == len(out)
    for v, p in zip(map(tuple, vox.tolist()), out):
        assert np.allclose(best[v][1], p)
    # pool exhaustion is reported where the reference throws: tiny voxels over a big cloud
    assert oracle.filter_centervox(scene_cloud(90000, 9), 0.004, RANGE, ORIGIN, LO, HI) is None


def test_filter_abi_rejects_bad_arguments(vamp):
    with pytest.raises(ValueError):
        vamp.filter_pointcloud(np.zeros((4, 3), np.float32), 0.02, 1.0, 0.03, ORIGIN, LO, HI, True, "voxelgrid")
    pts, ns = vamp.filter_pointcloud(np.zeros((0, 3), np.float32), 0.02, 1.0, 0.03, ORIGIN, LO, HI, True, "scdf")
    assert pts.shape == (0, 3)  # filter.hh:185-188: an empty cloud comes back empty (no device needed)


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("n,seed,min_dist", [(5000, 11, 0.02), (120000, 12, 0.015), (300, 13, 0.05)])
def test_gpu_scdf_matches_oracle(vamp, oracle, n, seed, min_dist, cull):
    pc = scene_cloud(n, seed)
    want = oracle.filter_scdf(pc, min_dist, RANGE, ORIGIN, LO, HI, cull)
    got, ns = vamp.filter_pointcloud(pc, min_dist, RANGE, 0.03, ORIGIN, LO, HI, cull, "scdf")
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert ns > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,vs", [(5000, 21, 0.03), (200000, 22, 0.0303), (64, 23, 0.2)])
def test_gpu_centervox_matches_oracle(vamp, oracle, n, seed, vs):
    pc = scene_cloud(n, seed)
    want = oracle.filter_centervox(pc, vs, RANGE, ORIGIN, LO, HI)
    got, ns = vamp.filter_pointcloud(pc, 0.0, RANGE, vs, ORIGIN, LO, HI, True, "centervox")
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_gpu_centervox_pool_exhaustion_is_a_status(vamp, oracle):
    pc = scene_cloud(90000, 9)
    assert oracle.filter_centervox(pc, 0.004, RANGE, ORIGIN, LO, HI) is None
    with pytest.raises(vamp.VmvError) as ei:
        vamp.filter_pointcloud(pc, 0.0, RANGE, 0.004, ORIGIN, LO, HI, True, "centervox")
    assert ei.value.status == 4  # VMV_ERR_CAPACITY


# ---- CAPT build on the GPU: identical arrays to the host builder (which the oracle pins, tests/test_capt_oracle.py) ----
def _capt_arrays(vamp, pts, r_min, r_max, r_point, build):
    e = vamp.Environment()
    e.add_capt_pointcloud(pts, r_min, r_max, r_point, build=build)
    return e.host_tables()["capt"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,radii", [(2000, 41, (0.012, 0.08)), (10000, 42, (0.015, 0.08)), (10000, 43, (0.012, 0.24)),
                                          (3000, 44, (0.02, 0.5)), (17, 45, (0.012, 0.08)), (4096, 46, (0.012, 0.1))])
def test_gpu_capt_build_equals_host_build(vamp, n, seed, radii):
    from vamp_mvt_amd.workloads import shell_cloud
    pts = shell_cloud(n, seed)
    a = _capt_arrays(vamp, pts, radii[0], radii[1], 0.0025, "host")
    b = _capt_arrays(vamp, pts, radii[0], radii[1], 0.0025, "gpu")
    assert a["nlog2"] == b["nlog2"]
    for key in ("tests", "aff_starts", "aabbs", "aff", "aabb_top"):
        assert a[key].shape == b[key].shape, key
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


@pytest.mark.gpu
def test_gpu_capt_build_drives_validation(vamp, oracle):
    """an environment whose point cloud was built on the GPU validates exactly like the oracle's"""
    from envs import build_oracle_env, spec_for
    spec = spec_for("capt", "fetch")
    oe = build_oracle_env(oracle, spec)
    e = vamp.Environment()
    for kind, p in spec:
        if kind == "sphere":
            e.add_sphere(vamp.Sphere(p[:3], p[3]))
        elif kind == "cuboid":
            e.add_cuboid(vamp.Cuboid.from_canonical(p))
        else:
            e.add_capt_pointcloud(*p, build="gpu")
    rid = oracle.robot("fetch")
    lo, span = oracle.bounds(rid)
    q = (lo + span * np.random.default_rng(3).random((6000, len(lo)), dtype=np.float32)).astype(np.float32)
    assert np.array_equal(vamp.fetch.validate_batch(q, e), oracle.validate_batch(rid, oe, q, threads=8))


# ---- <robot>.filter_self_from_pointcloud (bindings/robot_helper.hh:284-322) ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_gpu_filter_self_from_pointcloud_matches_oracle(vamp, oracle, name):
    """points overlapping the robot at a configuration or the environment are dropped, the rest keep their order"""
    from envs import make_env
    vamp.set_device(0)
    env, oenv = make_env("mixed", oracle, name)
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(5)
    q = (lo + span * np.float32(0.5)).astype(np.float32)
    fk = oracle.fk(rid, q)
    near = fk[rng.integers(len(fk), size=4000), :3] + rng.normal(0, 0.05, (4000, 3))  # around the robot's spheres
    far = rng.uniform([-1.2, -1.2, -0.2], [1.2, 1.2, 1.6], (6000, 3))
    pc = np.concatenate([near, far]).astype(np.float32)
    rng.shuffle(pc)
    for r in (0.0025, 0.03):
        want = oracle.filter_self_from_pointcloud(rid, oenv, q, pc, r)
        got = getattr(vamp, name).filter_self_from_pointcloud(pc, r, q, env)
        assert 0.05 * len(pc) < len(want) < 0.95 * len(pc)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert getattr(vamp, name).filter_self_from_pointcloud(pc[:0], 0.01, q, env).shape == (0, 3)
