"""Cases and queries of the reference-compiled point-cloud pins (tests/golden/ref_{mvt,capt,scdf,centervox}.npz).

Test infrastructure.  tools/make_cloud_golden.py runs these inputs through the reference's own collision/mvt.hh,
capt.hh, filter.hh and filter_centervox.hh (compiled in place: oracle/ref_cloud.cc) and stores what they answer; the
tests regenerate the same inputs from the same seeds and compare the oracle (CPU) and the HIP path (GPU) with the stored
answers.  Every input array's SHA-256 is stored next to the answers, so a generator that drifts fails loudly.

The shapes are the smallest at which these structures go wrong: one point, a voxel filled to capacity and one over,
clouds straddling the power-of-two padding and the 8-wide affordance vectors, points exactly on cell borders and
workspace faces, and `knife-edge` queries whose squared distance EQUALS the squared query radius in fp32."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from pins import scene_cloud
from vamp_mvt_amd.workloads import POINT_RADIUS, RADII, WORKSPACE, shell_cloud

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROBOTS = ("panda", "fetch", "baxter")
N_SCALAR = {"mvt": 6000, "capt": 4000}
N_RAKES = {"mvt": 750, "capt": 500}
# exactly representable workspace / radii: grid width 16, cell 0.125, inverse scale factor exactly 8
DYADIC_WS = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
DYADIC_MVT = (0.012, 0.125, *DYADIC_WS, 0.0078125)
MAX_TIE_DEPENDENT = 1  # per family (scdf, CAPT), over every case whose input can be chosen free of ties
# Inputs that cannot: they are recorded and compared as the stable-order variant, never called pins, and do not count
# towards the cap.
#  * scene_cloud(5000, seed): the first curve alone puts about 19 pairs of distinct points into one Morton cell (2.4 mm)
#    and which of the two survives depends on their order; none of the seeds 0..299 is free of it
#  * the survey's 10,000-point cloud is given (mt19937 seed 0), and its stream repeats three coordinates: at the Fetch
#    and Baxter radii the ORDER of the afforded points inside some leaves follows the tie order (array `aff` only;
#    tests, aabbs, aff_starts, the top box and every count are identical under both orders, and are pinned)
TIE_EXEMPT = {"scdf": tuple(f"n5000_cull{c}_d{d}" for c in (1, 0) for d in (0.02, 0.05)),
              "capt": tuple(f"survey_{v}_{r}" for v in ("fma", "plain") for r in ("fetch", "baxter"))}


def F32(a):
    return np.asarray(a, np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pack(bits):
    return np.packbits(np.asarray(bits, bool))


def unpack(packed, n):
    return np.unpackbits(np.asarray(packed, np.uint8))[:n].astype(bool)


def _mvt_params(robot):
    return (RADII[robot][0], RADII[robot][1], *WORKSPACE[robot], POINT_RADIUS)


def mvt_pool_cases():
    """the six clouds of test_mvt_pool_limits_match_between_product_and_oracle"""
    panda = _mvt_params("panda")
    return [
        (shell_cloud(1500, 3, 0.5, 1.0, 0.0, 1.2), panda),                     # fits
        (shell_cloud(10000, 3), panda),                                         # pools run out
        (np.random.default_rng(0).uniform(-1, 1, (5000, 3)).astype(np.float32), panda),   # > 10 % of voxels
        (np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (70, 1)) + np.float32(1e-4) * np.arange(70)[:, None], panda),
        (shell_cloud(300, 4), _mvt_params("fetch")),
        (shell_cloud(50, 4), _mvt_params("baxter")),
    ]


def dyadic_border_cloud():
    """points exactly on the workspace's min and max corners, on its faces and on interior cell borders (multiples of
    the cell width 0.125), every coordinate a multiple of 2^-10"""
    rng = np.random.default_rng(77)
    p = rng.integers(-1024, 1025, (48, 3)) / 1024.0
    rows = np.arange(48)
    p[rows, rng.integers(0, 3, 48)] = rng.integers(-8, 9, 48) * 0.125
    p[rows[::3], rng.integers(0, 3, 16)] = rng.integers(-8, 9, 16) * 0.125
    head = [[-1, -1, -1], [1, 1, 1], [1, -1, 0.5], [-1, 1, -0.25], [0.875, 0.875, 0.875], [1, 1, 0.875]]
    return np.concatenate([np.array(head, np.float64), p]).astype(np.float32)


def one_voxel_cloud(n):
    """n points inside Panda grid cell (20, 15, 15): capacity is 64 per voxel (mvt.hh:455-468)"""
    lo, hi = (np.array(a, np.float32) for a in WORKSPACE["panda"])
    width = F(hi[0] - lo[0])
    cell = width / F(np.floor(width / F(0.08)))
    centre = lo + (np.array([20, 15, 15], np.float32) + F(0.5)) * cell
    return (centre + np.random.default_rng(64).uniform(-0.02, 0.02, (65, 3))[:n]).astype(np.float32)


def mvt_cases():
    """-> [(name, points, (r_min, r_max, ws_min, ws_max, r_point))]"""
    panda = _mvt_params("panda")
    cases = [("one_point", np.array([[0.5, 0.1, 0.4]], np.float32), panda),
             ("voxel_full_64", one_voxel_cloud(64), panda),
             ("voxel_over_65", one_voxel_cloud(65), panda),
             ("shell_1500", shell_cloud(1500, 3, 0.5, 1.0, 0.0, 1.2), panda),
             ("dyadic_borders", dyadic_border_cloud(), DYADIC_MVT),
             # the other robots' radii on clouds small enough for their pools (grid 12 and 6: pool_4 and pool_5 run out)
             ("fetch_40", shell_cloud(40, 5), _mvt_params("fetch")),
             ("baxter_12", shell_cloud(12, 6), _mvt_params("baxter"))]
    cases += [(f"pool_{i}", pts, params) for i, (pts, params) in enumerate(mvt_pool_cases())]
    return cases


# ---- queries ---------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _near(rng, pts, n, r_lo, r_hi, r_point, u_max=1.8):
    """centre at (r + r_point) * u from a cloud point in a random direction, u uniform in [0, u_max): about 1 / u_max
    of them touch that point, the rest depend on its neighbours"""
    p = pts[rng.integers(len(pts), size=n)].astype(np.float64)
    r = rng.uniform(r_lo, r_hi, n)
    c = p + _unit(rng, n) * ((r + r_point) * rng.uniform(0, u_max, n))[:, None]
    return np.concatenate([c, r[:, None]], 1).astype(np.float32)


def _box(rng, pts, n, r_lo, r_hi, margin):
    lo, hi = pts.min(0).astype(np.float64) - margin, pts.max(0).astype(np.float64) + margin
    return np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.uniform(r_lo, r_hi, (n, 1))], 1).astype(np.float32)


def _radius_for(qr, r_point):
    """-> (r_minus, r, r_plus): fl(r + r_point) == qr exactly, one fp32 step of the sum below / above for the others;
    None if no fp32 r gives exactly qr"""
    rp = F(r_point)
    r = F(F(qr) - rp)
    for _ in range(4):
        s = F(r + rp)
        if s == qr:
            break
        r = np.nextafter(r, F(np.inf) if s < qr else F(-np.inf))
    else:
        return None
    lo = r
    while F(lo + rp) >= qr:
        lo = np.nextafter(lo, F(-np.inf))
    hi = r
    while F(hi + rp) <= qr:
        hi = np.nextafter(hi, F(np.inf))
    return lo, r, hi


def knife_edge(pts, r_point, want=40, ks=range(8, 41), inside=None):
    """Queries at the exact fp32 contact boundary of one cloud point: the centre is the point moved by qr = k / 512
    along one axis, exactly (c - p == qr without rounding, so c -+ qr is p again in the box tests), so dist^2 ==
    fl(qr * qr) == (r + r_point)^2 bit for bit, and every other point is farther than 1.01 qr; `inside` = (lo, hi) keeps
    the centres within the MVT's workspace (outside it the reference's cell walk can pass the point by).  Per site four
    queries -> expected answers
        r with fl(r + r_point) == qr  -> hit (the reference tests `<=`)
        the sum one step below        -> miss
        the sum one step above        -> hit
        centre one step farther out   -> miss (the first fp32 centre whose rounded offset exceeds qr)
    -> (spheres [4 m][4], expected bool[4 m])"""
    pts = np.ascontiguousarray(pts, np.float32)
    p64 = pts.astype(np.float64)
    out, expect, sites = [], [], 0
    order = np.argsort(-np.abs(p64 - p64.mean(0)).max(1), kind="stable")  # outermost points first: most isolated
    ks, n = list(ks), len(order)
    for t in range(min(6 * len(ks) * n, 6000)):  # every point in turn, then the next (axis, side, k) combination
        i, u = int(order[t % n]), t // n
        axis, sign = u % 3, (1.0, -1.0)[(u // 3) % 2]
        k = ks[(7 * (u // 6) + 5 * i) % len(ks)]
        qr = F(k / 512.0)
        radii = _radius_for(qr, r_point)
        c = pts[i].copy()
        c[axis] = F(pts[i, axis] + F(sign) * qr)
        if radii is None or float(c[axis]) - float(pts[i, axis]) != sign * float(qr):
            continue
        if inside is not None and not (np.all(c >= F32(inside[0])) and np.all(c <= F32(inside[1]))):
            continue
        d = np.linalg.norm(p64 - c.astype(np.float64), axis=1)
        d[i] = np.inf
        if d.min() <= 1.01 * float(qr):
            continue
        far = c.copy()
        far[axis] = np.nextafter(c[axis], F(sign * np.inf))
        while F(far[axis] - pts[i, axis]) == F(sign) * qr:  # until the rounded difference moves, too
            far[axis] = np.nextafter(far[axis], F(sign * np.inf))
        if inside is not None and not (F32(inside[0])[axis] <= far[axis] <= F32(inside[1])[axis]):
            continue
        out += [[*c, radii[1]], [*c, radii[0]], [*c, radii[2]], [*far, radii[1]]]
        expect += [True, False, True, False]
        sites += 1
        if sites == want:
            break
    return np.array(out, np.float32).reshape(-1, 4), np.array(expect, bool)


def top_box_knife(pts, r_point, want=12, ks=range(8, 41)):
    """CAPT tests its top box WITHOUT r_point (capt.hh:376, :431-438): the centre lies exactly r outside a face of the
    cloud's bounding box, straight out from the point that defines the face.  -> [r (touches the box: passes, then
    hits that point, which is r < r + r_point away), one step smaller r (outside the box: miss, although the point is
    within r + r_point)]"""
    pts = np.ascontiguousarray(pts, np.float32)
    out, expect = [], []
    for t in range(6 * want):
        axis, up = t % 3, (t // 3) % 2 == 0
        i = int(np.argmax(pts[:, axis]) if up else np.argmin(pts[:, axis]))
        r = F(list(ks)[(5 * t) % len(ks)] / 512.0)
        s = F(1.0 if up else -1.0)
        c = pts[i].copy()
        c[axis] = F(pts[i, axis] + s * r)
        if float(c[axis]) - float(pts[i, axis]) != float(s) * float(r):
            continue
        r_less = np.nextafter(r, F(0))
        if F(r_less * r_less) == F(r * r):
            continue
        out += [[*c, r], [*c, r_less]]
        expect += [True, False]
        if len(out) == 2 * want:
            break
    return np.array(out, np.float32).reshape(-1, 4), np.array(expect, bool)


def _box_face_queries(rng, pts, r_lo, r_hi, r_point, per_side=8):
    """centres whose reach ends exactly on a face of the cloud's bounding box, and one fp32 step farther out (MVT's
    global-box early exit, mvt.hh:211-218), straight out from the point that defines the face"""
    rp = F(r_point)
    out = []
    for axis in range(3):
        for up in (False, True):
            i = int(np.argmax(pts[:, axis]) if up else np.argmin(pts[:, axis]))
            face = pts[i, axis]
            for r in rng.uniform(r_lo, r_hi, per_side).astype(np.float32):
                qr = F(r + rp)
                inf = F(np.inf)
                if up:   # passes while fl(c - qr) <= face
                    c = F(face + qr)
                    while F(c - qr) > face:
                        c = np.nextafter(c, -inf)
                    while F(np.nextafter(c, inf) - qr) <= face:
                        c = np.nextafter(c, inf)
                    beyond = np.nextafter(c, inf)
                else:    # passes while fl(c + qr) >= face
                    c = F(face - qr)
                    while F(c + qr) < face:
                        c = np.nextafter(c, inf)
                    while F(np.nextafter(c, -inf) + qr) >= face:
                        c = np.nextafter(c, -inf)
                    beyond = np.nextafter(c, -inf)
                for v in (c, beyond):
                    q = [*pts[i], r]
                    q[axis] = v
                    out.append(q)
    return np.array(out, np.float32)


def _rakes(rng, scalar, knife_lo, knife_hi, n_rakes, far):
    """8-lane rakes whose lanes differ: one to three lanes come from the scalar queries, the rest lie far outside the
    cloud's box (`far`), so lanes inside and outside the box share a rake; the first rakes carry one knife-edge query
    each, alone, so the rake's answer is that query's"""
    rakes = np.zeros((n_rakes, 8, 4), np.float32)
    rakes[:, :, :3] = (far + rng.uniform(0, 1, (n_rakes, 8, 3))).astype(np.float32)
    rakes[:, :, 3] = scalar[rng.integers(len(scalar), size=(n_rakes, 8)), 3]
    n_knife = min(knife_hi - knife_lo, n_rakes // 3)
    for j in range(n_rakes):
        if j < n_knife:
            rakes[j, rng.integers(8)] = scalar[knife_lo + j]
        else:
            lanes = rng.permutation(8)[:rng.integers(1, 4)]
            rakes[j, lanes] = scalar[rng.integers(len(scalar), size=len(lanes))]
    return rakes


def mvt_queries(pts, params, seed):
    """-> dict(scalar [6000][4], rakes [750][8][4], knife=(lo, hi), expect bool[hi - lo])"""
    r_min, r_max, lo, hi, r_point = params
    rng = np.random.default_rng(seed)
    lo, hi = np.array(lo, np.float64), np.array(hi, np.float64)
    knife, expect = knife_edge(pts, r_point, inside=(lo, hi))
    faces = _box_face_queries(rng, pts, r_min, r_max, r_point)
    above = _near(rng, pts, 400, r_max, 3 * r_max, r_point)            # radii above r_max: the one-cell clamp
    # ... kept inside the workspace: below it (centre - workspace_min) * scale + 1 can fall under -1, and the
    # reference's cast of that to uint16 is undefined (mvt.hh:228; on x86 it walks 65,535 cells off the table)
    above[:, :3] = np.clip(above[:, :3], lo.astype(np.float32), hi.astype(np.float32))
    outside = _near(rng, pts, 400, r_min, r_max, r_point)              # centres outside the workspace, within reach of it
    axis, up = rng.integers(0, 3, 400), rng.integers(0, 2, 400).astype(bool)
    off = rng.uniform(0, r_max, 400)
    outside[np.arange(400), axis] = np.where(up, hi[axis] + off, lo[axis] - off).astype(np.float32)
    n_rest = N_SCALAR["mvt"] - len(knife) - len(faces) - 800
    near = _near(rng, pts, n_rest // 2, r_min, r_max, r_point)
    box = _box(rng, pts, n_rest - n_rest // 2, r_min, r_max, 2 * r_max)
    scalar = np.concatenate([knife, faces, above, outside, near, box])
    assert scalar.shape == (N_SCALAR["mvt"], 4) and np.isfinite(scalar).all()
    rakes = _rakes(rng, scalar, 0, len(knife), N_RAKES["mvt"], pts.max(0).astype(np.float64) + 10 * r_max + 1)
    return dict(scalar=scalar, rakes=rakes, knife=(0, len(knife)), expect=expect, sites=(len(knife) // 4, 0))


def knife_report(hits, q):
    """How the answers `hits` to q["scalar"] fall on the knife-edge sites: a site is `live` if it answers as expected
    (hit at equality, miss one step beyond), `dead` if every query of it misses (the site's point is not reachable from
    the centre's cell: the CAPT's own false negatives; the MVT has none inside its workspace), `other`
    for anything else, which no boundary explains."""
    lo, hi = q["knife"]
    rep = dict(live=0, dead=0, other=0)
    at = lo
    for width, count in ((4, q["sites"][0]), (2, q["sites"][1])):
        for _ in range(count):
            got, want = hits[at:at + width], q["expect"][at - lo:at - lo + width]
            rep["live" if np.array_equal(got, want) else "dead" if not got.any() else "other"] += 1
            at += width
    assert at == hi
    return rep


CAPT_SIZES = (1, 2, 7, 8, 9, 17, 255, 256, 257, 1000)


def tied_cloud():
    """9 points padded to 16: the root's median falls between the two largest x, which are EQUAL here while y and z
    differ, so the order in which the sort leaves them decides which point each half receives"""
    pts = shell_cloud(9, 409)
    a, b = np.argsort(pts[:, 0])[-2:]
    pts[a, 0] = pts[b, 0]
    return pts


def capt_cases():
    """-> [(name, points, (r_min, r_max, r_point))]: every cloud size at each robot's radii, and a cloud built to
    depend on the order of equal keys"""
    cases = [(f"n{n}_{robot}", shell_cloud(n, 100 + n), (*RADII[robot], POINT_RADIUS))
             for n in CAPT_SIZES for robot in ROBOTS]
    cases.append(("tied_x_panda", tied_cloud(), (*RADII["panda"], POINT_RADIUS)))
    return cases


def capt_queries(pts, params, seed):
    """-> dict(scalar [4000][4], rakes [500][8][4], knife=(lo, hi), expect): knife-edge queries against r + r_point and
    against the top box, then half near the cloud's points and half spread over its enlarged box"""
    r_min, r_max, r_point = params
    rng = np.random.default_rng(seed)
    # centres inside the cloud's box: outside it the top-box test, made WITHOUT r_point, answers first
    k1, e1 = knife_edge(pts, r_point, inside=(pts.min(0), pts.max(0)))
    k2, e2 = top_box_knife(pts, r_point)
    knife, expect = np.concatenate([k1, k2]), np.concatenate([e1, e2])
    n_rest = N_SCALAR["capt"] - len(knife)
    near = _near(rng, pts, n_rest // 2, r_min, r_max, r_point)
    box = _box(rng, pts, n_rest - n_rest // 2, r_min, r_max, 2 * r_max)
    scalar = np.concatenate([knife, near, box])
    assert scalar.shape == (N_SCALAR["capt"], 4) and np.isfinite(scalar).all()
    rakes = _rakes(rng, scalar, 0, len(knife), N_RAKES["capt"], pts.max(0).astype(np.float64) + 10 * r_max + 1)
    return dict(scalar=scalar, rakes=rakes, knife=(0, len(knife)), expect=expect, sites=(len(k1) // 4, len(k2) // 2))


def survey_capt_cases():
    """the survey's 10,000-point cloud (pins.capt_cloud) in both roundings at the three robots' radii: too large to
    store, kept as shapes + digests"""
    import pins
    return [(f"survey_{'fma' if fma else 'plain'}_{robot}", (fma,), (*RADII[robot], POINT_RADIUS))
            for fma in (True, False) for robot in ROBOTS], pins.capt_cloud


# ---- filters ---------------------------------------------------------------------------------------------------------
ORIGIN = np.array([0.0, 0.0, 0.333], np.float32)
RANGE = np.float32(1.19)
LO, HI = ORIGIN - RANGE, ORIGIN + RANGE
SCDF_SEED = {1: 31, 2: 32, 300: 33, 5000: 34}
CENTERVOX_SEED = {1: 51, 64: 52, 5000: 53}
EXHAUSTION = dict(n=90000, seed=9, voxel_size=0.004)


def near_duplicates_cloud():
    """scene_cloud(300) plus 24 of its points moved by 1e-5: each pair shares its Morton cell on every curve, so the
    order of equal codes decides which of the two is kept"""
    pc = scene_cloud(300, 35)
    twins = pc[10:250:10] + np.float32(1e-5)
    return np.concatenate([pc, twins]).astype(np.float32)


def scdf_cases():
    """-> [(name, cloud, min_dist, max_range, origin, lo, hi, cull)]"""
    cases = []
    for n, seed in SCDF_SEED.items():
        pc = scene_cloud(n, seed)
        for cull in (True, False):
            for min_dist in (0.02, 0.05):
                cases.append((f"n{n}_cull{int(cull)}_d{min_dist}", pc, min_dist, RANGE, ORIGIN, LO, HI, cull))
    rng = np.random.default_rng(36)
    inside = (ORIGIN + rng.uniform(-0.6, 0.6, (40, 3))).astype(np.float32)
    first_culled = inside.copy()
    first_culled[0] = [3.0, -2.5, 0.1]           # the tail entries of filter.hh:195-216 all name point 0
    cases.append(("point0_culled", first_culled, 0.05, RANGE, ORIGIN, LO, HI, True))
    cases.append(("point0_kept", inside, 0.05, RANGE, ORIGIN, LO, HI, True))
    cases.append(("all_culled", (inside + np.float32(5.0)).astype(np.float32), 0.05, RANGE, ORIGIN, LO, HI, True))
    cases.append(("near_duplicates", near_duplicates_cloud(), 0.02, RANGE, ORIGIN, LO, HI, True))
    return cases


def centervox_cases():
    """-> [(name, cloud or None, voxel_size, max_range, origin, lo, hi)]; the exhaustion case carries no cloud (seed
    only: scene_cloud(**EXHAUSTION))"""
    cases = []
    for n, seed in CENTERVOX_SEED.items():
        # scene_cloud's point 0 is culled by construction: the one-point cloud is a point that is not
        pc = scene_cloud(n, seed) if n > 1 else (ORIGIN + np.array([[0.3, -0.2, 0.1]], np.float32)).astype(np.float32)
        for vs in (0.03, 0.0303, 0.2):
            cases.append((f"n{n}_vs{vs}", pc, vs, RANGE, ORIGIN, LO, HI))
    lo, hi = (np.array(a, np.float32) for a in DYADIC_WS)
    zero = np.zeros(3, np.float32)
    # voxel 0.125 over [-1, 1]^3: grid 16, inverse scale factor exactly 8; points on voxel borders and workcell faces
    cases.append(("dyadic_borders", dyadic_border_cloud(), 0.125, 4.0, zero, lo, hi))
    # pairs exactly equidistant from their voxel's centre (0.0625 + 0.125 k): the FIRST one inserted stays
    # (filter_centervox.hh:34 `<`); in the second and third pair the order of the two is swapped
    c = np.array([0.0625, 0.0625, 0.0625])
    d = np.array([0.03125, 0.0, 0.0])
    e = np.array([0.0, 0.015625, 0.0])
    pairs = [c + d, c - d, c + 0.25 - d, c + 0.25 + d, c - 0.5 + e, c - 0.5 - e, c + 0.5 + d, c + 0.5 + e]
    cases.append(("equidistant", np.array(pairs, np.float32), 0.125, 4.0, zero, lo, hi))
    cases.append(("exhaustion", None, EXHAUSTION["voxel_size"], RANGE, ORIGIN, LO, HI))
    return cases


# ---- fixtures --------------------------------------------------------------------------------------------------------
def load(family):
    """-> (meta dict, arrays) of tests/golden/ref_<family>.npz"""
    z = np.load(os.path.join(GOLDEN, f"ref_{family}.npz"))
    return json.loads(bytes(z["meta"]).decode()), z


class Case:
    """one case of a fixture with its inputs regenerated (and checked against the stored digests) and the reference's
    recorded outputs"""

    def __init__(self, family, meta, z, **inputs):
        self.family, self.meta, self.z, self.name = family, meta, z, meta["name"]
        self.__dict__.update(inputs)

    def out(self, key, n=None):
        a = self.z[f"{self.name}__{key}"]
        return a if n is None else unpack(a, n)


def _check_sha(what, array, digest):
    assert sha(array) == digest, f"{what}: the regenerated input differs from the one the fixture was made from"


_cache = {}


def cases(family):
    """-> {name: Case} of tests/golden/ref_<family>.npz, built once per process"""
    if family in _cache:
        return _cache[family]
    meta, z = load(family)
    by_name = {m["name"]: m for m in meta["cases"]}
    out = {}
    if family == "mvt":
        for name, pts, params in mvt_cases():
            m = by_name[name]
            _check_sha(name, pts, m["pts_sha"])
            out[name] = Case(family, m, z, pts=pts, params=params)
    elif family == "capt":
        survey, cloud = survey_capt_cases()
        for name, pts, params in capt_cases():
            _check_sha(name, pts, by_name[name]["pts_sha"])
            out[name] = Case(family, by_name[name], z, pts=pts, params=params)
        clouds = {}
        for name, (fma,), params in survey:
            out[name] = Case(family, by_name[name], z, params=params, make_pts=lambda fma=fma: clouds.get(fma) if fma in clouds
                             else clouds.setdefault(fma, cloud(0, fma=fma)))
    elif family == "scdf":
        for name, pc, *args in scdf_cases():
            _check_sha(name, pc, by_name[name]["pts_sha"])
            out[name] = Case(family, by_name[name], z, pts=pc, args=tuple(args))
    else:
        for name, pc, *args in centervox_cases():
            out[name] = Case(family, by_name[name], z, pts=pc, args=tuple(args))
            if pc is not None:
                _check_sha(name, pc, by_name[name]["pts_sha"])
    assert set(out) == set(by_name), "the fixture's cases and the generators' differ"
    _cache[family] = out
    return out


def queries(case):
    """the regenerated queries of an MVT or CAPT case (cached on the case)"""
    if not hasattr(case, "_q"):
        make = mvt_queries if case.family == "mvt" else capt_queries
        q = make(case.pts, case.params, case.meta["seed"])
        _check_sha(case.name + " scalar queries", q["scalar"], case.meta["scalar_sha"])
        _check_sha(case.name + " rakes", q["rakes"], case.meta["rakes_sha"])
        case._q = q
    return case._q


def exhaustion_cloud():
    return scene_cloud(EXHAUSTION["n"], EXHAUSTION["seed"])


def names(family, keep=lambda m: True):
    """case names of a committed fixture, for parametrize (read from the fixture's own list)"""
    return [m["name"] for m in load(family)[0]["cases"] if keep(m)]


CAPT_KEYS = ("tests", "aff_starts", "aabbs", "aff", "aabb_top")


def built(m):
    return m["status"] == "built"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_capt_arrays(case, got):
    """got: dict of a CAPT's arrays -> bit for bit the reference's (stored arrays, else shapes + SHA-256)"""
    m = case.meta
    assert got["nlog2"] == m["nlog2"] and got["aff"].shape[1] == m["n_vectors"]
    for k in CAPT_KEYS:
        a = np.ascontiguousarray(got[k])
        assert list(a.shape) == m["shapes"][k], (case.name, k)
        if m["arrays_stored"]:
            assert np.array_equal(bits(a), bits(case.out(k))), (case.name, k)
        assert sha(a) == m["sha"][k], (case.name, k)
