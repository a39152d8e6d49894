"""Cases and queries of the reference-compiled primitive pins (tests/golden/ref_prims.npz).

Test infrastructure.  tools/make_prims_golden.py runs these environments and free spheres through the reference's own
collision/validity.hh, shapes.hh, environment.hh and sphere_*.hh (compiled in place: oracle/ref_prims.cc) and stores
what they answer; the tests regenerate the same inputs from the same seeds and compare the oracle (CPU) and the HIP
path (GPU) with the stored answers.  The SHA-256 of every input array is stored next to the answers.

Three answers per query (oracle/ref_prims.cc): `ref` (the reference as compiled), `nobreak` (the OR of the reference's
own predicate over every primitive, no sorted early break) and `exact` (the reference's loop with max_extent from the
correctly rounded sqrt: the deviation of DESIGN.md §3).  Where ref == nobreak the break cannot have mattered under
either square root, so exact == ref: such a query is a PIN.  Where ref != nobreak the query is `break_decided`: the
reference's answer there depends on the low bits of its approximate sqrt, which depend on the CPU; it is compared with
`exact` and not called a pin, and at most MAX_BREAK_DECIDED of the scalar queries of a case outside the radial and
not-finite families may be such.

Queries.  A quarter are uniform draws (radii over the four robots' min_max_radii range).  The rest are KNIFE-EDGE: the
segment from a sphere that misses (far outside the scene) to one that hits (centred inside a primitive) is bisected in
fp32 on the reference's answer until adjacent floats straddle the flip, and the query takes 3 steps below to 4 above it.
The segments are regenerated from the seed; the bisection's result (one float per segment, `t_lo`) is data the
reference produced and is stored.  Rakes mix 8 distinct spheres: far ones that break at once, knife-edge ones, uniform
ones.

Heightfields: the reference clamps the cell index to [0, xd] x [0, yd], one past the image on both axes.  xs == xd in
any row but the last reads the first cell of the next row, which is defined and pinned here; xs == xd in the last row
and ys == yd read past the buffer, so those queries are kept out of the fixture (`hf_index`) and the product and the
oracle are only required to agree with each other there (both read the last pixel)."""
from __future__ import annotations

import hashlib
import json
import os
import zlib

import numpy as np

from cloud_pins import F32, pack, sha, unpack  # noqa: F401
from vamp_mvt_amd.workloads import RADII

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "ref_prims.npz")
R_LO = min(v[0] for v in RADII.values())
R_HI = max(v[1] for v in RADII.values())
LISTS = ("spheres", "capsules", "z_capsules", "cuboids", "z_cuboids")
WIDTH = dict(spheres=4, capsules=8, z_capsules=8, cuboids=15, z_cuboids=15)
ANSWERS = ("ref", "nobreak", "exact")
MAX_BREAK_DECIDED = 0.001   # share of a case's scalar queries, outside the families below
UNCAPPED = ("radial", "nan", "zero_length")
FAR = 2.5                   # every primitive lies inside a ball of radius 1.25; the missing end of a segment is here
STEPS = tuple(range(-3, 5))


# ---- primitives ------------------------------------------------------------------------------------------------------
def capsule(p1, v, r):
    """x1 y1 z1 | xv yv zv | r | rdv, rdv as collision/factory.hh computes it (double division, narrowed)"""
    p1, v = F32(p1), F32(v)
    dot = F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])
    with np.errstate(divide="ignore"):
        rdv = F(np.float64(1.0) / np.float64(dot))
    return np.array([*p1, *v, r, rdv], np.float32)


def _rot(rng):
    """a general rotation (columns are the cuboid's axes)"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def cuboid(center, rot, half):
    rot = np.asarray(rot, np.float64)
    return np.concatenate([center, rot[:, 0], rot[:, 1], rot[:, 2], half]).astype(np.float32)


def yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _pos(rng, lo=0.3, hi=1.0):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d) * rng.uniform(lo, hi)


def _draw(rng, kind):
    """one small primitive inside the scene ball"""
    if kind == "spheres":
        return "sphere", np.array([*_pos(rng), rng.uniform(0.03, 0.12)], np.float32)
    if kind == "capsules":
        return "capsule", capsule(_pos(rng), rng.uniform(-0.2, 0.2, 3), rng.uniform(0.02, 0.08))
    if kind == "z_capsules":
        return "capsule", capsule(_pos(rng), [0.0, 0.0, rng.choice([-1, 1]) * rng.uniform(0.05, 0.2)], rng.uniform(0.02, 0.08))
    if kind == "cuboids":
        return "cuboid", cuboid(_pos(rng), _rot(rng), rng.uniform(0.02, 0.1, 3))
    return "cuboid", cuboid(_pos(rng), yaw(rng.uniform(-np.pi, np.pi)), rng.uniform(0.02, 0.1, 3))


def mirrored(kind, p):
    """the primitive mirrored in the plane x = 0: the same min_distance, bit for bit"""
    p = np.array(p, np.float32)
    if kind == "sphere":
        p[0] = -p[0]
    elif kind == "capsule":
        p[0], p[3] = -p[0], -p[3]
    else:
        p[[0, 3, 6, 9]] = -p[[0, 3, 6, 9]]
    return p


def heightfield(seed, xd, yd, scale=(0.17, 0.23, 0.9)):
    """centre and scales that are not dyadic; heights in [0.1, 0.4]"""
    rng = np.random.default_rng(seed)
    data = rng.uniform(0.1, 0.4, xd * yd).astype(np.float32)
    return (F32([0.013, -0.021, -0.3]), F32(scale), xd, yd, data)


def route(kind, p):
    """the list a primitive lands in (bindings/environment.cc:111-151)"""
    if kind == "sphere":
        return "spheres"
    if kind == "capsule":
        return "z_capsules" if p[3] == 0 and p[4] == 0 else "capsules"
    return "z_cuboids" if p[11] == F(1.0) else "cuboids"


# ---- cases -----------------------------------------------------------------------------------------------------------
NAN_BEAM = capsule([-1.0, 0.0, 0.0], [2.0, 0.0, 0.0], 0.05)     # the origin lies on its axis: min_distance = 0 / 0
NAN_POLE = capsule([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 0.05)      # z-aligned, starts at the origin
ORDINARY = {"beam": [capsule([0.75, 0.25, 0.1], [0.1, 0.3, 0.2], 0.04), capsule([-0.3, 0.55, 0.35], [-0.2, 0.1, 0.25], 0.06)],
            "pole": [capsule([0.7, -0.35, 0.1], [0.0, 0.0, 0.3], 0.04), capsule([-0.45, 0.4, 0.25], [0.0, 0.0, -0.2], 0.05)]}
ZERO_LENGTH = capsule([0.5, 0.2, 0.3], [0.0, 0.0, 0.0], 0.07)   # rdv = inf; lands in the z-aligned list


def _case(name, family, spec, n_scalar, n_rakes, **kw):
    d = dict(name=name, family=family, spec=spec, n_scalar=n_scalar, n_rakes=n_rakes, seed=zlib.crc32(name.encode()),
             order_defined=True, bisect_on="ref", record=ANSWERS, answer="exact")
    d.update(kw)
    return d


def all_cases():
    """-> list of case dicts; spec = [(kind, params)] in insertion order (the format of tests/envs.py)"""
    out = []
    rng = np.random.default_rng(20240607)
    one = F(1.0)
    zrot = cuboid([0.5, -0.3, 0.4], yaw(0.7), [0.11, 0.07, 0.05])
    assert zrot[11] == one
    almost = zrot.copy()
    almost[11] = np.nextafter(one, F(0.0))                          # 0x1.fffffep-1: the generic list
    singles = [("sphere", [("sphere", F32([0.4, -0.5, 0.3, 0.15]))]),
               ("cuboid", [("cuboid", cuboid([-0.45, 0.35, 0.5], _rot(rng), [0.12, 0.06, 0.09]))]),
               ("cuboid_axis_aligned", [("cuboid", cuboid([0.3, 0.6, -0.2], np.eye(3), [0.1, 0.05, 0.08]))]),
               ("cuboid_yaw_only", [("cuboid", zrot)]),
               ("cuboid_axis3z_below_one", [("cuboid", almost)]),
               ("capsule", [("capsule", capsule([0.3, 0.4, 0.2], [0.25, -0.2, 0.3], 0.06))]),
               ("capsule_z", [("capsule", capsule([-0.4, 0.3, 0.1], [0.0, 0.0, 0.45], 0.05))]),
               ("capsule_z_down", [("capsule", capsule([0.5, 0.5, 0.6], [0.0, 0.0, -0.35], 0.05))]),
               ("capsule_xv_1e-30", [("capsule", capsule([0.45, -0.35, 0.15], [1e-30, 0.0, 0.4], 0.05))])]
    for name, spec in singles:
        assert len({route(k, p) for k, p in spec}) == 1
        out.append(_case("one_" + name, "single", spec, 1600, 200))
    assert route(*singles[3][1][0]) == "z_cuboids" and route(*singles[4][1][0]) == "cuboids"
    assert route(*singles[8][1][0]) == "capsules" and route(*singles[6][1][0]) == "z_capsules"

    for n in (1, 7, 8, 9, 63, 64, 65):
        r = np.random.default_rng(1000 + n)
        spec = [_draw(r, kind) for _ in range(n) for kind in LISTS]
        if n == 8:   # a mirrored pair per kind: equal min_distance, the reference's sort is unstable there
            spec = spec[:-5] + [(k, mirrored(k, p)) for k, p in spec[:5]]
        order = r.permutation(len(spec))
        out.append(_case(f"mixed_{n}", "mixed", [spec[i] for i in order], 4000, 500, ties=(n == 8)))

    # radial approach: the sphere comes from the origin side along the line through the primitive's closest point to
    # the origin, so max_extent meets min_distance exactly where contact begins and the BREAK decides the answer
    r = np.random.default_rng(77)
    radial = {"sphere": [_draw(r, "spheres") for _ in range(3)], "capsule": [_draw(r, "capsules"), _draw(r, "z_capsules")],
              "cuboid": [_draw(r, "cuboids"), _draw(r, "z_cuboids")]}
    radial["mixed"] = [_draw(r, k) for k in LISTS for _ in range(4)]
    for name, spec in radial.items():
        out.append(_case("radial_" + name, "radial", spec, 512, 64))

    for xd, yd in ((4, 4), (16, 16), (5, 3)):
        out.append(_case(f"heightfield_{xd}x{yd}", "heightfield", [("heightfield", heightfield(xd * 100 + yd, xd, yd))], 1600, 200))
    # (cells wide enough for the image to cover the whole scene ball: no query may leave it)
    hf_spec = [("heightfield", heightfield(909, 6, 5, (0.55, 0.7, 0.9)))] + [_draw(r, k) for k in LISTS for _ in range(3)]
    out.append(_case("heightfield_6x5_with_lists", "heightfield", hf_spec, 1600, 200))

    # capsules whose axis passes through the origin, at every insertion position among two ordinary capsules of the
    # same list.  Only insertion-first leaves the reference's sorted order defined.
    for which, nan in (("beam", NAN_BEAM), ("pole", NAN_POLE)):
        for pos in range(3):
            caps = list(ORDINARY[which])
            caps.insert(pos, nan)
            first = pos == 0
            out.append(_case(f"nan_{which}_at_{pos}", "nan", [("capsule", c) for c in caps], 1600, 200, order_defined=first,
                             bisect_on="ref" if first else "nobreak", record=ANSWERS if first else ("nobreak", "exact"),
                             answer="exact" if first else "nobreak"))
    # a zero-length capsule (rdv = inf): the reference's min_distance is a NaN whose sign bit is CLEAR, so its loop breaks
    # at that entry: inserted first, the reference is blind to the whole list (recorded as `ref`).  The product stores 0
    # there, the entry never triggers a break, and the answer is `nobreak`.
    for pos in range(2):
        caps = list(ORDINARY["pole"])
        caps.insert(pos, ZERO_LENGTH)
        first = pos == 0
        out.append(_case(f"zero_length_at_{pos}", "zero_length", [("capsule", c) for c in caps], 1600, 200, order_defined=first,
                         bisect_on="nobreak", record=ANSWERS if first else ("nobreak", "exact"), answer="nobreak"))
    assert len({c["name"] for c in out}) == len(out)
    return out


def spec_sha(spec):
    parts = []
    for kind, p in spec:
        parts.append(kind.encode())
        for a in (p if kind == "heightfield" else (p,)):
            parts.append(np.ascontiguousarray(a, np.float32 if not isinstance(a, int) else np.int64).tobytes())
    return hashlib.sha256(b"".join(parts)).hexdigest()


def prims_of(spec):
    return [(i, kind, p) for i, (kind, p) in enumerate(spec) if kind != "heightfield"]


def hf_of(spec):
    return [p for kind, p in spec if kind == "heightfield"]


# ---- float64 geometry used to AIM queries (never to judge them) -----------------------------------------------------------
def closest_to_origin(kind, p):
    """the point of the primitive's solid closest to the origin, float64"""
    p = np.asarray(p, np.float64)
    if kind == "sphere":
        n = np.linalg.norm(p[:3])
        return p[:3] * (1.0 - p[3] / n)
    if kind == "capsule":
        v = p[3:6]
        vv = v @ v
        t = np.clip(-(p[:3] @ v) / vv, 0.0, 1.0) if vv > 0 else 0.0
        c = p[:3] + t * v
        n = np.linalg.norm(c)
        return c * (1.0 - p[6] / n)
    axes = p[3:12].reshape(3, 3)
    loc = np.clip(axes @ (-p[:3]), -p[12:15], p[12:15])
    return p[:3] + axes.T @ loc


def point_inside(rng, kind, p):
    p = np.asarray(p, np.float64)
    if kind == "sphere":
        return p[:3] + _pos(rng, 0.0, 0.5) * p[3]
    if kind == "capsule":
        return p[:3] + rng.uniform(0, 1) * p[3:6] + _pos(rng, 0.0, 0.5) * p[6]
    axes = p[3:12].reshape(3, 3)
    return p[:3] + axes.T @ (rng.uniform(-0.8, 0.8, 3) * p[12:15])


def hf_index(hf, c):
    """the reference's fp32 cell index (before any clamping to the buffer) for centres c[n][3]; >= xd * yd reads past
    the reference's buffer"""
    centre, scale, xd, yd, _ = hf
    inv = (F(1.0) / F32(scale)).astype(np.float32)
    c = F32(c)
    xo, yo = (centre[0] - c[:, 0]).astype(np.float32), (centre[1] - c[:, 1]).astype(np.float32)
    xs = np.floor(np.clip((inv[0] * xo).astype(np.float32) + F(xd // 2), F(0), F(xd)))
    ys = np.floor(np.clip((inv[1] * yo).astype(np.float32) + F(yd // 2), F(0), F(yd)))
    return (ys * F(xd) + xs).astype(np.int64), xs.astype(np.int64), ys.astype(np.int64)


def hf_height(hf, idx):
    centre, scale, xd, yd, data = hf
    zs = F(1.0) / F32(scale)[2]
    return (zs * data[idx] + centre[2]).astype(np.float32)


def hf_in_bounds(spec, spheres):
    keep = np.ones(len(spheres), bool)
    for hf in hf_of(spec):
        keep &= hf_index(hf, spheres[:, :3])[0] < hf[2] * hf[3]
    return keep


def _hf_safe_xy(rng, hf, n):
    """x, y strictly inside the image, where every cell index is inside the buffer"""
    centre, scale, xd, yd, _ = hf
    x_lo, x_hi = centre[0] - (xd - xd // 2) * scale[0], centre[0] + (xd // 2) * scale[0]
    y_lo, y_hi = centre[1] - (yd - yd // 2) * scale[1], centre[1] + (yd // 2) * scale[1]
    mx, my = 0.02 * scale[0], 0.02 * scale[1]
    return np.stack([rng.uniform(x_lo + mx, x_hi + 2 * scale[0], n), rng.uniform(y_lo + my, y_hi + 2 * scale[1], n)], 1)


# ---- queries ---------------------------------------------------------------------------------------------------------
def _radii(rng, n):
    return np.exp(rng.uniform(np.log(R_LO), np.log(R_HI), n))


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def segments(case, rng, n):
    """-> a[n][3] (misses), b[n][3] (hits), r[n], float32"""
    spec, family = case["spec"], case["family"]
    prims, hfs = prims_of(spec), hf_of(spec)
    r = _radii(rng, n)
    a, b = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        if family == "radial":
            _, kind, p = prims[rng.integers(len(prims))]
            cp = closest_to_origin(kind, p)
            r[i] = rng.uniform(R_LO, 0.1)
            a[i], b[i] = 0.0, cp      # at the origin max_extent = r < every min_distance: each list breaks at once
        elif hfs and (not prims or rng.random() < 0.5):
            hf = hfs[0]
            xy = _hf_safe_xy(rng, hf, 2)
            a[i] = [*xy[0], hf[0][2] + 1.5 + R_HI]
            b[i] = [*xy[1], hf[0][2] - 0.5]
        else:
            _, kind, p = prims[rng.integers(len(prims))]
            b[i] = point_inside(rng, kind, p)
            a[i] = _unit(rng, 1)[0] * FAR
            if hfs:      # stay above the terrain and inside the image on the way in
                a[i] = [*_hf_safe_xy(rng, hfs[0], 1)[0], hfs[0][0][2] + 1.5 + R_HI]
                r[i] = min(r[i], 0.1)
    return F32(a), F32(b), F32(r)


def at(a, b, r, t):
    """the sphere at parameter t of each segment: a + t * (b - a), every operation rounded to fp32"""
    d = (b - a).astype(np.float32)
    c = (a + (t[:, None] * d).astype(np.float32)).astype(np.float32)
    return np.concatenate([c, r[:, None]], 1).astype(np.float32)


def step(t, k):
    t = t.copy()
    for _ in range(abs(k)):
        t = np.nextafter(t, F(2.0) if k > 0 else F(-1.0))
    return t


def bisect(a, b, r, answer):
    """-> t_lo: answer(at(t_lo)) is the miss side and the next float up is not (adjacent floats straddle the flip)"""
    lo, hi = np.zeros(len(a), np.float32), np.ones(len(a), np.float32)
    assert not answer(at(a, b, r, lo)).any() and answer(at(a, b, r, hi)).all(), "a segment does not run from a miss to a hit"
    for _ in range(64):
        mid = (F(0.5) * (lo + hi)).astype(np.float32)
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        h = answer(at(a, b, r, mid))
        lo = np.where(live & ~h, mid, lo)
        hi = np.where(live & h, mid, hi)
    assert (np.nextafter(lo, F(2.0)) == hi).all()
    return lo


def knife(a, b, r, t_lo):
    return np.concatenate([at(a, b, r, step(t_lo, k)) for k in STEPS]).reshape(len(STEPS), -1, 4).transpose(1, 0, 2).reshape(-1, 4)


def _uniform(case, rng, n):
    hfs = hf_of(case["spec"])
    c = rng.uniform(-1.3, 1.3, (n, 3))
    if hfs:
        hf = hfs[0]
        c[:, :2] = _hf_safe_xy(rng, hf, n)
        idx = hf_index(hf, c)[0]
        c[:, 2] = hf_height(hf, np.minimum(idx, hf[2] * hf[3] - 1)) + rng.uniform(-0.05, 0.25, n)
    return np.concatenate([c, _radii(rng, n)[:, None]], 1).astype(np.float32)


def _hf_borders(hf, rng):
    """centres exactly on cell borders in x (every k in 0..xd, the upper border xs == xd included) and in y (rows below
    the last), one fp32 step to either side too, just above / on / below the surface of the cell they read"""
    centre, scale, xd, yd, _ = hf
    xs = [F(centre[0] - F(k - xd // 2) * scale[0]) for k in range(xd + 1)]
    ys = [F(centre[1] - F(j - yd // 2) * scale[1]) for j in range(yd)]
    ys += [F(y - F(0.37) * scale[1]) for y in ys]
    pts = []
    for x in xs:
        for dx in (-1, 0, 1):
            xx = step(F32([x]), dx)[0]
            for y in ys:
                for dy in (-1, 0, 1):
                    pts.append((xx, step(F32([y]), dy)[0]))
    xy = F32(pts)
    if len(xy) > 400:    # a sample, of which a quarter at the upper x border
        upper = np.flatnonzero(xy[:, 0] <= xs[-1])
        upper = upper[np.sort(rng.choice(len(upper), min(len(upper), 100), replace=False))]
        rest = np.sort(rng.choice(len(xy), 300, replace=False))
        xy = xy[np.union1d(upper, rest)]
    r = F32(rng.uniform(R_LO, 0.1, len(xy)))
    c = np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], 1)
    idx = hf_index(hf, c)[0]
    ok = idx < xd * yd
    c, r, idx = c[ok], r[ok], idx[ok]
    c[:, 2] = (hf_height(hf, idx) + r + F32(rng.choice([-1e-3, 0.0, 1e-3], len(c)))).astype(np.float32)
    return np.concatenate([c, r[:, None]], 1).astype(np.float32)


def n_segments(case):
    return (case["n_scalar"] * 3 // 4) // len(STEPS)


def make_queries(case, t_lo=None, answer=None):
    """-> dict(scalar [n][4], rakes [m][8][4], t_lo); with t_lo None the segments are bisected on answer(spheres)"""
    rng = np.random.default_rng(case["seed"])
    a, b, r = segments(case, rng, n_segments(case))
    if t_lo is None:
        t_lo = bisect(a, b, r, answer)
    kn = knife(a, b, r, F32(t_lo))
    parts = [kn]
    hfs = hf_of(case["spec"])
    if hfs:
        parts.append(_hf_borders(hfs[0], rng))
    parts.append(_uniform(case, rng, max(case["n_scalar"] - sum(len(p) for p in parts), 0)))
    scalar = np.concatenate(parts)
    scalar = scalar[hf_in_bounds(case["spec"], scalar)][:case["n_scalar"]]
    # rakes: lanes drawn from far spheres (every list breaks at its first entry), knife-edge and uniform ones
    m = case["n_rakes"]
    far = np.concatenate([_unit(rng, 8 * m) * rng.uniform(2.0, 3.0, (8 * m, 1)), _radii(rng, 8 * m)[:, None]], 1).astype(np.float32)
    if hfs:
        far[:, :2] = _hf_safe_xy(rng, hfs[0], 8 * m)
        far[:, 2] = np.abs(far[:, 2]) + 1.0
    pool = scalar[rng.integers(len(scalar), size=8 * m)]
    share = rng.choice([0.0, 0.15, 0.5, 1.0], size=(m, 1))          # of a rake's lanes that come from the pool
    lanes = rng.random((m, 8)) < share
    lanes[np.arange(m), rng.integers(8, size=m)] |= share[:, 0] > 0  # at least one such lane
    rakes = np.where(lanes.reshape(-1)[:, None], pool, far).astype(np.float32).reshape(m, 8, 4)
    return dict(scalar=np.ascontiguousarray(scalar), rakes=np.ascontiguousarray(rakes), t_lo=F32(t_lo))


# ---- sorted lists ----------------------------------------------------------------------------------------------------
def stored_min_distance(md):
    """the product's rule (include/vamp_mvt_amd.h): a min_distance that is not finite is stored as 0"""
    md = F32(md).copy()
    md[~np.isfinite(md)] = 0.0
    return md


def expected_lists(case, order, md):
    """the reference's sorted lists as {list: rows [n][width + 1]}: parameters from the regenerated spec in the stored
    order, min_distance as stored; where a min_distance is not finite, the rule above and a stable re-sort (the
    reference's own order is not defined there unless the entry was inserted first)"""
    out = {}
    for name in LISTS:
        o, d = order.get(name), md.get(name)
        if o is None:
            out[name] = np.zeros((0, WIDTH[name] + 1), np.float32)
            continue
        rows = np.array([np.concatenate([F32(case["spec"][i][1]), [0]]) for i in o], np.float32)
        rows[:, -1] = stored_min_distance(d)
        out[name] = rows[np.argsort(rows[:, -1], kind="stable")]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_lists(got, want):
    """bit for bit: the min_distance column in order, and the rows of every run of equal min_distance as a multiset"""
    if got.shape != want.shape:
        return False
    if len(got) == 0:
        return True
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g[:, -1], w[:, -1]):
        return False
    key = lambda u: u[np.lexsort(u.T[::-1])]
    for v in np.unique(g[:, -1]):
        sel = g[:, -1] == v
        if not np.array_equal(key(g[sel]), key(w[sel])):
            return False
    return True


# ---- fixture ---------------------------------------------------------------------------------------------------------
def load():
    z = np.load(FIXTURE)
    return json.loads(bytes(z["meta"]).decode()), z


class Case:
    """one case of the fixture with its inputs regenerated (and checked against the stored digests)"""

    def __init__(self, spec_case, meta, z):
        self.__dict__.update(spec_case)
        self.case, self.meta, self.z = spec_case, meta, z
        assert spec_sha(self.spec) == meta["spec_sha"], f"{self.name}: the regenerated environment differs from the fixture's"
        q = make_queries(spec_case, t_lo=z[f"{self.name}__t_lo"])
        assert sha(q["scalar"]) == meta["scalar_sha"] and sha(q["rakes"]) == meta["rakes_sha"], \
            f"{self.name}: the regenerated queries differ from the ones the fixture was made from"
        self.scalar, self.rakes = q["scalar"], q["rakes"]

    def has(self, key):
        return f"{self.name}__{key}" in self.z.files

    def out(self, key, rake=False):
        return unpack(self.z[f"{self.name}__{'rake_' if rake else ''}{key}"], len(self.rakes) if rake else len(self.scalar))

    def lists(self):
        order = {k: self.z[f"{self.name}__{k}_order"] for k in LISTS if self.has(f"{k}_order")}
        md = {k: self.z[f"{self.name}__{k}_md"] for k in order}
        return expected_lists(self.case, order, md)

    def want(self, rake=False):
        """what the oracle and the product must answer: `exact`; where the reference's order is not defined the rule
        makes that `nobreak` (the generator and test_ref_prim_pins.py assert the two coincide there)"""
        return self.out(self.answer, rake)


_cache = {}


def cases():
    if not _cache:
        meta, z = load()
        by_name = {m["name"]: m for m in meta["cases"]}
        specs = all_cases()
        assert {c["name"] for c in specs} == set(by_name), "the fixture's cases and the generators' differ"
        for c in specs:
            _cache[c["name"]] = Case(c, by_name[c["name"]], z)
    return _cache


def names(keep=lambda m: True):
    return [m["name"] for m in load()[0]["cases"] if keep(m)]
