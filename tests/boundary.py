"""Inputs at the exact fp32 contact boundary: configuration pairs, edges and free spheres one step either side of the
oracle's answer.

Test infrastructure, like workmix.py.  Uniform or perturbed samples almost never put a sphere within a margin's width of
touching (a handful in 12,000 within 1e-4 m), so a certified-free shortcut whose margin is wrong by tens of microns, or
a `<` / `<=` slip in a narrow-phase predicate, would pass every parity test.  The generators here bisect in fp32 until
two inputs one representable step apart straddle the oracle's answer; the contact that decides them is then within
~1e-7 m.  Bisection is vectorised over oracle batch calls; seeds are explicit (workmix.case_seed)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

import geom64
from workmix import _scaled_noise, mixed_configs, valid_seeds

THREADS = 16
_fp = ctypes.POINTER(ctypes.c_float)


@dataclass
class BoundaryPairs:
    q_lo: np.ndarray    # [n][dim] valid by the oracle
    q_hi: np.ndarray    # [n][dim] invalid by the oracle, one fp32 step along the segment from q_lo
    label: np.ndarray   # [n] the contact that decides the pair: "self", an environment kind, or "attachment"
    clear_lo: dict      # {kind: [n]} float64 clearances at q_lo (geom64.clearances)
    clear_hi: dict      # {kind: [n]} float64 clearances at q_hi
    a: np.ndarray       # segment start (valid endpoint)
    d: np.ndarray       # segment direction (fp32 b - a): q(t) = a + t * d in fp32
    t_lo: np.ndarray    # [n] fp32
    t_hi: np.ndarray    # [n] fp32

    def configs(self):
        """q_lo then q_hi, and the oracle's answers for them"""
        return np.concatenate([self.q_lo, self.q_hi]), np.r_[np.ones(len(self.q_lo), bool), np.zeros(len(self.q_hi), bool)]

    def counts(self):
        kinds, n = np.unique(self.label, return_counts=True)
        return dict(zip(kinds.tolist(), n.tolist()))


def _at(a, d, t):
    return (a + t[:, None] * d).astype(np.float32)


def bisect_segments(oracle, rid, oenv, a, b, rounds=200):
    """a valid, b invalid (oracle) -> t_lo, t_hi (fp32) with q(t_lo) valid, q(t_hi) invalid and no configuration
    between them: t_lo, t_hi adjacent floats, or q(t_mid) equal to one of the two ends."""
    a = np.ascontiguousarray(a, np.float32)
    d = (np.asarray(b, np.float32) - a).astype(np.float32)
    n = len(a)
    t_lo, t_hi = np.zeros(n, np.float32), np.ones(n, np.float32)
    done = np.zeros(n, bool)
    for _ in range(rounds):
        act = np.flatnonzero(~done)
        if len(act) == 0:
            break
        lo, hi = t_lo[act], t_hi[act]
        mid = ((lo + hi) * np.float32(0.5)).astype(np.float32)
        q_mid, q_lo, q_hi = _at(a[act], d[act], mid), _at(a[act], d[act], lo), _at(a[act], d[act], hi)
        stop = (mid <= lo) | (mid >= hi) | np.all(q_mid == q_lo, axis=1) | np.all(q_mid == q_hi, axis=1)
        done[act[stop]] = True
        act, mid, q_mid = act[~stop], mid[~stop], q_mid[~stop]
        if len(act) == 0:
            continue
        ok = oracle.validate_batch(rid, oenv, q_mid, threads=THREADS)
        t_lo[act[ok]] = mid[ok]
        t_hi[act[~ok]] = mid[~ok]
    assert done.all(), "bisection did not converge"
    return d, t_lo, t_hi


def label_pairs(oracle, name, spec, q_lo, q_hi):
    """-> labels, clearances at q_lo, clearances at q_hi.  A pair is `self` when the robot alone (an empty environment)
    already rejects q_hi; otherwise the kind of the nearest float64 contact at q_hi."""
    rid = oracle.robot(name)
    empty = oracle.env()
    self_hit = ~oracle.validate_batch(rid, empty, q_hi, threads=THREADS)
    cl_lo = geom64.clearances(oracle, name, spec, q_lo)
    cl_hi = geom64.clearances(oracle, name, spec, q_hi)
    kinds = [k for k in cl_hi if k != "self"]
    if kinds:
        nearest = np.array(kinds)[np.argmin(np.stack([cl_hi[k] for k in kinds]), axis=0)]
    else:
        nearest = np.full(len(q_hi), "self")
    return np.where(self_hit, "self", nearest), cl_lo, cl_hi


def _nearest(src, dst):
    """index into dst of each src row's nearest neighbour (joint-space L2)"""
    out = np.empty(len(src), np.int64)
    for s in range(0, len(src), 256):
        dd = ((src[s: s + 256, None, :] - dst[None]) ** 2).sum(axis=2)
        out[s: s + 256] = np.argmin(dd, axis=1)
    return out


def boundary_configs(oracle, name, oenv, n, seed, spec):
    """n valid -> invalid segments from mixed_configs endpoints, bisected to adjacent fp32 steps.  Half of the pairs end
    at the nearest invalid endpoint, half at the nearest endpoint the robot alone finds valid (an environment or
    attachment contact), so that environment kinds are reached on robots whose invalid samples mostly self-collide."""
    rid = oracle.robot(name)
    rng = np.random.default_rng(seed)
    _, q, ok = mixed_configs(oracle, name, oenv, max(4 * n, 800), seed)
    valid, invalid = q[ok], q[~ok]
    env_only = invalid[oracle.validate_batch(rid, oracle.env(), invalid, threads=THREADS)]
    starts = valid[rng.integers(len(valid), size=n)]
    ends = invalid[_nearest(starts, invalid)]
    if len(env_only):
        half = np.arange(n) % 2 == 1
        ends[half] = env_only[_nearest(starts[half], env_only)]
    d, t_lo, t_hi = bisect_segments(oracle, rid, oenv, starts, ends)
    q_lo, q_hi = _at(starts, d, t_lo), _at(starts, d, t_hi)
    label, cl_lo, cl_hi = label_pairs(oracle, name, spec, q_lo, q_hi)
    return BoundaryPairs(q_lo, q_hi, label, cl_lo, cl_hi, starts, d, t_lo, t_hi)


def _bisect_edges(oracle, rid, oenv, a, b, da, db, rounds=200):
    """edges (a + s * da, b + s * db), s in [0, 1] fp32: s = 0 valid, s = 1 invalid (oracle) -> s_lo, s_hi with the
    motion answer flipping between them (adjacent floats, or no edge in between)"""
    k = len(a)
    s_lo, s_hi = np.zeros(k, np.float32), np.ones(k, np.float32)
    done = np.zeros(k, bool)
    for _ in range(rounds):
        act = np.flatnonzero(~done)
        if len(act) == 0:
            break
        lo, hi = s_lo[act], s_hi[act]
        mid = ((lo + hi) * np.float32(0.5)).astype(np.float32)
        ends = [(_at(a[act], da[act], t), _at(b[act], db[act], t)) for t in (mid, lo, hi)]
        same = [np.all(ends[0][0] == e[0], axis=1) & np.all(ends[0][1] == e[1], axis=1) for e in ends[1:]]
        stop = (mid <= lo) | (mid >= hi) | same[0] | same[1]
        done[act[stop]] = True
        act, mid = act[~stop], mid[~stop]
        if len(act) == 0:
            continue
        ok = oracle.validate_motion_batch(rid, oenv, _at(a[act], da[act], mid), _at(b[act], db[act], mid), threads=THREADS)
        s_lo[act[ok]] = mid[ok]
        s_hi[act[~ok]] = mid[~ok]
    assert done.all(), "edge bisection did not converge"
    return s_lo, s_hi


def boundary_edges(oracle, name, oenv, n, seed, pairs=None):
    """-> (a, b, want): edges one fp32 step either side of the oracle's motion answer, of two families:
    - rays: a valid start, the goal on a ray whose length is bisected.  The flip comes from a rake sample touching a
      contact (mostly the goal itself) or from a change of the rake count ceil(distance / 8 * resolution).
    - sweeps: a valid edge of several rakes translated sideways, the translation bisected.  The flip is mostly decided
      by an interior sample of a later rake, i.e. by the iterated `block -= backstep` of the reference.
    Plus the zero-length edges at `pairs`' q_lo and q_hi when given."""
    rid = oracle.robot(name)
    _, span = oracle.bounds(rid)
    rng = np.random.default_rng(seed)
    seeds = valid_seeds(oracle, rid, oenv, rng)
    m = 3 * n
    zero = np.zeros((m, len(span)), np.float32)
    # rays
    a = seeds[rng.integers(len(seeds), size=m)]
    ray = _scaled_noise(rng, a.shape, 1.0, span)
    ray = (ray * rng.choice(np.array([0.1, 0.3, 1.0], np.float32), size=(m, 1))).astype(np.float32)
    keep = np.flatnonzero(~oracle.validate_motion_batch(rid, oenv, a, (a + ray).astype(np.float32), threads=THREADS))[:n]
    ra, rray = a[keep], ray[keep]
    l_lo, l_hi = _bisect_edges(oracle, rid, oenv, ra, ra, zero[keep], rray)
    # sweeps: short valid edges (rakes of 8 samples each, dozens of samples) pushed sideways until they touch
    a = seeds[rng.integers(len(seeds), size=4 * m)]
    b = (a + _scaled_noise(rng, a.shape, 0.5, span)).astype(np.float32)
    w = _scaled_noise(rng, a.shape, 0.3, span)
    keep = oracle.validate_motion_batch(rid, oenv, a, b, threads=THREADS)
    keep &= ~oracle.validate_motion_batch(rid, oenv, (a + w).astype(np.float32), (b + w).astype(np.float32), threads=THREADS)
    keep = np.flatnonzero(keep)[:n]
    sa, sb, sw = a[keep], b[keep], w[keep]
    s_lo, s_hi = _bisect_edges(oracle, rid, oenv, sa, sb, sw, sw)
    ea = [ra, ra, _at(sa, sw, s_lo), _at(sa, sw, s_hi)]
    eb = [_at(ra, rray, l_lo), _at(ra, rray, l_hi), _at(sb, sw, s_lo), _at(sb, sw, s_hi)]
    want = [np.ones(len(ra), bool), np.zeros(len(ra), bool), np.ones(len(sa), bool), np.zeros(len(sa), bool)]
    if pairs is not None:
        ea += [pairs.q_lo, pairs.q_hi]
        eb += [pairs.q_lo, pairs.q_hi]
        want += [np.ones(len(pairs.q_lo), bool), np.zeros(len(pairs.q_hi), bool)]
    perm = rng.permutation(sum(len(x) for x in ea))
    return (np.ascontiguousarray(np.concatenate(ea)[perm]), np.ascontiguousarray(np.concatenate(eb)[perm]),
            np.concatenate(want)[perm])


def sphere_collides(oracle, oenv, c, r):
    c = np.ascontiguousarray(c, np.float32)
    return bool(oracle.L.vo_sphere_environment_in_collision(oenv.h, c.ctypes.data_as(_fp), ctypes.c_float(float(r))))


def boundary_spheres(oracle, oenv, centres, r_max=1.0):
    """For each centre, a binary search over the fp32 bit pattern of r in [0, r_max] for the smallest radius at which
    the oracle says "collides".  -> spheres [m][4] at that radius and [m][4] at nextafter(r, 0) (free), for the centres
    that are free at r = 0 and collide at r_max."""
    hit, free = [], []
    top = int(np.float32(r_max).view(np.uint32))
    for c in np.asarray(centres, np.float32):
        if not np.all(np.isfinite(c)) or sphere_collides(oracle, oenv, c, 0.0) or not sphere_collides(oracle, oenv, c, r_max):
            continue
        lo, hi = 0, top  # bit patterns: lo free, hi collides
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if sphere_collides(oracle, oenv, c, np.uint32(mid).view(np.float32)):
                hi = mid
            else:
                lo = mid
        r = np.uint32(hi).view(np.float32)
        hit.append([*c, r])
        free.append([*c, np.nextafter(r, np.float32(0))])
    return np.array(hit, np.float32).reshape(-1, 4), np.array(free, np.float32).reshape(-1, 4)


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def boundary_centres(spec, seed, per=6):
    """Sphere centres around every primitive of the spec: off the faces, edges and corners of cuboids, off capsule ends
    and sides, off spheres, over heightfield cell borders and beyond the image's clamped border, around cloud points."""
    rng = np.random.default_rng(seed)
    out = []

    def gap(k):
        return rng.uniform(0.003, 0.12, (k, 1))

    for kind, p in spec:
        if kind == "sphere":
            p = np.asarray(p, np.float64)
            out.append(p[:3] + _unit(rng, per) * (p[3] + gap(per)))
        elif kind == "cuboid":
            p = np.asarray(p, np.float64)
            ax, h = p[3:12].reshape(3, 3), p[12:15]
            for _ in range(per):
                sgn = rng.choice([-1.0, 1.0], 3)
                which = rng.integers(3)  # 0: face, 1: edge, 2: corner
                on = np.zeros(3)
                on[rng.permutation(3)[: which + 1]] = 1.0
                pos = p[:3] + ((sgn * h * on) @ ax) + ((sgn * on) @ ax) / np.sqrt(on.sum()) * gap(1)[0]
                if which < 2:  # random point on the face / edge
                    free_axes = np.flatnonzero(on == 0)
                    pos += (rng.uniform(-1, 1, len(free_axes)) * h[free_axes]) @ ax[free_axes]
                out.append(pos[None])
        elif kind == "capsule":
            p = np.asarray(p, np.float64)
            p1, v, r = p[:3], p[3:6], p[6]
            vhat = v / np.linalg.norm(v)
            perp = np.cross(vhat, _unit(rng, per))
            perp /= np.linalg.norm(perp, axis=1, keepdims=True)
            k = per // 3 + 1
            out.append(p1 - vhat * (r + gap(k)))
            out.append(p1 + v + vhat * (r + gap(k)))
            out.append(p1 + rng.uniform(0, 1, (per, 1)) * v + perp * (r + gap(per)))
        elif kind == "heightfield":
            centre, scale, xd, yd, data = p
            centre, scale = np.asarray(centre, np.float64), np.asarray(scale, np.float64)
            img = np.asarray(data, np.float32).reshape(yd, xd)
            k = 6 * per
            ix, iy = rng.integers(-3, xd + 4, k), rng.integers(-3, yd + 4, k)
            # x = centre - (i - xd / 2) * scale is a cell border of the reference's index floor(xs * (cx - x) + xd / 2)
            x = centre[0] - (ix - xd // 2) * scale[0]
            y = centre[1] - (iy - yd // 2) * scale[1] + rng.uniform(0, scale[1], k)
            x[::2] += rng.uniform(0, scale[0], len(x[::2]))  # half the centres inside a cell
            h = img[np.clip(iy, 0, yd - 1), np.clip(ix, 0, xd - 1)] * scale[2] + centre[2]
            out.append(np.stack([x, y, h + rng.uniform(0.005, 0.3, k)], axis=1))
        elif kind in ("capt", "mvt"):
            pts = np.asarray(p[0], np.float64)
            r_point = p[3] if kind == "capt" else p[5]
            sel = pts[rng.integers(len(pts), size=40 * per)]
            out.append(sel + _unit(rng, len(sel)) * (r_point + gap(len(sel))))
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3), np.float32)


def tangency_spec_and_spheres():
    """Exactly representable tangencies: every test value is +0.0, which the reference's sign-bit rule treats as free,
    so each sphere here must be free and the next float of its radius must collide.  -> (spec, spheres [m][4])"""
    spec = [("sphere", np.array([2.0, 0.0, 0.5, 0.5], np.float32)),
            ("cuboid", np.array([0.0, 2.0, 0.5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.25, 0.5, 0.25], np.float32)),
            ("cuboid", np.array([-2.0, 0.0, 0.5, 1, 0, 0, 0, 0, 1, 0, -1, 0, 0.25, 0.25, 0.5], np.float32)),
            ("capsule", np.array([0.0, -2.0, 0.5, 0.0, 0.0, 0.5, 0.25, 4.0], np.float32)),
            ("capsule", np.array([1.0, -2.0, 0.5, 0.5, 0.0, 0.0, 0.25, 4.0], np.float32))]
    s = [[3.0, 0.0, 0.5, 0.5], [2.0, 0.0, 1.5, 0.5],          # sphere: distance 1 = 0.5 + 0.5
         [0.5, 2.0, 0.5, 0.25], [0.0, 2.0, 1.0, 0.25],        # z-aligned cuboid faces (x: 0.25 + 0.25, z: 0.25 + 0.25)
         [0.0, 2.75, 0.5, 0.25],                              # z-aligned cuboid face y: 0.5 + 0.25
         [-2.0, 0.75, 0.5, 0.25], [-2.0, 0.0, 1.0, 0.25],     # oriented cuboid (axes x, z, -y): faces along -y and z
         [-1.5, 0.0, 0.5, 0.25],                              # and along x
         [0.5, -2.0, 0.75, 0.25], [0.0, -2.0, -0.25, 0.5],    # z-aligned capsule: side 0.25 + 0.25, below the end
         [1.25, -1.5, 0.5, 0.25], [2.0, -2.0, 0.5, 0.25]]     # capsule along x: side, beyond the end
    return spec, np.array(s, np.float32)
