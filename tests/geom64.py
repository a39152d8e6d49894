"""Float64 geometric reference: signed clearance between the robot's spheres and every kind of contact.

Test infrastructure.  The sphere centres are the oracle's own fp32 forward kinematics (`fk_all`), attachments are posed
with its fp32 end-effector frame (`eefk`); everything after that is float64 geometry, independent of the reference's
fp32 predicates.  A clearance is the distance between the two surfaces (negative = penetration), except for
heightfields, whose clearance is the reference's own vertical one (`z - r - height`, sphere_heightfield.hh) with the
cell chosen by the reference's fp32 arithmetic.  Point clouds (CAPT, MVT) get the exact distance to the nearest point;
the reference's CAPT has documented false negatives (test_known_answers.py), so callers compare clouds one-sided."""
from __future__ import annotations

import json
import os

import numpy as np

ROBOTS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vamp_mvt_amd", "robots")
ENV_KINDS = ("sphere", "capsule", "z_capsule", "cuboid", "z_cuboid", "heightfield", "capt", "mvt")
CLOUD_KINDS = ("capt", "mvt")
_ROBOT_CACHE: dict = {}


def robot_model(name):
    """-> dict(groups = [(bound, fine indices)] of the environment groups, self_groups = [(bound_a, bound_b, pairs)],
    attach_groups = the environment groups of the links the attachment is checked against)"""
    if name not in _ROBOT_CACHE:
        with open(os.path.join(ROBOTS_DIR, f"{name}.json")) as f:
            d = json.load(f)
        groups = [(g["bound"], np.array(g["fine"], np.int64)) for g in d["env_groups"]]
        self_groups = [(g["bound_a"], g["bound_b"], np.array(g["pairs"], np.int64).reshape(-1, 2)) for g in d["self_groups"]]
        links = set(d.get("attach_links", []))
        attach = [(g["bound"], np.array(g["fine"], np.int64)) for g in d["env_groups"] if g["link"] in links]
        _ROBOT_CACHE[name] = dict(groups=groups, self_groups=self_groups, attach_groups=attach)
    return _ROBOT_CACHE[name]


def _norm(v):
    return np.sqrt(np.sum(v * v, axis=-1))


def sphere_clearance(c, r, prims):
    """c [m][3], r [m] vs spheres [k][4] (x, y, z, r) -> [m][k]"""
    p = np.asarray(prims, np.float64)[:, :4]
    return _norm(c[:, None, :] - p[None, :, :3]) - (r[:, None] + p[None, :, 3])


def capsule_clearance(c, r, prims):
    """capsules [k][8] (x1, y1, z1, xv, yv, zv, r, rdv): distance to the segment x1 .. x1 + v, minus both radii"""
    p = np.asarray(prims, np.float64)
    p1, v, rc = p[:, :3], p[:, 3:6], p[:, 6]
    vv = np.sum(v * v, axis=1)
    d = c[:, None, :] - p1[None]
    t = np.clip(np.sum(d * v[None], axis=2) / np.where(vv > 0, vv, 1.0)[None], 0.0, 1.0)
    closest = p1[None] + t[..., None] * v[None]
    return _norm(c[:, None, :] - closest) - (r[:, None] + rc[None])


def cuboid_clearance(c, r, prims, z_aligned=False):
    """cuboids [k][15] (centre, three unit axes, three half extents): distance to the box (0 inside), minus r.  The
    z-aligned kind is read the way the reference's test reads it: the first two axes in x, y, the third is +z."""
    p = np.asarray(prims, np.float64)
    d = c[:, None, :] - p[None, :, :3]
    if z_aligned:
        a1 = np.abs(d[..., 0] * p[None, :, 3] + d[..., 1] * p[None, :, 4])
        a2 = np.abs(d[..., 0] * p[None, :, 6] + d[..., 1] * p[None, :, 7])
        a3 = np.abs(d[..., 2])
    else:
        a1, a2, a3 = (np.abs(np.sum(d * p[None, :, 3 + 3 * k: 6 + 3 * k], axis=2)) for k in range(3))
    out = np.stack([np.maximum(a - p[None, :, 12 + k], 0.0) for k, a in enumerate((a1, a2, a3))], axis=2)
    return _norm(out) - r[:, None]


def heightfield_clearance(c, r, hf):
    """hf = (centre[3], scale[3], xd, yd, data): the reference's fp32 cell choice (clamped to the image, border cells
    repeated), then z - r - (zs * height + centre_z) in float64, zs the fp32 reciprocal the reference stores."""
    centre, scale, xd, yd, data = hf
    centre = np.asarray(centre, np.float32)
    inv = (np.float32(1.0) / np.asarray(scale, np.float32)).astype(np.float32)
    cf = c.astype(np.float32)
    with np.errstate(all="ignore"):
        xo = (centre[0] - cf[:, 0]).astype(np.float32)
        yo = (centre[1] - cf[:, 1]).astype(np.float32)
        xs = np.floor(np.clip((inv[0] * xo).astype(np.float32) + np.float32(xd // 2), np.float32(0), np.float32(xd)))
        ys = np.floor(np.clip((inv[1] * yo).astype(np.float32) + np.float32(yd // 2), np.float32(0), np.float32(yd)))
        index = ((ys * np.float32(xd)).astype(np.float32) + xs).astype(np.float32)
    idx = np.clip(np.rint(index).astype(np.int64), 0, xd * yd - 1)
    h = np.float64(inv[2]) * np.asarray(data, np.float32).reshape(-1)[idx].astype(np.float64) + np.float64(centre[2])
    return (c[:, 2] - r - h)[:, None]


def heightfield_cells(oracle, name, spec, q):
    """-> [n][spheres] the reference's cell index under every sphere of fk_all (first heightfield of the spec): a
    heightfield clearance is a step function of the centre, so a flip may sit on a cell border instead of at zero"""
    rid = oracle.robot(name)
    hf = env_parts(spec)[0]["heightfield"][0]
    centre, scale, xd, yd, _ = hf
    inv = (np.float32(1.0) / np.asarray(scale, np.float32)).astype(np.float32)
    out = []
    for qi in np.asarray(q, np.float32).reshape(-1, oracle.dimension(rid)):
        c = oracle.fk_all(rid, qi)[:, :3]
        xo = (np.float32(centre[0]) - c[:, 0]).astype(np.float32)
        yo = (np.float32(centre[1]) - c[:, 1]).astype(np.float32)
        xs = np.floor(np.clip((inv[0] * xo).astype(np.float32) + np.float32(xd // 2), np.float32(0), np.float32(xd)))
        ys = np.floor(np.clip((inv[1] * yo).astype(np.float32) + np.float32(yd // 2), np.float32(0), np.float32(yd)))
        out.append(ys * xd + xs)
    return np.array(out)


def cloud_clearance(c, r, points, r_point):
    """distance to the nearest cloud point minus (r + r_point) -> [m][1]"""
    p = np.asarray(points, np.float64)
    best = np.full(len(c), np.inf)
    for s in range(0, len(p), 512):
        d = c[:, None, :] - p[None, s: s + 512]
        best = np.minimum(best, np.sum(d * d, axis=2).min(axis=1))
    return (np.sqrt(best) - (r + r_point))[:, None]


def env_parts(spec):
    """spec (envs.spec_for) -> {kind: list of primitives} with the reference's list assignment (z-aligned iff
    axis_3_z == 1 / xv == yv == 0), plus the attachment (tf, spheres) or None"""
    parts = {k: [] for k in ENV_KINDS}
    attach = None
    for kind, p in spec:
        if kind == "sphere":
            parts["sphere"].append(np.asarray(p, np.float32))
        elif kind == "capsule":
            p = np.asarray(p, np.float32)
            parts["z_capsule" if p[3] == 0 and p[4] == 0 else "capsule"].append(p)
        elif kind == "cuboid":
            p = np.asarray(p, np.float32)
            parts["z_cuboid" if p[11] == 1.0 else "cuboid"].append(p)
        elif kind == "heightfield":
            parts["heightfield"].append(p)
        elif kind == "capt":
            parts["capt"].append((p[0], p[3]))
        elif kind == "mvt":
            parts["mvt"].append((p[0], p[5]))
        elif kind == "attach":
            attach = p
    return parts, attach


def env_clearance(parts, c, r):
    """-> {kind: [m] smallest clearance of the m spheres to any contact of that kind} for the kinds present"""
    c = np.asarray(c, np.float64)
    r = np.asarray(r, np.float64)
    out = {}
    for kind, prims in parts.items():
        if not prims:
            continue
        if kind == "sphere":
            v = sphere_clearance(c, r, prims)
        elif kind in ("capsule", "z_capsule"):
            v = capsule_clearance(c, r, prims)
        elif kind in ("cuboid", "z_cuboid"):
            v = cuboid_clearance(c, r, prims, kind == "z_cuboid")
        elif kind == "heightfield":
            v = np.concatenate([heightfield_clearance(c, r, h) for h in prims], axis=1)
        else:
            v = np.concatenate([cloud_clearance(c, r, pts, rp) for pts, rp in prims], axis=1)
        out[kind] = v.min(axis=1)
    return out


def attachment_spheres(oracle, rid, q, attach):
    """the attached spheres posed at configuration q: eefk (fp32, the oracle's) * tf * sphere in float64 -> [k][4]"""
    tf, sp = attach
    ee = oracle.eefk(rid, q).astype(np.float64)
    tf = np.asarray(tf, np.float32).astype(np.float64).reshape(4, 4)
    sp = np.asarray(sp, np.float32).astype(np.float64).reshape(-1, 4)
    m = ee @ tf
    return np.concatenate([sp[:, :3] @ m[:3, :3].T + m[:3, 3], sp[:, 3:4]], axis=1)


def clearances(oracle, name, spec, q):
    """-> {kind: [n] clearance} for each configuration of q[n][dim]: every environment kind present, `self` (the fine
    self pairs of robots/<robot>.json), and `attachment` (attached spheres vs. the environment and vs. the links of the
    attachment groups) when the spec holds one.  The reference tests a group's fine spheres only when its bounding
    sphere collides, so a group's clearance is the larger of its bounding sphere's and its fine spheres' (the two differ
    for heightfields, whose vertical test reads the cell under each centre)."""
    rid = oracle.robot(name)
    model = robot_model(name)
    parts, attach = env_parts(spec)
    q = np.asarray(q, np.float32).reshape(-1, oracle.dimension(rid))
    out = {}

    def put(kind, i, v):
        out.setdefault(kind, np.full(len(q), np.inf))[i] = min(out[kind][i], v) if kind in out else v

    for i, qi in enumerate(q):
        s = oracle.fk_all(rid, qi).astype(np.float64)
        for bound, fine in model["groups"]:
            b = min(env_clearance(parts, s[bound: bound + 1, :3], s[bound: bound + 1, 3]).values(), default=np.inf)
            for kind, v in env_clearance(parts, s[fine, :3], s[fine, 3]).items():
                put(kind, i, max(float(np.min(b)), float(np.min(v))))
        self_c = np.inf
        for ba, bb, pairs in model["self_groups"]:
            gate = float(sphere_clearance(s[ba: ba + 1, :3], s[ba: ba + 1, 3], s[bb: bb + 1])[0, 0])
            pa, pb = s[pairs[:, 0]], s[pairs[:, 1]]
            fine = float(np.min(_norm(pa[:, :3] - pb[:, :3]) - (pa[:, 3] + pb[:, 3])))
            self_c = min(self_c, max(gate, fine))
        put("self", i, self_c)
        if attach is not None:
            a = attachment_spheres(oracle, rid, qi, attach)
            vals = [float(np.min(v)) for v in env_clearance(parts, a[:, :3], a[:, 3]).values()]
            for bound, fine in model["attach_groups"]:
                gate = float(np.min(sphere_clearance(s[bound: bound + 1, :3], s[bound: bound + 1, 3], a)))
                vals.append(max(gate, float(np.min(sphere_clearance(a[:, :3], a[:, 3], s[fine])))))
            put("attachment", i, min(vals))
    return out


def min_clearance(cl):
    """the smallest clearance of every configuration over all kinds"""
    return np.min(np.stack(list(cl.values())), axis=0)
