"""float64 side of the clearance-gradient tests: the distance of ONE fixed witness - a fine sphere against one contact, or a
self pair - as a function of the configuration, from the generator's float64 tape (tools/gen_hip.py: eval_tape) and the
distance forms of tests/geom64.py, and its difference quotients.  Shared by tests/test_clearance_grad.py (no device: the
witness is the float64 minimiser) and tests/test_clearance_grad_gpu.py (the witness is the device's)."""
import functools

import numpy as np

import geom64
import self_gates

H = 1e-6  # step of the difference quotients (radians; metres for a prismatic joint)
# Bound on |device gradient - float64 central difference|, per radian (per metre for a prismatic joint), and the kink
# rule's threshold.  Measured once on an MI355X over every case of tests/test_clearance_grad_gpu.py (four robots x the
# `six` and `many` scenes at 257 configurations, the Panda against each kind alone): at most 1.18e-4 for `env` (Fetch in
# `many`, a witness centre 9 mm from the obstacle sphere's centre: the fp32 centre's ~1e-6 m over |c - p| is the
# normal's error; the next configurations are at 3e-5) and 2.6e-5 for `self` (Baxter), no case left out at a kink.  The
# bound is about four times the largest figure - far inside the hundredfold the value bound of the clearance tests gave
# itself - and below the 1e-3 at which a wrong joint, sign or normal on centimetre lever arms (1e-2 or more) would still
# stand out; that cap is a condition, not a measurement.
GRAD_BOUND = 5e-4
KINK_CAP = 0.01  # at most this share of a (robot, scene)'s cases may be left out as kinks
KIND_NAMES = ("sphere", "capsule", "z_capsule", "cuboid", "z_cuboid")  # geom64.env_parts' names of witness kinds 0..4
_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53)


@functools.lru_cache(maxsize=None)
def gen_hip():
    return self_gates.gen_hip()


@functools.lru_cache(maxsize=None)
def model(robot):
    return self_gates.model(robot)


def halton_q(m, n, skip=0):
    """n Halton configurations strictly inside the model's joint bounds, float64"""
    out = np.zeros((n, m["dimension"]))
    for i in range(n):
        for j in range(m["dimension"]):
            k, b, f, v = skip + i + 1, _PRIMES[j], 1.0, 0.0
            while k:
                f /= b
                v += f * (k % b)
                k //= b
            out[i, j] = v
    return np.asarray(m["lower"]) + np.asarray(m["span"]) * out


def stencil(q):
    """q [n][dim] -> [n][1 + 2 * dim][dim]: q itself, then q + H e_j and q - H e_j for every joint j"""
    n, dim = q.shape
    out = np.repeat(q[:, None, :], 1 + 2 * dim, axis=1)
    for j in range(dim):
        out[:, 1 + 2 * j, j] += H
        out[:, 2 + 2 * j, j] -= H
    return out


def quotients(f):
    """f [n][1 + 2 * dim] on the stencil -> (central, forward, backward) difference quotients [n][dim]"""
    f0, fp, fm = f[:, :1], f[:, 1::2], f[:, 2::2]
    return (fp - fm) / (2 * H), (fp - f0) / H, (f0 - fm) / H


def centres_on_stencil(robot, q):
    """float64 centres of the fine spheres on the stencil: [n][1 + 2 * dim][spheres][3]"""
    m = model(robot)
    s = stencil(np.asarray(q, np.float64))
    c = gen_hip().eval_tape(m, s.reshape(-1, s.shape[-1]))[:, :m["n_spheres"]]
    return c.reshape(s.shape[0], s.shape[1], m["n_spheres"], 3)


def contact_distance(kind, prim, c, r, height=None):
    """float64 clearance of centres c [k][3] with radius r against ONE contact: kind 0..4 with its row `prim` of the
    kind's table, or kind 5 with the fixed `height` of the heightfield cell -> [k]"""
    rr = np.full(len(c), float(r))
    one = np.asarray(prim, np.float64)[None, :] if kind < 5 else None
    if kind == 0:
        return geom64.sphere_clearance(c, rr, one)[:, 0]
    if kind in (1, 2):
        return geom64.capsule_clearance(c, rr, one)[:, 0]
    if kind in (3, 4):
        return geom64.cuboid_clearance(c, rr, one, kind == 4)[:, 0]
    return c[:, 2] - rr - height


def pair_distance(ca, cb, ra, rb):
    return geom64._norm(ca - cb) - (ra + rb)


def float64_witness(robot, spec, q):
    """The float64 flat minimiser for configurations q [n][dim]: -> list of dict(sphere, kind, prim, height) (None without
    contacts) and int [n] self pair index.  Contacts are geom64.env_parts(spec)'s; a heightfield's cell is the one its
    fp32 rule picks at q."""
    m = model(robot)
    ns = m["n_spheres"]
    radii = np.asarray(m["radii"][:ns], np.float64)
    c = gen_hip().eval_tape(m, np.asarray(q, np.float64))[:, :ns]
    parts = geom64.env_parts(list(spec))[0]
    pairs = np.array([p for sg in m["self_groups"] for p in sg["pairs"]], np.int64).reshape(-1, 2)
    n = len(q)
    flat_c, flat_r = c.reshape(-1, 3), np.tile(radii, n)
    cols, vals = [], []  # per contact (kind, row), and the value matrices [n * spheres][contacts of the kind]
    for kind, name in enumerate(KIND_NAMES):
        if parts[name]:
            rows = np.stack([np.asarray(p, np.float64) for p in parts[name]])
            cols += [(kind, row) for row in rows]
            vals.append(geom64.sphere_clearance(flat_c, flat_r, rows) if kind == 0 else
                        geom64.capsule_clearance(flat_c, flat_r, rows) if kind in (1, 2) else
                        geom64.cuboid_clearance(flat_c, flat_r, rows, kind == 4))
    for hf in parts["heightfield"]:
        cols.append((5, None))
        vals.append(geom64.heightfield_clearance(flat_c, flat_r, hf))
    env_w = [None] * n
    if cols:
        v = np.concatenate(vals, axis=1).reshape(n, ns, len(cols))
        for i in range(n):
            s, k = np.unravel_index(np.argmin(v[i]), v[i].shape)
            kind, prim = cols[k]
            # (a heightfield: the height of the cell under the sphere at q, held fixed from here on)
            env_w[i] = dict(sphere=int(s), kind=kind, prim=prim, height=None if kind < 5 else float(c[i, s, 2] - radii[s] - v[i, s, k]))
    if len(pairs):
        d = pair_distance(c[:, pairs[:, 0]], c[:, pairs[:, 1]], radii[pairs[:, 0]], radii[pairs[:, 1]])
        self_w = d.argmin(axis=1)
    else:
        self_w = np.full(n, -1)
    return env_w, self_w, pairs


def witness_quotients(robot, q, env_w, self_w, pairs):
    """difference quotients of the fixed witnesses' float64 distances: -> (env, self), each (central, forward, backward)
    [n][dim]; a configuration without a witness has zeros"""
    m = model(robot)
    radii = np.asarray(m["radii"][:m["n_spheres"]], np.float64)
    c = centres_on_stencil(robot, q)
    n, k = c.shape[:2]
    fe, fs = np.zeros((n, k)), np.zeros((n, k))
    for i in range(n):
        w = env_w[i]
        if w is not None:
            fe[i] = contact_distance(w["kind"], w["prim"], c[i, :, w["sphere"]], radii[w["sphere"]], w["height"])
        if self_w[i] >= 0:
            a, b = pairs[self_w[i]]
            fs[i] = pair_distance(c[i, :, a], c[i, :, b], radii[a], radii[b])
    return quotients(fe), quotients(fs)


def kinks(quot, bound=None):
    """bool [n][dim]: the fixed witness's own distance has a kink within H of q - its forward and backward difference
    quotients disagree by more than the bound (a capsule's end clamp; a cuboid's face, edge or corner change)"""
    _, fwd, bwd = quot
    return np.abs(fwd - bwd) > (GRAD_BOUND if bound is None else bound)
