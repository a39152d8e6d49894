"""Shared by the optimize_multi tests and tools/optimize_defaults_study.py: a float64 clearance-and-gradient callback for
tests/optimize_serial.py built from the generator's tangent tape and tests/geom64.py (no device), and the grazing case of
DESIGN §5l."""
import numpy as np

import clearance_grad_ref as ref
import geom64
from oracle_lib import CAGE_START

GRAZE_GOAL = [1.2, 0.3, 0.0, -1.5, 0.0, 2.0, 0.785]
GRAZE_CENTRE = (0.45, 0.25, 0.75)
GRAZE_CLEARANCE = 0.005


def straight(a, b, n, dtype=np.float32):
    """n waypoints on the line a -> b (float64 arithmetic, cast), the ends copied"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    X = (a64 + (b64 - a64) * np.linspace(0.0, 1.0, n)[:, None]).astype(dtype)
    X[0], X[-1] = np.asarray(a, dtype), np.asarray(b, dtype)
    return X


def graze_line(n=33, dtype=np.float32):
    return straight(CAGE_START, GRAZE_GOAL, n, dtype)


def graze_radius(min_env_at):
    """the radius of the sphere at GRAZE_CENTRE that leaves GRAZE_CLEARANCE to the waypoints; min_env_at(radius) -> the
    smallest env clearance over them (a sphere's clearance is linear in its radius)"""
    r0 = 0.1
    return r0 + float(min_env_at(r0)) - GRAZE_CLEARANCE


class Clearance64:
    """X [N][dim] -> (values [N][2], grads [N][2][dim]) in float64: the flat minima of vmv_clearance_batch's definition and
    the gradients of their witnesses held fixed (the self pair's analytically, the contact's spatial normal by central
    differences of its float64 distance, a heightfield's cell held fixed: normal +z), through the tape's Jacobians"""

    def __init__(self, robot, spec):
        self.m = ref.model(robot)
        self.gh = ref.gen_hip()
        self.tt = self.gh.tangent_tape(self.m)
        self.ns = self.m["n_spheres"]
        self.radii = np.asarray(self.m["radii"][:self.ns], np.float64)
        self.parts = geom64.env_parts(list(spec))[0]
        self.pairs = np.array([p for sg in self.m["self_groups"] for p in sg["pairs"]], np.int64).reshape(-1, 2)

    def __call__(self, X):
        X = np.asarray(X, np.float64)
        N, dim, ns = len(X), X.shape[1], self.ns
        c, J = self.gh.eval_tangent_tape(self.m, X, self.tt)
        values, grads = np.full((N, 2), np.inf), np.zeros((N, 2, dim))
        flat_c, flat_r = c.reshape(-1, 3), np.tile(self.radii, N)
        cols, vals = [], []
        for kind, name in enumerate(ref.KIND_NAMES):
            if self.parts[name]:
                rows = np.stack([np.asarray(p, np.float64) for p in self.parts[name]])
                cols += [(kind, row, None) for row in rows]
                vals.append(geom64.sphere_clearance(flat_c, flat_r, rows) if kind == 0 else
                            geom64.capsule_clearance(flat_c, flat_r, rows) if kind in (1, 2) else
                            geom64.cuboid_clearance(flat_c, flat_r, rows, kind == 4))
        for hf in self.parts["heightfield"]:
            cols.append((5, None, hf))
            vals.append(geom64.heightfield_clearance(flat_c, flat_r, hf))
        if cols:
            v = np.concatenate(vals, axis=1).reshape(N, ns, len(cols))
            h = 1e-6
            probe = np.concatenate([np.eye(3), -np.eye(3)]) * h
            for i in range(N):
                s, k = np.unravel_index(np.argmin(v[i]), v[i].shape)
                kind, prim, _ = cols[k]
                values[i, 0] = v[i, s, k]
                if kind == 5:
                    normal = np.array([0.0, 0.0, 1.0])
                else:
                    d = ref.contact_distance(kind, prim, c[i, s][None, :] + probe, self.radii[s])
                    normal = (d[:3] - d[3:]) / (2 * h)
                grads[i, 0] = normal @ J[i, s]
        if len(self.pairs):
            a, b = self.pairs[:, 0], self.pairs[:, 1]
            dd = c[:, a] - c[:, b]
            L = np.sqrt((dd * dd).sum(-1))
            sv = L - (self.radii[a] + self.radii[b])[None, :]
            kp = sv.argmin(1)
            rows = np.arange(N)
            values[:, 1] = sv[rows, kp]
            nn = dd[rows, kp] / np.maximum(L[rows, kp], 1e-300)[:, None]
            grads[:, 1] = np.einsum("nk,nkj->nj", nn, J[rows, a[kp]] - J[rows, b[kp]])
        return values, grads
