"""float64 statement of the end-effector constraints (include/vamp_mvt_amd.h: vmv_ee_constraint, vmv_constraint_*_batch;
csrc/vmv_constraint.h states them in full) on the generator's own tapes, through tests/ik_serial.py.  Not
bit-exact to the device, which works in fp32: it serves to state the conditions the device tests rest on and to judge the
device's answers.  The set-up is the library's: float64 arithmetic, every value of the record rounded once to fp32.  Lanes
are vectorised with numpy; every lane is independent."""
from dataclasses import dataclass, field

import numpy as np

import ik_serial as K

MAX_SAMPLES = 1024  # kConstraintMaxSamples


@dataclass
class Settings:
    """vmv_constraint_settings with its defaults"""
    max_iterations: int = 16
    pos_tol: float = 1e-4
    rot_tol: float = 1e-3
    rot_weight: float = 0.25
    damping: float = 1e-2
    max_step: float = 0.5
    check_step: float = 0.05


@dataclass
class Constraint:
    """vmv_ee_constraint"""
    frame: np.ndarray = field(default_factory=lambda: np.eye(4))
    pos_lo: tuple = (-np.inf, -np.inf, -np.inf)
    pos_hi: tuple = (np.inf, np.inf, np.inf)
    tool_axis: tuple = (0.0, 0.0, 1.0)
    ref_axis: tuple = (0.0, 0.0, 1.0)
    max_angle: float = 0.0


def upright(tool_axis, max_angle, frame=None):
    return Constraint(frame=np.eye(4) if frame is None else np.asarray(frame, np.float64), tool_axis=tuple(tool_axis), max_angle=max_angle)


def box(lo, hi, frame=None):
    return Constraint(frame=np.eye(4) if frame is None else np.asarray(frame, np.float64), pos_lo=tuple(lo), pos_hi=tuple(hi))


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def record(c, s):
    """constraint_setup (csrc/vmv_constraint.h): the device record of one constraint, its fp32 values held in float64"""
    F = _f32(np.asarray(c.frame).reshape(4, 4))
    lo, hi = _f32(c.pos_lo), _f32(c.pos_hi)
    m = float(np.float32(c.max_angle))
    axis = m > 0.0
    u, d = np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0])
    if axis:
        u = _f32(c.tool_axis) / np.linalg.norm(_f32(c.tool_axis))
        d = F[:3, :3] @ _f32(c.ref_axis) / np.linalg.norm(_f32(c.ref_axis))
        d = d / np.linalg.norm(d)
    return dict(t=F[:3, 3], R=F[:3, :3], lo=lo, hi=hi, lo_band=_f32(lo - s.pos_tol), hi_band=_f32(hi + s.pos_tol), u=_f32(u), d=_f32(d),
                cos_m=_f32(np.cos(m)), sin_m=_f32(np.sin(m)), cos_band=_f32(np.cos(m + s.rot_tol)) if axis else np.float64(-2.0),
                axis=np.bool_(axis))


def records(constraints, n, s):
    """one Constraint (shared) or n of them -> dict of arrays with a leading lane axis"""
    items = [constraints] if isinstance(constraints, Constraint) else list(constraints)
    assert len(items) in (1, n)
    recs = [record(c, s) for c in items] or [record(Constraint(), s)]  # (an empty batch still has the fields)
    idx = np.zeros(n, np.int64) if len(recs) == 1 else np.arange(n)
    return {k: np.stack([r[k] for r in recs])[idx] for k in recs[0]}


def residual(t, R, C, slack=0.0):
    """the residual and the band test of frames (t [n][3], R [n][3][3]) against the records C; slack widens the band test
    (metres for the box, a difference of cosines for the cone)"""
    p = np.einsum("nrk,nr->nk", C["R"], t - C["t"])
    v = p - np.clip(p, C["lo"], C["hi"])
    a = np.einsum("nrk,nk->nr", R, C["u"])
    c = np.cross(a, C["d"])
    sn, cs = np.linalg.norm(c, axis=1), np.einsum("nr,nr->n", a, C["d"])
    n = c / np.where(sn > 0.0, sn, 1.0)[:, None]
    far = cs * C["cos_m"] + sn * C["sin_m"]
    near = sn * C["cos_m"] - cs * C["sin_m"]
    s = np.where(far <= 0.0, 1.0, near)
    axis = C["axis"].astype(bool)
    tilted = axis & (cs < C["cos_m"])
    anti = axis & (sn == 0.0) & (cs < 0.0)
    inside = ((p >= C["lo_band"] - slack) & (p <= C["hi_band"] + slack)).all(axis=1)
    band = inside & (~axis | (cs >= C["cos_band"] - slack))
    res = np.stack([np.linalg.norm(v, axis=1), np.where(tilted, np.arctan2(near, far), 0.0)], axis=1)
    return dict(p=p, v=v, a=a, n=n, s=s, sn=sn, cs=cs, tilted=tilted, anti=anti, band=band, res=res)


def in_band(robot, q, constraints, s=None, slack=0.0):
    """the band test of configurations q [n][dim] in float64 -> (bool[n], the residual dict)"""
    s = s or Settings()
    q = np.asarray(q, np.float64)
    C = records(constraints, len(q), s)
    finite = np.isfinite(q).all(axis=1)
    t, R, _ = K.frame_jac(robot, np.where(finite[:, None], q, 0.0))
    r = residual(t, R, C, slack)
    return r["band"] & finite, r


def band_margin(robot, q, constraints, s=None):
    """per configuration the distance to the nearest face of the band: min over the box faces of |p - face| (metres) and
    |cos - cos_band| for the cone; inf where a part is free"""
    s = s or Settings()
    ok, r = in_band(robot, q, constraints, s)
    C = records(constraints, len(r["p"]), s)
    box_m = np.minimum(np.abs(r["p"] - C["lo_band"]), np.abs(r["p"] - C["hi_band"])).min(axis=1)
    cone_m = np.where(C["axis"].astype(bool), np.abs(r["cs"] - C["cos_band"]), np.inf)
    return np.minimum(box_m, cone_m)


def ee_mask(robot):
    """bool[dim]: the joints that move the end effector (kEeJointMask)"""
    g, m = K.gen_hip(), K.model(robot)
    mask = g.ee_joint_mask(m, g.ee_tangent_tape(m))
    return np.array([bool(mask >> j & 1) for j in range(m["dimension"])])


def project(robot, q_in, constraints, s=None):
    """vmv_constraint_project_batch in float64: q_in [n][dim] -> dict(q, res [n][2], converged, evaluations, nonfinite)"""
    s = s or Settings()
    q_in = np.asarray(q_in, np.float64)
    n, dim = q_in.shape
    C = records(constraints, n, s)
    lo, hi = K.bounds(robot)
    finite = np.isfinite(q_in).all(axis=1)
    q = np.clip(np.where(finite[:, None], q_in, 0.0), lo, hi)
    moves = ee_mask(robot)

    def evaluate(x):
        t, R, J = K.frame_jac(robot, x)
        r = residual(t, R, C)
        e = np.zeros((n, 6))
        e[:, :3] = -r["v"]
        e[:, 3] = np.where(r["tilted"], s.rot_weight * r["s"], 0.0)
        Jw = np.zeros((n, 6, dim))
        Jw[:, :3] = np.einsum("nrk,nrj->nkj", C["R"], J[:, :3]) * (r["v"] != 0.0)[:, :, None]
        b = np.cross(r["a"], r["n"])
        Jw[:, 3] = s.rot_weight * np.einsum("nr,nrj->nj", r["n"], J[:, 3:]) * r["tilted"][:, None]
        Jw[:, 4] = s.rot_weight * np.einsum("nr,nrj->nj", b, J[:, 3:]) * r["tilted"][:, None]
        Jw[:, :, ~moves] = 0.0
        return Jw, e, 0.5 * (e ** 2).sum(axis=1), r

    Jw, e, E, r = evaluate(q)
    stuck = r["anti"] & finite
    converged = r["band"] & finite & ~stuck
    done = converged | stuck | ~finite
    res = r["res"].copy()
    lam = np.full(n, float(s.damping))
    evals = np.zeros(n, np.int64)
    for _ in range(s.max_iterations):
        if done.all():
            break
        cand = np.where(moves[None, :], K.step(q, Jw, e, lam, lo, hi, s.max_step), q)
        Jc, ec, Ec, rc = evaluate(cand)
        live = ~done
        acc = live & (Ec < E)
        evals += live
        lam = K.damped(lam, live, acc)
        q[acc], Jw[acc], e[acc], E[acc], res[acc] = cand[acc], Jc[acc], ec[acc], Ec[acc], rc["res"][acc]
        converged = converged | (acc & rc["band"])
        done = done | (acc & rc["band"])
    given = stuck | ~finite
    q = np.where(given[:, None], q_in, q)
    res[~finite] = np.nan
    return dict(q=q, res=res, converged=converged, evaluations=evals, nonfinite=~finite)


def edge_samples32(a, b, check_step=0.05):
    """the band samples of the edge a -> b as the device forms them, all in fp32: -> float32 [n_c][dim], or None for an
    edge of more than MAX_SAMPLES samples or of non-finite length"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = (b - a).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.float32(0.0)
        for j, x in enumerate(d):
            sq = np.float32(x * x) if j == 0 else np.float32(sq + np.float32(x * x))
        count = max(np.float32(1.0), np.ceil(np.float32(np.sqrt(sq)) / np.float32(check_step)))
    if not np.isfinite(sq) or not count <= np.float32(MAX_SAMPLES):  # (the device's samples of a NaN length are NaN: out of band)
        return None
    n_c = int(count)
    t = (np.arange(1, n_c + 1, dtype=np.float32) / np.float32(n_c)).astype(np.float32)
    return (a[None, :] + (d[None, :] * t[:, None]).astype(np.float32)).astype(np.float32)


# ---- the inputs the tests share ------------------------------------------------------------------------------------------
ROBOTS = K.ROBOTS
N = 130  # two full waves and a 2-lane tail
SKIP = 20000  # Halton configurations SKIP + 1 .. + N: clear of the inverse-kinematics tests' targets and seeds


def configs(robot, n=N):
    return K.halton32(robot, n, SKIP)


def rotated_frame(origin):
    """a frame C turned 0.4 rad about (1, 2, 2) / 3 at `origin`, exactly representable in fp32 after the cast"""
    k = np.array([1.0, 2.0, 2.0]) / 3.0
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.4) * Kx + (1 - np.cos(0.4)) * (Kx @ Kx)
    F = np.eye(4)
    F[:3, :3], F[:3, 3] = R, origin
    return F.astype(np.float32).astype(np.float64)


def zero_pose(robot):
    """the end-effector frame of the robot's zero configuration clipped to its bounds (float64)"""
    lo, hi = K.bounds(robot)
    q0 = np.clip(np.zeros((1, len(lo))), lo, hi)
    t, R, _ = K.frame_jac(robot, q0)
    return t[0], R[0]


def cases(robot):
    """the three constraints of the device tests: upright(z, 0.1); a plane at the height of the zero pose's end effector;
    a 20 cm box with a 0.3 rad cone in a rotated frame C at the zero pose's end effector"""
    t0, R0 = zero_pose(robot)
    z = float(np.float32(t0[2]))
    C = rotated_frame(t0)
    ref = C[:3, :3].T @ (R0 @ np.array([0.0, 0.0, 1.0]))  # the zero pose's own tool axis, in C: the cone is reachable
    return {"upright": upright((0.0, 0.0, 1.0), 0.1),
            "plane": Constraint(pos_lo=(-np.inf, -np.inf, z), pos_hi=(np.inf, np.inf, z)),
            "box_cone": Constraint(frame=C, pos_lo=(-0.1, -0.1, -0.1), pos_hi=(0.1, 0.1, 0.1), tool_axis=(0.0, 0.0, 1.0),
                                   ref_axis=tuple(float(x) for x in ref), max_angle=0.3)}
