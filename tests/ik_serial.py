"""float64 statement of vmv_ik_batch's iteration (include/vamp_mvt_amd.h) on the generator's own tapes
(tools/gen_hip.py: ee_model, eval_tape, eval_tangent_tape).  Not bit-exact to the device, which works in fp32: it serves to
choose inputs, to state the conditions the device tests rest on, and to measure residuals of the device's answers.  Lanes
are vectorised with numpy; every lane is independent."""
import functools
from dataclasses import dataclass

import numpy as np

import self_gates

# vmv_ik_batch's fixed constants (csrc/vmv_robot_tu.inc: kIkLambdaFactor, kIkLambdaFloor, kIkLambdaCeil)
LAMBDA_FACTOR, LAMBDA_FLOOR, LAMBDA_CEIL = 4.0, 1e-5, 1e6
_PRIMES = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59)  # vmv_halton_configs' bases


@dataclass
class Settings:
    """vmv_ik_settings with the defaults of vamp_mvt_amd.IKSettings"""
    n_seeds: int = 32
    max_iterations: int = 64
    pos_tol: float = 1e-4
    rot_tol: float = 1e-3
    rot_weight: float = 0.25
    damping: float = 1e-2
    max_step: float = 0.5
    position_only: bool = False


@functools.lru_cache(maxsize=None)
def gen_hip():
    return self_gates.gen_hip()


@functools.lru_cache(maxsize=None)
def model(robot):
    return self_gates.model(robot)


@functools.lru_cache(maxsize=None)
def ee(robot):
    """-> (ee model, its tangent tape)"""
    em = gen_hip().ee_model(model(robot))
    return em, gen_hip().tangent_tape(em)


def halton32(robot, n, skip=0):
    """Samples skip + 1 .. skip + n of vmv_halton_configs, float32 [n][dim], by its own arithmetic (vmv_common.h:
    halton_element): u = float(reversed digits) / float(b^digits), then u * span + lower, one fp32 rounding each."""
    m = model(robot)
    out = np.zeros((n, m["dimension"]), np.float32)
    for i in range(n):
        for j in range(m["dimension"]):
            k, b, num, den = skip + i + 1, _PRIMES[j], 0, 1
            while k:
                num, den, k = num * b + k % b, den * b, k // b
            u = np.float32(num) / np.float32(den)
            out[i, j] = np.float32(u * np.float32(m["span"][j])) + np.float32(m["lower"][j])
    return out


def bounds(robot):
    """[lower, lower + span] as the device holds them: fp32, the sum rounded once"""
    m = model(robot)
    lo = np.asarray(m["lower"], np.float32)
    return lo.astype(np.float64), (lo + np.asarray(m["span"], np.float32)).astype(np.float64)


def frame_jac(robot, q):
    """float64 end-effector frame and Jacobian of q [n][dim]: -> (t [n][3], R [n][3][3], J [n][6][dim]); rows 0-2 of J are
    dt/dq_j, rows 3-5 the world-frame angular velocity, omega = vee((dR/dq_j) R^T)"""
    em, tt = ee(robot)
    f, df = gen_hip().eval_tangent_tape(em, np.asarray(q, np.float64), tt)  # [n][4][3], [n][4][3][dim]
    t, R = f[:, 0], np.swapaxes(f[:, 1:], 1, 2)  # f[:, 1 + k] is column k
    dR = np.moveaxis(df[:, 1:], 1, 2)  # [n][row][column][dim]
    A = np.einsum("nakj,nbk->nabj", dR, R)
    w = 0.5 * np.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], axis=1)
    return t, R, np.concatenate([df[:, 0], w], axis=1)


def frames44(robot, q):
    """float64 [n][4][4] frames as vmv_eefk_batch lays them out"""
    t, R, _ = frame_jac(robot, q)
    out = np.zeros((len(t), 4, 4))
    out[:, :3, :3], out[:, :3, 3], out[:, 3, 3] = R, t, 1.0
    return out


def errors(t, R, target):
    """-> (e_p [n][3], e_w [n][3] unrescaled, tr(R*^T R) [n]) against target [n][4][4]"""
    Rs, ts = target[:, :3, :3], target[:, :3, 3]
    e_w = 0.5 * np.cross(np.swapaxes(R, 1, 2), np.swapaxes(Rs, 1, 2)).sum(axis=1)  # over the three columns
    return ts - t, e_w, np.einsum("nij,nij->n", Rs, R)


def residuals(robot, q, target):
    """-> (|e_p| [n], |e_w| [n] unrescaled, tr(R*^T R) [n]) of configurations q against target [n][4][4]"""
    t, R, _ = frame_jac(robot, q)
    e_p, e_w, tr = errors(t, R, np.asarray(target, np.float64).reshape(-1, 4, 4))
    return np.linalg.norm(e_p, axis=1), np.linalg.norm(e_w, axis=1), tr


def weighted(e_p, e_w, tr, s):
    """the weighted error e [n][6] of the iteration: e_w rescaled to unit length where tr <= 1, times rot_weight"""
    n_w = np.linalg.norm(e_w, axis=1)
    far = (tr <= 1.0) & (n_w > 0.0)
    scale = np.where(far, 1.0 / np.where(far, n_w, 1.0), 1.0)
    w = 0.0 if s.position_only else s.rot_weight
    return np.concatenate([e_p, w * scale[:, None] * e_w], axis=1)


def energy(robot, q, target, s):
    t, R, _ = frame_jac(robot, q)
    e_p, e_w, tr = errors(t, R, np.asarray(target, np.float64).reshape(-1, 4, 4))
    return 0.5 * (weighted(e_p, e_w, tr, s) ** 2).sum(axis=1)


def step(q, Jw, e, lam, lo, hi, max_step, hold=True):
    """lm_step (csrc/vmv_robot_tu.inc): the candidates clip(q + delta), delta = Jm^T (Jm Jm^T + lam I)^-1 e capped at max_step"""
    g = np.einsum("nij,ni->nj", Jw, e)  # a joint at a bound whose descent direction g_j points outward sits this step out
    held = (((q <= lo) & (g < 0.0)) | ((q >= hi) & (g > 0.0))) & hold
    Jm = np.where(held[:, None, :], 0.0, Jw)
    A = np.einsum("nij,nkj->nik", Jm, Jm) + lam[:, None, None] * np.eye(6)[None]
    d = np.einsum("nij,ni->nj", Jm, np.linalg.solve(A, e[:, :, None])[:, :, 0])
    return np.clip(q + d * (max_step / np.maximum(np.abs(d).max(axis=1), max_step))[:, None], lo, hi)


def damped(lam, live, acc, factor=LAMBDA_FACTOR, floor=LAMBDA_FLOOR, ceil=LAMBDA_CEIL):
    """lm_accept's schedule: a live lane's lambda falls by `factor` after an accepted step, rises after a rejected one"""
    return np.where(live, np.where(acc, np.maximum(lam / factor, floor), np.minimum(lam * factor, ceil)), lam)


def solve(robot, targets, seeds, s, factor=LAMBDA_FACTOR, floor=LAMBDA_FLOOR, ceil=LAMBDA_CEIL, hold=True):
    """targets [n][4][4] (or [n][16]), seeds [n][dim], one lane each -> dict(q, err [n][2], converged, iterations, E, E_seed).
    hold=False: the iteration without the bound rule (DESIGN.md 5k records the comparison)."""
    target = np.asarray(targets, np.float64).reshape(-1, 4, 4)
    lo, hi = bounds(robot)
    q = np.clip(np.asarray(seeds, np.float64), lo, hi)
    n, dim = q.shape
    w = 0.0 if s.position_only else s.rot_weight
    W = np.array([1.0, 1.0, 1.0, w, w, w])

    def evaluate(x):
        t, R, J = frame_jac(robot, x)
        e_p, e_w, tr = errors(t, R, target)
        e = weighted(e_p, e_w, tr, s)
        n_p, n_w = np.linalg.norm(e_p, axis=1), np.linalg.norm(e_w, axis=1)
        ok = (n_p <= s.pos_tol) & (s.position_only | ((tr > 1.0) & (n_w <= s.rot_tol)))
        return J * W[None, :, None], e, 0.5 * (e ** 2).sum(axis=1), np.stack([n_p, n_w], axis=1), ok

    Jw, e, E, err, done = evaluate(q)
    E_seed = E.copy()
    lam = np.full(n, float(s.damping))
    its = np.zeros(n, np.int64)
    for _ in range(s.max_iterations):
        if done.all():
            break
        cand = step(q, Jw, e, lam, lo, hi, s.max_step, hold)
        Jc, ec, Ec, errc, okc = evaluate(cand)
        live = ~done
        acc = live & (Ec < E)
        its += live
        lam = damped(lam, live, acc, factor, floor, ceil)
        q[acc], Jw[acc], e[acc], E[acc], err[acc] = cand[acc], Jc[acc], ec[acc], Ec[acc], errc[acc]
        done = done | (acc & okc)
    return dict(q=q, err=err, converged=done, iterations=its, E=E, E_seed=E_seed)


# ---- the inputs the device tests share (tests/test_ik.py holds the condition they rest on) ----------------------------
ROBOTS = ("panda", "ur5", "fetch", "baxter")
N_TARGETS = 33
# Targets are the frames of Halton configurations TARGET_SKIP + 1 .. + 33.  Skip 0 for Panda, Fetch and Baxter.  The UR5's
# first 33 leave two targets with 2 converged seeds of 32 (its wrist reaches most poses in one of eight branches only and
# about 29 % of its lanes converge), short of the 4 the condition asks for; the blocks at 33, 66, 99 and 132 likewise; the
# block at 165 meets it.
TARGET_SKIP = {"panda": 0, "ur5": 165, "fetch": 0, "baxter": 0}
SEED_SKIP = 5000  # the Halton seeds: clear of every target's own configuration, which would converge at once
MIN_CONVERGED = 4


def target_configs(robot):
    return halton32(robot, N_TARGETS, TARGET_SKIP[robot])


def lanes(targets, seeds):
    """targets [T][...], seeds [S][dim] shared -> one row per (target, seed), target-major as vmv_ik_batch lays them out"""
    t = np.asarray(targets)
    return np.repeat(t, len(seeds), axis=0), np.tile(seeds, (len(t), 1))
