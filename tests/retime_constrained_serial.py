"""Serial statement of vmv_retime_multi_constrained (include/vamp_mvt_amd.h) — TEST INFRASTRUCTURE ONLY.

One path at a time: the set-up of tests/retime_serial.py with a level per corner, retime_serial's own profile and
sample, and the round loop - ask every consecutive sample pair, blame the blends a failing pair touches, raise their
corners' levels.  Validity and the band are the caller's hooks `valid(a, b)` and `band_edge(a, b)` (None: always 1).  The
tests without a device pass hand-made callbacks, the CPU oracle or the float64 band of tests/constraint_serial.py; the
device tests pass the product's validate_motion_batch and constraint_check_motion_batch asked one pair at a time, which is
legitimate for the reason tests/rrtc_constrained_serial.py gives: each answer is its pair's own, bit for bit.

Nothing here imports the package."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import retime_serial as RS

STATUS = RS.STATUS + ("out_of_band",)  # VMV_RETIME_*, with VMV_RETIME_OUT_OF_BAND = 5
NONE = RS.NONE


@dataclass(frozen=True)
class Settings(RS.Settings):
    """vmv_retime_constrained_settings with its defaults"""
    blend_halvings: int = 3
    max_rounds: int = 8


def setup(waypoints, S, levels):
    """retime_serial.setup with a level per DISTINCT waypoint (levels[i] <= H: the blend half-length times 2^-levels[i],
    exactly; above: 0, a stop) -> (what, distinct, intervals, Pieces or None, corner per piece (0: a line), keep)"""
    w32 = np.asarray(waypoints, np.float32)
    dim = w32.shape[1] if w32.ndim == 2 else 0
    if w32.size and not np.isfinite(w32).all():
        return "non_finite", 0, 0, None, [], []
    keep = []
    for i in range(len(w32)):
        if not keep or not np.array_equal(w32[i], w32[keep[-1]]):
            keep.append(i)
    m = len(keep)
    if m < 2:
        return "trivial", m, 0, None, [], keep
    w = w32[keep].astype(np.float64)
    blend, step = float(np.float32(S.blend)), float(np.float32(S.grid_step))
    diff = w[1:] - w[:-1]
    total = np.zeros(m - 1)
    for j in range(dim):  # left to right
        total = total + diff[:, j] * diff[:, j]
    L = np.sqrt(total)
    u = diff / L[:, None]
    d = np.zeros(m)
    for i in range(1, m - 1):
        if levels[i] <= S.blend_halvings:
            d[i] = np.ldexp(min(blend, min(0.5 * L[i - 1], 0.5 * L[i])), -int(levels[i]))
    rec, corner, grid, stop_next, quotients = [], [], 0, True, []
    for e in range(m - 1):
        span = L[e] - d[e] - d[e + 1]
        if span > RS.MIN_SPAN:
            quotients.append(span / step)
            n = max(2, int(np.ceil(span / step)))
            rec.append((w[e] + d[e] * u[e], u[e], u[e], 0.0, span, n, grid, stop_next))
            corner.append(0)
            grid, stop_next = grid + n, False
        if e + 1 < m - 1:
            if d[e + 1] > 0.0:
                span = 2.0 * d[e + 1]
                quotients.append(span / step)
                n = max(2, int(np.ceil(span / step)))
                rec.append((w[e + 1] - d[e + 1] * u[e], u[e], u[e + 1], d[e + 1], span, n, grid, stop_next))
                corner.append(e + 1)
                grid, stop_next = grid + n, False
            else:
                stop_next = True
    if grid > S.max_grid:
        return "too_long", 2, grid, None, [], keep
    if not rec:
        return "trivial", 1, 0, None, [], keep
    cols = list(zip(*rec))
    P = RS.Pieces(np.array(cols[0]), np.array(cols[1]), np.array(cols[2]), np.array(cols[3], np.float64),
                  np.array(cols[4], np.float64), np.array(cols[5], np.int64), np.array(cols[6], np.int64),
                  np.array(cols[7], bool), tuple(quotients))
    return "ok", 2, grid, P, corner, keep


@dataclass
class Result(RS.Result):
    first_invalid: int = NONE
    rounds: int = 0
    levels: np.ndarray = None  # uint8, one per input waypoint
    repaired: int = 0
    stops: int = 0
    questions: int = 0
    history: list = field(default_factory=list)  # per round: (levels per distinct waypoint, failing pairs, blamed corners)


def _ask(hook, pos):
    """the hook's answers for the consecutive pairs of pos: one pair at a time, or through hook.batch(starts, goals) where a
    hook offers it (the product's batched calls, whose answers do not depend on the batch)"""
    if hook is None or len(pos) < 2:
        return np.ones(max(len(pos) - 1, 0), bool)
    if hasattr(hook, "batch"):
        return np.asarray(hook.batch(pos[:-1], pos[1:]), bool)
    return np.array([bool(hook(pos[k], pos[k + 1])) for k in range(len(pos) - 1)])


def retime_constrained(waypoints, vel_limits, acc_limits, S=None, valid=None, band_edge=None, dtype=np.float32):
    """one path -> Result; `history` tells what every round saw"""
    S = S or Settings()
    dim = len(vel_limits)
    w32 = np.asarray(waypoints, np.float32).reshape(-1, dim)
    H = S.blend_halvings
    levels = np.full(len(w32), H + 1 if S.stop_at_waypoints else 0, np.int64)  # per distinct waypoint; len(w32) suffice
    empty = [np.zeros(0, dtype)] + [np.zeros((0, dim), dtype)] * 3
    asks = valid is not None or band_edge is not None
    history, questions, keep = [], 0, []

    def done(status, N, count, T, arrays, first_invalid=NONE, rounds=0, P=None, prof=None, where=None):
        out = np.zeros(len(w32), np.uint8)
        inner = range(1, len(keep) - 1)
        for i in inner:
            out[keep[i]] = levels[i]
        return Result(status, N, count, T, *arrays, P, prof, where, first_invalid=first_invalid, rounds=rounds, levels=out,
                      repaired=sum(1 for i in inner if levels[i] > 0), stops=sum(1 for i in inner if levels[i] == H + 1),
                      questions=questions, history=history)

    rnd = 0
    while True:
        rnd += 1
        what, distinct, N, P, corner, keep = setup(w32, S, levels)
        if what == "non_finite":
            return done("non_finite", 0, 0, dtype(0), empty, rounds=rnd)
        if what == "too_long":
            return done("too_long", N, 0, dtype(0), empty, rounds=rnd)
        if what == "trivial":
            if distinct == 0:
                return done("complete", 0, 0, dtype(0), empty, rounds=rnd)
            one = [np.zeros(1, dtype), w32[:1].astype(dtype), np.zeros((1, dim), dtype), np.zeros((1, dim), dtype)]
            return done("complete", 0, 1, dtype(0), one, rounds=rnd)
        prof = RS.profile(P, vel_limits, acc_limits, dtype)
        if not np.isfinite(prof.T).all():
            return done("stalled", N, 0, dtype(0), empty, rounds=rnd, P=P, prof=prof)
        T = prof.T[N]
        count = RS.n_samples(T, S.dt)
        if count > S.max_samples:
            return done("too_long", N, 0, T, empty, rounds=rnd, P=P, prof=prof)
        t, pos, vel, acc, a, s = RS.sample(P, prof, S.dt, count, dtype)
        pos[0], pos[-1] = w32[0], w32[-1]  # the samples are asked as returned
        vel[0], vel[-1] = 0, 0
        arrays = [t, pos, vel, acc]
        fails = []  # (pair, valid, band, the corners it blames, whether it jumps over a whole blend at level H)
        if asks:
            questions += count - 1
            ok_v, ok_b = _ask(valid, pos), _ask(band_edge, pos)
            for k in range(count - 1):
                v, b = bool(ok_v[k]), bool(ok_b[k])
                if not (v and b):
                    mine = sorted({corner[q] for q in range(a[k], a[k + 1] + 1) if P.d[q] > 0.0})
                    over = any(P.d[q] > 0.0 and levels[corner[q]] == H for q in range(a[k] + 1, a[k + 1]))
                    fails.append((k, v, b, mine, over))
        blamed = sorted({i for f in fails for i in f[3]})
        orphan = any(not f[3] for f in fails)
        history.append((levels[:len(keep)].copy(), fails, blamed))
        if not fails:
            return done("complete", N, count, T, arrays, rounds=rnd, P=P, prof=prof, where=(a, s))
        if orphan or rnd >= S.max_rounds:
            return done("collision" if not fails[0][1] else "out_of_band", N, count, T, arrays, first_invalid=fails[0][0],
                        rounds=rnd, P=P, prof=prof, where=(a, s))
        for i in blamed:
            levels[i] += 1


def band64(robot, constraint, settings=None):
    """the float64 band test of an edge on the device's own fp32 samples (tests/constraint_serial.py) -> band_edge(a, b)"""
    import constraint_serial as CS
    cs = settings or CS.Settings()

    def band_edge(a, b):
        q = CS.edge_samples32(a, b, cs.check_step)
        return q is not None and bool(CS.in_band(robot, q, constraint, cs)[0].all())

    return band_edge
