"""Statement of vmv_retime_multi (include/vamp_mvt_amd.h) in vectorised numpy: the float64 set-up of a blended
path from fp32 waypoints, the velocity profile on its grid, and the samples.  `dtype` switches the arithmetic of the profile
and the samples: np.float32 is the definition - one rounding per written operation, the device's results bit for bit -
and np.float64 is its twin, for the properties that want the mathematics rather than the roundings.  Sums run left to
right; nothing here imports the package.  No validation here: that is validate_motion's part."""
import functools
from dataclasses import dataclass, replace

import numpy as np

STATUS = ("complete", "collision", "too_long", "non_finite", "stalled")  # VMV_RETIME_*
ROBOTS = ("panda", "ur5", "fetch", "baxter")
DIM = {"panda": 7, "ur5": 6, "fetch": 8, "baxter": 14}
NONE = 0xFFFFFFFF
TINY = 1e-6      # a tangent component that is not larger gives no line and no velocity cap
MIN_SPAN = 1e-9  # a line that is not longer is left out


@dataclass(frozen=True)
class Settings:
    """vmv_retime_settings with its defaults"""
    blend: float = 0.1
    grid_step: float = 0.02
    dt: float = 0.01
    max_grid: int = 4096
    max_samples: int = 65536
    stop_at_waypoints: bool = False


@dataclass
class Pieces:
    """the piece records in float64, as the host makes them; the device reads them rounded to fp32"""
    base: np.ndarray   # [P][dim]
    u_in: np.ndarray   # [P][dim]
    u_out: np.ndarray  # [P][dim]
    d: np.ndarray      # [P]
    span: np.ndarray   # [P]
    n: np.ndarray      # [P] int64
    first: np.ndarray  # [P] int64
    stop: np.ndarray   # [P] bool
    quotients: tuple = ()  # every span / grid_step that went under a ceil


def setup(waypoints, S):
    """-> (what, distinct, intervals, Pieces or None); what: "ok", "trivial", "too_long", "non_finite" """
    w32 = np.asarray(waypoints, np.float32)
    dim = w32.shape[1] if w32.ndim == 2 else 0
    if w32.size and not np.isfinite(w32).all():
        return "non_finite", 0, 0, None
    keep = []
    for i in range(len(w32)):
        if not keep or not np.array_equal(w32[i], w32[keep[-1]]):
            keep.append(i)
    m = len(keep)
    if m < 2:
        return "trivial", m, 0, None
    w = w32[keep].astype(np.float64)
    blend, step = float(np.float32(S.blend)), float(np.float32(S.grid_step))
    diff = w[1:] - w[:-1]
    total = np.zeros(m - 1)
    for j in range(dim):  # left to right
        total = total + diff[:, j] * diff[:, j]
    L = np.sqrt(total)
    u = diff / L[:, None]
    d = np.zeros(m)
    if not S.stop_at_waypoints:
        d[1:-1] = np.minimum(blend, np.minimum(0.5 * L[:-1], 0.5 * L[1:]))
    rec, grid, stop_next, quotients = [], 0, True, []
    for e in range(m - 1):
        span = L[e] - d[e] - d[e + 1]
        if span > MIN_SPAN:
            quotients.append(span / step)
            n = max(2, int(np.ceil(span / step)))
            rec.append((w[e] + d[e] * u[e], u[e], u[e], 0.0, span, n, grid, stop_next))
            grid, stop_next = grid + n, False
        if e + 1 < m - 1:
            if d[e + 1] > 0.0:
                span = 2.0 * d[e + 1]
                quotients.append(span / step)
                n = max(2, int(np.ceil(span / step)))
                rec.append((w[e + 1] - d[e + 1] * u[e], u[e], u[e + 1], d[e + 1], span, n, grid, stop_next))
                grid, stop_next = grid + n, False
            else:
                stop_next = True
    if grid > S.max_grid:
        return "too_long", 2, grid, None
    if not rec:
        return "trivial", 1, 0, None
    cols = list(zip(*rec))
    return "ok", 2, grid, Pieces(np.array(cols[0]), np.array(cols[1]), np.array(cols[2]), np.array(cols[3], np.float64),
                                 np.array(cols[4], np.float64), np.array(cols[5], np.int64), np.array(cols[6], np.int64),
                                 np.array(cols[7], bool), tuple(quotients))


@dataclass
class Profile:
    """per interval (N rows): piece, k, delta, two_d, the curvature c [N][dim], the bands slope / g / line
    [N][2 dim] in the lanes' order (2 j + end) and the caps; per grid point (N + 1): xv, K, x, T; per interval: u"""
    piece: np.ndarray
    k: np.ndarray
    delta: np.ndarray
    two_d: np.ndarray
    c: np.ndarray
    slope: np.ndarray
    g: np.ndarray
    line: np.ndarray
    cap: np.ndarray
    pre: np.ndarray  # [N] what bounds K_i without the neighbour: caps, velocity caps, the joint lines' pairs
    xv: np.ndarray
    K: np.ndarray
    x: np.ndarray
    u: np.ndarray
    T: np.ndarray
    vel_binds: bool
    acc_binds: bool


def _records(P, dtype):
    return (P.base.astype(dtype), P.u_in.astype(dtype), P.u_out.astype(dtype), P.d.astype(dtype), P.span.astype(dtype))


def profile(P, vel_limits, acc_limits, dtype=np.float32):
    f = dtype
    base, u_in, u_out, d, span = _records(P, f)
    V, A = np.asarray(vel_limits, np.float32).astype(f), np.asarray(acc_limits, np.float32).astype(f)
    dim = len(V)
    inf = f(np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        delta_p = span / P.n.astype(f)
        dd = d + d
        c_p = np.where((d > 0)[:, None], (u_out - u_in) / np.where(dd > 0, dd, f(1))[:, None], f(0)).astype(f)
        piece = np.repeat(np.arange(len(P.n)), P.n)
        k = np.concatenate([np.arange(n) for n in P.n])
        N = len(k)
        delta = delta_p[piece]
        two_d = delta + delta
        c, uin = c_p[piece], u_in[piece]
        s0, s1 = k.astype(f) * delta, (k + 1).astype(f) * delta
        a0, a1 = uin + c * s0[:, None], uin + c * s1[:, None]
        a = np.stack([a0, a1], axis=2).reshape(N, 2 * dim)  # lane 2 j + end
        cc = np.stack([a0, a1 + two_d[:, None] * c], axis=2).reshape(N, 2 * dim)
        e = np.repeat(c, 2, axis=1)
        Ab, Vb = np.repeat(A, 2)[None, :], np.repeat(V, 2)[None, :]
        line = np.abs(cc) > f(TINY)
        safe = np.where(line, cc, f(1))
        slope = np.where(line, (-e) / safe, f(0)).astype(f)
        g = np.where(line, Ab / np.abs(safe), inf).astype(f)
        cap = np.where(~line & (e != 0), Ab / np.abs(np.where(e != 0, e, f(1))), inf).astype(f)
        moving = np.abs(a) > f(TINY)
        ratio = Vb / np.abs(np.where(moving, a, f(1)))
        vc = np.where(moving, ratio * ratio, inf).astype(f)
        v_start, v_end = vc[:, 0::2].min(axis=1), vc[:, 1::2].min(axis=1)
        den = slope[:, :, None] - slope[:, None, :]  # lower line of band p against upper line of band q
        num = g[:, :, None] + g[:, None, :]
        th = np.where(den > 0, num / np.where(den > 0, den, f(1)), inf).reshape(N, -1).min(axis=1)

        xv = np.full(N + 1, inf, f)
        xv[:N] = np.minimum(xv[:N], v_start)
        xv[1:] = np.minimum(xv[1:], v_end)
        xv[P.first[P.stop]] = 0
        xv[N] = 0
        K = np.zeros(N + 1, f)
        K[:N] = np.minimum(np.minimum(th, cap.min(axis=1)), xv[:N])
        pre = K[:N].copy()
        zero = f(0)
        for i in range(N - 1, -1, -1):  # backward
            sd, gd = slope[i] * two_d[i], g[i] * two_d[i]  # the reach lines, times 2 Delta
            den1 = f(-1) - sd
            den2 = f(1) + sd
            th1 = np.where(line[i] & (den1 > 0), gd / np.where(den1 > 0, den1, f(1)), inf)
            th2 = np.where(line[i] & (den2 > 0), (K[i + 1] + gd) / np.where(den2 > 0, den2, f(1)), inf)
            K[i] = max(zero, min(K[i], th1.min(), th2.min()))
        x, u, T = np.zeros(N + 1, f), np.zeros(N + 1, f), np.zeros(N + 1, f)
        acc_binds = False
        for i in range(N):  # forward
            sx = slope[i] * x[i]
            up = np.where(line[i], g[i] + sx, inf).min()
            lo = np.where(line[i], sx - g[i], -inf).max()
            reach_up, reach_lo = (K[i + 1] - x[i]) / two_d[i], (-x[i]) / two_d[i]
            ui = max(min(up, reach_up), max(lo, reach_lo))
            acc_binds = acc_binds or (up < reach_up) or (lo > reach_lo and ui == lo)
            xn = min(max(x[i] + two_d[i] * ui, zero), K[i + 1])
            u[i] = ui
            T[i + 1] = T[i] + two_d[i] / (np.sqrt(x[i]) + np.sqrt(xn))
            x[i + 1] = xn
    inner = np.isfinite(xv) & (xv > 0)
    vel_binds = bool((x[inner] >= xv[inner] * f(1 - 1e-6)).any())
    return Profile(piece, k, delta, two_d, c, slope, g, line, cap, pre, xv, K, x, u, T, vel_binds, bool(acc_binds))


def sample_quotient(T, dt):
    return float(T) / float(np.float32(dt))


def n_samples(T, dt):
    return int(np.ceil(sample_quotient(T, dt))) + 1


def sample(P, prof, dt, count, dtype=np.float32):
    """-> times [S], positions, velocities, accelerations [S][dim], and where each sample lies: piece, s"""
    f = dtype
    base, u_in, u_out, d, span = _records(P, f)
    N = len(prof.k)
    ks = np.arange(count)
    t = np.minimum(ks.astype(f) * f(np.float32(dt)), prof.T[N])
    i = np.clip(np.searchsorted(prof.T[:N], t, side="right") - 1, 0, N - 1)  # the last interval with T_i <= t
    a = prof.piece[i]
    s0 = prof.k[i].astype(f) * prof.delta[i]
    x, u, tau = prof.x[i], prof.u[i], t - prof.T[i]
    sigma = np.minimum(np.maximum(np.sqrt(x) * tau + (f(0.5) * u) * (tau * tau), f(0)), prof.delta[i])
    s = s0 + sigma
    ss = s * s
    xs = np.maximum(x + (u + u) * sigma, f(0))
    rate = np.sqrt(xs)
    c, uin = prof.c[i], u_in[a]
    qp = uin + c * s[:, None]
    pos = (base[a] + uin * s[:, None]) + (f(0.5) * c) * ss[:, None]
    vel = qp * rate[:, None]
    acc = qp * u[:, None] + c * xs[:, None]
    return t, pos, vel, acc, a, s


@dataclass
class Result:
    status: str
    intervals: int
    samples: int
    duration: object  # dtype scalar
    times: np.ndarray
    positions: np.ndarray
    velocities: np.ndarray
    accelerations: np.ndarray
    pieces: object = None
    profile: object = None
    where: object = None  # (piece, s) of every sample


def retime(waypoints, vel_limits, acc_limits, S=None, dtype=np.float32):
    """one path -> Result (status "collision" is never given here)"""
    S = S or Settings()
    dim = len(vel_limits)
    w32 = np.asarray(waypoints, np.float32).reshape(-1, dim)
    empty = [np.zeros(0, dtype)] + [np.zeros((0, dim), dtype)] * 3
    what, distinct, N, P = setup(w32, S)
    if what == "non_finite":
        return Result("non_finite", 0, 0, dtype(0), *empty)
    if what == "too_long":
        return Result("too_long", N, 0, dtype(0), *empty)
    if what == "trivial":
        if distinct == 0:
            return Result("complete", 0, 0, dtype(0), *empty)
        return Result("complete", 0, 1, dtype(0), np.zeros(1, dtype), w32[:1].astype(dtype), np.zeros((1, dim), dtype),
                      np.zeros((1, dim), dtype))
    prof = profile(P, vel_limits, acc_limits, dtype)
    if not np.isfinite(prof.T).all():
        return Result("stalled", N, 0, dtype(0), *empty, P, prof)
    T = prof.T[N]
    count = n_samples(T, S.dt)
    if count > S.max_samples:
        return Result("too_long", N, 0, T, *empty, P, prof)
    t, pos, vel, acc, a, s = sample(P, prof, S.dt, count, dtype)
    pos[0], pos[-1] = w32[0], w32[-1]  # the waypoints' own bits, at rest
    vel[0], vel[-1] = 0, 0
    return Result("complete", N, count, T, t, pos, vel, acc, P, prof, (a, s))


# ---- what the tests measure ------------------------------------------------------------------------------------------
def line_time(w0, w1, V, A):
    """closed form of a straight rest-to-rest motion: the trapezoid or triangle of the limiting joints (float64)"""
    diff = np.asarray(w1, np.float64) - np.asarray(w0, np.float64)
    L = np.sqrt((diff * diff).sum())
    un = np.abs(diff / L)
    move = un > 0
    v = (np.asarray(V, np.float64)[move] / un[move]).min()
    a = (np.asarray(A, np.float64)[move] / un[move]).min()
    return L / v + v / a if L >= v * v / a else 2.0 * np.sqrt(L / a)


def limit_ratios(R, V, A, sub=8):
    """-> (largest |qdot_j| / V_j at the grid points, largest |qddot_j| / A_j at `sub` sub-samples of every interval,
    both ends included), evaluated in float64 from the result's profile"""
    P, pr = R.pieces, R.profile
    N = len(pr.k)
    V, A = np.asarray(V, np.float64), np.asarray(A, np.float64)
    c = pr.c.astype(np.float64)
    uin = P.u_in[pr.piece]
    delta, x, u = pr.delta.astype(np.float64), pr.x.astype(np.float64), pr.u.astype(np.float64)
    s0 = pr.k * delta
    worst_a = 0.0
    for m in range(sub + 1):
        sg = (m / sub) * delta
        qp = uin + c * (s0 + sg)[:, None]
        xs = np.maximum(x[:N] + 2.0 * u[:N] * sg, 0.0)
        worst_a = max(worst_a, float((np.abs(qp * u[:N, None] + c * xs[:, None]) / A).max()))
    qp0, qp1 = uin + c * s0[:, None], uin + c * (s0 + delta)[:, None]
    worst_v = max(float((np.abs(qp0) * np.sqrt(x[:N, None]) / V).max()), float((np.abs(qp1) * np.sqrt(x[1:, None]) / V).max()))
    return worst_v, worst_a


def path_position64(R):
    """the float64 blended path at the places of R's samples"""
    P = R.pieces
    a, s = R.where
    s = s.astype(np.float64)
    dd = np.where(P.d > 0, 2.0 * P.d, 1.0)
    c = np.where((P.d > 0)[:, None], (P.u_out - P.u_in) / dd[:, None], 0.0)
    return P.base[a] + P.u_in[a] * s[:, None] + 0.5 * c[a] * (s * s)[:, None]


# ---- the shared case set ---------------------------------------------------------------------------------------------
SEED = 2602  # chosen so that no quotient under a ceil comes near an integer (tests/test_retime.py holds the condition)
CASE_SETTINGS = Settings(grid_step=0.019, max_grid=1200)  # (2 blend / grid_step is no integer)


def limits(robot):
    dim = DIM[robot]
    return (1.0 + 0.1 * np.arange(dim)).astype(np.float32), (2.0 + 0.3 * np.arange(dim)).astype(np.float32)


def _line_of(q0, direction, length):
    direction = np.asarray(direction, np.float64)
    return np.stack([q0, q0 + length * direction / np.sqrt((direction * direction).sum())]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases(robot):
    """-> tuple of (name, float32 [len][dim] waypoints), in shuffled order"""
    dim = DIM[robot]
    rng = np.random.default_rng(SEED + dim)
    q0 = rng.uniform(-0.5, 0.5, dim)
    e = np.eye(dim)
    ones = np.ones(dim)
    skew = 1.0 + 0.37 * np.arange(dim)
    out = []
    out.append(("line_cap", _line_of(q0, ones, 2.61)))
    out.append(("line_no_cap", _line_of(q0, skew, 0.27)))
    out.append(("line_1mm", _line_of(q0, e[1], 0.001)))
    out.append(("right_angle", np.stack([q0, q0 + 0.5 * e[0], q0 + 0.5 * e[0] + 0.5 * e[1]])))
    out.append(("collinear", np.stack([q0, q0 + 0.25 * ones, q0 + 0.77 * ones])))
    out.append(("reversal", np.stack([q0, q0 + 0.13 * skew, q0])))
    out.append(("one_joint", np.stack([q0, q0 + 0.3 * e[2], q0 + 0.81 * e[2]])))
    zig = [q0]
    for k in range(5):
        zig.append(zig[-1] + 0.05 * (e[k % 3] if k % 2 == 0 else -e[(k + 1) % 3] + 0.3 * e[3]))
    out.append(("short_segments", np.stack(zig)))
    curve = [q0]
    for k in range(39):
        curve.append(curve[-1] + 0.05 * (np.cos(0.1 * k) * e[0] + np.sin(0.1 * k) * e[1] + 0.2 * e[dim - 1]))
    out.append(("bspline_40", np.stack(curve)))
    a, b, c = q0, q0 + 0.4 * e[0] - 0.2 * e[3], q0 + 0.1 * ones
    out.append(("duplicates", np.stack([a, a, b, b, b, c])))
    out.append(("no_waypoints", np.zeros((0, dim))))
    out.append(("one_waypoint", np.stack([q0])))
    out.append(("one_waypoint_thrice", np.stack([q0, q0, q0])))
    bad = np.stack([q0, q0 + 0.3 * ones, q0 + 0.5 * e[0]])
    bad[1, 2] = np.nan
    out.append(("nan_waypoint", bad))
    bad = np.stack([q0, q0 + 0.3 * ones])
    bad[1, 0] = np.inf
    out.append(("inf_waypoint", bad))
    step = CASE_SETTINGS.grid_step
    out.append(("at_max_grid", _line_of(q0, skew, step * (CASE_SETTINGS.max_grid - 0.5))))
    out.append(("over_max_grid", _line_of(q0, skew, step * (CASE_SETTINGS.max_grid + 0.5))))
    for total in (63, 64, 65):
        out.append((f"intervals_{total}", _line_of(q0, ones - 0.5 * e[0], step * (total - 0.5))))
    walk, length = [q0], 0.0
    while length < 950 * step:
        walk.append(rng.uniform(-1.6, 1.6, dim) * np.sqrt(7.0 / dim))
        length += np.sqrt(((walk[-1] - walk[-2]) ** 2).sum())
    out.append(("intervals_1100", np.stack(walk)))
    out.append(("joint_0_alone", _line_of(q0, e[0], 0.35)))  # Fetch's prismatic joint
    out.append(("uneven_corner", np.stack([q0, q0 + 0.3 * e[1], q0 + 0.3 * e[1] + 0.05 * e[2] + 0.01 * e[0]])))
    for k in range(4):
        count = 3 + k
        out.append((f"random_{count}", np.stack([q0] + [rng.uniform(-1.0, 1.0, dim) for _ in range(count - 1)])))
    order = rng.permutation(len(out))
    return tuple((out[i][0], np.ascontiguousarray(out[i][1], np.float32)) for i in order)


@functools.lru_cache(maxsize=None)
def results(robot, stop_at_waypoints=False, dt=CASE_SETTINGS.dt, dtype=np.float32):
    """the statement's results over the robot's case set, in its order; computed once per session"""
    S = replace(CASE_SETTINGS, stop_at_waypoints=stop_at_waypoints, dt=dt)
    V, A = limits(robot)
    return tuple(retime(w, V, A, S, dtype) for _, w in cases(robot))
