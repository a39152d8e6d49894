"""float64 statement of vmv_cartesian_multi (include/vamp_mvt_amd.h): the line between two frames (axis and
angle, the segment count m, pose k) and the tracking of its poses, on tests/ik_serial.py's frame_jac, errors, weighted and
its Levenberg-Marquardt step with the bound rule (ik_serial.solve).  Like ik_serial it is not bit-exact to the device,
which tracks in fp32: it serves to choose inputs, to hold the conditions the device tests rest on, and to measure the
residuals of the device's waypoints.  No validation here: that is validate_motion's part."""
import functools
from dataclasses import dataclass, replace

import numpy as np

import ik_serial

STATUS = ("complete", "ik_failed", "joint_jump", "collision", "invalid_start", "too_long", "non_finite")  # VMV_CART_*


@dataclass
class Settings:
    """vmv_cartesian_settings with its defaults"""
    pos_step: float = 0.01
    rot_step: float = 0.05
    max_iterations: int = 16
    pos_tol: float = 1e-4
    rot_tol: float = 1e-3
    rot_weight: float = 0.25
    damping: float = 1e-2
    max_step: float = 0.5
    max_joint_step: float = 0.3
    max_waypoints: int = 1024
    position_only: bool = False

    def ik(self):
        return ik_serial.Settings(n_seeds=1, max_iterations=self.max_iterations, pos_tol=self.pos_tol, rot_tol=self.rot_tol,
                                  rot_weight=self.rot_weight, damping=self.damping, max_step=self.max_step,
                                  position_only=self.position_only)


def rot(axis, theta):
    """Rodrigues' formula: cos I + sin [a]x + (1 - cos) a a^T"""
    a = np.asarray(axis, np.float64)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.cos(theta) * np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * np.outer(a, a)


def axis_angle(R):
    """-> (axis, theta in [0, pi]) of a rotation matrix: atan2 of the skew part's norm and the trace; beyond 120 degrees
    the axis comes from the symmetric part, signed like the skew part"""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    theta = float(np.arctan2(s, c))
    if c >= -0.5:
        return (np.array([0.0, 0.0, 1.0]) if s < 1e-12 else v / s), theta
    S = 0.5 * (R + R.T) - np.cos(theta) * np.eye(3)
    a = S[:, int(np.argmax(np.diag(S)))]
    a = a / np.linalg.norm(a)
    return (-a if a @ v < 0.0 else a), theta


@dataclass
class Line:
    p0: np.ndarray
    dp: np.ndarray
    R0: np.ndarray
    axis: np.ndarray
    theta: float
    m: int
    ratios: tuple  # the two quotients under the ceils

    def pose(self, k):
        """pose k = 0 .. m as a float64 [4][4] frame"""
        s = k / self.m
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = self.R0 @ rot(self.axis, s * self.theta), self.p0 + s * self.dp
        return T


def line(T0, T1, s):
    """the line from frame T0 to frame T1 ([4][4]; taken as they are, in float64)"""
    T0, T1 = np.asarray(T0, np.float64).reshape(4, 4), np.asarray(T1, np.float64).reshape(4, 4)
    dp = T1[:3, 3] - T0[:3, 3]
    axis, theta = axis_angle(T0[:3, :3].T @ T1[:3, :3])
    if s.position_only:
        theta = 0.0
    ratios = (float(np.linalg.norm(dp) / s.pos_step), float(theta / s.rot_step))
    m = int(max(1, np.ceil(ratios[0]), np.ceil(ratios[1])))
    return Line(T0[:3, 3].copy(), dp, T0[:3, :3].copy(), axis, theta, m, ratios)


def start_frames(robot, starts):
    """what the host sets the lines up from: the starts' frames rounded to fp32 (the device's own differ in the last bits)"""
    return ik_serial.frames44(robot, starts).astype(np.float32)


def track(robot, starts, targets, s, frames=None):
    """All problems side by side, pose by pose -> dict(lines, status [n] (names), achieved [n], evaluations [n],
    worst_evaluations [n] (the most one accepted waypoint took), fail_residual [n] (|e_p| at the waypoint that failed, NaN
    otherwise), paths (list of float64 [achieved + 1][dim])).  frames: the start frames to build the lines from
    (default: start_frames)."""
    starts = np.asarray(starts, np.float64)
    targets = np.asarray(targets, np.float64).reshape(-1, 4, 4)
    n = len(starts)
    frames = start_frames(robot, starts) if frames is None else np.asarray(frames).reshape(-1, 4, 4)
    lines = [line(frames[p], targets[p], s) for p in range(n)]
    status = np.array(["complete"] * n, dtype=object)
    achieved, evaluations, worst = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    fail_residual = np.full(n, np.nan)
    paths = [[starts[p].copy()] for p in range(n)]
    live = np.ones(n, bool)
    for p in range(n):
        if lines[p].m + 1 > s.max_waypoints:
            status[p], live[p] = "too_long", False
    prev = starts.copy()
    k = 0
    while live.any():
        k += 1
        idx = np.flatnonzero(live)
        poses = np.stack([lines[p].pose(k) for p in idx])
        r = ik_serial.solve(robot, poses, prev[idx], s.ik())
        jump = np.abs(r["q"] - prev[idx]).max(axis=1)
        for i, p in enumerate(idx):
            evaluations[p] += int(r["iterations"][i])
            if r["converged"][i] and jump[i] <= s.max_joint_step:
                achieved[p] += 1
                worst[p] = max(worst[p], int(r["iterations"][i]))
                prev[p] = r["q"][i]
                paths[p].append(r["q"][i].copy())
                live[p] = k < lines[p].m
            else:
                status[p] = "joint_jump" if r["converged"][i] else "ik_failed"
                fail_residual[p] = r["err"][i, 0]
                live[p] = False
    return dict(lines=lines, status=status, achieved=achieved, evaluations=evaluations, worst_evaluations=worst,
                fail_residual=fail_residual, paths=[np.array(w) for w in paths])


# ---- the inputs the device tests share (tests/test_cartesian.py holds the conditions they rest on) ---------------------
ROBOTS = ik_serial.ROBOTS
N_STARTS = ik_serial.N_TARGETS  # 33 Halton starts, with ik_serial's TARGET_SKIP rule for the UR5
# world-frame directions of the motion, taken in turn from DIRECTION_SHIFT[robot] on.  The shift is chosen with this
# statement: the UR5's lines from shift 0 leave 15 of its lines complete within max_iterations / 2 evaluations per waypoint
# (7 end as joint jumps next to its wrist singularity), short of the half the condition asks for; shift 1 leaves 25.
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 0), (0, 1, 1), (1, 0, 1),
              (-1, 1, 0), (1, -1, 1))
DIRECTION_SHIFT = {"panda": 0, "ur5": 1, "fetch": 0, "baxter": 0}
ROT_AXES = ((0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 1))
LONG_LINES = ((0.6, 0.0, 0.8), (0.0, -0.8, 0.6), (-0.64, 0.48, 0.6))  # unit directions of the 1.5 m lines
MARGIN = 0.05  # the quotients under the ceils are kept this far from an integer by construction (the test asks 1e-3)
REACH_RESIDUAL = 0.05  # metres: what the best pose towards a line's end still misses where the line has left the reach


def _clear_of_integers(value, step, nudge):
    while abs(value / step - round(value / step)) < MARGIN:
        value += nudge
    return value


@functools.lru_cache(maxsize=None)
def cases(robot):
    """-> (starts float32 [38][dim], targets float32 [38][4][4], names): 33 Halton starts whose frames are moved 5 - 25 cm
    along DIRECTIONS and turned by up to 0.3 rad about ROT_AXES (in the tool frame), then the fixed extras on the first
    starts: zero motion, 1.5 m lines (three, so that every robot has its three lines that leave the reach), a pure rotation.
    position_only is a setting of the call: the device test runs the same set once more with it."""
    s = Settings()
    starts = ik_serial.target_configs(robot)
    F = ik_serial.frames44(robot, starts)
    targets, names = [], []
    for i in range(N_STARTS):
        T = F[i].copy()
        d = np.asarray(DIRECTIONS[(i + DIRECTION_SHIFT[robot]) % len(DIRECTIONS)], np.float64)
        dist = _clear_of_integers(0.05 + 0.2 * ((i * 0.6180339887) % 1.0), s.pos_step, 0.0007)
        ang = _clear_of_integers(0.3 * ((i * 0.7548776662) % 1.0), s.rot_step, 0.0035)
        a = np.asarray(ROT_AXES[i % len(ROT_AXES)], np.float64)
        T[:3, 3] += dist * d / np.linalg.norm(d)
        T[:3, :3] = T[:3, :3] @ rot(a / np.linalg.norm(a), ang)
        targets.append(T)
        names.append(f"halton{i}")
    extra = [F[0].copy()]
    for i, d in enumerate(LONG_LINES):
        extra.append(F[1 + i].copy())
        extra[-1][:3, 3] += 1.5037 * np.asarray(d, np.float64)
    extra.append(F[4].copy())
    extra[-1][:3, :3] = extra[-1][:3, :3] @ rot(np.array([0.0, 0.0, 1.0]), 0.2613)
    names += ["zero_motion", "long_line0", "long_line1", "long_line2", "pure_rotation"]
    starts = np.concatenate([starts, starts[:5]])
    return starts, np.stack(targets + extra).astype(np.float32), tuple(names)


@functools.lru_cache(maxsize=None)
def tracked(robot, position_only=False):
    """the statement's answer for cases(robot), computed once per session"""
    starts, targets, _ = cases(robot)
    return track(robot, starts, targets, Settings(position_only=position_only))


def fast_complete(robot, position_only=False):
    """bool [38]: the lines that complete with every waypoint converging within max_iterations / 2 evaluations"""
    r = tracked(robot, position_only)
    return (r["status"] == "complete") & (r["worst_evaluations"] <= Settings().max_iterations // 2)


@functools.lru_cache(maxsize=None)
def _left_reach(robot, position_only):
    starts, targets, _ = cases(robot)
    r = tracked(robot, position_only)
    s = Settings(position_only=position_only)
    idx = np.flatnonzero((r["status"] == "ik_failed") & (r["worst_evaluations"] <= s.max_iterations // 2))
    out = np.zeros(len(starts), bool)
    if len(idx):
        far = ik_serial.solve(robot, targets[idx], np.stack([r["paths"][p][-1] for p in idx]), replace(s.ik(), max_iterations=64))
        out[idx] = far["err"][:, 0] > REACH_RESIDUAL
    return out


def left_reach(robot, position_only=False):
    """bool [38]: the lines that fail ik_failed because they leave the reach: every waypoint before the failing one
    converged within max_iterations / 2 evaluations, and from the last waypoint 64 evaluations of the same iteration
    towards the line's END still miss it by more than REACH_RESIDUAL.  (The residual at the failing waypoint itself
    cannot be that large: it is one pos_step from a pose that was reached, and the iteration never accepts a worse state.)"""
    return _left_reach(robot, bool(position_only)).copy()


def robust(robot, position_only=False):
    """bool [38]: the cases whose statement answer the device must reproduce"""
    return fast_complete(robot, position_only) | left_reach(robot, position_only)
