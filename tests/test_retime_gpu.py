"""planning.retime_multi / <robot>.retime_multi on the device.

The yardstick is tests/retime_serial.py: its fp32 form is the definition, and the device's answer equals it bit for bit -
status, intervals, samples, the duration and every sample.  A path's answer is its own whatever the batch.  What the
trajectory promises is then checked in float64 from the device's samples, and validity against the CPU oracle's
validate_motion_batch on the same sample pairs."""
import numpy as np
import pytest

import retime_serial as R
from test_retime import ACC_BAR

pytestmark = pytest.mark.gpu
ROBOTS = R.ROBOTS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return (a.status == b.status and a.intervals == b.intervals and a.first_invalid == b.first_invalid and
            np.array_equal(bits(np.float32(a.duration)), bits(np.float32(b.duration))) and
            all(x.shape == y.shape and np.array_equal(bits(x), bits(y))
                for x, y in ((a.times, b.times), (a.positions, b.positions), (a.velocities, b.velocities),
                             (a.accelerations, b.accelerations))))


def settings(vamp, **kw):
    S = R.replace(R.CASE_SETTINGS, **kw)
    return vamp.planning.RetimeSettings(blend=S.blend, grid_step=S.grid_step, dt=S.dt, max_grid=S.max_grid,
                                        max_samples=S.max_samples, stop_at_waypoints=S.stop_at_waypoints)


@pytest.fixture(scope="module")
def sets(vamp):
    """per robot: the shared case set and ONE call over it - shared by the tests, left unchanged"""
    out = {}
    for robot in ROBOTS:
        mod = getattr(vamp, robot)
        paths = [w for _, w in R.cases(robot)]
        V, A = R.limits(robot)
        out[robot] = dict(mod=mod, paths=paths, V=V, A=A, got=vamp.planning.retime_multi(mod, paths, V, A, None, settings(vamp)))
    return out


def against_statement(names, got, want):
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        assert g.status == w.status, (name, g.status, w.status)
        assert g.intervals == w.intervals and len(g.times) == w.samples, (name, g.intervals, w.intervals, len(g.times), w.samples)
        assert np.array_equal(bits(np.float32(g.duration)), bits(w.duration)), (name, g.duration, w.duration)
        assert g.first_invalid == -1
        for what, x, y in (("times", g.times, w.times), ("positions", g.positions, w.positions),
                           ("velocities", g.velocities, w.velocities), ("accelerations", g.accelerations, w.accelerations)):
            assert x.dtype == np.float32 and x.shape == y.shape, (name, what)
            differ = np.flatnonzero((bits(x) != bits(y)).reshape(len(x), max(x[:1].size, 1)).any(axis=1))
            assert differ.size == 0, (name, what, differ[:5], x[differ[:1]], y[differ[:1]])


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_case_set_equals_the_fp32_statement_bit_for_bit(sets, robot):
    case = sets[robot]
    against_statement([n for n, _ in R.cases(robot)], case["got"], R.results(robot))
    assert sum(len(g.times) for g in case["got"]) > 2000  # (the set is not one of stillborn paths: 20 paths of 100 samples)


@pytest.mark.parametrize("robot", ROBOTS)
def test_stop_at_waypoints_equals_the_statement(vamp, sets, robot):
    case = sets[robot]
    got = vamp.planning.retime_multi(case["mod"], case["paths"], case["V"], case["A"], None, settings(vamp, stop_at_waypoints=True))
    against_statement([n for n, _ in R.cases(robot)], got, R.results(robot, stop_at_waypoints=True))


@pytest.mark.parametrize("dt", (0.001, 0.05))
@pytest.mark.parametrize("robot", ("panda", "baxter"))
def test_other_sampling_periods_equal_the_statement(vamp, sets, robot, dt):
    case = sets[robot]
    got = vamp.planning.retime_multi(case["mod"], case["paths"], case["V"], case["A"], None, settings(vamp, dt=dt))
    against_statement([n for n, _ in R.cases(robot)], got, R.results(robot, dt=dt))


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_paths_answer_does_not_depend_on_the_batch(vamp, sets, robot):
    case = sets[robot]
    mod, paths, V, A, got = case["mod"], case["paths"], case["V"], case["A"], case["got"]
    S = settings(vamp)
    back = vamp.planning.retime_multi(mod, paths[::-1], V, A, None, S)[::-1]
    twice = vamp.planning.retime_multi(mod, paths + paths, V, A, None, S)
    assert all(same(a, b) for a, b in zip(got, back))
    assert all(same(a, b) for a, b in zip(got + got, twice)) and len(twice) == 2 * len(got)
    for p, w in enumerate(paths):
        alone = vamp.planning.retime_multi(mod, [w], V, A, None, S)
        assert len(alone) == 1 and same(alone[0], got[p]), R.cases(robot)[p][0]
    # in the empty environment the sample pairs are validated (the robot against itself): the same samples, whole
    free = vamp.planning.retime_multi(mod, paths, V, A, [None] * len(paths), S)
    for a, b in zip(got, free):
        assert (b.status, b.first_invalid >= 0) in ((a.status, False), ("collision", True)) and b.first_invalid < max(len(b.times) - 1, 0)
        b.status, b.first_invalid = a.status, a.first_invalid
        assert same(a, b)


@pytest.mark.parametrize("robot", ROBOTS)
def test_what_the_trajectory_promises_in_float64(sets, robot):
    case = sets[robot]
    V, A = case["V"].astype(np.float64), case["A"].astype(np.float64)
    dt = float(np.float32(R.CASE_SETTINGS.dt))
    worst_a = worst_p = worst_d = 0.0
    for (name, w), g, s in zip(R.cases(robot), case["got"], R.results(robot)):
        if g.status != "complete" or len(g.times) < 2:
            continue
        pos, vel, acc = (x.astype(np.float64) for x in (g.positions, g.velocities, g.accelerations))
        assert np.array_equal(bits(g.positions[0]), bits(w[0])) and np.array_equal(bits(g.positions[-1]), bits(w[-1]))
        assert not vel[0].any() and not vel[-1].any() and g.times[0] == 0 and g.times[-1] == g.duration
        ratio_a = float((np.abs(acc) / A).max())
        worst_a = max(worst_a, ratio_a)
        assert ratio_a <= ACC_BAR, (name, ratio_a)
        # velocity is bounded at the grid points; between them |q'_j| and x are both linear in s, so each is at most its
        # larger end value: their product bounds every sample of the interval
        pr = s.profile
        N = len(pr.k)
        uin, c, delta = s.pieces.u_in[pr.piece], pr.c.astype(np.float64), pr.delta.astype(np.float64)
        s0 = pr.k * delta
        q_end = np.maximum(np.abs(uin + c * s0[:, None]), np.abs(uin + c * (s0 + delta)[:, None]))
        x_end = np.maximum(pr.x[:N], pr.x[1:]).astype(np.float64)
        bound = float((q_end * np.sqrt(x_end)[:, None] / V).max())
        assert float((np.abs(vel) / V).max()) <= bound * (1 + 1e-6), name
        deviation = float(np.abs(pos - R.path_position64(s)).max())
        worst_p = max(worst_p, deviation)
        assert deviation <= 1e-5, (name, deviation)
        if len(pos) > 3:  # (the last sample is at T, not at a multiple of dt)
            central = (pos[2:-1] - pos[:-3]) / (2.0 * dt)
            off = np.abs(central - vel[1:-2]) / (A * dt)
            worst_d = max(worst_d, float(off.max()))
            assert off.max() <= 1.0, (name, float(off.max()))
    print(f"{robot}: worst |qddot| / A {worst_a:.7f}, worst distance to the float64 path {worst_p:.3g}, "
          f"worst central difference against the velocity {worst_d:.3g} of A dt")


def test_validity_is_validate_motions_on_the_sample_pairs(vamp, oracle):
    """a sphere on the blended corner of a 3-waypoint Panda path, and one clear of it"""
    mod = vamp.panda
    V, A = R.limits("panda")
    a = np.array([0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785], np.float32)
    b, c = a.copy(), a.copy()
    b[0], c[0], c[1] = 0.8, 0.8, -0.2
    path = np.stack([a, b, c])
    corner = mod.fk_batch(b[None])[0]  # [n_spheres][4]
    tip = corner[np.argmax(np.linalg.norm(corner[:, :2], axis=1))]
    rid = oracle.robot("panda")
    results = []
    for centre in (tip[:3], tip[:3] + np.array([0.0, 0.0, 1.5], np.float32)):
        env, oenv = vamp.Environment(), oracle.env()
        env.add_sphere(vamp.Sphere([float(v) for v in centre], 0.08))
        oenv.add_sphere(*[float(v) for v in centre], 0.08)
        got = vamp.planning.retime_multi(mod, [path], V, A, [env])[0]
        free = vamp.planning.retime_multi(mod, [path], V, A, None)[0]
        assert np.array_equal(bits(got.positions), bits(free.positions))  # the samples are returned whole
        valid = oracle.validate_motion_batch(rid, oenv, got.positions[:-1], got.positions[1:])
        want = int(np.argmin(valid)) if not valid.all() else -1
        assert got.first_invalid == want and got.status == ("collision" if want >= 0 else "complete"), (got.first_invalid, want)
        results.append(got.status)
    assert results == ["collision", "complete"]
    raw = mod.retime_multi_raw([path, path], V, A, [None, None], vamp.planning.RetimeSettings())
    assert raw["validation_calls"] == 1 and raw["questions"] == 2 * (len(free.times) - 1)
