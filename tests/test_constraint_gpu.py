"""<robot>.project_batch, <robot>.constraint_check_batch and <robot>.constraint_check_motion_batch on the device.

There is no reference for constraints; the yardsticks are the float64 evaluation of the generator's end-effector tape and
the float64 statement of the residual, the band test and the projection (tests/constraint_serial.py).  A projection is
checked for what it promises - in the band by the float64 tape, inside the joint bounds, fixed points returned bit for bit -
and everything else is bit for bit: a lane against itself in other batches, orders and record layouts, an edge against the
band tests of its own samples.  SLACK: the device's frame differs from the float64 tape's (its sine is a polynomial); each
test measures the largest difference on its own outputs and allows twice that at a band face."""
import numpy as np
import pytest

import constraint_serial as S
import ik_serial as K

pytestmark = pytest.mark.gpu
ROBOTS = S.ROBOTS
NAMES = ("upright", "plane", "box_cone")
# The device's converged share is held against the float64 statement's on the same 130 rows (computed in the fixture on the
# CPU; DESIGN.md 5o records the figures) less this margin for fp32 lanes that stall one step from the band.
MARGIN = 0.05


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)  # (bytes: the results hold float32, int32 and bool arrays)


def to_vamp(vamp, c):
    return vamp.EEConstraint(frame=c.frame, pos_lo=c.pos_lo, pos_hi=c.pos_hi, tool_axis=c.tool_axis, ref_axis=c.ref_axis, max_angle=c.max_angle)


def frame_slack(mod, robot, q):
    """twice the largest difference between eefk_batch and the float64 tape on q"""
    q = np.ascontiguousarray(q, np.float32)
    return 2.0 * float(np.abs(mod.eefk_batch(q).astype(np.float64) - K.frames44(robot, q.astype(np.float64))).max())


@pytest.fixture(scope="module")
def cases(vamp):
    """per robot and constraint: the 130 configurations, the constraint in both forms, ONE projection of all rows and the
    float64 statement's projection of the same rows - shared by the tests, left unchanged"""
    out = {}
    for robot in ROBOTS:
        mod = getattr(vamp, robot)
        q = S.configs(robot)
        for name, c in S.cases(robot).items():
            vc = to_vamp(vamp, c)
            out[robot, name] = dict(mod=mod, q=q, c=c, vc=vc, got=mod.project_batch(q, vc), want=S.project(robot, q, c))
    return out


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_projection_keeps_its_promises(vamp, cases, robot, name):
    case = cases[robot, name]
    mod, q0, c, vc = case["mod"], case["q"], case["c"], case["vc"]
    q, res, conv, evals = case["got"]
    n, dim = S.N, mod.dimension()
    assert q.shape == (n, dim) and res.shape == (n, 2) and conv.shape == (n,) and evals.shape == (n,)
    assert q.dtype == np.float32 and conv.dtype == bool
    lo, hi = K.bounds(robot)
    assert np.isfinite(q).all() and ((q >= lo) & (q <= hi)).all()
    slack = frame_slack(mod, robot, q)
    ok, r = S.in_band(robot, q, c, slack=slack)
    share, want_share = float(conv.mean()), float(case["want"]["converged"].mean())
    print(f"{robot} {name}: converged {share:.3f} (float64 statement {want_share:.3f}), mean evaluations {evals.mean():.1f}, "
          f"slack {slack:.2e}, largest float64 residual of a converged row {r['res'][conv].max(axis=0)}")
    assert conv.any() and ok[conv].all()
    assert share >= want_share - MARGIN
    # a row that is not converged ran all 16 evaluations - or none, where its axes were antiparallel: it is back as given
    stuck = ~conv & (evals == 0)
    assert ((evals >= 0) & (evals <= 16)).all() and (evals[~conv & ~stuck] == 16).all()
    assert np.array_equal(bits(q[stuck]), bits(q0[stuck]))
    # joints that do not move the end effector come back bit for bit (Baxter's other arm)
    moves = S.ee_mask(robot)
    assert np.array_equal(bits(q[:, ~moves]), bits(q0[:, ~moves])) and (robot != "baxter" or (~moves).sum() == 7)
    # the reported residuals are the float64 ones of the returned rows, up to the frames' difference d = slack / 2: |v| is
    # 1-Lipschitz in p and each p_k moves by at most sqrt(3) d, so |v| by at most 3 d; the angle is atan2 of |a x d| and
    # a . d, 1-Lipschitz in each on the unit circle, and these move by at most 2 sqrt(3) d and 3 d: 10 d covers the sum
    exact = S.in_band(robot, q, c)[1]["res"]
    assert np.abs(res[:, 0] - exact[:, 0]).max() <= 2 * slack and np.abs(res[:, 1] - exact[:, 1]).max() <= 5 * slack
    # a fixed point: a converged row is inside the bounds and in the band, so it comes back bit for bit with 0 evaluations
    q2, res2, conv2, evals2 = mod.project_batch(q[conv], vc)
    assert np.array_equal(bits(q2), bits(q[conv])) and conv2.all() and (evals2 == 0).all()
    assert np.array_equal(bits(res2), bits(res[conv]))
    # ... and the check agrees with the projection's own converged test on every row
    assert np.array_equal(mod.constraint_check_batch(q, vc), conv)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_lane_is_its_own(vamp, cases, robot, name):
    """subsets, a permutation, n = 1 and n = 0, shared against per-lane records, mixed records, torch against numpy"""
    import torch

    case = cases[robot, name]
    mod, q0, vc = case["mod"], case["q"], case["vc"]
    whole = case["got"]

    def same(got, idx):
        return all(np.array_equal(bits(np.asarray(g)), bits(np.asarray(w)[idx])) for g, w in zip(got, whole))

    for idx in (np.arange(64), np.arange(63, 130), np.array([129]), np.random.default_rng(5).permutation(130), np.arange(0, 130, 7)):
        assert same(mod.project_batch(q0[idx], vc), idx)
    assert same(mod.project_batch(q0, [vc] * S.N), np.arange(S.N))  # one record per lane
    empty = mod.project_batch(q0[:0], vc)
    assert [len(x) for x in empty] == [0, 0, 0, 0]
    # every lane its own constraint: rows of three different constraints in one call
    kinds = [cases[robot, NAMES[i % 3]] for i in range(S.N)]
    mixed = mod.project_batch(q0, [k["vc"] for k in kinds])
    for i in range(S.N):
        assert all(np.array_equal(bits(np.asarray(m[i])), bits(np.asarray(w[i]))) for m, w in zip(mixed, kinds[i]["got"])), i
    tq, tres, tconv, tev = mod.project_batch(torch.from_numpy(q0).cuda(), vc)
    assert same((tq.cpu().numpy(), tres.cpu().numpy(), tconv.cpu().numpy(), tev.cpu().numpy().astype(np.int32)), np.arange(S.N))
    ok = mod.constraint_check_batch(torch.from_numpy(whole[0]).cuda(), vc)
    assert np.array_equal(ok.cpu().numpy(), mod.constraint_check_batch(whole[0], vc))


@pytest.mark.parametrize("robot", ROBOTS)
def test_non_finite_rows(vamp, cases, robot):
    case = cases[robot, "upright"]
    mod, vc = case["mod"], case["vc"]
    q = case["q"].copy()
    spoiled = [0, 64, 65, 129]
    q[0, 0], q[64, 1], q[65, -1], q[129, 2] = np.nan, np.inf, -np.inf, np.nan
    got = mod.project_batch(q, vc)
    from vamp_mvt_amd import _lib
    import ctypes

    status = np.zeros(len(q), np.uint32)
    out, res = np.zeros_like(q), np.zeros((len(q), 2), np.float32)
    recs = (_lib.EeConstraint * 1)(vc.struct())
    cs = vamp.ConstraintSettings().struct()
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    assert _lib.lib.vmv_constraint_project_batch_host(vamp.robots.index(robot), fp(q), len(q), recs, 1, ctypes.byref(cs), fp(out), fp(res),
                                                      status.ctypes.data_as(_lib.c_u32_p)) == 0
    assert ((status >> 30) & 1).astype(bool).tolist() == [i in spoiled for i in range(len(q))]
    assert not (status[spoiled] >> 31).any() and (status[spoiled] & 0x3fffffff == 0).all()
    assert np.array_equal(bits(out), bits(got[0]))
    assert np.array_equal(bits(got[0][spoiled]), bits(q[spoiled])) and np.isnan(got[1][spoiled]).all() and not got[2][spoiled].any()
    clean = np.setdiff1d(np.arange(len(q)), spoiled)
    assert all(np.array_equal(bits(np.asarray(g)[clean]), bits(np.asarray(w)[clean])) for g, w in zip(got, case["got"]))
    ok, r = mod.constraint_check_batch(q, vc, residuals=True)
    assert not ok[spoiled].any() and np.isnan(r[spoiled]).all()
    assert np.array_equal(ok[clean], mod.constraint_check_batch(case["q"], vc)[clean])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_check_against_the_float64_band_test(vamp, cases, robot, name):
    """the inputs (mostly out of band), the projections (at the band's faces) and points between them"""
    case = cases[robot, name]
    mod, c, vc = case["mod"], case["c"], case["vc"]
    q1 = case["got"][0]
    mid = ((case["q"].astype(np.float64) + q1) / 2).astype(np.float32)
    q = np.concatenate([case["q"], q1, mid])
    got, res = mod.constraint_check_batch(q, vc, residuals=True)
    assert got.shape == (len(q),) and got.dtype == bool
    slack = frame_slack(mod, robot, q)
    want, r = S.in_band(robot, q, c)
    # the margin is metres for the box and a difference of cosines for the cone; both move by at most the frame's slack
    clear = S.band_margin(robot, q, c) > slack
    print(f"{robot} {name}: {got.sum()} of {len(q)} in band, {int((~clear).sum())} within {slack:.2e} of a face")
    assert clear.sum() >= len(q) // 2 and np.array_equal(got[clear], want[clear])
    assert np.abs(res[:, 0] - r["res"][:, 0]).max() <= 2 * slack
    for n in (1, 63, 64, 65, 0):  # a word, its neighbours, nothing
        assert np.array_equal(mod.constraint_check_batch(q[:n], vc), got[:n])
    assert np.array_equal(mod.constraint_check_batch(q, [vc] * len(q)), got)


@pytest.mark.parametrize("robot", ROBOTS)
def test_motion_check_is_the_and_of_its_samples(vamp, cases, robot):
    """edges between converged rows (short and long), zero-length edges, an edge of exactly check_step, one just beyond 64
    samples and one beyond the 1,024 cap: bit for bit the AND of constraint_check_batch over the samples the statement
    forms in fp32"""
    case = cases[robot, "upright"]
    mod, vc = case["mod"], case["vc"]
    q = case["got"][0][case["got"][2]]
    dim = mod.dimension()
    moves = np.flatnonzero(S.ee_mask(robot))
    rng = np.random.default_rng(3)
    a = [q[i] for i in range(24)] + [q[i] for i in range(8)]
    b = [q[i + 1] for i in range(24)] + [(q[i] + rng.normal(0, 0.02, dim) * S.ee_mask(robot)).astype(np.float32) for i in range(8)]
    a += [q[0], q[1]]  # zero-length edges: one sample, the end point itself
    b += [q[0], q[1]]
    unit = np.zeros(dim, np.float32)
    unit[moves[-1]] = 1.0  # the last wrist joint: it turns the tool about its own axis, or nearly
    base = np.zeros(dim, np.float32)
    for length in (np.float32(0.05), np.float32(64 * 0.05 + 0.01), np.float32(1024 * 0.05 + 0.01)):
        a.append(base.copy())
        b.append((base + unit * length).astype(np.float32))
    a, b = np.array(a, np.float32), np.array(b, np.float32)
    counts = [None if S.edge_samples32(x, y) is None else len(S.edge_samples32(x, y)) for x, y in zip(a, b)]
    assert counts[-3:] == [1, 65, None] and counts[32:34] == [1, 1] and max(c for c in counts if c) >= 65
    got = mod.constraint_check_motion_batch(a, b, vc)
    assert got.shape == (len(a),) and got.dtype == bool
    want = []
    for x, y in zip(a, b):
        s = S.edge_samples32(x, y)
        want.append(False if s is None else bool(mod.constraint_check_batch(s, vc).all()))
    print(f"{robot}: {int(got.sum())} of {len(got)} edges in band; samples per edge {counts}")
    assert got.tolist() == want and not got[-1] and got[32] and got[33] and got.any() and not got.all()
    # The chord error of check_step, per passing edge: with u the edge's unit direction, the tool axis turns at a rate of at
    # most sum_j |u_j| rad per unit of joint-space length (over the joints that move the end effector), so between two
    # passing samples h = |b - a| / n_c apart no point is farther beyond the cone than sum_j |u_j| * h / 2: 0.025 rad for the
    # 65-sample edge along one joint, 0 for a zero-length edge.  The passing samples passed in fp32: the float64 cosine differs
    # by at most 3 d = 1.5 slack (d the frames' difference), the angle by that over sin(band angle).  Where a sample sits
    # is held bit for bit by the AND above; this holds what the spacing promises.  Measured at 4x finer float64 samples.
    band = 0.1 + 1e-3
    moves = S.ee_mask(robot)
    tol = 1.5 * frame_slack(mod, robot, np.concatenate([a[got], b[got]])) / np.sin(band)
    worst, tightest = -np.inf, np.inf  # (a negative excess: every finer sample lies inside the band)
    for x, y, n_c in zip(a[got].astype(np.float64), b[got].astype(np.float64), [c for c, g in zip(counts, got) if g]):
        t = np.arange(4, 4 * n_c + 1) / (4.0 * n_c)
        fine = x[None, :] + (y - x)[None, :] * t[:, None]
        cs = S.in_band(robot, fine, case["c"])[1]["cs"]
        excess = float((np.arccos(np.clip(cs, -1.0, 1.0)) - band).max())
        length = np.linalg.norm(y - x)
        bound = (np.abs(y - x)[moves].sum() / length if length > 0 else 0.0) * (length / n_c) / 2
        worst, tightest = max(worst, excess), min(tightest, bound + tol - excess)
        assert excess <= bound + tol, (n_c, excess, bound, tol)
    print(f"{robot}: largest angle beyond the band between passing samples {worst:.3e} rad; least room under an edge's bound {tightest:.3e}")
    # an edge is its own: alone, reversed order, per-edge records, torch
    import torch

    assert np.array_equal(mod.constraint_check_motion_batch(a[::-1], b[::-1], vc), got[::-1])
    assert np.array_equal(mod.constraint_check_motion_batch(a, b, [vc] * len(a)), got)
    assert all(mod.constraint_check_motion_batch(a[i:i + 1], b[i:i + 1], vc)[0] == got[i] for i in (0, 5, len(a) - 2, len(a) - 1))
    assert np.array_equal(mod.constraint_check_motion_batch(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), vc).cpu().numpy(), got)
    # a coarser check_step asks fewer samples, and the statement's samples follow it
    coarse = vamp.ConstraintSettings(check_step=0.5)
    want = [bool(mod.constraint_check_batch(S.edge_samples32(x, y, 0.5), vc, coarse).all()) for x, y in zip(a, b)]
    assert mod.constraint_check_motion_batch(a, b, vc, coarse).tolist() == want


def test_planning_helpers_on_the_device(vamp, cases):
    """project_goals gives in-band, collision-free rows; validate_paths_constrained is the AND over a path's edges"""
    P = vamp.planning
    case = cases["panda", "upright"]
    mod, vc, q = case["mod"], case["vc"], case["q"]
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.55, 0.0, 0.45], 0.2))
    sets = P.project_goals(mod, [q[:40], q[40:41], q[:0]], vc, [env, None, env])
    assert [g.shape[1] for g in sets] == [7, 7, 7] and len(sets[2]) == 0 and 0 < len(sets[0]) <= 40
    rows = np.concatenate(sets)
    assert mod.constraint_check_batch(rows, vc).all()
    assert mod.validate_batch(sets[0], env).all()
    keep = case["got"][2][:40] & mod.validate_batch(case["got"][0][:40], env)
    assert np.array_equal(bits(sets[0]), bits(case["got"][0][:40][keep]))  # the projection's rows, in order
    paths = [rows[:4], rows[4:6], rows[6:7], q[:3]]
    valid, band = P.validate_paths_constrained(mod, paths, [env, None, env, None], vc)
    for p, path in enumerate(paths):
        e = [env, None, env, None][p]
        assert valid[p] == bool(mod.validate_motion_batch(path[:-1], path[1:], e).all())
        assert band[p] == bool(mod.constraint_check_motion_batch(path[:-1], path[1:], vc).all())
    assert band[2] and valid[2] and not band[3]  # a single waypoint asks nothing; raw Halton rows are out of band
