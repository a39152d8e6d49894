"""vmv_eefk_jacobian_batch(_host), vmv_ik_batch(_host), <robot>.eefk_jacobian*, <robot>.ik_batch and planning.ik_goals: what
needs no device.  The generator's end-effector tangent tape against float64 finite differences, the generated text, the
symbols, every argument check (they run before any device query), ik_goals' bookkeeping on a fake robot, and the
condition the device tests rest on: in float64 (tests/ik_serial.py) every test target has at least 4 converged seeds."""
import ctypes

import numpy as np
import pytest

import clearance_grad_ref as ref
import ik_serial as K
from test_clearance_grad import TANGENT_BOUND  # 1e-6, derived there: float64 tangents against h = 1e-6 central differences

ROBOTS = K.ROBOTS
VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 2, 6
SYMBOLS = ("vmv_eefk_jacobian_batch", "vmv_eefk_jacobian_batch_host", "vmv_ik_batch", "vmv_ik_batch_host")
FILL = np.float32(-123.0)
MARK = np.uint32(0xabcdef01)


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_ee_tangent_tape_matches_float64_finite_differences(robot):
    g, m = ref.gen_hip(), ref.model(robot)
    dim = m["dimension"]
    em, tt = g.ee_model(m), g.ee_tangent_tape(m)
    q = ref.halton_q(m, 16)
    f, df = g.eval_tangent_tape(em, q, tt)
    assert f.shape == (16, 4, 3) and df.shape == (16, 4, 3, dim)
    assert np.array_equal(f, g.eval_tape(em, q))  # the primal values are the tape's
    s = ref.stencil(q)
    on = g.eval_tape(em, s.reshape(-1, dim)).reshape(16, 1 + 2 * dim, 4, 3)
    fd = np.moveaxis((on[:, 1::2] - on[:, 2::2]) / (2 * ref.H), 1, 3)  # [16][4][3][dim]
    worst = float(np.abs(fd - df).max())
    print(f"{robot}: ee tangent tape against central differences, largest deviation {worst:.3e}")
    assert worst <= TANGENT_BOUND
    structural = np.zeros((4, 3, dim), bool)
    for i in range(4):
        for k, (kind, v) in enumerate(em["outputs"][i]):
            if kind == "op":
                structural[i, k, tt["nz"][v]] = True
    # a structurally zero entry is exactly zero in both: the output does not read that joint at all
    assert (fd[:, ~structural] == 0.0).all() and (df[:, ~structural] == 0.0).all()
    mask = g.ee_joint_mask(m, tt)
    assert [bool(mask >> j & 1) for j in range(dim)] == structural.any(axis=(0, 1)).tolist()
    assert mask != 0 and (robot != "baxter" or bin(mask).count("1") == 7)  # one arm of Baxter moves its end effector


@pytest.mark.parametrize("robot", ROBOTS)
def test_ee_tangent_tape_shape(vamp, robot):
    """forms name only earlier ops and tangents that exist; sin and cos sit on joint inputs"""
    g, m = ref.gen_hip(), ref.model(robot)
    em, tt = g.ee_model(m), g.ee_tangent_tape(m)
    assert em["ops"] == m["ee_ops"] and [o for grp in em["outputs"] for o in grp] == m["ee_outputs"]
    for (i, j), f in tt["tan"].items():
        assert j in tt["nz"][i]
        if f[0] in ("cos", "nsin"):
            assert em["ops"][f[1]][0] == "in" and em["ops"][f[1]][1] == j
        elif f[0] in ("copy", "neg"):
            assert f[1] < i and (f[1], j) in tt["tan"]
        elif f[0] in ("add", "sub"):
            assert f[1] < i and f[2] < i and (f[1], j) in tt["tan"] and (f[2], j) in tt["tan"]
        elif f[0] == "cmul":
            assert f[2] < i and (f[2], j) in tt["tan"]
        elif f[0] == "mul":
            assert 1 <= len(f[1]) <= 2 and all(x < i and y < i and (x, j) in tt["tan"] for x, y in f[1])
        else:
            assert f == ("one",) and em["ops"][i] == ["in", j, None]
    text = "\n".join(g.emit_ee_frame_jac(m))
    assert f"{len(tt['ops'])} primal and {g.tangent_op_count(em, tt)} tangent operations" in text
    assert "asm" not in text and "atomic" not in text
    # every primal line of ee_frame_jac is a line of ee_frame: the frames are the same operations
    import self_gates

    robot_text = self_gates.generated_text(robot)
    start = robot_text.index("void ee_frame(")
    ee_frame = robot_text[start:robot_text.index("    }\n", start)]
    primal = [ln for ln in text.splitlines() if ln.startswith("        const float e")]
    assert len(primal) == len(tt["ops"]) and all(ln in ee_frame for ln in primal)


def test_refusal_rule_holds_for_the_ee_tape():
    g, m = ref.gen_hip(), ref.model("ur5")
    ops = [list(o) for o in m["ee_ops"]]
    i = next(k for k, o in enumerate(ops) if o[0] == "mul")
    ops.append(["sin", i, None])
    with pytest.raises(ValueError):
        g.tangent_tape(dict(g.ee_model(m), ops=ops, outputs=[[["op", len(ops) - 1]] * 3] * 4))


def test_generated_sources_hold_the_function(vamp):
    import self_gates

    for robot in ROBOTS:
        text = self_gates.generated_text(robot)
        assert text.count("void ee_frame_jac(") == 2  # the robot's function and its traits entry
        a, b, c = text.index("void ee_frame("), text.index("void ee_frame_jac("), text.index("fkcc_attach(")
        assert a < b < c  # directly behind ee_frame, in front of the attachment code
        assert "kEeJointMask" in text


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib

    declared = _lib.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and hasattr(_lib.lib, s)
        assert getattr(_lib.lib, s).argtypes is not None and getattr(_lib.lib, s).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.IkSettings) == 32
    d = vamp.IKSettings()
    assert (d.n_seeds, d.max_iterations, d.pos_tol, d.rot_tol, d.rot_weight, d.damping, d.max_step, d.position_only) == \
        (32, 64, 1e-4, 1e-3, 0.25, 1e-2, 0.5, False)
    k = K.Settings()
    assert vars(d) == {f: getattr(k, f) for f in vars(d)}  # the serial statement runs the same defaults


def _settings(_lib, **kw):
    base = dict(n_seeds=4, max_iterations=8, pos_tol=1e-4, rot_tol=1e-3, rot_weight=0.25, damping=1e-2, max_step=0.5, position_only=0)
    base.update(kw)
    return _lib.IkSettings(*[base[f] for f, _ in _lib.IkSettings._fields_])


def _ik(_lib, host, robot=0, targets=True, settings=True, q=True, status=True, err=True, seeds=False, n_targets=2, skip=0, **kw):
    """one refused (or empty) vmv_ik_batch(_host) call with outputs pre-filled -> (status, message); the outputs are untouched"""
    s = _settings(_lib, **kw)
    rows = 2 * 4
    T = np.zeros((2, 16), np.float32)
    S = np.zeros((rows, 7), np.float32)
    Q = np.full((rows, 7), FILL, np.float32)
    E = np.full((rows, 2), FILL, np.float32)
    st = np.full(rows, MARK, np.uint32)
    if host:
        fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
        rc = _lib.lib.vmv_ik_batch_host(robot, fp(T) if targets else None, n_targets, fp(S) if seeds else None, skip,
                                        ctypes.byref(s) if settings else None, fp(Q) if q else None, fp(E) if err else None,
                                        st.ctypes.data_as(_lib.c_u32_p) if status else None)
    else:  # (the device entry point: refused before any pointer is used, so host addresses do for the test)
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        rc = _lib.lib.vmv_ik_batch(robot, vp(T) if targets else None, n_targets, vp(S) if seeds else None, skip,
                                   ctypes.byref(s) if settings else None, vp(Q) if q else None, vp(E) if err else None,
                                   vp(st) if status else None, None)
    assert (Q == FILL).all() and (E == FILL).all() and (st == MARK).all()  # a refused call writes nothing
    return rc, _lib.lib.vmv_last_error().decode()


@pytest.mark.parametrize("host", [True, False])
def test_ik_argument_checks(vamp, host):
    from vamp_mvt_amd import _lib

    assert _ik(_lib, host, robot=99)[0] == VMV_ERR_UNKNOWN_ROBOT
    assert _ik(_lib, host, robot=-1, targets=False)[0] == VMV_ERR_UNKNOWN_ROBOT  # the robot wins over a NULL pointer
    for missing in ("targets", "settings", "q", "status"):
        assert _ik(_lib, host, **{missing: False}) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")
    assert _ik(_lib, host, targets=False, n_seeds=0) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")  # ... over the settings
    limits = [(dict(n_seeds=0), "n_seeds"), (dict(n_seeds=1025), "n_seeds"), (dict(max_iterations=0), "max_iterations"),
              (dict(max_iterations=1 << 30), "max_iterations"), (dict(position_only=2), "position_only"),
              (dict(position_only=-1), "position_only")]
    for field in ("pos_tol", "rot_tol", "rot_weight", "damping", "max_step"):
        limits += [({field: v}, field) for v in (0.0, -1.0, float("nan"), float("inf"))]
    for kw, name in limits:
        rc, msg = _ik(_lib, host, **kw)
        assert rc == VMV_ERR_INVALID_ARGUMENT and msg.startswith(name + " must be"), (kw, msg)
    # the settings are read in the struct's order, and before the Halton limit and the size
    assert _ik(_lib, host, n_seeds=0, pos_tol=0.0)[1].startswith("n_seeds")
    assert _ik(_lib, host, rot_tol=-1.0, max_step=0.0)[1].startswith("rot_tol")
    assert _ik(_lib, host, damping=0.0, skip=1000000, n_targets=1 << 31)[1].startswith("damping")
    # the Halton limit: halton_skip + n_seeds <= 1,000,000, only where the call makes the seeds
    assert _ik(_lib, host, skip=1000000 - 3) == (VMV_ERR_INVALID_ARGUMENT, "halton_skip + n_seeds must not exceed 1,000,000")
    assert _ik(_lib, host, skip=(1 << 64) - 1)[1].startswith("halton_skip")  # (no wrap-around)
    assert _ik(_lib, host, skip=1000000 - 3, n_targets=1 << 31)[1].startswith("halton_skip")  # ... before the size
    assert _ik(_lib, host, skip=1000000 - 4, n_targets=0) == (VMV_OK, _lib.lib.vmv_last_error().decode())
    assert _ik(_lib, host, skip=1 << 40, seeds=True, n_targets=0)[0] == VMV_OK  # the caller's seeds: no limit on the skip
    # n_targets * n_seeds below 2^31
    assert _ik(_lib, host, n_targets=(1 << 31) // 4) == (VMV_ERR_INVALID_ARGUMENT, "n_targets * n_seeds must be below 2^31")
    assert _ik(_lib, host, n_targets=(1 << 31) // 4, seeds=True)[1].startswith("n_targets * n_seeds")
    assert _ik(_lib, host, n_targets=1 << 62, n_seeds=1024)[0] == VMV_ERR_INVALID_ARGUMENT  # (no wrap-around)
    # an empty batch needs no device, and a NULL d_err is allowed; a refusal still wins over it
    assert _ik(_lib, host, n_targets=0)[0] == VMV_OK and _ik(_lib, host, n_targets=0, err=False)[0] == VMV_OK
    assert _ik(_lib, host, n_targets=0, n_seeds=0)[0] == VMV_ERR_INVALID_ARGUMENT
    assert _ik(_lib, host, n_targets=0, q=False)[0] == VMV_ERR_INVALID_ARGUMENT


def _jac(_lib, host, robot=0, q=True, frames=True, jac=True, n=3):
    qa = np.zeros((3, 7), np.float32)
    F = np.full((3, 16), FILL, np.float32)
    J = np.full((3, 6, 7), FILL, np.float32)
    if host:
        fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
        rc = _lib.lib.vmv_eefk_jacobian_batch_host(robot, fp(qa) if q else None, n, fp(F) if frames else None, fp(J) if jac else None)
    else:
        vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        rc = _lib.lib.vmv_eefk_jacobian_batch(robot, vp(qa) if q else None, n, vp(F) if frames else None, vp(J) if jac else None, None)
    assert (F == FILL).all() and (J == FILL).all()
    return rc, _lib.lib.vmv_last_error().decode()


@pytest.mark.parametrize("host", [True, False])
def test_jacobian_argument_checks(vamp, host):
    from vamp_mvt_amd import _lib

    assert _jac(_lib, host, robot=4)[0] == VMV_ERR_UNKNOWN_ROBOT and _jac(_lib, host, robot=-1, q=False)[0] == VMV_ERR_UNKNOWN_ROBOT
    assert _jac(_lib, host, q=False) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")
    assert _jac(_lib, host, jac=False) == (VMV_ERR_INVALID_ARGUMENT, "null pointer")
    assert _jac(_lib, host, jac=False, n=0)[0] == VMV_ERR_INVALID_ARGUMENT  # a NULL array wins over the empty batch
    assert _jac(_lib, host, n=0)[0] == VMV_OK and _jac(_lib, host, n=0, frames=False)[0] == VMV_OK


def test_wrapper_shape_errors(vamp):
    with pytest.raises(TypeError):
        vamp.panda.ik_batch(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(TypeError):
        vamp.panda.ik_batch(np.zeros((2, 4, 4), np.float32), seeds=np.zeros((2, 31, 7), np.float32))
    with pytest.raises(TypeError):
        vamp.panda.eefk_jacobian_batch(np.zeros((2, 6), np.float32))
    q, err, conv, its = vamp.panda.ik_batch(np.zeros((0, 4, 4), np.float32))  # an empty batch needs no device
    assert q.shape == (0, 32, 7) and err.shape == (0, 32, 2) and conv.shape == (0, 32) and its.shape == (0, 32)


# ---- planning.ik_goals -----------------------------------------------------------------------------------------------
class FakeRobot:
    """ik_batch returns a fixed table; validate_batch_multi calls every row whose first joint is negative invalid"""

    def __init__(self, q, converged):
        self.q, self.converged, self.calls = np.asarray(q, np.float32), np.asarray(converged, bool), []

    def dimension(self):
        return self.q.shape[2]

    def ik_batch(self, targets, seeds=None, halton_skip=0, settings=None):
        self.calls.append(("ik", len(targets), settings))
        return self.q, np.zeros(self.q.shape[:2] + (2,), np.float32), self.converged, np.zeros(self.q.shape[:2], np.int32)

    def validate_batch_multi(self, rows, environments, counts):
        self.calls.append(("validate", np.array(rows), list(environments), list(counts)))
        return np.asarray(rows)[:, 0] >= 0


def test_ik_goals_filters_deduplicates_and_reports(vamp):
    from vamp_mvt_amd import planning

    a, b, c = [0.1, 0.2], [0.5, 0.5], [1.0, 1.0]
    near_a, bad = [0.105, 0.195], [-0.3, 0.4]
    q = [[a, near_a, b, bad], [bad, c, c, a], [bad, a, b, c], [a, b, c, near_a]]
    conv = [[1, 1, 1, 1], [1, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    robot = FakeRobot(q, conv)
    envs = ["e0", "e1", "e2", "e3"]
    settings = object()
    goals, empty = planning.ik_goals(robot, np.zeros((4, 4, 4), np.float32), envs, settings=settings)
    assert [c[0] for c in robot.calls] == ["ik", "validate"] and robot.calls[0][2] is settings  # one call each
    _, rows, got_envs, counts = robot.calls[1]
    assert counts == [4, 3, 1, 0] and got_envs == envs  # converged rows only, target p in envs[p]
    assert np.array_equal(rows, np.array([a, near_a, b, bad, bad, c, c, bad], np.float32))
    assert [g.tolist() for g in goals[0]] == np.array([a, b], np.float32).tolist()  # near_a is within 1e-2 of a; bad collides
    assert [g.tolist() for g in goals[1]] == np.array([c], np.float32).tolist()      # the second c repeats the first
    assert empty == [2, 3] and all(g.shape == (0, 2) for g in goals[2:])
    assert all(g.dtype == np.float32 and g.ndim == 2 for g in goals)
    # seed order decides which of two close solutions stays; a smaller dedup keeps both
    goals, _ = planning.ik_goals(FakeRobot(q, conv), np.zeros((4, 16), np.float32), envs, dedup=1e-3)
    assert len(goals[0]) == 3
    # a single environment is broadcast
    one = FakeRobot(q, conv)
    planning.ik_goals(one, np.zeros((4, 4, 4), np.float32), "env")
    assert one.calls[1][2] == ["env"] * 4
    with pytest.raises(ValueError):
        planning.ik_goals(FakeRobot(q, conv), np.zeros((4, 4, 4), np.float32), envs[:3])
    # nothing converged: no validation call, every target reported
    none = FakeRobot(q, np.zeros((4, 4), bool))
    goals, empty = planning.ik_goals(none, np.zeros((4, 4, 4), np.float32), envs)
    assert [c[0] for c in none.calls] == ["ik"] and empty == [0, 1, 2, 3]


# ---- the condition the device tests rest on ------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_every_device_test_target_has_four_converged_seeds_in_float64(robot):
    """Targets: the frames of Halton configurations TARGET_SKIP + 1 .. + 33 (ik_serial.py says why the UR5's are not the
    first 33); seeds: Halton samples SEED_SKIP + 1 .. + 32; the default settings.  With 8 seeds no robot meets the 4, so the
    device round trip runs 32."""
    s = K.Settings()
    cfg = K.target_configs(robot)
    lo, hi = K.bounds(robot)
    assert ((cfg >= lo) & (cfg <= hi)).all()
    T, S = K.lanes(K.frames44(robot, cfg.astype(np.float64)), K.halton32(robot, s.n_seeds, K.SEED_SKIP))
    r = K.solve(robot, T, S, s)
    per_target = r["converged"].reshape(K.N_TARGETS, s.n_seeds).sum(axis=1)
    print(f"{robot}: converged seeds per target min {per_target.min()} mean {per_target.mean():.1f}; "
          f"mean evaluations {r['iterations'].mean():.1f}")
    assert per_target.min() >= K.MIN_CONVERGED
    # the statement keeps its own promises: never worse than the seed, inside the bounds, converged rows within tolerance
    assert (r["E"] <= r["E_seed"]).all() and ((r["q"] >= lo) & (r["q"] <= hi)).all()
    n_p, n_w, tr = K.residuals(robot, r["q"], T)
    c = r["converged"]
    assert (n_p[c] <= s.pos_tol).all() and (n_w[c] <= s.rot_tol).all() and (tr[c] > 1.0).all()
    assert (r["iterations"][~c] == s.max_iterations).all()
