"""vmv_clearance_grad_batch(_host), vmv_clearance_grad_batch_multi(_host), <robot>.clearance_grad* and planning.push_out:
what needs no device.  The generator's tangent tape against float64 finite differences, the argument checks (they run
before any device query), the wrappers' shape and type errors, push_out's bookkeeping on a fake robot, and the kink rule
of the device test held against its cap with a float64 witness."""
import ctypes

import numpy as np
import pytest

import clearance_grad_ref as ref

ROBOTS = ("panda", "ur5", "fetch", "baxter")
VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 1, 2, 5, 6
SYMBOLS = ("vmv_clearance_grad_batch", "vmv_clearance_grad_batch_host", "vmv_clearance_grad_batch_multi",
           "vmv_clearance_grad_batch_multi_host")
FILL = np.float32(-123.0)
# Tangent tape against central differences of eval_tape, both float64, h = 1e-6: the quotient's truncation is h^2 / 6 times
# a third derivative of order 1 m (1e-13) and its rounding 1e-16 * 1 m / h = 1e-10, so 1e-6 leaves four orders; a wrong
# rule or a dropped tangent shows at the size of a lever arm, 1e-2 or more.  Derived, not measured.
TANGENT_BOUND = 1e-6


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_tangent_tape_matches_float64_finite_differences(robot):
    g, m = ref.gen_hip(), ref.model(robot)
    ns, dim = m["n_spheres"], m["dimension"]
    q = ref.halton_q(m, 16)
    tt = g.tangent_tape(m)
    c, jac = g.eval_tangent_tape(m, q, tt)
    assert c.shape == (16, ns, 3) and jac.shape == (16, ns, 3, dim)
    assert np.array_equal(c, g.eval_tape(m, q)[:, :ns])  # the primal values are the tape's
    on = ref.centres_on_stencil(robot, q)  # [16][1 + 2 dim][spheres][3]
    fd = (on[:, 1::2] - on[:, 2::2]) / (2 * ref.H)  # [16][dim][spheres][3]
    fd = np.moveaxis(fd, 1, 3)
    worst = float(np.abs(fd - jac).max())
    print(f"{robot}: tangent tape against central differences, largest deviation {worst:.3e}")
    assert worst <= TANGENT_BOUND
    # every tangent the function calls structurally zero is zero in the finite difference (exactly: the coordinate does
    # not read that joint at all)
    structural = np.zeros((ns, 3, dim), bool)
    for s in range(ns):
        for k, (kind, v) in enumerate(m["outputs"][s]):
            if kind == "op":
                structural[s, k, tt["nz"][v]] = True
    assert (fd[:, ~structural] == 0.0).all() and (jac[:, ~structural] == 0.0).all()
    assert structural.any(axis=(0, 1)).all()  # every joint moves some sphere


@pytest.mark.parametrize("robot", ROBOTS)
def test_tangent_tape_shape(robot):
    """forms name only earlier ops and tangents that exist; sin and cos sit on joint inputs; the counts are the ones the
    generated header comment states"""
    g, m = ref.gen_hip(), ref.model(robot)
    tt = g.tangent_tape(m)
    for (i, j), f in tt["tan"].items():
        assert j in tt["nz"][i]
        if f[0] in ("cos", "nsin"):
            assert m["ops"][f[1]][0] == "in" and m["ops"][f[1]][1] == j
        elif f[0] in ("copy", "neg"):
            assert f[1] < i and (f[1], j) in tt["tan"]
        elif f[0] in ("add", "sub"):
            assert f[1] < i and f[2] < i and (f[1], j) in tt["tan"] and (f[2], j) in tt["tan"]
        elif f[0] == "cmul":
            assert f[2] < i and (f[2], j) in tt["tan"]
        elif f[0] == "mul":
            assert 1 <= len(f[1]) <= 2 and all(x < i and y < i and (x, j) in tt["tan"] for x, y in f[1])
        else:
            assert f == ("one",) and m["ops"][i] == ["in", j, None]
    text = "\n".join(g.emit_sphere_fk_grad(m))
    assert f"{len(tt['ops'])} primal and {g.tangent_op_count(m, tt)} tangent operations" in text
    assert "asm" not in text and "atomic" not in text


def test_generated_sources_expose_the_function(vamp):
    import self_gates

    for robot in ROBOTS:
        text = self_gates.generated_text(robot)
        assert text.count("void sphere_fk_grad(") == 2  # the robot's function and its traits entry
        assert text.index("void sphere_fk(") < text.index("void sphere_fk_grad(")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
@pytest.fixture()
def raw(vamp):
    """-> (_lib, make): make() creates an unfinalized C environment (no device needed); all destroyed afterwards"""
    from vamp_mvt_amd import _lib

    handles = []

    def make():
        h = ctypes.c_void_p()
        assert _lib.lib.vmv_env_create(ctypes.byref(h)) == 0
        handles.append(h.value)
        return h.value

    yield _lib, make
    for h in handles:
        _lib.lib.vmv_env_destroy(h)


def _fp(a):
    from vamp_mvt_amd import _lib

    return a.ctypes.data_as(_lib.c_float_p)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _single(_lib, env, robot=0, q=True, out=True, grad=True, n=4, host=True):
    qa = np.zeros((n, 7), np.float32)
    values = np.full((n, 2), FILL, np.float32)
    g = np.full((n, 2, 7), FILL, np.float32)
    wit = np.full((n, 4), 7, np.uint32)
    if host:
        rc = _lib.lib.vmv_clearance_grad_batch_host(robot, env, _fp(qa) if q else None, n, _fp(values) if out else None,
                                                    _fp(g) if grad else None, wit.ctypes.data_as(_lib.c_u32_p))
    else:  # (the device entry point: refused before any pointer is used, so host addresses do for the test)
        rc = _lib.lib.vmv_clearance_grad_batch(robot, env, _vp(qa) if q else None, n, _vp(values) if out else None,
                                               _vp(g) if grad else None, _vp(wit), None)
    assert (values == FILL).all() and (g == FILL).all() and (wit == 7).all()  # a refused call writes nothing
    return rc, _lib.lib.vmv_last_error()


def _multi(_lib, handles, offsets, robot=0, q=True, out=True, grad=True, host=True):
    qa = np.zeros((8, 7), np.float32)
    values = np.full((8, 2), FILL, np.float32)
    g = np.full((8, 2, 7), FILL, np.float32)
    envs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    offs = np.ascontiguousarray(offsets, np.uint64)
    if host:
        rc = _lib.lib.vmv_clearance_grad_batch_multi_host(robot, envs, offs.ctypes.data_as(_lib.c_size_p), len(handles),
                                                          _fp(qa) if q else None, _fp(values) if out else None,
                                                          _fp(g) if grad else None, None)
    else:
        rc = _lib.lib.vmv_clearance_grad_batch_multi(robot, envs, offs.ctypes.data_as(_lib.c_size_p), len(handles),
                                                     _vp(qa) if q else None, _vp(values) if out else None,
                                                     _vp(g) if grad else None, None, None)
    assert (values == FILL).all() and (g == FILL).all()
    return rc, _lib.lib.vmv_last_error()


def _add_cloud(_lib, h, kind):
    pts = np.random.default_rng(3).uniform(0.3, 0.9, (64, 3)).astype(np.float32)
    if kind == "capt":
        rc = _lib.lib.vmv_env_add_capt_pointcloud(h, _fp(pts), len(pts), 0.01, 0.1, 0.005, None)
    else:
        lo, hi = np.full(3, -2.0, np.float32), np.full(3, 2.0, np.float32)
        rc = _lib.lib.vmv_env_add_mvt_pointcloud(h, _fp(pts), len(pts), 0.01, 0.1, _fp(lo), _fp(hi), 0.005, None, None)
    assert rc == 0, _lib.lib.vmv_last_error()


def _attach(_lib, h):
    tf = np.eye(4, dtype=np.float32)
    sp = np.array([[0, 0, 0.1, 0.03]], np.float32)
    assert _lib.lib.vmv_env_attach(h, _fp(tf), _fp(sp), 1) == 0


def test_symbols_are_declared_exported_and_bound(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in names and hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and getattr(_lib.lib, name).argtypes
    assert vamp.abi_version() == 1  # additive


def test_single_refuses_null_arrays_and_unknown_robots(raw):
    _lib, make = raw
    for host in (True, False):
        for env in (None, make()):
            for missing in ("q", "out", "grad"):
                rc, msg = _single(_lib, env, host=host, **{missing: False})
                assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in msg, (host, missing)
            assert _single(_lib, env, robot=99, host=host)[0] == VMV_ERR_UNKNOWN_ROBOT
            assert _single(_lib, env, robot=-1, host=host)[0] == VMV_ERR_UNKNOWN_ROBOT


@pytest.mark.parametrize("kind, word", [("capt", b"CAPT"), ("mvt", b"MVT"), ("attach", b"attachment")])
def test_out_of_scope_kinds_are_refused_by_name(raw, kind, word):
    _lib, make = raw
    h, plain = make(), make()
    _attach(_lib, h) if kind == "attach" else _add_cloud(_lib, h, kind)
    for host in (True, False):
        rc, msg = _single(_lib, h, host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and word in msg, msg
        rc, msg = _multi(_lib, [plain, h], [0, 4, 8], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and word in msg and b"envs[1]" in msg, msg


def test_multi_refuses_null_handles_pointers_and_bad_offsets(raw):
    _lib, make = raw
    a, b = make(), make()
    for host in (True, False):
        rc, msg = _multi(_lib, [a, None], [0, 4, 8], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"envs[1]" in msg
        for missing in ("q", "out", "grad"):
            rc, msg = _multi(_lib, [a, b], [0, 4, 8], host=host, **{missing: False})
            assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in msg, (host, missing)
        assert _multi(_lib, [a, b], [0, 4, 8], robot=99, host=host)[0] == VMV_ERR_UNKNOWN_ROBOT
        for offsets in ([1, 4, 8], [0, 5, 4], [0, 4, 3]):
            assert _multi(_lib, [a, b], offsets, host=host)[0] == VMV_ERR_INVALID_ARGUMENT
        # n >= 2^31 is refused before anything is read from q or allocated
        rc, msg = _multi(_lib, [a, b], [0, 1 << 30, 1 << 31], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"2^31" in msg


def test_unfinalized_environments_are_reported_without_a_device(raw):
    _lib, make = raw
    a, b = make(), make()
    for host in (True, False):
        rc, msg = _single(_lib, a, host=host)
        assert rc == VMV_ERR_NOT_FINALIZED and b"not finalized" in msg
        rc, msg = _multi(_lib, [a, b], [0, 3, 8], host=host)
        assert rc == VMV_ERR_NOT_FINALIZED and b"envs[0]" in msg


def test_empty_batches_need_no_device(raw):
    _lib, _ = raw
    values, g, qa = np.zeros((1, 2), np.float32), np.zeros((1, 2, 7), np.float32), np.zeros((1, 7), np.float32)
    L = _lib.lib
    assert L.vmv_clearance_grad_batch_host(0, None, _fp(qa), 0, _fp(values), _fp(g), None) == 0
    assert L.vmv_clearance_grad_batch(0, None, _vp(qa), 0, _vp(values), _vp(g), None, None) == 0
    offs = np.zeros(1, np.uint64)
    envs = (ctypes.c_void_p * 1)()
    assert L.vmv_clearance_grad_batch_multi_host(0, envs, offs.ctypes.data_as(_lib.c_size_p), 0, _fp(qa), _fp(values), _fp(g),
                                                 None) == 0
    assert L.vmv_clearance_grad_batch_multi(0, envs, offs.ctypes.data_as(_lib.c_size_p), 0, _vp(qa), _vp(values), _vp(g), None,
                                            None) == 0


# ---- the Python wrappers ---------------------------------------------------------------------------------------------
def test_python_wrappers_check_shapes_and_types(vamp):
    panda = vamp.panda
    with pytest.raises(TypeError):
        panda.clearance_grad_batch(np.zeros((4, 6), np.float32))
    with pytest.raises(TypeError):
        panda.clearance_grad_batch(np.zeros(7, np.float32))
    with pytest.raises(TypeError):
        panda.clearance_grad_batch(np.zeros((4, 7), np.float32), environment="scene")
    with pytest.raises(Exception):
        panda.clearance_grad([0.0] * 6)
    with pytest.raises(TypeError):
        panda.clearance_grad_batch_multi(np.zeros((4, 6), np.float32), [None], [4])
    with pytest.raises(ValueError):
        panda.clearance_grad_batch_multi(np.zeros((4, 7), np.float32), [None], [3])  # counts do not sum to n
    with pytest.raises(ValueError):
        panda.clearance_grad_batch_multi(np.zeros((4, 7), np.float32), [None, None], [4])  # one count per environment
    with pytest.raises(ValueError):
        panda.clearance_grad_batch_multi(np.zeros((4, 7), np.float32), [None, None], [5, -1])
    with pytest.raises(TypeError):
        panda.clearance_grad_batch_multi(np.zeros((4, 7), np.float32), ["scene"], [4])
    # empty batches come back empty, with the right shapes, without a device
    values, grad, wit = panda.clearance_grad_batch(np.zeros((0, 7), np.float32), witness=True)
    assert values.shape == (0, 2) and grad.shape == (0, 2, 7) and wit.shape == (0, 4)


def test_compute_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    for call in (lambda: vamp.panda.clearance_grad([0.0] * 7),
                 lambda: vamp.panda.clearance_grad_batch(np.zeros((3, 7), np.float32), witness=True),
                 lambda: vamp.panda.clearance_grad_batch_multi(np.zeros((3, 7), np.float32), [None], [3])):
        with pytest.raises(vamp.VmvError) as ei:
            call()
        assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback


# ---- push_out: the bookkeeping, with clearance_grad_batch replaced by analytic functions ---------------------------------
class _FakeRobot:
    """dimension 2, bounds [-1, 1]^2.  `env` clearance = fn(q) with its gradient, `self` clearance = +1 with gradient 0;
    records the batch of every call"""

    def __init__(self, fn):
        self.fn = fn
        self.calls = []

    def dimension(self):
        return 2

    def lower_bounds(self):
        return np.array([-1.0, -1.0], np.float32)

    def upper_bounds(self):
        return np.array([1.0, 1.0], np.float32)

    def clearance_grad_batch(self, q, environment=None, witness=False):
        q = np.asarray(q)
        assert q.dtype == np.float32 and q.ndim == 2 and q.shape[1] == 2 and len(q) > 0
        self.calls.append(q.copy())
        v, g = self.fn(q)
        values = np.stack([v, np.ones(len(q))], axis=1).astype(np.float32)
        grad = np.stack([g, np.zeros_like(g)], axis=1).astype(np.float32)
        return values, grad


def _plane(q):  # env = q0 - 0.5: a wall at q0 = 0.5, unit gradient
    return q[:, 0] - 0.5, np.stack([np.ones(len(q)), np.zeros(len(q))], axis=1)


MARGIN, MAX_STEP = 2.0 ** -6, 2.0 ** -4  # (binary fractions: the Newton step of the plane is exact in float32)


def test_push_out_steps_once_per_call_and_drops_what_has_reached():
    from vamp_mvt_amd.planning import push_out

    robot = _FakeRobot(_plane)
    q = np.array([[0.8, 0.0],                  # clear from the start: one evaluation, never moved
                  [0.5 + 2.0 ** -7, 0.125],    # half the margin short: one exact Newton step
                  [0.25, 0.25],                # 0.266 short: four steps of max_step, then a Newton step
                  [0.7, 0.375]], np.float32)
    out = push_out(robot, q, None, margin=MARGIN, max_steps=32, max_step=MAX_STEP)
    assert out.reached.all() and out.configurations.dtype == np.float32 and out.clearances.dtype == np.float32
    assert np.array_equal(out.configurations[[0, 3]], q[[0, 3]])
    assert out.calls == len(robot.calls)
    # one call per step, and a call asks about exactly the configurations the call before left below the margin, in order
    assert np.array_equal(robot.calls[0], q)
    for before, after in zip(robot.calls, robot.calls[1:]):
        short = _plane(before)[0].astype(np.float32) < np.float32(MARGIN)
        assert np.array_equal(after[:, 1], before[short, 1])
    assert [len(c) for c in robot.calls[:3]] == [4, 2, 1] and 6 <= len(robot.calls) <= 7
    assert out.configurations[1, 0] == np.float32(0.5 + 2.0 ** -6)  # the Newton step, exactly
    # the step cap: configuration 2 moves by max_step along the gradient, and only along it
    track = [c[c[:, 1] == np.float32(0.25)] for c in robot.calls]
    assert all(len(t) == 1 for t in track)  # (asked about in every call, and its second joint never moves)
    assert np.allclose(np.diff([t[0, 0] for t in track[:5]]), MAX_STEP, atol=1e-6)
    # the returned clearances are the fake's values at the returned configurations
    v = (out.configurations[:, 0] - np.float32(0.5)).astype(np.float32)
    assert np.array_equal(out.clearances[:, 0], v) and (out.clearances[:, 0] >= np.float32(MARGIN)).all()


def test_push_out_stops_after_max_steps_and_clips_to_the_bounds():
    from vamp_mvt_amd.planning import push_out

    robot = _FakeRobot(_plane)
    out = push_out(robot, np.array([[-0.9, 0.0]], np.float32), None, margin=MARGIN, max_steps=3, max_step=MAX_STEP)
    assert out.calls == 4 and not out.reached[0]  # the input and one evaluation after each of the three steps
    assert abs(float(out.configurations[0, 0]) - (-0.9 + 3 * MAX_STEP)) < 1e-5  # the best seen is the last
    assert np.array_equal(out.clearances[0], np.array([out.configurations[0, 0] - np.float32(0.5), 1.0], np.float32))
    # a wall behind the upper bound: the steps are clipped to q0 = 1 and the margin is never reached
    far = _FakeRobot(lambda q: (q[:, 0] - 1.005, np.stack([np.ones(len(q)), np.zeros(len(q))], axis=1)))
    out = push_out(far, np.array([[0.98, 0.0]], np.float32), None, margin=0.01, max_steps=4, max_step=0.05)
    assert not out.reached[0] and out.configurations[0, 0] == np.float32(1.0) and (np.concatenate(far.calls) <= 1.0).all()
    assert out.calls == 5
    with pytest.raises(TypeError):
        push_out(robot, np.zeros((3, 3), np.float32))
    empty = push_out(robot, np.zeros((0, 2), np.float32))
    assert empty.calls == 0 and empty.configurations.shape == (0, 2) and empty.reached.shape == (0,)


def test_push_out_keeps_the_best_seen_when_a_step_overshoots():
    from vamp_mvt_amd.planning import push_out

    def ridge(q):  # a narrow ridge at q0 = 0: the first-order step from its flank lands far down the other side
        x = q[:, 0].astype(np.float64)
        v = np.where(x < 0, 0.004 + 0.1 * x, 0.004 - 1.0 * x)
        g = np.where(x < 0, 0.1, -1.0)
        return v, np.stack([g, np.zeros(len(q))], axis=1)

    robot = _FakeRobot(ridge)
    q = np.array([[-0.01, 0.0]], np.float32)  # value 0.003; the step is +0.05 (capped), to value -0.036
    out = push_out(robot, q, None, margin=0.01, max_steps=1, max_step=0.05)
    assert out.calls == 2 and robot.calls[1][0, 0] > 0.03
    assert np.array_equal(out.configurations, q) and not out.reached[0]
    assert out.clearances[0, 0] == np.float32(ridge(q)[0][0])
    # with more steps it may wander, but what it returns is never worse than the input
    out = push_out(_FakeRobot(ridge), q, None, margin=0.01, max_steps=8, max_step=0.05)
    assert out.clearances.min(axis=1)[0] >= np.float32(0.003)


def test_push_out_leaves_zero_gradients_and_nan_values_where_they_are():
    from vamp_mvt_amd.planning import push_out

    def flat(q):  # a zero gradient in contact for q1 > 0 (a centre inside a box), NaN for q1 < 0, a wall otherwise
        v, g = _plane(q)
        v = np.where(q[:, 1] > 0, -0.02, np.where(q[:, 1] < 0, np.nan, v))
        g = np.where((q[:, 1] != 0)[:, None], 0.0, g)
        return v, g

    robot = _FakeRobot(flat)
    q = np.array([[0.2, 0.5], [0.2, -0.5], [0.5 + 2.0 ** -7, 0.0]], np.float32)
    out = push_out(robot, q, None, margin=MARGIN, max_steps=5, max_step=MAX_STEP)
    assert list(out.reached) == [False, False, True] and out.calls == 2
    assert [len(c) for c in robot.calls] == [3, 1]  # the two stalled ones are not asked about again
    assert np.array_equal(out.configurations[:2], q[:2])
    assert out.clearances[0, 0] == np.float32(-0.02) and np.isnan(out.clearances[1, 0])


# ---- the kink rule of the device test, held against its cap on the CPU ---------------------------------------------------
@pytest.mark.parametrize("kind", ["six", "many"])
@pytest.mark.parametrize("robot", ROBOTS)
def test_kinks_stay_within_the_cap_for_the_device_tests_seeds(robot, kind):
    """The device test may leave out a case whose fixed witness has a kink within h of q, at most 1 % per (robot, scene).
    Here the witness is the float64 minimiser (the device's differs from it only at near ties), at the same 257 Halton
    configurations and in the same scenes."""
    import test_clearance_grad_gpu as gpu_tests

    spec = gpu_tests.scene(robot, kind)
    q = gpu_tests.configurations(robot).astype(np.float64)
    env_w, self_w, pairs = ref.float64_witness(robot, spec, q)
    qe, qs = ref.witness_quotients(robot, q, env_w, self_w, pairs)
    left_out = int(ref.kinks(qe).sum() + ref.kinks(qs).sum())
    cases = 2 * q.size
    print(f"{robot} {kind}: {left_out} of {cases} cases have a kink within h")
    assert left_out <= ref.KINK_CAP * cases
