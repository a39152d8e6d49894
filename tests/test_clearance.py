"""vmv_clearance_batch(_host), vmv_clearance_batch_multi(_host), <robot>.clearance* and planning.path_clearance: what
needs no device.  The argument checks run before any device query, so they hold on a CPU-only machine too."""
import ctypes

import numpy as np
import pytest

VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NO_DEVICE, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 1, 2, 5, 6
SYMBOLS = ("vmv_clearance_batch", "vmv_clearance_batch_host", "vmv_clearance_batch_multi", "vmv_clearance_batch_multi_host")
FILL = np.float32(-123.0)


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


def _single(_lib, env, robot=0, q=True, out=True, n=4):
    qa = np.zeros((n, 7), np.float32)
    values = np.full((n, 2), FILL, np.float32)
    wit = np.full((n, 4), 7, np.uint32)
    rc = _lib.lib.vmv_clearance_batch_host(robot, env, _fp(qa) if q else None, n, _fp(values) if out else None,
                                           wit.ctypes.data_as(_lib.c_u32_p))
    assert (values == FILL).all() and (wit == 7).all()  # a refused call writes nothing
    return rc, _lib.lib.vmv_last_error()


def _multi(_lib, handles, offsets, robot=0, q=True, out=True, host=True):
    qa = np.zeros((8, 7), np.float32)
    values = np.full((8, 2), FILL, np.float32)
    envs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    offs = np.ascontiguousarray(offsets, np.uint64)
    if host:
        rc = _lib.lib.vmv_clearance_batch_multi_host(robot, envs, offs.ctypes.data_as(_lib.c_size_p), len(handles),
                                                     _fp(qa) if q else None, _fp(values) if out else None, None)
    else:  # (the device entry point: refused before any pointer is used, so host addresses do for the test)
        rc = _lib.lib.vmv_clearance_batch_multi(robot, envs, offs.ctypes.data_as(_lib.c_size_p), len(handles),
                                                ctypes.c_void_p(qa.ctypes.data) if q else None,
                                                ctypes.c_void_p(values.ctypes.data) if out else None, None, None)
    assert (values == FILL).all()
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


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in names and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert vamp.abi_version() == 1  # additive


def test_single_refuses_null_arrays_and_unknown_robots(raw):
    _lib, make = raw
    for env in (None, make()):
        rc, msg = _single(_lib, env, q=False)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in msg
        rc, msg = _single(_lib, env, out=False)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in msg
        assert _single(_lib, env, robot=99)[0] == VMV_ERR_UNKNOWN_ROBOT
        assert _single(_lib, env, robot=-1)[0] == VMV_ERR_UNKNOWN_ROBOT
    qa, values = np.zeros((4, 7), np.float32), np.zeros((4, 2), np.float32)
    L = _lib.lib
    assert L.vmv_clearance_batch(0, None, None, 4, ctypes.c_void_p(values.ctypes.data), None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_clearance_batch(0, None, ctypes.c_void_p(qa.ctypes.data), 4, None, None, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_clearance_batch(99, None, ctypes.c_void_p(qa.ctypes.data), 4, ctypes.c_void_p(values.ctypes.data), None,
                                 None) == VMV_ERR_UNKNOWN_ROBOT


@pytest.mark.parametrize("kind, word", [("capt", b"CAPT"), ("mvt", b"MVT"), ("attach", b"attachment")])
def test_out_of_scope_kinds_are_refused_by_name(raw, kind, word):
    """a point cloud or an attachment: VMV_ERR_INVALID_ARGUMENT naming the kind, before the finalized check and the device"""
    _lib, make = raw
    h, plain = make(), make()
    _attach(_lib, h) if kind == "attach" else _add_cloud(_lib, h, kind)
    rc, msg = _single(_lib, h)
    assert rc == VMV_ERR_INVALID_ARGUMENT and word in msg, msg
    for host in (True, False):
        rc, msg = _multi(_lib, [plain, h], [0, 4, 8], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and word in msg and b"envs[1]" in msg, msg


def test_a_detached_environment_is_in_scope_again(raw):
    _lib, make = raw
    h = make()
    _attach(_lib, h)
    assert _lib.lib.vmv_env_detach(h) == 0
    assert _single(_lib, h)[0] == VMV_ERR_NOT_FINALIZED


def test_multi_refuses_null_handles_and_pointers(raw):
    _lib, make = raw
    a, b = make(), make()
    for host in (True, False):
        rc, msg = _multi(_lib, [a, None], [0, 4, 8], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"envs[1]" in msg
        rc, msg = _multi(_lib, [None, b], [0, 4, 8], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"envs[0]" in msg
        assert _multi(_lib, [a, b], [0, 4, 8], q=False, host=host)[0] == VMV_ERR_INVALID_ARGUMENT
        rc, msg = _multi(_lib, [a, b], [0, 4, 8], out=False, host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in msg
        assert _multi(_lib, [a, b], [0, 4, 8], robot=99, host=host)[0] == VMV_ERR_UNKNOWN_ROBOT
    offs = np.array([0, 4, 8], np.uint64)
    qa, values = np.zeros((8, 7), np.float32), np.zeros((8, 2), np.float32)
    L = _lib.lib
    assert L.vmv_clearance_batch_multi_host(0, None, offs.ctypes.data_as(_lib.c_size_p), 2, _fp(qa), _fp(values),
                                            None) == VMV_ERR_INVALID_ARGUMENT
    envs = (ctypes.c_void_p * 2)(a, b)
    assert L.vmv_clearance_batch_multi_host(0, envs, None, 2, _fp(qa), _fp(values), None) == VMV_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("offsets", [[1, 4, 8], [0, 5, 4], [0, 4, 3]])
def test_multi_refuses_bad_offsets(raw, offsets):
    _lib, make = raw
    assert _multi(_lib, [make(), make()], offsets)[0] == VMV_ERR_INVALID_ARGUMENT


def test_multi_refuses_counts_beyond_the_32_bit_limit(raw):
    """n >= 2^31 is refused before anything is read from q or allocated"""
    _lib, make = raw
    for host in (True, False):
        rc, msg = _multi(_lib, [make(), make()], [0, 1 << 30, 1 << 31], host=host)
        assert rc == VMV_ERR_INVALID_ARGUMENT and b"2^31" in msg


def test_unfinalized_environments_are_reported_without_a_device(raw):
    _lib, make = raw
    a, b = make(), make()
    rc, msg = _single(_lib, a)
    assert rc == VMV_ERR_NOT_FINALIZED and b"not finalized" in msg
    for host in (True, False):
        rc, msg = _multi(_lib, [a, b], [0, 3, 8], host=host)
        assert rc == VMV_ERR_NOT_FINALIZED and b"envs[0]" in msg


def test_empty_batches_need_no_device(raw):
    _lib, _ = raw
    values = np.zeros((1, 2), np.float32)
    qa = np.zeros((1, 7), np.float32)
    assert _lib.lib.vmv_clearance_batch_host(0, None, _fp(qa), 0, _fp(values), None) == 0
    offs = np.zeros(1, np.uint64)
    envs = (ctypes.c_void_p * 1)()
    assert _lib.lib.vmv_clearance_batch_multi_host(0, envs, offs.ctypes.data_as(_lib.c_size_p), 0, _fp(qa), _fp(values), None) == 0


def test_python_wrappers_check_shapes_and_types(vamp):
    panda = vamp.panda
    with pytest.raises(TypeError):
        panda.clearance_batch(np.zeros((4, 6), np.float32))
    with pytest.raises(TypeError):
        panda.clearance_batch(np.zeros(7, np.float32))
    with pytest.raises(TypeError):
        panda.clearance_batch(np.zeros((4, 7), np.float32), environment="scene")
    with pytest.raises(Exception):
        panda.clearance([0.0] * 6)
    with pytest.raises(TypeError):
        panda.clearance_batch_multi(np.zeros((4, 6), np.float32), [None], [4])
    with pytest.raises(ValueError):
        panda.clearance_batch_multi(np.zeros((4, 7), np.float32), [None], [3])  # counts do not sum to n
    with pytest.raises(ValueError):
        panda.clearance_batch_multi(np.zeros((4, 7), np.float32), [None, None], [4])  # one count per environment
    with pytest.raises(ValueError):
        panda.clearance_batch_multi(np.zeros((4, 7), np.float32), [None, None], [5, -1])
    with pytest.raises(TypeError):
        panda.clearance_batch_multi(np.zeros((4, 7), np.float32), ["scene"], [4])


def test_compute_fails_loudly_without_gpu(vamp):
    if vamp.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(vamp.VmvError) as ei:
        vamp.panda.clearance([0.0] * 7)
    assert ei.value.status == VMV_ERR_NO_DEVICE  # there is no CPU fallback
    with pytest.raises(vamp.VmvError) as ei:
        vamp.panda.clearance_batch(np.zeros((3, 7), np.float32), witness=True)
    assert ei.value.status == VMV_ERR_NO_DEVICE


# ---- path_clearance: the sampling rule and the bookkeeping, with clearance_batch_multi replaced by a numpy function ----
class _FakeRobot:
    """dimension 2; `env` clearance = q[0] - 10 * environment, `self` clearance = -q[1]; records its calls"""

    def __init__(self, resolution=4):
        self._res = resolution
        self.calls = []

    def dimension(self):
        return 2

    def resolution(self):
        return self._res

    def clearance_batch_multi(self, q, environments, counts, witness=False):
        q = np.asarray(q)
        assert q.dtype == np.float32 and q.ndim == 2 and sum(counts) == len(q)
        self.calls.append((q.copy(), list(environments), list(counts)))
        shift = np.repeat(np.array([10.0 * e for e in environments]), counts)
        return np.stack([q[:, 0] - shift, -q[:, 1]], axis=1).astype(np.float32)


def test_path_samples_follow_the_m_rule():
    from vamp_mvt_amd.planning import path_samples

    path = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.26], [1.0, 0.26], [1.0, 0.26 + 1e-9]])
    q, at = path_samples(path, 4)
    # |b - a| * 4 = 4 -> m = 4; 1.04 -> m = 2; 0 -> m = max(1, 0) = 1; 4e-9 -> m = 1
    ms = [4, 2, 1, 1]
    assert len(q) == sum(m + 1 for m in ms) and q.dtype == np.float32
    want_at = [(s, k) for s, m in enumerate(ms) for k in range(m + 1)]
    assert [tuple(r) for r in at] == want_at
    for (s, k), got in zip(want_at, q):
        a, b = path[s], path[s + 1]
        assert np.array_equal(got, (a + (b - a) * (k / ms[s])).astype(np.float32))  # float64 on the host, then cast
    # both end points of every segment are samples, bit for bit the waypoints
    for s, m in enumerate(ms):
        first = want_at.index((s, 0))
        assert np.array_equal(q[first], path[s].astype(np.float32)) and np.array_equal(q[first + m], path[s + 1].astype(np.float32))
    # an exact multiple does not round up; just above it does
    assert len(path_samples(np.array([[0.0, 0.0], [0.5, 0.0]]), 4)[0]) == 3
    assert len(path_samples(np.array([[0.0, 0.0], [0.5 + 1e-12, 0.0]]), 4)[0]) == 4
    one, at1 = path_samples(np.array([[0.3, 0.4]]), 4)
    assert one.shape == (1, 2) and [tuple(r) for r in at1] == [(0, 0)]


def test_path_clearance_makes_one_call_and_reports_where(vamp):
    from vamp_mvt_amd.planning import path_clearance

    robot = _FakeRobot(resolution=4)
    paths = [np.array([[0.5, 0.0], [0.25, 0.0], [0.25, 0.5]]),  # env min 0.25 first at (0, 1); self min -0.5 at (1, 2)
             np.array([[3.0, 1.0], [2.0, 0.0]]),                 # in environment 1: env min 2 - 10 at (0, m); self -1 at (0, 0)
             np.zeros((0, 2)),
             np.array([[7.0, 7.0]])]
    got = path_clearance(robot, paths, [0, 1, 0, 0])
    assert len(robot.calls) == 1  # ONE clearance_batch_multi call for all paths
    q, envs, counts = robot.calls[0]
    m1 = int(np.ceil(np.sqrt(2.0) * 4))
    assert envs == [0, 1, 0, 0] and counts == [2 + 3, m1 + 1, 0, 1]
    assert got[0].env == 0.25 and got[0].env_at == (0, 1) and got[0].self_ == -0.5 and got[0].self_at == (1, 2)
    assert got[1].env == -8.0 and got[1].env_at == (0, m1) and got[1].self_ == -1.0 and got[1].self_at == (0, 0)
    assert got[2].env == float("inf") and got[2].self_ == float("inf") and got[2].env_at is None and got[2].self_at is None
    assert got[3].env == 7.0 and got[3].env_at == (0, 0) and got[3].self_ == -7.0 and got[3].self_at == (0, 0)
    # resolution: the robot's by default, the caller's when given
    robot2 = _FakeRobot(resolution=4)
    path_clearance(robot2, paths[:1], [0], resolution=16)
    assert robot2.calls[0][2] == [4 + 1 + 8 + 1]
