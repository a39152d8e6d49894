"""vmv_validate_motion_batch_multi(_host) / <robot>.validate_motion_batch_multi: the checks that need no device (they run
before any device query, so they hold on a CPU-only machine too)."""
import ctypes

import numpy as np
import pytest

VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 1, 5, 6
FILL = np.uint64(0x5A5A5A5A5A5A5A5A)
NAMES = ("vmv_validate_motion_batch_multi", "vmv_validate_motion_batch_multi_host")


@pytest.fixture()
def raw(vamp):
    """two created, unfinalized C environments (no device needed), destroyed afterwards"""
    from vamp_mvt_amd import _lib

    handles = []
    for _ in range(2):
        h = ctypes.c_void_p()
        assert _lib.lib.vmv_env_create(ctypes.byref(h)) == 0
        handles.append(h.value)
    yield _lib, handles
    for h in handles:
        _lib.lib.vmv_env_destroy(h)


def _host_call(_lib, handles, offsets, robot=0, n_rows=8, n_envs=None, drop=()):
    """one vmv_validate_motion_batch_multi_host call; `drop` names the pointers passed as NULL"""
    a = np.zeros((n_rows, 7), np.float32)
    b = np.full((n_rows, 7), 0.5, np.float32)
    bits = np.full(1, FILL, np.uint64)
    envs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    offs = np.ascontiguousarray(offsets, np.uint64)
    ptr = {"envs": envs, "offsets": offs.ctypes.data_as(_lib.c_size_p), "start": a.ctypes.data_as(_lib.c_float_p),
           "goal": b.ctypes.data_as(_lib.c_float_p), "bits": bits.ctypes.data_as(_lib.c_u64_p)}
    for k in drop:
        ptr[k] = None
    rc = _lib.lib.vmv_validate_motion_batch_multi_host(robot, ptr["envs"], ptr["offsets"],
                                                       len(handles) if n_envs is None else n_envs, ptr["start"],
                                                       ptr["goal"], ptr["bits"])
    return rc, bits


def test_motion_multi_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    for name in NAMES:
        assert name in names and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert vamp.abi_version() == 1  # the change is additive


@pytest.mark.parametrize("offsets", [[1, 4, 8], [0, 5, 4], [0, 9, 8], [0, 4, 3]])
def test_host_rejects_bad_offsets(raw, offsets):
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, offsets)
    assert rc == VMV_ERR_INVALID_ARGUMENT, _lib.lib.vmv_last_error()
    assert (bits == FILL).all()  # nothing written


@pytest.mark.parametrize("drop", ["envs", "offsets", "start", "goal", "bits"])
def test_host_rejects_null_pointers(raw, drop):
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, [0, 4, 8], drop=(drop,))
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"null pointer" in _lib.lib.vmv_last_error()
    assert (bits == FILL).all()


def test_host_rejects_null_handles(raw):
    _lib, handles = raw
    rc, bits = _host_call(_lib, [handles[0], None], [0, 4, 8])
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"envs[1]" in _lib.lib.vmv_last_error()
    assert (bits == FILL).all()


def test_device_entry_checks_its_pointers_without_a_device(raw):
    _lib, handles = raw
    offs = np.array([0, 4, 8], np.uint64)
    envs = (ctypes.c_void_p * 2)(*handles)
    buf = ctypes.c_void_p(1)  # never dereferenced: the NULL checks come first
    L, sp = _lib.lib, _lib.c_size_p
    for start, goal, bits in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert L.vmv_validate_motion_batch_multi(0, envs, offs.ctypes.data_as(sp), 2, start, goal, bits,
                                                 None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_validate_motion_batch_multi(0, None, offs.ctypes.data_as(sp), 2, buf, buf, buf,
                                             None) == VMV_ERR_INVALID_ARGUMENT
    # unfinalized environments are reported before any device query, by the device entry point too
    assert L.vmv_validate_motion_batch_multi(0, envs, offs.ctypes.data_as(sp), 2, buf, buf, buf,
                                             None) == VMV_ERR_NOT_FINALIZED


def test_host_rejects_batches_beyond_the_32_bit_limit(raw):
    """the kernels count in 32 bits: n >= 2^31 or n_envs >= 2^31 is refused before anything is read or allocated"""
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, [0, 1 << 30, 1 << 31])
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"2^31" in _lib.lib.vmv_last_error()
    assert (bits == FILL).all()
    rc, bits = _host_call(_lib, handles, [0, 4, 8], n_envs=1 << 31)  # (offsets[n_envs] is never read)
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"n_envs" in _lib.lib.vmv_last_error()
    assert (bits == FILL).all()


def test_host_reports_unfinalized_environments_and_unknown_robots_without_a_device(raw):
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, [0, 3, 8])
    assert rc == VMV_ERR_NOT_FINALIZED and b"not finalized" in _lib.lib.vmv_last_error()
    assert (bits == FILL).all()
    # empty segments and repeated handles are allowed, and are checked all the same
    rc, _ = _host_call(_lib, [handles[0], handles[0], handles[1]], [0, 0, 8, 8])
    assert rc == VMV_ERR_NOT_FINALIZED
    rc, bits = _host_call(_lib, handles, [0, 4, 8], robot=7)
    assert rc == VMV_ERR_UNKNOWN_ROBOT
    assert (bits == FILL).all()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library called: {name}")


def test_python_checks_counts_and_shapes_before_any_library_call(vamp, monkeypatch):
    a = np.zeros((10, 7), np.float32)
    b = np.ones((10, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    f = vamp.panda.validate_motion_batch_multi
    with pytest.raises(ValueError):
        f(a, b, [env, None], [4, 5])  # counts sum to 9
    with pytest.raises(ValueError):
        f(a, b, [env, None], [10])  # one count for two environments
    with pytest.raises(ValueError):
        f(a, b, [env, None], [12, -2])
    with pytest.raises(ValueError):
        f(a, b, [env], [[10]])
    with pytest.raises(ValueError):
        f(a, b, [env], [10.0])
    with pytest.raises(TypeError):
        f(a, b[:9], [env], [10])  # starts and goals of different shapes
    with pytest.raises(TypeError):
        f(np.zeros((10, 6), np.float32), np.zeros((10, 6), np.float32), [env], [10])  # wrong dimension
    with pytest.raises(TypeError):
        f(a[:, None, :], b[:, None, :], [env], [10])
    with pytest.raises(TypeError):
        f(a, b, ["not an environment"], [10])
    with pytest.raises(TypeError):
        f(a, b, [env, 3], [5, 5])
    assert env._handle is None  # nothing was built or finalized


def test_validate_paths_checks_its_arguments_before_any_library_call(vamp, monkeypatch):
    from vamp_mvt_amd import planning

    env = vamp.Environment()
    monkeypatch.setattr(vamp, "lib", _NoLibrary())
    path = [np.zeros(7, np.float32), np.ones(7, np.float32)]
    with pytest.raises(ValueError):
        planning.validate_paths(vamp.panda, [path, path], [env])  # one environment for two paths
    with pytest.raises(TypeError):
        planning.validate_paths(vamp.panda, [path], ["not an environment"])
    assert env._handle is None
