"""vmv_validate_batch_multi(_host) / <robot>.validate_batch_multi: the checks that need no device (they run before any
device query, so they hold on a CPU-only machine too)."""
import ctypes

import numpy as np
import pytest

VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 1, 5, 6


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


def _host_call(_lib, handles, offsets, robot=0, n_rows=8, bits_words=1):
    q = np.zeros((n_rows, 7), np.float32)
    bits = np.full(bits_words, 0x5A5A5A5A5A5A5A5A, np.uint64)
    envs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    offs = np.ascontiguousarray(offsets, np.uint64)
    rc = _lib.lib.vmv_validate_batch_multi_host(robot, envs, offs.ctypes.data_as(_lib.c_size_p), len(handles),
                                                q.ctypes.data_as(_lib.c_float_p), bits.ctypes.data_as(_lib.c_u64_p))
    return rc, bits


def test_multi_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    for name in ("vmv_validate_batch_multi", "vmv_validate_batch_multi_host"):
        assert name in names and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert vamp.abi_version() == 1  # the change is additive


@pytest.mark.parametrize("offsets", [[1, 4, 8], [0, 5, 4], [0, 9, 8], [0, 4, 3]])
def test_host_rejects_bad_offsets(raw, offsets):
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, offsets)
    assert rc == VMV_ERR_INVALID_ARGUMENT, _lib.lib.vmv_last_error()
    assert (bits == np.uint64(0x5A5A5A5A5A5A5A5A)).all()  # nothing written


def test_host_rejects_null_handles_and_pointers(raw):
    _lib, handles = raw
    rc, _ = _host_call(_lib, [handles[0], None], [0, 4, 8])
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"envs[1]" in _lib.lib.vmv_last_error()
    offs = np.array([0, 4, 8], np.uint64)
    q = np.zeros((8, 7), np.float32)
    bits = np.zeros(1, np.uint64)
    envs = (ctypes.c_void_p * 2)(*handles)
    L, sp, fp, up = _lib.lib, _lib.c_size_p, _lib.c_float_p, _lib.c_u64_p
    assert L.vmv_validate_batch_multi_host(0, None, offs.ctypes.data_as(sp), 2, q.ctypes.data_as(fp),
                                           bits.ctypes.data_as(up)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_validate_batch_multi_host(0, envs, None, 2, q.ctypes.data_as(fp),
                                           bits.ctypes.data_as(up)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_validate_batch_multi_host(0, envs, offs.ctypes.data_as(sp), 2, None,
                                           bits.ctypes.data_as(up)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_validate_batch_multi(0, envs, offs.ctypes.data_as(sp), 2, None, None, None) == VMV_ERR_INVALID_ARGUMENT


def test_host_rejects_batches_beyond_the_32_bit_limit(raw):
    """the kernels count in 32 bits: n >= 2^31 is refused before anything is read from q or allocated"""
    _lib, handles = raw
    rc, _ = _host_call(_lib, handles, [0, 1 << 30, 1 << 31])
    assert rc == VMV_ERR_INVALID_ARGUMENT and b"2^31" in _lib.lib.vmv_last_error()


def test_host_reports_unfinalized_environments_without_a_device(raw):
    _lib, handles = raw
    rc, bits = _host_call(_lib, handles, [0, 3, 8])
    assert rc == VMV_ERR_NOT_FINALIZED
    assert (bits == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    # empty segments and repeated handles are allowed, and are checked all the same
    rc, _ = _host_call(_lib, [handles[0], handles[0], handles[1]], [0, 0, 8, 8])
    assert rc == VMV_ERR_NOT_FINALIZED
    rc, _ = _host_call(_lib, handles, [0, 4, 8], robot=7)
    assert rc == VMV_ERR_UNKNOWN_ROBOT


def test_python_checks_counts_and_shapes_before_any_library_call(vamp):
    q = np.zeros((10, 7), np.float32)
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    with pytest.raises(ValueError):
        vamp.panda.validate_batch_multi(q, [env, None], [4, 5])  # counts sum to 9
    with pytest.raises(ValueError):
        vamp.panda.validate_batch_multi(q, [env, None], [10])  # one count for two environments
    with pytest.raises(ValueError):
        vamp.panda.validate_batch_multi(q, [env, None], [12, -2])
    with pytest.raises(ValueError):
        vamp.panda.validate_batch_multi(q, [env], [[10]])
    with pytest.raises(TypeError):
        vamp.panda.validate_batch_multi(np.zeros((10, 6), np.float32), [env], [10])
    with pytest.raises(TypeError):
        vamp.panda.validate_batch_multi(q, ["not an environment"], [10])
    assert env._handle is None  # nothing was built or finalized
