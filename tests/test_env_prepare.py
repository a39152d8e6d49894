"""vmv_env_prepare_multi and the robot-part inspection calls: the declarations and the checks that need no device (they
run before any device query, in the header's order, so they hold on a CPU-only machine too)."""
import ctypes

import pytest

VMV_OK, VMV_ERR_INVALID_ARGUMENT, VMV_ERR_NOT_FINALIZED, VMV_ERR_UNKNOWN_ROBOT = 0, 1, 5, 6
SYMBOLS = ("vmv_env_prepare_multi", "vmv_env_grid_info", "vmv_env_grid_cells", "vmv_env_robot_flags")


@pytest.fixture()
def raw(vamp):
    """two unfinalized C environments with a sphere each (no device needed), destroyed afterwards"""
    from vamp_mvt_amd import _lib

    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    handles = [env._build(finalize=False) for _ in range(2)]
    yield _lib, [h.value for h in handles]
    for h in handles:
        _lib.lib.vmv_env_destroy(h)


def _prepare(_lib, handles, robot=0, n=None):
    envs = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    return _lib.lib.vmv_env_prepare_multi(robot, envs, len(handles) if n is None else n)


def test_symbols_are_declared_and_exported(vamp):
    from vamp_mvt_amd import _lib

    names = _lib.declared_symbols()
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in names and hasattr(exported, name), name
    assert vamp.abi_version() == 1  # the change is additive


def test_no_environments_is_ok(vamp):
    from vamp_mvt_amd import _lib

    assert _lib.lib.vmv_env_prepare_multi(0, None, 0) == VMV_OK
    envs = (ctypes.c_void_p * 1)(None)
    assert _lib.lib.vmv_env_prepare_multi(0, envs, 0) == VMV_OK


def test_checks_come_in_the_documented_order(raw):
    _lib, handles = raw
    # an unknown robot is reported before anything else is looked at
    for robot in (-1, 4, 7):
        assert _lib.lib.vmv_env_prepare_multi(robot, None, 2) == VMV_ERR_UNKNOWN_ROBOT
        assert _prepare(_lib, [None, handles[0]], robot=robot) == VMV_ERR_UNKNOWN_ROBOT
        assert _lib.lib.vmv_env_prepare_multi(robot, None, 0) == VMV_ERR_UNKNOWN_ROBOT
    # then null pointers: the array, then any handle (before the state of the handles in front of it)
    assert _lib.lib.vmv_env_prepare_multi(0, None, 2) == VMV_ERR_INVALID_ARGUMENT
    assert _prepare(_lib, [handles[0], None]) == VMV_ERR_INVALID_ARGUMENT
    assert b"envs[1]" in _lib.lib.vmv_last_error()
    assert _prepare(_lib, [None, handles[0]]) == VMV_ERR_INVALID_ARGUMENT
    assert b"envs[0]" in _lib.lib.vmv_last_error()
    # then unfinalized environments (repeated handles are allowed, and checked all the same)
    assert _prepare(_lib, handles) == VMV_ERR_NOT_FINALIZED
    assert b"envs[0]" in _lib.lib.vmv_last_error()
    assert _prepare(_lib, [handles[1], handles[1], handles[0]]) == VMV_ERR_NOT_FINALIZED
    for robot in range(4):
        assert _prepare(_lib, handles, robot=robot) == VMV_ERR_NOT_FINALIZED


def test_inspection_calls_check_their_arguments_without_a_device(raw):
    _lib, handles = raw
    L = _lib.lib
    dims = (ctypes.c_uint32 * 3)()
    origin = (ctypes.c_float * 3)()
    inv_cell, words, n = ctypes.c_float(), ctypes.c_uint32(), ctypes.c_size_t()
    skip, hit = ctypes.c_uint64(), ctypes.c_uint32()
    h = handles[0]
    assert L.vmv_env_grid_info(h, 9, 0, dims, origin, ctypes.byref(inv_cell), ctypes.byref(words)) == VMV_ERR_UNKNOWN_ROBOT
    assert L.vmv_env_grid_cells(h, 9, 0, None, 0, ctypes.byref(n)) == VMV_ERR_UNKNOWN_ROBOT
    assert L.vmv_env_robot_flags(h, 9, ctypes.byref(skip), ctypes.byref(hit)) == VMV_ERR_UNKNOWN_ROBOT
    assert L.vmv_env_grid_info(None, 0, 0, dims, origin, ctypes.byref(inv_cell), ctypes.byref(words)) == VMV_ERR_INVALID_ARGUMENT
    for grid_class in (-1, 4):
        assert L.vmv_env_grid_info(h, 0, grid_class, dims, origin, ctypes.byref(inv_cell), ctypes.byref(words)) == \
            VMV_ERR_INVALID_ARGUMENT
        assert L.vmv_env_grid_cells(h, 0, grid_class, None, 0, ctypes.byref(n)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_env_grid_cells(h, 0, 0, None, 0, None) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_env_robot_flags(None, 0, ctypes.byref(skip), ctypes.byref(hit)) == VMV_ERR_INVALID_ARGUMENT
    assert L.vmv_env_grid_info(h, 0, 0, dims, origin, ctypes.byref(inv_cell), ctypes.byref(words)) == VMV_ERR_NOT_FINALIZED
    assert L.vmv_env_grid_cells(h, 0, 0, None, 0, ctypes.byref(n)) == VMV_ERR_NOT_FINALIZED
    assert L.vmv_env_robot_flags(h, 0, ctypes.byref(skip), ctypes.byref(hit)) == VMV_ERR_NOT_FINALIZED


def test_python_prepare_checks_its_list_before_any_library_call(vamp):
    env = vamp.Environment()
    env.add_sphere(vamp.Sphere([0.5, 0.0, 0.5], 0.1))
    with pytest.raises(TypeError):
        vamp.panda.prepare([env, "not an environment"])
    assert env._handle is None  # nothing was built or finalized
