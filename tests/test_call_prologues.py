"""The argument checks of every batched C entry point, characterised: which status a refused call returns, what
vmv_last_error() says, which check wins when two apply, and that a refused call writes nothing.

Table-driven: ROWS describes each call's arguments, CASES the ways to spoil them.  The expected (status, message) of
every (call, case) is recorded in tests/golden/call_prologues.json, taken on a machine without a device
(`python tests/test_call_prologues.py --record` rewrites it; message null = the call sets none).  Without a device no
environment can be finalized, so the "valid" case of a call that needs one is an unfinalized environment, and
nothing here ever reaches a kernel: host arrays stand in for device pointers.  On a machine that has a device the
cases whose recorded status is NO_DEVICE / HIP (the call got as far as the device) are left to the GPU tests."""
import ctypes
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_prologues.json")
N = 4          # batch size of a spoiled call (two environments: 0..2, 2..4)
FILL = 0xA5    # every output byte before the call
REACHED_DEVICE = (2, 3)  # VMV_ERR_NO_DEVICE, VMV_ERR_HIP

# argument kinds: robot | env (required) | env? (NULL = none) | envs offsets n_envs | in (required input array) |
# out (required output) | out? (optional output) | n | stream | an int / float literal
_V = ("robot", "env", "in", "n", "out", "stream")
_M = ("robot", "envs", "offsets", "n_envs", "in", "out", "stream")
ROWS = {
    "vmv_validate_batch": _V,
    "vmv_validate_batch_env": _V,
    "vmv_validate_batch_host": _V[:-1],
    "vmv_validate_motion_batch": ("robot", "env", "in", "in", "n", "out", "stream"),
    "vmv_validate_motion_batch_host": ("robot", "env", "in", "in", "n", "out"),
    "vmv_validate_batch_multi": _M,
    "vmv_validate_batch_multi_host": _M[:-1],
    "vmv_validate_motion_batch_multi": ("robot", "envs", "offsets", "n_envs", "in", "in", "out", "stream"),
    "vmv_validate_motion_batch_multi_host": ("robot", "envs", "offsets", "n_envs", "in", "in", "out"),
    "vmv_env_prepare_multi": ("robot", "envs", "n_envs"),
    "vmv_clearance_batch": ("robot", "env?", "in", "n", "out", "out?", "stream"),
    "vmv_clearance_batch_host": ("robot", "env?", "in", "n", "out", "out?"),
    "vmv_clearance_batch_multi": ("robot", "envs", "offsets", "n_envs", "in", "out", "out?", "stream"),
    "vmv_clearance_batch_multi_host": ("robot", "envs", "offsets", "n_envs", "in", "out", "out?"),
    "vmv_clearance_grad_batch": ("robot", "env?", "in", "n", "out", "out", "out?", "stream"),
    "vmv_clearance_grad_batch_host": ("robot", "env?", "in", "n", "out", "out", "out?"),
    "vmv_clearance_grad_batch_multi": ("robot", "envs", "offsets", "n_envs", "in", "out", "out", "out?", "stream"),
    "vmv_clearance_grad_batch_multi_host": ("robot", "envs", "offsets", "n_envs", "in", "out", "out", "out?"),
    "vmv_fk_batch": ("robot", "in", "n", "out", "stream"),
    "vmv_fk_batch_host": ("robot", "in", "n", "out"),
    "vmv_eefk_batch": ("robot", "in", "n", "out", "stream"),
    "vmv_eefk_batch_host": ("robot", "in", "n", "out"),
    "vmv_contacts_batch_host": ("robot", "env", "in", "n", "out", "out"),
    "vmv_spheres_in_collision_batch": ("env", "in", "n", "out", "stream"),
    "vmv_spheres_in_collision_batch_host": ("env", "in", "n", "out"),
    "vmv_filter_self_from_pointcloud": ("robot", "env", "in", "in", "n", 0.01, "out?", N, "out"),
    "vmv_env_grid_info": ("env", "robot", 0, "out?", "out?", "out?", "out?"),
    "vmv_env_grid_cells": ("env", "robot", 0, "out?", 16, "out"),
    "vmv_env_robot_flags": ("env", "robot", "out?", "out?"),
    "vmv_fill_uniform_configs": ("robot", "out", "n", 7, "stream"),
    "vmv_halton_configs": ("robot", 0, "out", "n", "stream"),
}
CLEARANCE = tuple(s for s in ROWS if "clearance" in s)


def _cases(symbol):
    """-> [(case name, {argument index or kind: replacement})]; a replacement of a pointer is None (NULL)"""
    spec = ROWS[symbol]
    pointers = [i for i, k in enumerate(spec) if k in ("env", "envs", "offsets", "in", "out")]
    cases = [("valid", {})]
    if "robot" in spec:
        cases += [("robot=99", {"robot": 99}), ("robot=-1", {"robot": -1})]
    cases += [(f"arg{i}=NULL", {i: None}) for i in pointers]
    cases += [(f"arg{i}=NULL (optional)", {i: None}) for i, k in enumerate(spec) if k in ("env?", "out?")]
    size = "n" if "n" in spec else "n_envs" if "n_envs" in spec else None
    if size:
        cases.append((f"{size}=0", {size: 0}))
        cases += [(f"arg{i}=NULL, {size}=0", {i: None, size: 0}) for i in pointers]
        if "robot" in spec:
            cases.append((f"robot=99, {size}=0", {"robot": 99, size: 0}))
    if "robot" in spec:  # which check wins
        cases += [(f"robot=99, arg{i}=NULL", {"robot": 99, i: None}) for i in pointers]
    if len(pointers) > 1:
        cases.append(("every pointer NULL", {i: None for i in pointers}))
    if "envs" in spec:
        cases += [("envs[1]=NULL", {"envs": ["plain", None]}), ("envs[0]=NULL", {"envs": [None, "plain"]})]
    if "offsets" in spec:
        cases += [("offsets[0]=1", {"offsets": [1, 2, 4]}), ("offsets decreasing", {"offsets": [0, 3, 2]}),
                  ("all segments empty", {"offsets": [0, 0, 0]}), ("envs[1]=NULL, all segments empty",
                                                                  {"envs": ["plain", None], "offsets": [0, 0, 0]})]
    if symbol in CLEARANCE:
        for kind in ("capt", "mvt", "attach"):
            one = {"envs": ["plain", kind]} if "envs" in spec else {"env?": kind}
            cases.append((f"environment with {kind}", one))
            cases.append((f"environment with {kind}, first output NULL", {**one, spec.index("out"): None}))
            cases.append((f"environment with {kind}, robot=99", {**one, "robot": 99}))
            cases.append((f"environment with {kind}, {size}=0", {**one, size: 0}))
    return cases


ALL = [(s, name) for s in ROWS for name, _ in _cases(s)]


def _world(vamp):
    """-> (_lib, {kind: handle of an unfinalized environment}, a device is present)"""
    from vamp_mvt_amd import _lib

    L = _lib.lib
    fp = lambda a: a.ctypes.data_as(_lib.c_float_p)  # noqa: E731
    envs = {}
    for kind in ("plain", "capt", "mvt", "attach"):
        h = ctypes.c_void_p()
        assert L.vmv_env_create(ctypes.byref(h)) == 0
        assert L.vmv_env_add_sphere(h, 0.5, 0.0, 0.5, 0.1) == 0
        pts = np.random.default_rng(3).uniform(0.3, 0.9, (64, 3)).astype(np.float32)
        lo, hi = np.full(3, -2.0, np.float32), np.full(3, 2.0, np.float32)
        if kind == "capt":
            assert L.vmv_env_add_capt_pointcloud(h, fp(pts), len(pts), 0.01, 0.1, 0.005, None) == 0
        elif kind == "mvt":
            assert L.vmv_env_add_mvt_pointcloud(h, fp(pts), len(pts), 0.01, 0.1, fp(lo), fp(hi), 0.005, None, None) == 0
        elif kind == "attach":
            assert L.vmv_env_attach(h, fp(np.eye(4, dtype=np.float32)), fp(np.array([[0, 0, 0.1, 0.03]], np.float32)), 1) == 0
        envs[kind] = h.value
    count = ctypes.c_int(0)
    L.vmv_device_count(ctypes.byref(count))
    yield _lib, envs, count.value > 0
    for h in envs.values():
        L.vmv_env_destroy(h)


@pytest.fixture(scope="module")
def world(vamp):
    yield from _world(vamp)


def _call(_lib, envs, symbol, changes):
    """one call of `symbol` with `changes` applied -> (status, message or None, the outputs are untouched)"""
    L = _lib.lib
    fn = getattr(L, symbol)
    keep, outputs, args = [], [], []
    for i, kind in enumerate(ROWS[symbol]):
        value = changes.get(i, changes.get(kind, kind)) if isinstance(kind, str) else kind
        if value in ("env", "env?"):
            value = envs["plain"]
        elif isinstance(value, str) and value in envs:
            value = envs[value]
        elif value == "envs" or isinstance(value, list) and kind == "envs":
            names = ["plain", "plain"] if value == "envs" else value
            keep.append((ctypes.c_void_p * 2)(*[envs[x] if x else None for x in names]))
            value = ctypes.addressof(keep[-1])
        elif value == "offsets" or isinstance(value, list):
            keep.append(np.array([0, N // 2, N] if value == "offsets" else value, np.uint64))
            value = keep[-1].ctypes.data
        elif value == "in":
            keep.append(np.zeros(1024, np.float32))
            value = keep[-1].ctypes.data
        elif value in ("out", "out?"):
            outputs.append(np.full(4096, FILL, np.uint8))
            value = outputs[-1].ctypes.data
        elif value == "n":
            value = N
        elif value == "n_envs":
            value = 2
        elif value == "robot":
            value = 0
        elif value == "stream":
            value = None
        t = fn.argtypes[i]
        args.append(ctypes.cast(ctypes.c_void_p(value), t) if hasattr(t, "contents") else value)
    # a message no case produces, so that "the call set none" shows
    marker = np.array([0, 2, 2, 1], np.uint64)
    three = (ctypes.c_void_p * 3)(*[envs["plain"]] * 3)
    buf = np.zeros(4, np.float32)
    assert L.vmv_clearance_batch_multi(0, three, marker.ctypes.data_as(_lib.c_size_p), 3, buf.ctypes.data, buf.ctypes.data,
                                       None, None) == 1
    before = L.vmv_last_error().decode()
    assert "offsets[3] < offsets[2]" in before
    rc = fn(*args)
    after = L.vmv_last_error().decode()
    message = None if after == before else after
    return rc, message, all(bool((o == FILL).all()) for o in outputs)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_every_recorded_case(golden):
    assert sorted(golden) == sorted(f"{s} / {c}" for s, c in ALL)


@pytest.mark.parametrize("symbol", list(ROWS))
def test_prologue(world, golden, symbol):
    _lib, envs, have_device = world
    for name, changes in _cases(symbol):
        want_rc, want_message = golden[f"{symbol} / {name}"]
        if have_device and want_rc in REACHED_DEVICE:
            continue
        rc, message, untouched = _call(_lib, envs, symbol, changes)
        print(f"{symbol} / {name}: {rc} {message!r}")
        assert (rc, message) == (want_rc, want_message), f"{symbol} / {name}"
        assert untouched or rc == 0, f"{symbol} / {name}: a refused call wrote to an output"
        assert untouched, f"{symbol} / {name}: no call here can reach a kernel, yet an output changed"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    assert "--record" in sys.argv
    import vamp_mvt_amd  # noqa: F401
    from vamp_mvt_amd import _lib as the_lib

    gen = _world(vamp_mvt_amd)
    _, the_envs, device = next(gen)
    assert not device, "record on a machine without a device"
    table = {}
    for s, c in ALL:
        r, m, same = _call(the_lib, the_envs, s, dict(_cases(s))[c])
        assert same, (s, c)
        table[f"{s} / {c}"] = [r, m]
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(table), "cases recorded")
