"""The argument checks of the calls that take end-effector constraints, and of the two path calls whose environments may
be NULL, characterised: which status a refused call returns, what vmv_last_error() says, which check wins when two
apply, and that a refused call writes nothing - neither its output arrays nor *out.

Table-driven, in the manner of test_call_prologues.py: ROWS names each call's arguments, `_cases` the ways to spoil
them.  The expected (status, message) of every (call, case) is recorded in tests/golden/constrained_prologues.json (per call one line per outcome, with the cases
that have it), taken on a machine without a device (`python tests/test_constrained_prologues.py --record` rewrites it; message null = the
call sets none).  Without a device no environment can be finalized, so the environments of a "valid" call are
unfinalized ones and nothing here reaches a kernel: host arrays stand in for device pointers.  On a machine that has a
device the cases whose recorded status is NO_DEVICE / HIP (the call got as far as the device) are left to the GPU tests."""
import ctypes
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constrained_prologues.json")
N = 3          # lanes, problems or paths of a spoiled call (paths of 2 waypoints each)
FILL = 0xA5    # every output byte before the call
HANDLE = 0xA5A5A5A5  # *out before the call
REACHED_DEVICE = (2, 3)  # VMV_ERR_NO_DEVICE, VMV_ERR_HIP
NAN, INF = float("nan"), float("inf")

# argument kinds: robot | envs (required) | envs? (NULL = no environments, the default here) | n | in (required input array) |
# in? (optional input) | limits (required, [dim] positive) | offsets (required, [n + 1]) | offsets? | settings (the
# call's own struct) | cons n_cons cset (the constraints, their count, their settings) | out (required output) |
# out? (optional output) | handle (the result object's address) | stream
_BATCH = ("robot", "in", "n", "cons", "n_cons", "cset")
_PATHS = ("robot", "envs", "n", "in", "offsets", "settings", "cons", "n_cons", "cset", "handle")
ROWS = {
    "vmv_constraint_project_batch": _BATCH + ("out", "out?", "out", "stream"),
    "vmv_constraint_project_batch_host": _BATCH + ("out", "out?", "out"),
    "vmv_constraint_check_batch": _BATCH + ("out", "out?", "stream"),
    "vmv_constraint_check_batch_host": _BATCH + ("out", "out?"),
    "vmv_constraint_check_motion_batch": ("robot", "in", "in", "n", "cons", "n_cons", "cset", "out", "stream"),
    "vmv_constraint_check_motion_batch_host": ("robot", "in", "in", "n", "cons", "n_cons", "cset", "out"),
    "vmv_rrtc_multi_constrained": ("robot", "envs", "n", "in", "in", "offsets?", "in?", "settings", "cons", "n_cons", "cset", "handle"),
    "vmv_simplify_multi_constrained": _PATHS,
    "vmv_optimize_multi_constrained": _PATHS,
    "vmv_retime_multi_constrained": ("robot", "envs?", "n", "in", "offsets", "limits", "limits", "cons", "n_cons", "settings", "cset",
                                     "handle"),
    "vmv_retime_band_pairs_host": ("robot", "in", "offsets", "n", "cons", "n_cons", "cset", "out"),
    "vmv_retime_multi": ("robot", "envs?", "n", "in", "offsets", "limits", "limits", "settings", "handle"),
    "vmv_cartesian_multi": ("robot", "envs?", "n", "in", "frames", "settings", "handle"),
}
DESTROY = {"vmv_rrtc_multi_constrained": "vmv_plans_destroy", "vmv_simplify_multi_constrained": "vmv_paths_destroy",
           "vmv_optimize_multi_constrained": "vmv_optimized_destroy", "vmv_retime_multi_constrained": "vmv_retime_destroy",
           "vmv_retime_multi": "vmv_retime_destroy", "vmv_cartesian_multi": "vmv_cartesian_destroy"}
CSET_FIELDS = ("max_iterations", "pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "check_step")
BAD_CONSTRAINTS = ("pos_lo > pos_hi", "a frame that is not rigid", "max_angle NaN")
# the call's own value that its prologue checks between the constraint settings and the constraints, or next to them
OWN = {"vmv_rrtc_multi_constrained": [("max_stretch", NAN), ("max_stretch", -1.0), ("max_stretch", INF)],
       "vmv_retime_multi_constrained": [("blend_halvings", 8), ("blend_halvings", 9)]}


def _cases(symbol):
    """-> [(case name, {argument index, kind or special key: replacement})]; a replacement of a pointer is None (NULL).
    Special keys: "cset.<field>" a constraint-settings field, "own" (field, value) of OWN, "bad" (index, kind of
    BAD_CONSTRAINTS), "envs" a list of environment kinds."""
    spec = ROWS[symbol]
    constrained = "cons" in spec
    pointers = [i for i, k in enumerate(spec) if k in ("envs", "in", "limits", "offsets", "frames", "settings", "cons", "cset", "out",
                                                       "handle")]
    optional = [i for i, k in enumerate(spec) if k in ("envs?", "in?", "offsets?", "out?")]
    cases = [("valid", {}), ("robot=99", {"robot": 99}), ("robot=-1", {"robot": -1})]
    cases += [(f"arg{i}=NULL", {i: None}) for i in pointers]
    cases += [(f"arg{i}=NULL (optional)", {i: None}) for i in optional]
    cases += [(f"arg{i} given (optional)", {i: "given"}) for i, k in enumerate(spec) if k in ("envs?", "in?", "offsets?")]
    cases.append(("every pointer NULL", {i: None for i in pointers}))
    cases += [(f"robot=99, arg{i}=NULL", {"robot": 99, i: None}) for i in pointers]
    cases += [("n=0", {"n": 0})] + [(f"n=0, arg{i}=NULL", {"n": 0, i: None}) for i in pointers]
    if "envs" in spec or "envs?" in spec:
        cases += [("envs[1]=NULL", {"envs": ["plain", None, "plain"]}), ("envs[2]=NULL", {"envs": ["plain", "plain", None]})]
        cases += [(f"environment with {kind}", {"envs": ["plain", kind, "plain"]}) for kind in ("capt", "mvt", "attach")]
        cases += [(f"environment with {kind}, arg{spec.index('handle')}=NULL", {"envs": ["plain", kind, "plain"], spec.index("handle"): None})
                  for kind in ("capt", "mvt", "attach")]
    if not constrained:
        return cases
    cons, cset = spec.index("cons"), spec.index("cset")
    cases += [(f"n_constraints={k}", {"n_cons": k}) for k in (0, 1, 2, N + 1)]
    cases += [(f"n=0, n_constraints={k}", {"n": 0, "n_cons": k}) for k in (0, 1, 2)]
    cases.append(("max_iterations=2^30", {"cset.max_iterations": 1 << 30}))
    cases.append(("max_iterations=2^30 - 1", {"cset.max_iterations": (1 << 30) - 1}))
    cases += [(f"{f}={v!r}", {f"cset.{f}": v}) for f in CSET_FIELDS[1:] for v in (NAN, -1.0, INF)]
    cases += [(f"{f}={v!r}", {"own": (f, v)}) for f, v in OWN.get(symbol, [])]
    for count in (N, 1):
        for k in sorted({0, count - 1}):
            cases += [(f"constraints[{k}] of {count}: {bad}", {"n_cons": count, "bad": (k, bad)}) for bad in BAD_CONSTRAINTS]
    cases.append(("constraints[0] and [2] bad", {"bads": [(0, "max_angle NaN"), (2, "pos_lo > pos_hi")]}))
    # which check wins
    cases += [
        ("n_constraints=2, pos_tol=nan", {"n_cons": 2, "cset.pos_tol": NAN}),
        ("constraints=NULL, n_constraints=2", {cons: None, "n_cons": 2}),
        ("constraint settings=NULL, n_constraints=2", {cset: None, "n_cons": 2}),
        ("constraints=NULL, n_constraints=0", {cons: None, "n_cons": 0}),
        ("constraints=NULL, constraint settings=NULL, n_constraints=0", {cons: None, cset: None, "n_cons": 0}),
        ("constraints=NULL, pos_tol=nan", {cons: None, "cset.pos_tol": NAN}),
        ("pos_tol=nan, check_step=-1", {"cset.pos_tol": NAN, "cset.check_step": -1.0}),
        ("pos_tol=nan, constraints[0] bad", {"cset.pos_tol": NAN, "bad": (0, "pos_lo > pos_hi")}),
        ("n_constraints=2, constraints[0] bad", {"n_cons": 2, "bad": (0, "pos_lo > pos_hi")}),
        ("robot=99, constraints[0] bad", {"robot": 99, "bad": (0, "pos_lo > pos_hi")}),
        ("n=0, constraints[0] bad", {"n": 0, "n_cons": 1, "bad": (0, "pos_lo > pos_hi")}),
        ("n=0, pos_tol=nan", {"n": 0, "cset.pos_tol": NAN}),
    ]
    for f, v in OWN.get(symbol, [])[:1] + OWN.get(symbol, [])[-1:]:
        cases += [(f"{f}={v!r}, constraints[0] bad", {"own": (f, v), "bad": (0, "pos_lo > pos_hi")}),
                  (f"{f}={v!r}, pos_tol=nan", {"own": (f, v), "cset.pos_tol": NAN}),
                  (f"{f}={v!r}, n_constraints=2", {"own": (f, v), "n_cons": 2}),
                  (f"{f}={v!r}, constraints=NULL", {"own": (f, v), cons: None})]
    if "settings" in spec:  # the call's own checks come first
        cases.append((f"arg{spec.index('settings')}=NULL, constraints[0] bad", {spec.index("settings"): None, "bad": (0, "pos_lo > pos_hi")}))
    if "envs" in spec or "envs?" in spec:  # (every environment here is unfinalized: the "valid" case shows its refusal)
        cases += [("envs[1]=NULL, constraints[0] bad", {"envs": ["plain", None, "plain"], "bad": (0, "pos_lo > pos_hi")}),
                  ("environment with capt, constraints[2] bad", {"envs": ["plain", "capt", "plain"], "bad": (2, "max_angle NaN")}),
                  ("environment with capt, n_constraints=2", {"envs": ["plain", "capt", "plain"], "n_cons": 2}),
                  ("environment with capt, pos_tol=nan", {"envs": ["plain", "capt", "plain"], "cset.pos_tol": NAN})]
    if "envs?" in spec:
        given = {spec.index("envs?"): "given"}
        cases += [("environments given, constraints[2] bad", {**given, "bad": (2, "max_angle NaN")}),
                  ("environments given, n_constraints=0", {**given, "n_cons": 0}),
                  ("environments given, n_constraints=2", {**given, "n_cons": 2}),
                  ("environments given, n=0", {**given, "n": 0})]
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


def _settings(_lib, symbol, own):
    """the call's own settings struct, good values"""
    if symbol == "vmv_rrtc_multi_constrained":
        return _lib.RrtcGoalsSettings(_lib.RrtcSettings(0.5, 1, 1.0, 100, 64, 0), 0, 4.0, 0.0001, 1.0, 0)
    if symbol == "vmv_simplify_multi_constrained":
        return _lib.SimplifySettings(1, 0, 1, (ctypes.c_uint32 * 8)(2), 4, 0.001, 0.5, 0, 0, 0)
    if symbol == "vmv_optimize_multi_constrained":
        return _lib.OptimizeSettings(10, 1, 0.1, 0.1, 0.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0)
    if symbol == "vmv_retime_multi_constrained":
        s = _lib.RetimeConstrainedSettings()
        if own and own[0] == "blend_halvings":
            s.blend_halvings = own[1]
        return s
    return _lib.RetimeSettings() if symbol == "vmv_retime_multi" else _lib.CartesianSettings()


def _constraints(_lib, count, bads):
    """`count` constraints that restrict nothing (at least one record, so that a count of 0 still has a pointer)"""
    records = (_lib.EeConstraint * max(count, N + 1))()
    for c in records:
        c.frame[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
        c.pos_lo[:], c.pos_hi[:] = [-INF] * 3, [INF] * 3
        c.tool_axis[:], c.ref_axis[:], c.max_angle = [0, 0, 1], [0, 0, 1], 0.0
    for k, bad in bads:
        c = records[k]
        if bad == "pos_lo > pos_hi":
            c.pos_lo[0], c.pos_hi[0] = 1.0, 0.0
        elif bad == "a frame that is not rigid":
            c.frame[0] = 2.0
        else:
            assert bad == "max_angle NaN"
            c.max_angle = NAN
    return records


def _call(_lib, envs, symbol, changes):
    """one call of `symbol` with `changes` applied -> (status, message or None, the outputs and *out are untouched)"""
    L = _lib.lib
    fn = getattr(L, symbol)
    spec = ROWS[symbol]
    n = changes.get("n", N)
    n_cons = changes.get("n_cons", N if n else 1)
    own = changes.get("own")
    bads = changes.get("bads", [changes["bad"]] if "bad" in changes else [])
    keep, outputs, args, handle = [], [], [], None
    for i, kind in enumerate(spec):
        value = changes.get(i, "envs" if kind == "envs?" and "envs" in changes else kind)
        if value == "given":
            value = kind[:-1]
        if value is None or value in ("envs?", "in?", "offsets?", "stream"):
            value = None
        elif value == "robot":
            value = changes.get("robot", 0)
        elif value == "n":
            value = n
        elif value == "n_cons":
            value = n_cons
        elif value == "envs":
            names = changes.get("envs", ["plain"] * N)
            keep.append((ctypes.c_void_p * N)(*[envs[x] if x else None for x in names]))
            value = ctypes.addressof(keep[-1])
        elif value == "in":
            keep.append(np.zeros(1024, np.float32))
            value = keep[-1].ctypes.data
        elif value == "limits":
            keep.append(np.ones(16, np.float32))
            value = keep[-1].ctypes.data
        elif value == "frames":
            keep.append(np.tile(np.eye(4, dtype=np.float32).reshape(-1), N))
            value = keep[-1].ctypes.data
        elif value == "offsets":  # paths of 2 waypoints (for vmv_rrtc_multi_constrained: sets of 2 goals)
            keep.append(np.arange(N + 1, dtype=np.uintp) * 2)
            value = keep[-1].ctypes.data
        elif value == "settings":
            keep.append(_settings(_lib, symbol, own))
            value = ctypes.addressof(keep[-1])
        elif value == "cons":
            keep.append(_constraints(_lib, n_cons, bads))
            value = ctypes.addressof(keep[-1])
        elif value == "cset":
            base = _lib.ConstraintSettings()
            for key, v in changes.items():
                if isinstance(key, str) and key.startswith("cset."):
                    setattr(base, key[5:], v)
            keep.append(_lib.ConstraintPlanSettings(base, own[1] if own and own[0] == "max_stretch" else 0.0)
                        if symbol == "vmv_rrtc_multi_constrained" else base)
            value = ctypes.addressof(keep[-1])
        elif value in ("out", "out?"):
            outputs.append(np.full(4096, FILL, np.uint8))
            value = outputs[-1].ctypes.data
        elif value == "handle":
            handle = ctypes.c_void_p(HANDLE)
            value = ctypes.addressof(handle)
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
    untouched = all(bool((o == FILL).all()) for o in outputs)
    if handle is not None and handle.value != HANDLE:
        if rc == 0:  # (an accepted call with n = 0: the empty result)
            assert getattr(L, DESTROY[symbol])(handle) == 0
        else:
            untouched = False
    elif handle is not None and rc == 0:
        untouched = False  # an accepted call hands out its result
    return rc, message, untouched


@pytest.fixture(scope="module")
def golden():
    """{"<call> / <case>": [status, message]} from the file's {call: [[status, message, [the cases with that outcome]]]}"""
    with open(GOLDEN) as f:
        return {f"{s} / {c}": [rc, message] for s, outcomes in json.load(f).items() for rc, message, names in outcomes for c in names}


def test_the_table_covers_every_recorded_case(golden):
    assert len(set(ALL)) == len(ALL)
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
        assert untouched, f"{symbol} / {name}: no call here can reach a kernel, yet an output or *out changed"


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
        table.setdefault(s, {}).setdefault((r, m), []).append(c)
    with open(GOLDEN, "w") as f:  # one line per outcome of a call
        f.write("{\n" + ",\n".join(json.dumps(s) + ": [\n" + ",\n".join(json.dumps([r, m, names]) for (r, m), names in outcomes.items()) + "]"
                                  for s, outcomes in table.items()) + "\n}\n")
    print(len(ALL), "cases recorded")
