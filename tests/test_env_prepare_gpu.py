"""<robot>.prepare / vmv_env_prepare_multi on the GPU: the robot part (broad-phase grids, reach certificates, static
links) built for many environments in one call equals, bit for bit, the part the first use builds on the host, for
every environment kind; and every validity bit stays what it is.

Throughout, environment A is built and used the lazy way (one one-configuration validate_batch), its twin B from the
same spec goes through `prepare` (or through a multi-environment validate call, which takes the same path)."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from envs import build_oracle_env, build_product_env, capsule, counted_spec, rot_cuboid, spec_for, yaw_cuboid

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "ur5", "fetch", "baxter"]
KINDS = ["empty", "cage", "shell64", "mixed", "many", "capt", "clouds", "mvt", "heightfield", "attach"]
EXTRA = ["ill-formed", "far", "static", "huge"]
# robots whose generated tables hold reach certificates (tools/gen_hip.py: link_samples); Fetch has none, so its
# link_skip is 0 in every environment
CERTIFIED = ["panda", "ur5", "baxter"]
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


def _ill_formed_spec(robot):
    """the ill-formed scene of tests/test_multi_env_gpu.py: stretched / sheared cuboid axes, a capsule whose rdv is
    not 1 / |v|^2"""
    out = []
    for k, (kind, p) in enumerate(spec_for("mixed", robot, seed=5)):
        p = np.array(p, np.float32)
        if kind == "cuboid" and k % 2 == 0:
            p[3:6] *= np.float32(1.7)
            p[6:9] += np.float32(0.4) * p[9:12]
        if kind == "capsule" and k % 3 == 0:
            p[7] *= np.float32(0.45)
        out.append((kind, p))
    return out


def _static_sphere(vamp, robot):
    """a small sphere at the centre of one of the robot's static spheres (one that no joint moves)"""
    mod = getattr(vamp, robot)
    lo, hi = np.array(mod.lower_bounds(), np.float32), np.array(mod.upper_bounds(), np.float32)
    rng = np.random.default_rng(3)
    fk = mod.fk_batch((lo + (hi - lo) * rng.random((16, len(lo)), dtype=np.float32)).astype(np.float32))
    still = np.flatnonzero((fk == fk[0]).all(axis=(0, 2)))
    assert len(still), f"{robot} has no static sphere"
    return ("sphere", np.array([*fk[0, still[0], :3], 0.02], np.float32))


def _specs(vamp, robot):
    specs = [spec_for(k, robot) for k in KINDS] + [_ill_formed_spec(robot)]
    specs.append([("sphere", np.array([50.0, 40.0, 30.0, 0.3], np.float32)),      # far outside the robot's reach
                  ("cuboid", rot_cuboid([60.0, -20.0, 5.0], [0.3, -0.2, 0.9], [0.2, 0.1, 0.3])),
                  ("cuboid", yaw_cuboid([-40.0, 30.0, 2.0], 0.7, [0.2, 0.1, 0.3])),
                  ("capsule", capsule([55.0, 55.0, 1.0], [55.3, 54.8, 1.4], 0.05)),
                  ("capsule", capsule([-45.0, 35.0, 1.0], [-45.0, 35.0, 1.6], 0.05))])
    specs.append(spec_for("cage", robot) + [_static_sphere(vamp, robot)])          # something on a static link
    specs.append([("sphere", np.array([-6000.0, 0.0, 0.5, 0.2], np.float32)),     # extents beyond 10^4 m: no grid
                  ("sphere", np.array([6000.0, 0.3, 0.5, 0.2], np.float32))])
    return specs


def _lazy(mod, spec):
    """environment A: the robot part built by its first use"""
    env = build_product_env(spec)
    mod.validate_batch(np.zeros((1, mod.dimension()), np.float32), env)
    return env


def _same_part(a, b, what):
    assert a["link_skip"] == b["link_skip"], (what, hex(a["link_skip"]), hex(b["link_skip"]))
    assert a["static_hit"] == b["static_hit"], what
    for c, (ga, gb) in enumerate(zip(a["grids"], b["grids"])):
        assert (ga is None) == (gb is None), (what, c)
        if ga is None:
            continue
        assert np.array_equal(ga["dims"], gb["dims"]), (what, c)
        assert np.array_equal(ga["origin"].view(np.uint32), gb["origin"].view(np.uint32)), (what, c)
        assert np.float32(ga["inv_cell"]).view(np.uint32) == np.float32(gb["inv_cell"]).view(np.uint32), (what, c)
        assert ga["cells"].shape == gb["cells"].shape, (what, c)
        assert np.array_equal(ga["cells"], gb["cells"]), \
            (what, c, f"{int((ga['cells'] != gb['cells']).sum())} of {ga['cells'].size} cell words differ")


def _configs(oracle, robot, n, rng):
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    return rid, (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize("robot", ROBOTS)
def test_prepared_parts_and_bits_equal_the_lazy_ones(vamp, oracle, robot):
    """identical robot part, identical bits, every environment kind, one prepare call"""
    mod = getattr(vamp, robot)
    specs = _specs(vamp, robot)
    names = KINDS + EXTRA
    A = [_lazy(mod, s) for s in specs]
    B = [build_product_env(s) for s in specs]
    rng = np.random.default_rng(sum(map(ord, robot)))
    order = list(rng.permutation(len(B))) + [1, 9, 1]  # shuffled, with repeated handles
    mod.prepare([B[i] for i in order])
    parts = []
    for name, a, b in zip(names, A, B):
        pa, pb = a.robot_part(mod), b.robot_part(robot)
        _same_part(pa, pb, (robot, name))
        parts.append(pb)
    part = dict(zip(names, parts))
    # the scenes do exercise what they are there for
    if robot in CERTIFIED:
        assert part["far"]["link_skip"] != 0 and part["empty"]["link_skip"] != 0
    else:
        assert part["far"]["link_skip"] == 0
    assert part["static"]["static_hit"] == 1 and part["cage"]["static_hit"] == 0
    assert all(g is None for g in part["huge"]["grids"]) and all(g is None for g in part["ill-formed"]["grids"])
    assert all(g is not None and g["cells"].any() for g in part["shell64"]["grids"])
    assert all(g is None for g in part["many"]["grids"])  # 250 primitives do not pack into four candidate words
    # identical bits: the multi calls over B against the per-environment calls over A, and the oracle
    counts = [int(c) for c in rng.choice([1, 63, 64, 65, 300], len(B))]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    rid, q = _configs(oracle, robot, int(offsets[-1]), rng)
    q2 = (q + rng.normal(0, 0.2, q.shape)).astype(np.float32)
    got = mod.validate_batch_multi(q, B, counts)
    got_m = mod.validate_motion_batch_multi(q, q2, B, counts)
    want = np.concatenate([mod.validate_batch(q[a:b], e) for e, a, b in zip(A, offsets[:-1], offsets[1:])])
    want_m = np.concatenate([mod.validate_motion_batch(q[a:b], q2[a:b], e) for e, a, b in zip(A, offsets[:-1], offsets[1:])])
    assert np.array_equal(got, want), f"{robot}: {int((got != want).sum())} configurations differ"
    assert np.array_equal(got_m, want_m), f"{robot}: {int((got_m != want_m).sum())} edges differ"
    assert got.any() and not got.all(), "degenerate workload"
    for name, spec, a, b in zip(names, specs, offsets[:-1], offsets[1:]):
        idx = np.arange(a, min(b, a + 48))
        oenv = build_oracle_env(oracle, spec)
        assert np.array_equal(got[idx], oracle.validate_batch(rid, oenv, q[idx], threads=8)), (robot, name)
        idx = idx[:8]
        assert np.array_equal(got_m[idx], oracle.validate_motion_batch(rid, oenv, q[idx], q2[idx])), (robot, name)


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch"])
def test_mbm_scenes_prepared_in_one_call(vamp, oracle, golden_dir, robot):
    """the 1,300 MotionBenchMaker scenes prepared in one call; the pinned valid counts; 50 parts against lazy twins"""
    from test_mbm import HERE, STANDARD, problem_primitives

    mod = getattr(vamp, robot)
    g = np.load(os.path.join(golden_dir, f"mbm_{robot}.npz"))
    names = [str(x) for x in g["names"]]
    specs = [problem_primitives(vamp, g, i) for i in range(len(names))]
    envs = [build_product_env(s) for s in specs]
    mod.prepare(envs)
    q = np.stack([np.stack([g["start"][i], g["goal"][i]]) for i in range(len(names))]).reshape(-1, g["start"].shape[1])
    got = mod.validate_batch_multi(q.astype(np.float32), envs, [2] * len(names))
    both = got.reshape(-1, 2).all(axis=1)
    assert int(sum(b for b, name in zip(both, names) if name in STANDARD)) == HERE[robot]
    for i in np.random.default_rng(2024).choice(len(names), 50, replace=False):
        _same_part(_lazy(mod, specs[i]).robot_part(mod), envs[i].robot_part(mod), (robot, names[i], int(g["index"][i])))


def test_multi_validate_calls_build_through_the_batch_path(vamp):
    """a first validate_batch_multi / validate_motion_batch_multi on fresh environments leaves them with the parts
    of lazily built twins"""
    mod = vamp.panda
    specs = [spec_for(k, "panda") for k in KINDS] + [counted_spec("panda", (3, 2, 2, 3, 2), seed=s) for s in range(6)]
    q = np.zeros((len(specs), 7), np.float32)
    B = [build_product_env(s) for s in specs]
    mod.validate_batch_multi(q, B, [1] * len(B))
    C = [build_product_env(s) for s in specs]
    mod.validate_motion_batch_multi(q, q, C, [1] * len(C))
    for k, spec in enumerate(specs):
        want = _lazy(mod, spec).robot_part(mod)
        _same_part(want, B[k].robot_part(mod), ("validate_batch_multi", k))
        _same_part(want, C[k].robot_part(mod), ("validate_motion_batch_multi", k))


def test_prepare_twice_and_over_environments_already_used(vamp):
    """idempotence and mixing with the lazy path"""
    mod = vamp.ur5
    specs = [counted_spec("ur5", (4, 2, 1, 3, 2), seed=s) for s in range(12)] + [spec_for("capt", "ur5"), []]
    A = [_lazy(mod, s) for s in specs]
    B = [build_product_env(s) for s in specs]
    for b in B[::2]:  # half of them already used the lazy way
        mod.validate_batch(np.zeros((1, 6), np.float32), b)
    mod.prepare(B)
    first = [b.robot_part(mod) for b in B]
    mod.prepare(B)
    mod.prepare(B[3:9] + [None])
    for a, b, p in zip(A, B, first):
        _same_part(a.robot_part(mod), p, "first prepare")
        _same_part(p, b.robot_part(mod), "second prepare")
    # another robot's part of the same environments is its own
    vamp.panda.prepare(B)
    for s, b in zip(specs[:4], B[:4]):
        _same_part(_lazy(vamp.panda, s).robot_part("panda"), b.robot_part("panda"), "panda after ur5")
        _same_part(_lazy(mod, s).robot_part(mod), b.robot_part(mod), "ur5 untouched")


def test_prepare_and_first_uses_on_another_thread(vamp, oracle):
    """one thread prepares 200 environments while another uses them one by one; all answers equal the twins'"""
    mod = vamp.panda
    specs = [counted_spec("panda", (5, 2, 2, 3, 2), seed=100 + s) for s in range(200)]
    _, q = _configs(oracle, "panda", 256, np.random.default_rng(11))
    want = [mod.validate_batch(q, build_product_env(s)) for s in specs]
    B = [build_product_env(s) for s in specs]
    for b in B:
        b.handle()  # finalized up front: the threads share the handles, not their construction
    got, errors = [None] * len(B), []

    def prepare():
        try:
            mod.prepare(B)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def use():
        try:
            for k in reversed(range(len(B))):  # from the other end: the two meet in the middle
                got[k] = mod.validate_batch(q, B[k])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=prepare), threading.Thread(target=use)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(len(B)):
        assert np.array_equal(got[k], want[k]), k
    assert any(w.any() for w in want) and not all(w.all() for w in want)
    for k in (0, 99, 199):
        _same_part(_lazy(mod, specs[k]).robot_part(mod), B[k].robot_part(mod), k)


_CHILD = r"""
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import numpy as np
import vamp_mvt_amd as vamp
from envs import build_product_env, spec_for
from test_env_prepare_gpu import _lazy, _same_part
vamp.set_device(0)
mod = vamp.panda
specs = [spec_for(k, "panda") for k in ("cage", "shell64", "mixed", "attach")]
specs.append([("sphere", np.array([50.0, 40.0, 30.0, 0.3], np.float32))])
A = [_lazy(mod, s) for s in specs]
B = [build_product_env(s) for s in specs]
mod.prepare(B)
parts = [b.robot_part(mod) for b in B]
for k, (a, p) in enumerate(zip(A, parts)):
    _same_part(a.robot_part(mod), p, k)
cells = sum(int(np.prod(g["dims"])) for p in parts for g in p["grids"] if g is not None)
print("RESULT", cells, sum(p["link_skip"] != 0 for p in parts))
"""


def _child(env_extra):
    env = dict(os.environ, **env_extra)
    code = _CHILD.format(tests=TESTS, root=os.path.join(TESTS, ".."))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_extra, r.stdout[-2000:], r.stderr[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
    return int(line[1]), int(line[2])


def test_switches_mean_the_same_in_both_paths():
    """VMV_NO_GRID, VMV_NO_LINK_SKIP, VMV_GRID_CELLS in a fresh process each (the first failing child ends the test)"""
    cells, skips = _child({})
    assert cells > 0 and skips > 0
    cells_off, skips_kept = _child({"VMV_NO_GRID": "1"})
    assert cells_off == 0 and skips_kept == skips
    cells_kept, skips_off = _child({"VMV_NO_LINK_SKIP": "1"})
    assert cells_kept == cells and skips_off == 0
    cells_few, _ = _child({"VMV_GRID_CELLS": "4000"})
    assert 0 < cells_few < cells


def test_environment_of_another_device_is_refused_and_nothing_prepared(vamp):
    """an environment finalized on another device is refused, and the call prepares nothing"""
    if vamp.device_count() < 2:
        pytest.skip("needs two GPUs")
    from vamp_mvt_amd import _lib

    vamp.set_device(1)
    try:
        other = build_product_env(spec_for("cage", "panda"))
        h1 = other.handle()
    finally:
        vamp.set_device(0)
    spec = spec_for("shell64", "panda")
    here = build_product_env(spec)
    handles = (ctypes.c_void_p * 2)(here.handle(), h1)
    assert _lib.lib.vmv_env_prepare_multi(0, handles, 2) == 1 and b"device" in _lib.lib.vmv_last_error()
    # nothing was prepared: `here` still builds (the lazy way) to what its twin holds
    _same_part(_lazy(vamp.panda, spec).robot_part("panda"), here.robot_part("panda"), "after the refused call")
