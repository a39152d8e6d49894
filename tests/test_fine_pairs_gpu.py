"""The pair-dealt fine phase of the primitive-only configuration kernels (vmv_device.h env_fine_pairs) on the GPU.  Every
case compares, word for word, the environment stage (vmv_validate_batch_env) of the default instance with the packed
instance (VMV_FINE_PAIRS=0, computed once for all cases by a child process), and checks the bits against the CPU
oracle: wherever the oracle finds no self-collision, the stage's bit is the oracle's answer for the configuration.

Scenes: shell64 (the three-list variant), the mixed five-list scene (shared candidate words), no primitive at all, 128
primitives (all four candidate words), a cluster of 96 small spheres and 28 z-aligned cuboids inside the gate of one
link (one lane's sphere list alone holds more candidates than the entry list: several fills), a pebble (one lane through
a gate, one or two entries), and the ill-formed scene, which must keep the variant with the reference's groups.
Batches: n in {1, 63, 64, 65, 257, 1000}, one configuration 64 times, 63 far configurations with the touching one first,
last or in between, a non-finite row in the middle of a word; one multi-environment call whose segments start inside
words."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from envs import SHELL, build_oracle_env, build_product_env, spec_for
from vamp_mvt_amd.workloads import shell_spec, yaw_cuboid

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SIZES = [1, 63, 64, 65, 257, 1000]
EVERYWHERE = ["panda", "ur5"]
SCENES = {"panda": ["shell64", "mixed", "empty", "p128", "cluster", "pebble", "ill-formed"],
          "ur5": ["shell64", "mixed", "empty", "p128", "cluster", "pebble", "ill-formed"],
          "fetch": ["shell64", "mixed"], "baxter": ["shell64", "mixed"]}
PAIR_ENTRIES = 64  # vmv::kPairEntries (checked against the header below)
MARGIN = 1e-4      # vmv::kCandidateMargin


def _gen_hip():
    import self_gates

    return self_gates.gen_hip(), self_gates.model


def _uniform(oracle, robot, n, seed):
    lo, span = oracle.bounds(oracle.robot(robot))
    return (lo + span * np.random.default_rng(seed).random((n, len(lo)), dtype=np.float32)).astype(np.float32)


_ANCHOR = {}


def _anchor(oracle, robot):
    """(q0, centre, far configurations): q0 is a configuration without self-collision; centre is where q0 puts the
    largest fine sphere behind the last merged gate of the primitive-only walk (a hand: a ball of that sphere's radius
    around centre lies inside the sphere, so inside the gate's); far = 63 configurations without self-collision whose
    spheres all stay more than 0.25 m away from centre"""
    if robot in _ANCHOR:
        return _ANCHOR[robot]
    g, model = _gen_hip()
    m = model(robot)
    gate = g.merged_groups(m)[-1]
    big = max(gate["fine"], key=lambda s: m["radii"][s])
    assert m["radii"][big] > 0.0215, "the cluster (offsets up to 0.012 m per axis) must fit inside the sphere"
    rid = oracle.robot(robot)
    q = _uniform(oracle, robot, 600, 77)
    ok = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
    q0 = None
    for c in q[ok]:
        centre = oracle.fk_all(rid, c)[big, :3].astype(np.float64)
        if centre[2] > 0.35 and np.hypot(centre[0], centre[1]) > 0.35:  # away from the base and the floor
            q0 = c
            break
    assert q0 is not None
    far = []
    for c in q[ok]:
        s = oracle.fk(rid, c).astype(np.float64)
        if (np.linalg.norm(s[:, :3] - centre, axis=1) - s[:, 3]).min() > 0.25:
            far.append(c)
        if len(far) == 63:
            break
    assert len(far) == 63
    _ANCHOR[robot] = (q0, centre, np.array(far, np.float32))
    return _ANCHOR[robot]


def _cluster_spec(oracle, robot):
    """96 spheres and 28 z-aligned cuboids, each under 1 cm, their centres within 1.2 cm per axis of _anchor's centre"""
    _, centre, _ = _anchor(oracle, robot)
    rng = np.random.default_rng(31)
    spec = []
    for i in range(96 + 28):
        c = (centre + rng.uniform(-0.012, 0.012, 3)).astype(np.float32)
        if i < 96:
            spec.append(("sphere", np.array([*c, rng.uniform(0.003, 0.008)], np.float32)))
        else:
            spec.append(("cuboid", yaw_cuboid(c, rng.uniform(0, 2 * np.pi), rng.uniform(0.003, 0.008, 3))))
    return spec


def _pebble_spec(oracle, robot):
    _, centre, _ = _anchor(oracle, robot)
    c = centre.astype(np.float32)
    return [("sphere", np.array([*c, 0.01], np.float32)),
            ("cuboid", yaw_cuboid((c + np.float32([0.0, 0.0, 0.03])).astype(np.float32), 0.3, np.float32([0.01, 0.01, 0.01])))]


def _ill_formed_spec(robot):
    """the scene of tests/test_multi_env_gpu.py: stretched / sheared cuboid axes, a capsule whose rdv is not 1 / |v|^2"""
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


def _spec(oracle, robot, scene):
    if scene == "shell64":
        return shell_spec(0)
    if scene == "mixed":
        return spec_for("mixed", robot)
    if scene == "empty":
        return []
    if scene == "p128":
        return shell_spec(5, 64, 64, *SHELL[robot])
    if scene == "cluster":
        return _cluster_spec(oracle, robot)
    if scene == "pebble":
        return _pebble_spec(oracle, robot)
    assert scene == "ill-formed"
    return _ill_formed_spec(robot)


def _batches(oracle, robot, scene):
    """{name: configurations} of one (robot, scene)"""
    seed = sum(map(ord, robot + scene))
    out = {}
    for n in SIZES:
        q = _uniform(oracle, robot, n, seed + n)
        if scene in ("cluster", "pebble"):  # every other row near the anchor: lanes that do reach the obstacles
            q0 = _anchor(oracle, robot)[0]
            near = (q0 + np.random.default_rng(seed + n + 1).normal(0, 0.04, q.shape)).astype(np.float32)
            q[::2] = near[::2]
        out[f"n{n}"] = q
    if robot in EVERYWHERE and scene in ("shell64", "cluster", "pebble"):
        q0, _, far = _anchor(oracle, robot)
        if scene == "shell64":  # a valid configuration and one that collides with the scene only, 64 times each
            q = _uniform(oracle, robot, 400, seed + 5)
            rid = oracle.robot(robot)
            want = oracle.validate_batch(rid, build_oracle_env(oracle, _spec(oracle, robot, scene)), q, threads=8).astype(bool)
            no_self = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
            out["same_valid"] = np.tile(q[np.nonzero(want)[0][0]], (64, 1))
            out["same_invalid"] = np.tile(q[np.nonzero(no_self & ~want)[0][0]], (64, 1))
        else:
            out["same_touching"] = np.tile(q0, (64, 1))
            for name, at in (("touch_lane0", 0), ("touch_lane63", 63), ("touch_lane20", 20)):
                out[name] = np.insert(far, at, q0, axis=0)
    if scene == "shell64":
        q = _uniform(oracle, robot, 257, seed + 9)
        q[100, 2] = np.nan  # bit 36 of word 1
        out["nonfinite"] = q
    return out


def _env_stage(vamp, robot, env, q):
    """vmv_validate_batch_env -> the validity words"""
    import torch

    n = q.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    tw = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")  # (the stage must write every word)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = vamp.lib.vmv_validate_batch_env(vamp.lib.vmv_robot_id(robot.encode()), env.handle(), ctypes.c_void_p(tq.data_ptr()), n,
                                         ctypes.c_void_p(tw.data_ptr()), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return tw.cpu().numpy().view(np.uint64)


MULTI_COUNTS = [37, 100, 91]  # segments of the multi-environment call: they start at bits 0, 37 and 9 of their words
MULTI_SCENES = ["shell64", "mixed", "cluster"]


def _multi_configs(oracle, robot):
    q = _uniform(oracle, robot, sum(MULTI_COUNTS), 4242)
    q0 = _anchor(oracle, robot)[0]
    q[-91::3] = (q0 + np.random.default_rng(5).normal(0, 0.04, q[-91::3].shape)).astype(np.float32)
    return q


def _child(out_path):
    """every case's words on the instance this process selects (run with VMV_FINE_PAIRS=0 by the fixture below)"""
    sys.path.insert(0, ROOT)
    import vamp_mvt_amd as vamp
    from oracle_lib import Oracle

    oracle = Oracle()
    vamp.set_device(0)
    res = {}
    for robot, scenes in SCENES.items():
        for scene in scenes:
            env = build_product_env(_spec(oracle, robot, scene))
            for name, q in _batches(oracle, robot, scene).items():
                res[f"{robot}/{scene}/{name}"] = _env_stage(vamp, robot, env, q)
    for robot in EVERYWHERE:
        envs = [build_product_env(_spec(oracle, robot, s)) for s in MULTI_SCENES]
        res[f"{robot}/multi"] = getattr(vamp, robot).validate_batch_multi(_multi_configs(oracle, robot), envs, MULTI_COUNTS)
    np.savez(out_path, **res)


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """the packed instance's words of every case, from one child process with VMV_FINE_PAIRS=0"""
    out = str(tmp_path_factory.mktemp("fine_pairs") / "packed.npz")
    env = dict(os.environ, VMV_FINE_PAIRS="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, check=True, timeout=600, cwd=ROOT)
    return dict(np.load(out))


def test_entry_list_capacity_is_what_the_cluster_scene_assumes():
    with open(os.path.join(ROOT, "vamp_mvt_amd", "csrc", "vmv_device.h")) as f:
        text = f.read()
    assert "constexpr int kPairEntries = kWave;" in text and "constexpr int kWave = 64;" in text
    assert "constexpr float kCandidateMargin = 1e-4f;" in text


@pytest.mark.parametrize("robot", EVERYWHERE)
def test_cluster_scene_overflows_the_entry_list_of_one_lane(oracle, robot):
    """counted on the CPU with the oracle's FK: the primitives within reach + 1e-4 of the gate's sphere at q0"""
    q0, _, _ = _anchor(oracle, robot)
    g, model = _gen_hip()
    gate = g.merged_groups(model(robot))[-1]
    c = oracle.fk_all(oracle.robot(robot), q0)[gate["bound"], :3].astype(np.float64)
    radius = float(gate["radius"])
    sph = np.array([p for kind, p in _cluster_spec(oracle, robot) if kind == "sphere"], np.float64)
    cub = np.array([p for kind, p in _cluster_spec(oracle, robot) if kind == "cuboid"], np.float64)
    near_spheres = int((np.linalg.norm(sph[:, :3] - c, axis=1) - sph[:, 3] - radius < MARGIN).sum())
    d = c - cub[:, :3]
    loc = np.stack([(d * cub[:, 3 + 3 * i:6 + 3 * i]).sum(1) for i in range(3)], 1)
    near_cuboids = int((np.linalg.norm(np.maximum(np.abs(loc) - cub[:, 12:15], 0.0), axis=1) - radius < MARGIN).sum())
    print(robot, "candidates of the lane at q0: spheres", near_spheres, "z-cuboids", near_cuboids, "entry list", PAIR_ENTRIES)
    assert near_spheres > PAIR_ENTRIES            # one lane's candidates of ONE list: two fills, whoever else passes
    assert near_spheres + near_cuboids <= 4 * 32  # and the scene still fits the candidate words
    assert len(sph) == 96 and len(cub) == 28


CASES = [(robot, scene) for robot, scenes in SCENES.items() for scene in scenes]


@pytest.mark.parametrize("robot,scene", CASES)
def test_pairs_equal_packed_rounds_and_the_oracle(vamp, oracle, packed, robot, scene):
    spec = _spec(oracle, robot, scene)
    env, oenv = build_product_env(spec), build_oracle_env(oracle, spec)
    rid = oracle.robot(robot)
    reached = False
    for name, q in _batches(oracle, robot, scene).items():
        n = q.shape[0]
        words = _env_stage(vamp, robot, env, q)
        old = packed[f"{robot}/{scene}/{name}"]
        assert words.shape == old.shape and np.array_equal(words, old), (robot, scene, name)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
        assert not bits[n:].any(), (robot, scene, name)  # nothing set beyond n
        finite = np.isfinite(q).all(axis=1)
        assert not bits[:n][~finite].any()
        idx = np.nonzero(finite)[0]
        want = oracle.validate_batch(rid, oenv, q[idx], threads=8).astype(bool)
        no_self = oracle.validate_batch(rid, oracle.env(), q[idx], threads=8).astype(bool)
        assert np.array_equal(bits[idx] & no_self, want), (robot, scene, name, int(((bits[idx] & no_self) != want).sum()))
        reached |= bool((no_self & ~want).any())
        if name.startswith("touch_lane"):
            at = int(name[len("touch_lane"):])
            assert not bits[at] and bits[:n].sum() == n - 1, (robot, scene, name)  # the touching lane alone
        if name in ("same_touching", "same_invalid"):
            assert not bits[:n].any()
        if name == "same_valid":
            assert bits[:n].all()
    if scene != "empty":
        assert reached, "no configuration of any batch collides with the scene"


@pytest.mark.parametrize("robot", EVERYWHERE)
def test_multi_environment_call_with_segments_inside_words(vamp, oracle, packed, robot):
    specs = [_spec(oracle, robot, s) for s in MULTI_SCENES]
    envs = [build_product_env(s) for s in specs]
    q = _multi_configs(oracle, robot)
    mod = getattr(vamp, robot)
    got = mod.validate_batch_multi(q, envs, MULTI_COUNTS)
    offs = np.concatenate([[0], np.cumsum(MULTI_COUNTS)])
    assert offs[1] % 64 != 0 and offs[2] % 64 != 0
    per_scene = np.concatenate([mod.validate_batch(q[a:b], e) for e, a, b in zip(envs, offs[:-1], offs[1:])])
    assert np.array_equal(got, per_scene)
    assert np.array_equal(got, packed[f"{robot}/multi"])
    rid = oracle.robot(robot)
    want = np.concatenate([oracle.validate_batch(rid, build_oracle_env(oracle, s), q[a:b], threads=8)
                           for s, a, b in zip(specs, offs[:-1], offs[1:])]).astype(bool)
    assert np.array_equal(got, want)
    assert got.any() and not got.all()


@pytest.mark.parametrize("robot", EVERYWHERE)
def test_ill_formed_scene_keeps_the_variant_with_the_reference_groups(vamp, oracle, robot):
    env = build_product_env(_ill_formed_spec(robot))
    part = env.robot_part(getattr(vamp, robot))
    assert all(g is None for g in part["grids"])  # no broad-phase grid: the full sorted loops of the kEnvFull variant


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
