"""The max_extent test of the pair-dealt fine phase (vmv_device.h within_extent) where its shortcut must not decide: a
pair whose min_distance lies within 1e-6 of the sphere's max_extent takes the correctly rounded root, every other pair
the bare one.  Scene per robot: one obstacle sphere placed radially beyond the robot sphere that reaches farthest from
the origin at a configuration q0, tangent to it, so that for that pair min_distance - max_extent and the sphere-sphere
test value are both zero to rounding; 293 configurations spread around q0 from 1e-8 to 1e-3 rad, which move the robot
sphere through the contact and the pair in and out of the band.  The environment stage's words equal the packed
instance's (VMV_FINE_PAIRS=0: the candidate walks, which this change leaves alone; one child process) and the oracle's
answers, both answers occur, and the band is reached (counted on the CPU in float64)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from envs import build_oracle_env, build_product_env

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
ROBOTS = ["panda", "ur5"]
N = 256 + 37
R_OBSTACLE = 0.02


def _scene(oracle, robot):
    """-> (spec, configurations, rows inside the band)"""
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(sum(map(ord, robot)))
    q = (lo + span * rng.random((400, len(lo)), dtype=np.float32)).astype(np.float32)
    ok = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
    best = None
    for c in q[ok]:
        s = oracle.fk(rid, c).astype(np.float64)
        ext = np.linalg.norm(s[:, :3], axis=1) + s[:, 3]
        order = np.argsort(ext)
        if best is None or ext[order[-1]] - ext[order[-2]] > best[0]:  # the farthest sphere stands well clear of the next
            best = (ext[order[-1]] - ext[order[-2]], c, int(order[-1]))
    _, q0, si = best
    s0 = oracle.fk(rid, q0).astype(np.float64)[si]
    dist = np.linalg.norm(s0[:3])
    centre = s0[:3] / dist * (dist + s0[3] + R_OBSTACLE)
    spec = [("sphere", np.array([*centre, R_OBSTACLE], np.float32))]
    sigma = 10.0 ** np.linspace(-8, -3, N)
    qs = (q0[None, :] + rng.normal(size=(N, len(lo))) * sigma[:, None]).astype(np.float32)
    p = spec[0][1].astype(np.float64)
    md = np.linalg.norm(p[:3]) - p[3]
    in_band = 0
    for c in qs:
        s = oracle.fk(rid, c).astype(np.float64)[si]
        ext = np.linalg.norm(s[:3]) + s[3]
        in_band += abs(md - ext) < 5e-7 * ext
    return spec, qs, int(in_band)


def _env_stage(vamp, robot, env, q):
    import torch

    n = q.shape[0]
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    tw = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = vamp.lib.vmv_validate_batch_env(vamp.lib.vmv_robot_id(robot.encode()), env.handle(), ctypes.c_void_p(tq.data_ptr()), n,
                                         ctypes.c_void_p(tw.data_ptr()), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return tw.cpu().numpy().view(np.uint64)


def _child(out_path):
    sys.path.insert(0, ROOT)
    import vamp_mvt_amd as vamp
    from oracle_lib import Oracle

    oracle = Oracle()
    vamp.set_device(0)
    res = {}
    for robot in ROBOTS:
        spec, q, _ = _scene(oracle, robot)
        res[robot] = _env_stage(vamp, robot, build_product_env(spec), q)
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_extent") / "packed.npz")
    env = dict(os.environ, VMV_FINE_PAIRS="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, check=True, timeout=300, cwd=ROOT)
    return dict(np.load(out))


@pytest.mark.parametrize("robot", ROBOTS)
def test_pairs_at_the_extent_boundary_equal_the_packed_rounds_and_the_oracle(vamp, oracle, packed, robot):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)
    spec, q, in_band = _scene(oracle, robot)
    print(robot, "configurations with |min_distance - max_extent| < 5e-7 * max_extent:", in_band, "of", N)
    assert in_band >= 16
    words = _env_stage(vamp, robot, build_product_env(spec), q)
    assert np.array_equal(words, packed[robot])
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert not bits[N:].any()
    rid = oracle.robot(robot)
    want = oracle.validate_batch(rid, build_oracle_env(oracle, spec), q, threads=8).astype(bool)
    no_self = oracle.validate_batch(rid, oracle.env(), q, threads=8).astype(bool)
    assert np.array_equal(bits[:N] & no_self, want)
    print(robot, "valid", int(want.sum()), "of", N)
    assert 16 <= want.sum() <= N - 16  # the contact decides: both answers occur


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
