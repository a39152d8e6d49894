"""The HIP primitive narrow phase and environment loop against the COMPILED REFERENCE, directly (GPU).

The per-case tests read tests/golden/ref_prims.npz only: what the reference's own collision/validity.hh, shapes.hh,
environment.hh and sphere_*.hh answered for the environments and free spheres of tests/prim_pins.py (see
tests/test_ref_prim_pins.py for the CPU half and the meaning of `ref`, `nobreak`, `exact` and `break_decided`).  No
oracle stands between the HIP code and the reference there.

`Environment.spheres_in_collision` treats each sphere as its own replicated rake, so its answers are compared with the
per-sphere `exact` and, per rake, with the OR over the rake's eight spheres; that OR equals the rake's own `exact`
except where a lane's own break decides its answer (radial family; see
test_ref_prim_pins.rakes_where_a_lanes_own_break_decides).  The rake-wide loop of the robot kernels is compared with
the oracle's on the same scenes in test_robot_path_on_radial_and_origin_capsule_scenes."""
import ctypes

import numpy as np
import pytest

import prim_pins as pp
from envs import build_oracle_env
from test_ref_prim_pins import past_the_buffer_queries, rakes_where_a_lanes_own_break_decides
from vamp_mvt_amd.workloads import environment_from_spec
from workmix import case_seed, mixed_configs, mixed_edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)
    return vamp


def device_call(vamp, env, spheres):
    """vmv_spheres_in_collision_batch on device arrays and the current stream (spheres_in_collision goes through
    vmv_spheres_in_collision_batch_host)"""
    import torch
    s = torch.from_numpy(np.ascontiguousarray(spheres, np.float32)).cuda()
    hits = torch.zeros(len(spheres), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vamp.check(vamp.lib.vmv_spheres_in_collision_batch(env.handle(), ctypes.c_void_p(s.data_ptr()), len(spheres),
                                                       ctypes.c_void_p(hits.data_ptr()), stream), "vmv_spheres_in_collision_batch")
    torch.cuda.synchronize()
    return hits.cpu().numpy().astype(bool)


@pytest.mark.parametrize("name", pp.names())
def test_gpu_equals_reference(device, name):
    """the sorted lists the kernels are given, every sphere, every rake, through the host call and the device call"""
    case = pp.cases()[name]
    env = environment_from_spec(case.spec)
    tables, want = env.host_tables(), case.lists()
    for key in pp.LISTS:
        assert pp.same_lists(tables[key], want[key]), (name, key)
    got = env.spheres_in_collision(case.scalar)
    assert np.array_equal(got, case.want()), (name, np.nonzero(got != case.want())[0][:10])
    assert np.array_equal(device_call(device, env, case.scalar), got), name
    lanes = env.spheres_in_collision(case.rakes.reshape(-1, 4))
    assert np.array_equal(device_call(device, env, case.rakes.reshape(-1, 4)), lanes), name
    lane_or = lanes.reshape(-1, 8).any(1)
    assert np.array_equal(lane_or, case.out("lane_or", rake=True)), name
    assert np.array_equal(lane_or != case.want(rake=True), rakes_where_a_lanes_own_break_decides(case)), name


def test_gpu_heightfield_index_past_the_buffer_reads_the_last_pixel(device):
    """ys == yd, and xs == xd in the last row: the reference reads past its buffer; the product reads the last pixel,
    as the oracle does (test_ref_prim_pins.test_heightfield_index_past_the_buffer_reads_the_last_pixel)"""
    hf, spheres, want = past_the_buffer_queries()
    env = environment_from_spec([("heightfield", hf)])
    assert np.array_equal(env.spheres_in_collision(spheres), want)


def _scene(name):
    return {c["name"]: c for c in pp.all_cases()}[name]["spec"]


# (robot, scene, degenerate): a capsule through the origin always touches the base of Panda and Baxter (their first
# spheres contain the origin), so every configuration is invalid there under the rule, and `valid` would mean a break
# skipped that capsule; UR5's spheres start 0.74 above the origin, where the beam scene is an ordinary one
ROBOT_SCENES = [("panda", "radial_mixed", False), ("panda", "radial_capsule", False), ("baxter", "radial_capsule", False),
                ("ur5", "nan_beam_at_1", False), ("ur5", "nan_beam_at_2", False),
                ("panda", "nan_beam_at_1", True), ("panda", "nan_pole_at_1", True), ("panda", "zero_length_at_0", False),
                ("baxter", "nan_beam_at_1", True), ("baxter", "nan_pole_at_2", True)]


@pytest.mark.parametrize("name,scene,degenerate", ROBOT_SCENES)
def test_robot_path_on_radial_and_origin_capsule_scenes(device, oracle, name, scene, degenerate):
    """validate_batch and validate_motion_batch (the rake-wide loop, candidate words and live-prefix counts over the
    min_distance array) against the oracle on the scenes whose break decides and whose min_distance was not finite"""
    spec = _scene(scene)
    env, oenv = environment_from_spec(spec), build_oracle_env(oracle, spec)
    mod = getattr(device, name)
    rid = oracle.robot(name)
    n, m = 2000, 400
    if degenerate:
        lo, span = oracle.bounds(rid)
        rng = np.random.default_rng(case_seed(name, scene))
        q = (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)
        a, b = q[:m], q[m:2 * m]
        want, want_e = oracle.validate_batch(rid, oenv, q, threads=8), oracle.validate_motion_batch(rid, oenv, a, b, threads=8)
        assert not want.any() and not want_e.any()
    else:
        rid, q, want = mixed_configs(oracle, name, oenv, n, case_seed(name, scene, "prim-pins"))
        rid, a, b, want_e = mixed_edges(oracle, name, oenv, m, case_seed(name, scene, "prim-pin-edges"), zero_every=7)
        for w, k in ((want, n), (want_e, m)):
            assert 0.05 * k < int(w.sum()) < 0.95 * k, f"degenerate case: {int(w.sum())} of {k} valid"   # _non_degenerate
    assert np.array_equal(mod.validate_batch(q, env), want)
    assert np.array_equal(mod.validate_motion_batch(a, b, env), want_e)
