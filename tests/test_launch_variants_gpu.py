"""The launchers pick every validation kernel from a table indexed by the environment's class (csrc/vmv_robot_launch.inc;
classes Z = kEnvZOnly, P = kEnvPrims, F = kEnvFull, C = kEnvClouds).  Where each entry is reached with real work:

  configurations, one environment [pair-dealt][class]: test_gpu_parity.test_validate_batch_bit_exact, kinds empty / cage /
      shell64 (Z), mixed (P), capt / heightfield (F), clouds (C), attach (the attachment kernel); Panda and UR5 take the
      pair-dealt row there, Fetch and Baxter the plain one; the plain Z and P on Panda and UR5:
      test_fine_pairs_gpu.test_pairs_equal_packed_rounds_and_the_oracle (its child process runs with VMV_FINE_PAIRS=0);
  configurations, many environments [pair-dealt][class | attachment]: test_multi_env_gpu.test_multi_is_bit_identical_..
      (every kind in one call: all five columns on UR5, pair-dealt row, and on Fetch, plain row); P in both rows on
      Panda and UR5: test_fine_pairs_gpu.test_multi_environment_call_with_segments_inside_words;
  edges, one environment [fused][class]: test_gpu_parity.test_edge_schedules_are_bit_exact, VMV_EDGE_TASKS=1 (two kernels:
      shell64 Z, mixed P, capt / heightfield F, clouds C) and 3 (fused Z and P on Panda and UR5), kind attach (the walk);
  edges, many environments [first, later pass][class]: test_multi_env_motion_gpu.test_multi_is_bit_identical_.. (Z, P, F
      and the attachment walk with hundreds of edges on Panda).

What those leave out is C in the two multi-environment calls: test_multi_env_gpu.py draws an EMPTY cloud-only segment for
Panda, and test_multi_env_motion_gpu.py draws 9 cloud-only edges for Panda and 1 for UR5, which can leave the later pass
without a task.  These are the cases here.

Three segments of 130 items - two full validity words and a partial one, so both boundaries fall inside a word: the
cloud-only scene, an EMPTY segment on a primitive scene, the scene with an attachment.  Bit for bit against the oracle."""
import numpy as np
import pytest
from envs import make_env
from workmix import case_seed, mixed_configs, mixed_edges

pytestmark = pytest.mark.gpu

N = 130
KINDS = ["clouds", "mixed", "attach"]
COUNTS = [N, 0, N]


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


@pytest.fixture(scope="module", params=["panda", "ur5"])
def scenes(request, oracle):
    robot = request.param
    made = [make_env(k, oracle, robot) for k in KINDS]
    return robot, [e for e, _ in made], [o for _, o in made]


def test_cloud_only_segment_of_a_configuration_batch(vamp, oracle, scenes):
    robot, envs, oenvs = scenes
    parts = [mixed_configs(oracle, robot, oenvs[k], N, case_seed("launch-variants", robot, KINDS[k], "configs")) for k in (0, 2)]
    q = np.concatenate([p[1] for p in parts])
    want = np.concatenate([p[2] for p in parts]).astype(bool)
    for w in (want[:N], want[N:]):
        assert w.any() and not w.all(), "degenerate segment"
    got = getattr(vamp, robot).validate_batch_multi(q, envs, COUNTS)
    assert got.dtype == bool and np.array_equal(got, want)


def test_cloud_only_segment_of_an_edge_batch(vamp, oracle, scenes):
    robot, envs, oenvs = scenes
    parts = [mixed_edges(oracle, robot, oenvs[k], N, case_seed("launch-variants", robot, KINDS[k], "edges"), zero_every=7)
             for k in (0, 2)]
    a, b = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    want = np.concatenate([p[3] for p in parts]).astype(bool)
    for w in (want[:N], want[N:]):  # valid edges of more than one rake: the later pass has tasks in both classes
        assert w.any() and not w.all(), "degenerate segment"
    got = getattr(vamp, robot).validate_motion_batch_multi(a, b, envs, COUNTS)
    assert got.dtype == bool and np.array_equal(got, want)
