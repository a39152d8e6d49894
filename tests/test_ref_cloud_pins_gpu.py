"""The HIP point-cloud paths against the COMPILED REFERENCE, directly (GPU).

These read tests/golden/ref_{mvt,capt,scdf,centervox}.npz only: what the reference's own collision/mvt.hh, capt.hh,
filter.hh and filter_centervox.hh answered for the inputs of tests/cloud_pins.py (see tests/test_ref_cloud_pins.py for
the CPU half and the meaning of `tie_dependent`).  No oracle stands between the HIP code and the reference here.

`Environment.spheres_in_collision` treats each sphere as its own replicated rake, so it is compared with
CAPT::collides_simd on eight copies of the sphere (`solo_hits`): collides_simd tests the top box per axis and
CAPT::collides by distance, and the two differ at the box's corners.  MVT::collides and collides_simd agree lane for
lane, so the MVT is compared with the scalar answers.  An 8-lane rake is the OR of its spheres' answers."""
import numpy as np
import pytest

import cloud_pins as cp
from cloud_pins import bits as _bits, built, check_capt_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)
    return vamp


def check_queries(env, case, scalar_key):
    q = cp.queries(case)
    s, r = q["scalar"], q["rakes"]
    got = env.spheres_in_collision(s)
    want = case.out(scalar_key, len(s))
    assert np.array_equal(got, want), (case.name, np.nonzero(got != want)[0][:10])
    got = env.spheres_in_collision(r.reshape(-1, 4)).reshape(-1, 8).any(1)
    want = case.out("rake_hits", len(r))
    assert np.array_equal(got, want), (case.name, np.nonzero(got != want)[0][:10])


@pytest.mark.parametrize("name", cp.names("mvt", built))
def test_gpu_mvt_queries_equal_reference(device, name):
    """an environment holding only this cloud: every sphere == MVT::collides, every rake == MVT::collides_simd"""
    case = cp.cases("mvt")[name]
    env = device.Environment()
    env.add_mvt_pointcloud(case.pts, *case.params)
    check_queries(env, case, "hits")


@pytest.mark.parametrize("name", cp.names("mvt", lambda m: not built(m)))
def test_gpu_mvt_capacity_where_reference_terminates(device, name):
    case = cp.cases("mvt")[name]
    with pytest.raises(device.VmvError) as ei:
        device.Environment().add_mvt_pointcloud(case.pts, *case.params)
    assert ei.value.status == 4  # VMV_ERR_CAPACITY


@pytest.mark.parametrize("build", ["gpu", "host"])
@pytest.mark.parametrize("name", cp.names("capt", lambda m: m["seeded"]))
def test_gpu_capt_equals_reference(device, name, build):
    """device-built and host-built arrays bit for bit, then the query on each: the query's copy of the tree, the
    distance grid, blocked planes and two gates in flight, against the reference itself"""
    case = cp.cases("capt")[name]
    env = device.Environment()
    if not case.meta["simd"]:
        # one point: the reference's collides_simd, the query its environment check uses, is undefined there (it reads
        # tests[0] of an empty vector), so both builders refuse the cloud (tests/test_ref_cloud_pins.py pins the tree
        # and CAPT::collides through the oracle)
        with pytest.raises(device.VmvError) as ei:
            env.add_capt_pointcloud(case.pts, *case.params, build=build)
        assert ei.value.status == 1  # VMV_ERR_INVALID_ARGUMENT
        return
    env.add_capt_pointcloud(case.pts, *case.params, build=build)
    check_capt_arrays(case, env.host_tables()["capt"][0])
    check_queries(env, case, "solo_hits")


@pytest.mark.parametrize("build", ["gpu", "host"])
@pytest.mark.parametrize("name", cp.names("capt", lambda m: not m["seeded"]))
def test_gpu_capt_survey_cloud_equals_reference(device, name, build):
    """the survey's 10,000-point cloud by shape and digest (see test_oracle_capt_survey_cloud_equals_reference)"""
    case = cp.cases("capt")[name]
    env = device.Environment()
    env.add_capt_pointcloud(case.make_pts(), *case.params, build=build)
    check_capt_arrays(case, env.host_tables()["capt"][0])


@pytest.mark.parametrize("name", cp.names("scdf"))
def test_gpu_scdf_equals_reference(device, name):
    case = cp.cases("scdf")[name]
    min_dist, max_range, origin, lo, hi, cull = case.args
    got, _ = device.filter_pointcloud(case.pts, min_dist, max_range, 0.03, origin, lo, hi, cull, "scdf")
    want = case.out("kept")
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", cp.names("centervox"))
def test_gpu_centervox_equals_reference(device, name):
    """kept points in the reference's order; VMV_ERR_CAPACITY where the reference threw"""
    case = cp.cases("centervox")[name]
    pts = case.pts if case.pts is not None else cp.exhaustion_cloud()
    vs, max_range, origin, lo, hi = case.args
    if case.meta["status"] != "built":
        with pytest.raises(device.VmvError) as ei:
            device.filter_pointcloud(pts, 0.0, max_range, vs, origin, lo, hi, True, "centervox")
        assert ei.value.status == 4
        return
    got, _ = device.filter_pointcloud(pts, 0.0, max_range, vs, origin, lo, hi, True, "centervox")
    want = case.out("kept")
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
