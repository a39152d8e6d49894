"""The oracle and the product's host paths against the COMPILED REFERENCE (CPU only).

tests/golden/ref_{mvt,capt,scdf,centervox}.npz hold what the reference's own collision/mvt.hh, capt.hh, filter.hh and
filter_centervox.hh answered (compiled in place by oracle/ref_cloud.cc; made by tools/make_cloud_golden.py from the
inputs of tests/cloud_pins.py).  Every other point-cloud test compares HIP with oracle/vamp_oracle.c; these compare the
oracle itself, and the host builders, with the reference, so a misreading of those headers cannot hide in both.

A CAPT or scdf case is a PIN only where two opposite orders of equal sort keys gave identical bytes (`tie_dependent`
false): the reference's own unstable sort leaves nothing else open.  Flagged cases are compared with the stable-order
variant, which is the order the oracle keeps."""
import ctypes
import os
import sys

import numpy as np
import pytest

import cloud_pins as cp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import make_cloud_golden as gen  # noqa: E402

_bits, built, check_capt_arrays = cp.bits, cp.built, cp.check_capt_arrays


# ---- MVT ----------------------------------------------------------------------------------------------------------------
def product_mvt_info(pts, params):
    """vmv_env_add_mvt_pointcloud + vmv_env_mvt_info on a handle that is never finalized: the host builder alone"""
    from vamp_mvt_amd._lib import lib
    fp = ctypes.POINTER(ctypes.c_float)
    h = ctypes.c_void_p()
    lib.vmv_env_create(ctypes.byref(h))
    reason = ctypes.c_int(0)
    p = np.ascontiguousarray(pts, np.float32)
    lo, hi = np.array(params[2], np.float32), np.array(params[3], np.float32)
    rc = lib.vmv_env_add_mvt_pointcloud(h, p.ctypes.data_as(fp), len(p), params[0], params[1], lo.ctypes.data_as(fp),
                                        hi.ctypes.data_as(fp), params[4], None, ctypes.byref(reason))
    info = None
    if rc == 0:
        gw, cap, nv, isf, box = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_float(), (ctypes.c_float * 6)()
        lib.vmv_env_mvt_info(h, 0, ctypes.byref(gw), ctypes.byref(cap), ctypes.byref(nv), ctypes.byref(isf), box)
        info = (gw.value, cap.value, nv.value, np.array([isf.value, *box], np.float32))
    lib.vmv_env_destroy(h)
    return rc, reason.value, info


@pytest.mark.parametrize("name", cp.names("mvt"))
def test_mvt_build_equals_reference(vamp, oracle, name):
    """built / terminated, grid width, per-voxel capacity, occupied voxels, inverse scale factor and global box: the
    oracle's and the product's host builder's == the reference constructor's"""
    case = cp.cases("mvt")[name]
    m = case.meta
    e = oracle.env()
    reason = e.add_mvt(case.pts, *case.params)
    rc, product_reason, info = product_mvt_info(case.pts, case.params)
    assert (reason == 0) == (m["status"] == "built") and product_reason == reason
    if m["status"] != "built":
        assert rc == 4 and m["what"]  # VMV_ERR_CAPACITY where the reference printed what() and terminated
        return
    want = case.out("info")
    o = e.mvt(0)
    assert (o["grid_width"], o["capacity"], o["n_voxels"]) == (m["grid_width"], m["capacity"], m["n_voxels"])
    assert np.array_equal(_bits(np.array([o["inverse_scale_factor"], *o["global_box"]], np.float32)), _bits(want))
    assert rc == 0 and info[:3] == (m["grid_width"], m["capacity"], m["n_voxels"])
    assert np.array_equal(_bits(info[3]), _bits(want))


@pytest.mark.parametrize("name", cp.names("mvt", built))
def test_oracle_mvt_queries_equal_reference(oracle, name):
    """every scalar answer == MVT::collides, every 8-lane rake == MVT::collides_simd"""
    case = cp.cases("mvt")[name]
    q = cp.queries(case)
    e = oracle.env()
    assert e.add_mvt(case.pts, *case.params) == 0
    s = q["scalar"]
    got = np.array([e.mvt_collides(s[i, :3], s[i, 3]) for i in range(len(s))])
    want = case.out("hits", len(s))
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    r = q["rakes"]
    got = np.array([e.mvt_collides_simd(r[j, :, 0], r[j, :, 1], r[j, :, 2], r[j, :, 3]) for j in range(len(r))])
    assert np.array_equal(got, case.out("rake_hits", len(r)))


# ---- CAPT ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cp.names("capt", lambda m: m["seeded"]))
def test_oracle_capt_equals_reference(vamp, oracle, name):
    """nlog2, every array bit for bit (oracle and the product's host build), every scalar, single-sphere and rake
    answer.  `tied_x_panda` is tie_dependent: it holds the stable-order variant, which the oracle keeps."""
    case = cp.cases("capt")[name]
    q = cp.queries(case)
    e = oracle.env()
    e.add_capt(case.pts, *case.params)
    check_capt_arrays(case, e.capt(0))
    pe = vamp.Environment()
    if len(case.pts) < 2:
        # The reference builds a one-leaf tree that CAPT::collides answers (pinned above and below through the oracle),
        # but the query its environment check uses, collides_simd, reads tests[0] of an empty vector there: the product
        # refuses such a cloud instead of inventing an answer.
        with pytest.raises(vamp.VmvError) as ei:
            pe.add_capt_pointcloud(case.pts, *case.params, build="host")
        assert ei.value.status == 1  # VMV_ERR_INVALID_ARGUMENT
    else:
        pe.add_capt_pointcloud(case.pts, *case.params, build="host")
        check_capt_arrays(case, pe.host_tables()["capt"][0])
    s, r = q["scalar"], q["rakes"]
    got = np.array([e.capt_collides(s[i, :3], s[i, 3]) for i in range(len(s))])
    assert np.array_equal(got, case.out("hits", len(s))), np.nonzero(got != case.out("hits", len(s)))[0][:10]
    if not case.meta["simd"]:  # one point: the reference's collides_simd is undefined there (no tests to read)
        return
    got = np.array([e.capt_collides_simd(s[i:i + 1, 0], s[i:i + 1, 1], s[i:i + 1, 2], s[i:i + 1, 3]) for i in range(len(s))])
    assert np.array_equal(got, case.out("solo_hits", len(s))), np.nonzero(got != case.out("solo_hits", len(s)))[0][:10]
    got = np.array([e.capt_collides_simd(r[j, :, 0], r[j, :, 1], r[j, :, 2], r[j, :, 3]) for j in range(len(r))])
    assert np.array_equal(got, case.out("rake_hits", len(r)))


@pytest.mark.parametrize("name", cp.names("capt", lambda m: not m["seeded"]))
def test_oracle_capt_survey_cloud_equals_reference(oracle, name):
    """The survey's 10,000-point cloud in both roundings at the three robots' radii, by shape and digest: 24,169 /
    177,408 / 873,895 affordance vectors with the survey driver's fused multiply-adds and 873,894 at Baxter's radii
    without them, now from the compiled reference instead of the survey's note.  At the Fetch and Baxter radii the
    order of the points inside `aff` follows the order of three repeated coordinates (cloud_pins.TIE_EXEMPT): that
    digest is the stable-order variant's, everything else is the same under both orders."""
    case = cp.cases("capt")[name]
    e = oracle.env()
    e.add_capt(case.make_pts(), *case.params)
    check_capt_arrays(case, e.capt(0))


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cp.names("scdf"))
def test_oracle_scdf_equals_reference(oracle, name):
    case = cp.cases("scdf")[name]
    got = oracle.filter_scdf(case.pts, *case.args)
    want = case.out("kept")
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", cp.names("centervox"))
def test_oracle_centervox_equals_reference(oracle, name):
    """kept points in the reference's order; None where the reference threw (pool exhausted)"""
    case = cp.cases("centervox")[name]
    pts = case.pts if case.pts is not None else cp.exhaustion_cloud()
    got = oracle.filter_centervox(pts, *case.args)
    if case.meta["status"] != "built":
        assert got is None and case.meta["what"] == "Voxel pool exhausted"
        return
    want = case.out("kept")
    assert got is not None and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


# ---- the fixtures themselves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mvt", "capt", "scdf", "centervox"])
def test_fixtures_are_current(family):
    """regenerated in memory from the compiled reference == the committed file, key for key"""
    if not gen.available():
        pytest.skip("oracle/_ref/libref_cloud.so not built (needs the reference at build time)")
    assert gen.differences(family) == []


def test_fixtures_are_not_degenerate():
    """what the generator asserted, asserted again on the committed files: a regenerated fixture cannot go quietly
    degenerate"""
    for family in ("capt", "scdf"):
        meta = cp.load(family)[0]["cases"]
        flagged = [m["name"] for m in meta if m["tie_dependent"]]
        counted = [n for n in flagged if n not in cp.TIE_EXEMPT[family]]
        assert 1 <= len(counted) <= cp.MAX_TIE_DEPENDENT, counted       # one on purpose, never more than the cap
        assert set(flagged) - set(counted) <= set(cp.TIE_EXEMPT[family])
        assert sum(not m["tie_dependent"] for m in meta) >= 15          # the pins proper
    for m in cp.load("capt")[0]["cases"]:
        if not m["seeded"]:
            assert set(m["tie_dependent_outputs"]) <= {"aff"}, m["name"]
    for family in ("mvt", "capt"):
        for name, case in cp.cases(family).items():
            m = case.meta
            if "hit_rate" not in m:
                continue
            n = cp.N_SCALAR[family]
            hits = case.out("hits", n)
            assert 0.2 <= hits.mean() <= 0.8 and abs(hits.mean() - m["hit_rate"]) < 1e-4, name
            lo, hi = m["knife"]
            q = dict(knife=(lo, hi), expect=case.out("expect", hi - lo),
                     sites=(m["knife_sites"]["live"] + m["knife_sites"]["dead"], 0))
            if family == "capt":  # four-query sites first, then the two-query top-box sites
                q = cp.queries(case)
            sites = cp.knife_report(hits, q)
            assert sites == m["knife_sites"] and sites["other"] == 0, name
            # both answers at the boundary: hit at equality, miss one step beyond
            assert sites["live"] >= (32 if family == "mvt" or m["n"] >= 17 else 1), name
            assert family == "capt" or sites["dead"] == 0, name
    mvt = cp.load("mvt")[0]["cases"]
    assert {m["status"] for m in mvt} == {"built", "terminated"}
    assert {m["what"] for m in mvt if m["status"] == "terminated"} == {
        "Voxel capacity exceeded", "Voxel index pool exhausted", "Point coordinate pool exhausted"}
    for name in ("ref_mvt", "ref_capt", "ref_scdf", "ref_centervox"):
        assert os.path.getsize(os.path.join(cp.GOLDEN, name + ".npz")) <= gen.MAX_FIXTURE_BYTES
