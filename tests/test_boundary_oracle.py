"""The boundary generators and the oracle at the exact fp32 contact boundary, on the CPU.

Pairs of configurations one fp32 step apart that straddle the oracle's answer must straddle a real geometric contact:
float64 clearance (geom64.py, on the oracle's own fp32 FK spheres) within FLIP_TOL of zero.  The oracle is a restatement
of the reference; this is the check it cannot fake.  Away from the boundary the oracle must agree with float64
geometry outright."""
import numpy as np
import pytest

import boundary
import geom64
from envs import build_oracle_env, counted_spec, spec_for
from workmix import case_seed, mixed_configs

ROBOTS = ["panda", "ur5", "fetch", "baxter"]
KINDS = ["cage", "mixed", "heightfield", "attach", "counted"]
FLIP_TOL = 1e-6  # metres: measured flips sit within 3e-7 on every robot; the tightest kernel margin is 1e-4
AWAY = 1e-5


def spec_of(kind, name):
    return counted_spec(name, (8, 8, 8, 8, 8), seed=3) if kind == "counted" else spec_for(kind, name)


_CACHE = {}


def pairs_for(oracle, name, kind, n=48):
    key = (name, kind)
    if key not in _CACHE:
        spec = spec_of(kind, name)
        oenv = build_oracle_env(oracle, spec)
        _CACHE[key] = (spec, oenv, boundary.boundary_configs(oracle, name, oenv, n, case_seed(name, kind, "boundary"), spec))
    return _CACHE[key]


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("kind", KINDS + ["capt"])
def test_pairs_straddle_the_oracle_one_step_apart(oracle, name, kind):
    spec, oenv, bp = pairs_for(oracle, name, kind)
    rid = oracle.robot(name)
    assert len(bp.q_lo) == 48
    assert oracle.validate_batch(rid, oenv, bp.q_lo, threads=8).all()
    assert not oracle.validate_batch(rid, oenv, bp.q_hi, threads=8).any()
    adjacent = bp.t_hi == np.nextafter(bp.t_lo, np.float32(2))
    mid = ((bp.t_lo + bp.t_hi) * np.float32(0.5)).astype(np.float32)
    q_mid = (bp.a + mid[:, None] * bp.d).astype(np.float32)
    same = np.all(q_mid == bp.q_lo, axis=1) | np.all(q_mid == bp.q_hi, axis=1)
    assert np.all(adjacent | same)
    assert np.all(bp.t_lo < bp.t_hi)


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("kind", KINDS)
def test_flips_sit_at_a_real_contact(oracle, name, kind):
    """every pair's labelled contact is within FLIP_TOL of touching at q_hi, and nothing penetrates at q_lo; a heightfield
    flip may instead sit on a cell border (the reference's test is a step function of the centre)"""
    spec, oenv, bp = pairs_for(oracle, name, kind)
    lo_min = geom64.min_clearance(bp.clear_lo)
    assert lo_min.min() > -FLIP_TOL, (bp.label[np.argmin(lo_min)], lo_min.min())
    at = np.array([bp.clear_hi[k][i] for i, k in enumerate(bp.label)])
    border = np.zeros(len(at), bool)
    if kind == "heightfield":
        hf = bp.label == "heightfield"
        lo_hf = bp.clear_lo["heightfield"]
        assert np.all(at[hf] <= FLIP_TOL) and np.all(lo_hf[hf] >= -FLIP_TOL)
        moved = np.any(geom64.heightfield_cells(oracle, name, spec, bp.q_lo) !=
                       geom64.heightfield_cells(oracle, name, spec, bp.q_hi), axis=1)
        border = hf & moved
    bad = ~border & (np.abs(at) > FLIP_TOL)
    assert not bad.any(), list(zip(bp.label[bad], at[bad]))


@pytest.mark.parametrize("name", ROBOTS)
def test_cloud_flips_have_a_point_in_reach(oracle, name):
    """one-sided for point clouds (the reference's CAPT misses some contacts, test_known_answers.py): every cloud-labelled
    invalid configuration has a point within r + r_point, and no valid one penetrates anything else"""
    for kind in ("capt",):
        spec, oenv, bp = pairs_for(oracle, name, kind)
        cloud = bp.label == "capt"
        assert np.all(bp.clear_hi["capt"][cloud] <= FLIP_TOL)
        others = {k: v for k, v in bp.clear_lo.items() if k not in geom64.CLOUD_KINDS}
        assert geom64.min_clearance(others).min() > -FLIP_TOL


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("kind", ["cage", "mixed", "heightfield", "attach", "empty"])
def test_oracle_matches_float64_away_from_the_boundary(oracle, name, kind):
    """uniform and workmix configurations with |clearance| > 1e-5 m: the oracle's answer is clearance > 0"""
    spec = spec_of(kind, name)
    oenv = build_oracle_env(oracle, spec)
    rid = oracle.robot(name)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(case_seed(name, kind, "away") % 100000)
    uni = (lo + span * rng.random((150, len(lo)), dtype=np.float32)).astype(np.float32)
    _, mix, _ = mixed_configs(oracle, name, oenv, 250, case_seed(name, kind, "away-mixed"))
    q = np.concatenate([uni, mix])
    c = geom64.min_clearance(geom64.clearances(oracle, name, spec, q))
    far = np.abs(c) > AWAY
    assert far.sum() > 0.9 * len(q)
    got = oracle.validate_batch(rid, oenv, q, threads=8)
    assert np.array_equal(got[far], c[far] > 0)


def test_exact_tangencies_are_free(oracle):
    """+0.0 is free under the reference's sign-bit rule: every exactly representable tangency, and a radius just
    above it collides"""
    spec, s = boundary.tangency_spec_and_spheres()
    oenv = build_oracle_env(oracle, spec)
    for row in s:
        assert not boundary.sphere_collides(oracle, oenv, row[:3], row[3]), row
        assert boundary.sphere_collides(oracle, oenv, row[:3], row[3] * np.float32(1.0001)), row
    hit, free = boundary.boundary_spheres(oracle, oenv, s[:, :3])
    assert len(hit) == len(s)
    assert np.all(free[:, 3] >= s[:, 3])


@pytest.mark.parametrize("kind", ["counted", "heightfield", "mixed"])
def test_radius_flips_sit_at_a_real_contact(oracle, kind):
    """free spheres at the smallest colliding fp32 radius: float64 clearance within FLIP_TOL of zero"""
    spec = spec_of(kind, "panda")
    oenv = build_oracle_env(oracle, spec)
    centres = boundary.boundary_centres(spec, case_seed("radius", kind) % 100000)
    hit, free = boundary.boundary_spheres(oracle, oenv, centres)
    assert len(hit) > 0.5 * len(centres)
    for s, want in ((hit, True), (free, False)):
        got = [boundary.sphere_collides(oracle, oenv, x[:3], x[3]) for x in s]
        assert all(g == want for g in got)
    parts, _ = geom64.env_parts(spec)
    c = geom64.env_clearance(parts, hit[:, :3], hit[:, 3])
    c = np.min(np.stack(list(c.values())), axis=0)
    assert np.abs(c).max() < FLIP_TOL, np.abs(c).max()
