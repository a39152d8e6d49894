"""HIP path vs oracle at the exact fp32 contact boundary (tests/boundary.py): configurations, edges and free spheres one
step either side of a contact, under every switch that changes which certified-free shortcut decides them.

Every shortcut of the device path (broad-phase grid cells, fine-phase candidate words, reach certificates, the CAPT
distance grid and radius-bucket cut) is sound only by a margin; these inputs sit ~1e-7 m from the contact, far inside
every margin, so a margin that is wrong by tens of microns or a predicate that reads +0.0 as a hit fails here."""
import numpy as np
import pytest

import boundary
from envs import build_oracle_env, build_product_env, counted_spec, spec_for
from workmix import case_seed

pytestmark = pytest.mark.gpu
ROBOTS = ["panda", "ur5", "fetch", "baxter"]
KINDS = ["cage", "shell64", "mixed", "many", "capt", "clouds", "heightfield", "mvt", "attach", "empty", "counted"]
N_PAIRS = 48
# (environment, contact kind) -> fewest boundary pairs over the four robots: the kinds each environment is there for
MIN_PAIRS = {("cage", "sphere"): 60, ("shell64", "sphere"): 30, ("shell64", "z_cuboid"): 30, ("mixed", "capsule"): 10,
             ("mixed", "z_capsule"): 4, ("mixed", "cuboid"): 20, ("mixed", "z_cuboid"): 10, ("mixed", "sphere"): 6,
             ("many", "sphere"): 10, ("many", "z_cuboid"): 10, ("capt", "capt"): 40, ("clouds", "capt"): 40,
             ("heightfield", "heightfield"): 30, ("mvt", "mvt"): 40, ("attach", "attachment"): 20, ("empty", "self"): 150,
             ("counted", "sphere"): 10, ("counted", "capsule"): 10, ("counted", "z_capsule"): 10,
             ("counted", "cuboid"): 10, ("counted", "z_cuboid"): 10}
# settings of the environment build and the launchers that change which shortcut decides a contact; none may change
# an answer
SWITCHES = [{}, {"VMV_NO_GRID": "1"}, {"VMV_GRID_CELLS": "1000", "VMV_GRID_MIN_CELL": "0.09"},
            {"VMV_GRID_CELLS": "400000", "VMV_GRID_MIN_CELL": "0.013"}, {"VMV_NO_LINK_SKIP": "1"},
            {"VMV_CAPT_NO_PREFIX": "1"}, {"VMV_CAPT_NO_DIST_GRID": "1"}, {"VMV_SELF_GROUP": "1"},
            {"VMV_SELF_GROUP": "8"}]
SPHERE_SWITCHES = SWITCHES[:4] + SWITCHES[5:7]


def spec_of(kind, name):
    return counted_spec(name, (8, 8, 8, 8, 8), seed=3) if kind == "counted" else spec_for(kind, name)


def cases():
    # the "many" shell (250 primitives, 0.35 m in) leaves Fetch and Baxter no valid configuration at all
    return [(n, k) for n in ROBOTS for k in KINDS if not (k == "many" and n in ("fetch", "baxter"))]


@pytest.fixture(scope="module", autouse=True)
def _device(vamp):
    assert vamp.device_count() >= 1, "no HIP device visible"
    vamp.set_device(0)


@pytest.fixture(scope="module")
def pairs(oracle):
    """(robot, environment) -> (spec, oracle env, BoundaryPairs), generated once for the module"""
    out = {}
    for name, kind in cases():
        spec = spec_of(kind, name)
        oenv = build_oracle_env(oracle, spec)
        out[(name, kind)] = (spec, oenv, boundary.boundary_configs(oracle, name, oenv, N_PAIRS,
                                                                   case_seed(name, kind, "boundary"), spec))
    return out


def _with(monkeypatch, switch):
    for k in {k for s in SWITCHES for k in s}:
        monkeypatch.delenv(k, raising=False)
    for k, v in switch.items():
        monkeypatch.setenv(k, v)


def test_boundary_pairs_cover_every_contact_kind(pairs):
    total = {}
    for (name, kind), (_, _, bp) in pairs.items():
        for label, n in bp.counts().items():
            total[(kind, label)] = total.get((kind, label), 0) + n
    short = {k: (total.get(k, 0), m) for k, m in MIN_PAIRS.items() if total.get(k, 0) < m}
    assert not short, short


@pytest.mark.parametrize("name,kind", cases())
def test_boundary_configs_bit_exact(vamp, oracle, monkeypatch, pairs, name, kind):
    """both sides of every pair, under every switch: the oracle's answers (valid, then invalid)"""
    spec, oenv, bp = pairs[(name, kind)]
    q, want = bp.configs()
    rid = oracle.robot(name)
    assert np.array_equal(oracle.validate_batch(rid, oenv, q, threads=8), want)
    mod = getattr(vamp, name)
    for switch in SWITCHES:
        _with(monkeypatch, switch)
        env = build_product_env(spec)
        got = mod.validate_batch(q, env)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (switch, [(bool(want[i]), bp.label[i % len(bp.label)]) for i in bad[:8]])
        assert np.array_equal(mod.validate_batch(q[::-1].copy(), env), want[::-1]), switch


@pytest.mark.parametrize("name", ROBOTS)
@pytest.mark.parametrize("kind", ["shell64", "mixed", "capt", "heightfield", "attach", "counted"])
def test_boundary_edges_every_schedule(vamp, oracle, monkeypatch, pairs, name, kind):
    """edges whose length is bisected to the oracle's flip (a rake sample touching, or the rake count changing) and
    zero-length edges at the configuration pairs, under the default schedule and VMV_EDGE_TASKS 1 and 3, in ragged batches
    and in one batch large enough to leave the fused task schedule"""
    spec, oenv, bp = pairs[(name, kind)]
    rid = oracle.robot(name)
    a, b, want = boundary.boundary_edges(oracle, name, oenv, 48, case_seed(name, kind, "boundary-edges"), bp)
    assert np.array_equal(oracle.validate_motion_batch(rid, oenv, a, b, threads=8), want)
    mod = getattr(vamp, name)
    env = build_product_env(spec)
    for mode in (None, "1", "3"):
        if mode is None:
            monkeypatch.delenv("VMV_EDGE_TASKS", raising=False)
        else:
            monkeypatch.setenv("VMV_EDGE_TASKS", mode)
        assert np.array_equal(mod.validate_motion_batch(a, b, env), want), mode
        for m in (1, 7, 9, 65):
            assert np.array_equal(mod.validate_motion_batch(a[:m], b[:m], env), want[:m]), (mode, m)
    monkeypatch.delenv("VMV_EDGE_TASKS", raising=False)
    reps = 17000 // len(a) + 1  # past VMV_EDGE_FUSED_BELOW (16,384 edges): the unforced launcher's two-pass tasks
    assert np.array_equal(mod.validate_motion_batch(np.tile(a, (reps, 1)), np.tile(b, (reps, 1)), env), np.tile(want, reps))


def _far_spec(offset):
    """one cloud and a few primitives of every kind translated by `offset` metres along x and y"""
    from vamp_mvt_amd.workloads import POINT_RADIUS, RADII, shell_cloud
    spec = []
    for kind, p in counted_spec("panda", (3, 3, 3, 3, 3), seed=5):
        p = np.array(p, np.float32)
        p[0] += np.float32(offset)
        p[1] -= np.float32(offset)
        spec.append((kind, p))
    pts = shell_cloud(800, 11, 0.4, 0.9) + np.array([offset, -offset, 0], np.float32)
    spec.append(("capt", (pts.astype(np.float32), *RADII["panda"], POINT_RADIUS)))
    return spec


SPHERE_ENVS = ["counted", "cage", "mixed", "heightfield", "capt", "mvt", "tangency", "far90", "far120"]


def _sphere_spec(kind):
    if kind == "tangency":
        return boundary.tangency_spec_and_spheres()[0]
    if kind.startswith("far"):
        return _far_spec(float(kind[3:]))
    return spec_of(kind, "panda")


@pytest.mark.parametrize("kind", SPHERE_ENVS)
def test_boundary_free_spheres(vamp, oracle, monkeypatch, kind):
    """free spheres at the smallest colliding fp32 radius and one float below it, around every primitive kind, over
    heightfield cell borders, around cloud points, and beyond +-100 m (where the CAPT radius-bucket cut is switched
    off): the oracle's answers under the grid and CAPT switches"""
    spec = _sphere_spec(kind)
    oenv = build_oracle_env(oracle, spec)
    centres = boundary.boundary_centres(spec, case_seed("boundary-spheres", kind) % 100000)
    if kind == "tangency":
        _, tangent = boundary.tangency_spec_and_spheres()
        centres = np.concatenate([centres, tangent[:, :3]])
    hit, free = boundary.boundary_spheres(oracle, oenv, centres)
    s = np.concatenate([hit, free])
    want = np.r_[np.ones(len(hit), bool), np.zeros(len(free), bool)]
    if kind == "tangency":
        s = np.concatenate([s, tangent])
        want = np.r_[want, np.zeros(len(tangent), bool)]
    assert len(hit) > 0.4 * len(centres), (len(hit), len(centres))
    for switch in SPHERE_SWITCHES:
        _with(monkeypatch, switch)
        env = build_product_env(spec)
        got = env.spheres_in_collision(s)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (switch, s[bad[:6]].tolist())
