"""The oracle's primitive narrow phase and environment loop against the COMPILED REFERENCE (CPU).

tests/golden/ref_prims.npz holds what the reference's own collision/validity.hh, shapes.hh, environment.hh and
sphere_*.hh answered (compiled in place: oracle/ref_prims.cc) for the environments and free spheres of
tests/prim_pins.py: the sorted lists with their min_distance, and per sphere and per 8-lane rake `ref`, `nobreak` and
`exact` (see prim_pins).  Nothing of the reference is needed to run these tests; test_fixtures_are_current regenerates
the fixture where oracle/_ref/libref_prims.so is built.

What the oracle (and the HIP path, tests/test_ref_prim_pins_gpu.py) must answer is `exact`: the reference's loop,
predicates and min_distance with max_extent from the correctly rounded sqrt.  Where a min_distance is not finite and
the entry was not inserted first, the reference's own sorted order is not defined; the product's rule (such a
min_distance is stored as 0) then answers `nobreak`.  For the zero-length capsule the reference's NaN has its sign bit
clear, its loop breaks at that entry and is blind to the rest of the list; the rule answers `nobreak` there too.

Pin certificate: where ref == nobreak, exact == ref.  It holds on every case outside the radial family.  In the radial
family (max_extent meets min_distance to the last bit, by construction) it does not: the reference's v * rsqrt(v) can
exceed the exact root, so the reference reaches a primitive that `exact` breaks in front of.  Measured on the fixture:
28 of 2,048 radial scalar queries have ref == nobreak == 1 and exact == 0, every one a contact within fp32 rounding of
touching; against the float64 clearance `exact` is wrong on 37 of those 2,048 queries and `ref` on 481."""
import os
import sys

import numpy as np
import pytest

import prim_pins as pp
from envs import build_oracle_env

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import make_prims_golden as gen  # noqa: E402

NAMES = pp.names()


def oracle_lists(env):
    return dict(spheres=env.spheres(), capsules=env.capsules(0), z_capsules=env.capsules(1), cuboids=env.cuboids(0),
                z_cuboids=env.cuboids(1))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference(oracle, name):
    """input digests (checked when the case is regenerated), the sorted lists and min_distance bit for bit, every
    sphere, and the OR over each rake's spheres"""
    case = pp.cases()[name]
    env = build_oracle_env(oracle, case.spec)
    want = case.lists()
    for key, got in oracle_lists(env).items():
        assert pp.same_lists(got, want[key]), (name, key)
    got = env.spheres_in_collision(case.scalar)
    assert np.array_equal(got, case.want()), (name, np.nonzero(got != case.want())[0][:10])
    lane_or = env.spheres_in_collision(case.rakes.reshape(-1, 4)).reshape(-1, 8).any(1)
    assert np.array_equal(lane_or, case.out("lane_or", rake=True)), name
    differ = lane_or != case.want(rake=True)
    assert np.array_equal(differ, rakes_where_a_lanes_own_break_decides(case)), name


def rakes_where_a_lanes_own_break_decides(case):
    """A rake breaks on its LARGEST max_extent, a sphere on its own (Environment.spheres_in_collision and the oracle's
    free-sphere query treat each sphere as its own replicated rake).  A lane whose own break sits exactly in front of a
    primitive it touches (min_distance - max_extent == +0) is tested against that primitive only in the company of a
    lane that reaches further: the rake's `exact` is then 1 and the OR over its spheres' own `exact` 0.  That is the
    same loop asked two different questions, not two predicates: it happens in the radial family only, every such rake
    holds a sphere whose own answer its own break decides (nobreak 1, exact 0), and the robot kernels, which do work
    rake-wide, are compared with the oracle's rake-wide loop on these scenes (tests/test_ref_prim_pins_gpu.py)."""
    differ = case.out("lane_or", rake=True) != case.want(rake=True)
    if differ.any():
        assert case.family == "radial", case.name
        assert case.want(rake=True)[differ].all() and case.out("nobreak", rake=True)[differ].all(), case.name
    return differ


def test_rake_and_sphere_answers_differ_only_where_a_lanes_own_break_decides():
    n = 0
    for case in pp.cases().values():
        n += int(rakes_where_a_lanes_own_break_decides(case).sum())
    assert n == sum(m.get("rake_exact_differs_from_lane_or", 0) for m in pp.load()[0]["cases"]) and n <= 4


def test_pin_certificate_and_break_decided_cap():
    """needs the fixture only"""
    meta = {m["name"]: m for m in pp.load()[0]["cases"]}
    radial_violations = 0
    for name, case in pp.cases().items():
        if not case.order_defined:
            continue
        m = meta[name]
        for rake in (False, True):
            ref, nobreak, exact = (case.out(k, rake) for k in pp.ANSWERS)
            assert not (exact & ~nobreak).any() and not (ref & ~nobreak).any(), name   # a hit is some predicate's hit
            decided = ref != nobreak
            assert int(decided.sum()) == m["rake_break_decided" if rake else "break_decided"]
            broken = ~decided & (exact != ref)
            if case.family == "radial":
                assert (ref[broken] & ~exact[broken]).all(), name
                radial_violations += int(broken.sum())
            else:
                assert not broken.any(), (name, np.nonzero(broken)[0][:10])
            if not rake and case.family not in pp.UNCAPPED:
                assert decided.mean() <= pp.MAX_BREAK_DECIDED, (name, decided.mean())
                assert abs(decided.mean() - m["break_decided_share"]) < 1e-6
    assert radial_violations == sum(m.get("certificate_violations", 0) for m in meta.values())
    assert 0 < radial_violations <= 40   # measured: 28 (module docstring); the family must stay where the break decides


def test_radial_family_three_way_record():
    """ref, nobreak, exact and the float64 clearance: which answer is geometrically right.  `exact` may be wrong only
    within fp32 rounding of touching (|clearance| below 2 ulp of the sphere's extent)"""
    for name, case in pp.cases().items():
        if case.family != "radial":
            continue
        clear = case.z[f"{name}__clear64"]
        ref, nobreak, exact = (case.out(k) for k in pp.ANSWERS)
        assert (ref != nobreak).mean() > 0.1, name                       # the break decides here, by construction
        wrong = exact != (clear < 0)
        extent = np.linalg.norm(case.scalar[:, :3].astype(np.float64), axis=1) + case.scalar[:, 3]
        assert (np.abs(clear[wrong]) <= 2 * np.spacing(extent[wrong].astype(np.float32))).all(), name
        assert wrong.sum() <= (ref != (clear < 0)).sum(), name


def test_not_finite_min_distance_rule(vamp, oracle):
    """a capsule whose axis passes through the origin (0 / 0 in collision/shapes.hh:165-189) and a zero-length capsule:
    min_distance is stored as 0, in the oracle, the C ABI's host tables and the Python property; the entry sorts first"""
    others = pp.ORDINARY["pole"]
    for p in (pp.NAN_BEAM, pp.NAN_POLE, pp.ZERO_LENGTH):
        assert vamp.Cylinder.from_canonical(p).min_distance == 0.0
        env = vamp.Environment()
        o = oracle.env()
        for c in (others[0], p, others[1]):
            env.add_capsule(vamp.Cylinder.from_canonical(c))
            o.add_capsule(c)
        key = "z_capsules" if pp.route("capsule", p) == "z_capsules" else "capsules"
        for rows in (env.host_tables()[key], oracle_lists(o)[key]):
            assert np.array_equal(rows[0, :8], p) and rows[0, 8] == 0.0 and not np.signbit(rows[0, 8])
            assert np.isfinite(rows[:, 8]).all() and (np.diff(rows[:, 8]) >= 0).all()
    # where the reference's order is defined (inserted first, sign bit of the NaN set) the rule reproduces it
    for name in ("nan_beam_at_0", "nan_pole_at_0"):
        case = pp.cases()[name]
        assert np.array_equal(case.out("ref"), case.out("exact")) and np.array_equal(case.out("exact"), case.out("nobreak"))
    # elsewhere it answers nobreak; the reference's loop over its own (undefined) order does not
    for name in ("nan_beam_at_1", "nan_beam_at_2", "nan_pole_at_1", "nan_pole_at_2", "zero_length_at_0", "zero_length_at_1"):
        case = pp.cases()[name]
        assert case.answer == "nobreak" and (case.out("exact") != case.out("nobreak")).sum() > 50
    assert not pp.cases()["zero_length_at_0"].out("ref").any()   # blind to the whole list


@pytest.mark.parametrize("name", NAMES)
def test_host_tables_equal_reference(vamp, name):
    """the C ABI's sorted lists (host code, no GPU): what the kernels are given"""
    from vamp_mvt_amd.workloads import environment_from_spec
    case = pp.cases()[name]
    tables = environment_from_spec(case.spec).host_tables()
    want = case.lists()
    for key in pp.LISTS:
        assert pp.same_lists(tables[key], want[key]), (name, key)


def past_the_buffer_queries():
    """heightfield queries whose cell index the reference clamps one past the image: ys == yd, and xs == xd in the last
    row -> (heightfield, spheres, expected) under the rule that such an index reads the LAST pixel"""
    hf = pp.heightfield(503, 5, 3)
    centre, scale, xd, yd, data = hf
    rng = np.random.default_rng(5)
    x_lo, y_lo = centre[0] - (xd - xd // 2) * scale[0], centre[1] - (yd - yd // 2) * scale[1]
    xy = np.concatenate([np.stack([rng.uniform(x_lo - 1.0, x_lo + xd * scale[0] + 1.0, 300), rng.uniform(y_lo - 1.0, y_lo, 300)], 1),
                         np.stack([rng.uniform(x_lo - 1.0, x_lo, 100), rng.uniform(y_lo, y_lo + scale[1], 100)], 1)])
    c = np.concatenate([xy, np.zeros((len(xy), 1))], 1).astype(np.float32)
    idx = pp.hf_index(hf, c)[0]
    keep = idx >= xd * yd
    assert keep.sum() > 300
    c, r = c[keep], rng.uniform(pp.R_LO, 0.1, int(keep.sum())).astype(np.float32)
    last = pp.hf_height(hf, np.full(len(c), xd * yd - 1))
    c[:, 2] = (last + r + rng.choice([-1e-3, 1e-3], len(c)).astype(np.float32)).astype(np.float32)
    want = np.signbit(((c[:, 2] - r).astype(np.float32) - last).astype(np.float32))
    assert 0.2 < want.mean() < 0.8
    return hf, np.concatenate([c, r[:, None]], 1).astype(np.float32), want


def test_heightfield_index_past_the_buffer_reads_the_last_pixel(oracle):
    """the reference gathers past its buffer there (undefined; kept out of the fixture); the oracle and the product
    (tests/test_ref_prim_pins_gpu.py) read the last pixel"""
    hf, spheres, want = past_the_buffer_queries()
    env = build_oracle_env(oracle, [("heightfield", hf)])
    assert np.array_equal(env.spheres_in_collision(spheres), want)


def test_fixture_is_not_degenerate():
    meta, z = pp.load()
    assert len(meta["cases"]) == len(pp.all_cases()) and meta["cpu_model"]
    for m in meta["cases"]:
        assert 0.1 * m["n_scalar"] < m["hits"] < 0.9 * m["n_scalar"], m["name"]
        assert 0.1 * m["n_rakes"] < m["rake_hits"] < 0.9 * m["n_rakes"], m["name"]
        assert m["n_scalar"] <= 6000 and m["n_rakes"] <= 750
    # the mirrored pairs really tie, in every list
    assert all(len(np.unique(z[f"mixed_8__{k}_md"])) < len(z[f"mixed_8__{k}_md"]) for k in pp.LISTS)
    # heightfields: queries exactly on cell borders, the wrapping upper x border (xs == xd below the last row) included
    for name, case in pp.cases().items():
        if case.family == "heightfield":
            hf = pp.hf_of(case.spec)[0]
            idx, xs, ys = pp.hf_index(hf, case.scalar[:, :3])
            assert (idx < hf[2] * hf[3]).all() and ((xs == hf[2]) & (ys < hf[3] - 1)).sum() >= 10, name
    sizes = {int(n) for m in meta["cases"] if m["family"] == "mixed" for n in [m["name"].split("_")[1]]}
    assert sizes == {1, 7, 8, 9, 63, 64, 65}


def test_fixtures_are_current():
    """regenerated in memory from the compiled reference == the committed file, key for key"""
    if not gen.available():
        pytest.skip("oracle/_ref/libref_prims.so not built (needs the reference at build time)")
    recorded = pp.load()[0]["cpu_model"]
    if gen.cpu_model() != recorded:
        pytest.skip(f"`ref` follows the CPU's approximate reciprocal square root; the fixture was generated on {recorded!r}")
    assert gen.differences() == []
