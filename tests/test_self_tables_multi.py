"""The three- and four-joint clearance tables of the self-collision kernels (tools/gen_hip.py: self_tables_multi; data in
vamp_mvt_amd/csrc/gen/<robot>_dev.inc) against the oracle's own fp32 FK: wherever a table says "group certainly free", no
fine pair of that group may collide and the nearest pair stays more than 5e-5 m clear — for configurations drawn
everywhere in joint space, on cell borders of every table joint, and with the other joints anywhere.  Outside the joint
bounds every bit reads 1.  Each table must also remove at least half of its group's gate firings on a seeded uniform
sample (the rule by which a group gets a table at all), so a table of ones cannot pass."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GEN = os.path.join(ROOT, "vamp_mvt_amd", "csrc", "gen")
MAX_BYTES = 256 * 1024  # new tables per robot


def _tables(robot):
    path = os.path.join(GEN, f"{robot}_dev.inc")
    if not os.path.exists(path):
        pytest.skip("generated sources not built")
    text = open(path).read()
    out = []
    for m in re.finditer(r"// multi-joint table (\d+): joints ([\d, ]+); (\d+) cells per joint; (\S+) vs\. (\S+) \([^\n]*\n"
                         r"\s*__device__ const unsigned kSelfMulti\d+\[(\d+)\] = \{\n(.*?)\n    \};", text, re.S):
        ti, joints, n = int(m.group(1)), [int(j) for j in m.group(2).split(",")], int(m.group(3))
        words = np.array([int(v.strip().rstrip("u"), 16) for v in m.group(7).replace("\n", "").split(",") if v.strip()], np.uint32)
        assert len(words) == int(m.group(6)) == n ** len(joints) // 32
        fn = text[text.index(f"unsigned self_multi{ti}(const float"):]
        fn = fn[:fn.index("return")]
        coords = re.findall(r"f(\d) = \(q\[(\d+)\] - (\S+)f\) \* (\S+)f;", fn)
        assert [int(c[1]) for c in coords] == joints
        out.append(dict(joints=joints, n=n, words=words, a=m.group(4), b=m.group(5),
                        lo=[np.float32(float.fromhex(c[2])) for c in coords],
                        inv=[np.float32(float.fromhex(c[3])) for c in coords]))
    return out


def _bits(t, q):
    """the device's answer (vmv::self_table_bit): fp32 cell coordinates, 1 outside the grid"""
    inside = np.ones(len(q), bool)
    idx = np.zeros(len(q), np.int64)
    for j, lo_j, inv_j in zip(t["joints"], t["lo"], t["inv"]):
        f = (q[:, j] - lo_j) * inv_j  # fp32
        assert f.dtype == np.float32
        inside &= (f >= 0) & (f < t["n"])
        idx = idx * t["n"] + np.clip(np.nan_to_num(f).astype(np.int64), 0, t["n"] - 1)
    bit = (t["words"][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1
    return np.where(inside, bit, 1), inside


def _pairs(model, radii, S, a, b):
    g = next(g for g in model["self_groups"] if g["a"] == a and g["b"] == b)
    pr = np.array(g["pairs"])
    d = S[:, pr[:, 0], :3] - S[:, pr[:, 1], :3]
    sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]  # fp32, sql2_3's order
    rs = radii[pr[:, 0]] + radii[pr[:, 1]]
    db = S[:, g["bound_a"], :3] - S[:, g["bound_b"], :3]
    sqb = (db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1]) + db[..., 2] * db[..., 2]
    rb = radii[g["bound_a"]] + radii[g["bound_b"]]
    return sq, rs, sqb - rb * rb < 0


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch", "baxter"])
def test_cells_marked_free_hold_no_colliding_pair(oracle, robot):
    tables = _tables(robot)
    if robot == "panda":
        assert sorted((t["a"], t["b"]) for t in tables) == [("panda_link1", "panda_link5"), ("panda_link2", "panda_link5")]
    assert sum(4 * len(t["words"]) for t in tables) <= MAX_BYTES
    model = json.load(open(os.path.join(ROOT, "vamp_mvt_amd", "robots", f"{robot}.json")))
    radii = np.array(model["radii"], np.float32)
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(2025)
    n = 40000
    for t in tables:
        assert 3 <= len(t["joints"]) <= 4
        q = (lo + span * rng.random((n, len(lo)), dtype=np.float32)).astype(np.float32)
        # a third of the samples on (and a hair off) cell borders of every table joint
        k = n // 3
        for axis, lo_a, inv_a in zip(t["joints"], t["lo"], t["inv"]):
            edge = rng.integers(0, t["n"] + 1, size=k).astype(np.float64) / float(inv_a) + float(lo_a)
            q[:k, axis] = (edge + rng.choice([-1e-6, 0.0, 1e-6], size=k)).astype(np.float32)
        q[k:k + 50] *= np.float32(1.5)  # outside the joint bounds: the bit must read 1
        q[k + 50:k + 60, t["joints"][-1]] = np.float32(np.nan)
        bit, inside = _bits(t, q)
        assert (~inside).sum() >= 10 and (bit[~inside] == 1).all()
        S = np.stack([oracle.fk_all(rid, c) for c in q])  # fp32 sphere centres, the oracle's FK
        sq, rs, _ = _pairs(model, radii, S, t["a"], t["b"])
        collides = (sq - rs * rs < 0).any(axis=1)
        free = bit == 0
        assert free.any(), (robot, t["a"], t["b"])
        assert not (collides & free).any(), (robot, t["a"], t["b"], q[np.nonzero(collides & free)[0][:3]])
        # how close the skipped configurations come: must stay clear of the fp32 noise floor (~1e-6 m)
        clearance = (np.sqrt(sq[free].astype(np.float64)) - rs).min()
        print(robot, t["a"], t["b"], "cells", t["n"], "free samples", int(free.sum()), "least clearance", clearance)
        assert clearance > 5e-5, (robot, t["a"], t["b"], clearance)


@pytest.mark.parametrize("robot", ["panda", "ur5", "fetch", "baxter"])
def test_tables_remove_half_of_their_gate_firings(oracle, robot):
    tables = _tables(robot)
    model = json.load(open(os.path.join(ROOT, "vamp_mvt_amd", "robots", f"{robot}.json")))
    radii = np.array(model["radii"], np.float32)
    rid = oracle.robot(robot)
    lo, span = oracle.bounds(rid)
    rng = np.random.default_rng(77)
    q = (lo + span * rng.random((20000, len(lo)), dtype=np.float32)).astype(np.float32)
    S = np.stack([oracle.fk_all(rid, c) for c in q])
    for t in tables:
        bit, inside = _bits(t, q)
        _, _, gate = _pairs(model, radii, S, t["a"], t["b"])
        fires, kept = int(gate.sum()), int((gate & (bit != 0)).sum())
        print(robot, t["a"], t["b"], "gate fires", fires, "with the bit", kept)
        assert fires >= 0.015 * len(q), (robot, t["a"], t["b"], fires)  # (the builder asks for 2 % on its own sample)
        assert 2 * kept <= fires, (robot, t["a"], t["b"], fires, kept)
