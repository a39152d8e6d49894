"""The gates of the self-collision half on the CPU, for the tests of the screen (validate_self_kernel, fkcc_self_screen):
the clearance tables as the generated sources hold them, and per configuration and group the clearance of the bounding
pair (the generator's float64 tape) and the group's table bit (the device's fp32 cell arithmetic)."""
import importlib.util
import json
import os
import re

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GEN = os.path.join(ROOT, "vamp_mvt_amd", "csrc", "gen")


def gen_hip():
    spec = importlib.util.spec_from_file_location("gen_hip", os.path.join(ROOT, "tools", "gen_hip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def model(robot):
    with open(os.path.join(ROOT, "vamp_mvt_amd", "robots", f"{robot}.json")) as f:
        return json.load(f)


def generated_text(robot):
    path = os.path.join(GEN, f"{robot}_dev.inc")
    assert os.path.exists(path), "generated sources not built (build() writes them)"
    with open(path) as f:
        return f.read()


def _group_index(m, a, b):
    (gi,) = [i for i, g in enumerate(m["self_groups"]) if g["a"] == a and g["b"] == b]
    return gi


def tables(robot, m, text):
    """-> (two-joint tables, multi-joint tables) in the form tools/gen_hip.py: gate_rates takes them"""
    two, multi = [], []
    for t in re.finditer(r"// table (\d+): joints (\d+), (\d+); ([^\n]*)\n\s*__device__ const unsigned char kSelfTable\d+\[(\d+) \* \d+\] = \{\n(.*?)\n    \};",
                         text, re.S):
        ti, i, j, names, n = int(t.group(1)), int(t.group(2)), int(t.group(3)), t.group(4), int(t.group(5))
        data = np.array([int(v) for v in t.group(6).replace("\n", "").split(",") if v.strip()], np.uint8).reshape(n, n)
        fn = text[text.index(f"unsigned self_table{ti}(const float"):]
        lo_i, inv_i = re.search(r"fi = \(q\[\d+\] - (\S+)f\) \* (\S+)f;", fn).groups()
        lo_j, inv_j = re.search(r"fj = \(q\[\d+\] - (\S+)f\) \* (\S+)f;", fn).groups()
        bits = re.findall(r"bit (\d+): (\S+) vs\. (\S+) \(", names)
        assert [int(b) for b, _, _ in bits] == list(range(len(bits)))
        two.append(dict(joints=(i, j), table=data, lo=(float.fromhex(lo_i), float.fromhex(lo_j)),
                        inv=(float.fromhex(inv_i), float.fromhex(inv_j)), groups=[_group_index(m, a, b) for _, a, b in bits]))
    for t in re.finditer(r"// multi-joint table (\d+): joints ([\d, ]+); (\d+) cells per joint; (\S+) vs\. (\S+) \([^\n]*\n"
                         r"\s*__device__ const unsigned kSelfMulti\d+\[(\d+)\] = \{\n(.*?)\n    \};", text, re.S):
        ti, joints, n = int(t.group(1)), [int(j) for j in t.group(2).split(",")], int(t.group(3))
        words = np.array([int(v.strip().rstrip("u"), 16) for v in t.group(7).replace("\n", "").split(",") if v.strip()], np.uint32)
        assert len(words) == int(t.group(6)) == n ** len(joints) // 32
        fn = text[text.index(f"unsigned self_multi{ti}(const float"):]
        coords = re.findall(r"f(\d) = \(q\[(\d+)\] - (\S+)f\) \* (\S+)f;", fn[:fn.index("return")])
        assert [int(c[1]) for c in coords] == joints
        multi.append(dict(group=_group_index(m, t.group(4), t.group(5)), joints=joints, n=n, words=words,
                          lo=[float.fromhex(c[2]) for c in coords], inv=[float.fromhex(c[3]) for c in coords]))
    return two, multi


def table_bits(m, two, multi, q):
    """[N][groups] bool: the table bit the device reads for each group (True where a group has no table; a multi-joint
    table replaces a two-joint one, as in the generated gates).  q is fp32; every bit reads 1 outside a table's grid."""
    assert q.dtype == np.float32
    bits = np.ones((len(q), len(m["self_groups"])), bool)
    for t in two:
        n = t["table"].shape[0]
        f = [(q[:, j] - np.float32(lo)) * np.float32(inv) for j, lo, inv in zip(t["joints"], t["lo"], t["inv"])]
        inside = (f[0] >= 0) & (f[1] >= 0) & (f[0] < n) & (f[1] < n)
        cell = t["table"][np.clip(np.nan_to_num(f[0]).astype(np.int64), 0, n - 1), np.clip(np.nan_to_num(f[1]).astype(np.int64), 0, n - 1)]
        for bit, gi in enumerate(t["groups"]):
            bits[:, gi] = np.where(inside, ((cell >> bit) & 1) != 0, True)
    for t in multi:
        n = t["n"]
        inside = np.ones(len(q), bool)
        idx = np.zeros(len(q), np.int64)
        for j, lo, inv in zip(t["joints"], t["lo"], t["inv"]):
            f = (q[:, j] - np.float32(lo)) * np.float32(inv)
            inside &= (f >= 0) & (f < n)
            idx = idx * n + np.clip(np.nan_to_num(f).astype(np.int64), 0, n - 1)
        bits[:, t["group"]] = np.where(inside, ((t["words"][idx >> 5] >> (idx & 31).astype(np.uint32)) & 1) != 0, True)
    return bits


def gate_clearance(m, q):
    """[N][groups] float64: distance of the bounding pair's centres minus the radii (negative = the gate fires)"""
    c = gen_hip().eval_tape(m, q.astype(np.float64))
    r = np.array(m["radii"])
    return np.stack([np.linalg.norm(c[:, g["bound_a"]] - c[:, g["bound_b"]], axis=1) - (r[g["bound_a"]] + r[g["bound_b"]])
                     for g in m["self_groups"]], axis=1)
