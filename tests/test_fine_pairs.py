"""The pair-dealt fine phase of the environment kernels (vmv_device.h env_fine_pairs), the parts that need no device:
the dealing itself, as tools/experiments/pair_fine_study.py models it (pair_rounds: runs of whole spheres, fills of the
entry list, entry-major pairs), and where the generator emits the calls (tools/gen_hip.py emit_env_link; text in
vamp_mvt_amd/csrc/gen/<robot>_dev.inc)."""
import importlib.util
import os
import re

import numpy as np
import pytest

import self_gates

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ROBOTS = ["panda", "ur5", "fetch", "baxter"]


def _study():
    spec = importlib.util.spec_from_file_location("pair_fine_study", os.path.join(ROOT, "tools", "experiments", "pair_fine_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_dealing(study, k, owners, sizes, cap, slots):
    rounds = study.pair_rounds(k, owners, sizes, cap, slots)
    n_spheres = sum(sizes)
    want = sorted((s * k + j, e) for s in range(n_spheres) for e, j in enumerate(owners))
    got = sorted(p for r in rounds for p in r)
    assert got == want, (k, len(owners), sizes, cap, slots)  # every (item, entry) pair once, and no other
    assert all(0 < len(r) <= 64 for r in rounds)
    return rounds


def test_every_pair_is_dealt_exactly_once():
    study = _study()
    rng = np.random.default_rng(13)
    for case in range(300):
        k = int(rng.integers(1, 65))
        chunk = int(rng.integers(1, 9))
        slots = chunk * 64
        n_spheres = int(rng.integers(1, 30))
        sizes = [min(chunk, n_spheres - c0) for c0 in range(0, n_spheres, chunk)]
        cap = int(rng.choice([1, 2, 7, 64, 128, 256]))
        P = int(rng.choice([0, 1, 2, int(rng.integers(0, 4 * k + 1)), int(rng.integers(0, 129))]))
        owners = [int(j) for j in rng.integers(0, k, P)]
        rounds = _check_dealing(study, k, owners, sizes, cap, slots)
        if P == 0:
            assert rounds == []


def test_dealing_at_the_edges():
    study = _study()
    assert study.pair_rounds(5, [], [4, 4, 1], 64, 256) == []  # P = 0: no round at all
    # capacity 1: one fill per entry, every fill its own rounds
    rounds = _check_dealing(study, 3, [0, 2, 2, 1], [4, 3], 1, 256)
    assert len(rounds) == 4 and all(len({e for _, e in r}) == 1 for r in rounds)
    # 64 lanes through the gate, four spheres per run: the slots are full and every run is flushed on its own
    rounds = _check_dealing(study, 64, list(range(64)) * 2, [4, 4, 2], 64, 256)
    assert len(rounds) == 2 * (4 + 4 + 2)
    # a lone lane with one candidate: one round with as many pairs as spheres
    rounds = _check_dealing(study, 1, [0], [4, 4, 4], 64, 256)
    assert [len(r) for r in rounds] == [12]


def test_packed_rounds_model_covers_every_item_once():
    study = _study()
    rng = np.random.default_rng(5)
    for _ in range(100):
        k, chunk, n_spheres = int(rng.integers(1, 65)), int(rng.integers(1, 9)), int(rng.integers(1, 30))
        sizes = [min(chunk, n_spheres - c0) for c0 in range(0, n_spheres, chunk)]
        ranges = study.packed_rounds(k, sizes, chunk * 64)
        assert [a for a, _ in ranges] == [0] + [b for _, b in ranges[:-1]] and ranges[-1][1] == k * n_spheres
        assert all(0 < b - a <= 64 for a, b in ranges)


@pytest.mark.parametrize("robot", ROBOTS)
def test_generator_emits_the_pair_calls_in_the_primitive_only_configuration_walk_only(robot):
    text = self_gates.generated_text(robot)
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"\n    (fkcc_\w+|static_env_hit)\(", text)]
    body = {}
    for at, name in heads:
        body.setdefault(name, text[at:text.index("\n    }\n", at)])  # (up to the function's closing brace)
    assert "fkcc_env" in body and "fkcc_env_paired" in body
    pairs = re.findall(r"vmv::env_pairs_(?:run|flush)<", text)
    assert pairs and len(pairs) == len(re.findall(r"vmv::env_pairs_(?:run|flush)<", body["fkcc_env"]))  # nowhere else
    assert "vmv::env_fine_pairs<" not in text  # (only through the two calls, which keep the packed rounds without candidate words)
    # every pair call sits under `if constexpr (PAIRS && G == 1)` with the packed call of the same link as its `else`
    walk = body["fkcc_env"]
    lines = walk.split("\n")
    for i, line in enumerate(lines):
        if "vmv::env_pairs_" in line:
            assert line.strip().startswith("if constexpr (PAIRS && G == 1) vmv::env_pairs_"), line
            alt = lines[i + 1].strip()
            assert alt.startswith("else vmv::env_fine_flush<G, Tab, V, kPackSlots>(") or \
                alt.startswith("else vmv::env_fine_packed<G, Tab, V, kPackSlots>("), alt
    n_packed = len(re.findall(r"vmv::env_fine_(?:packed|flush)<G, Tab, V, kPackSlots>", walk))
    assert n_packed == len(pairs)
    assert re.search(r"template <int G, int V, bool PAIRS = false>\n    __device__ __forceinline__ bool\n    fkcc_env\(", text)
    # the walk that keeps the reference's groups is routed before any pair call and never sees PAIRS
    assert "PAIRS" not in body["fkcc_env_paired"] and "PAIRS" not in body.get("fkcc_fused", "")
    assert walk.index("return fkcc_env_paired<G, V>(E, q, slab, skip);") < walk.index("vmv::env_pairs_")
    g = self_gates.gen_hip()
    on = re.search(r"static constexpr bool kFinePairs = (true|false);", text).group(1) == "true"
    assert on == (robot in g.FINE_PAIRS)
