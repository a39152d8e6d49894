#!/usr/bin/env python3
"""Offline study (oracle FK = test infrastructure; geometry in numpy): the fine phase of the primitive-only environment
kernels per wave of 64 uniform configurations in the 64-primitive shell scene, as built today — merged gates
(gen_hip.merged_groups), a link's items packed into kPackSlots slots and run by env_fine_flush's rule, every round
walking each list's candidate words until its busiest lane is done (vmv::list_masked) — against the same (item,
candidate) pairs dealt evenly per link, one pair per lane and round (pair_rounds below).
    python tools/experiments/pair_fine_study.py [waves] [entry capacity]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
WAVE = 64


def packed_rounds(k, sizes, slots):
    """The item ranges [(first, last)) of the rounds one link runs today: chunks of `sizes` fine spheres staged as k items
    per sphere into `slots` slots; before a chunk that would not fit, the whole 64-item rounds staged so far are run (all
    of it if the carried remainder still would not fit), and everything at the end of the link."""
    out, fill, done = [], 0, 0

    def run(n):
        nonlocal fill, done
        for b in range(0, n, WAVE):
            out.append((done + b, done + min(b + WAVE, n)))
        fill -= n
        done += n

    for ci, n in enumerate(sizes):
        if ci > 0 and fill + k * n > slots:
            r = fill // WAVE * WAVE
            if fill - r + k * n > slots:
                r = fill
            run(r)
        fill += k * n
    run(fill)
    return out


def pair_rounds(k, owners, sizes, cap, slots):
    """The dealing of one link's (item, entry) pairs.  k lanes passed the gate; entry e belongs to the lane of rank
    owners[e] (entries in list order); the link's fine spheres are staged whole, chunk by chunk (`sizes`), into `slots`
    item slots and run whenever the next chunk would not fit and at the end; the entry list holds `cap` entries, so a
    link with more is processed in several fills per run.  Pair t of a run of S spheres from sphere s0 against a fill of
    P entries from entry e0 is (entry e0 + t // S, sphere s0 + t % S) — entry-major, so that the lanes of a round share
    few entries and a list with two kinds of entry changes kind once per fill; its item is sphere * k + owner.
    -> rounds, each the list of the (item, entry) pairs its lanes evaluate, at most 64."""
    assert cap >= 1 and all(k * n <= slots for n in sizes)
    rounds, P = [], len(owners)

    def run(s0, S):
        for e0 in range(0, P, cap):
            Pf = min(cap, P - e0)
            for b in range(0, S * Pf, WAVE):
                rounds.append([((s0 + t % S) * k + owners[e0 + t // S], e0 + t // S) for t in range(b, min(b + WAVE, S * Pf))])

    s0 = staged = 0
    for ci, n in enumerate(sizes):
        if ci > 0 and (staged + n) * k > slots:
            run(s0, staged)
            s0, staged = s0 + staged, 0
        staged += n
    run(s0, staged)
    return rounds


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_hip
    from oracle_lib import Oracle
    from vamp_mvt_amd.workloads import shell_spec

    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 64  # vmv::kPairEntries
    m = json.load(open(os.path.join(ROOT, "vamp_mvt_amd", "robots", "panda.json")))
    groups = [g for g in gen_hip.merged_groups(m) if g["link"] not in set(gen_hip.static_links(m))]
    C = min(gen_hip.ENV_CHUNK.get("panda", gen_hip.DEFAULT_CHUNK), max(len(g["fine"]) for g in gen_hip.merged_groups(m)))
    slots = C * WAVE  # kPackSlots
    o = Oracle()
    rid = o.robot("panda")
    lob, span = o.bounds(rid)
    spec = shell_spec(0)
    sph = np.array([p for kind, p in spec if kind == "sphere"], np.float64)
    cub = np.array([p for kind, p in spec if kind == "cuboid"], np.float64)  # c(3) ax1(3) ax2(3) ax3(3) half(3)
    R = np.array(m["radii"], np.float64)
    MARGIN = 1e-4  # vmv::kCandidateMargin

    def dist(c):  # distance from point c to the surface of every primitive, per list (the kernel's two one-word lists)
        d = c - cub[:, :3]
        loc = np.stack([(d * cub[:, 3 + 3 * i:6 + 3 * i]).sum(1) for i in range(3)], 1)
        return [np.linalg.norm(sph[:, :3] - c, axis=1) - sph[:, 3],
                np.linalg.norm(np.maximum(np.abs(loc) - cub[:, 12:15], 0.0), axis=1)]

    rng = np.random.default_rng(0)
    tot = dict(gates=0, items=0, rounds=0, steps_sphere=0, steps_zcuboid=0, pairs=0, ideal=0, pair_rounds=0, fills=0, joint_rounds=0, joint_evals=0, steps_first=0)
    top = dict(link_pairs=0, link_entries=0, list_entries=0, lane_cands=0, lane_cands_list=0)
    for w in range(waves):
        q = (lob + span * rng.random((WAVE, len(lob)), dtype=np.float32)).astype(np.float32)
        S = np.stack([o.fk_all(rid, c) for c in q]).astype(np.float64)
        bad = np.zeros(WAVE, bool)
        for g in groups:
            b, fine = g["bound"], g["fine"]
            lanes, cands = [], []
            for i in range(WAVE):
                d = [x - g["radius"] for x in dist(S[i, b, :3])]
                if not bad[i] and min(x.min() for x in d) < 0:
                    lanes.append(i)
                    cands.append([int((x < MARGIN).sum()) for x in d])  # per list: candidates the gate records
            k = len(lanes)
            if k == 0:
                continue
            sizes = [len(fine[c0:c0 + C]) for c0 in range(0, len(fine), C)]
            tot["gates"] += 1
            tot["items"] += k * len(fine)
            # (a) as built: a round's steps per list = the largest candidate count among the lanes its items work for
            for first, last in packed_rounds(k, sizes, slots):
                js = {i % k for i in range(first, last)}
                tot["rounds"] += 1
                tot["steps_sphere"] += max(cands[j][0] for j in js)
                tot["steps_zcuboid"] += max(cands[j][1] for j in js)
                # (the measurement build VMV_ABLATE_ENV=10: an item evaluates its first candidate only)
                tot["steps_first"] += max(min(cands[j][0], 1) for j in js) + max(min(cands[j][1], 1 - min(cands[j][0], 1)) for j in js)
            # (b) the same pairs, one per lane and round: each list's entries dealt on their own (a round runs one
            # prim_eval), and both lists' entries in one list (a round that holds both kinds runs both)
            pairs = entries = 0
            for t in range(2):
                owners = [j for j in range(k) for _ in range(cands[j][t])]
                pr = pair_rounds(k, owners, sizes, cap, slots)
                assert sum(len(r) for r in pr) == len(owners) * len(fine)
                pairs += len(owners) * len(fine)
                entries += len(owners)
                tot["pair_rounds"] += len(pr)
                tot["fills"] += -(-len(owners) // cap)
                top["list_entries"] = max(top["list_entries"], len(owners))
            owners = [j for t in range(2) for j in range(k) for _ in range(cands[j][t])]
            n_sphere = sum(c[0] for c in cands)
            pr = pair_rounds(k, owners, sizes, cap, slots)
            tot["joint_rounds"] += len(pr)
            tot["joint_evals"] += sum(len({e < n_sphere for _, e in r}) for r in pr)
            tot["pairs"] += pairs
            tot["ideal"] += -(-pairs // WAVE)
            top["link_pairs"] = max(top["link_pairs"], pairs)
            top["link_entries"] = max(top["link_entries"], entries)
            top["lane_cands"] = max(top["lane_cands"], max(sum(c) for c in cands))
            top["lane_cands_list"] = max(top["lane_cands_list"], max(max(c) for c in cands))
            for j, i in enumerate(lanes):
                if any(min(x.min() for x in dist(S[i, s, :3])) - R[s] < 0 for s in fine):
                    bad[i] = True
    per = {key: round(v / waves, 2) for key, v in tot.items()}
    steps = per["steps_sphere"] + per["steps_zcuboid"]
    print(f"panda, shell64, {waves} waves of 64 uniform configurations; chunk {C}, {slots} item slots, entry list of {cap}")
    print(f"(a) as built, per wave: gates with a passing lane {per['gates']}, items {per['items']}, rounds {per['rounds']}, "
          f"max-over-lanes steps {steps:.2f} (sphere list {per['steps_sphere']}, z-cuboid list {per['steps_zcuboid']})")
    print(f"    with every item cut to its first candidate (VMV_ABLATE_ENV=10): steps {per['steps_first']}")
    print(f"(b) dealt evenly per link, per wave: pairs {per['pairs']} = {per['pairs'] / WAVE:.2f} steps' worth of lanes; "
          f"ceil(pairs / 64) per link: {per['ideal']}")
    print(f"    one entry list per primitive list: rounds = evaluation steps {per['pair_rounds']} ({per['fills']} list fills): "
          f"{100 * (1 - per['pair_rounds'] / steps):.0f} % of (a)'s steps removed")
    print(f"    one entry list for both: rounds {per['joint_rounds']} ({100 * (1 - per['joint_rounds'] / steps):.0f} % removed), "
          f"evaluation steps {per['joint_evals']} with both kinds run where a round holds both "
          f"({100 * (1 - per['joint_evals'] / steps):.0f} % removed)")
    print(f"(c) largest seen: pairs of one link {top['link_pairs']}, entries of one link {top['link_entries']} (of one list "
          f"{top['list_entries']}), candidates "
          f"of one lane {top['lane_cands']} (in one list {top['lane_cands_list']})")


if __name__ == "__main__":
    main()
