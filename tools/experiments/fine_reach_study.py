#!/usr/bin/env python3
"""Offline study (oracle FK = test infrastructure; geometry in numpy): pruning the pair-dealt fine phase of the
primitive-only environment kernels (vmv_device.h env_fine_pairs) by each fine sphere's reach from its gate's centre
(fine_reach, reach_classes below).  The model of pair_fine_study.py — merged gates, whole spheres staged chunk
by chunk into kPackSlots item slots and run when the next chunk would not fit, an entry list of kPairEntries per fill,
one pair per lane and round, colliding lanes leaving the wave — extended with the class rule as it would be built:
a candidate's class is the number of the gate's thresholds its distance exceeds, the entries of a list are grouped by
class, class c is tested by the first S_c spheres (descending reach), the pairs of all classes share one index space
per (gate, list, run, fill), and a chunk no live entry needs is not staged.  The thresholds are chosen per gate, from
the reach values, by minimising the modelled rounds on the sample itself.
Printed per wave, for today's dealing, for one threshold (one class bit per candidate: what the two spare candidate
words hold next to a two-word candidate layout such as shell64's), for three (two bits) and for the exact per-entry
rule: pairs, rounds, the (lane, sphere) items some pair needs, staged spheres, steps of the entry walks, hits lost.
    python tools/experiments/fine_reach_study.py [robot] [waves]"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
WAVE = 64
CAP = 64  # vmv::kPairEntries
MARGIN = 1e-4      # vmv::kCandidateMargin
REACH_PAD = 5e-6   # the pad of the merged gate radii (tools/gen_hip.py: merged_groups)
MAX_THRESHOLDS = 3  # two class bits per candidate


def fine_reach(gen_hip, m):
    """Per gate of gen_hip.merged_groups (same order): how far each fine sphere reaches from the gate's centre,
    reach_s = |c_s - c_gate| + r_s.  It does not depend on the configuration (the fine spheres of a gate are rigidly
    attached to its centre): taken from the float64 tape over the 96 configurations merged_groups takes its radii from,
    and rounded up to fp32 with the same 5e-6 m pad.  A fine sphere can only touch a primitive whose surface lies closer
    than reach_s + MARGIN to the gate's centre (triangle inequality, 1-Lipschitz primitive distances), so a primitive
    at distance d needs the spheres with reach_s + MARGIN > d only: with the spheres in descending reach, a prefix.
    -> list of dict(link, bound, order=[fine sphere ids by descending reach], reach=[their reach, descending])."""
    rng = np.random.default_rng(12345)
    lo, sp = np.array(m["lower"]), np.array(m["span"])
    q = lo + sp * rng.random((96, m["dimension"]))
    q[:32] *= 2.5
    C = gen_hip.eval_tape(m, q)
    R = np.array(m["radii"], np.float64)
    out = []
    for grp in gen_hip.merged_groups(m):
        fine = list(grp["fine"])
        d = np.linalg.norm(C[:, fine, :] - C[:, [grp["bound"]], :], axis=2) + R[fine][None, :]
        far = [float(np.nextafter(np.float32(v + REACH_PAD), np.float32(np.inf))) for v in d.max(axis=0)]
        idx = sorted(range(len(fine)), key=lambda i: (-far[i], i))
        out.append(dict(link=grp["link"], bound=grp["bound"], order=[fine[i] for i in idx], reach=[far[i] for i in idx]))
    return out


def reach_classes(reach, cuts):
    """Class rule of one gate.  reach: descending (fine_reach); cuts: positions of the spheres whose reach sets a
    threshold, descending (so the thresholds ascend), at most MAX_THRESHOLDS.  tau_c = reach[cut_c] + MARGIN; the class
    of a candidate is the number of thresholds that the distance from the gate's centre to its surface exceeds; class c
    is tested by the first S_c spheres, those with reach + MARGIN > tau_c (class 0: all of them).
    -> (taus ascending, S = [S_0, S_1, ...] non-increasing)."""
    assert len(cuts) <= MAX_THRESHOLDS and list(cuts) == sorted(set(cuts), reverse=True)
    taus = [reach[c] + MARGIN for c in cuts]
    S = [len(reach)] + [sum(1 for r in reach if r + MARGIN > t) for t in taus]
    return taus, S


def candidate_class(taus, d):
    """class of the candidates at distances d (gate centre to surface)"""
    d = np.asarray(d, np.float64)
    return (d[..., None] > np.asarray(taus, np.float64)).sum(axis=-1) if len(taus) else np.zeros(d.shape, int)


def runs_of(k, n_spheres, chunk, slots):
    """[(s0, S)]: the runs of a gate with n_spheres fine spheres to stage and k passing lanes (pair_fine_study.pair_rounds)"""
    out, s0, staged = [], 0, 0
    for c0 in range(0, n_spheres, chunk):
        n = min(chunk, n_spheres - c0)
        if c0 > 0 and (staged + n) * k > slots:
            out.append((s0, staged))
            s0, staged = s0 + staged, 0
        staged += n
    out.append((s0, staged))
    return out


def list_rounds(prefix, runs):
    """One list of one gate.  prefix: per entry the number of leading spheres it is tested by.  Entries are grouped by
    descending prefix (= by class), filled CAP at a time; a run (s0, S) gives an entry clamp(prefix - s0, 0, S) pairs.
    -> (pairs, rounds)"""
    prefix = sorted(prefix, reverse=True)
    pairs = rounds = 0
    for s0, S in runs:
        for e0 in range(0, len(prefix), CAP):
            n = sum(min(max(p - s0, 0), S) for p in prefix[e0:e0 + CAP])
            pairs += n
            rounds += -(-n // WAVE)
    return pairs, rounds


def gate_cost(units, n_fine, S_of, chunk, slots):
    """units: per (wave) of one gate dict(k, d=[per list: array of entry distances], ...); S_of(d) -> prefix per entry.
    -> dict(pairs, rounds, staged, flat = rounds if every (gate, list) were one run and one fill: ceil(pairs / 64))"""
    tot = dict(pairs=0, rounds=0, staged=0, flat=0)
    for u in units:
        pre = [S_of(d) for d in u["d"]]
        need = max([int(p.max()) for p in pre if len(p)] + [0])  # spheres some live entry needs
        staged = min(n_fine, -(-need // chunk) * chunk)          # whole chunks
        runs = runs_of(u["k"], staged, chunk, slots) if staged else []
        tot["staged"] += staged
        for p in pre:
            a, b = list_rounds(p.tolist(), runs)
            tot["pairs"] += a
            tot["rounds"] += b
            tot["flat"] += -(-int(p.sum()) // WAVE)
    return tot


def choose_cuts(units, reach, n_thresholds, chunk, slots):
    """the cut set (reach_classes) of at most n_thresholds thresholds with the fewest modelled rounds; () if none
    lowers them"""
    n = len(reach)
    distinct = [i for i in range(1, n) if reach[i] < reach[i - 1]]  # cutting at i excludes spheres i.. (and ties behind)

    def cost(cuts):
        taus, S = reach_classes(reach, cuts)
        S = np.array(S)
        return gate_cost(units, n, lambda d: S[candidate_class(taus, d)], chunk, slots)["rounds"]

    best, best_cuts = cost(()), ()
    for m in range(1, n_thresholds + 1):
        for cuts in itertools.combinations(reversed(distinct), m):
            c = cost(cuts)
            if c < best:
                best, best_cuts = c, cuts
    return best_cuts


def sample(robot, waves, seed=0):
    """-> (gen_hip, model, gates, per gate the units of the sample).  A unit: one wave at one gate with a passing lane:
    k, lanes, per list the entry distances d (gate centre to the candidate's surface), owners (rank) and primitive ids."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_hip
    from oracle_lib import Oracle
    from vamp_mvt_amd.workloads import shell_spec

    m = json.load(open(os.path.join(ROOT, "vamp_mvt_amd", "robots", f"{robot}.json")))
    static = set(gen_hip.static_links(m))
    groups = gen_hip.merged_groups(m)
    reach = fine_reach(gen_hip, m)
    gates = [dict(g, order=r["order"], reach=r["reach"]) for g, r in zip(groups, reach) if g["link"] not in static]
    o = Oracle()
    rid = o.robot(robot)
    lob, span = o.bounds(rid)
    spec = shell_spec(0)
    sph = np.array([p for kind, p in spec if kind == "sphere"], np.float64)
    cub = np.array([p for kind, p in spec if kind == "cuboid"], np.float64)  # c(3) ax1(3) ax2(3) ax3(3) half(3)
    R = np.array(m["radii"], np.float64)
    margin = MARGIN

    def dist(c):  # distance from point c to the surface of every primitive, per list (the kernel's two one-word lists)
        d = c - cub[:, :3]
        loc = np.stack([(d * cub[:, 3 + 3 * i:6 + 3 * i]).sum(1) for i in range(3)], 1)
        return [np.linalg.norm(sph[:, :3] - c, axis=1) - sph[:, 3],
                np.linalg.norm(np.maximum(np.abs(loc) - cub[:, 12:15], 0.0), axis=1)]

    rng = np.random.default_rng(seed)
    units = [[] for _ in gates]
    for w in range(waves):
        q = (lob + span * rng.random((WAVE, len(lob)), dtype=np.float32)).astype(np.float32)
        S = np.stack([o.fk_all(rid, c) for c in q]).astype(np.float64)
        bad = np.zeros(WAVE, bool)
        for gi, g in enumerate(gates):
            lanes, d, owner, prim = [], [[], []], [[], []], [[], []]
            for i in range(WAVE):
                dd = dist(S[i, g["bound"], :3])
                if not bad[i] and min(x.min() for x in dd) - g["radius"] < 0:
                    for t in range(2):
                        for p in np.nonzero(dd[t] - g["radius"] < margin)[0]:
                            d[t].append(dd[t][p])
                            owner[t].append(len(lanes))
                            prim[t].append(int(p))
                    lanes.append(i)
            if not lanes:
                continue
            # the exact predicates of every (lane, fine sphere, candidate): hit[t][entry][position in g["order"]]
            hit = [np.array([[dist(S[lanes[j], s, :3])[t][p] - R[s] < 0 for s in g["order"]] for j, p in zip(owner[t], prim[t])],
                            bool).reshape(len(prim[t]), len(g["order"])) for t in range(2)]
            units[gi].append(dict(k=len(lanes), d=[np.array(x, np.float64) for x in d], owner=owner, hit=hit))
            for j, i in enumerate(lanes):
                if any(h[np.array(ow) == j].any() for h, ow in zip(hit, owner) if len(ow)):
                    bad[i] = True
    chunk = min(gen_hip.ENV_CHUNK.get(robot, gen_hip.DEFAULT_CHUNK), max(len(g["fine"]) for g in groups))
    return gen_hip, m, gates, units, chunk


def evaluate(gates, units, rule, chunk):
    """rule(gate index) -> S_of(d).  -> totals over the sample, and rounds per gate"""
    slots = chunk * WAVE
    tot = dict(pairs=0, rounds=0, flat=0, staged=0, items=0, walk=0, hits=0, lost=0)
    per_gate = []
    for gi, g in enumerate(gates):
        S_of = rule(gi)
        c = gate_cost(units[gi], len(g["order"]), S_of, chunk, slots)
        per_gate.append([c["rounds"], 0])
        for key in ("pairs", "rounds", "flat", "staged"):
            tot[key] += c[key]
        for u in units[gi]:
            need = set()
            for t in range(2):
                pre = S_of(u["d"][t])
                for e, p in enumerate(pre):
                    need |= {(u["owner"][t][e], s) for s in range(int(p))}
                    tot["hits"] += int(u["hit"][t][e].sum())
                    tot["lost"] += int(u["hit"][t][e][int(p):].sum())
                # entry walk: one bit per lane and step, class by class (entries grouped by class)
                for cls in set(pre.tolist()):
                    own = [o_ for o_, p in zip(u["owner"][t], pre) if p == cls]
                    per_gate[-1][1] += max(own.count(j) for j in set(own))
            tot["items"] += len(need)
        tot["walk"] += per_gate[-1][1]
    return tot, per_gate


def main():
    robot = sys.argv[1] if len(sys.argv) > 1 else "panda"
    waves = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    gen_hip, m, gates, units, chunk = sample(robot, waves)
    slots = chunk * WAVE
    margin = MARGIN
    print(f"{robot}, shell64, {waves} waves of 64 uniform configurations, seed 0; chunk {chunk}, {slots} item slots, entry list of {CAP}")
    for g in gates:
        print(f"  gate {g['link']}: radius {g['radius']:.4f}, {len(g['order'])} fine spheres, reach "
              + " ".join(f"{r:.3f}" for r in g["reach"]))
    rules = {}
    rules["today"] = lambda gi: (lambda d, n=len(gates[gi]["order"]): np.full(len(d), n, int))
    cuts = {}
    for name, n_thr in (("one threshold", 1), ("three thresholds", 3)):
        cuts[name] = [choose_cuts(units[gi], g["reach"], n_thr, chunk, slots) for gi, g in enumerate(gates)]

        def rule(gi, name=name):
            taus, S = reach_classes(gates[gi]["reach"], cuts[name][gi])
            S = np.array(S)
            return lambda d: S[candidate_class(taus, d)]
        rules[name] = rule
    rules["exact per entry"] = lambda gi: (lambda d, r=np.array(gates[gi]["reach"]): (r[None, :] + margin > np.asarray(d)[:, None]).sum(1)
                                           if len(d) else np.zeros(0, int))
    print("per wave; rounds as built (chunked runs, fills) and as ceil(pairs / 64) per (gate, list); per gate: rounds / entry-walk steps")
    print("                      pairs   rounds   ceil   items   staged spheres   entry-walk steps   hits lost   per gate")
    for name, rule in rules.items():
        tot, per_gate = evaluate(gates, units, rule, chunk)
        print(f"  {name:18s} {tot['pairs'] / waves:7.1f}  {tot['rounds'] / waves:7.2f} {tot['flat'] / waves:6.2f}  {tot['items'] / waves:6.0f}  {tot['staged'] / waves:11.1f}"
              f"  {tot['walk'] / waves:15.2f}   {tot['lost']:4d} of {tot['hits']}   " + " ".join(f"{r / waves:.2f}/{w / waves:.2f}" for r, w in per_gate))
        if name in cuts:
            for g, c in zip(gates, cuts[name]):
                taus, S = reach_classes(g["reach"], c)
                print(f"      {g['link']}: " + ("no classes" if not c else "tau " + " ".join(f"{t:.4f}" for t in taus) + "  S " + " ".join(map(str, S))))


if __name__ == "__main__":
    main()
