#!/usr/bin/env python3
"""Generates tests/golden/ref_{mvt,capt,scdf,centervox}.npz from the reference's own point-cloud headers.

Needs oracle/_ref/libref_cloud.so and libref_cloud_rev.so (oracle/ref_cloud.cc: collision/mvt.hh, capt.hh, filter.hh
and filter_centervox.hh compiled from where they lie; `make -C oracle ref`).  The inputs come from tests/cloud_pins.py;
the fixtures hold inputs (or their SHA-256 where they are regenerated from seeds), parameters and what the reference
answered.  Data only.

Tie-order certificate.  capt.hh and filter.hh sort with an unstable third-party sort, for which oracle/shim/pdqsort.h
stands in; the only thing that leaves open is the order of equal keys.  Every CAPT and scdf case is run under two
stand-ins with OPPOSITE orders of equal keys (stable, and reverse-then-stable).  A case whose every output is
byte-identical under both is committed as a pin; one that differs is flagged `tie_dependent` (it then records the
stable variant and is compared with the oracle only as such).  At most cloud_pins.MAX_TIE_DEPENDENT cases per family
may be flagged; one per family is built to be.

Cases in which the reference throws (the noexcept MVT constructor -> std::terminate, the centervox pools) run in a
child process, which records "built" or "terminated" and the what() text.

usage: tools/make_cloud_golden.py            write the four fixtures
       tools/make_cloud_golden.py --check    regenerate in memory and compare with the committed files"""
from __future__ import annotations

import ctypes
import json
import os
import pickle
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
LIB_A = os.path.join(REF_DIR, "libref_cloud.so")
LIB_B = os.path.join(REF_DIR, "libref_cloud_rev.so")
FULL_ARRAY_BYTES = 24 * 1024   # CAPT arrays above this are stored as shapes + digests
FULL_CLOUD_POINTS = 1500       # clouds above this are stored as digests (they are regenerated from their seeds)
MAX_FIXTURE_BYTES = 573126     # the largest fixture committed before these (mbm_fetch.npz)

_fp = ctypes.POINTER(ctypes.c_float)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def available():
    return os.path.exists(LIB_A) and os.path.exists(LIB_B)


def _f(a):
    return a.ctypes.data_as(_fp)


def _c(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


class RefCloud:
    """ctypes view of one variant of oracle/_ref/libref_cloud*.so"""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        S, V, f = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float
        L.ref_mvt_create.restype = L.ref_capt_create.restype = V
        L.ref_mvt_create.argtypes = [_fp, S, f, f, _fp, _fp, f]
        L.ref_capt_create.argtypes = [_fp, S, f, f, f]
        L.ref_mvt_destroy.argtypes = L.ref_capt_destroy.argtypes = [V]
        L.ref_mvt_info.argtypes = [V, _u32p, _fp]
        L.ref_capt_sizes.argtypes = [V, _u32p]
        L.ref_capt_arrays.argtypes = [V, _fp, _u32p, _fp, _fp, _fp, _fp, _fp]
        for fn in (L.ref_mvt_collides, L.ref_mvt_collides_simd, L.ref_capt_collides, L.ref_capt_collides_simd):
            fn.argtypes = [V, _fp, S, _u8p]
        L.ref_filter_scdf.restype = L.ref_filter_centervox.restype = S
        L.ref_filter_scdf.argtypes = [_fp, S, f, f, _fp, _fp, _fp, ctypes.c_int, _fp]
        L.ref_filter_centervox.argtypes = [_fp, S, f, f, _fp, _fp, _fp, _fp]
        self.reversed = bool(L.ref_ties_reversed())

    def _answers(self, fn, h, spheres, n):
        s = _c(spheres)
        out = np.zeros(n, np.uint8)
        fn(h, _f(s), n, out.ctypes.data_as(_u8p))
        return out.astype(bool)

    # -- MVT --
    def mvt(self, pts, params):
        r_min, r_max, lo, hi, r_point = params
        pts = _c(pts)
        return ctypes.c_void_p(self.L.ref_mvt_create(_f(pts), len(pts), r_min, r_max, _f(_c(lo)), _f(_c(hi)), r_point))

    def mvt_info(self, h):
        u, f = np.zeros(3, np.uint32), np.zeros(7, np.float32)
        self.L.ref_mvt_info(h, u.ctypes.data_as(_u32p), _f(f))
        return u, f

    def mvt_collides(self, h, spheres):
        return self._answers(self.L.ref_mvt_collides, h, spheres, len(spheres))

    def mvt_collides_simd(self, h, rakes):
        return self._answers(self.L.ref_mvt_collides_simd, h, rakes, len(rakes))

    # -- CAPT --
    def capt(self, pts, params):
        pts = _c(pts)
        return ctypes.c_void_p(self.L.ref_capt_create(_f(pts), len(pts), *params))

    def capt_arrays(self, h):
        u = np.zeros(5, np.uint32)
        self.L.ref_capt_sizes(h, u.ctypes.data_as(_u32p))
        nlog2, n_tests, n_starts, n_leaves, n_aff = (int(v) for v in u)
        assert n_leaves == 1 << nlog2 and n_tests == n_leaves - 1 and n_starts == n_leaves + 1
        tests, starts = np.zeros(n_tests, np.float32), np.zeros(n_starts, np.uint32)
        aabbs, aff, top = np.zeros((n_leaves, 6), np.float32), np.zeros((3, n_aff, 8), np.float32), np.zeros(6, np.float32)
        self.L.ref_capt_arrays(h, _f(tests), starts.ctypes.data_as(_u32p), _f(aabbs), _f(aff[0]), _f(aff[1]), _f(aff[2]),
                               _f(top))
        return dict(nlog2=nlog2, tests=tests, aff_starts=starts, aabbs=aabbs, aff=aff, aabb_top=top)

    def capt_collides(self, h, spheres):
        return self._answers(self.L.ref_capt_collides, h, spheres, len(spheres))

    def capt_collides_simd(self, h, rakes):
        return self._answers(self.L.ref_capt_collides_simd, h, rakes, len(rakes))

    # -- filters --
    def scdf(self, pc, min_dist, max_range, origin, lo, hi, cull):
        pc = _c(pc, (-1, 3))
        out = np.zeros((max(len(pc), 1), 3), np.float32)
        m = self.L.ref_filter_scdf(_f(pc), len(pc), min_dist, max_range, _f(_c(origin)), _f(_c(lo)), _f(_c(hi)),
                                   int(cull), _f(out))
        return out[:m].copy()

    def centervox(self, pc, voxel_size, max_range, origin, lo, hi):
        pc = _c(pc, (-1, 3))
        out = np.zeros((max(len(pc), 1), 3), np.float32)
        m = self.L.ref_filter_centervox(_f(pc), len(pc), voxel_size, max_range, _f(_c(origin)), _f(_c(lo)), _f(_c(hi)),
                                        _f(out))
        return out[:m].copy()


# ---- cases in which the reference may throw: a child process ----------------------------------------------------------
def _probe_child(path):
    with open(path, "rb") as fh:
        jobs = pickle.load(fh)
    ref = RefCloud(LIB_A)
    for i, (kind, args) in jobs:
        if kind == "mvt":
            ref.L.ref_mvt_destroy(ref.mvt(*args))
        else:
            ref.centervox(*args)
        print(f"\ndone {i}", flush=True)


def probe(jobs):
    """jobs: [(kind, args)] -> [("built", "") | ("terminated", what() text)]: the jobs run in order in a child process;
    where the child is terminated, the job it was in is recorded and a new child takes the rest"""
    result = [None] * len(jobs)
    todo = list(enumerate(jobs))
    while todo:
        with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as fh:
            pickle.dump(todo, fh)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe", fh.name], capture_output=True,
                               text=True)
        finally:
            os.unlink(fh.name)
        done = [int(m) for m in re.findall(r"^done (\d+)$", r.stdout, re.M)]
        for i in done:
            result[i] = ("built", "")
        todo = [t for t in todo if t[0] not in done]
        if r.returncode != 0:
            if r.returncode != -6:  # anything but abort() is a failure of the probe itself
                raise RuntimeError(f"probe failed with status {r.returncode}:\n{r.stderr[-2000:]}")
            what = re.search(r"what\(\):\s*(.*)", r.stderr)
            result[todo[0][0]] = ("terminated", what.group(1).strip() if what else "")
            todo = todo[1:]
        else:
            assert not todo
    return result


# ---- families ---------------------------------------------------------------------------------------------------------
def _hit_rate(hits):
    rate = float(np.mean(hits))
    assert 0.2 <= rate <= 0.8, f"hit rate {rate:.3f} outside [0.2, 0.8]"
    return round(rate, 4)


def gen_mvt(ref, _rev):
    import cloud_pins as cp
    cases = cp.mvt_cases()
    status = probe([("mvt", (pts, params)) for _, pts, params in cases])
    meta, arrays = dict(cases=[]), {}
    for idx, ((name, pts, params), (state, what)) in enumerate(zip(cases, status)):
        m = dict(name=name, n=len(pts), r_min=params[0], r_max=params[1], ws_min=list(map(float, params[2])),
                 ws_max=list(map(float, params[3])), r_point=params[4], status=state, what=what, pts_sha=cp.sha(pts),
                 pts_stored=len(pts) <= FULL_CLOUD_POINTS)
        if m["pts_stored"]:
            arrays[f"{name}__pts"] = pts
        if state == "built":
            h = ref.mvt(pts, params)
            u, f = ref.mvt_info(h)
            q = cp.mvt_queries(pts, params, 1000 + idx)
            hits, rake_hits = ref.mvt_collides(h, q["scalar"]), ref.mvt_collides_simd(h, q["rakes"])
            ref.L.ref_mvt_destroy(h)
            lo, hi = q["knife"]
            sites = cp.knife_report(hits, q)
            assert sites["live"] >= 32 and sites["dead"] == sites["other"] == 0, f"{name}: knife-edge sites {sites}"
            n_knife_rakes = min(hi - lo, len(rake_hits) // 3)   # the first rakes carry one knife-edge query each
            assert np.array_equal(rake_hits[:n_knife_rakes], hits[lo:lo + n_knife_rakes])
            m.update(grid_width=int(u[0]), capacity=int(u[1]), n_voxels=int(u[2]), seed=1000 + idx,
                     scalar_sha=cp.sha(q["scalar"]), rakes_sha=cp.sha(q["rakes"]), knife=[lo, hi],
                     knife_sites=sites, hit_rate=_hit_rate(hits), rake_hit_rate=round(float(rake_hits.mean()), 4))
            arrays[f"{name}__info"] = f            # inverse_scale_factor, global box
            arrays[f"{name}__hits"] = cp.pack(hits)
            arrays[f"{name}__rake_hits"] = cp.pack(rake_hits)
            arrays[f"{name}__expect"] = cp.pack(q["expect"])
        meta["cases"].append(m)
    return meta, arrays


def _capt_outputs(ref, pts, params, q):
    h = ref.capt(pts, params)
    a = ref.capt_arrays(h)
    out = dict(a)
    if q is not None:
        out["hits"] = ref.capt_collides(h, q["scalar"])
    if q is not None and a["nlog2"] > 0:
        # a one-point tree has no tests: collides_simd reads tests[0] of an empty vector and leaves past the only one
        # (capt.hh:445-458), which is undefined, so only the scalar answers are recorded there
        # each scalar query as a rake of eight copies of itself: collides_simd tests the top box per axis, collides by
        # distance (capt.hh:376 vs :431-438), so the two can differ at the box's corners
        out["solo_hits"] = ref.capt_collides_simd(h, np.repeat(q["scalar"][:, None, :], 8, 1))
        out["rake_hits"] = ref.capt_collides_simd(h, q["rakes"])
    ref.L.ref_capt_destroy(h)
    return out


def _check_cap(family, meta):
    import cloud_pins as cp
    flagged = [m["name"] for m in meta["cases"] if m["tie_dependent"] and m["name"] not in cp.TIE_EXEMPT[family]]
    assert 1 <= len(flagged) <= cp.MAX_TIE_DEPENDENT, f"tie-dependent {family} cases: {flagged}"


CAPT_KEYS = ("tests", "aff_starts", "aabbs", "aff", "aabb_top")


def _differing(a, b):
    """keys whose bytes differ between the two tie orders"""
    return [k for k in a if np.asarray(a[k]).shape != np.asarray(b[k]).shape or
            np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def gen_capt(ref, rev):
    import cloud_pins as cp
    meta, arrays = dict(cases=[]), {}

    def record(name, pts, params, q, seed, store_pts):
        a, b = _capt_outputs(ref, pts, params, q), _capt_outputs(rev, pts, params, q)
        m = dict(name=name, n=len(pts), r_min=params[0], r_max=params[1], r_point=params[2], pts_sha=cp.sha(pts),
                 pts_stored=store_pts, tie_dependent=bool(_differing(a, b)), tie_dependent_outputs=_differing(a, b),
                 seeded=q is not None, nlog2=a["nlog2"], n_vectors=int(a["aff"].shape[1]),
                 shapes={k: list(a[k].shape) for k in CAPT_KEYS}, sha={k: cp.sha(a[k]) for k in CAPT_KEYS})
        # what does not depend on the tie order in ANY case: nlog2 and every shape (the vector count among them)
        assert b["nlog2"] == a["nlog2"] and all(a[k].shape == b[k].shape for k in CAPT_KEYS), name
        assert q is not None or set(m["tie_dependent_outputs"]) <= {"aff"}, name
        m["arrays_stored"] = sum(a[k].nbytes for k in CAPT_KEYS) <= FULL_ARRAY_BYTES
        if store_pts:
            arrays[f"{name}__pts"] = pts
        if m["arrays_stored"]:
            for k in CAPT_KEYS:
                arrays[f"{name}__{k}"] = a[k]
        if q is not None:
            lo, hi = q["knife"]
            sites = cp.knife_report(a["hits"], q)
            assert sites["other"] == 0 and (sites["live"] >= 32 or len(pts) < 17), f"{name}: knife-edge sites {sites}"
            m.update(seed=seed, scalar_sha=cp.sha(q["scalar"]), rakes_sha=cp.sha(q["rakes"]), knife=[lo, hi],
                     knife_sites=sites,
                     hit_rate=_hit_rate(a["hits"]), simd="rake_hits" in a)
            if m["simd"]:
                m.update(rake_hit_rate=round(float(a["rake_hits"].mean()), 4),
                         scalar_differs_from_solo=int((a["hits"] != a["solo_hits"]).sum()))
            for k in ("hits", "solo_hits", "rake_hits")[:3 if m["simd"] else 1]:
                arrays[f"{name}__{k}"] = cp.pack(a[k])
            arrays[f"{name}__expect"] = cp.pack(q["expect"])
        meta["cases"].append(m)

    for idx, (name, pts, params) in enumerate(cp.capt_cases()):
        record(name, pts, params, cp.capt_queries(pts, params, 2000 + idx), 2000 + idx, True)
    survey, cloud = cp.survey_capt_cases()
    clouds = {}
    for name, (fma,), params in survey:
        if fma not in clouds:
            clouds[fma] = cloud(0, fma=fma)
        record(name, clouds[fma], params, None, None, False)
    _check_cap("capt", meta)
    return meta, arrays


def gen_scdf(ref, rev):
    import cloud_pins as cp
    meta, arrays = dict(cases=[]), {}
    stored = {}
    for name, pc, min_dist, max_range, origin, lo, hi, cull in cp.scdf_cases():
        a = ref.scdf(pc, min_dist, max_range, origin, lo, hi, cull)
        b = rev.scdf(pc, min_dist, max_range, origin, lo, hi, cull)
        digest = cp.sha(pc)
        if digest not in stored:       # the cull / min_dist variants of one cloud share its array
            stored[digest] = f"{name}__pts"
            arrays[stored[digest]] = pc
        arrays[f"{name}__kept"] = a
        meta["cases"].append(dict(name=name, n=len(pc), pts=stored[digest], pts_sha=digest, min_dist=min_dist,
                                  max_range=float(max_range), origin=list(map(float, origin)), ws_min=list(map(float, lo)),
                                  ws_max=list(map(float, hi)), cull=bool(cull), n_kept=len(a), n_kept_reversed=len(b),
                                  tie_dependent=a.shape != b.shape or a.tobytes() != b.tobytes()))
    _check_cap("scdf", meta)
    return meta, arrays


def gen_centervox(ref, _rev):
    import cloud_pins as cp
    from pins import scene_cloud
    cases = cp.centervox_cases()
    clouds = [pc if pc is not None else scene_cloud(cp.EXHAUSTION["n"], cp.EXHAUSTION["seed"]) for _, pc, *_ in cases]
    status = probe([("centervox", (pc, *c[2:])) for pc, c in zip(clouds, cases)])
    meta, arrays = dict(cases=[]), {}
    stored = {}
    for (name, given, vs, max_range, origin, lo, hi), pc, (state, what) in zip(cases, clouds, status):
        digest = cp.sha(pc)
        m = dict(name=name, n=len(pc), pts=None, pts_sha=digest, voxel_size=vs, max_range=float(max_range),
                 origin=list(map(float, origin)), ws_min=list(map(float, lo)), ws_max=list(map(float, hi)), status=state,
                 what=what)
        if given is not None:
            if digest not in stored:
                stored[digest] = f"{name}__pts"
                arrays[stored[digest]] = pc
            m["pts"] = stored[digest]
        else:
            m["seed"] = dict(cp.EXHAUSTION)
        if state == "built":
            kept = ref.centervox(pc, vs, max_range, origin, lo, hi)
            arrays[f"{name}__kept"] = kept
            m["n_kept"] = len(kept)
        meta["cases"].append(m)
    return meta, arrays


FAMILIES = dict(mvt=gen_mvt, capt=gen_capt, scdf=gen_scdf, centervox=gen_centervox)


def generate(family):
    """-> (meta, arrays) of one fixture, made now from the reference"""
    ref, rev = RefCloud(LIB_A), RefCloud(LIB_B)
    assert not ref.reversed and rev.reversed
    return FAMILIES[family](ref, rev)


def differences(family):
    """regenerate in memory and compare with the committed fixture -> list of differing keys (empty: current)"""
    import cloud_pins as cp
    meta, arrays = generate(family)
    old_meta, old = cp.load(family)
    diff = [] if json.loads(json.dumps(meta)) == old_meta else ["meta"]
    keys = set(arrays) | (set(old.files) - {"meta"})
    for k in sorted(keys):
        if k not in arrays or k not in old.files or arrays[k].dtype != old[k].dtype or \
                arrays[k].shape != old[k].shape or np.ascontiguousarray(arrays[k]).tobytes() != old[k].tobytes():
            diff.append(k)
    return diff


def main():
    import cloud_pins as cp
    if not available():
        sys.exit("oracle/_ref/libref_cloud.so is missing: run `make -C oracle ref` where the reference is present")
    if "--check" in sys.argv:
        bad = {f: d for f in FAMILIES if (d := differences(f))}
        print("fixtures are current" if not bad else f"stale: {bad}")
        sys.exit(1 if bad else 0)
    for family in FAMILIES:
        meta, arrays = generate(family)
        path = os.path.join(cp.GOLDEN, f"ref_{family}.npz")
        np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
        size = os.path.getsize(path)
        assert size <= MAX_FIXTURE_BYTES, f"{path}: {size} bytes"
        flagged = {m["name"]: m.get("tie_dependent_outputs", True) for m in meta["cases"] if m.get("tie_dependent")}
        print(f"{os.path.basename(path)}: {size} bytes, {len(meta['cases'])} cases, tie_dependent: {flagged}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--probe":
        _probe_child(sys.argv[2])
    else:
        main()
