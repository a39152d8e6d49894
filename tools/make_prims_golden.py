#!/usr/bin/env python3
"""Generates tests/golden/ref_prims.npz from the reference's own primitive narrow phase and environment loop.

Needs oracle/_ref/libref_prims.so (oracle/ref_prims.cc: collision/validity.hh with shapes.hh, environment.hh and the
sphere_*.hh predicates compiled from where they lie; `make -C oracle ref`).  The cases and queries come from
tests/prim_pins.py; the fixture holds digests of the regenerated inputs, the sorted lists as (insertion index,
min_distance), one bisection result per knife-edge segment, and three bit-packed answers per query and per rake:
`ref`, `nobreak` and `exact` (see tests/prim_pins.py).  Data only.

Pin certificate, asserted here: where ref == nobreak, exact == ref.  Queries with ref != nobreak are counted as
`break_decided`; above prim_pins.MAX_BREAK_DECIDED of a case's scalar queries (outside the radial and not-finite
families) the generator fails.  The CPU model is recorded: `ref` on break-decided queries depends on it.

usage: tools/make_prims_golden.py            write the fixture (and its row in tests/golden/README.md)
       tools/make_prims_golden.py --check    regenerate in memory and compare with the committed file"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LIB = os.path.join(ROOT, "oracle", "_ref", "libref_prims.so")
README = os.path.join(ROOT, "tests", "golden", "README.md")
MAX_FIXTURE_BYTES = 149663     # the largest ref_*.npz committed before this one (ref_capt.npz)

_fp = ctypes.POINTER(ctypes.c_float)
_u8p = ctypes.POINTER(ctypes.c_uint8)


def available():
    return os.path.exists(LIB)


def _f(a):
    return a.ctypes.data_as(_fp)


def _c(a):
    return np.ascontiguousarray(a, np.float32)


class RefEnv:
    """one environment of oracle/_ref/libref_prims.so, built from a spec [(kind, params)] in insertion order"""
    _L = None

    @classmethod
    def lib(cls):
        if cls._L is None:
            L = cls._L = ctypes.CDLL(LIB)
            S, V, f = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float
            L.ref_env_create.restype = V
            L.ref_env_destroy.argtypes = [V]
            L.ref_env_add_sphere.argtypes = [V, f, f, f, f]
            L.ref_env_add_cuboid.argtypes = L.ref_env_add_capsule.argtypes = [V, _fp]
            L.ref_env_add_heightfield.argtypes = [V, _fp, _fp, S, S, _fp]
            L.ref_env_counts.argtypes = [V, ctypes.POINTER(S)]
            L.ref_env_get_spheres.argtypes = [V, _fp]
            L.ref_env_get_cuboids.argtypes = L.ref_env_get_capsules.argtypes = [V, ctypes.c_int, _fp]
            L.ref_env_query.argtypes = L.ref_env_query_rakes.argtypes = [V, _fp, S, _u8p]
            L.ref_env_values.argtypes = [V, ctypes.c_int, S, _fp, S, _fp]
        return cls._L

    def __init__(self, spec):
        L = self.L = self.lib()
        self.h = ctypes.c_void_p(L.ref_env_create())
        for kind, p in spec:
            if kind == "sphere":
                L.ref_env_add_sphere(self.h, *(float(v) for v in p))
            elif kind == "cuboid":
                L.ref_env_add_cuboid(self.h, _f(_c(p)))
            elif kind == "capsule":
                L.ref_env_add_capsule(self.h, _f(_c(p)))
            else:
                centre, scale, xd, yd, data = p
                L.ref_env_add_heightfield(self.h, _f(_c(centre)), _f(_c(scale)), xd, yd, _f(_c(data)))

    def __del__(self):
        try:
            self.L.ref_env_destroy(self.h)
        except Exception:
            pass

    def lists(self):
        """-> {list: rows [n][width + 1]} as the reference sorted them"""
        n = (ctypes.c_size_t * 6)()
        self.L.ref_env_counts(self.h, n)
        out = {}
        for key, cnt, width, get in (("spheres", n[0], 5, lambda a: self.L.ref_env_get_spheres(self.h, _f(a))),
                                     ("capsules", n[1], 9, lambda a: self.L.ref_env_get_capsules(self.h, 0, _f(a))),
                                     ("z_capsules", n[2], 9, lambda a: self.L.ref_env_get_capsules(self.h, 1, _f(a))),
                                     ("cuboids", n[3], 16, lambda a: self.L.ref_env_get_cuboids(self.h, 0, _f(a))),
                                     ("z_cuboids", n[4], 16, lambda a: self.L.ref_env_get_cuboids(self.h, 1, _f(a)))):
            a = np.zeros((max(cnt, 1), width), np.float32)
            get(a)
            out[key] = a[:cnt]
        return out

    def query(self, spheres, rakes=False):
        """-> bool [n][3] = ref, nobreak, exact (spheres [n][4], or rakes [n][8][4])"""
        s = _c(spheres)
        n = len(s)
        out = np.zeros((n, 3), np.uint8)
        (self.L.ref_env_query_rakes if rakes else self.L.ref_env_query)(self.h, _f(s), n, out.ctypes.data_as(_u8p))
        return out.astype(bool)

    def values(self, kind, index, spheres):
        s = _c(spheres)
        out = np.zeros(len(s), np.float32)
        assert self.L.ref_env_values(self.h, kind, index, _f(s), len(s), _f(out)) == 0
        return out


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _orders(case, lists):
    """the reference's sorted rows -> (insertion index of each row, its min_distance); asserts what the lists must hold"""
    import prim_pins as pp
    order, md = {}, {}
    for name, rows in lists.items():
        if not len(rows):
            continue
        mine = [(i, p) for i, kind, p in pp.prims_of(case["spec"]) if pp.route(kind, p) == name]
        assert len(mine) == len(rows), (case["name"], name, "list assignment differs from bindings/environment.cc")
        key = {np.ascontiguousarray(p, np.float32).tobytes(): i for i, p in mine}
        assert len(key) == len(mine)
        order[name] = np.array([key[r[:-1].tobytes()] for r in rows], np.uint16)
        md[name] = rows[:, -1].copy()
        if case["order_defined"]:
            d = pp.stored_min_distance(md[name])
            assert (np.diff(d) >= 0).all(), (case["name"], name)
    return order, md


def _clearance64(case, spheres):
    """the float64 geometric clearance of every sphere (tests/geom64.py): which answer is geometrically right"""
    import geom64
    parts, _ = geom64.env_parts(case["spec"])
    cl = geom64.env_clearance(parts, spheres[:, :3].astype(np.float64), spheres[:, 3].astype(np.float64))
    return np.min(np.stack(list(cl.values())), axis=0)


def generate():
    """-> (meta, arrays), made now from the reference"""
    import prim_pins as pp
    meta = dict(cpu_model=cpu_model(), max_break_decided=pp.MAX_BREAK_DECIDED, cases=[])
    arrays = {}
    for case in pp.all_cases():
        name = case["name"]
        env = RefEnv(case["spec"])
        col = pp.ANSWERS.index(case["bisect_on"])
        q = pp.make_queries(case, answer=lambda s: env.query(s)[:, col])
        again = pp.make_queries(case, t_lo=q["t_lo"])
        assert pp.sha(again["scalar"]) == pp.sha(q["scalar"]) and pp.sha(again["rakes"]) == pp.sha(q["rakes"])
        order, md = _orders(case, env.lists())
        for k in order:
            arrays[f"{name}__{k}_order"], arrays[f"{name}__{k}_md"] = order[k], md[k]
        arrays[f"{name}__t_lo"] = q["t_lo"]
        s, r = env.query(q["scalar"]), env.query(q["rakes"], rakes=True)
        lane = env.query(q["rakes"].reshape(-1, 4)).reshape(len(r), 8, 3)
        m = dict(name=name, family=case["family"], seed=case["seed"], n_scalar=len(s), n_rakes=len(r),
                 order_defined=case["order_defined"], record=list(case["record"]), answer=case["answer"], spec_sha=pp.spec_sha(case["spec"]),
                 scalar_sha=pp.sha(q["scalar"]), rakes_sha=pp.sha(q["rakes"]),
                 hits=int(s[:, 1].sum()), rake_hits=int(r[:, 1].sum()))
        assert 0.1 * len(s) < m["hits"] < 0.9 * len(s) and 0.1 * len(r) < m["rake_hits"] < 0.9 * len(r), (name, m)
        if case["order_defined"]:
            bd, rbd = s[:, 0] != s[:, 1], r[:, 0] != r[:, 1]
            # the pin certificate.  It rests on the approximate sqrt never exceeding the exact one; the radial family
            # is built to sit where that fails (max_extent == min_distance to the last bit), and records how often
            viol = int((s[~bd, 2] != s[~bd, 0]).sum()) + int((r[~rbd, 2] != r[~rbd, 0]).sum())
            m["certificate_violations"] = viol
            assert viol == 0 or case["family"] == "radial", (name, viol)
            m["break_decided"], m["rake_break_decided"] = int(bd.sum()), int(rbd.sum())
            m["break_decided_share"] = round(float(bd.mean()), 6)
            m["ref_differs_from_exact"] = int((s[:, 0] != s[:, 2]).sum())
            if case["family"] not in pp.UNCAPPED:
                assert bd.mean() <= pp.MAX_BREAK_DECIDED, (name, m["break_decided_share"])
            # a rake's answer against the OR of its spheres' own answers (each broadcast to 8 lanes)
            m["rake_ref_differs_from_lane_or"] = int((r[:, 0] != lane[:, :, 0].any(1)).sum())
            m["rake_exact_differs_from_lane_or"] = int((r[:, 2] != lane[:, :, 2].any(1)).sum())
            m["rake_exact_differs_from_lane_or_outside_break_decided"] = int(((r[:, 2] != lane[:, :, 2].any(1)) & ~rbd).sum())
        else:
            # the reference's own order is not defined: `exact` follows that order and is kept only as a record; the
            # product's rule (a min_distance that is not finite is stored as 0) answers `nobreak`
            m["exact_differs_from_nobreak"] = int((s[:, 2] != s[:, 1]).sum())
        for i, key in enumerate(pp.ANSWERS):
            if key in case["record"]:
                arrays[f"{name}__{key}"], arrays[f"{name}__rake_{key}"] = pp.pack(s[:, i]), pp.pack(r[:, i])
        arrays[f"{name}__rake_lane_or"] = pp.pack(lane[:, :, pp.ANSWERS.index(case["answer"])].any(1))
        if case["family"] == "radial":
            arrays[f"{name}__clear64"] = _clearance64(case, q["scalar"])
            m["exact_wrong_by_geometry"] = int((s[:, 2] != (arrays[f"{name}__clear64"] < 0)).sum())
            m["ref_wrong_by_geometry"] = int((s[:, 0] != (arrays[f"{name}__clear64"] < 0)).sum())
        meta["cases"].append(m)
    return meta, arrays


def _comparable(meta):
    meta = json.loads(json.dumps(meta))
    meta.pop("cpu_model")   # recorded, not compared: a different CPU shows in the arrays if it matters
    return meta


def differences():
    """regenerate in memory and compare with the committed fixture -> list of differing keys (empty: current)"""
    import prim_pins as pp
    meta, arrays = generate()
    old_meta, old = pp.load()
    diff = [] if _comparable(meta) == _comparable(old_meta) else ["meta"]
    for k in sorted(set(arrays) | (set(old.files) - {"meta"})):
        if k not in arrays or k not in old.files or arrays[k].dtype != old[k].dtype or \
                arrays[k].shape != old[k].shape or np.ascontiguousarray(arrays[k]).tobytes() != old[k].tobytes():
            diff.append(k)
    return diff


def write_npz(path, arrays):
    """np.savez_compressed with the entries' timestamps fixed: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def readme_row(meta):
    n = len(meta["cases"])
    return ("| `ref_prims.npz` | " + str(n) + " primitive environments through the reference's own `collision/validity.hh`, `shapes.hh`, "
            "`environment.hh` and `sphere_*.hh` (compiled in place: `oracle/ref_prims.cc`): sorted lists as insertion index + "
            "`min_distance`, one bisection result per knife-edge segment, and `ref` / `nobreak` / `exact` answers per sphere and per "
            "8-lane rake (bit-packed); float64 clearances for the radial family; inputs as SHA-256 of arrays regenerated from seeds by "
            "`tests/prim_pins.py` | `tools/make_prims_golden.py` |\n")


def main():
    import prim_pins as pp
    if not available():
        sys.exit("oracle/_ref/libref_prims.so is missing: run `make -C oracle ref` where the reference is present")
    if "--check" in sys.argv:
        bad = differences()
        print("fixture is current" if not bad else f"stale: {bad}")
        sys.exit(1 if bad else 0)
    meta, arrays = generate()
    write_npz(pp.FIXTURE, dict(meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays))
    size = os.path.getsize(pp.FIXTURE)
    assert size <= MAX_FIXTURE_BYTES, f"{pp.FIXTURE}: {size} bytes"
    with open(README) as f:
        rows = [line for line in f if not line.startswith("| `ref_prims.npz`")]
    with open(README, "w") as f:
        f.writelines(rows + [readme_row(meta)])
    print(f"ref_prims.npz: {size} bytes, {len(meta['cases'])} cases")
    for m in meta["cases"]:
        print({k: v for k, v in m.items() if not k.endswith("_sha") and k not in ("seed", "record")})


if __name__ == "__main__":
    main()
