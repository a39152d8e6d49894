"""vamp_mvt_amd — MI355X-native motion validation behind the `vamp` names for this path.

Host-side mirror of the reference's Python surface for ONE hot path (reference `vamp._core`,
src/impl/vamp/bindings/{environment.cc,robot_helper.hh}): `Sphere`, `Cuboid`, `Cylinder`, `Environment`
and the per-robot modules `panda`, `ur5`, `fetch`, `baxter` with `validate`, `fk`, `dimension`,
`resolution`, `n_spheres`, `min_max_radii`, `joint_names`, `end_effector` — plus the batched calls the
reference lists as planned (`README.md:346`): `validate_batch`, `validate_motion_batch`, `fk_batch`.

Everything computes on the GPU through the C ABI (include/vamp_mvt_amd.h -> libvamp_mvt_amd.so).  There is
no CPU path: without a HIP device every compute call raises VmvError(VMV_ERR_NO_DEVICE).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import sys
import types

import numpy as np

from . import _lib
from ._lib import VmvError, check, lib

__all__ = ["robots", "Sphere", "Cuboid", "Cylinder", "Attachment", "filter_pointcloud", "HeightField", "make_heightfield", "png_to_heightfield", "Environment", "device_count", "set_device", "abi_version",
           "VmvError", "unpack_bits", "POINT_RADIUS", "IKSettings", "EEConstraint", "ConstraintSettings"]

POINT_RADIUS = 0.0025  # reference src/vamp/constants.py:25


def abi_version() -> int:
    return lib.vmv_abi_version()


def device_count() -> int:
    n = ctypes.c_int(0)
    lib.vmv_device_count(ctypes.byref(n))
    return n.value


def set_device(index: int) -> None:
    check(lib.vmv_set_device(int(index)), "vmv_set_device")


class _RobotList(list):
    """`vamp.robots` is a list in the reference package (src/vamp/__init__.py:46) and `robots()` a function in its
    extension module (bindings/python.cc.in); this is both"""

    def __call__(self):
        return list(self)


robots = _RobotList(lib.vmv_robot_name(i).decode() for i in range(lib.vmv_num_robots()))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise TypeError(f"expected float32 array of shape {shape}, got {a.shape}")
    return a


def _fp(a):
    return a.ctypes.data_as(_lib.c_float_p)


def _ptr(a, pointer_type):
    """an optional array as the library takes it: NULL for None"""
    return None if a is None else a.ctypes.data_as(pointer_type)


_SIMPLIFY_OPS = {"BSPLINE": 0, "SHORTCUT": 2}  # VMV_SIMPLIFY_*: the routines vmv_simplify_multi runs


def unpack_bits(words: np.ndarray, n: int) -> np.ndarray:
    """uint64 validity words (bit i%64 of word i//64) -> bool[n]."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


# ---------------------------------------------------------------------------------------------------------
# shapes (reference collision/shapes.hh, collision/factory.hh; Python classes of bindings/environment.cc:22-99)
# ---------------------------------------------------------------------------------------------------------
def _rotation_zyx(rho, theta, phi):
    """AngleAxis(phi, Z) * AngleAxis(theta, Y) * AngleAxis(rho, X) in fp32 (collision/factory.hh:37-39).

    Parity note: the reference evaluates this with Eigen's float AngleAxis/matrix products; Eigen is not
    available offline, so the result is equal to tolerance, not pinned bit-for-bit ("parity unpinned").
    Callers that need bit-exact primitives pass canonical parameters (`Cuboid.from_canonical`)."""
    f = np.float32
    cr, sr = f(math.cos(f(rho))), f(math.sin(f(rho)))
    ct, st = f(math.cos(f(theta))), f(math.sin(f(theta)))
    cp, sp = f(math.cos(f(phi))), f(math.sin(f(phi)))
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], np.float32)
    ry = np.array([[ct, 0, st], [0, 1, 0], [-st, 0, ct]], np.float32)
    rz = np.array([[cp, -sp, 0], [sp, cp, 0], [0, 0, 1]], np.float32)
    return (rz @ ry @ rx).astype(np.float32)


class Sphere:
    """vamp.Sphere(center, radius) — bindings/environment.cc:22-40."""

    def __init__(self, center, radius):
        c = _f32(center, (3,))
        self.x, self.y, self.z, self.r = float(c[0]), float(c[1]), float(c[2]), float(np.float32(radius))
        self.name = ""

    @property
    def position(self):
        return [self.x, self.y, self.z]

    @property
    def min_distance(self):
        f = np.float32
        return float(np.sqrt(f(self.x) * f(self.x) + f(self.y) * f(self.y) + f(self.z) * f(self.z)) - f(self.r))

    def __repr__(self):
        return f"Sphere(({self.x}, {self.y}, {self.z}), r={self.r})"


class Cuboid:
    """vamp.Cuboid(center, euler_xyz, half_extents) — collision/factory.hh:26-101."""

    def __init__(self, center, euler_xyz, half_extents):
        c, e, h = _f32(center, (3,)), _f32(euler_xyz, (3,)), _f32(half_extents, (3,))
        rot = _rotation_zyx(e[0], e[1], e[2])
        self.params = np.concatenate([c, rot[:, 0], rot[:, 1], rot[:, 2], h]).astype(np.float32)
        self.name = ""

    @classmethod
    def from_canonical(cls, params15):
        """centre xyz | axis_1 xyz | axis_2 xyz | axis_3 xyz | half extents (collision/shapes.hh:32-49)."""
        self = cls.__new__(cls)
        self.params = _f32(params15, (15,)).copy()
        self.name = ""
        return self

    x = property(lambda s: float(s.params[0]))
    y = property(lambda s: float(s.params[1]))
    z = property(lambda s: float(s.params[2]))
    # read-only parameters under the reference's names (bindings/environment.cc:60-98)
    axis_1_x, axis_1_y, axis_1_z = (property(lambda s, i=i: float(s.params[i])) for i in (3, 4, 5))
    axis_2_x, axis_2_y, axis_2_z = (property(lambda s, i=i: float(s.params[i])) for i in (6, 7, 8))
    axis_3_x, axis_3_y, axis_3_z = (property(lambda s, i=i: float(s.params[i])) for i in (9, 10, 11))
    axis_1_r, axis_2_r, axis_3_r = (property(lambda s, i=i: float(s.params[i])) for i in (12, 13, 14))

    @property
    def min_distance(self):
        """collision/shapes.hh:52-67 (computed by the C ABI's host code, the same function the kernels' tables use)"""
        e = Environment()
        e.add_cuboid(self)
        t = e.host_tables()
        return float((t["cuboids"] if len(t["cuboids"]) else t["z_cuboids"])[0, 15])


class Attachment:
    """vamp.Attachment(tf) — bindings/environment.cc:241-269, collision/attachments.hh: spheres rigidly attached at a
    frame `tf` (4 x 4) relative to the end effector.  add_sphere / add_spheres, relative_frame, set_ee_pose(tf) +
    posed_spheres (host-side float arithmetic, for inspection; the kernels pose per configuration themselves)."""

    def __init__(self, tf):
        self.relative_frame = _f32(tf, (4, 4)).copy()
        self.spheres = []
        self.posed_spheres = []

    def add_sphere(self, sphere: "Sphere"):
        self.spheres.append(sphere)

    def add_spheres(self, spheres):
        self.spheres.extend(spheres)

    def set_ee_pose(self, tf):
        n_tf = (_f32(tf, (4, 4)).astype(np.float64) @ self.relative_frame.astype(np.float64))
        self.posed_spheres = [Sphere((n_tf[:3, :3] @ np.array([s.x, s.y, s.z]) + n_tf[:3, 3]).astype(np.float32), s.r)
                              for s in self.spheres]

    def _arrays(self):
        sp = np.array([[s.x, s.y, s.z, s.r] for s in self.spheres], np.float32).reshape(-1, 4)
        return self.relative_frame.copy(), sp


def filter_pointcloud(pc, min_dist, max_range, voxel_size, origin, workcell_min, workcell_max, cull, filter_type,
                      return_device_time=False):
    """vamp.filter_pointcloud (bindings/environment.cc:183-239) -> (points [m][3] float32, nanoseconds).
    filter_type "scdf" = collision/filter.hh:175-275, "centervox" = collision/filter_centervox.hh; both run on the GPU
    and return the reference's points in the reference's order.  (The reference returns an empty list for any other
    filter_type; this raises, as its Python caller src/vamp/pointcloud.py:145 does.)"""
    if filter_type not in ("scdf", "centervox"):
        raise ValueError("filter_type must be one of: 'scdf', 'centervox'")
    pts = _f32(pc).reshape(-1, 3)
    n = pts.shape[0]
    out = np.zeros((max(n, 1), 3), np.float32)
    m, ns, dns = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib.vmv_filter_pointcloud(_fp(pts), n, float(min_dist), float(max_range), float(voxel_size), _fp(_f32(origin)),
                                    _fp(_f32(workcell_min)), _fp(_f32(workcell_max)), int(bool(cull)),
                                    0 if filter_type == "scdf" else 1, _fp(out), n, ctypes.byref(m), ctypes.byref(ns),
                                    ctypes.byref(dns)), "vmv_filter_pointcloud")
    res = out[:m.value].copy()
    return (res, int(ns.value), int(dns.value)) if return_device_time else (res, int(ns.value))


class HeightField:
    """vamp.HeightField (bindings/environment.cc:102-109, collision/shapes.hh:250-312): flattened `data` with
    xd = dimensions[0] used as the row length of the lookup (index = ys * xd + xs, sphere_heightfield.hh:22), exactly
    as the reference does.  xs, ys, zs are the reciprocal scales (collision/factory.hh:376-386)."""

    def __init__(self, center, scaling, dimensions, data):
        self.center = _f32(center).reshape(3).copy()
        self.scaling = _f32(scaling).reshape(3).copy()
        self.xd, self.yd = int(dimensions[0]), int(dimensions[1])
        self.data = _f32(data).reshape(-1).copy()
        if self.data.size != self.xd * self.yd:
            raise TypeError("data must hold dimensions[0] * dimensions[1] values")
        self.x, self.y, self.z = (float(v) for v in self.center)
        one = np.float32(1.0)
        self.xs, self.ys, self.zs = (float(one / v) for v in self.scaling)


def make_heightfield(center, scaling, dimensions, data) -> HeightField:
    """vamp.make_heightfield (bindings/environment.cc:100)."""
    return HeightField(center, scaling, dimensions, data)


def png_to_heightfield(filename, center, scaling) -> HeightField:
    """vamp.png_to_heightfield (reference src/vamp/__init__.py:54-66): grey-scale image / 255, flipped vertically;
    dimensions = array.shape, as the reference passes them."""
    from PIL import Image  # same optional dependency as the reference

    array = np.asarray(Image.open(filename).convert("L")) * 1 / 255.0
    array = np.flip(array, axis=0)
    return make_heightfield(center, scaling, array.shape, list(array.flatten()))


class Cylinder:
    """vamp.Cylinder(center, euler_xyz, radius, length) | Cylinder(endpoint1, endpoint2, radius)
    — collision/factory.hh:104-223; the environment treats it as a capsule (environment.cc:134-147)."""

    def __init__(self, *args):
        f = np.float32
        if len(args) == 4:
            c, e = _f32(args[0], (3,)), _f32(args[1], (3,))
            radius, length = f(args[2]), f(args[3])
            rot = _rotation_zyx(e[0], e[1], e[2])
            half = f(length / f(2))
            p1 = (c + rot[:, 2] * half).astype(np.float32)
            p2 = (c - rot[:, 2] * half).astype(np.float32)
        elif len(args) == 3:
            p1, p2, radius = _f32(args[0], (3,)), _f32(args[1], (3,)), f(args[2])
        else:
            raise TypeError("Cylinder(center, euler_xyz, radius, length) or Cylinder(endpoint1, endpoint2, radius)")
        v = (p2 - p1).astype(np.float32)
        dot = f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2])
        rdv = f(1.0 / float(dot))  # static_cast<float>(1.0 / dot): double division, then narrowed
        self.params = np.array([p1[0], p1[1], p1[2], v[0], v[1], v[2], radius, rdv], np.float32)
        self.name = ""

    # read-only parameters under the reference's names (bindings/environment.cc:42-58)
    x1, y1, z1, xv, yv, zv, r, rdv = (property(lambda s, i=i: float(s.params[i])) for i in range(8))
    x2 = property(lambda s: float(np.float32(s.params[0]) + np.float32(s.params[3])))
    y2 = property(lambda s: float(np.float32(s.params[1]) + np.float32(s.params[4])))
    z2 = property(lambda s: float(np.float32(s.params[2]) + np.float32(s.params[5])))

    @property
    def min_distance(self):
        """collision/shapes.hh:165-189"""
        e = Environment()
        e.add_capsule(self)
        t = e.host_tables()
        return float((t["capsules"] if len(t["capsules"]) else t["z_capsules"])[0, 8])

    @classmethod
    def from_canonical(cls, params8):
        """x1 y1 z1 | xv yv zv | r | rdv (collision/shapes.hh:128-143)."""
        self = cls.__new__(cls)
        self.params = _f32(params8, (8,)).copy()
        self.name = ""
        return self


class Environment:
    """vamp.Environment — bindings/environment.cc:111-163 (write-only from Python there, too).

    Host-side this is a recipe; the device image is (re)built lazily by the C ABI on first use after a change
    (the reference re-sorts on every add and converts the whole environment on every call)."""

    def __init__(self):
        self._ops = []
        self._handle = None
        self._device = None
        self._generation = 0  # handles destroyed so far: what holds a handle beyond one call (DeviceRoadmaps) compares it

    # -- mutation ------------------------------------------------------------------------------------------
    def _dirty(self):
        if self._handle is not None:
            lib.vmv_env_destroy(self._handle)
            self._handle = None
            self._generation += 1

    def add_sphere(self, sphere: Sphere):
        self._ops.append(("sphere", (sphere.x, sphere.y, sphere.z, sphere.r)))
        self._dirty()

    def add_cuboid(self, cuboid: Cuboid):
        self._ops.append(("cuboid", cuboid.params.copy()))
        self._dirty()

    def add_capsule(self, capsule: Cylinder):
        self._ops.append(("capsule", capsule.params.copy()))
        self._dirty()

    def attach(self, attachment: Attachment):
        """Environment.attach (environment.cc:178-180): at most one attachment; a later one replaces it."""
        self._ops = [op for op in self._ops if op[0] != "attach"]
        self._ops.append(("attach", attachment._arrays()))
        self._dirty()

    def detach(self):
        self._ops = [op for op in self._ops if op[0] != "attach"]
        self._dirty()

    def add_heightfield(self, heightfield: HeightField):
        self._ops.append(("heightfield", heightfield))
        self._dirty()

    def add_capt_pointcloud(self, points, r_min, r_max, r_point, build="host", return_device_time=False):
        """-> CAPT build time in nanoseconds (environment.cc:152-163).  build="gpu" builds the same arrays on the
        device (csrc/vmv_capt_gpu.hip); with return_device_time also the HIP-event time of the device work alone."""
        if build not in ("host", "gpu"):
            raise ValueError("build must be 'host' or 'gpu'")
        pts = _f32(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise TypeError("points must be [n][3]")
        self._ops.append(("capt_gpu" if build == "gpu" else "capt", (pts.copy(), float(r_min), float(r_max), float(r_point))))
        self._dirty()
        # build once now to report the time, as the reference does
        h = ctypes.c_void_p()
        check(lib.vmv_env_create(ctypes.byref(h)), "vmv_env_create")
        ns, dns = ctypes.c_uint64(0), ctypes.c_uint64(0)
        try:
            if build == "gpu":
                check(lib.vmv_env_add_capt_pointcloud_gpu(h, _fp(pts), pts.shape[0], r_min, r_max, r_point, ctypes.byref(ns),
                                                          ctypes.byref(dns)), "vmv_env_add_capt_pointcloud_gpu")
            else:
                check(lib.vmv_env_add_capt_pointcloud(h, _fp(pts), pts.shape[0], r_min, r_max, r_point, ctypes.byref(ns)),
                      "vmv_env_add_capt_pointcloud")
        finally:
            lib.vmv_env_destroy(h)
        return (int(ns.value), int(dns.value)) if return_device_time else int(ns.value)

    def add_mvt_pointcloud(self, points, r_min, r_max, workspace_aabb_min, workspace_aabb_max, r_point):
        """-> MVT build time in nanoseconds (environment.cc:164-177).  Raises VmvError(VMV_ERR_CAPACITY) where the
        reference would terminate on an exhausted pool (mvt.hh:634-648)."""
        pts = _f32(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise TypeError("points must be [n][3]")
        lo, hi = _f32(workspace_aabb_min, (3,)), _f32(workspace_aabb_max, (3,))
        h = ctypes.c_void_p()
        check(lib.vmv_env_create(ctypes.byref(h)), "vmv_env_create")
        ns = ctypes.c_uint64(0)
        try:
            check(lib.vmv_env_add_mvt_pointcloud(h, _fp(pts), pts.shape[0], r_min, r_max, _fp(lo), _fp(hi), r_point,
                                                 ctypes.byref(ns), None), "vmv_env_add_mvt_pointcloud")
        finally:
            lib.vmv_env_destroy(h)
        self._ops.append(("mvt", (pts.copy(), float(r_min), float(r_max), lo.copy(), hi.copy(), float(r_point))))
        self._dirty()
        return int(ns.value)

    def __del__(self):
        try:
            self._dirty()
        except Exception:
            pass

    # -- device image ----------------------------------------------------------------------------------------
    def _build(self, finalize=True):
        h = ctypes.c_void_p()
        check(lib.vmv_env_create(ctypes.byref(h)), "vmv_env_create")
        try:
            for kind, arg in self._ops:
                if kind == "sphere":
                    check(lib.vmv_env_add_sphere(h, *arg), "vmv_env_add_sphere")
                elif kind == "cuboid":
                    check(lib.vmv_env_add_cuboid(h, _fp(arg)), "vmv_env_add_cuboid")
                elif kind == "capsule":
                    check(lib.vmv_env_add_capsule(h, _fp(arg)), "vmv_env_add_capsule")
                elif kind == "attach":
                    tf, sp = arg
                    check(lib.vmv_env_attach(h, _fp(tf), _fp(sp), sp.shape[0]), "vmv_env_attach")
                elif kind == "heightfield":
                    check(lib.vmv_env_add_heightfield(h, _fp(arg.center), _fp(arg.scaling), arg.xd, arg.yd, _fp(arg.data)),
                          "vmv_env_add_heightfield")
                elif kind == "mvt":
                    pts, r_min, r_max, lo, hi, r_point = arg
                    check(lib.vmv_env_add_mvt_pointcloud(h, _fp(pts), pts.shape[0], r_min, r_max, _fp(lo), _fp(hi),
                                                         r_point, None, None), "vmv_env_add_mvt_pointcloud")
                elif kind == "capt_gpu":
                    pts, r_min, r_max, r_point = arg
                    check(lib.vmv_env_add_capt_pointcloud_gpu(h, _fp(pts), pts.shape[0], r_min, r_max, r_point, None, None),
                          "vmv_env_add_capt_pointcloud_gpu")
                else:
                    pts, r_min, r_max, r_point = arg
                    check(lib.vmv_env_add_capt_pointcloud(h, _fp(pts), pts.shape[0], r_min, r_max, r_point, None),
                          "vmv_env_add_capt_pointcloud")
            if finalize:
                check(lib.vmv_env_finalize(h), "vmv_env_finalize")
        except Exception:
            lib.vmv_env_destroy(h)
            raise
        return h

    def handle(self):
        """Finalized C-ABI handle (sorted + uploaded to the current device; rebuilt if the device changed)."""
        dev = ctypes.c_int(-1)
        lib.vmv_get_device(ctypes.byref(dev))
        if self._handle is not None and self._device != dev.value:
            self._dirty()
        if self._handle is None:
            self._handle = self._build()
            self._device = dev.value
        return self._handle

    def spheres_in_collision(self, spheres):
        """sphere_environment_in_collision (collision/validity.hh:47-158) for free spheres [n][4] = x y z r -> bool[n]
        (each sphere on its own: primitive lists, heightfields, CAPT and MVT clouds)."""
        s = _f32(spheres)
        if s.ndim != 2 or s.shape[1] != 4:
            raise TypeError("spheres must be [n][4] = x y z r")
        hits = np.zeros(s.shape[0], np.uint8)
        check(lib.vmv_spheres_in_collision_batch_host(self.handle(), _fp(s), s.shape[0],
                                                      hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
              "vmv_spheres_in_collision_batch_host")
        return hits.astype(bool)

    def robot_part(self, robot):
        """What this environment holds for `robot` (a robot module or its name), built by `<robot>.prepare` or by the
        first use: {"grids": four of {"dims", "origin", "inv_cell", "cells" uint32[dx][dy][dz][words]} or None (no
        broad-phase grid), "link_skip", "static_hit"}.  Builds the part the first-use way if it is not built yet."""
        rid = robot._id if isinstance(robot, _Robot) else lib.vmv_robot_id(str(robot).encode())
        h = self.handle()
        grids = []
        for c in range(4):
            dims, origin = np.zeros(3, np.uint32), np.zeros(3, np.float32)
            inv_cell, words = ctypes.c_float(0), ctypes.c_uint32(0)
            check(lib.vmv_env_grid_info(h, rid, c, dims.ctypes.data_as(_lib.c_u32_p), _fp(origin), ctypes.byref(inv_cell),
                                        ctypes.byref(words)), "vmv_env_grid_info")
            if not dims.any():
                grids.append(None)
                continue
            cells = np.zeros((int(dims[0]), int(dims[1]), int(dims[2]), int(words.value)), np.uint32)
            n = ctypes.c_size_t(0)
            check(lib.vmv_env_grid_cells(h, rid, c, cells.ctypes.data_as(_lib.c_u32_p), cells.size, ctypes.byref(n)),
                  "vmv_env_grid_cells")
            if n.value != cells.size:
                raise RuntimeError(f"grid {c}: {n.value} cell words, expected {cells.size}")
            grids.append(dict(dims=dims, origin=origin, inv_cell=float(inv_cell.value), cells=cells))
        skip, hit = ctypes.c_uint64(0), ctypes.c_uint32(0)
        check(lib.vmv_env_robot_flags(h, rid, ctypes.byref(skip), ctypes.byref(hit)), "vmv_env_robot_flags")
        return dict(grids=grids, link_skip=int(skip.value), static_hit=int(hit.value))

    # -- inspection (host tables; no GPU needed) ----------------------------------------------------------------
    def host_tables(self):
        """Sorted primitive tables as the kernels see them (built without uploading)."""
        h = self._build(finalize=False)
        try:
            counts = (ctypes.c_size_t * 6)()
            check(lib.vmv_env_counts(h, counts), "vmv_env_counts")
            n = ctypes.c_size_t(0)
            out = {}
            sp = np.zeros((max(counts[0], 1), 5), np.float32)
            lib.vmv_env_get_spheres(h, _fp(sp), counts[0], ctypes.byref(n))
            out["spheres"] = sp[:counts[0]]
            for key, z, cnt, width, fn in (("cuboids", 0, counts[3], 16, lib.vmv_env_get_cuboids),
                                           ("z_cuboids", 1, counts[4], 16, lib.vmv_env_get_cuboids),
                                           ("capsules", 0, counts[1], 9, lib.vmv_env_get_capsules),
                                           ("z_capsules", 1, counts[2], 9, lib.vmv_env_get_capsules)):
                a = np.zeros((max(cnt, 1), width), np.float32)
                fn(h, z, _fp(a), cnt, ctypes.byref(n))
                out[key] = a[:cnt]
            capts = []
            for i in range(counts[5]):
                nlog2, naff = ctypes.c_uint32(0), ctypes.c_uint32(0)
                check(lib.vmv_env_capt_sizes(h, i, ctypes.byref(nlog2), ctypes.byref(naff)), "vmv_env_capt_sizes")
                leaves = 1 << nlog2.value
                t = np.zeros(leaves - 1, np.float32)
                st = np.zeros(leaves + 1, np.uint32)
                bb = np.zeros((leaves, 6), np.float32)
                aff = np.zeros((3, naff.value, 8), np.float32)
                top = np.zeros(6, np.float32)
                check(lib.vmv_env_capt_arrays(h, i, _fp(t), st.ctypes.data_as(_lib.c_u32_p), _fp(bb), _fp(aff[0]),
                                              _fp(aff[1]), _fp(aff[2]), _fp(top)), "vmv_env_capt_arrays")
                capts.append(dict(nlog2=nlog2.value, tests=t, aff_starts=st, aabbs=bb, aff=aff, aabb_top=top))
            out["capt"] = capts
            return out
        finally:
            lib.vmv_env_destroy(h)


# ---------------------------------------------------------------------------------------------------------
# per-robot modules (reference bindings/robot_helper.hh:326-597, path subset + batched calls)
# ---------------------------------------------------------------------------------------------------------
_NO_ENVIRONMENT = object()  # _Robot._batched: the call takes no environment
_NO_CONTEXT = contextlib.nullcontext()
# a zero-length ctypes array at a numpy buffer passes where the pointer type is declared, at half the cost of
# ndarray.ctypes.data_as (which dominates the Python side of a one-configuration call); the caller holds the array
_AT = {t: (t._type_ * 0).from_address for t in (_lib.c_float_p, _lib.c_u64_p, _lib.c_u32_p)}
_OUTPUT_DTYPES = {"bits": ("int64", np.uint64), "f32": ("float32", np.float32), "u32": ("int32", np.uint32)}  # torch, numpy


def _is_torch_cuda(x):
    t = sys.modules.get("torch")
    return t is not None and isinstance(x, t.Tensor) and x.is_cuda


def _check_environments(environments):
    for e in environments:
        if e is not None and not isinstance(e, Environment):
            raise TypeError(f"expected Environment or None, got {type(e).__name__}")


def _env_handles(environments):
    """-> (the Environment objects, the empty environment for None; the c_void_p array of their finalized handles).
    The caller holds the list until the library call has returned: the handles live as long as the objects."""
    envs = [_EMPTY_ENVIRONMENT if e is None else e for e in environments]
    return envs, (ctypes.c_void_p * max(len(envs), 1))(*[e.handle() for e in envs])


def _segments(environments, counts):
    """one count per environment -> (the environments as a checked list, uint64[n + 1]: the exclusive offsets and the total)"""
    environments, counts = list(environments), np.asarray(counts)
    if counts.ndim != 1 or len(counts) != len(environments):
        raise ValueError(f"expected one count per environment, got {counts.shape} counts for {len(environments)}")
    if counts.size and (not np.issubdtype(counts.dtype, np.integer) or (counts < 0).any()):
        raise ValueError("counts must be non-negative integers")
    _check_environments(environments)
    return environments, np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.uint64)


# the planner wrappers (<robot>.*_raw) are composed from the helpers below: one copy of every shared check and of the readout
def _endpoints(dim, starts, goals):
    """starts and goals as two float32 [n][dim] arrays -> (starts, goals, n)"""
    a, b = _f32(starts), _f32(goals)
    if a.ndim != 2 or a.shape[1] != dim or a.shape != b.shape:
        raise TypeError(f"expected two [n][{dim}] arrays")
    return a, b, a.shape[0]


def _one_per(environments, n, what):
    """one environment per `what` ("problem", "path")"""
    if len(environments) != n:
        raise ValueError(f"expected one environment per {what}, got {len(environments)} for {n} {what}s")


def _skips(skips, n, what, draws=None):
    """one Halton skip per `what` ("problem", "roadmap") -> uint64[n], None for None; draws: the samples a call takes
    from the sequence, where it is held to the sequence's validity limit"""
    if skips is None:
        return None
    sk = np.asarray(skips)
    if sk.shape != (n,):
        raise ValueError(f"expected one skip per {what}, got shape {sk.shape} for {n} {what}s")
    if sk.size and (not np.issubdtype(sk.dtype, np.integer) or (sk < 0).any()):
        raise ValueError("skips must be non-negative integers")
    if draws is not None and sk.size and int(sk.max()) + draws > 1000000:
        raise ValueError("skip + n_samples may not exceed 1,000,000 (the Halton sequence's validity limit)")
    return np.ascontiguousarray(sk, np.uint64)


def _samples(samples, n, ns, dim):
    """the caller's samples, [ns][dim] for all or [n][ns][dim] -> float32 [n][ns][dim], None for None"""
    if samples is None:
        return None
    sm = _f32(samples)
    if sm.shape == (ns, dim):
        sm = np.ascontiguousarray(np.broadcast_to(sm, (n, ns, dim)))
    if sm.shape != (n, ns, dim):
        raise TypeError(f"expected samples as [{ns}][{dim}] or [{n}][{ns}][{dim}]")
    return sm


def _rrtc_settings_struct(settings, also=()):
    """vmv_rrtc_settings from an RRTCMultiSettings-shaped object, checked as rrtc_multi_raw documents; also: further
    fields of the settings that must fit 32 bits, named in the same refusal"""
    rng, ratio = float(settings.range), float(settings.tree_ratio)
    max_it, max_s, every = int(settings.max_iterations), int(settings.max_samples), int(getattr(settings, "check_every", 0))
    if not (math.isfinite(rng) and rng > 0):
        raise ValueError("range must be finite and positive")
    if not (0 <= max_it < 2 ** 32 and 2 <= max_s < 2 ** 32 and 0 <= every < 2 ** 32 and
            all(0 <= int(getattr(settings, k)) < 2 ** 32 for k in also)):
        raise ValueError("max_iterations, max_samples (>= 2)" + "".join(f", {k}" for k in also) +
                         " and check_every must fit 32 bits")
    return _lib.RrtcSettings(rng, int(bool(settings.balance)), ratio, max_it, max_s, every)


def _cut_radius(settings):
    """-> the radius beyond which no neighbour is taken, checked"""
    radius = float(settings.radius)
    if not radius > 0:
        raise ValueError("radius must be positive (inf = no cut)")
    return radius


def _roadmap_sampling(settings):
    """-> (n_samples, k, radius) of a PRMMultiSettings- or RoadmapsSettings-shaped object, checked"""
    ns, k = int(settings.n_samples), int(settings.k)
    if ns % 64 != 0 or not 64 <= ns <= 8128:
        raise ValueError("n_samples must be a multiple of 64 from 64 to 8,128")
    if not 1 <= k <= 16:
        raise ValueError("k must be from 1 to 16")
    return ns, k, _cut_radius(settings)


def _waypoints(path, dim):
    """one path -> float32 [len][dim] (an empty path: [0][dim])"""
    a = np.asarray(path, dtype=np.float32)
    if a.size == 0:
        a = np.zeros((0, dim), np.float32)
    if a.ndim != 2 or a.shape[1] != dim:
        raise TypeError(f"expected every path as [len][{dim}] waypoints")
    return a


def _packed_paths(paths, dim):
    """-> (the paths as a list of float32 [len][dim] arrays, their waypoints packed, uintp[n + 1] offsets into those)"""
    pts = [_waypoints(p, dim) for p in paths]
    offsets = np.zeros(len(pts) + 1, np.uintp)
    offsets[1:] = np.cumsum([len(a) for a in pts], dtype=np.int64)
    return pts, np.ascontiguousarray(np.concatenate(pts + [np.zeros((0, dim), np.float32)])), offsets


def _read_plans(plans, n, dim, extra=None):
    """What every vmv_plans handle of n problems answers -> dict(status, iterations, sizes [n][2], path_lengths, paths
    [sum(path_lengths)][dim], rounds, questions); extra(plans, out) adds the call's own part while the handle lives.
    Destroys the handle, whatever happens."""
    try:
        status, iterations = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        sizes, lengths = np.zeros((n, 2), np.uint32), np.zeros(n, np.uint32)
        rounds, questions = ctypes.c_uint64(0), ctypes.c_uint64(0)
        counts = [x.ctypes.data_as(_lib.c_u32_p) for x in (iterations, sizes, lengths)]
        totals = [ctypes.byref(rounds), ctypes.byref(questions)]
        check(lib.vmv_plans_summary(plans, status.ctypes.data_as(_lib.c_u8_p), *counts, *totals), "vmv_plans_summary")
        paths = np.zeros((int(lengths.sum()), dim), np.float32)
        check(lib.vmv_plans_paths(plans, _fp(paths), paths.size), "vmv_plans_paths")
        out = dict(status=status, iterations=iterations, sizes=sizes, path_lengths=lengths, paths=paths,
                   rounds=int(rounds.value), questions=int(questions.value))
        if extra is not None:
            extra(plans, out)
    finally:
        lib.vmv_plans_destroy(plans)
    return out


def _read_result(n, entry, readout, destroy):
    """The life cycle of a path call's result handle, as `_read_plans` has it for the planners: nothing for n == 0 (->
    None: the caller's zeros stand and the library is not touched); else entry(byref(handle)), the checked entry call,
    then -> readout(handle) while the handle lives; `destroy` (a symbol's name) runs whatever happens."""
    if n == 0:
        return None
    out = ctypes.c_void_p()
    entry(ctypes.byref(out))
    try:
        return readout(out)
    finally:
        getattr(lib, destroy)(out)


def _torch_unpack_bits(bits, n):
    """unpack_bits for a torch int64 tensor of validity words -> torch.bool[n] on the same device"""
    import torch

    shifts = torch.arange(64, device=bits.device, dtype=torch.int64)
    return (((bits[:, None] >> shifts[None, :]) & 1) != 0).reshape(-1)[:n]


def _simplify_settings_struct(settings, longest=0):
    """vmv_simplify_settings from a SimplifyMultiSettings-shaped object, checked as simplify_multi_raw documents;
    longest: the longest input path in waypoints"""
    ops = []
    for op in settings.operations:
        name = str(getattr(op, "name", op)).upper()
        if name in ("REDUCE", "PERTURB"):
            raise NotImplementedError(f"{name} draws random numbers: simplify_multi runs SHORTCUT and BSPLINE only")
        if name not in _SIMPLIFY_OPS:
            raise ValueError(f"unknown simplification routine {op!r}")
        ops.append(_SIMPLIFY_OPS[name])
    if len(ops) > 8:
        raise ValueError("at most 8 operations per iteration")
    if int(getattr(settings, "interpolate", 0)) != 0:
        raise NotImplementedError("interpolate is not part of simplify_multi: interpolate the returned paths")
    max_it, max_steps = int(settings.max_iterations), int(settings.max_steps)
    max_wp, w = int(getattr(settings, "max_waypoints", 0)), int(getattr(settings, "questions_per_round", 0))
    every = int(getattr(settings, "check_every", 0))
    if not (0 <= max_it < 2 ** 32 and 0 <= max_steps < 2 ** 32 and 0 <= every < 2 ** 32 and 0 <= max_wp <= 2 ** 24):
        raise ValueError("max_iterations, max_steps and check_every must fit 32 bits, max_waypoints 24")
    if w not in (0, 2, 4, 8, 16, 32, 64):
        raise ValueError("questions_per_round must be one of 2, 4, 8, 16, 32, 64 (0 = default)")
    if longest > (max_wp or 2048):
        raise ValueError(f"max_waypoints is below the longest path ({longest} waypoints)")
    return _lib.SimplifySettings(max_it, 0, len(ops), (ctypes.c_uint32 * 8)(*ops), max_steps, float(settings.min_change),
                               float(settings.midpoint_interpolation), max_wp, w, every)


def _optimize_settings_struct(settings, longest=0):
    """vmv_optimize_settings from an OptimizeMultiSettings-shaped object, checked as the library checks it; longest: the
    longest input path in waypoints"""
    max_it, every, max_wp = int(settings.max_iterations), int(settings.validate_every), int(settings.max_waypoints)
    if not (0 < max_it < 2 ** 32 and 0 < every < 2 ** 32):
        raise ValueError("max_iterations and validate_every must be positive and fit 32 bits")
    if not 0 < max_wp <= 1024:
        raise ValueError("max_waypoints must be between 1 and 1,024")
    if longest > max_wp:
        raise ValueError(f"max_waypoints is below the longest path ({longest} waypoints)")
    positive = {k: float(getattr(settings, k)) for k in ("step", "max_step", "env_margin", "self_margin")}
    weights = {k: float(getattr(settings, k)) for k in ("smooth_weight", "env_weight", "self_weight")}
    for k, v in positive.items():
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{k} must be positive and finite")
    for k, v in weights.items():
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{k} must be finite and not negative")
    if np.isnan(float(settings.min_change)):
        raise ValueError("min_change must not be NaN")
    return _lib.OptimizeSettings(max_it, every, positive["step"], positive["max_step"], float(settings.min_change),
                                 weights["smooth_weight"], weights["env_weight"], weights["self_weight"],
                                 positive["env_margin"], positive["self_margin"], max_wp)


def _cartesian_settings_struct(settings):
    """vmv_cartesian_settings from a CartesianSettings-shaped object, checked as the library checks it (0 or a negative
    number asks for the library's default)"""
    names = ("pos_step", "rot_step", "pos_tol", "rot_tol", "rot_weight", "damping", "max_step", "max_joint_step")
    values = {k: float(getattr(settings, k)) for k in names}
    for k, v in values.items():
        if not np.isfinite(v):
            raise ValueError(f"{k} must be finite")
    max_it, max_wp = int(settings.max_iterations), int(settings.max_waypoints)
    if not 0 <= max_it < 2 ** 30:
        raise ValueError("max_iterations must be from 0 (default) to 2^30 - 1")
    if not 0 <= max_wp <= 1024:
        raise ValueError("max_waypoints must be from 0 (default) to 1,024")
    return _lib.CartesianSettings(values["pos_step"], values["rot_step"], max_it, values["pos_tol"], values["rot_tol"],
                                  values["rot_weight"], values["damping"], values["max_step"], values["max_joint_step"],
                                  max_wp, int(bool(settings.position_only)))


def _retime_settings_struct(settings):
    """vmv_retime_settings from a RetimeSettings-shaped object, checked as the library checks it (0 or a negative number
    asks for the library's default)"""
    values = {k: float(getattr(settings, k)) for k in ("blend", "grid_step", "dt")}
    for k, v in values.items():
        if not np.isfinite(v):
            raise ValueError(f"{k} must be finite")
    for k in ("grid_step", "dt"):
        if 0 < values[k] < 1e-6:
            raise ValueError(f"{k} must be at least 1e-6 (0 = default)")
    max_grid, max_samples = int(settings.max_grid), int(settings.max_samples)
    if not 0 <= max_grid <= 4096:
        raise ValueError("max_grid must be from 0 (default) to 4,096")
    if not 0 <= max_samples < 2 ** 32:
        raise ValueError("max_samples must be from 0 (default) and fit 32 bits")
    return _lib.RetimeSettings(values["blend"], values["grid_step"], values["dt"], max_grid, max_samples,
                               int(bool(settings.stop_at_waypoints)))


def _retime_constrained_settings_struct(settings):
    """vmv_retime_constrained_settings from a RetimeConstrainedSettings-shaped object, checked as the library checks it"""
    base = _retime_settings_struct(settings)
    halvings, max_rounds = int(settings.blend_halvings), int(settings.max_rounds)
    if not 0 <= halvings <= 8:
        raise ValueError("blend_halvings must be from 0 (default) to 8")
    if not 0 <= max_rounds < 2 ** 32:
        raise ValueError("max_rounds must be from 0 (default) and fit 32 bits")
    return _lib.RetimeConstrainedSettings(base, halvings, max_rounds)


def _joint_limits(limits, dim, name):
    """-> float32 [dim], every entry finite and positive"""
    a = _f32(limits)
    if a.shape != (dim,):
        raise TypeError(f"expected {name} as [{dim}] values")
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError(f"{name} must be finite and positive")
    return a


class IKSettings:
    """vmv_ik_settings (include/vamp_mvt_amd.h) with the defaults of <robot>.ik_batch: n_seeds seeds per target (1 ..
    1,024), max_iterations, pos_tol (m), rot_tol (rad; the sine of the residual angle is compared), rot_weight (metres per
    radian: the weight of the rotation rows), damping (the initial lambda), max_step (the largest joint change of one
    step), position_only (the orientation is free)."""

    def __init__(self, n_seeds=32, max_iterations=64, pos_tol=1e-4, rot_tol=1e-3, rot_weight=0.25, damping=1e-2,
                 max_step=0.5, position_only=False):
        self.n_seeds, self.max_iterations = n_seeds, max_iterations
        self.pos_tol, self.rot_tol, self.rot_weight = pos_tol, rot_tol, rot_weight
        self.damping, self.max_step, self.position_only = damping, max_step, position_only

    def struct(self):
        return _lib.IkSettings(int(self.n_seeds), int(self.max_iterations), float(self.pos_tol), float(self.rot_tol),
                               float(self.rot_weight), float(self.damping), float(self.max_step), int(bool(self.position_only)))

    def __repr__(self):
        return "IKSettings(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items()) + ")"


class EEConstraint:
    """vmv_ee_constraint (include/vamp_mvt_amd.h): a tolerance band on the end-effector frame (R, t).  frame: the rigid
    4 x 4 frame C in the world (None = the world itself); pos_lo / pos_hi: bounds on p = C_R^T (t - C_t) per axis (None =
    free; equal bounds are a plane or a line); the angle between R tool_axis and C_R ref_axis is at most max_angle (rad, at
    most pi/2; 0 = the orientation is free).  The library normalises the axes and refuses what is not a constraint."""

    def __init__(self, frame=None, pos_lo=None, pos_hi=None, tool_axis=(0.0, 0.0, 1.0), ref_axis=(0.0, 0.0, 1.0), max_angle=0.0):
        self.frame = np.eye(4, dtype=np.float32) if frame is None else _f32(frame).reshape(-1)
        if self.frame.size != 16:
            raise TypeError("expected frame as a 4 x 4 matrix")
        self.frame = self.frame.reshape(4, 4)
        self.pos_lo = np.full(3, -np.inf, np.float32) if pos_lo is None else _f32(pos_lo, (3,))
        self.pos_hi = np.full(3, np.inf, np.float32) if pos_hi is None else _f32(pos_hi, (3,))
        self.tool_axis, self.ref_axis = _f32(tool_axis, (3,)), _f32(ref_axis, (3,))
        self.max_angle = float(max_angle)

    @classmethod
    def upright(cls, tool_axis, max_angle, frame=None):
        """tool_axis (in the end-effector frame) stays within max_angle of the z axis of `frame` (None = the world's)"""
        return cls(frame=frame, tool_axis=tool_axis, ref_axis=(0.0, 0.0, 1.0), max_angle=max_angle)

    @classmethod
    def box(cls, lo, hi, frame=None):
        """the end-effector position stays within [lo, hi] along the axes of `frame` (None = the world)"""
        return cls(frame=frame, pos_lo=lo, pos_hi=hi)

    def struct(self):
        c = _lib.EeConstraint()
        c.frame[:] = self.frame.reshape(-1).tolist()
        c.pos_lo[:], c.pos_hi[:] = self.pos_lo.tolist(), self.pos_hi.tolist()
        c.tool_axis[:], c.ref_axis[:] = self.tool_axis.tolist(), self.ref_axis.tolist()
        c.max_angle = self.max_angle
        return c

    def __repr__(self):
        return "EEConstraint(" + ", ".join(f"{k}={np.asarray(v).tolist()!r}" for k, v in vars(self).items()) + ")"


class ConstraintSettings:
    """vmv_constraint_settings (include/vamp_mvt_amd.h) with its defaults: max_iterations evaluations after the first;
    pos_tol (m) and rot_tol (rad) widen the nominal band into the one every test asks; rot_weight, damping and max_step
    as IKSettings'; check_step: the joint-space distance between two band samples of an edge."""

    def __init__(self, max_iterations=16, pos_tol=1e-4, rot_tol=1e-3, rot_weight=0.25, damping=1e-2, max_step=0.5,
                 check_step=0.05):
        self.max_iterations, self.pos_tol, self.rot_tol = max_iterations, pos_tol, rot_tol
        self.rot_weight, self.damping, self.max_step = rot_weight, damping, max_step
        self.check_step = check_step

    def struct(self):
        return _lib.ConstraintSettings(int(self.max_iterations), float(self.pos_tol), float(self.rot_tol), float(self.rot_weight),
                                       float(self.damping), float(self.max_step), float(self.check_step))

    def __repr__(self):
        return "ConstraintSettings(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items()) + ")"


def _constraint_records(constraints, n):
    """one EEConstraint (shared) or a sequence of n -> (ctypes array, count)"""
    items = [constraints] if isinstance(constraints, EEConstraint) else list(constraints)
    if not all(isinstance(c, EEConstraint) for c in items):
        raise TypeError("expected an EEConstraint or a sequence of them")
    if len(items) != 1 and len(items) != n:
        raise ValueError(f"expected 1 constraint or {n} (one per row), got {len(items)}")
    return (_lib.EeConstraint * len(items))(*[c.struct() for c in items]), len(items)


class _Robot(types.ModuleType):
    def __init__(self, name: str):
        super().__init__(f"{__name__}.{name}")
        self._id = lib.vmv_robot_id(name.encode())
        if self._id < 0:
            raise ImportError(f"robot {name} missing from the library")
        self._name = name
        self._dim = lib.vmv_robot_dimension(self._id)
        self._ns = lib.vmv_robot_n_spheres(self._id)
        lo, sp, ds = (np.zeros(self._dim, np.float32) for _ in range(3))
        check(lib.vmv_robot_bounds(self._id, _fp(lo), _fp(sp), _fp(ds)), "vmv_robot_bounds")
        self._lower, self._span, self._descale = lo, sp, ds

    # constants ---------------------------------------------------------------------------------------------
    def dimension(self):
        return self._dim

    def resolution(self):
        return lib.vmv_robot_resolution(self._id)

    def n_spheres(self):
        return self._ns

    def min_max_radii(self):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        check(lib.vmv_robot_min_max_radii(self._id, ctypes.byref(a), ctypes.byref(b)), "vmv_robot_min_max_radii")
        return (a.value, b.value)

    def joint_names(self):
        return [lib.vmv_robot_joint_name(self._id, j).decode() for j in range(self._dim)]

    def end_effector(self):
        return lib.vmv_robot_end_effector(self._id).decode()

    def lower_bounds(self):
        return self._lower.copy()

    def upper_bounds(self):
        return (self._lower + self._span).astype(np.float32)

    # single-configuration calls (drop-in names) --------------------------------------------------------------
    def validate(self, configuration, environment: Environment | None = None, check_bounds: bool = False) -> bool:
        """<robot>.validate(q, env=Environment(), check_bounds=False) — robot_helper.hh:255-267."""
        q = _f32(configuration, (self._dim,))
        if check_bounds:
            t = ((q - self._lower) * self._descale).astype(np.float32)  # descale_configuration, panda.hh:82-85
            if not (bool((t <= np.float32(1)).all()) and bool((t >= np.float32(0)).all())):
                return False
        return bool(self.validate_batch(q[None, :], environment)[0])

    def validate_motion(self, start, goal, environment: Environment | None = None) -> bool:
        """validate_motion<Robot, 8, resolution>(start, goal, env) — planning/validate.hh:70-77."""
        a, b = _f32(start, (self._dim,)), _f32(goal, (self._dim,))
        return bool(self.validate_motion_batch(a[None, :], b[None, :], environment)[0])

    def debug(self, configuration, environment: Environment | None = None):
        """<robot>.debug(q, env) — robot_helper.hh:249-253 (Robot::fkcc_debug): (per fine sphere the objects it collides
        with, the fine sphere pairs of the self-collision groups that overlap).  Objects are reported as
        (list, position) = position in the environment's sorted "spheres" / "capsules" / "z_capsules" / "cuboids" /
        "z_cuboids" tables (Environment.host_tables()) or ("heightfield", index) — the reference reports `name`s, which
        this environment does not keep."""
        q = _f32(configuration, (self._dim,))[None, :]
        h = self._env(environment)
        ns = self.n_spheres()
        words = np.zeros((1, ns, 9), np.uint32)
        npairs = ctypes.c_size_t(0)
        check(lib.vmv_robot_self_pairs(self._id, ctypes.byref(npairs), None), "vmv_robot_self_pairs")
        pairs = np.zeros((max(npairs.value, 1), 2), np.uint16)
        check(lib.vmv_robot_self_pairs(self._id, ctypes.byref(npairs), pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))),
              "vmv_robot_self_pairs")
        pw = np.zeros((1, max((npairs.value + 31) // 32, 1)), np.uint32)
        check(lib.vmv_contacts_batch_host(self._id, h, _fp(q), 1, words.ctypes.data_as(_lib.c_u32_p),
                                          pw.ctypes.data_as(_lib.c_u32_p)), "vmv_contacts_batch_host")
        base = np.zeros(5, np.uint32)
        check(lib.vmv_env_report_layout(h, base.ctypes.data_as(_lib.c_u32_p)), "vmv_env_report_layout")
        counts = (ctypes.c_size_t * 6)()
        check(lib.vmv_env_counts(h, counts), "vmv_env_counts")
        names = ("spheres", "capsules", "z_capsules", "cuboids", "z_cuboids")
        per_sphere = []
        for s in range(ns):
            hits = []
            for li, name in enumerate(names):
                for i in range(counts[li]):
                    if (int(words[0, s, int(base[li]) + i // 32]) >> (i % 32)) & 1:
                        hits.append((name, i))
            hits += [("heightfield", i) for i in range(4) if (int(words[0, s, 8]) >> i) & 1]
            per_sphere.append(hits)
        hit_pairs = [(int(pairs[p, 0]), int(pairs[p, 1])) for p in range(npairs.value)
                     if (int(pw[0, p // 32]) >> (p % 32)) & 1]
        return per_sphere, hit_pairs

    def eefk(self, configuration):
        """<robot>.eefk(q) -> 4 x 4 end-effector frame — robot_helper.hh:279-282."""
        return self.eefk_batch(_f32(configuration, (self._dim,))[None, :])[0]

    def eefk_batch(self, configurations):
        return self._batched("vmv_eefk_batch", [configurations], [((4, 4), "f32", True)])[0]

    def eefk_jacobian(self, configuration):
        """(4 x 4 frame, float32[6][dim]): eefk's frame and the end-effector Jacobian of one configuration, as
        eefk_jacobian_batch defines it."""
        frames, jac = self.eefk_jacobian_batch(_f32(configuration, (self._dim,))[None, :])
        return frames[0], jac[0]

    def eefk_jacobian_batch(self, configurations):
        """(float32[n][4][4], float32[n][6][dim]): eefk_batch's frames, bit for bit, and the geometric Jacobian in the
        world frame - rows 0-2 d translation / d q_j, rows 3-5 the angular velocity per unit of q_j (include/vamp_mvt_amd.h:
        vmv_eefk_jacobian_batch).  A joint that does not move the end effector has a zero column; a configuration with a
        non-finite joint has a NaN Jacobian.  numpy in -> numpy out; a torch CUDA tensor in -> torch CUDA tensors out."""
        return tuple(self._batched("vmv_eefk_jacobian_batch", [configurations], [((4, 4), "f32", True), ((6, self._dim), "f32", True)]))

    def ik_batch(self, targets, seeds=None, halton_skip=0, settings=None):
        """Inverse kinematics for many end-effector targets at once (include/vamp_mvt_amd.h: vmv_ik_batch): targets
        [n][4][4] (or [n][16]) frames as eefk_batch returns them; per target settings.n_seeds damped least-squares
        iterations, from seeds [n][n_seeds][dim] or, with seeds=None, from Halton samples halton_skip + 1 .. + n_seeds.
        -> (q float32[n][n_seeds][dim], err float32[n][n_seeds][2] = position (m) and rotation (sin of the angle)
        residuals, converged bool[n][n_seeds], iterations int32[n][n_seeds]).  q is the best state the iteration accepted:
        never worse than its seed, always inside the joint bounds.  A row whose target or seed has a non-finite entry
        comes back as its seed with NaN errors, not converged.  numpy in -> numpy out; torch CUDA tensors in -> torch CUDA
        tensors out, launched on torch's current stream."""
        s = settings or IKSettings()
        cs = s.struct()
        n_seeds = int(s.n_seeds)
        torch_in = _is_torch_cuda(targets)
        if seeds is not None and _is_torch_cuda(seeds) != torch_in:
            raise TypeError("targets and seeds must both be numpy arrays or both be torch CUDA tensors")
        if torch_in:
            import torch

            device = targets.device
            targets = targets.to(device).contiguous().float()
            if seeds is not None:
                seeds = seeds.to(device).contiguous().float()
        else:
            targets = _f32(targets)
            if seeds is not None:
                seeds = _f32(seeds)
        if targets.ndim < 2 or int(np.prod(tuple(targets.shape[1:]))) != 16:
            raise TypeError("expected targets as [n][4][4] (or [n][16]) frames")
        n = int(targets.shape[0])
        if seeds is not None and tuple(seeds.shape) != (n, n_seeds, self._dim):
            raise TypeError(f"expected seeds as [{n}][{n_seeds}][{self._dim}] (n_targets, settings.n_seeds, dimension)")
        shape = (n, n_seeds)
        if torch_in:
            with torch.cuda.device(device):
                q = torch.empty((*shape, self._dim), dtype=torch.float32, device=device)
                err = torch.empty((*shape, 2), dtype=torch.float32, device=device)
                status = torch.zeros(shape, dtype=torch.int32, device=device)
                ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
                check(lib.vmv_ik_batch(self._id, ptr(targets), n, None if seeds is None else ptr(seeds), int(halton_skip),
                                       ctypes.byref(cs), ptr(q), ptr(err), ptr(status),
                                       ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "vmv_ik_batch")
            return q, err, status < 0, status & 0x3fffffff
        q = np.zeros((*shape, self._dim), np.float32)
        err = np.zeros((*shape, 2), np.float32)
        status = np.zeros(shape, np.uint32)
        check(lib.vmv_ik_batch_host(self._id, _fp(targets), n, None if seeds is None else _fp(seeds), int(halton_skip),
                                    ctypes.byref(cs), _fp(q), _fp(err), status.ctypes.data_as(_lib.c_u32_p)), "vmv_ik_batch_host")
        return q, err, (status >> 31).astype(bool), (status & 0x3fffffff).astype(np.int32)

    def _constraint_call(self, symbol, inputs, constraints, settings, outputs):
        """The one path of the constraint calls.  inputs: one or two [n][dim] arrays (numpy -> `symbol`_host; torch CUDA ->
        `symbol` on torch's current stream); constraints: one EEConstraint or n; outputs: (trailing shape, numpy dtype,
        torch dtype name) each, "bits" as trailing shape for ceil(n / 64) validity words.  -> the output arrays."""
        cs = (settings or ConstraintSettings()).struct()
        torch_in = _is_torch_cuda(inputs[0])
        if not all(_is_torch_cuda(x) == torch_in for x in inputs):
            raise TypeError("the arrays must all be numpy arrays or all be torch CUDA tensors")
        if not torch_in:
            inputs = [_f32(x) for x in inputs]
        shape = tuple(inputs[0].shape)
        if len(shape) != 2 or shape[1] != self._dim or any(tuple(x.shape) != shape for x in inputs):
            raise TypeError(f"expected [n][{self._dim}] configurations" if len(inputs) == 1 else f"expected two [n][{self._dim}] arrays")
        n = shape[0]
        records, count = _constraint_records(constraints, n)
        shapes = [((n + 63) // 64,) if trailing == "bits" else (n, *trailing) for trailing, _, _ in outputs]
        if torch_in:
            import torch

            device = inputs[0].device
            with torch.cuda.device(device):
                inputs = [x.to(device).contiguous().float() for x in inputs]
                outs = [torch.zeros(s, dtype=getattr(torch, t), device=device) for s, (_, _, t) in zip(shapes, outputs)]
                ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
                check(getattr(lib, symbol)(self._id, *[ptr(x) for x in inputs], n, records, count, ctypes.byref(cs),
                                           *[ptr(o) for o in outs], ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                      symbol)
            return outs
        outs = [np.zeros(s, d) for s, (_, d, _) in zip(shapes, outputs)]
        fn = getattr(lib, symbol + "_host")
        types = fn.argtypes[len(fn.argtypes) - len(outs):]
        check(fn(self._id, *[_fp(x) for x in inputs], n, records, count, ctypes.byref(cs),
                 *[o.ctypes.data_as(t) for o, t in zip(outs, types)]), symbol + "_host")
        return outs

    def project_batch(self, configurations, constraint, settings=None):
        """Projects configurations [n][dim] into the band of an end-effector constraint (include/vamp_mvt_amd.h:
        vmv_constraint_project_batch): ik_batch's damped least-squares iteration on the constraint's residual.  constraint:
        one EEConstraint for all rows, or n of them.  -> (q float32[n][dim], residuals float32[n][2] = metres outside the
        box and radians beyond the cone, converged bool[n], evaluations int32[n]).  A row inside the joint bounds and in
        the band comes back bit for bit with 0 evaluations; a row with a non-finite joint comes back as given with NaN
        residuals.  numpy in -> numpy out; a torch CUDA tensor in -> torch CUDA tensors out."""
        q, res, status = self._constraint_call("vmv_constraint_project_batch", [configurations], constraint, settings,
                                               [((self._dim,), np.float32, "float32"), ((2,), np.float32, "float32"), ((), np.uint32, "int32")])
        if _is_torch_cuda(status):
            return q, res, status < 0, status & 0x3fffffff
        return q, res, (status >> 31).astype(bool), (status & 0x3fffffff).astype(np.int32)

    def constraint_check_batch(self, configurations, constraint, settings=None, residuals=False):
        """bool[n]: configuration i is in the band of its constraint (the nominal band widened by settings.pos_tol and
        rot_tol; a non-finite row is not).  residuals=True: also float32[n][2] as project_batch's."""
        bits, res = self._constraint_call("vmv_constraint_check_batch", [configurations], constraint, settings,
                                          [("bits", np.uint64, "int64"), ((2,), np.float32, "float32")])
        n = int(res.shape[0])
        ok = _torch_unpack_bits(bits, n) if _is_torch_cuda(bits) else unpack_bits(bits, n)
        return (ok, res) if residuals else ok

    def constraint_check_motion_batch(self, starts, goals, constraint, settings=None):
        """bool[n]: every band sample of the edge starts[e] -> goals[e] is in the band - max(1, ceil(|b - a| /
        settings.check_step)) samples a + (b - a) * (i / n_c); an edge of more than 1,024 samples is not."""
        (ok,) = self._constraint_call("vmv_constraint_check_motion_batch", [starts, goals], constraint, settings,
                                      [((), np.uint8, "uint8")])
        return ok != 0

    def fk(self, configuration):
        """<robot>.fk(q) -> list[Sphere] — robot_helper.hh:234-247."""
        out = self.fk_batch(_f32(configuration, (self._dim,))[None, :])[0]
        return [Sphere(s[:3], s[3]) for s in out]

    def filter_self_from_pointcloud(self, pc, point_radius, configuration, environment: Environment | None = None):
        """<robot>.filter_self_from_pointcloud — robot_helper.hh:284-322: the points [m][3] of `pc` whose sphere of radius
        `point_radius` touches neither the robot at `configuration` nor the environment (order preserved)."""
        pts = _f32(pc).reshape(-1, 3)
        q = _f32(configuration, (self._dim,))
        out = np.zeros((max(len(pts), 1), 3), np.float32)
        m = ctypes.c_size_t(0)
        check(lib.vmv_filter_self_from_pointcloud(self._id, self._env(environment), _fp(q), _fp(pts), len(pts),
                                                  float(point_radius), _fp(out), len(pts), ctypes.byref(m)),
              "vmv_filter_self_from_pointcloud")
        return out[:m.value].copy()

    # batched calls --------------------------------------------------------------------------------------------
    def _env(self, environment):
        # the default argument of the reference (`env = Environment()`): one cached empty environment, kept alive
        # here because the C handle must outlive the call
        if environment is None:
            environment = _EMPTY_ENVIRONMENT
        return environment.handle()

    def _batched(self, symbol, inputs, outputs, environment=_NO_ENVIRONMENT, nullable=False, environments=None, counts=None):
        """The one path of the batched calls.  inputs: one or two [n][dim] arrays; outputs: (trailing shape, dtype,
        wanted) each, dtype one of _OUTPUT_DTYPES; environment: None = the empty environment, or with `nullable` a NULL
        handle; environments / counts: the multi-environment form.  Every Python-side check runs before any library
        call (Environment.handle() is one).  numpy in: `symbol`_host, numpy out; torch CUDA tensors in: `symbol` on the
        tensor's device and torch's current stream, torch out.  -> the outputs (None where not wanted), validity words
        unpacked to bool[n]."""
        multi = environments is not None
        if multi:
            environments, offsets = _segments(environments, counts)
        elif nullable and environment is not None and not isinstance(environment, Environment):
            raise TypeError(f"expected Environment or None, got {type(environment).__name__}")
        torch_in = _is_torch_cuda(inputs[0])
        if torch_in and not all(_is_torch_cuda(x) for x in inputs):
            raise TypeError("starts is a torch CUDA tensor, goals is not")
        if not torch_in:
            inputs = [_f32(x) for x in inputs]
        shape = tuple(inputs[0].shape)
        if len(shape) != 2 or shape[1] != self._dim or tuple(inputs[-1].shape) != shape:
            raise TypeError(f"expected [n][{self._dim}] configurations" if len(inputs) == 1 else
                            f"expected two [n][{self._dim}] arrays")
        n = shape[0]
        if multi and int(offsets[-1]) != n:
            raise ValueError(f"counts sum to {int(offsets[-1])}, but there are {n} " +
                             ("configurations" if len(inputs) == 1 else "edges"))
        if torch_in:
            import torch

            device = inputs[0].device
        with torch.cuda.device(device) if torch_in else _NO_CONTEXT:
            if multi:
                envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
                head = [handles, offsets.ctypes.data_as(_lib.c_size_p), len(envs)]
            elif environment is _NO_ENVIRONMENT:
                head = []
            else:
                head = [None if nullable and environment is None else self._env(environment)]
            name = symbol if torch_in else symbol + "_host"
            fn = getattr(lib, name)
            types = fn.argtypes
            args = [self._id, *head]
            if torch_in:
                inputs = [x.to(device).contiguous().float() for x in inputs]  # (held until the call has returned)
            for a in inputs:
                args.append(ctypes.c_void_p(a.data_ptr()) if torch_in else _AT[types[len(args)]](a.ctypes.data))
            if not multi:
                args.append(n)
            outs = []
            for trailing, dtype, wanted in outputs:
                shape = ((n + 63) // 64,) if dtype == "bits" else (n, *trailing)
                if not wanted:
                    out = None
                elif torch_in:  # (validity words start at zero, as they always have; nothing else needs a fill)
                    out = (torch.zeros if dtype == "bits" else torch.empty)(shape, dtype=getattr(torch, _OUTPUT_DTYPES[dtype][0]),
                                                                            device=device)
                else:
                    out = np.zeros(shape, _OUTPUT_DTYPES[dtype][1])
                args.append(None if out is None else ctypes.c_void_p(out.data_ptr()) if torch_in else
                            _AT[types[len(args)]](out.ctypes.data))
                outs.append(out)
            if torch_in:
                args.append(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
            check(fn(*args), name)
        for i, (_, dtype, _) in enumerate(outputs):
            if dtype == "bits":
                outs[i] = (_torch_unpack_bits if torch_in else unpack_bits)(outs[i], n)
        return outs

    def validate_batch(self, configurations, environment: Environment | None = None):
        """bool[n] (numpy in -> numpy out; torch CUDA tensor in -> torch.bool CUDA tensor out)."""
        return self._batched("vmv_validate_batch", [configurations], [((), "bits", True)], environment)[0]

    def clearance(self, configuration, environment: Environment | None = None):
        """(env, self): the signed distance from contact of one configuration, as clearance_batch defines it."""
        out = self.clearance_batch(_f32(configuration, (self._dim,))[None, :], environment)
        return float(out[0, 0]), float(out[0, 1])

    def clearance_batch(self, configurations, environment: Environment | None = None, witness: bool = False):
        """float32[n][2] = (env, self) per configuration: the smallest signed distance (metres, negative = penetration)
        between a fine sphere of the robot and a contact of the environment - spheres, capsules, cuboids, heightfields
        (their vertical value) - and between the two spheres of a fine self pair (include/vamp_mvt_amd.h:
        vmv_clearance_batch).  environment=None: env = +inf.  witness=True: also uint32[n][4] = (env_sphere, env_kind,
        env_index, self_pair), UINT32_MAX where there is nothing to point at; env_kind 0 sphere, 1 capsule, 2 z-capsule,
        3 cuboid, 4 z-cuboid, 5 heightfield, env_index the position in Environment.host_tables()'s sorted list of that
        kind.  Environments with a point cloud or an attachment are refused.  numpy in -> numpy out; a torch CUDA tensor
        in -> torch CUDA tensors out (the witness as int32: UINT32_MAX reads -1), launched on torch's current stream."""
        out, wit = self._batched("vmv_clearance_batch", [configurations], [((2,), "f32", True), ((4,), "u32", witness)],
                                 environment, nullable=True)
        return (out, wit) if witness else out

    def clearance_batch_multi(self, configurations, environments, counts, witness: bool = False):
        """clearance_batch for configurations [sum(counts[:k]), sum(counts[:k + 1])) against environments[k] (None = the
        empty environment: env = +inf), in one call and one launch.  Bit for bit one clearance_batch per environment,
        concatenated.  numpy in -> numpy out; a torch CUDA tensor in -> torch CUDA tensors out, as clearance_batch."""
        out, wit = self._batched("vmv_clearance_batch_multi", [configurations], [((2,), "f32", True), ((4,), "u32", witness)],
                                 environments=environments, counts=counts)
        return (out, wit) if witness else out

    def clearance_grad(self, configuration, environment: Environment | None = None):
        """((env, self), float32[2][dim]): one configuration's clearances and their joint-space gradients, as
        clearance_grad_batch defines them."""
        values, grad = self.clearance_grad_batch(_f32(configuration, (self._dim,))[None, :], environment)
        return (float(values[0, 0]), float(values[0, 1])), grad[0]

    def clearance_grad_batch(self, configurations, environment: Environment | None = None, witness: bool = False):
        """(float32[n][2], float32[n][2][dim]): clearance_batch's values, bit for bit, and grad[i][0] = d env / d q,
        grad[i][1] = d self / d q with the witness held fixed: the contact normal times the witness spheres' Jacobians
        (include/vamp_mvt_amd.h: vmv_clearance_grad_batch).  Zeros where there is no witness (environment=None, an empty
        environment; a robot without self pairs), and for a sphere centre inside a cuboid, where the value is flat; NaN
        for a configuration with a non-finite joint.  witness=True appends clearance_batch's witness.  Shapes, types,
        refused environments and the numpy / torch convention are clearance_batch's."""
        out = self._batched("vmv_clearance_grad_batch", [configurations],
                            [((2,), "f32", True), ((2, self._dim), "f32", True), ((4,), "u32", witness)], environment, nullable=True)
        return tuple(out) if witness else tuple(out[:2])

    def clearance_grad_batch_multi(self, configurations, environments, counts, witness: bool = False):
        """clearance_grad_batch for configurations [sum(counts[:k]), sum(counts[:k + 1])) against environments[k] (None =
        the empty environment), in one call: one clearance launch and one gradient launch.  Bit for bit one
        clearance_grad_batch per environment, concatenated."""
        out = self._batched("vmv_clearance_grad_batch_multi", [configurations],
                            [((2,), "f32", True), ((2, self._dim), "f32", True), ((4,), "u32", witness)],
                            environments=environments, counts=counts)
        return tuple(out) if witness else tuple(out[:2])

    def prepare(self, environments):
        """Builds what each environment holds for this robot (broad-phase grids, reach certificates, static links) for
        all of them in one call, on the device, instead of one by one on their first use.  None = the empty
        environment.  Changes no answer: the parts are the ones the first use would build, bit for bit."""
        environments = list(environments)
        _check_environments(environments)
        envs, handles = _env_handles(environments)
        check(lib.vmv_env_prepare_multi(self._id, handles, len(envs)), "vmv_env_prepare_multi")

    def rrtc_multi_raw(self, starts, goals, environments, settings, skips=None):
        """vmv_rrtc_multi: lockstep RRT-Connect, problem p from starts[p] to goals[p] in environments[p] (None = the
        empty environment) with the Halton samples skips[p] + 1, ... (None = all 0).  settings: range, balance,
        tree_ratio, max_iterations, max_samples and optionally check_every.  -> dict of per-problem numpy arrays
        (status, iterations, sizes [n][2], path_lengths), the packed waypoints (paths [sum(path_lengths)][dim]) and
        the totals rounds and questions.  planning.rrtc_multi is the caller-facing form.  Every argument is checked
        before any library call."""
        environments = list(environments)
        _check_environments(environments)
        a, b, n = _endpoints(self._dim, starts, goals)
        _one_per(environments, n, "problem")
        sk = _skips(skips, n, "problem")
        cs = _rrtc_settings_struct(settings)
        envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
        plans = ctypes.c_void_p()
        check(lib.vmv_rrtc_multi(self._id, handles, n, _fp(a), _fp(b), _ptr(sk, _lib.c_u64_p), ctypes.byref(cs),
                                 ctypes.byref(plans)), "vmv_rrtc_multi")
        return _read_plans(plans, n, self._dim)

    def rrtc_multi_constrained_raw(self, starts, goals, goal_counts, environments, constraints, settings, constraint_settings=None,
                                   max_stretch=2.0, skips=None):
        """vmv_rrtc_multi_constrained: rrtc_multi_goals_raw under end-effector constraints - one EEConstraint for all
        problems or one per problem; constraint_settings: a ConstraintSettings (None = defaults); max_stretch: a projected
        node farther than max_stretch * range from the edge's near end is answered invalid.  -> rrtc_multi_goals_raw's dict
        plus band_refused per problem (the questions the constraint answered 0);
        status 4 (invalid_endpoint) where the start is out of band or no goal is in band."""
        return self.rrtc_multi_goals_raw(starts, goals, goal_counts, environments, settings, skips,
                                         constrained=(constraints, constraint_settings, float(max_stretch)))

    def rrtc_multi_goals_raw(self, starts, goals, goal_counts, environments, settings, skips=None, constrained=None):
        """vmv_rrtc_multi_goals: rrtc_multi_raw with goal sets, dynamic domain and start_tree_first.  goals: the goals of
        all problems packed, [sum(goal_counts)][dim]; goal_counts: goals per problem (each at least 1), None = one each.
        settings: those of rrtc_multi_raw and dynamic_domain, radius, alpha, min_radius, start_tree_first.
        -> rrtc_multi_raw's dict plus goal_indices per problem (-1 = unsolved).  planning.rrtc_multi_goals is the
        caller-facing form.  Every argument is checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        a, b = _f32(starts), _f32(goals)
        if a.ndim != 2 or a.shape[1] != self._dim or b.ndim != 2 or b.shape[1] != self._dim:
            raise TypeError(f"expected [n][{self._dim}] starts and packed [goals][{self._dim}] goals")
        n = a.shape[0]
        if goal_counts is None:
            offsets = None
            if b.shape[0] != n:
                raise TypeError(f"expected one goal per problem, got {b.shape[0]} for {n} problems")
        else:
            counts = np.asarray(goal_counts)
            if counts.shape != (n,) or (n and not np.issubdtype(counts.dtype, np.integer)):
                raise TypeError(f"expected one goal set per problem, got shape {counts.shape} for {n} problems")
            if n and (counts < 1).any():
                raise TypeError("every problem needs at least one goal")
            offsets = np.zeros(n + 1, np.uint64)
            np.cumsum(counts, out=offsets[1:])
            if int(offsets[n]) != b.shape[0]:
                raise TypeError(f"expected {int(offsets[n])} packed goals, got {b.shape[0]}")
        _one_per(environments, n, "problem")
        sk = _skips(skips, n, "problem")
        base = _rrtc_settings_struct(settings)
        if offsets is not None and n and int(np.diff(offsets).max()) + 1 > base.max_samples:
            raise ValueError("the start and the goals of a problem must fit max_samples")
        dynamic = bool(getattr(settings, "dynamic_domain", False))
        radius, alpha = float(getattr(settings, "radius", 4.0)), float(getattr(settings, "alpha", 0.0001))
        min_radius = float(getattr(settings, "min_radius", 1.0))
        if dynamic:
            if not (math.isfinite(radius) and radius > 0 and math.isfinite(min_radius) and min_radius > 0):
                raise ValueError("radius and min_radius must be finite and positive")
            if not (math.isfinite(alpha) and 0 <= alpha < 1):
                raise ValueError("alpha must be in [0, 1)")
        cs = _lib.RrtcGoalsSettings(base, int(dynamic), radius, alpha, min_radius,
                                    int(bool(getattr(settings, "start_tree_first", False))))
        if constrained is not None:  # (every Python-side check before any library call)
            records, count = _constraint_records(constrained[0], n)
            if not (math.isfinite(constrained[2]) and constrained[2] >= 0):
                raise ValueError("max_stretch must be finite and not negative")
            ps = _lib.ConstraintPlanSettings((constrained[1] or ConstraintSettings()).struct(), constrained[2])
        envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
        plans = ctypes.c_void_p()
        if constrained is not None:
            check(lib.vmv_rrtc_multi_constrained(self._id, handles, n, _fp(a), _fp(b), _ptr(offsets, _lib.c_size_p), _ptr(sk, _lib.c_u64_p),
                                                 ctypes.byref(cs), records, count, ctypes.byref(ps), ctypes.byref(plans)),
                  "vmv_rrtc_multi_constrained")
        else:
            check(lib.vmv_rrtc_multi_goals(self._id, handles, n, _fp(a), _fp(b), _ptr(offsets, _lib.c_size_p),
                                           _ptr(sk, _lib.c_u64_p), ctypes.byref(cs), ctypes.byref(plans)), "vmv_rrtc_multi_goals")

        def goal_indices(plans, out):
            indices = np.zeros(n, np.uint32)
            check(lib.vmv_plans_goal_indices(plans, indices.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_goal_indices")
            out["goal_indices"] = indices.view(np.int32).copy()
            if constrained is not None:
                refused = np.zeros(n, np.uint32)
                check(lib.vmv_plans_band_refused(plans, refused.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_band_refused")
                out["band_refused"] = refused

        return _read_plans(plans, n, self._dim, goal_indices)

    def aorrtc_multi_constrained_raw(self, starts, goals, environments, constraints, settings, constraint_settings=None,
                                     max_stretch=2.0, skips=None):
        """vmv_aorrtc_multi_constrained: aorrtc_multi_raw under end-effector constraints - one EEConstraint for all problems
        or one per problem; constraint_settings: a ConstraintSettings (None = defaults); max_stretch as in
        rrtc_multi_constrained_raw.  -> aorrtc_multi_raw's dict plus band_refused per problem (the questions of every stage
        the constraint answered 0); status 4 (invalid_endpoint) where the start or the goal is out of band."""
        return self.aorrtc_multi_raw(starts, goals, environments, settings, skips,
                                     constrained=(constraints, constraint_settings, float(max_stretch)))

    def aorrtc_multi_raw(self, starts, goals, environments, settings, skips=None, constrained=None):
        """vmv_aorrtc_multi: AORRTC for many problems (a first solution by rrtc_multi's contract, simplified by
        simplify_multi's, then cost-bounded RRT-Connect searches in lockstep), the arguments those of rrtc_multi_raw.
        settings: range, balance, tree_ratio, check_every, optimize, cost_bound_resample, simplify_intermediate,
        max_iterations, max_internal_iterations, max_samples, max_cost_bound_resamples, max_searches and `simplify` (as
        simplify_multi_raw takes it).  -> rrtc_multi_raw's dict plus first_costs, costs, searches, improvements per
        problem.  planning.aorrtc_multi is the caller-facing form.  Every argument is checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        a, b, n = _endpoints(self._dim, starts, goals)
        _one_per(environments, n, "problem")
        sk = _skips(skips, n, "problem")
        max_in, resamples = int(settings.max_internal_iterations), int(settings.max_cost_bound_resamples)
        base = _rrtc_settings_struct(settings, also=("max_searches",))
        if not 1 <= max_in < 2 ** 32:
            raise ValueError("max_internal_iterations must be positive and fit 32 bits")
        if not 0 <= resamples <= 64:
            raise ValueError("max_cost_bound_resamples must be from 0 to 64")
        cs = _lib.AorrtcSettings(base, _simplify_settings_struct(settings.simplify), int(bool(settings.optimize)),
                                 int(bool(settings.cost_bound_resample)), int(bool(settings.simplify_intermediate)),
                                 base.max_iterations, max_in, base.max_samples, resamples, int(settings.max_searches))
        if constrained is not None:  # (every Python-side check before any library call)
            records, count = _constraint_records(constrained[0], n)
            if not (math.isfinite(constrained[2]) and constrained[2] >= 0):
                raise ValueError("max_stretch must be finite and not negative")
            ps = _lib.ConstraintPlanSettings((constrained[1] or ConstraintSettings()).struct(), constrained[2])
        envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
        plans = ctypes.c_void_p()
        given = (self._id, handles, n, _fp(a), _fp(b), _ptr(sk, _lib.c_u64_p), ctypes.byref(cs))
        if constrained is not None:
            check(lib.vmv_aorrtc_multi_constrained(*given, records, count, ctypes.byref(ps), ctypes.byref(plans)),
                  "vmv_aorrtc_multi_constrained")
        else:
            check(lib.vmv_aorrtc_multi(*given, ctypes.byref(plans)), "vmv_aorrtc_multi")

        def search_costs(plans, out):
            first, costs = np.zeros(n, np.float32), np.zeros(n, np.float32)
            n_searches, improvements = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            check(lib.vmv_plans_costs(plans, _fp(first), _fp(costs), n_searches.ctypes.data_as(_lib.c_u32_p),
                                      improvements.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_costs")
            out.update(first_costs=first, costs=costs, searches=n_searches, improvements=improvements)
            if constrained is not None:
                refused = np.zeros(n, np.uint32)
                check(lib.vmv_plans_band_refused(plans, refused.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_band_refused")
                out["band_refused"] = refused

        return _read_plans(plans, n, self._dim, search_costs)

    def phs_samples(self, start, goal, max_cost, seed, counter, n):
        """vmv_phs_samples (test support): n successive samples of aorrtc_multi's device sampler for the foci start and
        goal under the bound max_cost, from the uniform stream (seed, counter) -> (q [n][dim], in_bounds bool[n], the
        counter after the last draw)"""
        a, b = _f32(start, (self._dim,)), _f32(goal, (self._dim,))
        q, ok, c = np.zeros((int(n), self._dim), np.float32), np.zeros(int(n), np.uint8), ctypes.c_uint32(0)
        check(lib.vmv_phs_samples(self._id, _fp(a), _fp(b), float(max_cost), int(seed) & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF,
                                  int(n), _fp(q), ok.ctypes.data_as(_lib.c_u8_p), ctypes.byref(c)),
              "vmv_phs_samples")
        return q, ok.astype(bool), int(c.value)

    def prm_multi_raw(self, starts, goals, environments, settings, skips=None, samples=None):
        """vmv_prm_multi: one roadmap per problem, problem p from starts[p] to goals[p] in environments[p] (None = the
        empty environment) over the Halton samples skips[p] + 1, ... (None = all 0) or over `samples`
        ([n][n_samples][dim], or [n_samples][dim] for every problem).  settings: n_samples, k, radius, keep_roadmaps.
        -> dict of per-problem numpy arrays (status, iterations, sizes [n][2] = valid vertices and valid edges,
        path_lengths, candidate_edges, costs), the packed waypoints (paths [sum(path_lengths)][dim]), the totals rounds
        and questions, and with keep_roadmaps `roadmaps`: per problem (vertex flags bool[n_samples + 2], candidate
        pairs uint32[m][2], their flags bool[m]).  planning.prm_multi is the caller-facing form.  Every argument is
        checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        a, b, n = _endpoints(self._dim, starts, goals)
        _one_per(environments, n, "problem")
        ns, k, radius = _roadmap_sampling(settings)
        keep = bool(getattr(settings, "keep_roadmaps", False))
        if n * (ns + 2) * k >= 2 ** 31:
            raise ValueError("n_problems * (n_samples + 2) * k must stay below 2^31")
        sm = _samples(samples, n, ns, self._dim)
        sk = _skips(skips, n, "problem", draws=ns if sm is None else None)
        cs = _lib.PrmSettings(ns, k, radius, int(keep))
        envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
        plans = ctypes.c_void_p()
        check(lib.vmv_prm_multi(self._id, handles, n, _fp(a), _fp(b), _ptr(sk, _lib.c_u64_p), _ptr(sm, _lib.c_float_p),
                                ctypes.byref(cs), ctypes.byref(plans)), "vmv_prm_multi")

        def roadmaps(plans, out):
            candidates, costs = np.zeros(n, np.uint32), np.zeros(n, np.float32)
            check(lib.vmv_plans_roadmap_summary(plans, None, candidates.ctypes.data_as(_lib.c_u32_p), None, _fp(costs)),
                  "vmv_plans_roadmap_summary")
            out.update(candidate_edges=candidates, costs=costs)
            if not keep:
                return
            out["roadmaps"] = []
            for p in range(n):
                vertex = np.zeros(ns + 2, np.uint8)
                check(lib.vmv_plans_roadmap_vertices(plans, p, vertex.ctypes.data_as(_lib.c_u8_p)), "vmv_plans_roadmap_vertices")
                m = int(candidates[p])
                pairs, flags = np.zeros((m, 2), np.uint32), np.zeros(m, np.uint8)
                got = ctypes.c_size_t(0)
                check(lib.vmv_plans_roadmap_edges(plans, p, pairs.ctypes.data_as(_lib.c_u32_p), flags.ctypes.data_as(_lib.c_u8_p),
                                                  m, ctypes.byref(got)), "vmv_plans_roadmap_edges")
                out["roadmaps"].append((vertex.astype(bool), pairs[:got.value], flags[:got.value].astype(bool)))

        return _read_plans(plans, n, self._dim, roadmaps)

    def roadmaps_build_raw(self, environments, settings, skips=None, samples=None):
        """vmv_roadmaps_build: one device-resident roadmap per environment (None = the empty environment) over the Halton
        samples skips[r] + 1, ... (None = all 0) or over `samples` ([n][n_samples][dim], or [n_samples][dim] for every
        roadmap).  settings: n_samples, k, radius.  -> (the handle, the Environment objects it refers to): the caller
        keeps both and ends with roadmaps_destroy_raw.  planning.build_roadmaps is the caller-facing form.  Every argument
        is checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        n = len(environments)
        ns, k, radius = _roadmap_sampling(settings)
        if n * ns * k >= 2 ** 31:
            raise ValueError("n_roadmaps * n_samples * k must stay below 2^31")
        sm = _samples(samples, n, ns, self._dim)
        sk = _skips(skips, n, "roadmap", draws=ns if sm is None else None)
        cs = _lib.RoadmapSettings(ns, k, radius)
        envs, handles = _env_handles(environments)
        handle = ctypes.c_void_p()
        check(lib.vmv_roadmaps_build(self._id, handles, n, _ptr(sk, _lib.c_u64_p), _ptr(sm, _lib.c_float_p), ctypes.byref(cs),
                                     ctypes.byref(handle)), "vmv_roadmaps_build")
        return handle, envs

    def roadmaps_query_raw(self, handle, n_roadmaps, starts, goals, index=None, settings=None):
        """vmv_roadmaps_query: query q from starts[q] to goals[q] against roadmap index[q] (None = all 0) of a handle of
        n_roadmaps roadmaps.  settings: k_connect, radius.  -> dict of per-query numpy arrays (status, iterations, sizes
        [n][2] = valid connection edges of the start and of the goal, path_lengths, costs, edges_checked), the packed
        waypoints (paths [sum(path_lengths)][dim]) and the totals rounds and questions.  DeviceRoadmaps.query is the
        caller-facing form.  Every argument is checked before any library call."""
        a, b, n = _endpoints(self._dim, starts, goals)
        kc = int(settings.k_connect)
        if not 1 <= kc <= 32:
            raise ValueError("k_connect must be from 1 to 32")
        radius = _cut_radius(settings)
        if n * (1 + 2 * kc) >= 2 ** 31:
            raise ValueError("n_queries * (1 + 2 * k_connect) must stay below 2^31")
        ix = None
        if index is not None:
            ix = np.asarray(index)
            if ix.shape != (n,):
                raise ValueError(f"expected one roadmap index per query, got shape {ix.shape} for {n} queries")
            if ix.size and (not np.issubdtype(ix.dtype, np.integer) or (ix < 0).any() or int(ix.max()) >= n_roadmaps):
                raise ValueError(f"roadmap indices must be integers from 0 to {n_roadmaps - 1}")
            ix = np.ascontiguousarray(ix, np.uint32)
        elif n and n_roadmaps < 1:
            raise ValueError("the handle holds no roadmap")
        cs = _lib.RoadmapQuerySettings(kc, radius)
        plans = ctypes.c_void_p()
        check(lib.vmv_roadmaps_query(handle, n, _ptr(ix, _lib.c_u32_p), _fp(a), _fp(b), ctypes.byref(cs), ctypes.byref(plans)),
              "vmv_roadmaps_query")

        def connections(plans, out):
            costs, asked = np.zeros(n, np.float32), np.zeros(n, np.uint32)
            check(lib.vmv_plans_query_summary(plans, _fp(costs), asked.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_query_summary")
            out.update(costs=costs, edges_checked=asked)

        return _read_plans(plans, n, self._dim, connections)

    def roadmaps_summary_raw(self, handle, n_roadmaps):
        """vmv_roadmaps_summary -> (valid samples, candidate edges, valid edges), uint32[n_roadmaps] each"""
        out = [np.zeros(n_roadmaps, np.uint32) for _ in range(3)]
        check(lib.vmv_roadmaps_summary(handle, *[x.ctypes.data_as(_lib.c_u32_p) for x in out]), "vmv_roadmaps_summary")
        return tuple(out)

    def roadmaps_roadmap_raw(self, handle, r, n_samples):
        """vmv_roadmaps_vertices and vmv_roadmaps_edges of roadmap r -> (samples [n_samples][dim], their flags bool[n_samples],
        candidate pairs uint32[m][2] of sample ids, their flags bool[m])"""
        samples, vertex = np.zeros((n_samples, self._dim), np.float32), np.zeros(n_samples, np.uint8)
        check(lib.vmv_roadmaps_vertices(handle, r, _fp(samples), vertex.ctypes.data_as(_lib.c_u8_p)), "vmv_roadmaps_vertices")
        m = ctypes.c_size_t(0)
        check(lib.vmv_roadmaps_edges(handle, r, None, None, 0, ctypes.byref(m)), "vmv_roadmaps_edges")
        pairs, flags = np.zeros((m.value, 2), np.uint32), np.zeros(m.value, np.uint8)
        check(lib.vmv_roadmaps_edges(handle, r, pairs.ctypes.data_as(_lib.c_u32_p), flags.ctypes.data_as(_lib.c_u8_p), m.value,
                                     None), "vmv_roadmaps_edges")
        return samples, vertex.astype(bool), pairs, flags.astype(bool)

    def roadmaps_destroy_raw(self, handle):
        """vmv_roadmaps_destroy"""
        check(lib.vmv_roadmaps_destroy(handle), "vmv_roadmaps_destroy")

    def fcit_multi_raw(self, starts, goals, environments, settings, skips=None, samples=None):
        """vmv_fcit_multi: a lazy A* search of the complete graph over each problem's valid samples, the arguments those
        of prm_multi_raw.  settings: n_samples, max_iterations, questions_per_round, check_every.  -> dict of
        per-problem numpy arrays (status, iterations = searches run, sizes [n][2] = valid vertices and blocked edges,
        path_lengths, costs, known_valid_edges), the packed waypoints (paths [sum(path_lengths)][dim]) and the totals
        rounds and questions.  planning.fcit_multi is the caller-facing form.  Every argument is checked before any
        library call."""
        environments = list(environments)
        _check_environments(environments)
        a, b, n = _endpoints(self._dim, starts, goals)
        _one_per(environments, n, "problem")
        ns, max_it = int(settings.n_samples), int(settings.max_iterations)
        per_round, every = int(settings.questions_per_round), int(getattr(settings, "check_every", 0))
        if ns % 64 != 0 or not 64 <= ns <= 2048:
            raise ValueError("n_samples must be a multiple of 64 from 64 to 2,048")
        if not 1 <= per_round <= 32:
            raise ValueError("questions_per_round must be from 1 to 32")
        if not (1 <= max_it < 2 ** 32 and 0 <= every < 2 ** 32):
            raise ValueError("max_iterations must be positive, and fit 32 bits as check_every must")
        if n * (ns + 2) * ((ns + 2 + 31) // 32) >= 2 ** 31 or n * per_round >= 2 ** 31:
            raise ValueError("n_problems * (n_samples + 2) * ceil((n_samples + 2) / 32) and n_problems * questions_per_round "
                             "must stay below 2^31")
        sm = _samples(samples, n, ns, self._dim)
        sk = _skips(skips, n, "problem", draws=ns if sm is None else None)
        cs = _lib.FcitSettings(ns, max_it, per_round, every)
        envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
        plans = ctypes.c_void_p()
        check(lib.vmv_fcit_multi(self._id, handles, n, _fp(a), _fp(b), _ptr(sk, _lib.c_u64_p), _ptr(sm, _lib.c_float_p),
                                 ctypes.byref(cs), ctypes.byref(plans)), "vmv_fcit_multi")

        def searches(plans, out):
            costs, known = np.zeros(n, np.float32), np.zeros(n, np.uint32)
            check(lib.vmv_plans_fcit_summary(plans, _fp(costs), known.ctypes.data_as(_lib.c_u32_p)), "vmv_plans_fcit_summary")
            out.update(costs=costs, known_valid_edges=known)

        return _read_plans(plans, n, self._dim, searches)

    def simplify_multi_constrained_raw(self, paths, environments, constraints, settings, constraint_settings=None):
        """vmv_simplify_multi_constrained: simplify_multi_raw inside the band of end-effector constraints - one
        EEConstraint for all paths or one per path; constraint_settings: a ConstraintSettings (None = defaults).
        -> simplify_multi_raw's dict plus band_refused per path (the questions of the serial loop the constraint answered
        0); status 2 (out_of_band) where the input's first waypoint or one of its edges is out of band."""
        return self.simplify_multi_raw(paths, environments, settings, constrained=(constraints, constraint_settings))

    def simplify_multi_raw(self, paths, environments, settings, constrained=None):
        """vmv_simplify_multi: the reference's simplify() with the SHORTCUT and BSPLINE routines for many paths in
        lockstep, path p ([len][dim] waypoints, any length) in environments[p] (None = the empty environment).
        settings: max_iterations, operations (a list of "SHORTCUT" / "BSPLINE"), max_steps, min_change,
        midpoint_interpolation and optionally interpolate (must be 0), max_waypoints, questions_per_round, check_every
        (0 = the library's default).  -> dict of per-path numpy arrays (status, iterations, lengths, questions), the
        packed waypoints (points [sum(lengths)][dim]) and the totals rounds and total_questions.
        planning.simplify_multi is the caller-facing form.  Every argument is checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        pts, packed, offsets = _packed_paths(paths, self._dim)
        n = len(pts)
        _one_per(environments, n, "path")
        cs = _simplify_settings_struct(settings, max((len(a) for a in pts), default=0))
        status, iterations = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        lengths, questions = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        rounds, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
        extra = {}
        if constrained is not None:  # (every Python-side check before any library call)
            records, count = _constraint_records(constrained[0], n)
            ps = (constrained[1] or ConstraintSettings()).struct()
            extra["band_refused"] = np.zeros(n, np.uint32)

        def entry(out):
            envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
            given = (self._id, handles, n, _fp(packed), offsets.ctypes.data_as(_lib.c_size_p), ctypes.byref(cs))
            if constrained is not None:
                check(lib.vmv_simplify_multi_constrained(*given, records, count, ctypes.byref(ps), out), "vmv_simplify_multi_constrained")
            else:
                check(lib.vmv_simplify_multi(*given, out), "vmv_simplify_multi")

        def readout(out):
            check(lib.vmv_paths_summary(out, status.ctypes.data_as(_lib.c_u8_p), iterations.ctypes.data_as(_lib.c_u32_p),
                                        lengths.ctypes.data_as(_lib.c_u32_p), questions.ctypes.data_as(_lib.c_u32_p),
                                        ctypes.byref(rounds), ctypes.byref(total)), "vmv_paths_summary")
            points = np.zeros((int(lengths.sum()), self._dim), np.float32)
            check(lib.vmv_paths_points(out, _fp(points), points.size), "vmv_paths_points")
            if constrained is not None:
                check(lib.vmv_paths_band_refused(out, extra["band_refused"].ctypes.data_as(_lib.c_u32_p)), "vmv_paths_band_refused")
            return points

        points = _read_result(n, entry, readout, "vmv_paths_destroy")
        return dict(status=status, iterations=iterations, lengths=lengths, questions=questions,
                    points=packed if points is None else points, rounds=int(rounds.value), total_questions=int(total.value), **extra)

    def optimize_multi_constrained_raw(self, paths, environments, constraints, settings, constraint_settings=None):
        """vmv_optimize_multi_constrained: optimize_multi_raw inside the band of end-effector constraints - one
        EEConstraint for all paths or one per path; constraint_settings: a ConstraintSettings (None = defaults).
        -> optimize_multi_raw's dict plus held per path (the projections of its iterations that did not converge);
        status 3 (out_of_band) where an end of the input is out of band or an inner waypoint cannot be projected."""
        return self.optimize_multi_raw(paths, environments, settings, constrained=(constraints, constraint_settings))

    def optimize_multi_raw(self, paths, environments, settings, constrained=None):
        """vmv_optimize_multi: the clearance-aware covariant gradient iteration for many paths in lockstep, path p
        ([len][dim] waypoints, any length) in environments[p] (None = the empty environment).  settings: max_iterations,
        validate_every, step, max_step, min_change, smooth_weight, env_weight, self_weight, env_margin, self_margin,
        max_waypoints.  -> dict of per-path numpy arrays (status, iterations, best_iteration, cost_first, cost,
        clearance_first [n][2], clearance [n][2]), the packed waypoints (points, the input's layout) and the totals
        clearance_calls and validation_calls.  planning.optimize_multi is the caller-facing form.  Every argument is
        checked before any library call."""
        environments = list(environments)
        _check_environments(environments)
        pts, packed, offsets = _packed_paths(paths, self._dim)
        n = len(pts)
        _one_per(environments, n, "path")
        cs = _optimize_settings_struct(settings, max((len(a) for a in pts), default=0))
        status, iterations, best = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        cost_first, cost = np.zeros(n, np.float32), np.zeros(n, np.float32)
        clr_first, clr = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        points = np.zeros_like(packed)
        calls, validations = ctypes.c_uint64(0), ctypes.c_uint64(0)
        extra = {}
        if constrained is not None:  # (every Python-side check before any library call)
            records, count = _constraint_records(constrained[0], n)
            ps = (constrained[1] or ConstraintSettings()).struct()
            extra["held"] = np.zeros(n, np.uint32)

        def entry(out):
            envs, handles = _env_handles(environments)  # `envs` stays referenced until the call returns
            given = (self._id, handles, n, _fp(packed), offsets.ctypes.data_as(_lib.c_size_p), ctypes.byref(cs))
            if constrained is not None:
                check(lib.vmv_optimize_multi_constrained(*given, records, count, ctypes.byref(ps), out), "vmv_optimize_multi_constrained")
            else:
                check(lib.vmv_optimize_multi(*given, out), "vmv_optimize_multi")

        def readout(out):
            if constrained is not None:
                check(lib.vmv_optimized_held(out, extra["held"].ctypes.data_as(_lib.c_u32_p)), "vmv_optimized_held")
            check(lib.vmv_optimized_summary(out, status.ctypes.data_as(_lib.c_u8_p),
                                            iterations.ctypes.data_as(_lib.c_u32_p), best.ctypes.data_as(_lib.c_u32_p),
                                            _fp(cost_first), _fp(cost), _fp(clr_first), _fp(clr), ctypes.byref(calls),
                                            ctypes.byref(validations)), "vmv_optimized_summary")
            check(lib.vmv_optimized_points(out, _fp(points), points.size), "vmv_optimized_points")

        _read_result(n, entry, readout, "vmv_optimized_destroy")
        return dict(status=status, iterations=iterations, best_iteration=best, cost_first=cost_first, cost=cost,
                    clearance_first=clr_first, clearance=clr, points=points, offsets=offsets.astype(np.int64),
                    clearance_calls=int(calls.value), validation_calls=int(validations.value), **extra)

    def cartesian_multi_raw(self, starts, targets, environments, settings):
        """vmv_cartesian_multi: straight-line end-effector motions for many problems in one call, problem p from
        starts[p] ([dim]) to the frame targets[p] ([4][4] or [16]) in environments[p] (None = the empty environment);
        environments=None is the kinematics-only call.  settings: the fields of planning.CartesianSettings.  -> dict of
        per-problem numpy arrays (status, segments, achieved, evaluations), the packed waypoints (points) with their
        offsets, and the totals validation_calls and questions.  planning.cartesian_multi is the caller-facing form.
        Every argument is checked before any library call."""
        a = _f32(starts)
        if a.ndim != 2 or a.shape[1] != self._dim:
            raise TypeError(f"expected starts as [n][{self._dim}] configurations")
        n = a.shape[0]
        t = _f32(targets)
        if t.ndim < 2 or t.shape[0] != n or int(np.prod(t.shape[1:])) != 16:
            raise TypeError(f"expected targets as [{n}][4][4] (or [{n}][16]) frames")
        if environments is not None:
            environments = list(environments)
            _check_environments(environments)
            _one_per(environments, n, "problem")
        cs = _cartesian_settings_struct(settings)
        status, segments = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        achieved, evaluations = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        calls, questions = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def entry(out):
            envs, handles = (None, None) if environments is None else _env_handles(environments)  # (`envs` lives through the call)
            check(lib.vmv_cartesian_multi(self._id, handles, n, _fp(a), _fp(t), ctypes.byref(cs), out), "vmv_cartesian_multi")

        def readout(out):
            counts = [x.ctypes.data_as(_lib.c_u32_p) for x in (segments, achieved, evaluations)]
            check(lib.vmv_cartesian_summary(out, status.ctypes.data_as(_lib.c_u8_p), *counts, ctypes.byref(calls),
                                            ctypes.byref(questions)), "vmv_cartesian_summary")
            points = np.zeros((int(achieved.sum()) + n, self._dim), np.float32)
            check(lib.vmv_cartesian_points(out, _fp(points), points.size), "vmv_cartesian_points")
            return points

        points = _read_result(n, entry, readout, "vmv_cartesian_destroy")
        if points is None:
            points = np.zeros((0, self._dim), np.float32)
        offsets = np.zeros(n + 1, np.int64)
        offsets[1:] = np.cumsum(achieved.astype(np.int64) + 1)
        return dict(status=status, segments=segments, achieved=achieved, evaluations=evaluations, points=points,
                    offsets=offsets, validation_calls=int(calls.value), questions=int(questions.value))

    def retime_multi_raw(self, paths, vel_limits, acc_limits, environments, settings, constrained=None):
        """vmv_retime_multi: time-optimal trajectories along many paths in one call, path p ([len][dim] waypoints, any
        length) in environments[p] (None = the empty environment); environments=None: nothing is validated.  vel_limits,
        acc_limits: [dim], finite and positive.  settings: the fields of planning.RetimeSettings.  -> dict of per-path
        numpy arrays (status, intervals, samples, duration, first_invalid; UINT32_MAX = none), the packed samples (times,
        positions, velocities, accelerations) with their offsets, and the totals validation_calls and questions.
        planning.retime_multi is the caller-facing form.  Every argument is checked before any library call."""
        if environments is not None:
            environments = list(environments)
            _check_environments(environments)
        pts, packed, offsets = _packed_paths(paths, self._dim)
        n = len(pts)
        if environments is not None:
            _one_per(environments, n, "path")
        vel, acc = _joint_limits(vel_limits, self._dim, "vel_limits"), _joint_limits(acc_limits, self._dim, "acc_limits")
        status, intervals, samples = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        duration, first_invalid = np.zeros(n, np.float32), np.full(n, 0xffffffff, np.uint32)
        calls, questions = ctypes.c_uint64(0), ctypes.c_uint64(0)
        extra = {}
        if constrained is None:
            cs = _retime_settings_struct(settings)
        else:  # (every Python-side check before any library call)
            cs = _retime_constrained_settings_struct(settings)
            records, count, ps = None, 0, None
            if constrained[0] is not None:
                records, count = _constraint_records(constrained[0], n)
                ps = ctypes.byref((constrained[1] or ConstraintSettings()).struct())
            extra = dict(rounds=np.zeros(n, np.uint32), repaired=np.zeros(n, np.uint32), stops=np.zeros(n, np.uint32),
                         levels=np.zeros(int(offsets[-1]) if n else 0, np.uint8), level_offsets=offsets.astype(np.int64))

        def entry(out):
            envs, handles = (None, None) if environments is None else _env_handles(environments)  # (`envs` lives through the call)
            given = (self._id, handles, n, _fp(packed), offsets.ctypes.data_as(_lib.c_size_p), _fp(vel), _fp(acc))
            if constrained is not None:
                check(lib.vmv_retime_multi_constrained(*given, records, count, ctypes.byref(cs), ps, out), "vmv_retime_multi_constrained")
            else:
                check(lib.vmv_retime_multi(*given, ctypes.byref(cs), out), "vmv_retime_multi")

        def readout(out):
            counts = [x.ctypes.data_as(_lib.c_u32_p) for x in (intervals, samples)]
            check(lib.vmv_retime_summary(out, status.ctypes.data_as(_lib.c_u8_p), *counts, _fp(duration),
                                         first_invalid.ctypes.data_as(_lib.c_u32_p), ctypes.byref(calls),
                                         ctypes.byref(questions)), "vmv_retime_summary")
            if constrained is not None:
                check(lib.vmv_retime_levels(out, extra["levels"].ctypes.data_as(_lib.c_u8_p),
                                            *[extra[k].ctypes.data_as(_lib.c_u32_p) for k in ("rounds", "repaired", "stops")]),
                      "vmv_retime_levels")
            total = int(samples.sum())
            arrays = [np.zeros(total, np.float32)] + [np.zeros((total, self._dim), np.float32) for _ in range(3)]
            check(lib.vmv_retime_samples(out, *[_fp(x) for x in arrays], total), "vmv_retime_samples")
            return arrays

        arrays = _read_result(n, entry, readout, "vmv_retime_destroy")
        if arrays is None:
            arrays = [np.zeros(0, np.float32)] + [np.zeros((0, self._dim), np.float32) for _ in range(3)]
        sample_offsets = np.zeros(n + 1, np.int64)
        sample_offsets[1:] = np.cumsum(samples.astype(np.int64))
        return dict(status=status, intervals=intervals, samples=samples, duration=duration, first_invalid=first_invalid,
                    times=arrays[0], positions=arrays[1], velocities=arrays[2], accelerations=arrays[3],
                    offsets=sample_offsets, validation_calls=int(calls.value), questions=int(questions.value), **extra)

    def retime_multi_constrained_raw(self, paths, vel_limits, acc_limits, environments, constraints, settings,
                                     constraint_settings=None):
        """vmv_retime_multi_constrained: retime_multi_raw whose corners carry levels, raised round by round until every
        returned sample pair is valid in environments[p] and inside the band of the path's constraint.  constraints: None,
        one EEConstraint for all paths or one per path; settings: the fields of planning.RetimeConstrainedSettings.
        -> retime_multi_raw's dict (status 5 = out_of_band) plus rounds, repaired, stops (per path) and levels (one
        uint8 per input waypoint, packed) with level_offsets.  planning.retime_multi_constrained is the caller-facing
        form.  Every argument is checked before any library call."""
        return self.retime_multi_raw(paths, vel_limits, acc_limits, environments, settings, constrained=(constraints, constraint_settings))

    def _retime_band_pairs(self, positions, sample_offsets, constraints, constraint_settings=None):
        """NOT part of the supported interface (the library's vmv_retime_band_pairs_host is not in the public header
        either): for the test that compares the band kernel with constraint_check_motion_batch.  The answers of retime_multi_constrained's band kernel for the
        consecutive pairs of packed sample lists -> uint8 [rows], 1 in every list's last row"""
        pos = np.ascontiguousarray(_f32(positions)).reshape(-1, self._dim)
        off = np.ascontiguousarray(sample_offsets, dtype=np.uintp)
        n = len(off) - 1
        if n < 1 or int(off[-1]) != len(pos):
            raise ValueError("sample_offsets must list at least one path and end at the row count")
        records, count = _constraint_records(constraints, n)
        ps = (constraint_settings or ConstraintSettings()).struct()
        ok = np.zeros(len(pos), np.uint8)
        check(lib.vmv_retime_band_pairs_host(self._id, _fp(pos), off.ctypes.data_as(_lib.c_size_p), n, records, count,
                                             ctypes.byref(ps), ok.ctypes.data_as(_lib.c_u8_p)), "vmv_retime_band_pairs_host")
        return ok

    def validate_batch_multi(self, configurations, environments, counts):
        """bool[n]: configurations [sum(counts[:k]), sum(counts[:k + 1])) against environments[k] (None = the empty
        environment), in one call.  The same answers as one validate_batch per environment, concatenated.  numpy in ->
        numpy out; torch CUDA tensor in -> torch.bool CUDA tensor out, launched on torch's current stream."""
        return self._batched("vmv_validate_batch_multi", [configurations], [((), "bits", True)],
                             environments=environments, counts=counts)[0]

    def validate_motion_batch_multi(self, starts, goals, environments, counts):
        """bool[n]: edges starts[i] -> goals[i], [sum(counts[:k]), sum(counts[:k + 1])) against environments[k] (None =
        the empty environment), in one call.  The same answers as one validate_motion_batch per environment,
        concatenated.  numpy in -> numpy out; torch CUDA tensors in -> torch.bool CUDA tensor out, launched on torch's
        current stream."""
        return self._batched("vmv_validate_motion_batch_multi", [starts, goals], [((), "bits", True)],
                             environments=environments, counts=counts)[0]

    def validate_motion_batch(self, starts, goals, environment: Environment | None = None):
        return self._batched("vmv_validate_motion_batch", [starts, goals], [((), "bits", True)], environment)[0]

    def fk_batch(self, configurations):
        """float32 [n][n_spheres][4] = x y z r."""
        return self._batched("vmv_fk_batch", [configurations], [((self._ns, 4), "f32", True)])[0]

    def halton_device(self, n: int, skip: int = 0):
        """Samples skip+1 .. skip+n of the reference's Halton sequence (random/halton.hh), generated on the GPU.
        Returns a torch float32 CUDA tensor [n][dimension] (bit-exact against the reference's sequence)."""
        import torch

        q = torch.empty((n, self._dim), dtype=torch.float32, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        check(lib.vmv_halton_configs(self._id, int(skip), ctypes.c_void_p(q.data_ptr()), n, stream),
              "vmv_halton_configs")
        return q

    # device-resident (torch tensors are only the memory/stream plumbing) ------------------------------------
    def validate_bits_device(self, q, environment, bits, goals=None):
        """q (and goals): torch float32 CUDA [n][dim] contiguous; bits: torch int64 CUDA [ceil(n/64)].
        Launches on torch's current stream; returns nothing (bits is filled in place)."""
        import torch

        n = q.shape[0]
        assert q.is_contiguous() and q.dtype == torch.float32 and q.shape[1] == self._dim
        assert bits.is_contiguous() and bits.dtype == torch.int64 and bits.numel() >= (n + 63) // 64
        stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
        env = self._env(environment)
        if goals is None:
            check(lib.vmv_validate_batch(self._id, env, ctypes.c_void_p(q.data_ptr()), n,
                                         ctypes.c_void_p(bits.data_ptr()), stream), "vmv_validate_batch")
        else:
            assert goals.is_contiguous() and goals.shape == q.shape and goals.dtype == torch.float32
            check(lib.vmv_validate_motion_batch(self._id, env, ctypes.c_void_p(q.data_ptr()),
                                                ctypes.c_void_p(goals.data_ptr()), n, ctypes.c_void_p(bits.data_ptr()),
                                                stream), "vmv_validate_motion_batch")


_EMPTY_ENVIRONMENT = Environment()

from . import api as _api  # noqa: E402  (the reference's planner-facing names; needs the classes above)
from .api import (AORRTCSettings, FCITNeighborParams, FCITSettings, PRMNeighborParams, PRMSettings,  # noqa: E402,F401
                  RRTCSettings, SimplifyRoutine, SimplifySettings, results_to_dict, DEFAULT_ITERATIONS, ROBOT_RRT_RANGES)

_ROBOT_MODULES = {}
for _name in robots:
    _mod = _Robot(_name)
    _api.install(_mod)
    _ROBOT_MODULES[_name] = _mod
    globals()[_name] = _mod
    sys.modules[_mod.__name__] = _mod
    __all__.append(_name)
__all__ += ["configure_robot_and_planner_with_kwargs", "problem_dict_to_vamp", "results_to_dict", "RRTCSettings",
            "PRMSettings", "PRMNeighborParams", "FCITSettings", "FCITNeighborParams", "AORRTCSettings", "SimplifySettings",
            "SimplifyRoutine"]


def configure_robot_and_planner_with_kwargs(robot_name: str, planner_name: str, **kwargs):
    """vamp.configure_robot_and_planner_with_kwargs (reference src/vamp/__init__.py:69-139)"""
    if robot_name not in _ROBOT_MODULES:
        raise AttributeError(robot_name)
    return _api.configure_robot_and_planner_with_kwargs(_ROBOT_MODULES, robot_name, planner_name, **kwargs)


def problem_dict_to_vamp(problem, ignore_names=()):
    """vamp.problem_dict_to_vamp (reference src/vamp/__init__.py:140-186): MotionBenchMaker scene dict -> Environment.
    Cylinders become capsules, except in the "box" problem where they are over-approximated by cuboids."""
    env = Environment()
    for obj in problem["sphere"]:
        if obj["name"] not in ignore_names:
            s = Sphere(obj["position"], obj["radius"])
            s.name = obj["name"]
            env.add_sphere(s)
    for obj in problem["cylinder"]:
        if obj["name"] in ignore_names:
            continue
        if problem["problem"] == "box":
            c = Cuboid(obj["position"], obj["orientation_euler_xyz"], [obj["radius"], obj["radius"], obj["length"] / 2])
            c.name = obj["name"]
            env.add_cuboid(c)
        else:
            c = Cylinder(obj["position"], obj["orientation_euler_xyz"], obj["radius"], obj["length"])
            c.name = obj["name"]
            env.add_capsule(c)
    for obj in problem["box"]:
        if obj["name"] not in ignore_names:
            c = Cuboid(obj["position"], obj["orientation_euler_xyz"], obj["half_extents"])
            c.name = obj["name"]
            env.add_cuboid(c)
    return env
