// Test program: the device-free part of the launchers' plan (vamp_mvt_amd/csrc/vmv_common.h: env_class, the index of every
// per-robot kernel table, and MultiTableLayout, the [segments | tiles] table of the multi-environment launches) under
// AddressSanitizer + UBSan.  vmv_common.h needs the HIP headers, so this is compiled as HIP for the host only; it makes no
// HIP call.  Built and run by tests/test_native_sanitize.py (CPU only).
#include "../../vamp_mvt_amd/csrc/vmv_common.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int fail(const char *what)
{
    std::printf("FAIL: %s\n", what);
    return 1;
}

// an environment of nothing but `n` floats of sphere records
static vmv::EnvLaunch spheres(uint32_t n_floats)
{
    vmv::EnvLaunch e{};
    e.host.n_sphere = n_floats / 4u;
    e.host.n_floats = n_floats;
    return e;
}

// the table filled through the layout's own pointers, in a buffer of exactly `bytes`: every write in bounds (ASan), every
// pointer aligned for its type (UBSan), the tiles behind the segments
static bool layout_ok(size_t n_segs, size_t n_tiles)
{
    const vmv::MultiTableLayout T(n_segs, n_tiles);
    if (T.tiles_at % 16u != 0u || T.tiles_at < n_segs * sizeof(vmv::MultiSeg) || T.tiles_at >= n_segs * sizeof(vmv::MultiSeg) + 16u)
        return false;
    if (T.bytes != T.tiles_at + n_tiles * sizeof(vmv::MultiTile)) return false;
    std::vector<char> raw(T.bytes + 16u);
    char *base = raw.data() + (16u - reinterpret_cast<uintptr_t>(raw.data()) % 16u) % 16u;  // as the lease's buffers: 16-byte aligned
    std::memset(base, 0x5a, T.bytes);
    vmv::MultiSeg *segs = T.segs(base);
    vmv::MultiTile *tiles = T.tiles(base);
    if (static_cast<void *>(segs) != base || reinterpret_cast<char *>(tiles) != base + T.tiles_at) return false;
    for (size_t k = 0; k < n_segs; ++k) segs[k] = vmv::MultiSeg{nullptr, (uint32_t) k, (uint32_t) k + 1u, 0u, 7u};
    for (size_t t = 0; t < n_tiles; ++t) tiles[t] = vmv::MultiTile{(uint32_t) (t % (n_segs ? n_segs : 1u)), (uint32_t) t};
    for (size_t k = 0; k < n_segs; ++k)  // the tiles did not overwrite a segment
        if (segs[k].lo != k || segs[k].hi != k + 1u || segs[k].slab != 7u) return false;
    for (size_t t = 0; t < n_tiles; ++t)
        if (tiles[t].word != t) return false;
    return true;
}

int main()
{
    // ---- the class of an environment: 0 kEnvZOnly, 1 kEnvPrims, 2 kEnvFull, 3 kEnvClouds
    static_assert(vmv::kEnvClasses == 4 && vmv::kEdgeMultiClasses == vmv::kEnvClasses, "one index for every table");
    vmv::EnvLaunch e{};
    if (vmv::env_class(e) != 0) return fail("the empty environment runs kEnvZOnly");
    e = spheres(64);
    e.host.n_zcapsule = 3, e.host.n_zcuboid = 2;
    if (vmv::env_class(e) != 0) return fail("spheres, z-capsules and z-cuboids run kEnvZOnly");
    e.host.n_attach = 5;
    if (vmv::env_class(e) != 0) return fail("an attachment does not change the class");
    e = spheres(64);
    e.host.n_capsule = 1;
    if (vmv::env_class(e) != 1) return fail("a capsule asks for kEnvPrims");
    e = spheres(64);
    e.host.n_cuboid = 1;
    if (vmv::env_class(e) != 1) return fail("a cuboid asks for kEnvPrims");
    // ill-formed primitives: the variant that keeps the reference's groups, whatever the lists hold
    e.host.ill_formed = 1;
    if (vmv::env_class(e) != 2) return fail("an ill-formed cuboid falls to kEnvFull");
    e = spheres(64);
    e.host.ill_formed = 1;
    if (vmv::env_class(e) != 2) return fail("ill_formed falls to kEnvFull without capsules and cuboids too");
    e = spheres(0);
    e.host.n_capt = 1;
    if (vmv::env_class(e) != 3) return fail("a point cloud alone runs kEnvClouds");
    e.host.n_capt = 2;
    if (vmv::env_class(e) != 3) return fail("two point clouds alone run kEnvClouds");
    e = spheres(64);
    e.host.n_capt = 1;
    if (vmv::env_class(e) != 2) return fail("a point cloud beside primitives runs kEnvFull");
    for (int what = 0; what < 2; ++what)
        for (uint32_t n_capt = 0; n_capt < 2; ++n_capt)
        {
            e = spheres(0);
            e.host.n_capt = n_capt;
            (what ? e.host.n_mvt : e.host.n_heightfield) = 1;
            if (vmv::env_class(e) != 2) return fail("an MVT cloud or a heightfield runs kEnvFull, with a CAPT cloud or without");
        }

    // ---- the [segments | tiles] table: 0, 1 and 3 segments, without tiles and with
    static_assert(sizeof(vmv::MultiSeg) == 24 && sizeof(vmv::MultiTile) == 8, "the sizes the cases below are chosen for");
    for (const size_t n_segs : {size_t{0}, size_t{1}, size_t{3}})
        for (const size_t n_tiles : {size_t{0}, size_t{1}, size_t{5}, size_t{1000}})
            if (!layout_ok(n_segs, n_tiles)) return fail("MultiTableLayout");
    if (vmv::MultiTableLayout(0, 0).bytes != 0u) return fail("the empty table has no bytes");
    if (vmv::MultiTableLayout(1, 0).tiles_at != 32u) return fail("one segment: 24 bytes rounded to 32");
    if (vmv::MultiTableLayout(3, 2).tiles_at != 80u || vmv::MultiTableLayout(3, 2).bytes != 96u)
        return fail("three segments: 72 bytes rounded to 80, two tiles behind them");
    if (vmv::MultiTableLayout(2, 1).tiles_at != 48u) return fail("two segments end on a boundary: no padding");
    std::printf("OK\n");
    return 0;
}
