// vmv_prm_common.h — what the roadmap calls share (vmv_prm_multi; vmv_roadmaps_*): the limits,
// the fp32 arithmetic of the contract (d2, the (d2, id) order, fl(g + w)) and the steps of the kernels that do not depend
// on where a call keeps its vertices.  The kernels themselves stay with each call: their vertex layouts differ.
#pragma once

#include "vmv_common.h"

#include <cmath>

namespace vmv
{
    constexpr uint32_t kPrmBlock = 256;
    constexpr uint32_t kPrmKMax = 16;
    constexpr uint32_t kPrmMaxDim = 16;
    constexpr uint32_t kPrmMinSamples = 64, kPrmMaxSamples = 8128;
    constexpr uint32_t kPrmMaxVertices = kPrmMaxSamples + 2;
    constexpr uint32_t kPrmSsspBlock = 512;
    constexpr uint32_t kPrmLaunchBlocks = 32768;  // workgroups per launch of the per-problem kernels: a larger call
                                                  // is launched chunk by chunk of problems (grids stay far below 2^32 threads)
    constexpr uint32_t kNone = 0xffffffffu;
    constexpr uint32_t kInfBits = 0x7f800000u;

    __device__ __forceinline__ bool bit_at(const uint64_t *__restrict__ bits, size_t i)
    {
        return (bits[i >> 6] >> (i & 63u)) & 1ull;
    }
    __device__ __forceinline__ float dist2(const float *__restrict__ a, const float *__restrict__ b, uint32_t dim)
    {
        float sum = 0.f;
        for (uint32_t j = 0; j < dim; ++j)
        {
            const float df = a[j] - b[j];
            sum = sum + df * df;
        }
        return sum;
    }

    // The k best of a neighbour search sit in registers as a sorted list of kPrmKMax entries, fully unrolled; the
    // list's first kPrmKMax - k entries hold the key 0, below every real key (d2 > 0), so they never move and the k-th
    // best is always the last entry: one strict `<` against it rejects most candidates.  Keys are the bits of d2
    // (positive floats order as unsigned integers; +inf included); an empty entry holds 0xffffffff.  Candidates come
    // in ascending id order, so among equal keys the strict `<` keeps the lower id.
    __device__ __forceinline__ void knn_list_init(uint32_t (&bk)[kPrmKMax], uint32_t (&bi)[kPrmKMax], uint32_t k)
    {
#pragma unroll
        for (uint32_t s = 0; s < kPrmKMax; ++s) bk[s] = s < kPrmKMax - k ? 0u : kNone, bi[s] = kNone;
    }
    __device__ __forceinline__ void knn_list_insert(uint32_t (&bk)[kPrmKMax], uint32_t (&bi)[kPrmKMax], uint32_t key, uint32_t u)
    {
#pragma unroll
        for (int s = kPrmKMax - 1; s >= 1; --s)
        {
            const bool shift = key < bk[s - 1];
            const bool here = !shift && key < bk[s];
            bi[s] = shift ? bi[s - 1] : (here ? u : bi[s]);
            bk[s] = shift ? bk[s - 1] : (here ? key : bk[s]);
        }
        if (key < bk[0]) bk[0] = key, bi[0] = u;
    }

    // slot s of vertex v is an edge of the list iff v < u, or v is not among u's neighbours (nbr_p: [vertices][k])
    __device__ __forceinline__ bool owns(const uint32_t *__restrict__ nbr_p, uint32_t k, uint32_t v, uint32_t u)
    {
        if (v < u) return true;
        bool found = false;
        for (uint32_t t = 0; t < k; ++t) found |= nbr_p[(size_t) u * k + t] == v;
        return !found;
    }

    // One edge {a, b} of weight w in a shortest-path sweep.  g lives in LDS as the bits of non-negative floats, which
    // order as unsigned integers: g[v] = min over the edges {u, v} of fl(g[u] + w) is reached by edge-parallel sweeps with
    // atomicMin in both directions; fl(a + w) is monotone in a and >= a, so the least fixpoint is the same whatever the
    // order of the relaxations.  A w that is not finite relaxes nothing.  -> whether g changed
    __device__ __forceinline__ int sssp_relax(uint32_t *g, uint32_t a, uint32_t b, float w)
    {
        int changed = 0;
        if (!(w < INFINITY)) return 0;
        const uint32_t ga = g[a], gb = g[b];
        if (ga < kInfBits)
        {
            const uint32_t c = __float_as_uint(__uint_as_float(ga) + w);
            if (c < gb) changed |= atomicMin(&g[b], c) > c;
        }
        if (gb < kInfBits)
        {
            const uint32_t c = __float_as_uint(__uint_as_float(gb) + w);
            if (c < ga) changed |= atomicMin(&g[a], c) > c;
        }
        return changed;
    }
    // whether u, over an edge of weight w, may be the parent of a vertex whose g is gc
    __device__ __forceinline__ bool sssp_is_parent(const uint32_t *g, uint32_t gc, uint32_t u, float w)
    {
        const uint32_t gu = g[u];
        return w < INFINITY && gu < gc && __float_as_uint(__uint_as_float(gu) + w) == gc;
    }

#define VMV_PRM_LAUNCHED(name)                                \
    do                                                        \
    {                                                         \
        const hipError_t e_ = hipGetLastError();              \
        if (e_ != hipSuccess)                                 \
        {                                                     \
            (void) hipDeviceSynchronize();                    \
            return hip_status(e_, name);                      \
        }                                                     \
    } while (0)
}  // namespace vmv
