// vmv_prm_common.h — what the roadmap calls share (vmv_prm_multi; vmv_fcit_multi, §5g; vmv_roadmaps_*, §5h):
// the limits, the fp32 arithmetic of the contract (d2, the (d2, id) order, fl(g + w)), the per-problem vertex layout of
// vmv_prm_multi and vmv_fcit_multi with its stage 1 (prm_stage_vertices), the Halton fill, the edge-offsets kernel and the
// walk gather.  The neighbour, count, write and shortest-path kernels stay with vmv_prm_multi and vmv_roadmaps_*: their
// vertex layouts differ (endpoints as vertices 0 and 1 there, samples alone here), and with them every line.
// Kernels defined here have internal linkage: each translation unit launches its own copy.
#pragma once

#include "vmv_lockstep.h"

#include <cmath>
#include <cstring>

namespace vmv
{
    constexpr uint32_t kPrmBlock = 256;
    constexpr uint32_t kPrmKMax = 16;
    constexpr uint32_t kPrmMinSamples = 64, kPrmMaxSamples = 8128;
    constexpr uint32_t kPrmMaxVertices = kPrmMaxSamples + 2;
    constexpr uint32_t kPrmSsspBlock = 512;
    constexpr uint32_t kPrmLaunchBlocks = 32768;  // workgroups per launch of the per-problem kernels: a larger call
                                                  // is launched chunk by chunk of problems (grids stay far below 2^32 threads)
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

    // The vertex layout of vmv_prm_multi and vmv_fcit_multi: the samples of all problems [P][n_samples][dim], then
    // (start, goal) of all problems [P][2][dim]; vertex 0 = start, 1 = goal, 2 + i = sample i.  Params: PrmLayout or a
    // call's own parameter struct with these members.
    struct PrmLayout
    {
        uint32_t dim, n_samples, n_problems;
    };
    template <typename Params>
    __device__ __forceinline__ size_t vertex_at(const Params &P, uint32_t p, uint32_t v)  // index into verts / vbits
    {
        return v < 2u ? (size_t) P.n_problems * P.n_samples + 2u * (size_t) p + v : (size_t) p * P.n_samples + (v - 2u);
    }
    template <typename Params>
    __device__ __forceinline__ bool ends_valid(const Params &P, const uint64_t *__restrict__ vbits, uint32_t p)
    {
        return bit_at(vbits, vertex_at(P, p, 0)) && bit_at(vbits, vertex_at(P, p, 1));
    }

    struct JointBounds
    {
        float lower[kPlanMaxDim], span[kPlanMaxDim];
    };

    namespace
    {
        // verts [total / dim][dim]: sample s is element skips[s / n_samples] + 1 + s % n_samples of the Halton sequence
        __global__ __launch_bounds__(kPrmBlock) void halton_fill_kernel(float *__restrict__ verts, const uint64_t *__restrict__ skips,
                                                                         const size_t total, const uint32_t n_samples,
                                                                         const uint32_t dim, const JointBounds B)
        {
            const size_t i = (size_t) blockIdx.x * kPrmBlock + threadIdx.x;
            if (i >= total) return;
            const uint32_t j = (uint32_t) (i % dim);
            const size_t s = i / dim;
            verts[i] = halton_element(skips[s / n_samples] + 1ull + s % n_samples, (int) j, B.lower[j], B.span[j]);
        }

        // edge_offsets[p] = first[p * stride] for p = 0 .. n: the first candidate edge of each problem / roadmap
        __global__ __launch_bounds__(kPrmBlock) void edge_offsets_kernel(uint32_t *__restrict__ edge_offsets,
                                                                          const uint32_t *__restrict__ first, const uint32_t n,
                                                                          const uint32_t stride)
        {
            const uint32_t p = blockIdx.x * kPrmBlock + threadIdx.x;
            if (p <= n) edge_offsets[p] = first[(size_t) p * stride];
        }

        // the waypoints of problem p's walk [P][V] of vertex ids, packed at offsets[p]; its length is
        // path_len[p * len_stride]; backwards: the walk was written from the goal
        __global__ __launch_bounds__(kPrmBlock) void walk_gather_kernel(const PrmLayout L, const float *__restrict__ verts,
                                                                         const uint32_t *__restrict__ walks,
                                                                         const uint32_t *__restrict__ path_len, const uint32_t len_stride,
                                                                         const bool backwards, const uint64_t *__restrict__ offsets,
                                                                         float *__restrict__ paths)
        {
            const uint32_t p = blockIdx.x * kPrmBlock + threadIdx.x, V = L.n_samples + 2u;
            if (p >= L.n_problems) return;
            const uint32_t stored = path_len[(size_t) p * len_stride], len = stored <= V ? stored : 0u;
            const uint32_t *walk = walks + (size_t) p * V;
            float *out = paths + offsets[p] * L.dim;
            for (uint32_t s = 0; s < len; ++s)
            {
                const uint32_t v = walk[backwards ? len - 1u - s : s];
                if (v >= V) return;
                const float *q = verts + vertex_at(L, p, v) * L.dim;
                for (uint32_t j = 0; j < L.dim; ++j) out[(size_t) s * L.dim + j] = q[j];
            }
        }
    }  // namespace

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

    namespace
    {
    // n_sets * n_samples Halton samples into verts, set r after skips[r] (NULL = zeros); `kernel` names the launch in
    // vmv_last_error()
    inline int halton_fill(float *verts, uint64_t *d_skips, const uint64_t *skips, size_t n_sets, uint32_t n_samples, uint32_t dim,
                           const float *lower, const float *span, hipStream_t stream, const char *kernel)
    {
        if (int rc = upload_skips(d_skips, skips, n_sets, stream); rc != VMV_OK) return rc;
        JointBounds B{};
        for (uint32_t j = 0; j < dim; ++j) B.lower[j] = lower[j], B.span[j] = span[j];
        const size_t total = n_sets * n_samples * dim;
        hipLaunchKernelGGL(halton_fill_kernel, dim3((uint32_t) ((total + kPrmBlock - 1) / kPrmBlock)), dim3(kPrmBlock), 0, stream, verts,
                           d_skips, total, n_samples, dim, B);
        VMV_PRM_LAUNCHED(kernel);
        return VMV_OK;
    }

    // Stage 1 of vmv_prm_multi and vmv_fcit_multi: the vertices in PrmLayout's order (the caller's samples or the Halton
    // fill; then start, goal of every problem) and ONE vmv_validate_batch_multi call over 2 n segments: the samples of
    // each problem, then its two endpoints.
    inline int prm_stage_vertices(int robot, const vmv_env *const *envs, size_t n, uint32_t n_samples, uint32_t dim, const float *starts,
                                  const float *goals, const uint64_t *skips, const float *samples, const float *lower,
                                  const float *span, float *verts, uint64_t *d_skips, uint64_t *d_vbits, hipStream_t stream,
                                  const char *halton_kernel)
    {
        const size_t ns = n_samples, n_sample_cfgs = n * ns;
        if (samples)
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(verts, samples, n_sample_cfgs * dim * 4, hipMemcpyHostToDevice, stream));
        else if (int rc = halton_fill(verts, d_skips, skips, n, n_samples, dim, lower, span, stream, halton_kernel); rc != VMV_OK)
            return rc;
        std::vector<float> ends(2 * n * (size_t) dim);
        for (size_t p = 0; p < n; ++p)
        {
            std::memcpy(&ends[(2 * p) * (size_t) dim], starts + p * (size_t) dim, (size_t) dim * 4);
            std::memcpy(&ends[(2 * p + 1) * (size_t) dim], goals + p * (size_t) dim, (size_t) dim * 4);
        }
        VMV_LOCKSTEP_HIP(hipMemcpy(verts + n_sample_cfgs * dim, ends.data(), ends.size() * 4, hipMemcpyHostToDevice));
        std::vector<const vmv_env *> envs2(2 * n);
        std::vector<size_t> seg(2 * n + 1);
        for (size_t p = 0; p < n; ++p)
        {
            envs2[p] = envs2[n + p] = envs[p];
            seg[p] = p * ns, seg[n + p] = n_sample_cfgs + 2 * p;
        }
        seg[2 * n] = n_sample_cfgs + 2 * n;
        const int rc = vmv_validate_batch_multi(robot, envs2.data(), seg.data(), 2 * n, verts, d_vbits, stream);
        if (rc != VMV_OK) (void) hipDeviceSynchronize();
        return rc;
    }
    }  // namespace
}  // namespace vmv
