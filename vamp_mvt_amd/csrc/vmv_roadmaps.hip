// vmv_roadmaps.hip — device-resident roadmaps: built once per scene, asked many times (vmv_roadmaps_*).
//
// vmv_roadmaps_build has the shape of vmv_prm_multi without endpoints: the samples of all roadmaps and ONE
// vmv_validate_batch_multi call; rm_knn_kernel (the k nearest valid samples of every valid sample); the candidate edges
// counted, scanned and written in the contract's order and ONE vmv_validate_motion_batch_multi call.  The host
// synchronises once, for the per-roadmap edge counts.  Samples, validity words, pairs, weights and edge answers stay on
// the device inside the handle.
//
// vmv_roadmaps_query is a fixed launch sequence with no host synchronisation before the results: the 2 Q endpoints,
// grouped by roadmap, and ONE vmv_validate_batch_multi call; rm_connect_kernel (one wave per endpoint: its k_connect
// nearest valid samples); 1 + 2 k_connect edge questions per query and ONE vmv_validate_motion_batch_multi call;
// rm_query_sssp_kernel (one workgroup per query: the fp32 shortest-path fixpoint over the roadmap's shared edge list plus
// the query's own connection edges, and the parent walk); the paths gathered into the packed vmv_plans buffers.
//
// The Halton fill and the edge-offsets kernel are vmv_prm_common.h's, shared with vmv_prm_multi; the result tail is
// pack_paths of vmv_lockstep.h.
// Arithmetic contract: that of vmv_prm_multi.hip (fp32, one rounding per written operation, keys (d2, id)).  On the device
// the queries are in the order of the host's stable counting sort by roadmap ("position" s below); the host un-permutes.
// Plain vector stores; atomics on LDS words only.  Every loop has a bound that holds whatever the data says.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"
#include "vmv_prm_common.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

struct vmv_roadmaps
{
    int robot = -1, dim = 0, device = -1;
    uint32_t n_samples = 0, k = 0;
    size_t n = 0;
    std::vector<const vmv_env *> envs;       // [n] as finalized at build time; they must outlive the handle
    std::vector<uint32_t> edge_offsets;      // [n + 1] first candidate edge of each roadmap
    std::vector<uint32_t> valid_vertices, valid_edges;  // [n]
    vmv::DeviceBuffers mem;                  // owns everything below
    float *verts = nullptr;                  // [n][n_samples][dim]
    uint64_t *vbits = nullptr;               // their validity; a roadmap owns whole words
    uint32_t *d_edge_offsets = nullptr;      // [n + 1]
    uint32_t *pairs = nullptr;               // [E][2] sample ids a < b, in candidate order
    float *weights = nullptr;                // [E]
    uint64_t *ebits = nullptr;               // the edges' answers
};

namespace vmv
{
    namespace
    {
        constexpr uint32_t kConnectMax = 32;

        struct BuildParams
        {
            uint32_t dim, n_samples, k, n_roadmaps;
            float r2;
        };
        struct BuildArrays
        {
            float *verts;            // [R][n_samples][dim]
            const uint64_t *vbits;
            uint64_t *skips;         // [R] the Halton skips the samples come after
            uint32_t *nbr;           // [R][n_samples][k] neighbour lists, kNone after the last
            uint32_t *counts;        // [R * n_samples + 1] candidate edges owned by (roadmap, sample), the last 0
            uint32_t *first;         // [R * n_samples + 1] their exclusive scan, the last the total
            uint32_t *edge_offsets;  // [R + 1]
            uint32_t *pairs;         // [E][2]
            float *weights;          // [E]
            float *q_a, *q_b;        // [E][dim] the edge questions
            const uint64_t *ebits;
            uint32_t *stats;         // [R][2] valid vertices, valid edges
        };

        // prm_knn_kernel over a roadmap's samples alone: one lane per sample, a workgroup within one roadmap (roadmap
        // r0 + blockIdx.x / tiles, tile blockIdx.x % tiles), the candidates through LDS a tile of kPrmBlock at a time.
        // n_samples is a multiple of 64, not of kPrmBlock: the last tile may be short.
        template <int DIM>
        __global__ __launch_bounds__(kPrmBlock) void rm_knn_kernel(const BuildParams P, const BuildArrays D, const uint32_t r0, const uint32_t tiles)
        {
            __shared__ __align__(16) float s_tile[kPrmBlock * DIM];
            __shared__ uint32_t s_valid[kPrmBlock];
            const uint32_t r = r0 + blockIdx.x / tiles, tid = threadIdx.x, v = (blockIdx.x % tiles) * kPrmBlock + tid;
            const uint32_t ns = P.n_samples, dim = P.dim;
            const size_t base_r = (size_t) r * ns;
            const bool query = v < ns && bit_at(D.vbits, base_r + v);
            float q[DIM];
#pragma unroll
            for (int j = 0; j < DIM; ++j) q[j] = (query && (uint32_t) j < dim) ? D.verts[(base_r + v) * dim + j] : 0.f;
            uint32_t bk[kPrmKMax], bi[kPrmKMax];
            knn_list_init(bk, bi, P.k);
            const uint32_t r2_bits = __float_as_uint(P.r2);

            for (uint32_t base = 0; base < ns; base += kPrmBlock)  // <= ceil(n_samples / kPrmBlock) tiles
            {
                const uint32_t u_mine = base + tid;
                const bool ok = u_mine < ns && bit_at(D.vbits, base_r + u_mine);
                s_valid[tid] = ok ? 1u : 0u;
#pragma unroll
                for (int j = 0; j < DIM; ++j)
                    s_tile[tid * DIM + j] = (ok && (uint32_t) j < dim) ? D.verts[(base_r + u_mine) * dim + j] : 0.f;
                __syncthreads();
                const uint32_t count = ns - base < kPrmBlock ? ns - base : kPrmBlock;
                if (query)
                    for (uint32_t c = 0; c < count; ++c)
                    {
                        if (!s_valid[c]) continue;  // the same in every lane
                        const uint32_t u = base + c;
                        float sum = 0.f;
#pragma unroll
                        for (int j = 0; j < DIM; ++j)
                        {
                            const float df = q[j] - s_tile[c * DIM + j];
                            sum = sum + df * df;
                        }
                        const uint32_t key = __float_as_uint(sum);  // valid samples are finite: sum is in [+0, +inf]
                        if (!(key < bk[kPrmKMax - 1])) continue;
                        if (key == 0u || key > r2_bits || u == v) continue;
                        knn_list_insert(bk, bi, key, u);
                    }
                __syncthreads();  // the tile is rewritten
            }
            if (v < ns)
            {
                uint32_t *out = D.nbr + (base_r + v) * P.k;
#pragma unroll
                for (uint32_t s = 0; s < kPrmKMax; ++s)
                    if (s >= kPrmKMax - P.k) out[s - (kPrmKMax - P.k)] = bi[s];
            }
        }

        // counts[r * n_samples + v] = the candidate edges sample v of roadmap r contributes; counts[R * n_samples] = 0,
        // so that the exclusive scan ends with the total
        __global__ __launch_bounds__(kPrmBlock) void rm_count_kernel(const BuildParams P, const BuildArrays D)
        {
            const size_t total = (size_t) P.n_roadmaps * P.n_samples;
            const size_t i = (size_t) blockIdx.x * kPrmBlock + threadIdx.x;
            if (i > total) return;
            uint32_t n = 0;
            if (i < total && bit_at(D.vbits, i))
            {
                const uint32_t v = (uint32_t) (i % P.n_samples);
                const uint32_t *nbr_r = D.nbr + (i - v) * P.k;
                for (uint32_t s = 0; s < P.k; ++s)
                {
                    const uint32_t u = nbr_r[(size_t) v * P.k + s];
                    if (u >= P.n_samples) break;  // kNone: the list ended
                    n += owns(nbr_r, P.k, v, u) ? 1u : 0u;
                }
            }
            D.counts[i] = n;
        }

        // the edges of (r, v) start at first[r * n_samples + v], in slot order; each is asked lower id -> higher id
        __global__ __launch_bounds__(kPrmBlock) void rm_write_kernel(const BuildParams P, const BuildArrays D)
        {
            const size_t total = (size_t) P.n_roadmaps * P.n_samples;
            const size_t i = (size_t) blockIdx.x * kPrmBlock + threadIdx.x;
            if (i >= total) return;
            uint32_t e = D.first[i];
            const uint32_t end = D.first[i + 1];
            const uint32_t v = (uint32_t) (i % P.n_samples), dim = P.dim;
            const uint32_t *nbr_r = D.nbr + (i - v) * P.k;
            const float *verts_r = D.verts + (i - v) * dim;
            for (uint32_t s = 0; s < P.k && e < end; ++s)
            {
                const uint32_t u = nbr_r[(size_t) v * P.k + s];
                if (u >= P.n_samples) break;
                if (!owns(nbr_r, P.k, v, u)) continue;
                const uint32_t a = v < u ? v : u, b = v < u ? u : v;
                const float *qa = verts_r + (size_t) a * dim, *qb = verts_r + (size_t) b * dim;
                D.pairs[2 * (size_t) e] = a, D.pairs[2 * (size_t) e + 1] = b;
                D.weights[e] = sqrtf(dist2(qa, qb, dim));
                for (uint32_t j = 0; j < dim; ++j) D.q_a[(size_t) e * dim + j] = qa[j], D.q_b[(size_t) e * dim + j] = qb[j];
                ++e;
            }
        }

        // one workgroup per roadmap: its valid samples and valid edges
        __global__ __launch_bounds__(kPrmBlock) void rm_stats_kernel(const BuildParams P, const BuildArrays D)
        {
            __shared__ uint32_t s_count[2];
            const uint32_t r = blockIdx.x, tid = threadIdx.x;
            if (tid < 2u) s_count[tid] = 0u;
            __syncthreads();
            uint32_t mine = 0;
            for (uint32_t v = tid; v < P.n_samples; v += kPrmBlock) mine += bit_at(D.vbits, (size_t) r * P.n_samples + v) ? 1u : 0u;
            if (mine) atomicAdd(&s_count[0], mine);
            mine = 0;
            for (uint32_t e = D.edge_offsets[r] + tid; e < D.edge_offsets[r + 1]; e += kPrmBlock) mine += bit_at(D.ebits, e) ? 1u : 0u;
            if (mine) atomicAdd(&s_count[1], mine);
            __syncthreads();
            if (tid < 2u) D.stats[2 * (size_t) r + tid] = s_count[tid];
        }

        // ---- queries ----
        struct QueryParams
        {
            uint32_t dim, n_samples, V, kc, per, n_queries;  // per = 1 + 2 kc question slots per query
            float r2;
        };
        struct QueryResult  // 32 bytes per query
        {
            uint32_t status, path_len, iterations, start_edges, goal_edges, edges_checked;
            float cost;
            uint32_t pad;
        };
        struct QueryArrays
        {
            // the handle's
            const float *verts;
            const uint64_t *vbits;
            const uint32_t *edge_offsets, *pairs;
            const float *weights;
            const uint64_t *ebits;
            // the call's, by position
            const float *ends;         // [Q][2][dim] start, goal
            const uint64_t *end_bits;  // [2 Q] their validity
            const uint32_t *roadmap;   // [Q]
            uint32_t *conn_id;         // [Q][2][kc] conn(start), conn(goal): sample ids
            float *conn_w;             // [Q][2][kc] their weights
            uint32_t *conn_n;          // [Q][2] their lengths
            float *q_a, *q_b;          // [Q][per][dim] the questions: start -> goal; start -> conn(start); goal -> conn(goal)
            const uint64_t *q_bits;    // their answers
            uint32_t *walk;            // [Q][V] the path's graph ids from the goal backwards
            QueryResult *result;       // [Q]
        };

        // One wave per endpoint (workgroup e0 + blockIdx.x = 2 * position + (0 start, 1 goal)).  Lane l owns the samples
        // l, l + 64, ...: it writes their keys (the bits of d2; kNone for a sample that is invalid, at d2 = 0 or beyond the
        // radius) into LDS and is the only lane to read them again, so the wave needs no barrier.  Then at most k_connect
        // selection passes: every lane's least (key, id) among its samples, a wave min-reduction, the winner's key struck
        // out.  The order is total, so the list is the contract's.  A query with an invalid endpoint asks nothing: all its
        // slots carry the null question (the endpoint to itself), as every slot beyond a list's end does.
        template <int DIM>
        __global__ __launch_bounds__(kWave) void rm_connect_kernel(const QueryParams P, const QueryArrays D, const uint32_t e0)
        {
            extern __shared__ uint32_t s_key[];  // [n_samples]
            const uint32_t ep = e0 + blockIdx.x, s = ep >> 1, side = ep & 1u, lane = threadIdx.x;
            const uint32_t ns = P.n_samples, dim = P.dim, kc = P.kc;
            const bool both = bit_at(D.end_bits, 2 * (size_t) s) && bit_at(D.end_bits, 2 * (size_t) s + 1);  // wave-uniform
            const float *me = D.ends + (size_t) ep * dim;
            const size_t slot0 = (size_t) s * P.per;
            float *qa = D.q_a + (slot0 + 1 + side * kc) * dim, *qb = D.q_b + (slot0 + 1 + side * kc) * dim;
            uint32_t found = 0;
            if (both)
            {
                const size_t base_r = (size_t) D.roadmap[s] * ns;
                const float *verts_r = D.verts + base_r * dim;
                const uint64_t *words = D.vbits + base_r / 64;
                float q[DIM];
#pragma unroll
                for (int j = 0; j < DIM; ++j) q[j] = (uint32_t) j < dim ? me[j] : 0.f;
                const uint32_t r2_bits = __float_as_uint(P.r2);
                for (uint32_t u = lane; u < ns; u += kWave)  // n_samples / 64 rounds
                {
                    uint32_t key = kNone;
                    if ((words[u >> 6] >> lane) & 1ull)
                    {
                        float sum = 0.f;
#pragma unroll
                        for (int j = 0; j < DIM; ++j)
                        {
                            const float df = q[j] - ((uint32_t) j < dim ? verts_r[(size_t) u * dim + j] : 0.f);
                            sum = sum + df * df;
                        }
                        const uint32_t bits = __float_as_uint(sum);  // finite operands: sum is in [+0, +inf]
                        if (bits != 0u && bits <= r2_bits) key = bits;
                    }
                    s_key[u] = key;
                }
                for (uint32_t pass = 0; pass < kc; ++pass)
                {
                    uint32_t bk = kNone, bu = kNone;
                    for (uint32_t u = lane; u < ns; u += kWave)  // ascending ids: the strict `<` keeps the lower one
                    {
                        const uint32_t key = s_key[u];
                        if (key < bk) bk = key, bu = u;
                    }
#pragma unroll
                    for (int off = kWave / 2; off >= 1; off >>= 1)
                    {
                        const uint32_t ok = __shfl_xor(bk, off), ou = __shfl_xor(bu, off);
                        if (ok < bk || (ok == bk && ou < bu)) bk = ok, bu = ou;
                    }
                    if (bk == kNone) break;  // the same in every lane: no sample is left
                    if ((bu & (kWave - 1u)) == lane) s_key[bu] = kNone;
                    if (lane == 0u) D.conn_id[(size_t) ep * kc + found] = bu, D.conn_w[(size_t) ep * kc + found] = sqrtf(__uint_as_float(bk));
                    if (lane < dim) qa[(size_t) found * dim + lane] = me[lane], qb[(size_t) found * dim + lane] = verts_r[(size_t) bu * dim + lane];
                    ++found;
                }
            }
            for (uint32_t i = found * dim + lane; i < kc * dim; i += kWave) qa[i] = qb[i] = me[i % dim];
            if (lane == 0u) D.conn_n[ep] = found;
            if (side == 0u && lane < dim)
            {
                D.q_a[slot0 * dim + lane] = me[lane];
                D.q_b[slot0 * dim + lane] = both ? me[dim + lane] : me[lane];  // the goal follows the start in `ends`
            }
        }

        // One workgroup per query (position s0 + blockIdx.x).  Graph ids: 0 = start, 1 = goal, 2 + i = sample i.  g lives
        // in LDS; a sweep relaxes the roadmap's valid edges, shared and read-only in global memory, and the query's valid
        // connection edges, one per thread of the first 2 k_connect; n_samples + 2 sweeps bound the fixpoint.  Then the
        // parent walk from the goal as in prm_sssp_kernel, at most n_samples + 1 steps.  Every branch around a barrier
        // depends on the query alone.
        __global__ __launch_bounds__(kPrmSsspBlock) void rm_query_sssp_kernel(const QueryParams P, const QueryArrays D, const uint32_t s0)
        {
            __shared__ uint32_t g[kPrmMaxVertices];
            __shared__ uint32_t s_best;
            const uint32_t s = s0 + blockIdx.x, tid = threadIdx.x, V = P.V, kc = P.kc;
            const size_t slot0 = (size_t) s * P.per;
            const bool both = bit_at(D.end_bits, 2 * (size_t) s) && bit_at(D.end_bits, 2 * (size_t) s + 1);
            QueryResult r{};
            r.status = VMV_PLAN_NO_PATH, r.cost = INFINITY;
            if (tid == 0u) s_best = kNone;

            const uint32_t n_start = D.conn_n[2 * (size_t) s], n_goal = D.conn_n[2 * (size_t) s + 1];
            bool c_has = false;  // this thread's connection edge {c_end, c_v}
            uint32_t c_end = 0, c_v = 0;
            float c_w = INFINITY;
            if (both && tid < 2u * kc)
            {
                c_end = tid / kc;
                const uint32_t i = tid % kc;
                if (i < (c_end ? n_goal : n_start) && bit_at(D.q_bits, slot0 + 1 + tid))
                {
                    c_has = true;
                    c_v = 2u + D.conn_id[2 * (size_t) s * kc + tid];
                    c_w = D.conn_w[2 * (size_t) s * kc + tid];
                }
            }
            const uint32_t start_edges = (uint32_t) __syncthreads_count(c_has && c_end == 0u);
            const uint32_t goal_edges = (uint32_t) __syncthreads_count(c_has && c_end == 1u);

            uint32_t *walk = D.walk + (size_t) s * V;
            if (!both)
                r.status = VMV_PLAN_INVALID_ENDPOINT;
            else
            {
                r.start_edges = start_edges, r.goal_edges = goal_edges, r.edges_checked = 1u + n_start + n_goal;
                if (bit_at(D.q_bits, slot0))  // the direct edge comes first
                {
                    const float *me = D.ends + 2 * (size_t) s * P.dim;
                    r.status = VMV_PLAN_SOLVED, r.path_len = 2, r.cost = sqrtf(dist2(me, me + P.dim, P.dim));
                    if (tid == 0u) walk[0] = 1u, walk[1] = 0u;
                }
                else
                {
                    r.iterations = P.n_samples;
                    const uint32_t rm = D.roadmap[s], e_lo = D.edge_offsets[rm], e_hi = D.edge_offsets[rm + 1];
                    for (uint32_t v = tid; v < V; v += kPrmSsspBlock) g[v] = v == 0u ? 0u : kInfBits;
                    __syncthreads();
                    for (uint32_t sweep = 0; sweep < V; ++sweep)
                    {
                        int changed = 0;
                        for (uint32_t e = e_lo + tid; e < e_hi; e += kPrmSsspBlock)
                            if (bit_at(D.ebits, e))
                                changed |= sssp_relax(g, 2u + D.pairs[2 * (size_t) e], 2u + D.pairs[2 * (size_t) e + 1], D.weights[e]);
                        if (c_has) changed |= sssp_relax(g, c_end, c_v, c_w);
                        if (!__syncthreads_or(changed)) break;
                    }
                    if (g[1] < kInfBits)
                    {
                        uint32_t cur = 1u, len = 1u;
                        bool lost = false;
                        if (tid == 0u) walk[0] = 1u;
                        for (uint32_t step = 0; step + 1u < V && cur != 0u; ++step)
                        {
                            const uint32_t gc = g[cur];
                            uint32_t best = kNone;
                            if (cur >= 2u)
                                for (uint32_t e = e_lo + tid; e < e_hi; e += kPrmSsspBlock)
                                {
                                    if (!bit_at(D.ebits, e)) continue;
                                    const uint32_t a = 2u + D.pairs[2 * (size_t) e], b = 2u + D.pairs[2 * (size_t) e + 1];
                                    if (a != cur && b != cur) continue;
                                    const uint32_t u = a == cur ? b : a;
                                    if (u < best && sssp_is_parent(g, gc, u, D.weights[e])) best = u;
                                }
                            if (c_has && (c_end == cur || c_v == cur))
                            {
                                const uint32_t u = c_end == cur ? c_v : c_end;
                                if (u < best && sssp_is_parent(g, gc, u, c_w)) best = u;
                            }
                            if (best != kNone) atomicMin(&s_best, best);
                            __syncthreads();
                            best = s_best;
                            __syncthreads();
                            if (tid == 0u) s_best = kNone;
                            if (best == kNone)  // only where an edge is below half an ulp of g: ends as NO_PATH
                            {
                                lost = true;
                                break;
                            }
                            cur = best;
                            if (tid == 0u) walk[len] = cur;
                            ++len;
                            __syncthreads();
                        }
                        if (!lost && cur == 0u) r.status = VMV_PLAN_SOLVED, r.path_len = len, r.cost = __uint_as_float(g[1]);
                    }
                }
            }
            if (tid == 0u) D.result[s] = r;
        }

        __global__ __launch_bounds__(kPrmBlock) void rm_gather_kernel(const QueryParams P, const QueryArrays D,
                                                                       const uint64_t *__restrict__ offsets, float *__restrict__ paths)
        {
            const uint32_t s = blockIdx.x * kPrmBlock + threadIdx.x;
            if (s >= P.n_queries) return;
            const uint32_t len = D.result[s].path_len <= P.V ? D.result[s].path_len : 0u;
            const uint32_t *walk = D.walk + (size_t) s * P.V;
            const float *verts_r = D.verts + (size_t) D.roadmap[s] * P.n_samples * P.dim;
            float *out = paths + offsets[s] * P.dim;
            for (uint32_t i = 0; i < len; ++i)
            {
                const uint32_t v = walk[len - 1u - i];
                if (v >= P.V) return;
                const float *q = v < 2u ? D.ends + (2 * (size_t) s + v) * P.dim : verts_r + (size_t) (v - 2u) * P.dim;
                for (uint32_t j = 0; j < P.dim; ++j) out[(size_t) i * P.dim + j] = q[j];
            }
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with
        // the robot's part built.
        int roadmaps_build_run(const float *lower, const float *span, const uint64_t *skips, const float *samples,
                               const vmv_roadmap_settings &S, vmv_roadmaps *rm)
        {
            const size_t n = rm->n, ns = S.n_samples, n_cfgs = n * ns;
            const int dim = rm->dim;
            BuildParams P{};
            P.dim = (uint32_t) dim, P.n_samples = S.n_samples, P.k = S.k, P.n_roadmaps = (uint32_t) n;
            P.r2 = S.radius * S.radius;
            const uint32_t n32 = (uint32_t) n;
            hipStream_t stream = nullptr;
            VMV_LOCKSTEP_HIP(hipGetDevice(&rm->device));

            DeviceBuffers tmp;  // what the build alone needs
            BuildArrays D{};
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->verts, n_cfgs * (size_t) dim));
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->vbits, n_cfgs / 64));
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->d_edge_offsets, n + 1));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.skips, n));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.nbr, n_cfgs * S.k));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.counts, n_cfgs + 1));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.first, n_cfgs + 1));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.stats, 2 * n));
            D.verts = rm->verts, D.vbits = rm->vbits, D.edge_offsets = rm->d_edge_offsets;

            // 1. the samples of all roadmaps; one validation call
            if (samples)
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.verts, samples, n_cfgs * (size_t) dim * 4, hipMemcpyHostToDevice, stream));
            else if (int rc = halton_fill(D.verts, D.skips, skips, n, S.n_samples, P.dim, lower, span, stream, "rm_halton_kernel"); rc != VMV_OK)
                return rc;
            {
                std::vector<size_t> seg(n + 1);
                for (size_t r = 0; r <= n; ++r) seg[r] = r * ns;
                if (int rc = vmv_validate_batch_multi(rm->robot, rm->envs.data(), seg.data(), n, D.verts, rm->vbits, stream); rc != VMV_OK)
                {
                    (void) hipDeviceSynchronize();
                    return rc;
                }
            }

            // 2. neighbours
            {
                const uint32_t tiles = (uint32_t) ((ns + kPrmBlock - 1) / kPrmBlock), chunk = kPrmLaunchBlocks / tiles;  // tiles <= 32
                for (uint32_t r0 = 0; r0 < n32; r0 += chunk)
                {
                    const dim3 grid(std::min(chunk, n32 - r0) * tiles);
                    if (dim <= 8)
                        hipLaunchKernelGGL(rm_knn_kernel<8>, grid, dim3(kPrmBlock), 0, stream, P, D, r0, tiles);
                    else
                        hipLaunchKernelGGL(rm_knn_kernel<16>, grid, dim3(kPrmBlock), 0, stream, P, D, r0, tiles);
                    VMV_PRM_LAUNCHED("rm_knn_kernel");
                }
            }

            // 3. candidate edges: counted, scanned, written in the contract's order; one validation call
            const uint32_t sample_blocks = (uint32_t) ((n_cfgs + 1 + kPrmBlock - 1) / kPrmBlock);
            hipLaunchKernelGGL(rm_count_kernel, dim3(sample_blocks), dim3(kPrmBlock), 0, stream, P, D);
            VMV_PRM_LAUNCHED("rm_count_kernel");
            {
                size_t scan_bytes = 0;
                VMV_LOCKSTEP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, D.counts, D.first, (int) (n_cfgs + 1), stream));
                uint8_t *scan_tmp = nullptr;
                VMV_LOCKSTEP_HIP(tmp.alloc(&scan_tmp, scan_bytes));
                VMV_LOCKSTEP_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, D.counts, D.first, (int) (n_cfgs + 1), stream));
            }
            hipLaunchKernelGGL(edge_offsets_kernel, dim3((n32 + 1 + kPrmBlock - 1) / kPrmBlock), dim3(kPrmBlock), 0, stream, D.edge_offsets,
                               D.first, n32, P.n_samples);
            VMV_PRM_LAUNCHED("rm_offsets_kernel");
            rm->edge_offsets.resize(n + 1);
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(rm->edge_offsets.data(), D.edge_offsets, (n + 1) * 4, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));  // the build's one synchronisation before its results
            const size_t E = rm->edge_offsets[n];
            if (E >= kMultiMaxConfigs) return hip_status(hipErrorInvalidValue, "vmv_roadmaps_build: 2^31 candidate edges or more");
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->pairs, 2 * E));
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->weights, E));
            VMV_LOCKSTEP_HIP(rm->mem.alloc(&rm->ebits, (E + 63) / 64));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.q_a, E * (size_t) dim));
            VMV_LOCKSTEP_HIP(tmp.alloc(&D.q_b, E * (size_t) dim));
            D.pairs = rm->pairs, D.weights = rm->weights, D.ebits = rm->ebits;
            if (E > 0)
            {
                hipLaunchKernelGGL(rm_write_kernel, dim3(sample_blocks), dim3(kPrmBlock), 0, stream, P, D);
                VMV_PRM_LAUNCHED("rm_write_kernel");
                std::vector<size_t> seg(rm->edge_offsets.begin(), rm->edge_offsets.end());
                if (int rc = vmv_validate_motion_batch_multi(rm->robot, rm->envs.data(), seg.data(), n, D.q_a, D.q_b, rm->ebits, stream);
                    rc != VMV_OK)
                {
                    (void) hipDeviceSynchronize();
                    return rc;
                }
            }

            // 4. the summary's counts; the copy also ends the build before its temporaries are freed
            hipLaunchKernelGGL(rm_stats_kernel, dim3(n32), dim3(kPrmBlock), 0, stream, P, D);
            VMV_PRM_LAUNCHED("rm_stats_kernel");
            std::vector<uint32_t> stats(2 * n);
            VMV_LOCKSTEP_HIP(hipMemcpy(stats.data(), D.stats, 2 * n * 4, hipMemcpyDeviceToHost));
            rm->valid_vertices.resize(n), rm->valid_edges.resize(n);
            for (size_t r = 0; r < n; ++r) rm->valid_vertices[r] = stats[2 * r], rm->valid_edges[r] = stats[2 * r + 1];
            return VMV_OK;
        }

        // The caller has checked every argument and n > 0.  order[s] = the query at position s (stable counting sort by
        // roadmap); seg_envs / seg_lo: the roadmaps that have queries and their first positions (seg_lo ends with n).
        int roadmaps_query_run(const vmv_roadmaps *rm, size_t n, const std::vector<uint32_t> &order, const std::vector<uint32_t> &roadmap,
                               const std::vector<const vmv_env *> &seg_envs, const std::vector<size_t> &seg_lo, const float *starts,
                               const float *goals, const vmv_roadmap_query_settings &S, vmv_plans *plans)
        {
            const int dim = rm->dim;
            QueryParams P{};
            P.dim = (uint32_t) dim, P.n_samples = rm->n_samples, P.V = rm->n_samples + 2u, P.kc = S.k_connect, P.per = 1u + 2u * S.k_connect;
            P.n_queries = (uint32_t) n, P.r2 = S.radius * S.radius;
            const size_t per = P.per, V = P.V, n_slots = n * per, n_segs = seg_envs.size();
            const uint32_t n32 = (uint32_t) n;
            hipStream_t stream = nullptr;

            DeviceBuffers mem;
            QueryArrays D{};
            float *d_ends = nullptr;
            uint64_t *d_end_bits = nullptr, *d_q_bits = nullptr, *d_path_offsets = nullptr;
            uint32_t *d_roadmap = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_ends, 2 * n * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_end_bits, (2 * n + 63) / 64));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_roadmap, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.conn_id, 2 * n * S.k_connect));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.conn_w, 2 * n * S.k_connect));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.conn_n, 2 * n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.q_a, n_slots * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.q_b, n_slots * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_q_bits, (n_slots + 63) / 64));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.walk, n * V));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.result, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_path_offsets, n));
            D.verts = rm->verts, D.vbits = rm->vbits, D.edge_offsets = rm->d_edge_offsets, D.pairs = rm->pairs, D.weights = rm->weights;
            D.ebits = rm->ebits, D.ends = d_ends, D.end_bits = d_end_bits, D.roadmap = d_roadmap, D.q_bits = d_q_bits;

            // 1. the endpoints by position, one segment per roadmap that has queries; one validation call
            std::vector<float> ends(2 * n * (size_t) dim);
            for (size_t s = 0; s < n; ++s)
            {
                std::memcpy(&ends[(2 * s) * (size_t) dim], starts + order[s] * (size_t) dim, (size_t) dim * 4);
                std::memcpy(&ends[(2 * s + 1) * (size_t) dim], goals + order[s] * (size_t) dim, (size_t) dim * 4);
            }
            VMV_LOCKSTEP_HIP(hipMemcpy(d_ends, ends.data(), ends.size() * 4, hipMemcpyHostToDevice));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_roadmap, roadmap.data(), n * 4, hipMemcpyHostToDevice));
            std::vector<size_t> seg(n_segs + 1);
            for (size_t k = 0; k <= n_segs; ++k) seg[k] = 2 * seg_lo[k];
            if (int rc = vmv_validate_batch_multi(rm->robot, seg_envs.data(), seg.data(), n_segs, d_ends, d_end_bits, stream); rc != VMV_OK)
            {
                (void) hipDeviceSynchronize();
                return rc;
            }

            // 2. connections
            for (uint32_t e0 = 0; e0 < 2u * n32; e0 += kPrmLaunchBlocks)
            {
                const dim3 grid(std::min(kPrmLaunchBlocks, 2u * n32 - e0));
                const size_t lds = (size_t) rm->n_samples * 4;
                if (dim <= 8)
                    hipLaunchKernelGGL(rm_connect_kernel<8>, grid, dim3(kWave), lds, stream, P, D, e0);
                else
                    hipLaunchKernelGGL(rm_connect_kernel<16>, grid, dim3(kWave), lds, stream, P, D, e0);
                VMV_PRM_LAUNCHED("rm_connect_kernel");
            }

            // 3. the questions, a fixed block per query; one validation call
            for (size_t k = 0; k <= n_segs; ++k) seg[k] = per * seg_lo[k];
            if (int rc = vmv_validate_motion_batch_multi(rm->robot, seg_envs.data(), seg.data(), n_segs, D.q_a, D.q_b, d_q_bits, stream);
                rc != VMV_OK)
            {
                (void) hipDeviceSynchronize();
                return rc;
            }

            // 4. shortest paths
            for (uint32_t s0 = 0; s0 < n32; s0 += kPrmLaunchBlocks)
            {
                hipLaunchKernelGGL(rm_query_sssp_kernel, dim3(std::min(kPrmLaunchBlocks, n32 - s0)), dim3(kPrmSsspBlock), 0, stream, P, D, s0);
                VMV_PRM_LAUNCHED("rm_query_sssp_kernel");
            }

            // 5. results: the per-query records back in the caller's order, then the paths gathered on the device
            std::vector<QueryResult> results(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(results.data(), D.result, n * sizeof(QueryResult), hipMemcpyDeviceToHost));
            plans->n = n, plans->dim = dim;
            plans->status.resize(n), plans->iterations.resize(n), plans->sizes2.resize(2 * n), plans->path_lengths.resize(n);
            plans->candidate_edges.resize(n), plans->costs.resize(n);
            uint64_t questions = 0;
            for (size_t s = 0; s < n; ++s)
            {
                const QueryResult &r = results[s];
                const size_t q = order[s];
                plans->status[q] = (uint8_t) r.status;
                plans->iterations[q] = r.iterations;
                plans->sizes2[2 * q] = r.start_edges, plans->sizes2[2 * q + 1] = r.goal_edges;
                plans->path_lengths[q] = r.path_len;
                plans->candidate_edges[q] = r.edges_checked, plans->costs[q] = r.cost;
                questions += r.edges_checked;
            }
            // the edge call is made whatever the endpoints are; one that carried null questions only is not counted
            plans->rounds = questions ? 2 : 1, plans->questions = questions;
            return pack_paths(mem, d_path_offsets, plans->path_lengths, (size_t) dim, order.data(), "rm_gather_kernel",
                              [&](const uint64_t *d_offsets, float *d_paths) {
                                  hipLaunchKernelGGL(rm_gather_kernel, dim3((n32 + kPrmBlock - 1) / kPrmBlock), dim3(kPrmBlock), 0, stream, P, D,
                                                     d_offsets, d_paths);
                              },
                              plans->paths);
        }

        bool on_its_device(const vmv_roadmaps *rm)
        {
            int device = -1;
            return hipGetDevice(&device) == hipSuccess && device == rm->device;
        }
        void expand_bits(const std::vector<uint64_t> &words, size_t first_bit, size_t count, uint8_t *out)
        {
            for (size_t i = 0; i < count; ++i) out[i] = (uint8_t) ((words[(first_bit + i) >> 6] >> ((first_bit + i) & 63)) & 1u);
        }
    }  // namespace
}  // namespace vmv

using vmv::hip_status;

extern "C"
{
    int vmv_roadmaps_build(int robot, const vmv_env *const *envs, size_t n_roadmaps, const uint64_t *halton_skips, const float *samples,
                           const vmv_roadmap_settings *settings, vmv_roadmaps **out)
    {
        // device-free checks first; the environments' own (unfinalized, another device) are those of vmv_env_prepare_multi
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n_roadmaps > 0 && !envs)) return VMV_ERR_INVALID_ARGUMENT;
        if (n_roadmaps >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t r = 0; r < n_roadmaps; ++r)
            if (!envs[r]) return VMV_ERR_INVALID_ARGUMENT;
        const uint32_t ns = settings->n_samples;
        if (ns % 64u != 0u || ns < vmv::kPrmMinSamples || ns > vmv::kPrmMaxSamples) return VMV_ERR_INVALID_ARGUMENT;
        if (settings->k < 1u || settings->k > vmv::kPrmKMax) return VMV_ERR_INVALID_ARGUMENT;
        if (!(settings->radius > 0.f)) return VMV_ERR_INVALID_ARGUMENT;  // NaN as well
        if (!samples && halton_skips)
            for (size_t r = 0; r < n_roadmaps; ++r)
                if (halton_skips[r] > 1000000ull || halton_skips[r] + ns > 1000000ull) return VMV_ERR_INVALID_ARGUMENT;
        if (n_roadmaps * (size_t) ns * (size_t) settings->k >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        const int rc = vmv::lockstep_call(robot, envs, n_roadmaps, dim, out, [&](vmv_roadmaps *rm) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            rm->robot = robot, rm->n = n_roadmaps;
            rm->envs.assign(envs, envs + n_roadmaps);
            return vmv::roadmaps_build_run(lower, span, halton_skips, samples, *settings, rm);
        });
        if (rc == VMV_OK) (*out)->robot = robot, (*out)->n_samples = ns, (*out)->k = settings->k;  // of an empty handle too
        return rc;
    }

    int vmv_roadmaps_query(const vmv_roadmaps *roadmaps, size_t n_queries, const uint32_t *roadmap_of_query, const float *starts,
                           const float *goals, const vmv_roadmap_query_settings *settings, vmv_plans **out)
    {
        if (!roadmaps || !settings || !out || (n_queries > 0 && (!starts || !goals))) return VMV_ERR_INVALID_ARGUMENT;
        if (settings->k_connect < 1u || settings->k_connect > vmv::kConnectMax) return VMV_ERR_INVALID_ARGUMENT;
        if (!(settings->radius > 0.f)) return VMV_ERR_INVALID_ARGUMENT;  // NaN as well
        if (n_queries >= vmv::kMultiMaxConfigs || n_queries * (size_t) (1u + 2u * settings->k_connect) >= vmv::kMultiMaxConfigs)
            return VMV_ERR_INVALID_ARGUMENT;
        const size_t R = roadmaps->n;
        if (n_queries > 0 && R == 0) return VMV_ERR_INVALID_ARGUMENT;  // roadmap 0 does not exist either
        if (roadmap_of_query)
            for (size_t q = 0; q < n_queries; ++q)
                if (roadmap_of_query[q] >= R) return VMV_ERR_INVALID_ARGUMENT;
        if (n_queries > 0 && !vmv::on_its_device(roadmaps)) return VMV_ERR_INVALID_ARGUMENT;

        // the stable counting sort by roadmap: one segment of the validation calls per roadmap that has queries
        std::vector<size_t> first(R + 1, 0);
        for (size_t q = 0; q < n_queries; ++q) ++first[(roadmap_of_query ? roadmap_of_query[q] : 0u) + 1];
        std::vector<const vmv_env *> seg_envs;
        std::vector<size_t> seg_lo;
        for (size_t r = 0; r < R; ++r)
        {
            if (first[r + 1]) seg_envs.push_back(roadmaps->envs[r]), seg_lo.push_back(first[r]);
            first[r + 1] += first[r];
        }
        seg_lo.push_back(n_queries);
        std::vector<uint32_t> order(n_queries), roadmap(n_queries);
        for (size_t q = 0; q < n_queries; ++q)
        {
            const uint32_t r = roadmap_of_query ? roadmap_of_query[q] : 0u;
            roadmap[first[r]] = r, order[first[r]++] = (uint32_t) q;
        }
        const int rc = vmv::lockstep_call(roadmaps->robot, seg_envs.data(), seg_envs.size(), roadmaps->dim, out, [&](vmv_plans *plans) {
            return vmv::roadmaps_query_run(roadmaps, n_queries, order, roadmap, seg_envs, seg_lo, starts, goals, *settings, plans);
        });
        if (rc == VMV_OK) (*out)->query = true;  // an empty result is a query result too
        return rc;
    }

    int vmv_roadmaps_summary(const vmv_roadmaps *roadmaps, uint32_t *valid_vertices, uint32_t *candidate_edges, uint32_t *valid_edges)
    {
        if (!roadmaps) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t r = 0; r < roadmaps->n; ++r)
        {
            if (valid_vertices) valid_vertices[r] = roadmaps->valid_vertices[r];
            if (candidate_edges) candidate_edges[r] = roadmaps->edge_offsets[r + 1] - roadmaps->edge_offsets[r];
            if (valid_edges) valid_edges[r] = roadmaps->valid_edges[r];
        }
        return VMV_OK;
    }

    int vmv_roadmaps_vertices(const vmv_roadmaps *roadmaps, size_t r, float *samples, uint8_t *valid)
    {
        if (!roadmaps || r >= roadmaps->n || !vmv::on_its_device(roadmaps)) return VMV_ERR_INVALID_ARGUMENT;
        const size_t ns = roadmaps->n_samples, dim = (size_t) roadmaps->dim;
        if (samples) VMV_LOCKSTEP_HIP(hipMemcpy(samples, roadmaps->verts + r * ns * dim, ns * dim * 4, hipMemcpyDeviceToHost));
        if (valid)
        {
            std::vector<uint64_t> words(ns / 64);
            VMV_LOCKSTEP_HIP(hipMemcpy(words.data(), roadmaps->vbits + r * ns / 64, words.size() * 8, hipMemcpyDeviceToHost));
            vmv::expand_bits(words, 0, ns, valid);
        }
        return VMV_OK;
    }

    int vmv_roadmaps_edges(const vmv_roadmaps *roadmaps, size_t r, uint32_t *pairs2, uint8_t *valid, size_t capacity, size_t *n)
    {
        if (!roadmaps || r >= roadmaps->n) return VMV_ERR_INVALID_ARGUMENT;
        const size_t lo = roadmaps->edge_offsets[r], count = roadmaps->edge_offsets[r + 1] - lo;
        if (n) *n = count;
        if ((pairs2 || valid) && capacity < count) return VMV_ERR_CAPACITY;
        if (!count || !(pairs2 || valid)) return VMV_OK;
        if (!vmv::on_its_device(roadmaps)) return VMV_ERR_INVALID_ARGUMENT;
        if (pairs2) VMV_LOCKSTEP_HIP(hipMemcpy(pairs2, roadmaps->pairs + 2 * lo, 2 * count * 4, hipMemcpyDeviceToHost));
        if (valid)
        {
            const size_t w0 = lo / 64, w1 = (lo + count + 63) / 64;
            std::vector<uint64_t> words(w1 - w0);
            VMV_LOCKSTEP_HIP(hipMemcpy(words.data(), roadmaps->ebits + w0, words.size() * 8, hipMemcpyDeviceToHost));
            vmv::expand_bits(words, lo - 64 * w0, count, valid);
        }
        return VMV_OK;
    }

    int vmv_roadmaps_destroy(vmv_roadmaps *roadmaps)
    {
        if (!roadmaps) return VMV_ERR_INVALID_ARGUMENT;
        delete roadmaps;
        return VMV_OK;
    }

    int vmv_plans_query_summary(const vmv_plans *plans, float *costs, uint32_t *edges_checked)
    {
        if (!plans || !plans->query) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t q = 0; q < plans->n; ++q)
        {
            if (costs) costs[q] = plans->costs[q];
            if (edges_checked) edges_checked[q] = plans->candidate_edges[q];
        }
        return VMV_OK;
    }
}
