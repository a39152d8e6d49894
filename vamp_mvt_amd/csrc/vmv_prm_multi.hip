// vmv_prm_multi.hip — a batched PRM over many independent problems (vmv_prm_multi).
//
// A fixed sequence of launches, whatever the problems are: the vertices (Halton samples or the caller's) and ONE
// vmv_validate_batch_multi call; prm_knn_kernel (the k nearest valid vertices of every valid vertex); the candidate
// edges counted, scanned and written in the contract's order and ONE vmv_validate_motion_batch_multi call;
// prm_sssp_kernel (one workgroup per problem: the fp32 shortest-path fixpoint and the parent walk); the paths gathered
// into the packed vmv_plans buffers.  The host synchronises once in between, for the per-problem edge counts the edge
// call's offsets need.
//
// Arithmetic contract: fp32, one rounding per written operation (-ffp-contract=off; sqrtf is correctly rounded on
// gfx950).  d2(v, u) = the sum over the joints in order of (v[j] - u[j])^2, so d2(v, u) == d2(u, v) bit for bit;
// neighbours are ordered by (d2, vertex id), a total order, so any parallel selection gives the same lists.  Joints
// beyond the robot's are staged as zeros: adding +0 to a non-negative or non-finite sum changes no bit.
// Vertex memory (vertex_at of vmv_prm_common.h, where stage 1, the Halton fill, the offsets kernel and the walk gather
// live too, shared with vmv_fcit_multi and vmv_roadmaps_*): the samples of all problems [P][n_samples][dim], then
// (start, goal) of all problems [P][2][dim]; a
// problem's samples own whole validity words (n_samples is a multiple of 64).  The P endpoint segments of two
// configurations each SHARE validity words: correctness there rests on vmv_validate_batch_multi's flat layout, which zeroes
// the words of a call with such segments and ORs / ANDs each segment's bits in atomically.
// Plain vector stores; atomics on LDS words only.  Every loop has a bound that holds whatever the data says.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"
#include "vmv_prm_common.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

namespace vmv
{
    namespace
    {
        struct PrmParams
        {
            uint32_t dim, n_samples, V, k, n_problems;
            float r2;
        };

        struct PrmResult  // 32 bytes per problem
        {
            uint32_t status, path_len, iterations, valid_vertices, candidate_edges, valid_edges;
            float cost;
            uint32_t pad;
        };

        struct PrmArrays
        {
            float *verts;             // [P * n_samples + 2 * P][dim]
            const uint64_t *vbits;    // validity of the vertices, in that order
            uint64_t *skips;          // [P] the Halton skips stage 1 samples after
            uint32_t *nbr;            // [P][V][k] neighbour lists, kNone after the last
            uint32_t *counts;         // [P * V + 1] candidate edges owned by (problem, vertex), the last 0
            uint32_t *first;          // [P * V + 1] their exclusive scan: first edge of (problem, vertex), the last the total
            uint32_t *edge_offsets;   // [P + 1] first edge of each problem
            uint32_t *pairs;          // [E][2] vertex ids a < b of edge e
            float *weights;           // [E]
            float *q_a, *q_b;         // [E][dim] the edge questions
            const uint64_t *ebits;    // their answers
            uint32_t *walk;           // [P][V] the path's vertex ids from the goal backwards
            PrmResult *result;        // [P]
        };

        // One lane per query vertex, a workgroup within one problem (problem p0 + blockIdx.x / tiles, tile blockIdx.x % tiles).  The candidates go through LDS a tile
        // of kPrmBlock at a time: every lane reads the same candidate (a broadcast read) and its validity flag is the
        // same in the whole wave.  The k best sit in the register list of vmv_prm_common.h.
        template <int DIM>
        __global__ __launch_bounds__(kPrmBlock) void prm_knn_kernel(const PrmParams P, const PrmArrays D, const uint32_t p0, const uint32_t tiles)
        {
            __shared__ __align__(16) float s_tile[kPrmBlock * DIM];
            __shared__ uint32_t s_valid[kPrmBlock];
            const uint32_t p = p0 + blockIdx.x / tiles, tid = threadIdx.x, v = (blockIdx.x % tiles) * kPrmBlock + tid, V = P.V, dim = P.dim;
            if (!ends_valid(P, D.vbits, p)) return;  // workgroup-uniform: INVALID_ENDPOINT asks nothing (the lists are not read)
            const bool query = v < V && bit_at(D.vbits, vertex_at(P, p, v));
            float q[DIM];
#pragma unroll
            for (int j = 0; j < DIM; ++j) q[j] = (query && (uint32_t) j < dim) ? D.verts[vertex_at(P, p, v) * dim + j] : 0.f;
            uint32_t bk[kPrmKMax], bi[kPrmKMax];
            knn_list_init(bk, bi, P.k);
            const uint32_t r2_bits = __float_as_uint(P.r2);

            for (uint32_t base = 0; base < V; base += kPrmBlock)  // <= ceil(V / kPrmBlock) tiles
            {
                const uint32_t u_mine = base + tid;
                const bool ok = u_mine < V && bit_at(D.vbits, vertex_at(P, p, u_mine));
                s_valid[tid] = ok ? 1u : 0u;
#pragma unroll
                for (int j = 0; j < DIM; ++j)
                    s_tile[tid * DIM + j] = (ok && (uint32_t) j < dim) ? D.verts[vertex_at(P, p, u_mine) * dim + j] : 0.f;
                __syncthreads();
                const uint32_t count = V - base < kPrmBlock ? V - base : kPrmBlock;
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
                        const uint32_t key = __float_as_uint(sum);  // valid vertices are finite: sum is in [+0, +inf]
                        if (!(key < bk[kPrmKMax - 1])) continue;
                        if (key == 0u || key > r2_bits || u == v || (u < 2u && v < 2u)) continue;
                        knn_list_insert(bk, bi, key, u);
                    }
                __syncthreads();  // the tile is rewritten
            }
            if (v < V)
            {
                uint32_t *out = D.nbr + ((size_t) p * V + v) * P.k;
#pragma unroll
                for (uint32_t s = 0; s < kPrmKMax; ++s)
                    if (s >= kPrmKMax - P.k) out[s - (kPrmKMax - P.k)] = bi[s];
            }
        }

        // counts[p * V + v] = the candidate edges vertex v of problem p contributes (vertex 0: the edge (0, 1) as well);
        // counts[P * V] = 0, so that the exclusive scan ends with the total
        __global__ __launch_bounds__(kPrmBlock) void prm_count_kernel(const PrmParams P, const PrmArrays D)
        {
            const size_t total = (size_t) P.n_problems * P.V;
            const size_t i = (size_t) blockIdx.x * kPrmBlock + threadIdx.x;
            if (i > total) return;
            uint32_t n = 0;
            if (i < total)
            {
                const uint32_t p = (uint32_t) (i / P.V), v = (uint32_t) (i % P.V);
                if (ends_valid(P, D.vbits, p) && bit_at(D.vbits, vertex_at(P, p, v)))
                {
                    const uint32_t *nbr_p = D.nbr + (size_t) p * P.V * P.k;
                    n = v == 0u ? 1u : 0u;
                    for (uint32_t s = 0; s < P.k; ++s)
                    {
                        const uint32_t u = nbr_p[(size_t) v * P.k + s];
                        if (u >= P.V) break;  // kNone: the list ended
                        n += owns(nbr_p, P.k, v, u) ? 1u : 0u;
                    }
                }
            }
            D.counts[i] = n;
        }

        // the edges of (p, v) start at first[p * V + v], in slot order
        __global__ __launch_bounds__(kPrmBlock) void prm_write_kernel(const PrmParams P, const PrmArrays D)
        {
            const size_t total = (size_t) P.n_problems * P.V;
            const size_t i = (size_t) blockIdx.x * kPrmBlock + threadIdx.x;
            if (i >= total) return;
            uint32_t e = D.first[i];
            const uint32_t end = D.first[i + 1];
            if (e == end) return;
            const uint32_t p = (uint32_t) (i / P.V), v = (uint32_t) (i % P.V), dim = P.dim;
            const uint32_t *nbr_p = D.nbr + (size_t) p * P.V * P.k;
            const auto emit = [&](uint32_t a, uint32_t b) {
                const float *qa = D.verts + vertex_at(P, p, a) * dim, *qb = D.verts + vertex_at(P, p, b) * dim;
                D.pairs[2 * (size_t) e] = a, D.pairs[2 * (size_t) e + 1] = b;
                D.weights[e] = sqrtf(dist2(qa, qb, dim));
                for (uint32_t j = 0; j < dim; ++j) D.q_a[(size_t) e * dim + j] = qa[j], D.q_b[(size_t) e * dim + j] = qb[j];
                ++e;
            };
            if (v == 0u) emit(0u, 1u);
            for (uint32_t s = 0; s < P.k && e < end; ++s)
            {
                const uint32_t u = nbr_p[(size_t) v * P.k + s];
                if (u >= P.V) break;
                if (owns(nbr_p, P.k, v, u)) emit(v < u ? v : u, v < u ? u : v);
            }
        }

        // One workgroup per problem.  g lives in LDS; sweeps of sssp_relax over the valid edges reach the least fixpoint
        // whatever the order of the relaxations, and V sweeps bound it.
        // Then the parent walk from the goal: per step the lowest id u with a valid
        // edge {u, cur}, fl(g[u] + w) == g[cur] and g[u] < g[cur] (a workgroup min-reduction), at most V steps.
        __global__ __launch_bounds__(kPrmSsspBlock) void prm_sssp_kernel(const PrmParams P, const PrmArrays D, const uint32_t p0)
        {
            __shared__ uint32_t g[kPrmMaxVertices];
            __shared__ uint32_t s_count[2], s_best;
            const uint32_t p = p0 + blockIdx.x, tid = threadIdx.x, V = P.V;
            PrmResult r{};
            r.status = VMV_PLAN_NO_PATH, r.cost = INFINITY;
            if (tid < 2u) s_count[tid] = 0u;
            if (tid == 0u) s_best = kNone;
            for (uint32_t v = tid; v < V; v += kPrmSsspBlock) g[v] = kInfBits;
            __syncthreads();
            uint32_t mine = 0;
            for (uint32_t v = tid; v < V; v += kPrmSsspBlock) mine += bit_at(D.vbits, vertex_at(P, p, v)) ? 1u : 0u;
            if (mine) atomicAdd(&s_count[0], mine);
            const uint32_t e0 = D.edge_offsets[p], e1 = D.edge_offsets[p + 1];
            mine = 0;
            for (uint32_t e = e0 + tid; e < e1; e += kPrmSsspBlock) mine += bit_at(D.ebits, e) ? 1u : 0u;
            if (mine) atomicAdd(&s_count[1], mine);
            if (tid == 0u) g[0] = 0u;
            __syncthreads();
            r.valid_vertices = s_count[0], r.valid_edges = s_count[1], r.candidate_edges = e1 - e0;

            uint32_t *walk = D.walk + (size_t) p * V;
            if (!ends_valid(P, D.vbits, p))
                r.status = VMV_PLAN_INVALID_ENDPOINT;
            else if (e1 > e0 && bit_at(D.ebits, e0))  // the edge (0, 1) comes first
            {
                r.status = VMV_PLAN_SOLVED, r.path_len = 2, r.cost = D.weights[e0];
                if (tid == 0u) walk[0] = 1u, walk[1] = 0u;
            }
            else
            {
                r.iterations = P.n_samples;
                for (uint32_t sweep = 0; sweep < V; ++sweep)
                {
                    int changed = 0;
                    for (uint32_t e = e0 + tid; e < e1; e += kPrmSsspBlock)
                    {
                        if (!bit_at(D.ebits, e)) continue;
                        changed |= sssp_relax(g, D.pairs[2 * (size_t) e], D.pairs[2 * (size_t) e + 1], D.weights[e]);  // an overflowed d2 relaxes nothing
                    }
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
                        for (uint32_t e = e0 + tid; e < e1; e += kPrmSsspBlock)
                        {
                            if (!bit_at(D.ebits, e)) continue;
                            const uint32_t a = D.pairs[2 * (size_t) e], b = D.pairs[2 * (size_t) e + 1];
                            if (a != cur && b != cur) continue;
                            const uint32_t u = a == cur ? b : a;
                            if (u < best && sssp_is_parent(g, gc, u, D.weights[e])) best = u;
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
            if (tid == 0u) D.result[p] = r;
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with
        // the robot's part built.
        int prm_multi_run(int robot, int dim, const float *lower, const float *span, const vmv_env *const *envs, size_t n,
                          const float *starts, const float *goals, const uint64_t *skips, const float *samples,
                          const vmv_prm_settings &S, vmv_plans *plans)
        {
            PrmParams P{};
            P.dim = (uint32_t) dim, P.n_samples = S.n_samples, P.V = S.n_samples + 2u, P.k = S.k, P.n_problems = (uint32_t) n;
            P.r2 = S.radius * S.radius;
            const size_t ns = S.n_samples, V = P.V, n_sample_cfgs = n * ns, n_cfgs = n_sample_cfgs + 2 * n, nv = n * V;
            const uint32_t n32 = (uint32_t) n;
            hipStream_t stream = nullptr;

            DeviceBuffers mem;
            PrmArrays D{};
            uint64_t *d_vbits = nullptr, *d_ebits = nullptr, *d_path_offsets = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&D.verts, n_cfgs * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_vbits, (n_cfgs + 63) / 64));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.skips, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.nbr, nv * S.k));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.counts, nv + 1));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.first, nv + 1));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.edge_offsets, n + 1));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.walk, nv));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.result, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_path_offsets, n));
            D.vbits = d_vbits;

            // 1. vertices: the samples of all problems, then (start, goal) of all problems; one validation call
            if (int rc = prm_stage_vertices(robot, envs, n, S.n_samples, P.dim, starts, goals, skips, samples, lower, span, D.verts, D.skips,
                                            d_vbits, stream, "prm_halton_kernel");
                rc != VMV_OK)
                return rc;
            uint64_t validation_calls = 1;

            // 2. neighbours
            {
                const uint32_t tiles = (uint32_t) ((V + kPrmBlock - 1) / kPrmBlock), chunk = kPrmLaunchBlocks / tiles;  // tiles <= 32
                for (uint32_t p0 = 0; p0 < n32; p0 += chunk)
                {
                    const dim3 grid(std::min(chunk, n32 - p0) * tiles);
                    if (dim <= 8)
                        hipLaunchKernelGGL(prm_knn_kernel<8>, grid, dim3(kPrmBlock), 0, stream, P, D, p0, tiles);
                    else
                        hipLaunchKernelGGL(prm_knn_kernel<16>, grid, dim3(kPrmBlock), 0, stream, P, D, p0, tiles);
                    VMV_PRM_LAUNCHED("prm_knn_kernel");
                }
            }

            // 3. candidate edges: counted, scanned, written in the contract's order; one validation call
            const uint32_t vertex_blocks = (uint32_t) ((nv + 1 + kPrmBlock - 1) / kPrmBlock);
            hipLaunchKernelGGL(prm_count_kernel, dim3(vertex_blocks), dim3(kPrmBlock), 0, stream, P, D);
            VMV_PRM_LAUNCHED("prm_count_kernel");
            {
                size_t scan_bytes = 0;
                VMV_LOCKSTEP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, D.counts, D.first, (int) (nv + 1), stream));
                uint8_t *scan_tmp = nullptr;
                VMV_LOCKSTEP_HIP(mem.alloc(&scan_tmp, scan_bytes));
                VMV_LOCKSTEP_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, D.counts, D.first, (int) (nv + 1), stream));
            }
            hipLaunchKernelGGL(edge_offsets_kernel, dim3((n32 + 1 + kPrmBlock - 1) / kPrmBlock), dim3(kPrmBlock), 0, stream, D.edge_offsets,
                               D.first, n32, P.V);
            VMV_PRM_LAUNCHED("prm_offsets_kernel");
            std::vector<uint32_t> edge_offsets(n + 1);
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(edge_offsets.data(), D.edge_offsets, (n + 1) * 4, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));  // the call's one synchronisation before its results
            const size_t E = edge_offsets[n];
            if (E >= kMultiMaxConfigs) return hip_status(hipErrorInvalidValue, "vmv_prm_multi: 2^31 candidate edges or more");
            VMV_LOCKSTEP_HIP(mem.alloc(&D.pairs, 2 * E));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.weights, E));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.q_a, E * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.q_b, E * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_ebits, (E + 63) / 64));
            D.ebits = d_ebits;
            if (E > 0)
            {
                hipLaunchKernelGGL(prm_write_kernel, dim3(vertex_blocks), dim3(kPrmBlock), 0, stream, P, D);
                VMV_PRM_LAUNCHED("prm_write_kernel");
                std::vector<size_t> seg(edge_offsets.begin(), edge_offsets.end());
                if (int rc = vmv_validate_motion_batch_multi(robot, envs, seg.data(), n, D.q_a, D.q_b, d_ebits, stream); rc != VMV_OK)
                {
                    (void) hipDeviceSynchronize();
                    return rc;
                }
                ++validation_calls;
            }

            // 4. shortest paths
            for (uint32_t p0 = 0; p0 < n32; p0 += kPrmLaunchBlocks)
            {
                hipLaunchKernelGGL(prm_sssp_kernel, dim3(std::min(kPrmLaunchBlocks, n32 - p0)), dim3(kPrmSsspBlock), 0, stream, P, D, p0);
                VMV_PRM_LAUNCHED("prm_sssp_kernel");
            }

            // 5. results: the per-problem records, then the paths gathered on the device into one packed buffer
            std::vector<PrmResult> results(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(results.data(), D.result, n * sizeof(PrmResult), hipMemcpyDeviceToHost));
            plans->n = n, plans->dim = dim, plans->rounds = validation_calls, plans->questions = E;
            plans->prm = true, plans->n_samples = S.n_samples;
            plans->status.resize(n), plans->iterations.resize(n), plans->sizes2.resize(2 * n), plans->path_lengths.resize(n);
            plans->candidate_edges.resize(n), plans->costs.resize(n);
            for (size_t p = 0; p < n; ++p)
            {
                const PrmResult &r = results[p];
                plans->status[p] = (uint8_t) r.status;
                plans->iterations[p] = r.iterations;
                plans->sizes2[2 * p] = r.valid_vertices, plans->sizes2[2 * p + 1] = r.valid_edges;
                plans->path_lengths[p] = r.path_len;
                plans->candidate_edges[p] = r.candidate_edges, plans->costs[p] = r.cost;
            }
            if (int rc = pack_paths(mem, d_path_offsets, plans->path_lengths, (size_t) dim, nullptr, "prm_gather_kernel",
                                    [&](const uint64_t *d_offsets, float *d_paths) {
                                        hipLaunchKernelGGL(walk_gather_kernel, dim3((n32 + kPrmBlock - 1) / kPrmBlock), dim3(kPrmBlock), 0, stream,
                                                           PrmLayout{P.dim, P.n_samples, P.n_problems}, D.verts, D.walk, &D.result->path_len,
                                                           (uint32_t) (sizeof(PrmResult) / 4), true, d_offsets, d_paths);
                                    },
                                    plans->paths);
                rc != VMV_OK)
                return rc;
            if (S.keep_roadmaps)
            {
                std::vector<uint64_t> vbits((n_cfgs + 63) / 64), ebits((E + 63) / 64);
                VMV_LOCKSTEP_HIP(hipMemcpy(vbits.data(), d_vbits, vbits.size() * 8, hipMemcpyDeviceToHost));
                const auto bit = [](const std::vector<uint64_t> &w, size_t i) { return (uint8_t) ((w[i >> 6] >> (i & 63)) & 1u); };
                plans->vertex_valid.resize(nv);
                for (size_t p = 0; p < n; ++p)
                    for (size_t v = 0; v < V; ++v)
                        plans->vertex_valid[p * V + v] = bit(vbits, v < 2 ? n_sample_cfgs + 2 * p + v : p * ns + (v - 2));
                plans->edge_offsets.assign(edge_offsets.begin(), edge_offsets.end());
                plans->edge_pairs.resize(2 * E), plans->edge_valid.resize(E);
                if (E)
                {
                    VMV_LOCKSTEP_HIP(hipMemcpy(ebits.data(), d_ebits, ebits.size() * 8, hipMemcpyDeviceToHost));
                    VMV_LOCKSTEP_HIP(hipMemcpy(plans->edge_pairs.data(), D.pairs, 2 * E * 4, hipMemcpyDeviceToHost));
                    for (size_t e = 0; e < E; ++e) plans->edge_valid[e] = bit(ebits, e);
                }
                plans->kept = true;
            }
            return VMV_OK;
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_prm_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                      const uint64_t *halton_skips, const float *samples, const vmv_prm_settings *settings, vmv_plans **out)
    {
        // device-free checks first; the environments' own (NULL handles again, unfinalized, another device) are those of
        // vmv_env_prepare_multi, which then builds the parts not yet built in one batch
        int dim = 0;
        if (int rc = vmv::check_planner_call(robot, settings, out, envs, n_problems, starts, goals, &dim); rc != VMV_OK) return rc;
        const uint32_t ns = settings->n_samples;
        if (ns % 64u != 0u || ns < vmv::kPrmMinSamples || ns > vmv::kPrmMaxSamples) return VMV_ERR_INVALID_ARGUMENT;
        if (settings->k < 1u || settings->k > vmv::kPrmKMax) return VMV_ERR_INVALID_ARGUMENT;
        if (!(settings->radius > 0.f)) return VMV_ERR_INVALID_ARGUMENT;  // NaN as well
        if (!samples && !vmv::halton_skips_ok(halton_skips, n_problems, ns)) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems * (size_t) (ns + 2u) * (size_t) settings->k >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems == 0)  // an empty result is a PRM result too
        {
            vmv_plans *plans = new (std::nothrow) vmv_plans;
            if (!plans) return VMV_ERR_HIP;
            plans->dim = dim, plans->prm = true, plans->n_samples = ns, plans->kept = settings->keep_roadmaps != 0;
            plans->edge_offsets.assign(1, 0u);
            *out = plans;
            return VMV_OK;
        }
        return vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            return vmv::prm_multi_run(robot, dim, lower, span, envs, n_problems, starts, goals, halton_skips, samples, *settings,
                                      plans);
        });
    }

    int vmv_plans_roadmap_summary(const vmv_plans *plans, uint32_t *valid_vertices, uint32_t *candidate_edges, uint32_t *valid_edges,
                                  float *costs)
    {
        if (!plans || !plans->prm) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t p = 0; p < plans->n; ++p)
        {
            if (valid_vertices) valid_vertices[p] = plans->sizes2[2 * p];
            if (candidate_edges) candidate_edges[p] = plans->candidate_edges[p];
            if (valid_edges) valid_edges[p] = plans->sizes2[2 * p + 1];
            if (costs) costs[p] = plans->costs[p];
        }
        return VMV_OK;
    }

    int vmv_plans_roadmap_vertices(const vmv_plans *plans, size_t p, uint8_t *valid)
    {
        if (!plans || !plans->prm || !plans->kept || p >= plans->n || !valid) return VMV_ERR_INVALID_ARGUMENT;
        const size_t V = (size_t) plans->n_samples + 2;
        std::memcpy(valid, plans->vertex_valid.data() + p * V, V);
        return VMV_OK;
    }

    int vmv_plans_roadmap_edges(const vmv_plans *plans, size_t p, uint32_t *pairs2, uint8_t *valid, size_t capacity, size_t *n)
    {
        if (!plans || !plans->prm || !plans->kept || p >= plans->n) return VMV_ERR_INVALID_ARGUMENT;
        const size_t lo = plans->edge_offsets[p], count = plans->edge_offsets[p + 1] - lo;
        if (n) *n = count;
        if ((pairs2 || valid) && capacity < count) return VMV_ERR_CAPACITY;
        if (pairs2 && count) std::memcpy(pairs2, plans->edge_pairs.data() + 2 * lo, 2 * count * 4);
        if (valid && count) std::memcpy(valid, plans->edge_valid.data() + lo, count);
        return VMV_OK;
    }
}
