// vmv_two_trees.h — the device side the two-tree planners share (vmv_rrtc_multi; vmv_aorrtc_multi, §5f): one
// pool of max_samples nodes per problem with the start tree from the front and the goal tree from the back, the
// workgroup's nearest-node search, the path trace and the steps of the two step kernels that are the same arithmetic.
//
// Contracts kept here: fp32, one rounding per written operation, sums over joints sequential in joint order; nearest()
// gives the FIRST index with the least key; trace_path() writes root(start tree) .. root(goal tree) whichever side is A.
// Everything has internal linkage: each translation unit compiles its own copy into its own step kernel.
#pragma once

#include "vmv_lockstep.h"

#include <cmath>

namespace vmv
{
    namespace
    {
        constexpr uint32_t kTreeBlock = 256;  // threads of a step kernel's workgroup
        constexpr uint32_t kTreeWaves = kTreeBlock / kWave;
        // the _constrained planners: what a step kernel stores in pending[a] where its question's far end is no new node
        // (else the node's pool element over all problems, p * max_samples + node_at(...)); constraint_round_kernel reads it
        constexpr uint64_t kNoPending = ~0ull;

        __device__ __forceinline__ size_t node_at(uint32_t side, uint32_t i, uint32_t max_samples)
        {
            return side ? (size_t) (max_samples - 1u - i) : (size_t) i;
        }

        // nodes of one side's tree; constant subscripts only, so that the state stays in registers
        __device__ __forceinline__ uint32_t count_of(const uint32_t (&n)[2], uint32_t side) { return side ? n[1] : n[0]; }
        __device__ __forceinline__ uint32_t grow(uint32_t (&n)[2], uint32_t side)  // -> index of the node now counted
        {
            const uint32_t i = count_of(n, side);
            if (side)
                n[1] = i + 1u;
            else
                n[0] = i + 1u;
            return i;
        }

        __device__ __forceinline__ float tree_dist(const float *a, const float *b, uint32_t dim)
        {
            float sum = 0.f;
            for (uint32_t j = 0; j < dim; ++j)
            {
                const float df = a[j] - b[j];
                sum = sum + df * df;
            }
            return sqrtf(sum);
        }

        __device__ __forceinline__ bool closer(float k, uint32_t i, float best_k, uint32_t best_i)
        {
            return k < best_k || (k == best_k && i < best_i);
        }

        struct Scored  // what a caller's functor makes of one node
        {
            bool admissible;
            float key, d;
        };

        // (first index with the least key among the admissible nodes, that node's distance) over nodes [0, count) of one
        // tree; the same values in every thread.  score(node pointer, pool index) -> Scored.  Called by all threads of
        // the workgroup (barriers, cross-lane reads with every lane enabled).  kNone where no key compares below +inf.
        // kKeyed = false: the key IS the distance, and nothing but (key, index) is carried: s_rd is not touched.
        template <bool kKeyed, typename Score>
        __device__ void nearest(const float *__restrict__ pool, const uint32_t side, const uint32_t count, const uint32_t dim,
                                const uint32_t max_samples, Score &&score, float *s_rk, float *s_rd, uint32_t *s_ri, float &out_d,
                                uint32_t &out_i)
        {
            float best_k = INFINITY, best_d = NAN;
            uint32_t best_i = kNone;
            for (uint32_t i = threadIdx.x; i < count; i += kTreeBlock)  // increasing i per lane: `<` keeps the first
            {
                const size_t at = node_at(side, i, max_samples);
                const Scored s = score(pool + at * dim, at);
                if (s.admissible && s.key < best_k) best_k = s.key, best_d = s.d, best_i = i;
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1)  // (all 64 lanes are enabled here: the loop above has ended)
            {
                const float ok = __shfl_xor(best_k, off);
                const uint32_t oi = (uint32_t) __shfl_xor((int) best_i, off);
                float od = NAN;
                if constexpr (kKeyed) od = __shfl_xor(best_d, off);
                if (closer(ok, oi, best_k, best_i)) best_k = ok, best_d = od, best_i = oi;
            }
            if ((threadIdx.x & (kWave - 1)) == 0)
            {
                s_rk[threadIdx.x / kWave] = best_k, s_ri[threadIdx.x / kWave] = best_i;
                if constexpr (kKeyed) s_rd[threadIdx.x / kWave] = best_d;
            }
            __syncthreads();
            best_k = s_rk[0], best_i = s_ri[0];
            if constexpr (kKeyed) best_d = s_rd[0];
#pragma unroll
            for (uint32_t w = 1; w < kTreeWaves; ++w)
                if (closer(s_rk[w], s_ri[w], best_k, best_i))
                {
                    best_k = s_rk[w], best_i = s_ri[w];
                    if constexpr (kKeyed) best_d = s_rd[w];
                }
            __syncthreads();  // s_rk / s_rd / s_ri and the caller's target may be rewritten after this
            out_d = kKeyed ? best_d : best_k, out_i = best_i;
        }

        // waypoints of a solved problem: root(A) .. new, then B_prev .. root(B) without its first node if that equals
        // `new` bit for bit; written start tree first (reversed where A is the goal tree).  One thread.
        // out == nullptr: count only.
        __device__ uint32_t trace_path(const uint32_t a_side, const uint32_t new_i, const uint32_t prev, const float *pool,
                                       const uint32_t *parent, const uint32_t dim, const uint32_t M, float *out)
        {
            const uint32_t sa = a_side, sb = sa ^ 1u;
            uint32_t la = 1, lb = 1;
            for (uint32_t i = new_i; parent[node_at(sa, i, M)] != i; i = parent[node_at(sa, i, M)]) ++la;
            for (uint32_t i = prev; parent[node_at(sb, i, M)] != i; i = parent[node_at(sb, i, M)]) ++lb;
            const uint32_t *pn = reinterpret_cast<const uint32_t *>(pool + node_at(sa, new_i, M) * dim);
            const uint32_t *pp = reinterpret_cast<const uint32_t *>(pool + node_at(sb, prev, M) * dim);
            bool same = true;
            for (uint32_t j = 0; j < dim; ++j) same = same && pn[j] == pp[j];
            const uint32_t skip = same ? 1u : 0u, len = la + lb - skip;
            if (!out) return len;
            const bool reversed = sa != 0;  // A is the goal tree: the path was collected goal -> start
            uint32_t pos = la;              // A's branch is written backwards from position la - 1
            for (uint32_t i = new_i;; i = parent[node_at(sa, i, M)])
            {
                --pos;
                const float *q = pool + node_at(sa, i, M) * dim;
                float *o = out + (size_t) (reversed ? len - 1u - pos : pos) * dim;
                for (uint32_t j = 0; j < dim; ++j) o[j] = q[j];
                if (parent[node_at(sa, i, M)] == i) break;
            }
            pos = la;
            uint32_t seen = 0;
            for (uint32_t i = prev;; i = parent[node_at(sb, i, M)], ++seen)
            {
                if (seen >= skip)
                {
                    const float *q = pool + node_at(sb, i, M) * dim;
                    float *o = out + (size_t) (reversed ? len - 1u - pos : pos) * dim;
                    for (uint32_t j = 0; j < dim; ++j) o[j] = q[j];
                    ++pos;
                }
                if (parent[node_at(sb, i, M)] == i) break;
            }
            return len;
        }

        // fresh trees: start and goal as the roots of side 0 and side 1, each its own parent; one thread
        __device__ __forceinline__ void init_roots(float *pool, uint32_t *parent, const float *start, const float *goal, uint32_t dim,
                                                   uint32_t M)
        {
            for (uint32_t j = 0; j < dim; ++j)
            {
                pool[node_at(0, 0, M) * dim + j] = start[j];
                pool[node_at(1, 0, M) * dim + j] = goal[j];
            }
            parent[node_at(0, 0, M)] = 0;
            parent[node_at(1, 0, M)] = 0;
        }

        // the side an iteration calls A, after the planner's balance rule
        __device__ __forceinline__ uint32_t next_a_side(const uint32_t (&n)[2], uint32_t a_side, uint32_t balance, float tree_ratio)
        {
            const float na = (float) count_of(n, a_side), nb = (float) count_of(n, a_side ^ 1u);
            return (!balance || fabsf(na - nb) / na < tree_ratio) ? a_side ^ 1u : a_side;
        }

        // steps of a connect march over the distance bd
        __device__ __forceinline__ uint32_t march_steps(float bd, float R)
        {
            const float c = ceilf(bd / R);
            return (c >= 1.f && c < 2147483648.f) ? (uint32_t) c : 1u;
        }

        // new = near + (t - near) * (min(d, R) / d) into A's next slot `next_at`, asked as near -> new; one joint per thread
        __device__ __forceinline__ void ask_extension(float *pool, size_t near_at, size_t next_at, uint32_t dim, const float *s_t, float d,
                                                      float R, float *qs, float *qg)
        {
            const float s = fminf(d, R) / d;
            if (threadIdx.x < dim)
            {
                const float near = pool[near_at * dim + threadIdx.x];
                const float nw = near + (s_t[threadIdx.x] - near) * s;
                pool[next_at * dim + threadIdx.x] = nw;
                qs[threadIdx.x] = near;
                qg[threadIdx.x] = nw;
            }
        }

        // the null question start -> start; its answer is ignored
        __device__ __forceinline__ void ask_nothing(float *qs, float *qg, const float *start, uint32_t dim)
        {
            if (threadIdx.x < dim) qs[threadIdx.x] = start[threadIdx.x], qg[threadIdx.x] = start[threadIdx.x];
        }
    }  // namespace
}  // namespace vmv
