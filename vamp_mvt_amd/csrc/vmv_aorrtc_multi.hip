// vmv_aorrtc_multi.hip — cost-bounded RRT-Connect rounds for many independent problems (vmv_aorrtc_multi).
//
// AORRTC (planning/aorrtc.hh) per problem: a first solution (vmv_rrtc_multi's contract), simplified (vmv_simplify_multi's
// contract), then searches under the cost bound of the best path so far, each on fresh trees inside the informed set of
// that bound, each new solution simplified and kept if it is cheaper.  The first solution and every simplification are
// calls of vmv_rrtc_multi / vmv_simplify_multi over the sub-batch concerned; search g of every still-optimising problem
// runs as ONE lockstep call of aox_step_kernel below (rounds of vmv_lockstep.h, one question per problem); the host
// compares costs between generations.
//
// The contract of one search, per problem (fp32, one rounding per written operation, -ffp-contract=off; sqrtf and / are
// correctly rounded on gfx950; sums over joints sequential in joint order):
//   uniform stream   seed = (uint32) halton_skip, a 32-bit counter c (0 at the first search, runs on through all searches
//                    of the problem), pre-incremented per draw: x = c * 0x9E3779B9 + seed; x ^= x >> 16;
//                    x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16; U = float(x >> 8) * 2^-24.
//   ln32(s), 0<s<1   e = unbiased exponent, m = mantissa in [1, 2); mantissa bits > 0x3504f3 (fl(sqrt 2)): m = m / 2, e = e + 1;
//                    t = (m - 1) / (m + 1), t2 = t * t, p = 1/11, p = p * t2 + 1/k for k = 9 7 5 3 1,
//                    ln32 = float(e) * HI + (float(e) * LO + (2 * t) * p), HI = 0x3f317180, LO = 0x3717f7d1 (ln 2 split).
//   Gaussian pair    repeat u1 = 2U - 1, u2 = 2U - 1, s = u1 u1 + u2 u2 until 0 < s < 1; m = sqrtf((-2 ln32(s)) / s);
//                    (u1 m, u2 m).
//   PHS frame        dmin = distance(start, goal), centre = (start + goal) * 0.5, a1 = (goal - start) / dmin, v = a1 with
//                    v[0] += (a1[0] >= 0 ? 1 : -1), vv = sum v[j] v[j]  (the Householder reflection e1 -> -+a1).
//   PHS sample       g[0 .. n+1] from ceil((n + 2) / 2) pairs (a surplus value dropped), norm = sqrtf(sum g[i] g[i]),
//                    r1 = max_cost * 0.5, rc = sqrtf(max(max_cost max_cost - dmin dmin, 0)) * 0.5,
//                    y[j] = (g[j] / norm) * (j == 0 ? r1 : rc), k = (2 * sum v[j] y[j]) / vv, t = centre + (y - v * k);
//                    out of bounds unless lower[j] <= t[j] <= fl(lower[j] + span[j]) for every joint (NaN: out).
//   nearest(T, t, c)      over the counted nodes i of T: d_i = sqrtf(sum (node_i[j] - t[j])^2), admissible iff
//                    !(cost_i > 0) || !(c < cost_i + d_i), key_i = sqrtf(d_i d_i + (cost_i - c)(cost_i - c)); the FIRST
//                    index with the least key among the admissible nodes, and its d_i.  An associative argmin: the
//                    workgroup's lanes stride over the tree (nearest<true> of vmv_two_trees.h with this key).
//   one search       fresh trees (roots cost 0, A = the start tree); while iterations < budget && |A| + |B| < max_samples:
//                    ++iterations, the balance swap of vmv_rrtc_multi; t = PHS sample, out of bounds: continue;
//                    g = dist(t, rootA), f = g + dist(t, rootB), c_rand = U * max(max_cost - f, 0) + g;
//                    (ni, d) = nearest(A, t, c_rand), !(d > 0): continue; new = near + (t - near) * (min(d, R) / d);
//                    ask near -> new, invalid: continue; new_cost = cost[ni] + dist(new, near);
//                    cost_bound_resample: g2 = dist(new, rootA), up to max_cost_bound_resamples times:
//                    cr = max(new_cost - g2, 0), draw U, (mi, md) = nearest(A, new, U * cr + g2) with `new` not yet
//                    counted; stop if mi == ni or !(cost[mi] + md < new_cost) or cr == 0; ask A[mi] -> new: valid:
//                    ni = mi, new_cost = cost[mi] + md; invalid: stop;
//                    add new (parent ni, cost new_cost); (bi, bd) = nearest(B, new, max_cost - new_cost);
//                    !((new_cost + bd) + cost[bi] < max_cost): continue; the connect march of vmv_rrtc_multi from B[bi]
//                    towards new, every added node with cost[prev] + dist(w, from); connected: solved, the path traced by
//                    vmv_rrtc_multi's trace_path (vmv_two_trees.h).  Unsolved: MAX_ITERATIONS if the budget was reached, else MAX_SAMPLES.
//
// aox_step_kernel: one 256-thread workgroup per unfinished problem; the phases are extend, re-parent (A[mi] -> new is in
// flight while `new` sits uncounted in A's next slot) and march.  One lane draws the sample and shares it through LDS;
// every branch is taken by the whole workgroup.  Iterations that ask nothing loop inside the kernel, at most kAoxSpinCap
// per launch (then a null question; the state carries on, so the cap changes no result).  A problem's two trees share one
// pool of max_samples nodes, the start tree from the front, the goal tree from the back (vmv_two_trees.h), with parent and
// cost arrays.
// Every store is a plain vector store by the owning workgroup; no atomics.
//
// vmv_aorrtc_multi_constrained is the same loop inside the band of an end-effector constraint: the first
// solution by vmv_rrtc_multi_constrained, every simplification by vmv_simplify_multi_constrained, and the searches by
// aox_step_constrained_kernel - the same body, which names each question's new node for the robot's
// constraint_round_kernel (vmv_rrtc_multi_constrained's, launched right behind it) and ANDs that kernel's answer in.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"
#include "vmv_two_trees.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace vmv
{
    namespace
    {
        constexpr uint32_t kAoxBlock = kTreeBlock;
        constexpr uint32_t kAoxDefaultCheckEvery = 16;
        constexpr uint32_t kAoxSpinCap = 64;        // iterations without a question per launch
        constexpr uint32_t kAoxMaxResamples = 64;   // max_cost_bound_resamples the call accepts

        enum : uint32_t
        {
            kAoxFresh = 0,     // nothing asked yet
            kAoxIdle = 1,      // a null question is in flight (the spin cap): the loop goes on
            kAoxExtend = 2,    // near -> new is in flight (new sits in A's next slot, not yet counted)
            kAoxReparent = 3,  // A[mi] -> new is in flight (new still uncounted)
            kAoxMarch = 4,     // step k of the connect march is in flight (w sits in B's next slot, not yet counted)
            kAoxDone = 5
        };

        struct AoxState  // 96 bytes per problem
        {
            uint32_t phase, status, iterations, counter;  // counter: the uniform stream's, kept across searches
            uint32_t n[2];           // nodes of the start tree (side 0) and the goal tree (side 1)
            uint32_t a_side, slot;   // which side is A; position of the question in flight in its round's arrays
            uint32_t new_i, ni, mi;  // `new` in A once counted; its parent so far; the parent being asked
            uint32_t resamples;      // cost-bound resamples made for `new`
            uint32_t bi, prev, k, n_steps;
            float bd, new_cost, cand_cost, g2;  // cand_cost: new_cost if A[mi] -> new is valid
            float max_cost;
            uint32_t budget, path_len, questions;
        };
        static_assert(sizeof(AoxState) == 96, "24 words per problem");

        struct AoxParams
        {
            uint32_t dim, max_samples, balance, resample, max_resamples;
            float range, tree_ratio;
            float lower[kPlanMaxDim], span[kPlanMaxDim];
        };

        struct AoxArrays
        {
            AoxState *state;              // [n_problems]
            float *pool;                  // [n_problems][max_samples][dim]
            uint32_t *parent;             // [n_problems][max_samples], indices within the node's own tree
            float *cost;                  // [n_problems][max_samples]
            const float *starts, *goals;  // [n_problems][dim]
            const uint64_t *skips;        // [n_problems]
            const float *max_cost;        // [n_problems] the bound of the search to come
            const uint32_t *budget;       // [n_problems] its iterations
            const uint32_t *active;       // [n_active] problem of each workgroup
            float *q_start, *q_goal;      // [n_active][dim] the round's questions
            const uint64_t *bits;         // answers of the previous round
            uint8_t *done;                // [n_problems]
            // vmv_aorrtc_multi_constrained only (aox_step<true>; not read otherwise): pending[a] = the pool element, over
            // all problems, of the new node the question's far end was written to - A's next slot for an extension, B's
            // next slot for a march step - or kNoPending for a re-parent, the null question and finished problems;
            // c_ok[slot] = the constraint round's answer to the previous question, ANDed into the validity bit
            uint64_t *pending;            // [n_active]
            const uint8_t *c_ok;          // [n_active]
        };

        struct PhsFrame
        {
            float centre[kPlanMaxDim], v[kPlanMaxDim];
            float dmin, vv;
        };

        __device__ __forceinline__ float aox_uniform(uint32_t seed, uint32_t &c)
        {
            ++c;
            uint32_t x = c * 0x9E3779B9u + seed;
            x ^= x >> 16;
            x *= 0x7feb352du;
            x ^= x >> 15;
            x *= 0x846ca68bu;
            x ^= x >> 16;
            return (float) (x >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
        }

        __device__ __forceinline__ float aox_ln32(float s)
        {
            const uint32_t bits = __float_as_uint(s);
            int e = (int) (bits >> 23) - 127;
            uint32_t mant = bits & 0x7fffffu;
            if (mant > 0x3504f3u)  // above fl(sqrt(2)): m / 2 and the next exponent
                e += 1, mant |= 0x3f000000u;
            else
                mant |= 0x3f800000u;
            const float m = __uint_as_float(mant);
            const float t = (m - 1.f) / (m + 1.f), t2 = t * t;
            float p = 1.f / 11.f;
            p = p * t2 + 1.f / 9.f;
            p = p * t2 + 1.f / 7.f;
            p = p * t2 + 1.f / 5.f;
            p = p * t2 + 1.f / 3.f;
            p = p * t2 + 1.f;
            const float ln2_hi = __uint_as_float(0x3f317180u), ln2_lo = __uint_as_float(0x3717f7d1u);
            return (float) e * ln2_hi + ((float) e * ln2_lo + (2.f * t) * p);
        }

        __device__ void aox_gaussian_pair(uint32_t seed, uint32_t &c, float &g0, float &g1)
        {
            float u1, u2, s;
            do
            {
                u1 = 2.f * aox_uniform(seed, c) - 1.f;
                u2 = 2.f * aox_uniform(seed, c) - 1.f;
                s = u1 * u1 + u2 * u2;
            } while (!(0.f < s && s < 1.f));
            const float m = sqrtf((-2.f * aox_ln32(s)) / s);
            g0 = u1 * m, g1 = u2 * m;
        }

        // one thread
        __device__ void phs_frame(const float *start, const float *goal, uint32_t dim, PhsFrame &F)
        {
            float sum = 0.f;
            for (uint32_t j = 0; j < dim; ++j)
            {
                const float df = goal[j] - start[j];
                sum = sum + df * df;
            }
            F.dmin = sqrtf(sum);
            float vv = 0.f;
            for (uint32_t j = 0; j < dim; ++j)
            {
                F.centre[j] = (start[j] + goal[j]) * 0.5f;
                float v = (goal[j] - start[j]) / F.dmin;
                if (j == 0) v = v + (v >= 0.f ? 1.f : -1.f);
                F.v[j] = v;
                vv = vv + v * v;
            }
            F.vv = vv;
        }

        // one thread; g: dim + 2 floats of scratch, t: the sample -> in bounds
        __device__ bool phs_sample(const PhsFrame &F, uint32_t dim, const float *lower, const float *span, float max_cost,
                                   uint32_t seed, uint32_t &c, float *g, float *t)
        {
            const uint32_t ng = dim + 2u;
            for (uint32_t i = 0; i < ng; i += 2)
            {
                float g0, g1;
                aox_gaussian_pair(seed, c, g0, g1);
                g[i] = g0;
                if (i + 1u < ng) g[i + 1u] = g1;
            }
            float sum = 0.f;
            for (uint32_t i = 0; i < ng; ++i) sum = sum + g[i] * g[i];
            const float norm = sqrtf(sum);
            const float r1 = max_cost * 0.5f;
            const float rc = sqrtf(fmaxf(max_cost * max_cost - F.dmin * F.dmin, 0.f)) * 0.5f;
            float dot = 0.f;
            for (uint32_t j = 0; j < dim; ++j)
            {
                g[j] = (g[j] / norm) * (j == 0 ? r1 : rc);  // y
                dot = dot + F.v[j] * g[j];
            }
            const float k = (2.f * dot) / F.vv;
            bool ok = true;
            for (uint32_t j = 0; j < dim; ++j)
            {
                const float x = F.centre[j] + (g[j] - F.v[j] * k);
                t[j] = x;
                ok = ok && lower[j] <= x && x <= lower[j] + span[j];
            }
            return ok;
        }

        // fresh trees, bound and budget for the search to come of every active problem; the uniform counter stays
        __global__ __launch_bounds__(kAoxBlock) void aox_init_kernel(const AoxParams P, const AoxArrays D, const uint32_t n_active)
        {
            const uint32_t a = blockIdx.x * kAoxBlock + threadIdx.x;
            if (a >= n_active) return;
            const uint32_t p = D.active[a], M = P.max_samples;
            init_roots(D.pool + (size_t) p * M * P.dim, D.parent + (size_t) p * M, D.starts + (size_t) p * P.dim,
                       D.goals + (size_t) p * P.dim, P.dim, M);
            float *cost = D.cost + (size_t) p * M;
            cost[node_at(0, 0, M)] = 0.f, cost[node_at(1, 0, M)] = 0.f;
            AoxState st{};
            st.phase = kAoxFresh, st.status = VMV_PLAN_MAX_ITERATIONS;
            st.counter = D.state[p].counter;
            st.n[0] = st.n[1] = 1;
            st.new_i = kNone;
            st.max_cost = D.max_cost[p], st.budget = D.budget[p];
            D.state[p] = st;
            D.done[p] = 0;
        }

        // One workgroup per active problem; every branch below is taken by the whole workgroup (its conditions are
        // values every thread holds alike), so the barriers and cross-lane reads inside nearest() are safe.
        // kConstrained (vmv_aorrtc_multi_constrained): every question names its pending node for
        // constraint_round_kernel, which runs between this kernel and the round's validation, projects that node in the
        // pool and in q_goal and answers c_ok; what is derived from a pending node is computed after the answer.
        template <bool kConstrained>
        __device__ __forceinline__ void aox_step(const AoxParams &P, const AoxArrays &D)
        {
            __shared__ float s_t[kPlanMaxDim];
            __shared__ float s_g[kPlanMaxDim + 2];
            __shared__ float s_rk[kTreeWaves], s_rd[kTreeWaves];
            __shared__ uint32_t s_ri[kTreeWaves];
            __shared__ PhsFrame s_frame;
            __shared__ float s_c;           // the sampled cost bound of the next search
            __shared__ uint32_t s_ok, s_counter;
            const uint32_t a = blockIdx.x, p = D.active[a], tid = threadIdx.x, dim = P.dim, M = P.max_samples;
            AoxState st = D.state[p];
            float *pool = D.pool + (size_t) p * M * dim;
            uint32_t *parent = D.parent + (size_t) p * M;
            float *cost = D.cost + (size_t) p * M;
            float *qs = D.q_start + (size_t) a * dim, *qg = D.q_goal + (size_t) a * dim;
            const float *start = D.starts + (size_t) p * dim, *goal = D.goals + (size_t) p * dim;
            const float R = P.range;
            const uint32_t seed = (uint32_t) D.skips[p];
            if (tid == 0) s_counter = st.counter;  // lane 0 alone draws
            __syncthreads();
            const auto save = [&]() {
                if (tid == 0)
                {
                    st.counter = s_counter;
                    D.state[p] = st;
                }
            };
            const auto pend = [&](uint64_t element) {  // the question just written: its new node, or kNoPending
                if constexpr (kConstrained)
                    if (tid == 0) D.pending[a] = element;
            };

            // the contract's nearest(T, s_t, c): T's first admissible node of the least key, and its distance to s_t
            const auto search = [&](uint32_t side, float c, float &out_d, uint32_t &out_i) {
                nearest<true>(
                    pool, side, count_of(st.n, side), dim, M,
                    [&](const float *q, size_t at) {
                        const float d = tree_dist(q, s_t, dim), ci = cost[at];
                        const float dc = ci - c;
                        return Scored{!(ci > 0.f) || !(c < ci + d), sqrtf(d * d + dc * dc), d};
                    },
                    s_rk, s_rd, s_ri, out_d, out_i);
            };

            enum { kLoop, kResample, kCommit, kMarchStep, kFinish } act = kLoop;
            if (st.phase == kAoxDone)
                act = kFinish;
            else if (st.phase != kAoxFresh && st.phase != kAoxIdle)
            {
                bool ans = (D.bits[st.slot >> 6] >> (st.slot & 63u)) & 1ull;
                if constexpr (kConstrained) ans = ans && D.c_ok[st.slot] != 0;
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                if (st.phase == kAoxExtend)
                {
                    if (ans)
                    {
                        const float *nw = pool + node_at(sa, count_of(st.n, sa), M) * dim;
                        st.new_cost = cost[node_at(sa, st.ni, M)] + tree_dist(nw, pool + node_at(sa, st.ni, M) * dim, dim);
                        st.g2 = tree_dist(nw, pool + node_at(sa, 0, M) * dim, dim);
                        st.resamples = 0;
                        act = kResample;
                    }
                }
                else if (st.phase == kAoxReparent)
                {
                    if (ans)
                        st.ni = st.mi, st.new_cost = st.cand_cost, act = kResample;
                    else
                        act = kCommit;
                }
                else  // kAoxMarch
                {
                    if (ans)
                    {
                        if constexpr (kConstrained)
                        {
                            // w was projected in place: its cost is that of the projected point.  Lane 0 alone reads it
                            // before the barriers of the loop below, which every other reader of cost[] lies behind.
                            const size_t w_at = node_at(sb, count_of(st.n, sb), M), prev_at = node_at(sb, st.prev, M);
                            if (tid == 0) cost[w_at] = cost[prev_at] + tree_dist(pool + w_at * dim, pool + prev_at * dim, dim);
                        }
                        st.prev = grow(st.n, sb);
                        if (++st.k == st.n_steps)
                            st.status = VMV_PLAN_SOLVED, act = kFinish;
                        else
                            act = kMarchStep;
                    }
                }
            }

            if (act == kResample)  // `new` sits uncounted in A's next slot with parent ni and cost new_cost so far
            {
                const uint32_t sa = st.a_side;
                const size_t new_at = node_at(sa, count_of(st.n, sa), M);
                if (tid < dim) s_t[tid] = pool[new_at * dim + tid];
                __syncthreads();
                act = kCommit;
                if (P.resample && st.resamples < P.max_resamples)  // one attempt per launch: its question ends the launch
                {
                    ++st.resamples;
                    const float cr = fmaxf(st.new_cost - st.g2, 0.f);
                    if (tid == 0) s_c = aox_uniform(seed, s_counter) * cr + st.g2;
                    __syncthreads();
                    const float c = s_c;
                    float md;
                    uint32_t mi;
                    search(sa, c, md, mi);
                    const float cand = mi == kNone ? INFINITY : cost[node_at(sa, mi, M)] + md;
                    if (mi != kNone && mi != st.ni && cand < st.new_cost && cr != 0.f)
                    {
                        if (tid < dim) qs[tid] = pool[node_at(sa, mi, M) * dim + tid], qg[tid] = s_t[tid];
                        st.mi = mi, st.cand_cost = cand;
                        st.phase = kAoxReparent, st.slot = a, ++st.questions;
                        pend(kNoPending);  // `new` is projected already: the edge is band-checked only
                        save();
                        return;
                    }
                }
            }

            if (act == kCommit)  // count `new`, then look for a connection that beats the bound
            {
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                st.new_i = grow(st.n, sa);
                const size_t new_at = node_at(sa, st.new_i, M);
                if (tid == 0) parent[new_at] = st.ni, cost[new_at] = st.new_cost;
                if (tid < dim) s_t[tid] = pool[new_at * dim + tid];
                __syncthreads();  // the cost is read by later searches of this launch
                search(sb, st.max_cost - st.new_cost, st.bd, st.bi);
                act = kLoop;
                if (st.bi != kNone && (st.new_cost + st.bd) + cost[node_at(sb, st.bi, M)] < st.max_cost)
                {
                    st.n_steps = march_steps(st.bd, R);
                    st.k = 0, st.prev = st.bi;
                    act = kMarchStep;
                }
            }

            if (act == kMarchStep)
            {
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                if (st.n[0] + st.n[1] >= M)
                    act = kLoop;  // the pool is full: the march ends unconnected
                else
                {
                    const float *o = pool + node_at(sb, st.bi, M) * dim, *nw = pool + node_at(sa, st.new_i, M) * dim;
                    const float *from = pool + node_at(sb, st.prev, M) * dim;
                    const size_t w_at = node_at(sb, count_of(st.n, sb), M);
                    const float s = st.bd > 0.f ? fminf((float) (st.k + 1u) * R, st.bd) / st.bd : 0.f;
                    float sum = 0.f;  // every thread computes the whole of w: dist(w, from) needs no exchange
                    for (uint32_t j = 0; j < dim; ++j)
                    {
                        float w = nw[j];
                        if (st.bd > 0.f) w = o[j] + (nw[j] - o[j]) * s;
                        const float df = w - from[j];
                        sum = sum + df * df;
                        if (tid == j) pool[w_at * dim + j] = w, qs[j] = from[j], qg[j] = w;
                    }
                    st.phase = kAoxMarch, st.slot = a, ++st.questions;
                    if (tid == 0) parent[w_at] = st.prev, cost[w_at] = cost[node_at(sb, st.prev, M)] + sqrtf(sum);
                    pend((uint64_t) p * M + w_at);
                    save();
                    return;
                }
            }

            if (act == kLoop)
            {
                if (tid == 0) phs_frame(start, goal, dim, s_frame);
                uint32_t spins = 0;
                for (;;)
                {
                    if (st.iterations >= st.budget)
                    {
                        st.status = VMV_PLAN_MAX_ITERATIONS, act = kFinish;
                        break;
                    }
                    if (st.n[0] + st.n[1] >= M)
                    {
                        st.status = VMV_PLAN_MAX_SAMPLES, act = kFinish;
                        break;
                    }
                    if (spins >= kAoxSpinCap)  // a null question; the loop goes on in the next round
                    {
                        ask_nothing(qs, qg, start, dim);
                        st.phase = kAoxIdle, st.slot = a;
                        pend(kNoPending);
                        save();
                        return;
                    }
                    ++spins;
                    ++st.iterations;
                    st.a_side = next_a_side(st.n, st.a_side, P.balance, P.tree_ratio);
                    const uint32_t sa = st.a_side, sb = sa ^ 1u;
                    if (tid == 0)
                    {
                        const bool ok = phs_sample(s_frame, dim, P.lower, P.span, st.max_cost, seed, s_counter, s_g, s_t);
                        s_ok = ok ? 1u : 0u;
                        if (ok)
                        {
                            const float g = tree_dist(s_t, pool + node_at(sa, 0, M) * dim, dim);
                            const float f = g + tree_dist(s_t, pool + node_at(sb, 0, M) * dim, dim);
                            const float c_range = fmaxf(st.max_cost - f, 0.f);
                            s_c = aox_uniform(seed, s_counter) * c_range + g;
                        }
                    }
                    __syncthreads();
                    const bool ok = s_ok != 0u;
                    const float c = s_c;
                    __syncthreads();  // lane 0 may draw again
                    if (!ok) continue;
                    float d;
                    uint32_t ni;
                    search(sa, c, d, ni);
                    if (ni == kNone || !(d > 0.f)) continue;
                    ask_extension(pool, node_at(sa, ni, M), node_at(sa, count_of(st.n, sa), M), dim, s_t, d, R, qs, qg);
                    st.ni = ni;
                    st.phase = kAoxExtend, st.slot = a, ++st.questions;
                    pend((uint64_t) p * M + node_at(sa, count_of(st.n, sa), M));
                    save();
                    return;
                }
            }

            // finished (now or in an earlier round)
            ask_nothing(qs, qg, start, dim);
            pend(kNoPending);
            if (st.phase != kAoxDone && tid == 0)
            {
                st.phase = kAoxDone, st.slot = a;
                st.path_len = st.status == VMV_PLAN_SOLVED ? trace_path(st.a_side, st.new_i, st.prev, pool, parent, dim, M, nullptr) : 0u;
                st.counter = s_counter;
                D.state[p] = st;
                D.done[p] = 1;
            }
        }

        __global__ __launch_bounds__(kAoxBlock) void aox_step_kernel(const AoxParams P, const AoxArrays D) { aox_step<false>(P, D); }

        __global__ __launch_bounds__(kAoxBlock) void aox_paths_kernel(const AoxParams P, const AoxArrays D, const uint32_t n_active,
                                                                       const uint64_t *__restrict__ offsets, float *__restrict__ paths)
        {
            const uint32_t a = blockIdx.x * kAoxBlock + threadIdx.x;
            if (a >= n_active) return;
            const uint32_t p = D.active[a];
            const AoxState st = D.state[p];
            if (st.phase != kAoxDone || st.status != VMV_PLAN_SOLVED) return;
            (void) trace_path(st.a_side, st.new_i, st.prev, D.pool + (size_t) p * P.max_samples * P.dim,
                              D.parent + (size_t) p * P.max_samples, P.dim, P.max_samples, paths + offsets[a] * P.dim);
        }

        // vmv_phs_samples: n successive samples of one problem's stream, drawn by one lane as aox_step_kernel draws them
        __global__ __launch_bounds__(kWave) void phs_samples_kernel(const AoxParams P, const float *__restrict__ start,
                                                                     const float *__restrict__ goal, const float max_cost,
                                                                     const uint32_t seed, const uint32_t counter, const uint32_t n,
                                                                     float *__restrict__ out_q, uint8_t *__restrict__ out_ok,
                                                                     uint32_t *__restrict__ out_counter)
        {
            __shared__ PhsFrame s_frame;
            __shared__ float s_g[kPlanMaxDim + 2], s_t[kPlanMaxDim];
            if (threadIdx.x != 0 || blockIdx.x != 0) return;
            phs_frame(start, goal, P.dim, s_frame);
            uint32_t c = counter;
            for (uint32_t i = 0; i < n; ++i)
            {
                const bool ok = phs_sample(s_frame, P.dim, P.lower, P.span, max_cost, seed, c, s_g, s_t);
                for (uint32_t j = 0; j < P.dim; ++j) out_q[(size_t) i * P.dim + j] = s_t[j];
                out_ok[i] = ok ? 1 : 0;
            }
            *out_counter = c;
        }

        // vmv_aorrtc_multi_constrained's step kernel: behind the others, so that none of them moves in the code object
        __global__ __launch_bounds__(kAoxBlock) void aox_step_constrained_kernel(const AoxParams P, const AoxArrays D)
        {
            aox_step<true>(P, D);
        }

        float host_dist(const float *a, const float *b, int dim)
        {
            float sum = 0.f;
            for (int j = 0; j < dim; ++j)
            {
                const float df = b[j] - a[j];
                sum = sum + df * df;
            }
            return std::sqrt(sum);
        }

        // Path::cost (planning/plan.hh:13-32): the fp32 sum of the segment lengths in order
        float host_path_cost(const std::vector<float> &pts, int dim)
        {
            const size_t len = pts.size() / (size_t) dim;
            if (len < 2) return std::numeric_limits<float>::infinity();
            float acc = 0.f;
            for (size_t k = 0; k + 1 < len; ++k) acc = acc + host_dist(&pts[k * dim], &pts[(k + 1) * dim], dim);
            return acc;
        }

        // vmv_aorrtc_multi_constrained's own part of a call, NULL throughout for vmv_aorrtc_multi: the caller's constraints
        // and plan settings (what every simplification is called with), the searches' constraint round - the launcher's
        // resolved settings with the robot's bounds, max_stretch * range - and its device side, which AoxSearches::setup
        // allocates: the records (one, or one per problem: a round picks by problem), the round's answers and, per
        // problem, the questions of all searches it answered 0.
        struct AoxConstrained
        {
            const vmv_ee_constraint *constraints;
            size_t n_constraints;
            const vmv_constraint_plan_settings *settings;
            ConstraintParams P;
            float stretch;
            ConstraintDev *d_cons = nullptr;
            uint8_t *d_c_ok = nullptr;
            uint32_t *d_refused = nullptr;
        };

        // vmv_simplify_multi over paths[idx[...]] in their environments, in place; a path longer than the simplifier's
        // max_waypoints stays as it is.  The call's rounds and questions are added to the totals.
        // con: vmv_simplify_multi_constrained with each path's constraint instead; a path that comes back
        // VMV_SIMPLIFY_OUT_OF_BAND stays as it is too, and each path's vmv_paths_band_refused is added to band_refused.
        int simplify_some(int robot, const vmv_env *const *envs, int dim, const std::vector<uint32_t> &idx,
                          std::vector<std::vector<float>> &paths, const vmv_simplify_settings &S, uint64_t &rounds,
                          uint64_t &questions, const AoxConstrained *con = nullptr, std::vector<uint32_t> *band_refused = nullptr)
        {
            const size_t max_waypoints = S.max_waypoints ? S.max_waypoints : 2048;  // the simplifier's default
            std::vector<uint32_t> which;
            std::vector<const vmv_env *> sub_envs;
            std::vector<float> points;
            std::vector<size_t> offsets{0};
            for (const uint32_t p : idx)
            {
                const size_t len = paths[p].size() / (size_t) dim;
                if (len > max_waypoints) continue;
                which.push_back(p), sub_envs.push_back(envs[p]);
                points.insert(points.end(), paths[p].begin(), paths[p].end());
                offsets.push_back(offsets.back() + len);
            }
            if (which.empty()) return VMV_OK;
            vmv_paths *out = nullptr;
            if (!con)
            {
                if (int rc = vmv_simplify_multi(robot, sub_envs.data(), which.size(), points.data(), offsets.data(), &S, &out); rc != VMV_OK)
                    return rc;
            }
            else
            {
                std::vector<vmv_ee_constraint> sub_cons;  // one per path of the call, unless one serves all
                for (size_t k = 0; con->n_constraints != 1 && k < which.size(); ++k) sub_cons.push_back(con->constraints[which[k]]);
                if (int rc = vmv_simplify_multi_constrained(robot, sub_envs.data(), which.size(), points.data(), offsets.data(), &S,
                                                            con->n_constraints == 1 ? con->constraints : sub_cons.data(),
                                                            con->n_constraints == 1 ? 1 : which.size(), &con->settings->base, &out);
                    rc != VMV_OK)
                    return rc;
            }
            std::vector<uint32_t> lengths(which.size()), refused(which.size(), 0u);
            std::vector<uint8_t> status(which.size());
            uint64_t r = 0, q = 0;
            int rc = vmv_paths_summary(out, status.data(), nullptr, lengths.data(), nullptr, &r, &q);
            if (rc == VMV_OK && con) rc = vmv_paths_band_refused(out, refused.data());
            size_t total = 0;
            for (const uint32_t len : lengths) total += len;
            std::vector<float> simplified(total * (size_t) dim);
            if (rc == VMV_OK) rc = vmv_paths_points(out, simplified.data(), simplified.size());
            (void) vmv_paths_destroy(out);
            if (rc != VMV_OK) return rc;
            size_t at = 0;
            for (size_t k = 0; k < which.size(); ++k)
            {
                const size_t count = (size_t) lengths[k] * (size_t) dim;
                if (status[k] != VMV_SIMPLIFY_OUT_OF_BAND) paths[which[k]].assign(simplified.begin() + at, simplified.begin() + at + count);
                if (con) (*band_refused)[which[k]] += refused[k];
                at += count;
            }
            rounds += r, questions += q;
            return VMV_OK;
        }

        // The searches of an aorrtc call: device buffers for all n problems, allocated once; one generation = one search of
        // every problem in `active`, each with its own bound and budget.
        struct AoxSearches
        {
            int robot, dim;
            size_t n;
            uint32_t check_every, max_resamples, max_samples;
            AoxParams P{};
            AoxArrays D{};
            DeviceBuffers mem;
            LockstepBuffers B;
            float *d_max_cost = nullptr;
            uint32_t *d_budget = nullptr;
            float *d_paths = nullptr;  // the traced paths of one generation, packed
            uint64_t paths_capacity = 0;  // in waypoints
            hipStream_t stream = nullptr;
            AoxConstrained *con = nullptr;  // vmv_aorrtc_multi_constrained: the constraint round after every step kernel
            ~AoxSearches()
            {
                if (d_paths) (void) hipFree(d_paths);
            }

            int setup(const float *starts, const float *goals, const uint64_t *skips)
            {
                VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
                VMV_LOCKSTEP_HIP(mem.alloc(&D.pool, n * (size_t) max_samples * (size_t) dim));
                VMV_LOCKSTEP_HIP(mem.alloc(&D.parent, n * (size_t) max_samples));
                VMV_LOCKSTEP_HIP(mem.alloc(&D.cost, n * (size_t) max_samples));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_max_cost, n));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_budget, n));
                if (int rc = B.alloc(mem, n, n, 1, (size_t) dim, stream); rc != VMV_OK) return rc;
                if (int rc = upload_problems(mem, n, (size_t) dim, starts, goals, skips, stream, &D.starts, &D.goals, &D.skips); rc != VMV_OK)
                    return rc;
                D.active = B.active, D.q_start = B.q_start, D.q_goal = B.q_goal, D.bits = B.bits, D.done = B.done;
                D.max_cost = d_max_cost, D.budget = d_budget;
                if (con)
                {
                    std::vector<ConstraintDev> recs(con->n_constraints);
                    for (size_t k = 0; k < recs.size(); ++k)
                        constraint_record(con->constraints[k], (double) con->P.pos_tol, (double) con->P.rot_tol, recs[k]);
                    if (int rc = upload_records(mem, recs.data(), recs.size(), &con->d_cons); rc != VMV_OK) return rc;
                    VMV_LOCKSTEP_HIP(mem.alloc(&D.pending, n));
                    VMV_LOCKSTEP_HIP(mem.alloc(&con->d_c_ok, n));
                    VMV_LOCKSTEP_HIP(mem.alloc(&con->d_refused, n));
                    VMV_LOCKSTEP_HIP(hipMemsetAsync(con->d_refused, 0, std::max<size_t>(n * 4, 16), stream));
                    D.c_ok = con->d_c_ok;
                }
                VMV_LOCKSTEP_HIP(hipMemsetAsync(D.state, 0, n * sizeof(AoxState), stream));  // every counter starts at 0
                VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
                return VMV_OK;
            }

            // One search of every problem of `active` (bound max_cost[p], budget[p] iterations; both indexed by problem).
            // -> states[p] of the active problems, and found[p] = the waypoints of those that solved it.
            int generation(const vmv_env *const *envs, const std::vector<uint32_t> &active_in, const std::vector<float> &max_cost,
                           const std::vector<uint32_t> &budget, std::vector<AoxState> &states, std::vector<std::vector<float>> &found,
                           uint64_t &rounds_total)
            {
                std::vector<uint32_t> active(active_in);
                std::vector<const vmv_env *> active_envs(active.size());
                uint32_t max_budget = 0;
                for (size_t k = 0; k < active.size(); ++k)
                    active_envs[k] = envs[active[k]], max_budget = std::max(max_budget, budget[active[k]]);
                const uint32_t na = (uint32_t) active.size();
                VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active.data(), na * 4ull, hipMemcpyHostToDevice));
                VMV_LOCKSTEP_HIP(hipMemcpy(d_max_cost, max_cost.data(), n * 4, hipMemcpyHostToDevice));
                VMV_LOCKSTEP_HIP(hipMemcpy(d_budget, budget.data(), n * 4, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(aox_init_kernel, dim3((na + kAoxBlock - 1) / kAoxBlock), dim3(kAoxBlock), 0, stream, P, D, na);
                VMV_LOCKSTEP_HIP(hipGetLastError());

                // an iteration asks at most 1 + max_resamples questions that add no node (an invalid extension; or the re-parent
                // questions and the march's invalid step), every other question adds a node; a null round of the spin cap stands
                // for kAoxSpinCap iterations that asked nothing: a bound on the rounds that does not depend on the device's answers
                const uint64_t max_rounds = (uint64_t) max_budget * (1ull + max_resamples) + max_samples + check_every + 2ull;
                uint64_t rounds = 0;
                const auto step = [&](uint32_t count) {
                    if (!con)
                    {
                        hipLaunchKernelGGL(aox_step_kernel, dim3(count), dim3(kAoxBlock), 0, stream, P, D);
                        return;
                    }
                    // the pending node projected and written back, the edge's band test: before the round's validation
                    hipLaunchKernelGGL(aox_step_constrained_kernel, dim3(count), dim3(kAoxBlock), 0, stream, P, D);
                    (void) robot_launchers(robot).constraint_round(con->P, con->d_cons, B.active, B.q_start, B.q_goal, D.pending, D.pool,
                                                                   con->stretch, con->d_c_ok, con->d_refused, count, stream);
                };
                if (int rc = lockstep_rounds(robot, stream, check_every, max_rounds, 1, active, active_envs, B.arrays(),
                                             con ? "vmv_aorrtc_multi_constrained" : "vmv_aorrtc_multi",
                                             con ? "aox_step_constrained_kernel" : "aox_step_kernel", step, rounds);
                    rc != VMV_OK)
                    return rc;
                rounds_total += rounds;

                states.resize(n);
                VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(AoxState), hipMemcpyDeviceToHost));
                std::vector<uint32_t> lengths(na);
                for (uint32_t k = 0; k < na; ++k) lengths[k] = states[active_in[k]].path_len;
                uint64_t total = 0;
                const std::vector<uint64_t> offsets = path_offsets_of(lengths.data(), na, total);
                if (!total) return VMV_OK;
                // (lockstep_rounds compacted d_active: the trace runs over the generation's whole list again)
                VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active_in.data(), na * 4ull, hipMemcpyHostToDevice));
                VMV_LOCKSTEP_HIP(hipMemcpy(B.path_offsets, offsets.data(), na * 8ull, hipMemcpyHostToDevice));
                if (total > paths_capacity)  // the trace buffer only grows: most generations reuse it
                {
                    const uint64_t want = std::max<uint64_t>(total, 2 * paths_capacity);
                    if (d_paths) (void) hipFree(d_paths);
                    d_paths = nullptr, paths_capacity = 0;
                    VMV_LOCKSTEP_HIP(hipMalloc(&d_paths, want * (size_t) dim * 4));
                    paths_capacity = want;
                }
                hipLaunchKernelGGL(aox_paths_kernel, dim3((na + kAoxBlock - 1) / kAoxBlock), dim3(kAoxBlock), 0, stream, P, D, na,
                                   B.path_offsets, d_paths);
                hipError_t e = hipGetLastError();
                std::vector<float> packed(total * (size_t) dim);
                if (e == hipSuccess) e = hipMemcpy(packed.data(), d_paths, packed.size() * 4, hipMemcpyDeviceToHost);
                if (e != hipSuccess) return hip_status(e, "aox_paths_kernel");
                for (uint32_t k = 0; k < na; ++k)
                {
                    const uint32_t p = active_in[k];
                    const size_t count = (size_t) lengths[k] * (size_t) dim;
                    found[p].assign(packed.begin() + offsets[k] * dim, packed.begin() + offsets[k] * dim + count);
                }
                return VMV_OK;
            }
        };

        // After the first stage: `plans` is vmv_rrtc_multi's result for the n > 0 problems and becomes the call's result.
        int aorrtc_after_first(int robot, int dim, const float *lower, const float *span, const vmv_env *const *envs, size_t n,
                               const float *starts, const float *goals, const uint64_t *skips, const vmv_aorrtc_settings &S,
                               vmv_plans *plans, AoxConstrained *con = nullptr)
        {
            const float inf = std::numeric_limits<float>::infinity();
            plans->first_costs.assign(n, inf), plans->final_costs.assign(n, inf);
            plans->searches.assign(n, 0), plans->improvements.assign(n, 0);
            std::vector<std::vector<float>> best(n);
            std::vector<uint32_t> solved;
            size_t at = 0;
            for (size_t p = 0; p < n; ++p)
            {
                const size_t count = (size_t) plans->path_lengths[p] * (size_t) dim;
                best[p].assign(plans->paths.begin() + at, plans->paths.begin() + at + count);
                at += count;
                if (plans->status[p] == VMV_PLAN_SOLVED) solved.push_back((uint32_t) p);
            }
            if (S.simplify_intermediate)
                if (int rc = simplify_some(robot, envs, dim, solved, best, S.simplify, plans->rounds, plans->questions, con,
                                           &plans->band_refused);
                    rc != VMV_OK)
                    return rc;
            std::vector<uint32_t> optimising;
            std::vector<float> dmin(n, 0.f);
            for (const uint32_t p : solved)
            {
                plans->first_costs[p] = plans->final_costs[p] = host_path_cost(best[p], dim);
                dmin[p] = host_dist(starts + (size_t) p * dim, goals + (size_t) p * dim, dim);
                if (S.optimize && best[p].size() != 2u * (size_t) dim) optimising.push_back(p);
            }

            if (!optimising.empty())
            {
                AoxSearches X;
                X.robot = robot, X.dim = dim, X.n = n, X.con = con;
                X.check_every = S.rrtc.check_every ? S.rrtc.check_every : kAoxDefaultCheckEvery;
                X.max_resamples = S.cost_bound_resample ? S.max_cost_bound_resamples : 0u, X.max_samples = S.max_samples;
                X.P.dim = (uint32_t) dim, X.P.max_samples = S.max_samples, X.P.balance = S.rrtc.balance ? 1u : 0u;
                X.P.resample = S.cost_bound_resample ? 1u : 0u, X.P.max_resamples = S.max_cost_bound_resamples;
                X.P.range = S.rrtc.range, X.P.tree_ratio = S.rrtc.tree_ratio;
                for (int j = 0; j < dim; ++j) X.P.lower[j] = lower[j], X.P.span[j] = span[j];
                if (int rc = X.setup(starts, goals, skips); rc != VMV_OK) return rc;
                std::vector<float> max_cost(n, 0.f);
                std::vector<uint32_t> budget(n, 0);
                std::vector<AoxState> states;
                std::vector<std::vector<float>> found(n);
                for (;;)
                {
                    std::vector<uint32_t> active;
                    for (const uint32_t p : optimising)
                        if (plans->iterations[p] < S.max_iterations && plans->final_costs[p] - dmin[p] > 1e-8f &&
                            (S.max_searches == 0 || plans->searches[p] < S.max_searches))
                        {
                            active.push_back(p);
                            max_cost[p] = plans->final_costs[p];
                            budget[p] = std::min(S.max_iterations - plans->iterations[p], S.max_internal_iterations);
                        }
                    if (active.empty()) break;
                    if (int rc = X.generation(envs, active, max_cost, budget, states, found, plans->rounds); rc != VMV_OK) return rc;
                    std::vector<uint32_t> improved;
                    for (const uint32_t p : active)
                    {
                        const AoxState &st = states[p];
                        ++plans->searches[p];
                        plans->iterations[p] += st.iterations;
                        plans->sizes2[2 * p] = st.n[st.a_side], plans->sizes2[2 * p + 1] = st.n[st.a_side ^ 1u];
                        plans->questions += st.questions;
                        if (st.status == VMV_PLAN_SOLVED) improved.push_back(p);
                    }
                    if (S.simplify_intermediate)
                        if (int rc = simplify_some(robot, envs, dim, improved, found, S.simplify, plans->rounds, plans->questions, con,
                                                   &plans->band_refused);
                            rc != VMV_OK)
                            return rc;
                    for (const uint32_t p : improved)
                    {
                        const float c = host_path_cost(found[p], dim);
                        if (c < plans->final_costs[p])
                        {
                            best[p].swap(found[p]);
                            plans->final_costs[p] = c;
                            ++plans->improvements[p];
                        }
                    }
                }
                if (con)  // the questions of all searches the constraint round answered 0
                {
                    std::vector<uint32_t> refused(n);
                    VMV_LOCKSTEP_HIP(hipMemcpy(refused.data(), con->d_refused, n * 4, hipMemcpyDeviceToHost));
                    for (size_t p = 0; p < n; ++p) plans->band_refused[p] += refused[p];
                }
            }

            plans->aorrtc = true;
            plans->paths.clear();
            for (size_t p = 0; p < n; ++p)
            {
                plans->path_lengths[p] = (uint32_t) (best[p].size() / (size_t) dim);
                plans->paths.insert(plans->paths.end(), best[p].begin(), best[p].end());
            }
            return VMV_OK;
        }

        // vmv_aorrtc_multi's own checks, device-free and in the header's order; those of vmv_rrtc_multi follow in the
        // first stage's call.  The simplifier's settings are checked by an empty call of the simplifier.
        int aorrtc_checks(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                          const vmv_aorrtc_settings *settings, vmv_plans *const *out, int *dim)
        {
            *dim = vmv_robot_dimension(robot);
            if (robot < 0 || robot >= vmv_num_robots() || *dim <= 0 || *dim > (int) kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
            if (!settings || !out || (n_problems > 0 && (!envs || !starts || !goals))) return VMV_ERR_INVALID_ARGUMENT;
            if (n_problems >= kMultiMaxConfigs / 64) return VMV_ERR_INVALID_ARGUMENT;  // (64 questions per path per round)
            const vmv_aorrtc_settings &S = *settings;
            if (S.max_internal_iterations == 0 || S.max_cost_bound_resamples > kAoxMaxResamples) return VMV_ERR_INVALID_ARGUMENT;
            vmv_paths *none = nullptr;
            if (int rc = vmv_simplify_multi(robot, nullptr, 0, nullptr, nullptr, &S.simplify, &none); rc != VMV_OK) return rc;
            (void) vmv_paths_destroy(none);
            return VMV_OK;
        }

        // the first stage's settings: rrtc's own with the two maxima of the AORRTC settings (aorrtc.hh:384-386)
        vmv_rrtc_settings aorrtc_first_stage(const vmv_aorrtc_settings &S)
        {
            vmv_rrtc_settings first = S.rrtc;
            first.max_iterations = S.max_iterations, first.max_samples = S.max_samples;
            return first;
        }

        // `plans`: the first stage's result, owned from here on: it becomes the call's result in *out, or is deleted
        int aorrtc_finish(int robot, int dim, const vmv_env *const *envs, size_t n, const float *starts, const float *goals,
                          const uint64_t *skips, const vmv_aorrtc_settings &S, vmv_plans *plans, AoxConstrained *con, vmv_plans **out)
        {
            int rc = VMV_OK;
            if (n > 0)
            {
                float lower[16], span[16], descale[16];
                rc = vmv_robot_bounds(robot, lower, span, descale);
                if (rc == VMV_OK) rc = aorrtc_after_first(robot, dim, lower, span, envs, n, starts, goals, skips, S, plans, con);
            }
            else
                plans->aorrtc = true;
            if (rc != VMV_OK)
            {
                delete plans;
                return rc;
            }
            *out = plans;
            return VMV_OK;
        }

        int phs_samples_run(int robot, int dim, const float *start, const float *goal, float max_cost, uint32_t seed, uint32_t counter,
                            size_t n, float *out_q, uint8_t *out_in_bounds, uint32_t *out_counter)
        {
            AoxParams P{};
            P.dim = (uint32_t) dim;
            float descale[16];
            if (int rc = vmv_robot_bounds(robot, P.lower, P.span, descale); rc != VMV_OK) return rc;
            DeviceBuffers mem;
            float *d_start = nullptr, *d_goal = nullptr, *d_q = nullptr;
            uint8_t *d_ok = nullptr;
            uint32_t *d_counter = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_start, (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_goal, (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_q, n * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_ok, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_counter, (size_t) 1));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_start, start, (size_t) dim * 4, hipMemcpyHostToDevice));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_goal, goal, (size_t) dim * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(phs_samples_kernel, dim3(1), dim3(kWave), 0, nullptr, P, d_start, d_goal, max_cost, seed, counter,
                               (uint32_t) n, d_q, d_ok, d_counter);
            VMV_LOCKSTEP_HIP(hipGetLastError());
            if (n)
            {
                VMV_LOCKSTEP_HIP(hipMemcpy(out_q, d_q, n * (size_t) dim * 4, hipMemcpyDeviceToHost));
                VMV_LOCKSTEP_HIP(hipMemcpy(out_in_bounds, d_ok, n, hipMemcpyDeviceToHost));
            }
            VMV_LOCKSTEP_HIP(hipMemcpy(out_counter, d_counter, 4, hipMemcpyDeviceToHost));
            return VMV_OK;
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_aorrtc_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                         const uint64_t *halton_skips, const vmv_aorrtc_settings *settings, vmv_plans **out)
    {
        int dim = 0;
        if (int rc = vmv::aorrtc_checks(robot, envs, n_problems, starts, goals, settings, out, &dim); rc != VMV_OK) return rc;
        const vmv_rrtc_settings first = vmv::aorrtc_first_stage(*settings);
        vmv_plans *plans = nullptr;
        if (int rc = vmv_rrtc_multi(robot, envs, n_problems, starts, goals, halton_skips, &first, &plans); rc != VMV_OK) return rc;
        return vmv::aorrtc_finish(robot, dim, envs, n_problems, starts, goals, halton_skips, *settings, plans, nullptr, out);
    }

    int vmv_aorrtc_multi_constrained(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                                     const uint64_t *halton_skips, const vmv_aorrtc_settings *settings,
                                     const vmv_ee_constraint *constraints, size_t n_constraints,
                                     const vmv_constraint_plan_settings *constraint_settings, vmv_plans **out)
    {
        // vmv_aorrtc_multi's checks in its order; then the first stage's call makes vmv_rrtc_multi's and the constraint's own
        // in vmv_rrtc_multi_constrained's order, all of them before it touches a device
        int dim = 0;
        if (int rc = vmv::aorrtc_checks(robot, envs, n_problems, starts, goals, settings, out, &dim); rc != VMV_OK) return rc;
        vmv_rrtc_goals_settings first{};  // one goal per problem, dynamic domain and start_tree_first off
        first.base = vmv::aorrtc_first_stage(*settings);
        vmv_plans *plans = nullptr;
        if (int rc = vmv_rrtc_multi_constrained(robot, envs, n_problems, starts, goals, nullptr, halton_skips, &first, constraints,
                                                n_constraints, constraint_settings, &plans);
            rc != VMV_OK)
            return rc;
        plans->rrtc_goals = false;  // (one goal per problem: there is no goal index to read)
        // the band once more for the searches: the checks passed above, so this cannot refuse
        vmv::AoxConstrained con{constraints, n_constraints, constraint_settings};
        vmv::ConstraintBand band{};
        float lower[16], span[16], descale[16];
        int rc = vmv_robot_bounds(robot, lower, span, descale);
        if (rc == VMV_OK && !vmv::constraint_band_resolve(constraints, n_constraints, constraint_settings->base, nullptr, band).empty())
            rc = VMV_ERR_INVALID_ARGUMENT;
        if (rc != VMV_OK)
        {
            delete plans;
            return rc;
        }
        vmv::constraint_band_bounds(band, lower, span, dim);
        con.P = band.P;
        con.stretch = (constraint_settings->max_stretch > 0.f ? constraint_settings->max_stretch : 2.f) * settings->rrtc.range;
        return vmv::aorrtc_finish(robot, dim, envs, n_problems, starts, goals, halton_skips, *settings, plans, &con, out);
    }

    int vmv_plans_costs(const vmv_plans *plans, float *first_costs, float *costs, uint32_t *searches, uint32_t *improvements)
    {
        if (!plans || !plans->aorrtc) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = plans->n;
        if (first_costs && n) std::memcpy(first_costs, plans->first_costs.data(), n * 4);
        if (costs && n) std::memcpy(costs, plans->final_costs.data(), n * 4);
        if (searches && n) std::memcpy(searches, plans->searches.data(), n * 4);
        if (improvements && n) std::memcpy(improvements, plans->improvements.data(), n * 4);
        return VMV_OK;
    }

    int vmv_phs_samples(int robot, const float *start, const float *goal, float max_cost, uint32_t seed, uint32_t counter,
                        size_t n, float *out_q, uint8_t *out_in_bounds, uint32_t *out_counter)
    {
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!start || !goal || !out_counter || (n > 0 && (!out_q || !out_in_bounds)) || n >= (size_t{1} << 24))
            return VMV_ERR_INVALID_ARGUMENT;
        return vmv::phs_samples_run(robot, dim, start, goal, max_cost, seed, counter, n, out_q, out_in_bounds, out_counter);
    }
}
