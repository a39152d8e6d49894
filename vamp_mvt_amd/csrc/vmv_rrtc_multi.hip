// vmv_rrtc_multi.hip — lockstep RRT-Connect over many independent problems (vmv_rrtc_multi), and the same
// with goal sets, dynamic domain and start_tree_first (vmv_rrtc_multi_goals): one set of kernels serves both.
//
// Every problem is a state machine in device memory, advanced by the rounds of vmv_lockstep.h with one question per
// problem: rrtc_step_kernel (one workgroup per unfinished problem) consumes the answer to the problem's previous edge
// question, updates the trees, advances to the next question and writes that edge into the round's start / goal arrays.
//
// Arithmetic contract: fp32, one rounding per written operation (-ffp-contract=off; sqrtf and / are correctly rounded
// on gfx950), the nearest node is the FIRST of the least sqrtf(sum of squares in joint order).  The workgroup's lanes
// stride over the tree; that changes the order nodes are LOOKED at, not the result: the (distance, index) argmin is
// associative.  A problem's two trees share one pool of max_samples nodes, the start tree from the front and the goal
// tree from the back; the planner's two size rules keep |A| + |B| <= max_samples.  The pool's addressing, the nearest
// search and the path trace are vmv_two_trees.h's, shared with vmv_aorrtc_multi.
// Every store is a plain vector store by the owning workgroup; no atomics.
//
// Goal sets: the direct phase asks start -> goal g in order of g, one question per round; the goal tree then starts with
// all goals as roots (goal g at index g, its own parent), which the nearest search, the march and the trace take as they
// are.  Dynamic domain: a radius per node (radii, FLT_MAX = unset), tested after the nearest search of an iteration - a
// rejected sample asks nothing, so the step kernel draws again in the same launch - and updated when the extension's
// answer arrives; the march neither reads nor writes a radius.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"
#include "vmv_two_trees.h"

#include <cmath>
#include <cstring>

namespace vmv
{
    namespace
    {
        constexpr uint32_t kRrtcBlock = kTreeBlock;
        constexpr uint32_t kRrtcDefaultCheckEvery = 16;
        constexpr float kRadiusUnset = 3.402823466e+38f;  // FLT_MAX: a node no extension has failed from yet

        enum : uint32_t
        {
            kPhaseInit = 0,    // nothing asked yet
            kPhaseDirect = 1,  // start -> goal k is in flight
            kPhaseExtend = 2,  // near -> new is in flight (new sits in A's next slot, not yet counted)
            kPhaseMarch = 3,   // step k of the connect march is in flight (w sits in B's next slot, not yet counted)
            kPhaseDone = 4
        };

        struct RrtcState  // 64 bytes per problem
        {
            uint32_t phase, status, iterations, draws;
            uint32_t n[2];     // nodes of the start tree (side 0) and the goal tree (side 1)
            uint32_t a_side;   // which side the planner currently calls A
            uint32_t slot;     // position of the question in flight in its round's arrays
            uint32_t new_i;    // `new` in A (kNone on a direct solution)
            uint32_t bi, prev; // B's node nearest to `new`; last node of the march
            uint32_t k, n_steps;  // k: the march's step; in the direct phase the goal asked; once done, the goal a solved path ends in
            float bd;
            uint32_t path_len, questions;
        };
        static_assert(sizeof(RrtcState) == 64, "one cache line half per problem");

        struct RrtcParams
        {
            uint32_t dim, max_samples, max_iterations, balance;
            float range, tree_ratio;
            uint32_t dynamic_domain, start_tree_first;  // rrtc_settings.hh; both 0 for vmv_rrtc_multi
            float radius, alpha, min_radius;
            float lower[kPlanMaxDim], span[kPlanMaxDim];
        };

        struct RrtcArrays
        {
            RrtcState *state;          // [n_problems]
            float *pool;               // [n_problems][max_samples][dim]
            uint32_t *parent;          // [n_problems][max_samples], indices within the node's own tree
            float *radii;              // [n_problems][max_samples] with dynamic domain, else NULL
            const float *starts;       // [n_problems][dim]
            const float *goals;        // [n_goals][dim], problem p owns goals [goal_offsets[p], goal_offsets[p + 1])
            const uint32_t *goal_offsets;  // [n_problems + 1]; NULL = one goal per problem
            const uint64_t *skips;     // [n_problems]
            const uint32_t *active;    // [n_active] problem of each workgroup
            float *q_start, *q_goal;   // [n_active][dim] the round's questions
            const uint64_t *bits;      // answers of the previous round
            uint8_t *done;             // [n_problems]
            // vmv_rrtc_multi_constrained only, both NULL otherwise (exactly as radii): pending[a] = the pool element (over all
            // problems) of the node the question's far end was written to - A's next slot for an extension, B's next slot for
            // a march step - or kNoPending for a direct and for the null question; c_ok[slot] = the constraint round's answer
            // to the previous question, ANDed into the validity bit
            uint64_t *pending;         // [n_active]
            const uint8_t *c_ok;       // [n_active]
        };

        __device__ __forceinline__ uint32_t first_goal(const RrtcArrays &D, uint32_t p) { return D.goal_offsets ? D.goal_offsets[p] : p; }
        __device__ __forceinline__ uint32_t goal_count(const RrtcArrays &D, uint32_t p)
        {
            return D.goal_offsets ? D.goal_offsets[p + 1] - D.goal_offsets[p] : 1u;
        }

        __global__ __launch_bounds__(kRrtcBlock) void rrtc_init_kernel(const RrtcParams P, const RrtcArrays D, const uint32_t n)
        {
            const uint32_t p = blockIdx.x * kRrtcBlock + threadIdx.x;
            if (p >= n) return;
            const uint32_t M = P.max_samples, g0 = first_goal(D, p), G = goal_count(D, p);
            float *pool = D.pool + (size_t) p * M * P.dim;
            uint32_t *parent = D.parent + (size_t) p * M;
            init_roots(pool, parent, D.starts + (size_t) p * P.dim, D.goals + (size_t) g0 * P.dim, P.dim, M);
            for (uint32_t g = 1; g < G; ++g)  // the further goals of a set: roots 1 .. G - 1 of the goal tree
            {
                for (uint32_t j = 0; j < P.dim; ++j) pool[node_at(1, g, M) * P.dim + j] = D.goals[(size_t) (g0 + g) * P.dim + j];
                parent[node_at(1, g, M)] = g;
            }
            if (D.radii)
            {
                D.radii[(size_t) p * M + node_at(0, 0, M)] = kRadiusUnset;
                for (uint32_t g = 0; g < G; ++g) D.radii[(size_t) p * M + node_at(1, g, M)] = kRadiusUnset;
            }
            RrtcState st{};
            st.phase = kPhaseInit, st.status = VMV_PLAN_MAX_ITERATIONS;
            st.n[0] = st.n[1] = 1;  // (a direct solution reports [1, 1]; the goal tree counts its G roots once it is used)
            st.a_side = P.start_tree_first ? 1u : 0u;
            st.new_i = kNone;
            D.state[p] = st;
            D.done[p] = 0;
        }

        // One workgroup per active problem; every branch below is taken by the whole workgroup (its conditions are
        // values every thread holds alike), so the barriers and cross-lane reads inside nearest() are safe.
        __global__ __launch_bounds__(kRrtcBlock) void rrtc_step_kernel(const RrtcParams P, const RrtcArrays D)
        {
            __shared__ float s_t[kPlanMaxDim];
            __shared__ float s_rd[kTreeWaves];
            __shared__ uint32_t s_ri[kTreeWaves];
            const uint32_t a = blockIdx.x, p = D.active[a], tid = threadIdx.x, dim = P.dim, M = P.max_samples;
            RrtcState st = D.state[p];
            float *pool = D.pool + (size_t) p * M * dim;
            uint32_t *parent = D.parent + (size_t) p * M;
            float *qs = D.q_start + (size_t) a * dim, *qg = D.q_goal + (size_t) a * dim;
            float *radii = D.radii ? D.radii + (size_t) p * M : nullptr;
            const float *start = D.starts + (size_t) p * dim, *goals = D.goals + (size_t) first_goal(D, p) * dim;
            const float R = P.range;
            // the nearest node is the first of the least distance to s_t: the key is the distance itself
            const auto to_target = [&](const float *q, size_t) {
                const float d = tree_dist(q, s_t, dim);
                return Scored{true, d, d};
            };

            enum { kLoop, kMarchStep, kFinish } act = kLoop;
            if (st.phase == kPhaseDone)
                act = kFinish;
            else if (st.phase == kPhaseInit)
            {
                if (tid < dim) qs[tid] = start[tid], qg[tid] = goals[tid];
                st.phase = kPhaseDirect, st.slot = a, st.questions = 1, st.k = 0;
                if (tid == 0) D.state[p] = st;
                if (D.pending && tid == 0) D.pending[a] = kNoPending;
                return;
            }
            else
            {
                const bool ans = ((D.bits[st.slot >> 6] >> (st.slot & 63u)) & 1ull) && (!D.c_ok || D.c_ok[st.slot] != 0);
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                if (st.phase == kPhaseDirect)
                {
                    const uint32_t G = goal_count(D, p);
                    if (ans)
                        st.status = VMV_PLAN_SOLVED, st.new_i = kNone, act = kFinish;  // st.k is the goal
                    else if (++st.k < G)  // the next goal of the set, in the next round
                    {
                        if (tid < dim) qs[tid] = start[tid], qg[tid] = goals[(size_t) st.k * dim + tid];
                        st.slot = a, ++st.questions;
                        if (tid == 0) D.state[p] = st;
                        if (D.pending && tid == 0) D.pending[a] = kNoPending;
                        return;
                    }
                    else
                        st.n[1] = G;  // no goal is direct: every goal is a root of the goal tree
                }
                else if (st.phase == kPhaseExtend)
                {
                    if (radii && tid == 0)  // the node the extension left from is the parent of A's next slot
                    {
                        // The one radius store of this launch.  A failed extension falls through to the loop below, whose
                        // first sample is often nearest to this same node: the loop's barriers (after its target is
                        // written, and inside nearest()) lie between this store and every thread's read of radii there.
                        const size_t near_at = node_at(sa, parent[node_at(sa, count_of(st.n, sa), M)], M);
                        const float r = radii[near_at];
                        if (ans)
                        {
                            if (r != kRadiusUnset) radii[near_at] = r * (1.f + P.alpha);
                        }
                        else
                            radii[near_at] = r == kRadiusUnset ? P.radius : fmaxf(r * (1.f - P.alpha), P.min_radius);
                    }
                    if (ans)
                    {
                        st.new_i = grow(st.n, sa);
                        if (tid < dim) s_t[tid] = pool[node_at(sa, st.new_i, M) * dim + tid];
                        __syncthreads();
                        nearest<false>(pool, sb, count_of(st.n, sb), dim, M, to_target, s_rd, nullptr, s_ri, st.bd, st.bi);
                        if (st.bi == kNone) st.bi = 0, st.bd = NAN;  // a non-finite root: the march's first step is invalid
                        st.n_steps = march_steps(st.bd, R);
                        st.k = 0, st.prev = st.bi;
                        act = kMarchStep;
                    }
                }
                else  // kPhaseMarch
                {
                    if (ans)
                    {
                        st.prev = grow(st.n, sb);
                        if (++st.k == st.n_steps)
                            st.status = VMV_PLAN_SOLVED, act = kFinish;
                        else
                            act = kMarchStep;
                    }
                }
            }

            if (act == kMarchStep)
            {
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                if (st.n[0] + st.n[1] >= M)
                    act = kLoop;  // the pool is full: the march ends unconnected
                else
                {
                    if (tid < dim)
                    {
                        const float o = pool[node_at(sb, st.bi, M) * dim + tid], nw = pool[node_at(sa, st.new_i, M) * dim + tid];
                        float w = nw;
                        if (st.bd > 0.f) w = o + (nw - o) * (fminf((float) (st.k + 1u) * R, st.bd) / st.bd);
                        pool[node_at(sb, count_of(st.n, sb), M) * dim + tid] = w;
                        qs[tid] = pool[node_at(sb, st.prev, M) * dim + tid];
                        qg[tid] = w;
                    }
                    st.phase = kPhaseMarch, st.slot = a, ++st.questions;
                    if (tid == 0)
                    {
                        parent[node_at(sb, count_of(st.n, sb), M)] = st.prev, D.state[p] = st;
                        if (radii) radii[node_at(sb, count_of(st.n, sb), M)] = kRadiusUnset;
                        if (D.pending) D.pending[a] = (uint64_t) p * M + node_at(sb, count_of(st.n, sb), M);
                    }
                    return;
                }
            }

            if (act == kLoop)
            {
                const uint64_t skip = D.skips[p];
                for (;;)
                {
                    if (st.iterations >= P.max_iterations)
                    {
                        st.status = VMV_PLAN_MAX_ITERATIONS, act = kFinish;
                        break;
                    }
                    if (st.n[0] + st.n[1] >= M)
                    {
                        st.status = VMV_PLAN_MAX_SAMPLES, act = kFinish;
                        break;
                    }
                    ++st.iterations;
                    st.a_side = next_a_side(st.n, st.a_side, P.balance, P.tree_ratio);
                    ++st.draws;
                    if (tid < dim) s_t[tid] = halton_element(skip + st.draws, (int) tid, P.lower[tid], P.span[tid]);
                    __syncthreads();
                    const uint32_t sa = st.a_side;
                    float d;
                    uint32_t ni;
                    nearest<false>(pool, sa, count_of(st.n, sa), dim, M, to_target, s_rd, nullptr, s_ri, d, ni);
                    if (ni == kNone || !(d > 0.f)) continue;
                    // dynamic domain: the sample lies outside the nearest node's radius - the iteration and its draw are
                    // spent, nothing is asked (every thread reads the same word, so the branch is the workgroup's)
                    if (radii && radii[node_at(sa, ni, M)] < d) continue;
                    ask_extension(pool, node_at(sa, ni, M), node_at(sa, count_of(st.n, sa), M), dim, s_t, d, R, qs, qg);
                    st.phase = kPhaseExtend, st.slot = a, ++st.questions;
                    if (tid == 0)
                    {
                        parent[node_at(sa, count_of(st.n, sa), M)] = ni, D.state[p] = st;
                        if (radii) radii[node_at(sa, count_of(st.n, sa), M)] = kRadiusUnset;
                        if (D.pending) D.pending[a] = (uint64_t) p * M + node_at(sa, count_of(st.n, sa), M);
                    }
                    return;
                }
            }

            // finished (now or in an earlier round)
            ask_nothing(qs, qg, start, dim);
            if (D.pending && tid == 0) D.pending[a] = kNoPending;
            if (st.phase != kPhaseDone && tid == 0)
            {
                st.phase = kPhaseDone, st.slot = a;
                st.path_len = 0u;
                if (st.status == VMV_PLAN_SOLVED)  // a direct solution is (start, goal k)
                {
                    st.path_len = st.new_i == kNone ? 2u : trace_path(st.a_side, st.new_i, st.prev, pool, parent, dim, M, nullptr);
                    if (st.new_i != kNone)  // the goal is the root the goal tree's branch ends in
                    {
                        uint32_t i = st.a_side ? st.new_i : st.prev;
                        while (parent[node_at(1, i, M)] != i) i = parent[node_at(1, i, M)];
                        st.k = i;
                    }
                }
                D.state[p] = st;
                D.done[p] = 1;
            }
        }

        __global__ __launch_bounds__(kRrtcBlock) void rrtc_trace_kernel(const RrtcParams P, const RrtcArrays D, const uint32_t n,
                                                                         const uint64_t *__restrict__ offsets, float *__restrict__ paths)
        {
            const uint32_t p = blockIdx.x * kRrtcBlock + threadIdx.x;
            if (p >= n) return;
            const RrtcState st = D.state[p];
            if (st.phase != kPhaseDone || st.status != VMV_PLAN_SOLVED) return;
            float *out = paths + offsets[p] * P.dim;
            if (st.new_i == kNone)  // direct
                for (uint32_t j = 0; j < P.dim; ++j)
                    out[j] = D.starts[(size_t) p * P.dim + j], out[P.dim + j] = D.goals[(size_t) (first_goal(D, p) + st.k) * P.dim + j];
            else
                (void) trace_path(st.a_side, st.new_i, st.prev, D.pool + (size_t) p * P.max_samples * P.dim,
                                  D.parent + (size_t) p * P.max_samples, P.dim, P.max_samples, out);
        }

        // vmv_rrtc_multi_constrained: what a round needs beside the step kernel - the resolved settings, the records on the
        // device (one, or one per problem of the run) and max_stretch * range
        struct ConstraintRound
        {
            ConstraintParams P;
            const ConstraintDev *d_cons;
            float stretch;
        };

    // The caller has checked every argument, n > 0, and every environment is finalized on the current device with the
    // robot's part built.  lower / span: the robot's joint bounds (Robot::s_a, s_m).  goal_offsets: NULL = goals is
    // [n][dim], one goal per problem.  `call` names the entry point in vmv_last_error().
    int rrtc_multi_run(int robot, int dim, const float *lower, const float *span, const vmv_env *const *envs, size_t n,
                       const float *starts, const float *goals, const size_t *goal_offsets, const uint64_t *skips,
                       const vmv_rrtc_goals_settings &GS, const char *call, vmv_plans *plans, const ConstraintRound *cr = nullptr)
    {
        const vmv_rrtc_settings &S = GS.base;
        RrtcParams P{};
        P.dim = (uint32_t) dim, P.max_samples = S.max_samples, P.max_iterations = S.max_iterations;
        P.balance = S.balance ? 1u : 0u, P.range = S.range, P.tree_ratio = S.tree_ratio;
        P.dynamic_domain = GS.dynamic_domain ? 1u : 0u, P.start_tree_first = GS.start_tree_first ? 1u : 0u;
        P.radius = GS.radius, P.alpha = GS.alpha, P.min_radius = GS.min_radius;
        for (int j = 0; j < dim; ++j) P.lower[j] = lower[j], P.span[j] = span[j];
        const uint32_t check_every = S.check_every ? S.check_every : kRrtcDefaultCheckEvery;
        hipStream_t stream = nullptr;

        DeviceBuffers mem;
        LockstepBuffers B;
        RrtcArrays D{};
        VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.pool, n * (size_t) S.max_samples * (size_t) dim));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.parent, n * (size_t) S.max_samples));
        if (int rc = B.alloc(mem, n, n, 1, (size_t) dim, stream); rc != VMV_OK) return rc;
        if (P.dynamic_domain) VMV_LOCKSTEP_HIP(mem.alloc(&D.radii, n * (size_t) S.max_samples));
        uint8_t *d_c_ok = nullptr;
        uint32_t *d_refused = nullptr;
        if (cr)
        {
            VMV_LOCKSTEP_HIP(mem.alloc(&d_refused, n));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(d_refused, 0, std::max<size_t>(n * 4, 16), stream));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.pending, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_c_ok, n));
            D.c_ok = d_c_ok;
        }
        size_t max_goals = 1;  // of one problem: its direct questions
        if (!goal_offsets)
        {
            if (int rc = upload_problems(mem, n, (size_t) dim, starts, goals, skips, stream, &D.starts, &D.goals, &D.skips); rc != VMV_OK)
                return rc;
        }
        else
        {
            std::vector<uint32_t> offsets32(n + 1);
            for (size_t k = 0; k <= n; ++k) offsets32[k] = (uint32_t) goal_offsets[k];
            for (size_t k = 0; k < n; ++k) max_goals = std::max(max_goals, goal_offsets[k + 1] - goal_offsets[k]);
            float *d_starts = nullptr, *d_goals = nullptr;
            uint32_t *d_offsets = nullptr;
            uint64_t *d_skips = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_starts, n * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_goals, goal_offsets[n] * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_offsets, n + 1));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_skips, n));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_starts, starts, n * (size_t) dim * 4, hipMemcpyHostToDevice));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_goals, goals, goal_offsets[n] * (size_t) dim * 4, hipMemcpyHostToDevice));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_offsets, offsets32.data(), (n + 1) * 4, hipMemcpyHostToDevice));
            if (int rc = upload_skips(d_skips, skips, n, stream); rc != VMV_OK) return rc;
            D.starts = d_starts, D.goals = d_goals, D.goal_offsets = d_offsets, D.skips = d_skips;
        }
        D.active = B.active, D.q_start = B.q_start, D.q_goal = B.q_goal, D.bits = B.bits, D.done = B.done;
        const uint32_t n32 = (uint32_t) n;
        hipLaunchKernelGGL(rrtc_init_kernel, dim3((n32 + kRrtcBlock - 1) / kRrtcBlock), dim3(kRrtcBlock), 0, stream, P, D, n32);
        VMV_LOCKSTEP_HIP(hipGetLastError());

        std::vector<uint32_t> active(n);
        std::vector<const vmv_env *> active_envs(envs, envs + n);
        for (size_t k = 0; k < n; ++k) active[k] = (uint32_t) k;
        VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active.data(), n * 4, hipMemcpyHostToDevice));

        // every problem ends within G + max_iterations + max_samples questions (each question after the G direct ones belongs
        // to a new iteration or adds a node): a bound on the rounds that does not depend on the device's answers
        const uint64_t max_rounds = 1ull + max_goals + (uint64_t) S.max_iterations + (uint64_t) S.max_samples + check_every;
        uint64_t rounds = 0;
        const auto step = [&](uint32_t na) {
            hipLaunchKernelGGL(rrtc_step_kernel, dim3(na), dim3(kRrtcBlock), 0, stream, P, D);
            if (cr)  // the pending node projected and written back, the edge's band test: before the round's validation
                (void) robot_launchers(robot).constraint_round(cr->P, cr->d_cons, B.active, B.q_start, B.q_goal, D.pending, D.pool,
                                                               cr->stretch, d_c_ok, d_refused, na, stream);
        };
        if (int rc = lockstep_rounds(robot, stream, check_every, max_rounds, 1, active, active_envs, B.arrays(), call,
                                     "rrtc_step_kernel", step, rounds);
            rc != VMV_OK)
            return rc;

        // results: the states, then the paths traced on the device into one packed buffer
        std::vector<RrtcState> states(n);
        VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(RrtcState), hipMemcpyDeviceToHost));
        plans->n = n, plans->dim = dim, plans->rounds = rounds, plans->questions = 0;
        plans->status.resize(n), plans->iterations.resize(n), plans->sizes2.resize(2 * n), plans->path_lengths.resize(n);
        plans->goal_indices.resize(n);
        if (cr)
        {
            plans->band_refused.resize(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(plans->band_refused.data(), d_refused, n * 4, hipMemcpyDeviceToHost));
        }
        for (size_t k = 0; k < n; ++k)
        {
            const RrtcState &st = states[k];
            plans->goal_indices[k] = st.status == VMV_PLAN_SOLVED ? st.k : UINT32_MAX;
            plans->status[k] = (uint8_t) st.status;
            plans->iterations[k] = st.iterations;
            plans->sizes2[2 * k] = st.n[st.a_side], plans->sizes2[2 * k + 1] = st.n[st.a_side ^ 1u];
            plans->path_lengths[k] = st.path_len;
            plans->questions += st.questions;
        }
        return pack_paths(mem, B.path_offsets, plans->path_lengths, (size_t) dim, nullptr, "rrtc_trace_kernel",
                          [&](const uint64_t *d_offsets, float *d_paths) {
                              hipLaunchKernelGGL(rrtc_trace_kernel, dim3((n32 + kRrtcBlock - 1) / kRrtcBlock), dim3(kRrtcBlock), 0, stream,
                                                 P, D, n32, d_offsets, d_paths);
                          },
                          plans->paths);
    }
    // vmv_rrtc_multi's checks in its order, then those of the goal table and of the dynamic domain's values
    int check_goals_call(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                         const size_t *goal_offsets, const uint64_t *halton_skips, const vmv_rrtc_goals_settings *settings, vmv_plans **out,
                         int *dim_out)
    {
        int dim = 0;
        if (int rc = check_planner_call(robot, settings, out, envs, n_problems, starts, goals, &dim); rc != VMV_OK) return rc;
        const vmv_rrtc_settings &base = settings->base;
        if (!std::isfinite(base.range) || !(base.range > 0.f) || base.max_samples < 2) return VMV_ERR_INVALID_ARGUMENT;
        if (!halton_skips_ok(halton_skips, n_problems, base.max_iterations)) return VMV_ERR_INVALID_ARGUMENT;
        if (goal_offsets && n_problems > 0)
        {
            if (goal_offsets[0] != 0) return VMV_ERR_INVALID_ARGUMENT;
            for (size_t k = 0; k < n_problems; ++k)
            {
                if (goal_offsets[k + 1] <= goal_offsets[k]) return VMV_ERR_INVALID_ARGUMENT;  // decreasing, or an empty set
                if (goal_offsets[k + 1] - goal_offsets[k] > (size_t) base.max_samples - 1) return VMV_ERR_INVALID_ARGUMENT;
            }
            if (goal_offsets[n_problems] >= (1ull << 31)) return VMV_ERR_INVALID_ARGUMENT;
        }
        if (settings->dynamic_domain)
        {
            if (!std::isfinite(settings->radius) || !(settings->radius > 0.f)) return VMV_ERR_INVALID_ARGUMENT;
            if (!std::isfinite(settings->min_radius) || !(settings->min_radius > 0.f)) return VMV_ERR_INVALID_ARGUMENT;
            if (!std::isfinite(settings->alpha) || !(settings->alpha >= 0.f) || !(settings->alpha < 1.f)) return VMV_ERR_INVALID_ARGUMENT;
        }
        *dim_out = dim;
        return VMV_OK;
    }

    // vmv_rrtc_multi_constrained behind its checks: ONE constraint_check launch over all starts and goals; a problem whose
    // start is out of band or that has no in-band goal ends VMV_PLAN_INVALID_ENDPOINT and takes no part; the others run
    // as a call of their own (a problem's result is its own) with their in-band goals, the round kernel in every round.
    int rrtc_constrained_run(int robot, int dim, const vmv_env *const *envs, size_t n, const float *starts, const float *goals,
                             const size_t *goal_offsets, const uint64_t *skips, const vmv_rrtc_goals_settings &GS,
                             ConstraintBand band, float max_stretch, vmv_plans *plans)
    {
        float lower[16], span[16], descale[16];
        if (int rc = vmv_robot_bounds(robot, lower, span, descale); rc != VMV_OK) return rc;
        constraint_band_bounds(band, lower, span, dim);
        const ConstraintParams &CP = band.P;
        const RobotLaunchers &L = robot_launchers(robot);
        hipStream_t stream = nullptr;
        std::vector<ConstraintDev> recs(band.count);
        constraint_band_records(band, recs.data());
        const auto first = [&](size_t p) { return goal_offsets ? goal_offsets[p] : p; };
        const size_t G = first(n), lanes = n + G;

        // ---- the endpoints' band test: lanes [0, n) the starts, [n, n + G) the goals, each with its problem's record
        std::vector<uint64_t> bits((lanes + 63) / 64);
        {
            DeviceBuffers mem;
            float *d_q = nullptr;
            ConstraintDev *d_recs = nullptr;
            uint64_t *d_bits = nullptr;
            std::vector<uint32_t> owner(CP.shared ? 0 : lanes);  // of a lane: its problem
            for (size_t p = 0; p < n && !CP.shared; ++p)
            {
                owner[p] = (uint32_t) p;
                for (size_t g = first(p); g < first(p + 1); ++g) owner[n + g] = (uint32_t) p;
            }
            const std::vector<ConstraintDev> up = CP.shared ? recs : constraint_band_expand(recs.data(), owner);
            VMV_LOCKSTEP_HIP(mem.alloc(&d_q, lanes * (size_t) dim));
            if (int rc = upload_records(mem, up.data(), up.size(), &d_recs); rc != VMV_OK) return rc;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_bits, bits.size()));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_q, starts, n * (size_t) dim * 4, hipMemcpyHostToDevice));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_q + n * (size_t) dim, goals, G * (size_t) dim * 4, hipMemcpyHostToDevice));
            if (int rc = L.constraint_check(CP, d_recs, d_q, lanes, d_bits, nullptr, stream); rc != VMV_OK) return rc;
            VMV_LOCKSTEP_HIP(hipMemcpy(bits.data(), d_bits, bits.size() * 8, hipMemcpyDeviceToHost));
        }
        const auto in_band = [&](size_t lane) { return ((bits[lane >> 6] >> (lane & 63u)) & 1ull) != 0; };

        // ---- the problems that take part, with their in-band goals (goal_of: the goal's index within its own set)
        std::vector<size_t> kept, offsets(1, 0);
        std::vector<uint32_t> goal_of, kept_owner;
        std::vector<float> k_starts, k_goals;
        std::vector<uint64_t> k_skips;
        std::vector<const vmv_env *> k_envs;
        for (size_t p = 0; p < n; ++p)
        {
            const size_t before = goal_of.size();
            for (size_t g = first(p); in_band(p) && g < first(p + 1); ++g)
                if (in_band(n + g))
                {
                    goal_of.push_back((uint32_t) (g - first(p)));
                    k_goals.insert(k_goals.end(), goals + g * (size_t) dim, goals + (g + 1) * (size_t) dim);
                }
            if (goal_of.size() == before) continue;
            kept.push_back(p), offsets.push_back(goal_of.size()), k_envs.push_back(envs[p]);
            k_starts.insert(k_starts.end(), starts + p * (size_t) dim, starts + (p + 1) * (size_t) dim);
            if (skips) k_skips.push_back(skips[p]);
            kept_owner.push_back((uint32_t) p);
        }
        plans->n = n, plans->dim = dim, plans->rounds = 0, plans->questions = 0;
        plans->status.assign(n, (uint8_t) VMV_PLAN_INVALID_ENDPOINT), plans->iterations.assign(n, 0u), plans->sizes2.assign(2 * n, 0u);
        plans->path_lengths.assign(n, 0u), plans->goal_indices.assign(n, UINT32_MAX), plans->paths.clear();
        plans->band_refused.assign(n, 0u);
        if (kept.empty()) return VMV_OK;

        DeviceBuffers mem;
        ConstraintDev *d_recs = nullptr;
        const std::vector<ConstraintDev> up = CP.shared ? recs : constraint_band_expand(recs.data(), kept_owner);
        if (int rc = upload_records(mem, up.data(), up.size(), &d_recs); rc != VMV_OK) return rc;
        const ConstraintRound cr{CP, d_recs, max_stretch * GS.base.range};
        vmv_plans sub;
        if (int rc = rrtc_multi_run(robot, dim, lower, span, k_envs.data(), kept.size(), k_starts.data(), k_goals.data(), offsets.data(),
                                    skips ? k_skips.data() : nullptr, GS, "vmv_rrtc_multi_constrained", &sub, &cr);
            rc != VMV_OK)
            return rc;
        for (size_t k = 0; k < kept.size(); ++k)  // (the others have no waypoints: the packed paths are the run's as they are)
        {
            const size_t p = kept[k];
            plans->status[p] = sub.status[k], plans->iterations[p] = sub.iterations[k], plans->path_lengths[p] = sub.path_lengths[k];
            plans->sizes2[2 * p] = sub.sizes2[2 * k], plans->sizes2[2 * p + 1] = sub.sizes2[2 * k + 1];
            if (sub.goal_indices[k] != UINT32_MAX) plans->goal_indices[p] = goal_of[offsets[k] + sub.goal_indices[k]];
            plans->band_refused[p] = sub.band_refused[k];
        }
        plans->paths = std::move(sub.paths), plans->rounds = sub.rounds, plans->questions = sub.questions;
        return VMV_OK;
    }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_rrtc_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                       const uint64_t *halton_skips, const vmv_rrtc_settings *settings, vmv_plans **out)
    {
        // device-free checks first; the environments' own (NULL handles again, unfinalized, another device) are those of
        // vmv_env_prepare_multi, which then builds the parts not yet built in one batch
        int dim = 0;
        if (int rc = vmv::check_planner_call(robot, settings, out, envs, n_problems, starts, goals, &dim); rc != VMV_OK) return rc;
        if (!std::isfinite(settings->range) || !(settings->range > 0.f) || settings->max_samples < 2) return VMV_ERR_INVALID_ARGUMENT;
        if (!vmv::halton_skips_ok(halton_skips, n_problems, settings->max_iterations)) return VMV_ERR_INVALID_ARGUMENT;
        return vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            vmv_rrtc_goals_settings all{};  // the additions off
            all.base = *settings;
            return vmv::rrtc_multi_run(robot, dim, lower, span, envs, n_problems, starts, goals, nullptr, halton_skips, all,
                                       "vmv_rrtc_multi", plans);
        });
    }

    int vmv_rrtc_multi_goals(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                             const size_t *goal_offsets, const uint64_t *halton_skips, const vmv_rrtc_goals_settings *settings,
                             vmv_plans **out)
    {
        int dim = 0;
        if (int rc = vmv::check_goals_call(robot, envs, n_problems, starts, goals, goal_offsets, halton_skips, settings, out, &dim); rc != VMV_OK)
            return rc;
        const int rc = vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            return vmv::rrtc_multi_run(robot, dim, lower, span, envs, n_problems, starts, goals, goal_offsets, halton_skips, *settings,
                                       "vmv_rrtc_multi_goals", plans);
        });
        if (rc == VMV_OK) (*out)->rrtc_goals = true;
        return rc;
    }

    int vmv_rrtc_multi_constrained(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                                   const size_t *goal_offsets, const uint64_t *halton_skips, const vmv_rrtc_goals_settings *settings,
                                   const vmv_ee_constraint *constraints, size_t n_constraints,
                                   const vmv_constraint_plan_settings *constraint_settings, vmv_plans **out)
    {
        // vmv_rrtc_multi_goals's checks in its order, then the constraint's own; none needs a device
        int dim = 0;
        if (int rc = vmv::check_goals_call(robot, envs, n_problems, starts, goals, goal_offsets, halton_skips, settings, out, &dim); rc != VMV_OK)
            return rc;
        const float ms = constraint_settings ? constraint_settings->max_stretch : 0.f;
        vmv::ConstraintBand band{};
        const std::string err = vmv::constraint_band_checks(
            constraints, n_constraints, constraint_settings ? &constraint_settings->base : nullptr, n_problems, "n_problems",
            std::isfinite(ms) && ms >= 0.f ? nullptr : "max_stretch must be finite and not negative (0 = default)", band);
        if (!err.empty()) return vmv::refuse_argument(err.c_str());
        const int rc = vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            return vmv::rrtc_constrained_run(robot, dim, envs, n_problems, starts, goals, goal_offsets, halton_skips, *settings, band,
                                             ms > 0.f ? ms : 2.f, plans);
        });
        if (rc == VMV_OK) (*out)->rrtc_goals = (*out)->constrained = true, (*out)->band_refused.resize(n_problems);
        return rc;
    }

    int vmv_plans_band_refused(const vmv_plans *plans, uint32_t *refused)
    {
        if (!plans || !plans->constrained) return VMV_ERR_INVALID_ARGUMENT;
        if (refused && plans->n) std::memcpy(refused, plans->band_refused.data(), plans->n * 4);
        return VMV_OK;
    }

    int vmv_plans_goal_indices(const vmv_plans *plans, uint32_t *goal_index)
    {
        if (!plans || !plans->rrtc_goals) return VMV_ERR_INVALID_ARGUMENT;
        if (goal_index && plans->n) std::memcpy(goal_index, plans->goal_indices.data(), plans->n * 4);
        return VMV_OK;
    }

    int vmv_plans_summary(const vmv_plans *plans, uint8_t *status, uint32_t *iterations, uint32_t *sizes2, uint32_t *path_lengths,
                          uint64_t *rounds, uint64_t *questions)
    {
        if (!plans) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = plans->n;
        if (status && n) std::memcpy(status, plans->status.data(), n);
        if (iterations && n) std::memcpy(iterations, plans->iterations.data(), n * 4);
        if (sizes2 && n) std::memcpy(sizes2, plans->sizes2.data(), 2 * n * 4);
        if (path_lengths && n) std::memcpy(path_lengths, plans->path_lengths.data(), n * 4);
        if (rounds) *rounds = plans->rounds;
        if (questions) *questions = plans->questions;
        return VMV_OK;
    }

    int vmv_plans_paths(const vmv_plans *plans, float *out, size_t capacity_floats)
    {
        if (!plans || (!out && !plans->paths.empty())) return VMV_ERR_INVALID_ARGUMENT;
        if (capacity_floats < plans->paths.size()) return VMV_ERR_CAPACITY;
        if (!plans->paths.empty()) std::memcpy(out, plans->paths.data(), plans->paths.size() * 4);
        return VMV_OK;
    }

    int vmv_plans_destroy(vmv_plans *plans)
    {
        if (!plans) return VMV_ERR_INVALID_ARGUMENT;
        delete plans;
        return VMV_OK;
    }
}
