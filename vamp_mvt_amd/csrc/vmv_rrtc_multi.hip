// vmv_rrtc_multi.hip — lockstep RRT-Connect over many independent problems (vmv_rrtc_multi).
//
// Every problem is a state machine in device memory, advanced by the rounds of vmv_lockstep.h with one question per
// problem: rrtc_step_kernel (one workgroup per unfinished problem) consumes the answer to the problem's previous edge
// question, updates the trees, advances to the next question and writes that edge into the round's start / goal arrays.
//
// Arithmetic contract: fp32, one rounding per written operation (-ffp-contract=off; sqrtf and / are correctly rounded
// on gfx950), the nearest node is the FIRST of the least sqrtf(sum of squares in joint order).  The workgroup's lanes
// stride over the tree; that changes the order nodes are LOOKED at, not the result: the (distance, index) argmin is
// associative.  A problem's two trees share one pool of max_samples nodes, the start tree from the front and the goal
// tree from the back; the planner's two size rules keep |A| + |B| <= max_samples.
// Every store is a plain vector store by the owning workgroup; no atomics.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"

#include <cmath>
#include <cstring>

namespace vmv
{
    namespace
    {
        constexpr uint32_t kRrtcBlock = 256;
        constexpr uint32_t kRrtcWaves = kRrtcBlock / kWave;
        constexpr uint32_t kRrtcMaxDim = 16;
        constexpr uint32_t kRrtcDefaultCheckEvery = 16;
        constexpr uint32_t kNone = 0xffffffffu;

        enum : uint32_t
        {
            kPhaseInit = 0,    // nothing asked yet
            kPhaseDirect = 1,  // start -> goal is in flight
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
            uint32_t k, n_steps;
            float bd;
            uint32_t path_len, questions;
        };
        static_assert(sizeof(RrtcState) == 64, "one cache line half per problem");

        struct RrtcParams
        {
            uint32_t dim, max_samples, max_iterations, balance;
            float range, tree_ratio;
            float lower[kRrtcMaxDim], span[kRrtcMaxDim];
        };

        struct RrtcArrays
        {
            RrtcState *state;          // [n_problems]
            float *pool;               // [n_problems][max_samples][dim]
            uint32_t *parent;          // [n_problems][max_samples], indices within the node's own tree
            const float *starts, *goals;  // [n_problems][dim]
            const uint64_t *skips;     // [n_problems]
            const uint32_t *active;    // [n_active] problem of each workgroup
            float *q_start, *q_goal;   // [n_active][dim] the round's questions
            const uint64_t *bits;      // answers of the previous round
            uint8_t *done;             // [n_problems]
        };

        __device__ __forceinline__ size_t node_at(uint32_t side, uint32_t i, uint32_t max_samples)
        {
            return side ? (size_t) (max_samples - 1u - i) : (size_t) i;
        }

        // nodes of one side's tree; constant subscripts only, so that the state stays in registers
        __device__ __forceinline__ uint32_t count_of(const RrtcState &st, uint32_t side) { return side ? st.n[1] : st.n[0]; }
        __device__ __forceinline__ uint32_t grow(RrtcState &st, uint32_t side)  // -> index of the node now counted
        {
            const uint32_t i = count_of(st, side);
            if (side)
                st.n[1] = i + 1u;
            else
                st.n[0] = i + 1u;
            return i;
        }

        __device__ __forceinline__ bool closer(float d, uint32_t i, float best_d, uint32_t best_i)
        {
            return d < best_d || (d == best_d && i < best_i);
        }

        // (first index with the least distance to s_t, that distance) over nodes [0, count) of one tree; the same
        // values in every thread.  Called by all threads of the workgroup (barriers, cross-lane reads with every lane
        // enabled).  kNone where no distance compares below +inf (a non-finite root).
        __device__ void nearest(const float *__restrict__ pool, const uint32_t side, const uint32_t count, const RrtcParams &P,
                                const float *s_t, float *s_rd, uint32_t *s_ri, float &out_d, uint32_t &out_i)
        {
            float best_d = INFINITY;
            uint32_t best_i = kNone;
            for (uint32_t i = threadIdx.x; i < count; i += kRrtcBlock)  // increasing i per lane: `<` keeps the first
            {
                const float *q = pool + node_at(side, i, P.max_samples) * P.dim;
                float sum = 0.f;
                for (uint32_t j = 0; j < P.dim; ++j)
                {
                    const float df = q[j] - s_t[j];
                    sum = sum + df * df;
                }
                const float d = sqrtf(sum);
                if (d < best_d) best_d = d, best_i = i;
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1)  // (all 64 lanes are enabled here: the loop above has ended)
            {
                const float od = __shfl_xor(best_d, off);
                const uint32_t oi = (uint32_t) __shfl_xor((int) best_i, off);
                if (closer(od, oi, best_d, best_i)) best_d = od, best_i = oi;
            }
            if ((threadIdx.x & (kWave - 1)) == 0) s_rd[threadIdx.x / kWave] = best_d, s_ri[threadIdx.x / kWave] = best_i;
            __syncthreads();
            best_d = s_rd[0], best_i = s_ri[0];
#pragma unroll
            for (uint32_t w = 1; w < kRrtcWaves; ++w)
                if (closer(s_rd[w], s_ri[w], best_d, best_i)) best_d = s_rd[w], best_i = s_ri[w];
            __syncthreads();  // s_rd / s_ri / s_t may be rewritten after this
            out_d = best_d, out_i = best_i;
        }

        // waypoints of a solved problem: root(A) .. new, then B_prev .. root(B) without its first node if that equals
        // `new` bit for bit; one thread.  out == nullptr: count only.
        __device__ uint32_t trace_path(const RrtcState &st, const float *pool, const uint32_t *parent, const RrtcParams &P,
                                       const float *start, const float *goal, float *out)
        {
            const uint32_t dim = P.dim;
            if (st.new_i == kNone)  // direct
            {
                if (out)
                    for (uint32_t j = 0; j < dim; ++j) out[j] = start[j], out[dim + j] = goal[j];
                return 2;
            }
            const uint32_t sa = st.a_side, sb = sa ^ 1u;
            uint32_t la = 1, lb = 1;
            for (uint32_t i = st.new_i; parent[node_at(sa, i, P.max_samples)] != i; i = parent[node_at(sa, i, P.max_samples)]) ++la;
            for (uint32_t i = st.prev; parent[node_at(sb, i, P.max_samples)] != i; i = parent[node_at(sb, i, P.max_samples)]) ++lb;
            const uint32_t *pn = reinterpret_cast<const uint32_t *>(pool + node_at(sa, st.new_i, P.max_samples) * dim);
            const uint32_t *pp = reinterpret_cast<const uint32_t *>(pool + node_at(sb, st.prev, P.max_samples) * dim);
            bool same = true;
            for (uint32_t j = 0; j < dim; ++j) same = same && pn[j] == pp[j];
            const uint32_t skip = same ? 1u : 0u, len = la + lb - skip;
            if (!out) return len;
            const bool reversed = sa != 0;  // A is the goal tree: the path was collected goal -> start
            uint32_t pos = la;              // pa is written backwards from position la - 1
            for (uint32_t i = st.new_i;; i = parent[node_at(sa, i, P.max_samples)])
            {
                --pos;
                const float *q = pool + node_at(sa, i, P.max_samples) * dim;
                float *o = out + (size_t) (reversed ? len - 1u - pos : pos) * dim;
                for (uint32_t j = 0; j < dim; ++j) o[j] = q[j];
                if (parent[node_at(sa, i, P.max_samples)] == i) break;
            }
            pos = la;
            uint32_t seen = 0;
            for (uint32_t i = st.prev;; i = parent[node_at(sb, i, P.max_samples)], ++seen)
            {
                if (seen >= skip)
                {
                    const float *q = pool + node_at(sb, i, P.max_samples) * dim;
                    float *o = out + (size_t) (reversed ? len - 1u - pos : pos) * dim;
                    for (uint32_t j = 0; j < dim; ++j) o[j] = q[j];
                    ++pos;
                }
                if (parent[node_at(sb, i, P.max_samples)] == i) break;
            }
            return len;
        }

        __global__ __launch_bounds__(kRrtcBlock) void rrtc_init_kernel(const RrtcParams P, const RrtcArrays D, const uint32_t n)
        {
            const uint32_t p = blockIdx.x * kRrtcBlock + threadIdx.x;
            if (p >= n) return;
            float *pool = D.pool + (size_t) p * P.max_samples * P.dim;
            uint32_t *parent = D.parent + (size_t) p * P.max_samples;
            for (uint32_t j = 0; j < P.dim; ++j)
            {
                pool[node_at(0, 0, P.max_samples) * P.dim + j] = D.starts[(size_t) p * P.dim + j];
                pool[node_at(1, 0, P.max_samples) * P.dim + j] = D.goals[(size_t) p * P.dim + j];
            }
            parent[node_at(0, 0, P.max_samples)] = 0;  // roots are their own parent
            parent[node_at(1, 0, P.max_samples)] = 0;
            RrtcState st{};
            st.phase = kPhaseInit, st.status = VMV_PLAN_MAX_ITERATIONS;
            st.n[0] = st.n[1] = 1;
            st.new_i = kNone;
            D.state[p] = st;
            D.done[p] = 0;
        }

        // One workgroup per active problem; every branch below is taken by the whole workgroup (its conditions are
        // values every thread holds alike), so the barriers and cross-lane reads inside nearest() are safe.
        __global__ __launch_bounds__(kRrtcBlock) void rrtc_step_kernel(const RrtcParams P, const RrtcArrays D)
        {
            __shared__ float s_t[kRrtcMaxDim];
            __shared__ float s_rd[kRrtcWaves];
            __shared__ uint32_t s_ri[kRrtcWaves];
            const uint32_t a = blockIdx.x, p = D.active[a], tid = threadIdx.x, dim = P.dim, M = P.max_samples;
            RrtcState st = D.state[p];
            float *pool = D.pool + (size_t) p * M * dim;
            uint32_t *parent = D.parent + (size_t) p * M;
            float *qs = D.q_start + (size_t) a * dim, *qg = D.q_goal + (size_t) a * dim;
            const float *start = D.starts + (size_t) p * dim, *goal = D.goals + (size_t) p * dim;
            const float R = P.range;

            enum { kLoop, kMarchStep, kFinish } act = kLoop;
            if (st.phase == kPhaseDone)
                act = kFinish;
            else if (st.phase == kPhaseInit)
            {
                if (tid < dim) qs[tid] = start[tid], qg[tid] = goal[tid];
                st.phase = kPhaseDirect, st.slot = a, st.questions = 1;
                if (tid == 0) D.state[p] = st;
                return;
            }
            else
            {
                const bool ans = (D.bits[st.slot >> 6] >> (st.slot & 63u)) & 1ull;
                const uint32_t sa = st.a_side, sb = sa ^ 1u;
                if (st.phase == kPhaseDirect)
                {
                    if (ans) st.status = VMV_PLAN_SOLVED, st.new_i = kNone, act = kFinish;
                }
                else if (st.phase == kPhaseExtend)
                {
                    if (ans)
                    {
                        st.new_i = grow(st, sa);
                        if (tid < dim) s_t[tid] = pool[node_at(sa, st.new_i, M) * dim + tid];
                        __syncthreads();
                        nearest(pool, sb, count_of(st, sb), P, s_t, s_rd, s_ri, st.bd, st.bi);
                        if (st.bi == kNone) st.bi = 0, st.bd = NAN;  // a non-finite root: the march's first step is invalid
                        const float c = ceilf(st.bd / R);
                        st.n_steps = (c >= 1.f && c < 2147483648.f) ? (uint32_t) c : 1u;
                        st.k = 0, st.prev = st.bi;
                        act = kMarchStep;
                    }
                }
                else  // kPhaseMarch
                {
                    if (ans)
                    {
                        st.prev = grow(st, sb);
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
                        pool[node_at(sb, count_of(st, sb), M) * dim + tid] = w;
                        qs[tid] = pool[node_at(sb, st.prev, M) * dim + tid];
                        qg[tid] = w;
                    }
                    st.phase = kPhaseMarch, st.slot = a, ++st.questions;
                    if (tid == 0) parent[node_at(sb, count_of(st, sb), M)] = st.prev, D.state[p] = st;
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
                    {
                        const float na = (float) count_of(st, st.a_side), nb = (float) count_of(st, st.a_side ^ 1u);
                        if (!P.balance || fabsf(na - nb) / na < P.tree_ratio) st.a_side ^= 1u;
                    }
                    ++st.draws;
                    if (tid < dim) s_t[tid] = halton_element(skip + st.draws, (int) tid, P.lower[tid], P.span[tid]);
                    __syncthreads();
                    const uint32_t sa = st.a_side;
                    float d;
                    uint32_t ni;
                    nearest(pool, sa, count_of(st, sa), P, s_t, s_rd, s_ri, d, ni);
                    if (ni == kNone || !(d > 0.f)) continue;
                    const float s = fminf(d, R) / d;
                    if (tid < dim)
                    {
                        const float near = pool[node_at(sa, ni, M) * dim + tid];
                        const float nw = near + (s_t[tid] - near) * s;
                        pool[node_at(sa, count_of(st, sa), M) * dim + tid] = nw;
                        qs[tid] = near;
                        qg[tid] = nw;
                    }
                    st.phase = kPhaseExtend, st.slot = a, ++st.questions;
                    if (tid == 0) parent[node_at(sa, count_of(st, sa), M)] = ni, D.state[p] = st;
                    return;
                }
            }

            // finished (now or in an earlier round): the null question start -> start, its answer is ignored
            if (tid < dim) qs[tid] = start[tid], qg[tid] = start[tid];
            if (st.phase != kPhaseDone && tid == 0)
            {
                st.phase = kPhaseDone, st.slot = a;
                st.path_len = st.status == VMV_PLAN_SOLVED ? trace_path(st, pool, parent, P, start, goal, nullptr) : 0u;
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
            (void) trace_path(st, D.pool + (size_t) p * P.max_samples * P.dim, D.parent + (size_t) p * P.max_samples, P,
                              D.starts + (size_t) p * P.dim, D.goals + (size_t) p * P.dim, paths + offsets[p] * P.dim);
        }

    // The caller has checked every argument, n > 0, and every environment is finalized on the current device with the
    // robot's part built.  lower / span: the robot's joint bounds (Robot::s_a, s_m).
    int rrtc_multi_run(int robot, int dim, const float *lower, const float *span, const vmv_env *const *envs, size_t n,
                       const float *starts, const float *goals, const uint64_t *skips, const vmv_rrtc_settings &S,
                       vmv_plans *plans)
    {
        RrtcParams P{};
        P.dim = (uint32_t) dim, P.max_samples = S.max_samples, P.max_iterations = S.max_iterations;
        P.balance = S.balance ? 1u : 0u, P.range = S.range, P.tree_ratio = S.tree_ratio;
        for (int j = 0; j < dim; ++j) P.lower[j] = lower[j], P.span[j] = span[j];
        const uint32_t check_every = S.check_every ? S.check_every : kRrtcDefaultCheckEvery;
        const size_t qn = n * (size_t) dim;
        hipStream_t stream = nullptr;

        DeviceBuffers mem;
        RrtcArrays D{};
        float *d_starts = nullptr, *d_goals = nullptr;
        uint64_t *d_skips = nullptr, *d_bits = nullptr, *d_offsets = nullptr;
        uint32_t *d_active = nullptr;
        VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.pool, n * (size_t) S.max_samples * (size_t) dim));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.parent, n * (size_t) S.max_samples));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_starts, qn));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_goals, qn));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_skips, n));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_active, n));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.q_start, qn));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.q_goal, qn));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_bits, (n + 63) / 64));
        VMV_LOCKSTEP_HIP(mem.alloc(&D.done, n));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_offsets, n));
        VMV_LOCKSTEP_HIP(hipHostMalloc(&mem.pinned, std::max<size_t>(n, 16), hipHostMallocDefault));
        uint8_t *h_done = static_cast<uint8_t *>(mem.pinned);
        D.starts = d_starts, D.goals = d_goals, D.skips = d_skips, D.active = d_active, D.bits = d_bits;

        VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_starts, starts, qn * 4, hipMemcpyHostToDevice, stream));
        VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_goals, goals, qn * 4, hipMemcpyHostToDevice, stream));
        if (skips)
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_skips, skips, n * 8, hipMemcpyHostToDevice, stream));
        else
            VMV_LOCKSTEP_HIP(hipMemsetAsync(d_skips, 0, n * 8, stream));
        VMV_LOCKSTEP_HIP(hipMemsetAsync(d_bits, 0, ((n + 63) / 64) * 8, stream));
        const uint32_t n32 = (uint32_t) n;
        hipLaunchKernelGGL(rrtc_init_kernel, dim3((n32 + kRrtcBlock - 1) / kRrtcBlock), dim3(kRrtcBlock), 0, stream, P, D, n32);
        VMV_LOCKSTEP_HIP(hipGetLastError());

        std::vector<uint32_t> active(n);
        std::vector<const vmv_env *> active_envs(envs, envs + n);
        for (size_t k = 0; k < n; ++k) active[k] = (uint32_t) k;
        VMV_LOCKSTEP_HIP(hipMemcpy(d_active, active.data(), n * 4, hipMemcpyHostToDevice));

        // every problem ends within 1 + max_iterations + max_samples questions (each question after the direct one belongs
        // to a new iteration or adds a node): a bound on the rounds that does not depend on the device's answers
        const uint64_t max_rounds = 2ull + (uint64_t) S.max_iterations + (uint64_t) S.max_samples + check_every;
        uint64_t rounds = 0;
        const LockstepArrays L{d_active, D.q_start, D.q_goal, d_bits, D.done, h_done, n};
        const auto step = [&](uint32_t na) { hipLaunchKernelGGL(rrtc_step_kernel, dim3(na), dim3(kRrtcBlock), 0, stream, P, D); };
        if (int rc = lockstep_rounds(robot, stream, check_every, max_rounds, 1, active, active_envs, L, "vmv_rrtc_multi",
                                     "rrtc_step_kernel", step, rounds);
            rc != VMV_OK)
            return rc;

        // results: the states, then the paths traced on the device into one packed buffer
        std::vector<RrtcState> states(n);
        VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(RrtcState), hipMemcpyDeviceToHost));
        plans->n = n, plans->dim = dim, plans->rounds = rounds, plans->questions = 0;
        plans->status.resize(n), plans->iterations.resize(n), plans->sizes2.resize(2 * n), plans->path_lengths.resize(n);
        std::vector<uint64_t> path_offsets(n);
        uint64_t total = 0;
        for (size_t k = 0; k < n; ++k)
        {
            const RrtcState &st = states[k];
            plans->status[k] = (uint8_t) st.status;
            plans->iterations[k] = st.iterations;
            plans->sizes2[2 * k] = st.n[st.a_side], plans->sizes2[2 * k + 1] = st.n[st.a_side ^ 1u];
            plans->path_lengths[k] = st.path_len;
            plans->questions += st.questions;
            path_offsets[k] = total;
            total += st.path_len;
        }
        plans->paths.resize(total * (size_t) dim);
        if (total)
        {
            float *d_paths = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_paths, total * (size_t) dim));
            VMV_LOCKSTEP_HIP(hipMemcpy(d_offsets, path_offsets.data(), n * 8, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(rrtc_trace_kernel, dim3((n32 + kRrtcBlock - 1) / kRrtcBlock), dim3(kRrtcBlock), 0, stream, P, D, n32,
                               d_offsets, d_paths);
            VMV_LOCKSTEP_HIP(hipGetLastError());
            VMV_LOCKSTEP_HIP(hipMemcpy(plans->paths.data(), d_paths, total * (size_t) dim * 4, hipMemcpyDeviceToHost));
        }
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
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kRrtcMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n_problems > 0 && (!envs || !starts || !goals))) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n_problems; ++k)
            if (!envs[k]) return VMV_ERR_INVALID_ARGUMENT;
        if (!std::isfinite(settings->range) || !(settings->range > 0.f) || settings->max_samples < 2) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n_problems; ++k)
        {
            const uint64_t skip = halton_skips ? halton_skips[k] : 0;
            if (skip > 1000000ull || skip + settings->max_iterations > 1000000ull) return VMV_ERR_INVALID_ARGUMENT;
        }
        if (!halton_skips && settings->max_iterations > 1000000u) return VMV_ERR_INVALID_ARGUMENT;
        return vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            return vmv::rrtc_multi_run(robot, dim, lower, span, envs, n_problems, starts, goals, halton_skips, *settings, plans);
        });
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
