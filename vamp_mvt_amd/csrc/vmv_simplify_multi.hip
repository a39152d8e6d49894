// vmv_simplify_multi.hip — lockstep path simplification over many independent paths (vmv_simplify_multi).
//
// simplify() of planning/simplify.hh with the SHORTCUT and BSPLINE routines.  Every path is a state machine in device
// memory, advanced by the rounds of vmv_lockstep.h with W questions per path: simplify_step_kernel (one wave per
// unfinished path) consumes the W answers of the path's previous questions, erases or replaces waypoints, advances the
// routine and writes the next W edges into the round's start / goal arrays.
//
// Why a window of W questions gives the serial loop's path: shortcut_path takes, for waypoint i, the first valid j of the
// scan j = size-1 .. i+2, i.e. the largest valid j; a window asks the next W candidates in that order and the lowest set
// answer bit is that j (or none of them is valid and the scan goes on).  smooth_bspline, after subdivide(), modifies only
// even indices and reads only their odd neighbours and themselves, so the candidates of one step are independent of each
// other and asking both motions of a candidate (instead of the second only after the first) changes no decision.
//
// Arithmetic contract: fp32, one rounding per written operation (-ffp-contract=off; sqrtf is correctly rounded on
// gfx950), interpolate(a, b, t) = a + (b - a) * t, distance = sqrtf(sum of squares in joint order).
// A path owns two buffers of max_waypoints waypoints: an erase moves the tail down in place (read, barrier, write, chunk
// by chunk), a subdivision writes into the other buffer.  Every store is a plain vector store by the owning wave; no
// atomics.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"

#include <cmath>
#include <cstring>

struct vmv_paths
{
    size_t n = 0;
    int dim = 0;
    std::vector<uint8_t> status;
    std::vector<uint32_t> iterations, lengths, questions;
    std::vector<float> points;  // packed in path order
    uint64_t rounds = 0, total_questions = 0;
};

namespace vmv
{
    namespace
    {
        constexpr uint32_t kSimpBlock = kWave;  // one wave per path: its answers are one ballot-sized word
        constexpr uint32_t kSimpDefaultCheckEvery = 16;
        constexpr uint32_t kSimpDefaultQuestions = 16;
        constexpr uint32_t kSimpDefaultWaypoints = 2048;
        constexpr uint32_t kSimpMaxWaypoints = 1u << 24;  // (index arithmetic in 32 bits with room to spare)
        constexpr uint32_t kSimpMaxCandidates = 32;       // B-spline candidates of one round: W / 2

        enum : uint32_t
        {
            kPhaseInit = 0,      // nothing asked yet
            kPhaseDirect = 1,    // front -> back is in flight
            kPhaseShortcut = 2,  // cnt candidates jtop, jtop - 1, ... of waypoint i are in flight (cnt == 0: none)
            kPhaseBspline = 3,   // both motions of cnt candidates (indices in cand[]) are in flight
            kPhaseNextOp = 4,    // (within one kernel call only) operation `op` of the iteration is to begin
            kPhaseDone = 5
        };
        enum : uint32_t
        {
            kFlagAny = 1,      // simplify(): an operation of this iteration changed the path
            kFlagResult = 2,   // the running routine's return value so far (shortcut: result, B-spline: changed)
            kFlagUpdated = 4   // smooth_bspline(): this step replaced a waypoint
        };

        struct SimplifyState  // 64 bytes per path
        {
            uint32_t phase, status, iterations, size;
            uint32_t cur;     // which of the path's two buffers holds it
            uint32_t op;      // operation of the iteration
            uint32_t flags;
            uint32_t slot;    // position of the questions in flight in their round's arrays (in units of W)
            uint32_t i, jtop; // shortcut: waypoint, next candidate to ask (the candidates are jtop .. i + 2)
            uint32_t cnt;     // real questions (shortcut) or candidates (B-spline) in flight
            uint32_t step;    // B-spline step
            uint32_t pos;     // B-spline: next index to look at; 0 = the step has not begun (no subdivision yet)
            uint32_t questions;
            uint32_t pad0, pad1;
        };
        static_assert(sizeof(SimplifyState) == 64, "one cache line half per path");

        struct SimplifyParams
        {
            uint32_t dim, max_waypoints, max_iterations, n_ops;
            uint32_t bspline_ops;  // bit k: operation k of the list is BSPLINE (else SHORTCUT)
            uint32_t max_steps, w;
            float min_change, midpoint;
        };

        struct SimplifyArrays
        {
            SimplifyState *state;     // [n_paths]
            float *buf;               // [n_paths][2][max_waypoints][dim]
            uint32_t *cand;           // [n_paths][kSimpMaxCandidates] indices of the B-spline candidates in flight
            const float *points;      // the input, packed
            const uint64_t *offsets;  // [n_paths + 1] in waypoints
            const uint32_t *active;   // [n_active] path of each workgroup
            float *q_start, *q_goal;  // [n_active][w][dim] the round's questions
            const uint64_t *bits;     // answers of the previous round
            uint8_t *done;            // [n_paths]
        };

        __device__ __forceinline__ float interpolate(float a, float b, float t) { return a + (b - a) * t; }

        // joint d of smooth_bspline's midpoint for waypoint idx (simplify.hh:33-35)
        __device__ __forceinline__ float bspline_midpoint(const float *path, uint32_t idx, uint32_t d, uint32_t dim, float mi)
        {
            const float c = path[(size_t) idx * dim + d];
            const float t1 = interpolate(c, path[(size_t) (idx - 1u) * dim + d], mi);
            const float t2 = interpolate(c, path[(size_t) (idx + 1u) * dim + d], mi);
            return interpolate(t1, t2, 0.5f);
        }

        __global__ __launch_bounds__(kSimpBlock) void simplify_init_kernel(const SimplifyParams P, const SimplifyArrays D)
        {
            const uint32_t p = blockIdx.x, lane = threadIdx.x;
            const uint64_t lo = D.offsets[p];
            const uint32_t len = (uint32_t) (D.offsets[p + 1] - lo);
            float *path = D.buf + (size_t) p * 2u * P.max_waypoints * P.dim;
            const float *in = D.points + lo * P.dim;
            for (size_t e = lane; e < (size_t) len * P.dim; e += kSimpBlock) path[e] = in[e];
            if (lane == 0)
            {
                SimplifyState st{};
                st.phase = len > 2 ? kPhaseInit : kPhaseDone;  // below 3 waypoints: returned as it is, without a question
                st.status = VMV_SIMPLIFY_OK, st.size = len;
                D.state[p] = st;
                D.done[p] = len > 2 ? 0 : 1;
            }
        }

        // One wave per active path; every branch below is taken by the whole wave (its conditions are values every lane
        // holds alike), so the barriers and the ballot are safe.
        __global__ __launch_bounds__(kSimpBlock) void simplify_step_kernel(const SimplifyParams P, const SimplifyArrays D)
        {
            __shared__ uint32_t s_cand[kSimpMaxCandidates];
            const uint32_t a = blockIdx.x, p = D.active[a], lane = threadIdx.x, dim = P.dim, M = P.max_waypoints, W = P.w;
            SimplifyState st = D.state[p];
            float *const base = D.buf + (size_t) p * 2u * M * dim;
            float *path = base + (size_t) st.cur * M * dim;
            uint32_t *const cand = D.cand + (size_t) p * kSimpMaxCandidates;
            float *const qs = D.q_start + (size_t) a * W * dim, *const qg = D.q_goal + (size_t) a * W * dim;
            const bool was_done = st.phase == kPhaseDone;
            enum { kEmitNull, kEmitDirect, kEmitShortcut, kEmitBspline } emit = kEmitNull;

            if (st.phase == kPhaseInit)
            {
                st.phase = kPhaseDirect, st.questions = 1;
                emit = kEmitDirect;
            }
            else if (!was_done)
            {
                const uint32_t s0 = st.slot * W;  // W divides 64: the path's answers sit in one word
                const uint64_t ans = D.bits[s0 >> 6] >> (s0 & 63u);
                if (st.phase == kPhaseDirect)
                {
                    if (ans & 1ull)  // the straight line is valid: (front, back)
                    {
                        float v = 0.f;
                        if (lane < dim) v = path[(size_t) (st.size - 1u) * dim + lane];
                        __syncthreads();
                        if (lane < dim) path[dim + lane] = v;
                        st.size = 2, st.phase = kPhaseDone;
                    }
                    else if (P.max_iterations == 0)
                        st.phase = kPhaseDone;
                    else
                        st.iterations = 1, st.op = 0, st.flags = 0, st.phase = kPhaseNextOp;
                }
                else if (st.phase == kPhaseShortcut)
                {
                    const uint64_t m = st.cnt >= 64u ? ans : ans & ((1ull << st.cnt) - 1ull);
                    if (m)  // the lowest set bit is the largest valid j: erase (i, j) exclusive
                    {
                        const uint32_t j = st.jtop - (uint32_t) __builtin_ctzll(m);
                        const size_t tail = (size_t) (st.size - j) * dim;
                        const float *src = path + (size_t) j * dim;
                        float *dst = path + (size_t) (st.i + 1u) * dim;
                        for (size_t b = 0; b < tail; b += kSimpBlock)  // dst < src: chunk c's stores end below chunk c + 1's loads
                        {
                            float v = 0.f;
                            if (b + lane < tail) v = src[b + lane];
                            __syncthreads();
                            if (b + lane < tail) dst[b + lane] = v;
                        }
                        st.size -= j - st.i - 1u;
                        st.flags |= kFlagResult;
                        ++st.i, st.jtop = st.size - 1u;
                    }
                    else
                        st.jtop -= st.cnt;  // (>= i + 1: the window ended at or above i + 2)
                }
                else  // kPhaseBspline: a candidate is replaced iff both its motions are valid
                {
                    const uint64_t both = ans & (ans >> 1) & 0x5555555555555555ull &
                                          (st.cnt >= 32u ? ~0ull : ((1ull << (2u * st.cnt)) - 1ull));
                    for (uint32_t e = lane; e < st.cnt * dim; e += kSimpBlock)  // (element e is read and written by this lane alone)
                    {
                        const uint32_t c = e / dim, d = e - c * dim;
                        if ((both >> (2u * c)) & 1ull)
                        {
                            const uint32_t idx = cand[c];
                            path[(size_t) idx * dim + d] = bspline_midpoint(path, idx, d, dim, P.midpoint);
                        }
                    }
                    if (both) st.flags |= kFlagUpdated | kFlagResult;
                }
                __syncthreads();

                while (st.phase != kPhaseDone)
                {
                    if (st.phase == kPhaseNextOp)
                    {
                        if (st.op == P.n_ops)  // the iteration is over
                        {
                            if (!(st.flags & kFlagAny) || st.iterations >= P.max_iterations)
                                st.phase = kPhaseDone;
                            else
                                ++st.iterations, st.op = 0, st.flags = 0;
                            continue;
                        }
                        if (st.size < 3)  // both routines return false below 3 waypoints
                        {
                            ++st.op;
                            continue;
                        }
                        st.flags &= ~(kFlagResult | kFlagUpdated);
                        st.cnt = 0;
                        if ((P.bspline_ops >> st.op) & 1u)
                            st.phase = kPhaseBspline, st.step = 0, st.pos = 0;
                        else
                            st.phase = kPhaseShortcut, st.i = 0, st.jtop = st.size - 1u;
                        continue;
                    }
                    bool over = false;  // the running routine returns
                    if (st.phase == kPhaseShortcut)
                    {
                        if (st.i + 2u >= st.size)  // the bound i < size - 2, re-evaluated after every erase
                            over = true;
                        else if (st.jtop < st.i + 2u)  // no valid j for this i
                        {
                            ++st.i, st.jtop = st.size - 1u;
                            continue;
                        }
                        else
                        {
                            st.cnt = min(W, st.jtop - (st.i + 1u));
                            st.questions += st.cnt;
                            emit = kEmitShortcut;
                            break;
                        }
                    }
                    else  // kPhaseBspline
                    {
                        bool scan = true;
                        if (st.pos == 0)  // a step begins
                        {
                            if (st.step == P.max_steps)
                                over = true, scan = false;
                            else if (2u * st.size - 1u > M)  // the subdivision is not made; the path stays as it stood
                            {
                                st.status = VMV_SIMPLIFY_CAPACITY, st.phase = kPhaseDone;
                                break;
                            }
                            else  // Path::subdivide (plan.hh:34-49) into the other buffer
                            {
                                float *dst = base + (size_t) (st.cur ^ 1u) * M * dim;
                                const uint32_t total = (2u * st.size - 1u) * dim;
                                for (uint32_t e = lane; e < total; e += kSimpBlock)
                                {
                                    const uint32_t w = e / dim, d = e - w * dim, k = w >> 1;
                                    const float c = path[(size_t) k * dim + d];
                                    dst[e] = (w & 1u) ? interpolate(c, path[(size_t) (k + 1u) * dim + d], 0.5f) : c;
                                }
                                st.cur ^= 1u, path = dst, st.size = 2u * st.size - 1u;
                                st.pos = 2, st.flags &= ~kFlagUpdated;
                                __syncthreads();
                            }
                        }
                        uint32_t nc = 0;
                        while (scan && nc < W / 2u && st.pos < st.size - 1u)  // the next W / 2 indices that pass min_change
                        {
                            const uint32_t idx = st.pos + 2u * lane;
                            bool pass = false;
                            if (idx < st.size - 1u)
                            {
                                float sum = 0.f;
                                for (uint32_t d = 0; d < dim; ++d)
                                {
                                    const float df = bspline_midpoint(path, idx, d, dim, P.midpoint) - path[(size_t) idx * dim + d];
                                    sum = sum + df * df;
                                }
                                pass = sqrtf(sum) > P.min_change;  // false for NaN
                            }
                            uint64_t mask = __ballot(pass);
                            const uint32_t want = W / 2u - nc;
                            if ((uint32_t) __popcll(mask) > want)  // keep the first `want`, go on behind the last of them
                            {
                                uint64_t keep = 0, rest = mask;
                                for (uint32_t t = 0; t < want; ++t)
                                {
                                    const uint64_t low = rest & (0ull - rest);
                                    keep |= low, rest ^= low;
                                }
                                mask = keep;
                                st.pos += 2u * (64u - (uint32_t) __builtin_clzll(keep));
                            }
                            else
                                st.pos += 2u * kSimpBlock;
                            if ((mask >> lane) & 1ull) s_cand[nc + (uint32_t) __popcll(mask & ((1ull << lane) - 1ull))] = idx;
                            nc += (uint32_t) __popcll(mask);
                        }
                        if (nc > 0)
                        {
                            __syncthreads();
                            if (lane < nc) cand[lane] = s_cand[lane];
                            st.cnt = nc, st.questions += 2u * nc;
                            emit = kEmitBspline;
                            break;
                        }
                        if (scan)  // the step is over
                        {
                            if (st.flags & kFlagUpdated)
                            {
                                ++st.step, st.pos = 0;
                                continue;
                            }
                            over = true;  // a step without an update ends the routine
                        }
                    }
                    if (over)
                    {
                        if (st.flags & kFlagResult) st.flags |= kFlagAny;
                        ++st.op, st.phase = kPhaseNextOp;
                    }
                }
            }

            // the round's W edges; unused slots, and every slot of a finished path, carry the null question front -> front
            __syncthreads();
            for (uint32_t e = lane; e < W * dim; e += kSimpBlock)
            {
                const uint32_t s = e / dim, d = e - s * dim;
                float vs = path[d], vg = path[d];
                if (emit == kEmitDirect)
                {
                    if (s == 0) vg = path[(size_t) (st.size - 1u) * dim + d];
                }
                else if (emit == kEmitShortcut)
                {
                    if (s < st.cnt) vs = path[(size_t) st.i * dim + d], vg = path[(size_t) (st.jtop - s) * dim + d];
                }
                else if (emit == kEmitBspline)
                {
                    if ((s >> 1) < st.cnt)
                    {
                        const uint32_t idx = s_cand[s >> 1];
                        const float mid = bspline_midpoint(path, idx, d, dim, P.midpoint);
                        if (s & 1u)
                            vs = mid, vg = path[(size_t) (idx + 1u) * dim + d];
                        else
                            vs = path[(size_t) (idx - 1u) * dim + d], vg = mid;
                    }
                }
                qs[e] = vs, qg[e] = vg;
            }
            if (!was_done && lane == 0)
            {
                st.slot = a;
                D.state[p] = st;
                if (st.phase == kPhaseDone) D.done[p] = 1;
            }
        }

        // the final paths, packed: one wave per path
        __global__ __launch_bounds__(kSimpBlock) void simplify_gather_kernel(const SimplifyParams P, const SimplifyArrays D,
                                                                              const uint64_t *__restrict__ out_offsets,
                                                                              float *__restrict__ out)
        {
            const uint32_t p = blockIdx.x;
            const SimplifyState st = D.state[p];
            const float *path = D.buf + ((size_t) p * 2u + st.cur) * P.max_waypoints * P.dim;
            float *o = out + out_offsets[p] * P.dim;
            for (size_t e = threadIdx.x; e < (size_t) st.size * P.dim; e += kSimpBlock) o[e] = path[e];
        }

        uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
        uint64_t sat_mul(uint64_t a, uint64_t b) { return (a && b > ~0ull / a) ? ~0ull : a * b; }

        // Rounds no path of the call can exceed, from the settings and the longest input alone: no path holds more than
        // S = min(max_waypoints, (longest - 1) * 2^(subdivisions the settings allow) + 1) waypoints; a shortcut pass over s
        // waypoints asks at most sum over i of ceil((s - i - 2) / W) <= s^2 / (2 W) + s windows, a B-spline step at most
        // ceil(s / 2 / (W / 2)) + 1.
        uint64_t round_bound(const SimplifyParams &P, size_t longest, uint32_t check_every)
        {
            uint64_t n_bspline = 0;
            for (uint32_t k = 0; k < P.n_ops; ++k) n_bspline += (P.bspline_ops >> k) & 1u;
            const uint64_t doublings = sat_mul(sat_mul(P.max_iterations, n_bspline), P.max_steps);
            uint64_t S = P.max_waypoints;
            if (doublings < 32) S = std::min<uint64_t>(S, (((uint64_t) longest - 1u) << doublings) + 1u);
            const uint64_t shortcut = S * S / (2ull * P.w) + S + 1u;  // S <= 2^24
            const uint64_t bspline = sat_mul(P.max_steps, S / P.w + 2u);
            const uint64_t per_iteration = sat_add(sat_mul(P.n_ops - n_bspline, shortcut), sat_mul(n_bspline, bspline));
            return sat_add(sat_mul(P.max_iterations, per_iteration), 2ull + check_every);
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with the
        // robot's part built.
        int simplify_multi_run(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                               const SimplifyParams &P, uint32_t check_every, vmv_paths *paths)
        {
            const size_t dim = P.dim, W = P.w, total_in = offsets[n];
            hipStream_t stream = nullptr;

            std::vector<uint32_t> active;
            std::vector<const vmv_env *> active_envs;
            std::vector<uint64_t> offsets64(n + 1);
            size_t longest = 0;
            for (size_t k = 0; k < n; ++k)
            {
                const size_t len = offsets[k + 1] - offsets[k];
                offsets64[k] = offsets[k];
                longest = std::max(longest, len);
                if (len > 2) active.push_back((uint32_t) k), active_envs.push_back(envs[k]);  // shorter ones ask nothing
            }
            offsets64[n] = total_in;
            const size_t na0 = active.size();

            DeviceBuffers mem;
            LockstepBuffers B;
            SimplifyArrays D{};
            float *d_points = nullptr;
            uint64_t *d_offsets = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.buf, n * 2u * (size_t) P.max_waypoints * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.cand, n * kSimpMaxCandidates));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_points, total_in * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_offsets, n + 1));
            if (int rc = B.alloc(mem, n, na0, W, dim, stream); rc != VMV_OK) return rc;
            D.points = d_points, D.offsets = d_offsets, D.active = B.active, D.q_start = B.q_start, D.q_goal = B.q_goal, D.bits = B.bits;
            D.done = B.done;

            if (total_in) VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_points, points, total_in * dim * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_offsets, offsets64.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
            const uint32_t n32 = (uint32_t) n;
            hipLaunchKernelGGL(simplify_init_kernel, dim3(n32), dim3(kSimpBlock), 0, stream, P, D);
            VMV_LOCKSTEP_HIP(hipGetLastError());
            if (na0) VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active.data(), na0 * 4, hipMemcpyHostToDevice));

            uint64_t rounds = 0;
            const auto step = [&](uint32_t na) { hipLaunchKernelGGL(simplify_step_kernel, dim3(na), dim3(kSimpBlock), 0, stream, P, D); };
            if (int rc = lockstep_rounds(robot, stream, check_every, round_bound(P, longest, check_every), W, active, active_envs, B.arrays(),
                                         "vmv_simplify_multi", "simplify_step_kernel", step, rounds);
                rc != VMV_OK)
                return rc;

            // results: the states, then the paths gathered on the device into one packed buffer
            std::vector<SimplifyState> states(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(SimplifyState), hipMemcpyDeviceToHost));
            paths->n = n, paths->dim = (int) dim, paths->rounds = rounds, paths->total_questions = 0;
            paths->status.resize(n), paths->iterations.resize(n), paths->lengths.resize(n), paths->questions.resize(n);
            for (size_t k = 0; k < n; ++k)
            {
                const SimplifyState &st = states[k];
                paths->status[k] = (uint8_t) st.status;
                paths->iterations[k] = st.iterations;
                paths->lengths[k] = st.size;
                paths->questions[k] = st.questions;
                paths->total_questions += st.questions;
            }
            return pack_paths(mem, B.path_offsets, paths->lengths, dim, nullptr, "simplify_gather_kernel",
                              [&](const uint64_t *d_out_offsets, float *d_out) {
                                  hipLaunchKernelGGL(simplify_gather_kernel, dim3(n32), dim3(kSimpBlock), 0, stream, P, D, d_out_offsets, d_out);
                              },
                              paths->points);
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_simplify_multi(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                           const vmv_simplify_settings *settings, vmv_paths **out)
    {
        // device-free checks first; the environments' own (NULL handles again, unfinalized, another device) are those of
        // vmv_env_prepare_multi, which then builds the parts not yet built in one batch
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n_paths > 0 && (!envs || !offsets))) return VMV_ERR_INVALID_ARGUMENT;
        const vmv_simplify_settings &S = *settings;
        const uint32_t W = S.questions_per_round ? S.questions_per_round : vmv::kSimpDefaultQuestions;
        if (W != 2 && W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return VMV_ERR_INVALID_ARGUMENT;
        if (S.interpolate != 0 || S.n_operations > 8) return VMV_ERR_INVALID_ARGUMENT;
        vmv::SimplifyParams P{};
        for (uint32_t k = 0; k < S.n_operations; ++k)
        {
            if (S.operations[k] == VMV_SIMPLIFY_BSPLINE)
                P.bspline_ops |= 1u << k;
            else if (S.operations[k] != VMV_SIMPLIFY_SHORTCUT)
                return VMV_ERR_INVALID_ARGUMENT;
        }
        if (n_paths >= vmv::kMultiMaxConfigs || n_paths * (size_t) W >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        const uint32_t max_waypoints = S.max_waypoints ? S.max_waypoints : vmv::kSimpDefaultWaypoints;
        if (max_waypoints > vmv::kSimpMaxWaypoints) return VMV_ERR_INVALID_ARGUMENT;
        if (n_paths > 0 && offsets[0] != 0) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n_paths; ++k)
        {
            if (offsets[k + 1] < offsets[k]) return VMV_ERR_INVALID_ARGUMENT;
            if (offsets[k + 1] - offsets[k] > max_waypoints) return VMV_ERR_INVALID_ARGUMENT;
        }
        if (n_paths > 0 && offsets[n_paths] > 0 && !points) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n_paths; ++k)
            if (!envs[k]) return VMV_ERR_INVALID_ARGUMENT;
        P.dim = (uint32_t) dim, P.max_waypoints = max_waypoints, P.max_iterations = S.max_iterations, P.n_ops = S.n_operations;
        P.max_steps = S.bspline_max_steps, P.w = W;
        P.min_change = S.bspline_min_change, P.midpoint = S.bspline_midpoint_interpolation;
        const uint32_t check_every = S.check_every ? S.check_every : vmv::kSimpDefaultCheckEvery;
        return vmv::lockstep_call(robot, envs, n_paths, dim, out, [&](vmv_paths *paths) {
            return vmv::simplify_multi_run(robot, envs, n_paths, points, offsets, P, check_every, paths);
        });
    }

    int vmv_paths_summary(const vmv_paths *paths, uint8_t *status, uint32_t *iterations, uint32_t *lengths, uint32_t *questions,
                          uint64_t *rounds, uint64_t *total_questions)
    {
        if (!paths) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = paths->n;
        if (status && n) std::memcpy(status, paths->status.data(), n);
        if (iterations && n) std::memcpy(iterations, paths->iterations.data(), n * 4);
        if (lengths && n) std::memcpy(lengths, paths->lengths.data(), n * 4);
        if (questions && n) std::memcpy(questions, paths->questions.data(), n * 4);
        if (rounds) *rounds = paths->rounds;
        if (total_questions) *total_questions = paths->total_questions;
        return VMV_OK;
    }

    int vmv_paths_points(const vmv_paths *paths, float *out, size_t capacity_floats)
    {
        if (!paths || (!out && !paths->points.empty())) return VMV_ERR_INVALID_ARGUMENT;
        if (capacity_floats < paths->points.size()) return VMV_ERR_CAPACITY;
        if (!paths->points.empty()) std::memcpy(out, paths->points.data(), paths->points.size() * 4);
        return VMV_OK;
    }

    int vmv_paths_destroy(vmv_paths *paths)
    {
        if (!paths) return VMV_ERR_INVALID_ARGUMENT;
        delete paths;
        return VMV_OK;
    }
}
