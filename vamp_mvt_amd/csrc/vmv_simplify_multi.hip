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
//
// vmv_simplify_multi_constrained (include/vamp_mvt_amd.h states the contract in full) runs the same state
// machine inside the band of an end-effector constraint: simplify_step_kernel<true> ANDs the answers of the band round
// (simplify_band_round_kernel of the robot's translation unit, launched right behind it) into the validity bits, names per
// slot what that round is to do (nothing, band-check the edge, project the B-spline midpoint first), takes the projected
// midpoints from a per-path buffer and counts the serial loop's refused questions from the consumed window.
// simplify_step_kernel<false> is the kernel vmv_simplify_multi always ran.
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
    bool constrained = false;            // made by vmv_simplify_multi_constrained
    std::vector<uint32_t> band_refused;  // [n] then
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
            uint32_t refused;  // vmv_simplify_multi_constrained: questions of the serial loop the constraint answered 0
            uint32_t pad1;
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

        // vmv_simplify_multi_constrained only (every pointer NULL otherwise; the unconstrained kernels never read them)
        enum : uint8_t
        {
            kBandNull = 0,      // a null slot: answered 1 without a test
            kBandEdge = 1,      // the edge's band test alone
            kBandProjGoal = 2,  // even B-spline slot: q_goal (the midpoint) is projected first
            kBandProjStart = 3  // odd B-spline slot: q_start (the midpoint) is projected first
        };
        struct SimplifyBand
        {
            uint8_t *pending;            // [n_active][w] what the band round is to do with each slot
            const uint8_t *c_ok;         // [n_active][w] its answers, ANDed into the validity bits
            const float *proj;           // [n_paths][kSimpMaxCandidates][dim] the projected midpoints of the window in flight
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

        __global__ __launch_bounds__(kSimpBlock) void simplify_init_kernel(const SimplifyParams P, const SimplifyArrays D,
                                                                           const uint8_t *__restrict__ out_of_band)
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
                const bool out = out_of_band != nullptr && out_of_band[p] != 0;  // (never set below 3 waypoints)
                const bool runs = len > 2 && !out;  // below 3 waypoints: returned as it is, without a question
                st.phase = runs ? kPhaseInit : kPhaseDone;
                st.status = out ? VMV_SIMPLIFY_OUT_OF_BAND : VMV_SIMPLIFY_OK, st.size = len;
                D.state[p] = st;
                D.done[p] = runs ? 0 : 1;
            }
        }

        // One wave per active path; every branch below is taken by the whole wave (its conditions are values every lane
        // holds alike), so the barriers and the ballot are safe.  Constrained (vmv_simplify_multi_constrained, the contract
        // at that entry point): the band round's answers are ANDed into the validity bits, the serial loop's refused
        // questions are counted from the consumed window, a B-spline replacement takes the projected midpoint and passes
        // the second min_change test, and every slot written carries its code for the band round.
        template <bool Constrained>
        __global__ __launch_bounds__(kSimpBlock) void simplify_step_kernel(const SimplifyParams P, const SimplifyArrays D,
                                                                           const SimplifyBand X)
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
                uint64_t ans = D.bits[s0 >> 6] >> (s0 & 63u);
                uint64_t band = ~0ull;  // bit s: the band round answered slot s with 1
                if constexpr (Constrained)
                {
                    band = __ballot(lane < W && X.c_ok[(size_t) s0 + lane] != 0);
                    ans &= band;
                }
                if (st.phase == kPhaseDirect)
                {
                    if constexpr (Constrained) st.refused += (band & 1ull) ? 0u : 1u;
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
                    if constexpr (Constrained)  // the serial scan asks the slots below the found one (all of them if none)
                    {
                        const uint64_t asked = m ? (m & (0ull - m)) - 1ull : (st.cnt >= 64u ? ~0ull : (1ull << st.cnt) - 1ull);
                        st.refused += (uint32_t) __popcll(~band & asked);
                    }
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
                    uint64_t both = ans & (ans >> 1) & 0x5555555555555555ull &
                                    (st.cnt >= 32u ? ~0ull : ((1ull << (2u * st.cnt)) - 1ull));
                    if constexpr (Constrained)
                    {
                        const uint64_t real = st.cnt >= 32u ? ~0ull : ((1ull << (2u * st.cnt)) - 1ull);
                        // the serial loop asks the first motion of every candidate, the second where the first was answered 1
                        const uint64_t asked = (0x5555555555555555ull | ((ans & 0x5555555555555555ull) << 1)) & real;
                        st.refused += (uint32_t) __popcll(~band & asked);
                        // the second min_change test, candidate `lane`: distance(path[index], mid_p) > min_change
                        bool moves = false;
                        if (lane < st.cnt && ((both >> (2u * lane)) & 1ull))
                        {
                            const float *mp = X.proj + ((size_t) p * kSimpMaxCandidates + lane) * dim;
                            const float *own = path + (size_t) cand[lane] * dim;
                            float sum = 0.f;
                            for (uint32_t d = 0; d < dim; ++d)
                            {
                                const float df = mp[d] - own[d];
                                sum = sum + df * df;
                            }
                            moves = sqrtf(sum) > P.min_change;  // false for NaN
                        }
                        const uint64_t keep = __ballot(moves);  // bit c: candidate c
                        uint64_t spread = 0;
                        for (uint64_t rest = keep; rest; rest &= rest - 1ull) spread |= 1ull << (2u * (uint32_t) __builtin_ctzll(rest));
                        both = spread;
                    }
                    for (uint32_t e = lane; e < st.cnt * dim; e += kSimpBlock)  // (element e is read and written by this lane alone)
                    {
                        const uint32_t c = e / dim, d = e - c * dim;
                        if ((both >> (2u * c)) & 1ull)
                        {
                            const uint32_t idx = cand[c];
                            if constexpr (Constrained)
                                path[(size_t) idx * dim + d] = X.proj[((size_t) p * kSimpMaxCandidates + c) * dim + d];
                            else
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
            if constexpr (Constrained)
            {
                if (lane < W)
                {
                    uint8_t code = kBandNull;
                    if (emit == kEmitDirect)
                        code = lane == 0 ? kBandEdge : kBandNull;
                    else if (emit == kEmitShortcut)
                        code = lane < st.cnt ? kBandEdge : kBandNull;
                    else if (emit == kEmitBspline)
                        code = (lane >> 1) < st.cnt ? ((lane & 1u) ? kBandProjStart : kBandProjGoal) : kBandNull;
                    X.pending[(size_t) a * W + lane] = code;
                }
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

        // The constrained call's look at its input, before the rounds: ONE band test over the first waypoint of every path
        // and ONE edge band test over every consecutive pair of the packed input (the pairs that straddle two paths are
        // asked too and not looked at), each with its path's record.  out_of_band[p] = 1: a path of 3 waypoints or more
        // with its first waypoint or an edge out of band.  d_recs: one record (shared) or one per path, for the rounds.
        int simplify_band_input(int robot, const ConstraintBand &cb, DeviceBuffers &mem, size_t n, const float *points,
                                const float *d_points, const size_t *offsets, size_t dim, hipStream_t stream, ConstraintDev **d_recs,
                                std::vector<uint8_t> &out_of_band)
        {
            const RobotLaunchers &L = robot_launchers(robot);
            const size_t total = offsets[n], n_edges = total > 0 ? total - 1 : 0;
            std::vector<ConstraintDev> recs(cb.count);
            constraint_band_records(cb, recs.data());
            if (int rc = upload_records(mem, recs.data(), cb.count, d_recs); rc != VMV_OK) return rc;
            out_of_band.assign(n, 0);

            std::vector<float> firsts(n * dim, 0.0f);
            for (size_t p = 0; p < n; ++p)
                if (offsets[p + 1] > offsets[p]) std::memcpy(&firsts[p * dim], points + offsets[p] * dim, dim * 4);
            DeviceBuffers tmp;  // what only this look needs
            float *d_firsts = nullptr;
            uint64_t *d_bits = nullptr;
            uint8_t *d_ok = nullptr;
            const ConstraintDev *d_edge_recs = *d_recs;
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_firsts, n * dim));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_bits, (n + 63) / 64));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_ok, n_edges));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_firsts, firsts.data(), n * dim * 4, hipMemcpyHostToDevice, stream));
            if (!cb.P.shared && n_edges)  // edge e begins at packed waypoint e: its path's record
            {
                std::vector<uint32_t> owner(n_edges);
                for (size_t p = 0; p < n; ++p)
                    for (size_t e = offsets[p]; e < offsets[p + 1] && e < n_edges; ++e) owner[e] = (uint32_t) p;
                ConstraintDev *d = nullptr;
                if (int rc = upload_records(tmp, constraint_band_expand(recs.data(), owner).data(), n_edges, &d); rc != VMV_OK) return rc;
                d_edge_recs = d;
            }
            if (int rc = L.constraint_check(cb.P, *d_recs, d_firsts, n, d_bits, nullptr, stream); rc != VMV_OK) return rc;
            if (n_edges)
                if (int rc = L.constraint_edges(cb.P, d_edge_recs, d_points, d_points + dim, n_edges, d_ok, stream); rc != VMV_OK) return rc;
            std::vector<uint64_t> bits((n + 63) / 64);
            std::vector<uint8_t> ok(n_edges);
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(bits.data(), d_bits, bits.size() * 8, hipMemcpyDeviceToHost, stream));
            if (n_edges) VMV_LOCKSTEP_HIP(hipMemcpyAsync(ok.data(), d_ok, n_edges, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
            for (size_t p = 0; p < n; ++p)
            {
                if (offsets[p + 1] - offsets[p] < 3) continue;  // returned as it is, whatever the tests said
                bool in = ((bits[p >> 6] >> (p & 63u)) & 1ull) != 0;
                for (size_t e = offsets[p]; in && e + 1 < offsets[p + 1]; ++e) in = ok[e] != 0;
                out_of_band[p] = in ? 0 : 1;
            }
            return VMV_OK;
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with the
        // robot's part built.
        // cb: vmv_simplify_multi_constrained's constraints and resolved settings (NULL: vmv_simplify_multi).
        int simplify_multi_run(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                               const SimplifyParams &P, uint32_t check_every, vmv_paths *paths, const ConstraintBand *cb = nullptr)
        {
            const size_t dim = P.dim, W = P.w, total_in = offsets[n];
            hipStream_t stream = nullptr;

            DeviceBuffers mem;
            float *d_points = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&d_points, total_in * dim));
            if (total_in) VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_points, points, total_in * dim * 4, hipMemcpyHostToDevice, stream));

            // the constrained call's look at the input: which paths take part, and the records of all paths on the device
            std::vector<uint8_t> out_of_band;
            ConstraintDev *d_recs = nullptr;
            uint8_t *d_out_of_band = nullptr;
            if (cb)
            {
                if (int rc = simplify_band_input(robot, *cb, mem, n, points, d_points, offsets, dim, stream, &d_recs, out_of_band); rc != VMV_OK)
                    return rc;
                VMV_LOCKSTEP_HIP(mem.alloc(&d_out_of_band, n));
                VMV_LOCKSTEP_HIP(hipMemcpy(d_out_of_band, out_of_band.data(), n, hipMemcpyHostToDevice));
            }

            std::vector<uint32_t> active;
            std::vector<const vmv_env *> active_envs;
            std::vector<uint64_t> offsets64(n + 1);
            size_t longest = 0;
            for (size_t k = 0; k < n; ++k)
            {
                const size_t len = offsets[k + 1] - offsets[k];
                offsets64[k] = offsets[k];
                longest = std::max(longest, len);
                if (len > 2 && !(cb && out_of_band[k])) active.push_back((uint32_t) k), active_envs.push_back(envs[k]);  // the others ask nothing
            }
            offsets64[n] = total_in;
            const size_t na0 = active.size();

            LockstepBuffers B;
            SimplifyArrays D{};
            SimplifyBand X{};
            uint64_t *d_offsets = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.buf, n * 2u * (size_t) P.max_waypoints * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.cand, n * kSimpMaxCandidates));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_offsets, n + 1));
            if (int rc = B.alloc(mem, n, na0, W, dim, stream); rc != VMV_OK) return rc;
            D.points = d_points, D.offsets = d_offsets, D.active = B.active, D.q_start = B.q_start, D.q_goal = B.q_goal, D.bits = B.bits;
            D.done = B.done;
            uint8_t *d_c_ok = nullptr;
            float *d_proj = nullptr;
            if (cb)
            {
                const size_t slots = std::max<size_t>(na0, 1) * W;
                VMV_LOCKSTEP_HIP(mem.alloc(&X.pending, slots));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_c_ok, slots + kSimpBlock));  // (a wave's worth of room behind the last slot)
                VMV_LOCKSTEP_HIP(mem.alloc(&d_proj, n * kSimpMaxCandidates * dim));
                VMV_LOCKSTEP_HIP(hipMemsetAsync(d_c_ok, 0, slots + kSimpBlock, stream));
                X.c_ok = d_c_ok, X.proj = d_proj;
            }

            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_offsets, offsets64.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
            const uint32_t n32 = (uint32_t) n;
            hipLaunchKernelGGL(simplify_init_kernel, dim3(n32), dim3(kSimpBlock), 0, stream, P, D, (const uint8_t *) d_out_of_band);
            VMV_LOCKSTEP_HIP(hipGetLastError());
            if (na0) VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active.data(), na0 * 4, hipMemcpyHostToDevice));

            uint64_t rounds = 0;
            const auto step = [&](uint32_t na) {
                if (!cb)
                {
                    hipLaunchKernelGGL(simplify_step_kernel<false>, dim3(na), dim3(kSimpBlock), 0, stream, P, D, X);
                    return;
                }
                // the step kernel names what each slot needs; the band round projects the B-spline midpoints in place and
                // answers every slot's band question before the round's validation reads the edges
                hipLaunchKernelGGL(simplify_step_kernel<true>, dim3(na), dim3(kSimpBlock), 0, stream, P, D, X);
                (void) robot_launchers(robot).simplify_band_round(cb->P, d_recs, B.active, B.q_start, B.q_goal, X.pending, d_proj,
                                                                   (uint32_t) (kSimpMaxCandidates * dim), d_c_ok, na, (uint32_t) W, stream);
            };
            if (int rc = lockstep_rounds(robot, stream, check_every, round_bound(P, longest, check_every), W, active, active_envs, B.arrays(),
                                         cb ? "vmv_simplify_multi_constrained" : "vmv_simplify_multi", "simplify_step_kernel", step, rounds);
                rc != VMV_OK)
                return rc;

            // results: the states, then the paths gathered on the device into one packed buffer
            std::vector<SimplifyState> states(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(SimplifyState), hipMemcpyDeviceToHost));
            paths->n = n, paths->dim = (int) dim, paths->rounds = rounds, paths->total_questions = 0;
            paths->status.resize(n), paths->iterations.resize(n), paths->lengths.resize(n), paths->questions.resize(n);
            if (cb) paths->band_refused.resize(n);
            for (size_t k = 0; k < n; ++k)
            {
                const SimplifyState &st = states[k];
                if (cb) paths->band_refused[k] = st.refused;
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

    // vmv_simplify_multi's checks, none of which needs a device, in the header's order -> the resolved settings
    int simplify_checks(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                        const vmv_simplify_settings *settings, vmv_paths *const *out, SimplifyParams &P, uint32_t &check_every)
    {
        // device-free checks first; the environments' own (NULL handles again, unfinalized, another device) are those of
        // vmv_env_prepare_multi, which then builds the parts not yet built in one batch
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n_paths > 0 && (!envs || !offsets))) return VMV_ERR_INVALID_ARGUMENT;
        const vmv_simplify_settings &S = *settings;
        const uint32_t W = S.questions_per_round ? S.questions_per_round : kSimpDefaultQuestions;
        if (W != 2 && W != 4 && W != 8 && W != 16 && W != 32 && W != 64) return VMV_ERR_INVALID_ARGUMENT;
        if (S.interpolate != 0 || S.n_operations > 8) return VMV_ERR_INVALID_ARGUMENT;
        for (uint32_t k = 0; k < S.n_operations; ++k)
        {
            if (S.operations[k] == VMV_SIMPLIFY_BSPLINE)
                P.bspline_ops |= 1u << k;
            else if (S.operations[k] != VMV_SIMPLIFY_SHORTCUT)
                return VMV_ERR_INVALID_ARGUMENT;
        }
        if (n_paths >= kMultiMaxConfigs || n_paths * (size_t) W >= kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        const uint32_t max_waypoints = S.max_waypoints ? S.max_waypoints : kSimpDefaultWaypoints;
        if (max_waypoints > kSimpMaxWaypoints) return VMV_ERR_INVALID_ARGUMENT;
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
        check_every = S.check_every ? S.check_every : kSimpDefaultCheckEvery;
        return VMV_OK;
    }
}  // namespace vmv

extern "C"
{
    int vmv_simplify_multi(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                           const vmv_simplify_settings *settings, vmv_paths **out)
    {
        vmv::SimplifyParams P{};
        uint32_t check_every = 0;
        if (int rc = vmv::simplify_checks(robot, envs, n_paths, points, offsets, settings, out, P, check_every); rc != VMV_OK) return rc;
        return vmv::lockstep_call(robot, envs, n_paths, (int) P.dim, out, [&](vmv_paths *paths) {
            return vmv::simplify_multi_run(robot, envs, n_paths, points, offsets, P, check_every, paths);
        });
    }

    int vmv_simplify_multi_constrained(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                                       const vmv_simplify_settings *settings, const vmv_ee_constraint *constraints, size_t n_constraints,
                                       const vmv_constraint_settings *constraint_settings, vmv_paths **out)
    {
        // vmv_simplify_multi's checks in its order, then the constraint's own in vmv_constraint_project_batch's; none needs a device
        vmv::SimplifyParams P{};
        uint32_t check_every = 0;
        if (int rc = vmv::simplify_checks(robot, envs, n_paths, points, offsets, settings, out, P, check_every); rc != VMV_OK) return rc;
        vmv::ConstraintBand cb{};
        const std::string err = vmv::constraint_band_checks(constraints, n_constraints, constraint_settings, n_paths, "n_paths", nullptr, cb);
        if (!err.empty()) return vmv::refuse_argument(err.c_str());
        const int rc = vmv::lockstep_call(robot, envs, n_paths, (int) P.dim, out, [&](vmv_paths *paths) {
            float lower[16], span[16], descale[16];
            if (int rb = vmv_robot_bounds(robot, lower, span, descale); rb != VMV_OK) return rb;
            vmv::constraint_band_bounds(cb, lower, span, (int) P.dim);
            return vmv::simplify_multi_run(robot, envs, n_paths, points, offsets, P, check_every, paths, &cb);
        });
        if (rc == VMV_OK) (*out)->constrained = true, (*out)->band_refused.resize(n_paths);
        return rc;
    }

    int vmv_paths_band_refused(const vmv_paths *paths, uint32_t *refused)
    {
        if (!paths || !paths->constrained) return VMV_ERR_INVALID_ARGUMENT;
        if (refused && paths->n) std::memcpy(refused, paths->band_refused.data(), paths->n * 4);
        return VMV_OK;
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
