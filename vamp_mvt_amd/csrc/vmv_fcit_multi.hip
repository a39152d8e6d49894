// vmv_fcit_multi.hip — a lazy search of the complete graph over many independent problems (vmv_fcit_multi).
//
// The vertices are vmv_prm_multi's (vmv_prm_common.h: the same memory layout, the same stage 1 with its ONE
// vmv_validate_batch_multi call).  Then lockstep rounds
// (vmv_lockstep.h): per round fcit_step_kernel, one workgroup per unfinished problem, consumes the answers to the
// problem's previous questions, advances the serial algorithm — A* over the valid vertices with every unchecked edge taken
// as free, the proposed path's edges asked from the start, the first invalid one blocked, search again — until it needs an
// answer it does not have, and writes questions_per_round edge questions: slot 0 is that answer, the others are
// predictions that only fill the answer cache.
//
// Arithmetic contract: fp32, one rounding per written operation (-ffp-contract=off; sqrtf is correctly rounded on
// gfx950).  d2(u, v) = the sum over the joints in order of (u[j] - v[j])^2 (symmetric bit for bit), w = sqrtf(d2),
// h(v) = w(v, 1); a search pops the open vertex least by (the bits of fl(g + h), vertex id) — non-negative floats order as
// unsigned integers — and never reopens a closed vertex.  Joints beyond the robot's are taken as zeros: adding +0 to a
// non-negative sum changes no bit.
// Pair state per problem, in global memory, two V x row_words bit matrices: `answers` holds the two cache bits of the pair
// {a, b}, a < b — the low bit at [a][b], the high bit at [b][a]: 0 unknown, 1 answered valid, 2 answered invalid, 3 valid
// and reached by the serial walk — and `blocked` is symmetric (a search reads the popped vertex's row).  One thread of the
// workgroup writes them; plain vector stores; atomics on LDS words only.  Every loop has a bound that holds whatever the
// data says.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_plans.h"
#include "vmv_prm_common.h"

#include <cmath>
#include <cstring>

namespace vmv
{
    namespace
    {
        constexpr uint32_t kFcitBlock = 256, kFcitWaves = kFcitBlock / kWave;
        constexpr uint32_t kFcitMinSamples = 64, kFcitMaxSamples = 2048;
        constexpr uint32_t kFcitMaxVertices = kFcitMaxSamples + 2;
        constexpr uint32_t kFcitMaxQuestions = 32;
        constexpr uint32_t kFcitDefaultCheckEvery = 4;
        constexpr uint32_t kFcitSearchCap = 64;   // searches per problem per round, committed and speculative together
        constexpr uint32_t kFcitMaxOverlay = 64;  // pairs a round's predictions may assume invalid
        constexpr unsigned long long kNoKey = ~0ull;

        enum : uint32_t { kPhaseInit = 0, kPhaseRun = 1, kPhaseDone = 2 };
        enum : uint32_t { kUnseen = 0, kOpen = 1, kClosed = 2 };
        enum : uint32_t { kWalkAsk = 0, kWalkBlocked = 1, kWalkSolved = 2 };

        struct FcitParams
        {
            uint32_t dim, n_samples, V, row_words, W, max_iterations, n_problems;
        };

        struct FcitState  // 56 bytes per problem; all zeros = a problem not yet started
        {
            uint32_t phase, status, iterations, blocked, known_valid, valid_vertices, questions;
            uint32_t have_path, path_len, pos;  // the proposed path (walk[0 .. path_len)) and the walk's next edge
            uint32_t slot_base, n_asked;        // the questions in flight: answers bits[slot_base + s], pairs asked[s]
            float cost;
            uint32_t pad;
        };

        struct FcitArrays
        {
            float *verts;           // [P * n_samples + 2 * P][dim], vmv_prm_multi's layout
            const uint64_t *vbits;  // validity of the vertices, in that order
            uint64_t *skips;        // [P] the Halton skips stage 1 samples after
            uint32_t *answers;      // [P][V][row_words]
            uint32_t *blocked;      // [P][V][row_words]
            uint32_t *walk;         // [P][V] the proposed path's vertex ids, start first
            uint32_t *asked;        // [P][W][2] the pairs a < b of the questions in flight
            FcitState *state;       // [P]
            uint8_t *done;          // [P]
            const uint32_t *active;
            float *q_start, *q_goal;  // [active][W][dim]
            const uint64_t *bits;
        };

        // the pair state of one problem; a < b wherever a pair is named
        struct PairBits
        {
            uint32_t *answers, *blocked;
            uint32_t row_words;
            __device__ __forceinline__ uint32_t get(uint32_t *m, uint32_t r, uint32_t c) const
            {
                return (m[(size_t) r * row_words + (c >> 5)] >> (c & 31u)) & 1u;
            }
            __device__ __forceinline__ void set(uint32_t *m, uint32_t r, uint32_t c) const
            {
                m[(size_t) r * row_words + (c >> 5)] |= 1u << (c & 31u);
            }
            __device__ __forceinline__ uint32_t answer(uint32_t a, uint32_t b) const { return get(answers, a, b) | (get(answers, b, a) << 1); }
            __device__ __forceinline__ void set_answer(uint32_t a, uint32_t b, uint32_t bits) const
            {
                if (bits & 1u) set(answers, a, b);
                if (bits & 2u) set(answers, b, a);
            }
            __device__ __forceinline__ void block(uint32_t a, uint32_t b) const { set(blocked, a, b), set(blocked, b, a); }
        };

        // what a workgroup keeps in LDS: the valid vertices in ascending id order (index 0 = start, 1 = goal) and their
        // search arrays, 13 bytes per vertex
        struct FcitLds
        {
            uint32_t g[kFcitMaxVertices];  // bits of a non-negative float
            float h[kFcitMaxVertices];
            uint16_t parent[kFcitMaxVertices], vid[kFcitMaxVertices];
            uint8_t flag[kFcitMaxVertices];
            unsigned long long words[kFcitMaxSamples / 64], red[kFcitWaves];
            uint32_t prefix[kFcitMaxSamples / 64 + 1];
            uint32_t overlay[kFcitMaxOverlay][2];  // pairs a search takes as blocked on top of `blocked`
            uint32_t other[kFcitMaxOverlay], n_other;  // the popped vertex's partners among them
            uint32_t ask[kFcitMaxQuestions][2];
            uint32_t n_ask, n_overlay, go_on;
            uint32_t walk_out, walk_a, walk_b, walk_pos, walk_known, walk_blocked;
        };

        // One A* search over the valid vertices, the pairs of `blocked` and the first n_overlay of L.overlay left out.
        // Called by the whole workgroup with workgroup-uniform arguments; returns alike in every thread: true = the goal
        // was popped (L.parent leads from index 1 back to 0, L.g[1] is the cost).  At most n_valid pops.
        template <int DIM>
        __device__ bool fcit_search(const FcitParams &P, const FcitArrays &D, FcitLds &L, const PairBits &B, uint32_t p, uint32_t n_valid,
                                    uint32_t n_overlay)
        {
            const uint32_t tid = threadIdx.x, dim = P.dim;
            __syncthreads();  // whoever still reads the last search's arrays
            for (uint32_t i = tid; i < n_valid; i += kFcitBlock) L.g[i] = i == 0u ? 0u : kInfBits, L.flag[i] = i == 0u ? kOpen : kUnseen;
            __syncthreads();
            for (uint32_t pop = 0; pop < n_valid; ++pop)
            {
                unsigned long long best = kNoKey;
                for (uint32_t i = tid; i < n_valid; i += kFcitBlock)
                    if (L.flag[i] == kOpen)
                    {
                        const float f = __uint_as_float(L.g[i]) + L.h[i];
                        const unsigned long long key = ((unsigned long long) __float_as_uint(f) << 32) | i;
                        best = key < best ? key : best;
                    }
#pragma unroll
                for (int off = kWave / 2; off >= 1; off >>= 1)
                {
                    const unsigned long long o = __shfl_xor(best, off, kWave);
                    best = o < best ? o : best;
                }
                if (tid % kWave == 0u) L.red[tid / kWave] = best;
                if (tid == 0u) L.n_other = 0u;
                __syncthreads();
#pragma unroll
                for (uint32_t w = 0; w < kFcitWaves; ++w) best = L.red[w] < best ? L.red[w] : best;
                if (best == kNoKey) return false;
                const uint32_t u = (uint32_t) best;  // indices ascend with the vertex ids
                if (u == 1u) return true;
                const uint32_t uid = L.vid[u];
                const float gu = __uint_as_float(L.g[u]);
                if (n_overlay)  // (uniform)
                {
                    if (tid < n_overlay && (L.overlay[tid][0] == uid || L.overlay[tid][1] == uid))
                        L.other[atomicAdd(&L.n_other, 1u)] = L.overlay[tid][0] == uid ? L.overlay[tid][1] : L.overlay[tid][0];
                    __syncthreads();
                }
                float q[DIM];
                {
                    const float *src = D.verts + vertex_at(P, p, uid) * dim;
#pragma unroll
                    for (int j = 0; j < DIM; ++j) q[j] = (uint32_t) j < dim ? src[j] : 0.f;
                }
                const uint32_t n_other = L.n_other;
                const uint32_t *row = B.blocked + (size_t) uid * B.row_words;
                for (uint32_t i = tid; i < n_valid; i += kFcitBlock)
                {
                    if (i == u || L.flag[i] == kClosed) continue;
                    const uint32_t v = L.vid[i];
                    if ((row[v >> 5] >> (v & 31u)) & 1u) continue;
                    bool skip = false;
                    for (uint32_t t = 0; t < n_other; ++t) skip |= L.other[t] == v;
                    if (skip) continue;
                    const float *src = D.verts + vertex_at(P, p, v) * dim;
                    float sum = 0.f;
#pragma unroll
                    for (int j = 0; j < DIM; ++j)
                    {
                        const float df = q[j] - ((uint32_t) j < dim ? src[j] : 0.f);
                        sum = sum + df * df;
                    }
                    const float c = gu + sqrtf(sum);
                    if (c < __uint_as_float(L.g[i])) L.g[i] = __float_as_uint(c), L.parent[i] = (uint16_t) u, L.flag[i] = kOpen;
                }
                if (tid == 0u) L.flag[u] = kClosed;
                __syncthreads();
            }
            return false;
        }

        // One workgroup per active problem; every branch below is taken by the whole workgroup (its conditions are values
        // every thread holds alike: the state, or LDS words read after a barrier).
        template <int DIM>
        __global__ __launch_bounds__(kFcitBlock) void fcit_step_kernel(const FcitParams P, const FcitArrays D)
        {
            __shared__ FcitLds L;
            const uint32_t a = blockIdx.x, p = D.active[a], tid = threadIdx.x, dim = P.dim, V = P.V, W = P.W, ns = P.n_samples;
            FcitState st = D.state[p];
            float *qs = D.q_start + (size_t) a * W * dim, *qg = D.q_goal + (size_t) a * W * dim;
            const float *start = D.verts + vertex_at(P, p, 0) * dim;
            const PairBits B{D.answers + (size_t) p * V * P.row_words, D.blocked + (size_t) p * V * P.row_words, P.row_words};
            uint32_t *walk = D.walk + (size_t) p * V, *asked = D.asked + (size_t) p * W * 2u;
            bool finish = st.phase == kPhaseDone, have_question = false;
            uint32_t n_valid = 0;

            if (st.phase != kPhaseDone)
            {
                // the valid vertices in ascending id order; h of each
                const uint32_t n_words = ns / 64u;
                if (tid < n_words) L.words[tid] = D.vbits[(size_t) p * n_words + tid];  // the samples own whole words
                __syncthreads();
                if (tid == 0u)
                {
                    uint32_t sum = 2u;
                    for (uint32_t w = 0; w < n_words; ++w) L.prefix[w] = sum, sum += (uint32_t) __popcll(L.words[w]);
                    L.prefix[n_words] = sum;
                }
                __syncthreads();
                const bool ends_ok = ends_valid(P, D.vbits, p);
                n_valid = L.prefix[n_words];
                if (st.phase == kPhaseInit)
                {
                    st.valid_vertices = n_valid - 2u + (bit_at(D.vbits, vertex_at(P, p, 0)) ? 1u : 0u) + (bit_at(D.vbits, vertex_at(P, p, 1)) ? 1u : 0u);
                    st.phase = kPhaseRun;
                    if (!ends_ok) st.status = VMV_PLAN_INVALID_ENDPOINT, finish = true;
                }
                else if (tid == 0u)  // the answers to the questions in flight go into the cache
                    for (uint32_t s = 0; s < st.n_asked && s < W; ++s)
                    {
                        const uint32_t x = asked[2u * s], y = asked[2u * s + 1u], slot = st.slot_base + s;
                        if (x < y && y < V && B.answer(x, y) == 0u) B.set_answer(x, y, ((D.bits[slot >> 6] >> (slot & 63u)) & 1ull) ? 1u : 2u);
                    }
                if (!finish)
                {
                    const float *goal = D.verts + vertex_at(P, p, 1) * dim;
                    for (uint32_t v = tid; v < V; v += kFcitBlock)
                    {
                        uint32_t i = v;
                        if (v >= 2u)
                        {
                            const unsigned long long word = L.words[(v - 2u) >> 6];
                            const uint32_t bit = (v - 2u) & 63u;
                            if (!((word >> bit) & 1ull)) continue;
                            i = L.prefix[(v - 2u) >> 6] + (uint32_t) __popcll(word & ((1ull << bit) - 1ull));
                        }
                        const float *src = D.verts + vertex_at(P, p, v) * dim;
                        float sum = 0.f;
                        for (uint32_t j = 0; j < dim; ++j)
                        {
                            const float df = src[j] - goal[j];
                            sum = sum + df * df;
                        }
                        L.vid[i] = (uint16_t) v, L.h[i] = sqrtf(sum);
                    }
                }
                __syncthreads();
            }

            // the serial algorithm, until it needs an answer it does not have, ends, or the round's searches are used up
            uint32_t searches = 0;
            while (!finish && !have_question)  // every turn but the last runs a search: at most kFcitSearchCap + 1 turns
            {
                if (!st.have_path)
                {
                    if (st.iterations >= P.max_iterations)
                    {
                        st.status = VMV_PLAN_MAX_ITERATIONS, finish = true;
                        break;
                    }
                    if (searches >= kFcitSearchCap) break;  // null questions; the state carries on in the next round
                    ++st.iterations, ++searches;
                    if (!fcit_search<DIM>(P, D, L, B, p, n_valid, 0u))
                    {
                        st.status = VMV_PLAN_NO_PATH, finish = true;
                        break;
                    }
                    uint32_t len = 1u;
                    for (uint32_t c = 1u; c != 0u && len < n_valid; c = L.parent[c]) ++len;
                    if (tid == 0u)
                    {
                        uint32_t c = 1u;
                        for (uint32_t k = len; k-- > 0u; c = L.parent[c]) walk[k] = L.vid[c];
                    }
                    st.have_path = 1u, st.path_len = len, st.pos = 0u, st.cost = __uint_as_float(L.g[1]);
                }
                __syncthreads();  // the answers and the path are written
                if (tid == 0u)  // the walk from st.pos, serial; its bit updates are this thread's alone
                {
                    uint32_t pos = st.pos, known = st.known_valid, blocked = st.blocked, out = kWalkSolved, x = 0u, y = 0u;
                    while (pos + 1u < st.path_len)  // <= V edges
                    {
                        x = walk[pos], y = walk[pos + 1u];
                        if (x > y)
                        {
                            const uint32_t t = x;
                            x = y, y = t;
                        }
                        const uint32_t s = B.answer(x, y);
                        if (s == 0u)
                        {
                            out = kWalkAsk;
                            break;
                        }
                        if (s == 2u)
                        {
                            B.block(x, y), ++blocked, out = kWalkBlocked;
                            break;
                        }
                        if (s == 1u) B.set_answer(x, y, 2u), ++known;
                        ++pos;
                    }
                    L.walk_out = out, L.walk_a = x, L.walk_b = y, L.walk_pos = pos, L.walk_known = known, L.walk_blocked = blocked;
                }
                __syncthreads();
                st.pos = L.walk_pos, st.known_valid = L.walk_known, st.blocked = L.walk_blocked;
                if (L.walk_out == kWalkSolved)
                    st.status = VMV_PLAN_SOLVED, finish = true;
                else if (L.walk_out == kWalkBlocked)
                    st.have_path = 0u;
                else
                    have_question = true;
            }

            uint32_t n_ask = 0;
            if (have_question)
            {
                // slot 0: the walk's question.  Predictions: the path's later unknown edges (all answered valid, the walk
                // needs them next); then, taking every question of the round and every cached invalid answer met as
                // invalid, search again and ask that path's first unknown edge, as long as slots and searches last.  A
                // problem's first question, the straight edge, goes alone: where it is valid the problem ends with it.
                if (tid == 0u)
                {
                    uint32_t n = 1u;
                    L.ask[0][0] = L.overlay[0][0] = L.walk_a, L.ask[0][1] = L.overlay[0][1] = L.walk_b;
                    for (uint32_t k = st.pos + 1u; k + 1u < st.path_len && n < W; ++k)
                    {
                        const uint32_t x = min(walk[k], walk[k + 1u]), y = max(walk[k], walk[k + 1u]);
                        if (B.answer(x, y) == 0u) L.ask[n][0] = x, L.ask[n][1] = y, ++n;
                    }
                    L.n_ask = n, L.n_overlay = 1u;
                }
                __syncthreads();
                n_ask = L.n_ask;
                uint32_t n_overlay = 1u;
                while (st.iterations > 1u && n_ask < W && searches < kFcitSearchCap && n_overlay < kFcitMaxOverlay)  // each turn adds an overlay pair
                {
                    ++searches;
                    if (!fcit_search<DIM>(P, D, L, B, p, n_valid, n_overlay)) break;
                    if (tid == 0u)
                    {
                        // the first edge from the start that is not known valid = the last one met walking back
                        uint32_t fx = 0u, fy = 0u, fs = 3u, steps = 0u;
                        for (uint32_t c = 1u; c != 0u && steps < n_valid; c = L.parent[c], ++steps)
                        {
                            const uint32_t i = L.vid[c], j = L.vid[L.parent[c]], x = min(i, j), y = max(i, j), s = B.answer(x, y);
                            if (s == 0u || s == 2u) fx = x, fy = y, fs = s;
                        }
                        uint32_t go_on = 0u;
                        if (fs != 3u)
                        {
                            bool in_flight = false;
                            for (uint32_t s = 0; s < n_ask; ++s) in_flight |= L.ask[s][0] == fx && L.ask[s][1] == fy;
                            if (fs == 0u && !in_flight) L.ask[n_ask][0] = fx, L.ask[n_ask][1] = fy, L.n_ask = n_ask + 1u;
                            L.overlay[n_overlay][0] = fx, L.overlay[n_overlay][1] = fy;
                            go_on = 1u;
                        }
                        L.go_on = go_on;
                    }
                    __syncthreads();
                    n_ask = L.n_ask;
                    if (!L.go_on) break;  // a path with every edge known valid: nothing to predict beyond it
                    ++n_overlay;
                }
            }

            // the round's questions: vertex a -> vertex b of every slot in use; start -> start (the null question) elsewhere
            for (uint32_t i = tid; i < W * dim; i += kFcitBlock)
            {
                const uint32_t s = i / dim, j = i % dim;
                const bool used = s < n_ask;
                qs[i] = used ? D.verts[vertex_at(P, p, L.ask[s][0]) * dim + j] : start[j];
                qg[i] = used ? D.verts[vertex_at(P, p, L.ask[s][1]) * dim + j] : start[j];
            }
            if (tid < n_ask) asked[2u * tid] = L.ask[tid][0], asked[2u * tid + 1u] = L.ask[tid][1];
            if (tid == 0u && st.phase != kPhaseDone)
            {
                st.slot_base = a * W, st.n_asked = n_ask, st.questions += n_ask;
                if (finish)
                {
                    st.phase = kPhaseDone;
                    if (st.status != VMV_PLAN_SOLVED) st.path_len = 0u, st.cost = INFINITY;
                }
                D.state[p] = st;
                if (finish) D.done[p] = 1;
            }
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with
        // the robot's part built.
        int fcit_multi_run(int robot, int dim, const float *lower, const float *span, const vmv_env *const *envs, size_t n,
                           const float *starts, const float *goals, const uint64_t *skips, const float *samples,
                           const vmv_fcit_settings &S, vmv_plans *plans)
        {
            FcitParams P{};
            P.dim = (uint32_t) dim, P.n_samples = S.n_samples, P.V = S.n_samples + 2u, P.row_words = (P.V + 31u) / 32u;
            P.W = S.questions_per_round, P.max_iterations = S.max_iterations, P.n_problems = (uint32_t) n;
            const uint32_t check_every = S.check_every ? S.check_every : kFcitDefaultCheckEvery;
            const size_t ns = S.n_samples, V = P.V, W = P.W, n_sample_cfgs = n * ns, n_cfgs = n_sample_cfgs + 2 * n, nv = n * V;
            const size_t matrix_words = nv * P.row_words, n_slots = n * W;
            const uint32_t n32 = (uint32_t) n;
            hipStream_t stream = nullptr;

            DeviceBuffers mem;
            LockstepBuffers B;
            FcitArrays D{};
            uint64_t *d_vbits = nullptr;
            VMV_LOCKSTEP_HIP(mem.alloc(&D.verts, n_cfgs * (size_t) dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_vbits, (n_cfgs + 63) / 64));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.skips, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.answers, matrix_words));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.blocked, matrix_words));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.walk, nv));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.asked, 2 * n_slots));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
            if (int rc = B.alloc(mem, n, n, W, (size_t) dim, stream); rc != VMV_OK) return rc;
            D.vbits = d_vbits, D.done = B.done, D.active = B.active, D.q_start = B.q_start, D.q_goal = B.q_goal, D.bits = B.bits;
            VMV_LOCKSTEP_HIP(hipMemsetAsync(D.answers, 0, matrix_words * 4, stream));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(D.blocked, 0, matrix_words * 4, stream));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(D.state, 0, n * sizeof(FcitState), stream));

            // 1. vertices: vmv_prm_multi's stage 1
            if (int rc = prm_stage_vertices(robot, envs, n, S.n_samples, P.dim, starts, goals, skips, samples, lower, span, D.verts, D.skips,
                                            d_vbits, stream, "fcit_halton_kernel");
                rc != VMV_OK)
                return rc;

            // 2. the rounds.  The first leaves out the problems with an invalid endpoint: a call of nothing else asks nothing.
            std::vector<uint64_t> vbits((2 * n + 63) / 64 + 1);
            {
                const size_t first_word = n_sample_cfgs / 64;  // n_samples is a multiple of 64: the endpoints' bits start a word
                VMV_LOCKSTEP_HIP(hipMemcpy(vbits.data(), d_vbits + first_word, ((n_cfgs + 63) / 64 - first_word) * 8, hipMemcpyDeviceToHost));
            }
            std::vector<uint32_t> active;
            std::vector<const vmv_env *> active_envs;
            std::vector<uint8_t> ends_ok(n);
            for (size_t p = 0; p < n; ++p)
            {
                ends_ok[p] = ((vbits[(2 * p) >> 6] >> ((2 * p) & 63)) & 1u) && ((vbits[(2 * p + 1) >> 6] >> ((2 * p + 1) & 63)) & 1u);
                active.push_back((uint32_t) p), active_envs.push_back(envs[p]);
            }
            const bool any_ok = std::find(ends_ok.begin(), ends_ok.end(), (uint8_t) 1) != ends_ok.end();
            VMV_LOCKSTEP_HIP(hipMemcpy(B.active, active.data(), n * 4, hipMemcpyHostToDevice));
            const auto step = [&](uint32_t na) {
                if (dim <= 8)
                    hipLaunchKernelGGL(fcit_step_kernel<8>, dim3(na), dim3(kFcitBlock), 0, stream, P, D);
                else
                    hipLaunchKernelGGL(fcit_step_kernel<16>, dim3(na), dim3(kFcitBlock), 0, stream, P, D);
            };
            uint64_t rounds = 0;
            if (any_ok)
            {
                // slot 0 of a round is a pair never asked before, or the round ran kFcitSearchCap committed searches: a bound
                // on the rounds that does not depend on the device's answers
                const uint64_t max_rounds = (uint64_t) V * (V - 1) / 2 + (uint64_t) S.max_iterations / kFcitSearchCap + check_every + 2ull;
                if (int rc = lockstep_rounds(robot, stream, check_every, max_rounds, W, active, active_envs, B.arrays(), "vmv_fcit_multi",
                                             "fcit_step_kernel", step, rounds);
                    rc != VMV_OK)
                    return rc;
            }
            else  // every problem ends in its first step, with no question: the step alone, no validation call
            {
                step(n32);
                VMV_PRM_LAUNCHED("fcit_step_kernel");
            }

            // 3. results: the states, then the paths gathered on the device into one packed buffer
            std::vector<FcitState> states(n);
            VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(FcitState), hipMemcpyDeviceToHost));
            plans->n = n, plans->dim = dim, plans->rounds = 1 + rounds, plans->questions = 0;
            plans->fcit = true, plans->n_samples = S.n_samples;
            plans->status.resize(n), plans->iterations.resize(n), plans->sizes2.resize(2 * n), plans->path_lengths.resize(n);
            plans->costs.resize(n), plans->known_valid.resize(n);
            for (size_t p = 0; p < n; ++p)
            {
                const FcitState &st = states[p];
                if (st.phase != kPhaseDone) return hip_status(hipErrorUnknown, "vmv_fcit_multi: a problem did not end");
                plans->status[p] = (uint8_t) st.status;
                plans->iterations[p] = st.iterations;
                plans->sizes2[2 * p] = st.valid_vertices, plans->sizes2[2 * p + 1] = st.blocked;
                plans->path_lengths[p] = st.path_len;
                plans->costs[p] = st.cost, plans->known_valid[p] = st.known_valid;
                plans->questions += st.questions;
            }
            return pack_paths(mem, B.path_offsets, plans->path_lengths, (size_t) dim, nullptr, "fcit_gather_kernel",
                              [&](const uint64_t *d_offsets, float *d_paths) {
                                  hipLaunchKernelGGL(walk_gather_kernel, dim3((n32 + kPrmBlock - 1) / kPrmBlock), dim3(kPrmBlock), 0, stream,
                                                     PrmLayout{P.dim, P.n_samples, P.n_problems}, D.verts, D.walk, &D.state->path_len,
                                                     (uint32_t) (sizeof(FcitState) / 4), false, d_offsets, d_paths);
                              },
                              plans->paths);
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_fcit_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                       const uint64_t *halton_skips, const float *samples, const vmv_fcit_settings *settings, vmv_plans **out)
    {
        // device-free checks first; the environments' own (NULL handles again, unfinalized, another device) are those of
        // vmv_env_prepare_multi, which then builds the parts not yet built in one batch
        int dim = 0;
        if (int rc = vmv::check_planner_call(robot, settings, out, envs, n_problems, starts, goals, &dim); rc != VMV_OK) return rc;
        const uint32_t ns = settings->n_samples, W = settings->questions_per_round;
        if (ns % 64u != 0u || ns < vmv::kFcitMinSamples || ns > vmv::kFcitMaxSamples) return VMV_ERR_INVALID_ARGUMENT;
        if (W < 1u || W > vmv::kFcitMaxQuestions) return VMV_ERR_INVALID_ARGUMENT;
        if (settings->max_iterations < 1u) return VMV_ERR_INVALID_ARGUMENT;
        if (!samples && !vmv::halton_skips_ok(halton_skips, n_problems, ns)) return VMV_ERR_INVALID_ARGUMENT;
        // the words of one pair-state matrix and the questions of one round, both counted in 32 bits somewhere
        if (n_problems * (size_t) (ns + 2u) * (size_t) ((ns + 2u + 31u) / 32u) >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems * (size_t) W >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems == 0)  // an empty result is a result of this call too
        {
            vmv_plans *plans = new (std::nothrow) vmv_plans;
            if (!plans) return VMV_ERR_HIP;
            plans->dim = dim, plans->fcit = true, plans->n_samples = ns;
            *out = plans;
            return VMV_OK;
        }
        return vmv::lockstep_call(robot, envs, n_problems, dim, out, [&](vmv_plans *plans) {
            float lower[16], span[16], descale[16];
            const int rc = vmv_robot_bounds(robot, lower, span, descale);
            if (rc != VMV_OK) return rc;
            return vmv::fcit_multi_run(robot, dim, lower, span, envs, n_problems, starts, goals, halton_skips, samples, *settings,
                                       plans);
        });
    }

    int vmv_plans_fcit_summary(const vmv_plans *plans, float *costs, uint32_t *known_valid_edges)
    {
        if (!plans || !plans->fcit) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t p = 0; p < plans->n; ++p)
        {
            if (costs) costs[p] = plans->costs[p];
            if (known_valid_edges) known_valid_edges[p] = plans->known_valid[p];
        }
        return VMV_OK;
    }
}
