// vmv_retime_multi.hip — time-optimal trajectories along many independent paths (vmv_retime_multi).  The host
// sets every path up in float64 from the fp32 waypoints (vmv_retime_path.h: straight pieces and parabolic blends, each
// cut into equal intervals), so it knows every path's grid and the packed layout before anything is launched.  ONE
// launch of retime_profile_kernel (one wave per path) computes the velocity profile on that grid; the host reads the
// durations and lays the samples out; ONE launch of retime_sample_kernel (one lane per sample) evaluates the trajectory
// every dt; with environments, ONE vmv_validate_motion_batch_multi call checks all consecutive sample pairs.  The contract
// is in include/vamp_mvt_amd.h; tests/retime_serial.py states it in numpy.
//
// The prologue is the existing calls' own: the handles are checked by an empty vmv_validate_batch_multi batch (robot,
// NULL, finalized; no device), then the device, then the environments' device and robot parts by vmv_env_prepare_multi.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"
#include "vmv_retime_path.h"

#include <cmath>
#include <cstring>

struct vmv_trajectories
{
    size_t n = 0;
    int dim = 0;
    std::vector<uint8_t> status;
    std::vector<uint32_t> intervals, samples, first_invalid;
    std::vector<float> duration;
    std::vector<float> times, positions, velocities, accelerations;  // packed in path order
    uint64_t validation_calls = 0, questions = 0;
};

namespace vmv
{
    namespace
    {
        struct RetimePathDev
        {
            uint32_t piece_lo, n_pieces;  // the path's records in the piece table
            uint32_t N;                   // its intervals, 2 .. kRetimeMaxGrid
            uint32_t grid_lo;             // first of its N + 1 entries in the packed x / u / T arrays
        };

        constexpr float kRetimeTiny = 1e-6f;  // a tangent component that is not larger gives no line and no velocity cap

        __device__ __forceinline__ float wave_min(float v)
        {
            for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
            return v;
        }
        __device__ __forceinline__ float wave_max(float v)
        {
            for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
            return v;
        }

        // What lane (2 j + end) knows about joint j at one end of an interval: the tangent there, and the constraint
        // |cc u + e x| <= A as the band |u - slope x| <= g (line), or as a cap on x where cc vanishes.
        struct RetimeBand
        {
            float a;      // q'_j at the lane's end
            float slope;  // -e / cc
            float g;      // A / |cc|; +inf without a line
            float cap;    // A / |e| where |cc| <= 1e-6 and e != 0; else +inf
            bool line;
        };
        __device__ __forceinline__ RetimeBand retime_band(bool lane_used, uint32_t end, uint32_t k, float delta, float two_d, float uin,
                                                          float c, float A)
        {
            const float inf = __builtin_inff();
            RetimeBand B;
            const float s = (float) (k + end) * delta;
            B.a = uin + c * s;
            const float cc = end ? B.a + two_d * c : B.a;
            B.line = lane_used && fabsf(cc) > kRetimeTiny;
            B.slope = B.line ? (-c) / cc : 0.0f;
            B.g = B.line ? A / fabsf(cc) : inf;
            B.cap = (lane_used && !B.line && c != 0.0f) ? A / fabsf(c) : inf;
            return B;
        }

        // One wave per path.  limits: [2][16], velocity then acceleration.  gx, gu, gT: the packed per-grid-point arrays
        // (x = sdot^2 at the point, u = sddot on the interval that starts there, T = the time the point is reached).
        __global__ __launch_bounds__(64) void retime_profile_kernel(const RetimePathDev *__restrict__ paths,
                                                                    const RetimePiece *__restrict__ pieces,
                                                                    const float *__restrict__ limits, uint32_t dim,
                                                                    float *__restrict__ gx, float *__restrict__ gu,
                                                                    float *__restrict__ gT)
        {
            __shared__ float K[kRetimeMaxGrid + 1];
            const RetimePathDev P = paths[blockIdx.x];
            if (P.N < 2u || P.N > kRetimeMaxGrid) return;  // (never launched so; the whole wave leaves)
            const uint32_t lane = threadIdx.x, j = lane >> 1, end = lane & 1u, nb = 2u * dim;
            const bool used = lane < nb;
            const float V = used ? limits[j] : 1.0f, A = used ? limits[16 + j] : 1.0f;
            const RetimePiece *pc = pieces + P.piece_lo;
            const float inf = __builtin_inff();
            const uint32_t pair_rounds = (nb * nb + 63u) / 64u;

            // 1. what does not depend on the neighbour: per grid point the caps, the velocity caps of the two tangents that
            // meet there, and the smallest threshold over all (lower line, upper line) pairs of the interval's joint lines
            float carry = inf;  // the velocity cap of the previous interval's end tangent
            for (uint32_t pi = 0; pi < P.n_pieces; ++pi)
            {
                const RetimePiece &R = pc[pi];
                const uint32_t n = R.n, first = R.first, stop = R.stop;
                const float d = R.d, delta = R.span / (float) n, two_d = delta + delta;
                const float uin = used ? R.u_in[j] : 0.0f;
                const float c = (used && d > 0.0f) ? (R.u_out[j] - uin) / (d + d) : 0.0f;
                for (uint32_t k = 0; k < n; ++k)
                {
                    const RetimeBand B = retime_band(used, end, k, delta, two_d, uin, c, A);
                    float vc = inf;
                    if (used && fabsf(B.a) > kRetimeTiny)
                    {
                        const float r = V / fabsf(B.a);
                        vc = r * r;
                    }
                    for (int m = 2; m < 64; m <<= 1) vc = fminf(vc, __shfl_xor(vc, m));  // even lanes: start, odd lanes: end
                    const float v_start = __shfl(vc, 0), v_end = __shfl(vc, 1);
                    float th = B.cap;
                    for (uint32_t r = 0; r < pair_rounds; ++r)
                    {
                        const uint32_t pq = r * 64u + lane;
                        const bool in = pq < nb * nb;
                        const uint32_t p = in ? pq / nb : 0u, q = in ? pq - p * nb : 0u;
                        const float sp = __shfl(B.slope, (int) p), gp = __shfl(B.g, (int) p);
                        const float sq = __shfl(B.slope, (int) q), gq = __shfl(B.g, (int) q);
                        const float den = sp - sq;  // lower line of band p against upper line of band q
                        if (in && den > 0.0f) th = fminf(th, (gp + gq) / den);
                    }
                    th = wave_min(th);
                    float Ki = fminf(fminf(th, v_start), carry);
                    carry = v_end;
                    if (k == 0u && stop) Ki = 0.0f;
                    if (lane == 0u) K[first + k] = Ki;
                }
            }
            if (lane == 0u) K[P.N] = 0.0f;
            __syncthreads();

            // 2. backward: K_i = the largest x from which K_{i+1} can be reached
            float Knext = 0.0f;
            for (uint32_t pi = P.n_pieces; pi-- > 0u;)
            {
                const RetimePiece &R = pc[pi];
                const uint32_t n = R.n, first = R.first;
                const float d = R.d, delta = R.span / (float) n, two_d = delta + delta;
                const float uin = used ? R.u_in[j] : 0.0f;
                const float c = (used && d > 0.0f) ? (R.u_out[j] - uin) / (d + d) : 0.0f;
                for (uint32_t k = n; k-- > 0u;)
                {
                    const RetimeBand B = retime_band(used, end, k, delta, two_d, uin, c, A);
                    // the reach lines u >= -x / (2 Delta) and u <= (K_{i+1} - x) / (2 Delta) against the band, both sides
                    // of each quotient multiplied by 2 Delta: an interval of 1e-9 costs no digit this way
                    const float sd = B.slope * two_d, gd = B.g * two_d;
                    const float den1 = -1.0f - sd;  // the reach's lower line against the band's upper line
                    const float den2 = 1.0f + sd;   // the band's lower line against the reach's upper line
                    float th = inf;
                    if (B.line && den1 > 0.0f) th = gd / den1;
                    if (B.line && den2 > 0.0f) th = fminf(th, (Knext + gd) / den2);
                    th = wave_min(th);
                    const float Ki = fmaxf(0.0f, fminf(K[first + k], th));
                    if (lane == 0u) K[first + k] = Ki;
                    Knext = Ki;
                }
            }
            __syncthreads();

            // 3. forward: the largest feasible u at every point, then the times
            float x = 0.0f, T = 0.0f;
            float *px = gx + P.grid_lo, *pu = gu + P.grid_lo, *pT = gT + P.grid_lo;
            for (uint32_t pi = 0; pi < P.n_pieces; ++pi)
            {
                const RetimePiece &R = pc[pi];
                const uint32_t n = R.n, first = R.first;
                const float d = R.d, delta = R.span / (float) n, two_d = delta + delta;
                const float uin = used ? R.u_in[j] : 0.0f;
                const float c = (used && d > 0.0f) ? (R.u_out[j] - uin) / (d + d) : 0.0f;
                for (uint32_t k = 0; k < n; ++k)
                {
                    const RetimeBand B = retime_band(used, end, k, delta, two_d, uin, c, A);
                    const float Kn = K[first + k + 1u];
                    const float sx = B.slope * x;
                    const float up = wave_min(B.line ? B.g + sx : inf);
                    const float lo = wave_max(B.line ? sx - B.g : -inf);
                    const float u = fmaxf(fminf(up, (Kn - x) / two_d), fmaxf(lo, (-x) / two_d));
                    const float xn = fminf(fmaxf(x + two_d * u, 0.0f), Kn);
                    const float Tn = T + two_d / (sqrtf(x) + sqrtf(xn));
                    if (lane == 0u) px[first + k] = x, pu[first + k] = u, pT[first + k] = T;
                    x = xn, T = Tn;
                }
            }
            if (lane == 0u) px[P.N] = x, pu[P.N] = 0.0f, pT[P.N] = T;
        }

        // One lane per (path, sample).  sample_lo: [n_paths + 1] first sample of each path of the list; the outputs are
        // packed in the list's order.
        __global__ __launch_bounds__(256) void retime_sample_kernel(const RetimePathDev *__restrict__ paths,
                                                                     const RetimePiece *__restrict__ pieces,
                                                                     const uint32_t *__restrict__ sample_lo, uint32_t n_paths,
                                                                     uint32_t dim, float dt, const float *__restrict__ gx,
                                                                     const float *__restrict__ gu, const float *__restrict__ gT,
                                                                     float *__restrict__ times, float *__restrict__ pos,
                                                                     float *__restrict__ vel, float *__restrict__ acc)
        {
            const uint32_t g = blockIdx.x * 256u + threadIdx.x;
            if (g >= sample_lo[n_paths]) return;
            uint32_t lo = 0u, hi = n_paths - 1u;  // the last path whose first sample is not behind g
            while (lo < hi)
            {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                if (sample_lo[mid] <= g) lo = mid;
                else hi = mid - 1u;
            }
            const RetimePathDev P = paths[lo];
            const uint32_t k = g - sample_lo[lo];
            const float *px = gx + P.grid_lo, *pu = gu + P.grid_lo, *pT = gT + P.grid_lo;
            const float t = fminf((float) k * dt, pT[P.N]);
            uint32_t i = 0u;  // the last interval that starts at or before t
            hi = P.N - 1u;
            while (i < hi)
            {
                const uint32_t mid = (i + hi + 1u) >> 1;
                if (pT[mid] <= t) i = mid;
                else hi = mid - 1u;
            }
            const RetimePiece *pc = pieces + P.piece_lo;
            uint32_t a = 0u;  // its piece
            hi = P.n_pieces - 1u;
            while (a < hi)
            {
                const uint32_t mid = (a + hi + 1u) >> 1;
                if (pc[mid].first <= i) a = mid;
                else hi = mid - 1u;
            }
            const RetimePiece &R = pc[a];
            const float delta = R.span / (float) R.n, d = R.d;
            const float s0 = (float) (i - R.first) * delta;
            const float x = px[i], u = pu[i], tau = t - pT[i];
            const float sigma = fminf(fmaxf(sqrtf(x) * tau + (0.5f * u) * (tau * tau), 0.0f), delta);
            const float s = s0 + sigma, ss = s * s;
            const float xs = fmaxf(x + (u + u) * sigma, 0.0f), rate = sqrtf(xs);
            times[g] = t;
            const size_t row = (size_t) g * dim;
            for (uint32_t j = 0; j < dim; ++j)
            {
                const float uin = R.u_in[j];
                const float c = d > 0.0f ? (R.u_out[j] - uin) / (d + d) : 0.0f;
                const float qp = uin + c * s;
                pos[row + j] = (R.base[j] + uin * s) + (0.5f * c) * ss;
                vel[row + j] = qp * rate;
                acc[row + j] = qp * u + c * xs;
            }
        }

        struct RetimeHostSettings
        {
            double blend, grid_step;
            float dt;
            uint32_t max_grid, max_samples;
            bool stop_at_waypoints;
        };

        // The caller has checked every argument, n > 0, and (with envs) every environment is finalized on the current
        // device with the robot's part built.
        int retime_multi_run(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                             const float *vel_limits, const float *acc_limits, const RetimeHostSettings &S, vmv_trajectories *res)
        {
            const size_t dim = (size_t) res->dim;
            hipStream_t stream = nullptr;
            res->n = n;
            res->status.assign(n, VMV_RETIME_COMPLETE), res->intervals.assign(n, 0), res->samples.assign(n, 0);
            res->first_invalid.assign(n, VMV_RETIME_NONE), res->duration.assign(n, 0.0f);

            // the paths: every N, the packed grid, who takes part
            std::vector<RetimePiece> pieces;
            std::vector<RetimePathDev> recs;
            std::vector<uint32_t> part;
            uint64_t grid = 0;
            for (size_t p = 0; p < n; ++p)
            {
                const size_t count = offsets[p + 1] - offsets[p];
                const RetimePath H = retime_path(count ? points + offsets[p] * dim : nullptr, count, dim, S.blend, S.grid_step,
                                                 S.max_grid, S.stop_at_waypoints);
                res->intervals[p] = (uint32_t) std::min<uint64_t>(H.intervals, 0xffffffffull);
                if (H.what == kRetimeNonFinite) res->status[p] = VMV_RETIME_NON_FINITE;
                else if (H.what == kRetimeTooLong) res->status[p] = VMV_RETIME_TOO_LONG;
                else if (H.what == kRetimeTrivial) res->samples[p] = H.distinct ? 1u : 0u;
                else
                {
                    recs.push_back(RetimePathDev{(uint32_t) pieces.size(), (uint32_t) H.pieces.size(), (uint32_t) H.intervals, (uint32_t) grid});
                    pieces.insert(pieces.end(), H.pieces.begin(), H.pieces.end());
                    grid += H.intervals + 1u;
                    part.push_back((uint32_t) p);
                    if (grid >= kMultiMaxConfigs || pieces.size() >= kMultiMaxConfigs)
                        return refuse_argument("vmv_retime_multi: the paths' grids together have 2^31 points or more");
                }
            }

            int device = 0;
            VMV_LOCKSTEP_HIP(hipGetDevice(&device));  // (a call whose paths are all trivial needs a device as well)
            std::vector<float> s_times, s_pos, s_vel, s_acc;  // the sampled paths' rows, in `sampled` order
            std::vector<uint32_t> sampled, sample_lo;
            if (!part.empty())
            {
                const auto padded = [](size_t bytes) { return (bytes + 255) & ~size_t{255}; };
                const size_t np = part.size();
                const size_t at_pieces = padded(np * sizeof(RetimePathDev)), at_limits = at_pieces + padded(pieces.size() * sizeof(RetimePiece));
                const size_t at_x = at_limits + padded(32 * 4), at_u = at_x + padded(grid * 4), at_T = at_u + padded(grid * 4);
                DeviceBuffers mem;
                char *base = nullptr;
                VMV_LOCKSTEP_HIP(mem.alloc(&base, at_T + padded(grid * 4)));
                RetimePathDev *d_paths = reinterpret_cast<RetimePathDev *>(base);
                RetimePiece *d_pieces = reinterpret_cast<RetimePiece *>(base + at_pieces);
                float *d_limits = reinterpret_cast<float *>(base + at_limits);
                float *d_x = reinterpret_cast<float *>(base + at_x), *d_u = reinterpret_cast<float *>(base + at_u);
                float *d_T = reinterpret_cast<float *>(base + at_T);
                float limits[32] = {};
                for (size_t j = 0; j < dim; ++j) limits[j] = vel_limits[j], limits[16 + j] = acc_limits[j];
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_paths, recs.data(), np * sizeof(RetimePathDev), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(RetimePiece), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_limits, limits, sizeof(limits), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemsetAsync(d_T, 0, grid * 4, stream));
                hipLaunchKernelGGL(retime_profile_kernel, dim3((uint32_t) np), dim3(64), 0, stream, d_paths, d_pieces, d_limits,
                                   (uint32_t) dim, d_x, d_u, d_T);
                VMV_LOCKSTEP_HIP(hipGetLastError());
                std::vector<float> T(grid);
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(T.data(), d_T, grid * 4, hipMemcpyDeviceToHost, stream));
                VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));

                // the durations, the samples' layout, who is sampled
                std::vector<RetimePathDev> srecs;
                uint64_t rows = 0;
                for (size_t a = 0; a < np; ++a)
                {
                    const uint32_t p = part[a];
                    bool finite = true;
                    for (uint32_t i = 0; i <= recs[a].N && finite; ++i) finite = std::isfinite(T[recs[a].grid_lo + i]);
                    if (!finite)
                    {
                        res->status[p] = VMV_RETIME_STALLED;
                        continue;
                    }
                    const float Tp = T[recs[a].grid_lo + recs[a].N];
                    res->duration[p] = Tp;
                    const uint64_t count = retime_samples(Tp, S.dt);
                    if (count > S.max_samples)
                    {
                        res->status[p] = VMV_RETIME_TOO_LONG;
                        continue;
                    }
                    res->samples[p] = (uint32_t) count;
                    sample_lo.push_back((uint32_t) rows), sampled.push_back(p), srecs.push_back(recs[a]);
                    rows += count;
                    if (rows >= kMultiMaxConfigs) return refuse_argument("vmv_retime_multi: the trajectories together have 2^31 samples or more");
                }
                sample_lo.push_back((uint32_t) rows);
                if (!sampled.empty())
                {
                    const size_t ns = sampled.size();
                    const size_t at_t = padded((ns + 1) * 4), at_p = at_t + padded(rows * 4);
                    const size_t each = padded(rows * dim * 4);
                    char *out = nullptr;
                    VMV_LOCKSTEP_HIP(mem.alloc(&out, at_p + 3 * each));
                    uint32_t *d_slo = reinterpret_cast<uint32_t *>(out);
                    float *d_t = reinterpret_cast<float *>(out + at_t), *d_p = reinterpret_cast<float *>(out + at_p);
                    float *d_v = reinterpret_cast<float *>(out + at_p + each), *d_a = reinterpret_cast<float *>(out + at_p + 2 * each);
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_paths, srecs.data(), ns * sizeof(RetimePathDev), hipMemcpyHostToDevice, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_slo, sample_lo.data(), (ns + 1) * 4, hipMemcpyHostToDevice, stream));
                    hipLaunchKernelGGL(retime_sample_kernel, dim3((uint32_t) ((rows + 255) / 256)), dim3(256), 0, stream, d_paths,
                                       d_pieces, d_slo, (uint32_t) ns, (uint32_t) dim, S.dt, d_x, d_u, d_T, d_t, d_p, d_v, d_a);
                    VMV_LOCKSTEP_HIP(hipGetLastError());
                    s_times.resize(rows), s_pos.resize(rows * dim), s_vel.resize(rows * dim), s_acc.resize(rows * dim);
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(s_times.data(), d_t, rows * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(s_pos.data(), d_p, rows * dim * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(s_vel.data(), d_v, rows * dim * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(s_acc.data(), d_a, rows * dim * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
                }
            }

            // the packed result: row 0 and the last row of a sampled path carry its first and last waypoint's bits at rest;
            // a path of one distinct waypoint is that waypoint at rest
            size_t total = 0;
            for (size_t p = 0; p < n; ++p) total += res->samples[p];
            res->times.assign(total, 0.0f), res->positions.assign(total * dim, 0.0f);
            res->velocities.assign(total * dim, 0.0f), res->accelerations.assign(total * dim, 0.0f);
            std::vector<size_t> row_of(n + 1, 0);
            for (size_t p = 0; p < n; ++p) row_of[p + 1] = row_of[p] + res->samples[p];
            for (size_t a = 0; a < sampled.size(); ++a)
            {
                const uint32_t p = sampled[a];
                const size_t count = res->samples[p], from = sample_lo[a], to = row_of[p];
                std::memcpy(res->times.data() + to, s_times.data() + from, count * 4);
                std::memcpy(res->positions.data() + to * dim, s_pos.data() + from * dim, count * dim * 4);
                std::memcpy(res->velocities.data() + to * dim, s_vel.data() + from * dim, count * dim * 4);
                std::memcpy(res->accelerations.data() + to * dim, s_acc.data() + from * dim, count * dim * 4);
                std::memcpy(res->positions.data() + (to + count - 1) * dim, points + (offsets[p + 1] - 1) * dim, dim * 4);
                std::fill_n(res->velocities.data() + (to + count - 1) * dim, dim, 0.0f);
            }
            for (size_t p = 0; p < n; ++p)
                if (res->samples[p])
                {
                    std::memcpy(res->positions.data() + row_of[p] * dim, points + offsets[p] * dim, dim * 4);
                    std::fill_n(res->velocities.data() + row_of[p] * dim, dim, 0.0f);
                }

            // validation: all consecutive sample pairs, a segment per sampled path as vmv_optimize_multi lays its paths'
            // edges out
            if (envs && !sampled.empty())
            {
                const size_t ns = sampled.size();
                std::vector<const vmv_env *> seg_envs(ns);
                std::vector<size_t> edge_seg(ns + 1, 0);
                for (size_t a = 0; a < ns; ++a) seg_envs[a] = envs[sampled[a]], edge_seg[a + 1] = edge_seg[a] + res->samples[sampled[a]] - 1u;
                const size_t n_edges = edge_seg[ns];
                if (n_edges)
                {
                    std::vector<float> e_start(n_edges * dim), e_goal(n_edges * dim);
                    std::vector<uint64_t> bits((n_edges + 63) / 64 + 1, 0);
                    for (size_t a = 0; a < ns; ++a)
                    {
                        const size_t edges = edge_seg[a + 1] - edge_seg[a];
                        if (!edges) continue;
                        const float *w = res->positions.data() + row_of[sampled[a]] * dim;
                        std::memcpy(e_start.data() + edge_seg[a] * dim, w, edges * dim * 4);
                        std::memcpy(e_goal.data() + edge_seg[a] * dim, w + dim, edges * dim * 4);
                    }
                    if (int rc = vmv_validate_motion_batch_multi_host(robot, seg_envs.data(), edge_seg.data(), ns, e_start.data(),
                                                                      e_goal.data(), bits.data());
                        rc != VMV_OK)
                        return rc;
                    ++res->validation_calls, res->questions += n_edges;
                    for (size_t a = 0; a < ns; ++a)
                    {
                        const uint32_t p = sampled[a];
                        const uint32_t bad = retime_first_invalid(bits.data(), edge_seg[a], (uint32_t) (edge_seg[a + 1] - edge_seg[a]), VMV_RETIME_NONE);
                        if (bad != VMV_RETIME_NONE) res->status[p] = VMV_RETIME_COLLISION, res->first_invalid[p] = bad;
                    }
                }
            }
            return VMV_OK;
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_retime_multi(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                         const float *vel_limits, const float *acc_limits, const vmv_retime_settings *settings, vmv_trajectories **out)
    {
        using vmv::refuse_argument;
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kRetimeMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings) return refuse_argument("vmv_retime_multi: settings is NULL");
        if (!out) return refuse_argument("vmv_retime_multi: out is NULL");
        if (!vel_limits) return refuse_argument("vmv_retime_multi: vel_limits is NULL");
        if (!acc_limits) return refuse_argument("vmv_retime_multi: acc_limits is NULL");
        if (n > 0 && !offsets) return refuse_argument("vmv_retime_multi: offsets is NULL");
        const vmv_retime_settings &S = *settings;
        if (!std::isfinite(S.blend)) return refuse_argument("vmv_retime_multi: blend is not finite");
        if (!std::isfinite(S.grid_step)) return refuse_argument("vmv_retime_multi: grid_step is not finite");
        if (!std::isfinite(S.dt)) return refuse_argument("vmv_retime_multi: dt is not finite");
        if (S.grid_step > 0.0f && S.grid_step < 1e-6f) return refuse_argument("vmv_retime_multi: grid_step is below 1e-6");
        if (S.dt > 0.0f && S.dt < 1e-6f) return refuse_argument("vmv_retime_multi: dt is below 1e-6");
        if (S.max_grid > vmv::kRetimeMaxGrid) return refuse_argument("vmv_retime_multi: max_grid is above 4,096");
        if (S.stop_at_waypoints != 0 && S.stop_at_waypoints != 1) return refuse_argument("vmv_retime_multi: stop_at_waypoints is neither 0 nor 1");
        for (int j = 0; j < dim; ++j)
        {
            if (!(std::isfinite(vel_limits[j]) && vel_limits[j] > 0.0f))
                return refuse_argument(("vmv_retime_multi: vel_limits[" + std::to_string(j) + "] is not finite and positive").c_str());
            if (!(std::isfinite(acc_limits[j]) && acc_limits[j] > 0.0f))
                return refuse_argument(("vmv_retime_multi: acc_limits[" + std::to_string(j) + "] is not finite and positive").c_str());
        }
        if (n >= vmv::kMultiMaxConfigs) return refuse_argument("vmv_retime_multi: n is 2^31 or more");
        if (n > 0 && offsets[0] != 0) return refuse_argument("vmv_retime_multi: offsets[0] is not 0");
        for (size_t k = 0; k < n; ++k)
            if (offsets[k + 1] < offsets[k])
                return refuse_argument(("vmv_retime_multi: offsets decrease at " + std::to_string(k + 1)).c_str());
        if (n > 0 && offsets[n] >= vmv::kMultiMaxConfigs) return refuse_argument("vmv_retime_multi: 2^31 waypoints or more");
        if (n > 0 && offsets[n] > 0 && !points) return refuse_argument("vmv_retime_multi: points is NULL");
        if (envs && n > 0)
        {
            static float nothing[2] = {0.f, 0.f};  // (an empty batch reads and writes no element)
            static uint64_t no_bits[2] = {0, 0};
            const std::vector<size_t> zeros(n + 1, 0);
            if (int rc = vmv_validate_batch_multi(robot, envs, zeros.data(), n, nothing, no_bits, nullptr); rc != VMV_OK) return rc;
        }
        const auto or_default = [](float v, float d) { return v > 0.0f ? v : d; };
        const vmv::RetimeHostSettings H{(double) or_default(S.blend, 0.1f), (double) or_default(S.grid_step, 0.02f), or_default(S.dt, 0.01f),
                                        S.max_grid ? S.max_grid : vmv::kRetimeMaxGrid, S.max_samples ? S.max_samples : 65536u,
                                        S.stop_at_waypoints != 0};

        vmv_trajectories *result = new (std::nothrow) vmv_trajectories;
        if (!result) return VMV_ERR_HIP;
        result->dim = dim;
        int rc = VMV_OK;
        if (n > 0)
        {
            if (envs) rc = vmv_env_prepare_multi(robot, envs, n);
            if (rc == VMV_OK) rc = vmv::retime_multi_run(robot, envs, n, points, offsets, vel_limits, acc_limits, H, result);
        }
        if (rc != VMV_OK)
        {
            delete result;
            return rc;
        }
        *out = result;
        return VMV_OK;
    }

    int vmv_retime_summary(const vmv_trajectories *result, uint8_t *status, uint32_t *intervals, uint32_t *samples, float *duration,
                           uint32_t *first_invalid, uint64_t *validation_calls, uint64_t *questions)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = result->n;
        if (status && n) std::memcpy(status, result->status.data(), n);
        if (intervals && n) std::memcpy(intervals, result->intervals.data(), n * 4);
        if (samples && n) std::memcpy(samples, result->samples.data(), n * 4);
        if (duration && n) std::memcpy(duration, result->duration.data(), n * 4);
        if (first_invalid && n) std::memcpy(first_invalid, result->first_invalid.data(), n * 4);
        if (validation_calls) *validation_calls = result->validation_calls;
        if (questions) *questions = result->questions;
        return VMV_OK;
    }

    int vmv_retime_samples(const vmv_trajectories *result, float *times, float *positions, float *velocities, float *accelerations,
                           size_t capacity_samples)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        const size_t total = result->times.size(), dim = (size_t) result->dim;
        if (total && (!times || !positions || !velocities || !accelerations)) return VMV_ERR_INVALID_ARGUMENT;
        if (capacity_samples < total) return VMV_ERR_CAPACITY;
        if (total)
        {
            std::memcpy(times, result->times.data(), total * 4);
            std::memcpy(positions, result->positions.data(), total * dim * 4);
            std::memcpy(velocities, result->velocities.data(), total * dim * 4);
            std::memcpy(accelerations, result->accelerations.data(), total * dim * 4);
        }
        return VMV_OK;
    }

    int vmv_retime_destroy(vmv_trajectories *result)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        delete result;
        return VMV_OK;
    }
}
