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

#include "vmv_constraint.h"
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
    bool levelled = false;                    // vmv_retime_multi_constrained's result: the four below are set
    std::vector<uint8_t> levels;              // one byte per input waypoint
    std::vector<uint32_t> rounds, repaired, stops;
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
        // packed in the list's order.  (The time of a sample and the two searches below stand a second time in
        // retime_sample_piece, vmv_retime_path.h, for retime_blame_kernel: the two texts must stay word for word.)
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

        // What the profile and sample kernels of one pass over some paths read, as the host lays it out
        struct RetimeLayout
        {
            std::vector<RetimePiece> pieces;
            std::vector<uint32_t> corner;  // per piece: the distinct waypoint its blend rounds (the constrained call's blame)
            std::vector<RetimePathDev> recs, srecs;  // of the paths that take part; of those that are sampled
            std::vector<uint32_t> part, sampled, sample_lo, ends;  // ends: per sampled path its first and last input waypoint
            uint64_t grid = 0, rows = 0;
        };

        // Host only: the paths of `list` set up (levels(p): a path's corner levels or nullptr) -> pieces, records and the
        // packed grid of those that take part; the others get their status and sample count.  each(p, H): the caller's own
        // look at a path's set-up, before anything of H is moved from.  `call` names the entry point in the message.
        template <typename Levels, typename Each>
        int retime_lay_out_paths(const std::vector<uint32_t> &list, const float *points, const size_t *offsets, size_t dim,
                                 const RetimeHostSettings &S, bool stop_at_waypoints, uint32_t halvings, const char *call, Levels &&levels,
                                 Each &&each, vmv_trajectories *res, RetimeLayout &L)
        {
            for (const uint32_t p : list)
            {
                const size_t count = offsets[p + 1] - offsets[p];
                RetimePath H = retime_path(count ? points + offsets[p] * dim : nullptr, count, dim, S.blend, S.grid_step, S.max_grid,
                                           stop_at_waypoints, levels(p), halvings);
                res->intervals[p] = (uint32_t) std::min<uint64_t>(H.intervals, 0xffffffffull);
                each(p, H);
                if (H.what == kRetimeNonFinite) res->status[p] = VMV_RETIME_NON_FINITE;
                else if (H.what == kRetimeTooLong) res->status[p] = VMV_RETIME_TOO_LONG;
                else if (H.what == kRetimeTrivial) res->samples[p] = H.distinct ? 1u : 0u;
                else
                {
                    L.recs.push_back(RetimePathDev{(uint32_t) L.pieces.size(), (uint32_t) H.pieces.size(), (uint32_t) H.intervals, (uint32_t) L.grid});
                    L.pieces.insert(L.pieces.end(), H.pieces.begin(), H.pieces.end());
                    L.corner.insert(L.corner.end(), H.corner.begin(), H.corner.end());
                    L.grid += H.intervals + 1u;
                    L.part.push_back(p);
                    if (L.grid >= kMultiMaxConfigs || L.pieces.size() >= kMultiMaxConfigs)
                        return refuse_argument((std::string(call) + ": the paths' grids together have 2^31 points or more").c_str());
                }
            }
            return VMV_OK;
        }

        // Host only: from the profile's T [L.grid] the durations, the sample counts and rows of the paths that are sampled,
        // the status of those that are not.
        inline int retime_lay_out_samples(const std::vector<float> &T, const size_t *offsets, const RetimeHostSettings &S, const char *call,
                                          vmv_trajectories *res, RetimeLayout &L)
        {
            for (size_t a = 0; a < L.part.size(); ++a)
            {
                const uint32_t p = L.part[a];
                const RetimePathDev &R = L.recs[a];
                bool finite = true;
                for (uint32_t i = 0; i <= R.N && finite; ++i) finite = std::isfinite(T[R.grid_lo + i]);
                if (!finite)
                {
                    res->status[p] = VMV_RETIME_STALLED;
                    continue;
                }
                const float Tp = T[R.grid_lo + R.N];
                res->duration[p] = Tp;
                const uint64_t count = retime_samples(Tp, S.dt);
                if (count > S.max_samples)
                {
                    res->status[p] = VMV_RETIME_TOO_LONG;
                    continue;
                }
                res->samples[p] = (uint32_t) count;
                L.sample_lo.push_back((uint32_t) L.rows), L.sampled.push_back(p), L.srecs.push_back(R);
                L.ends.push_back((uint32_t) offsets[p]), L.ends.push_back((uint32_t) (offsets[p + 1] - 1));
                L.rows += count;
                if (L.rows >= kMultiMaxConfigs)
                    return refuse_argument((std::string(call) + ": the trajectories together have 2^31 samples or more").c_str());
            }
            L.sample_lo.push_back((uint32_t) L.rows);
            return VMV_OK;
        }

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
            RetimeLayout Y;
            std::vector<uint32_t> all(n);
            for (size_t p = 0; p < n; ++p) all[p] = (uint32_t) p;
            if (int rc = retime_lay_out_paths(all, points, offsets, dim, S, S.stop_at_waypoints, 0u, "vmv_retime_multi",
                                              [](uint32_t) -> const uint8_t * { return nullptr; }, [](uint32_t, RetimePath &) {}, res, Y);
                rc != VMV_OK)
                return rc;
            const std::vector<RetimePiece> &pieces = Y.pieces;
            const std::vector<RetimePathDev> &recs = Y.recs, &srecs = Y.srecs;
            const std::vector<uint32_t> &part = Y.part, &sampled = Y.sampled, &sample_lo = Y.sample_lo;
            const uint64_t grid = Y.grid;

            int device = 0;
            VMV_LOCKSTEP_HIP(hipGetDevice(&device));  // (a call whose paths are all trivial needs a device as well)
            std::vector<float> s_times, s_pos, s_vel, s_acc;  // the sampled paths' rows, in `sampled` order
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
                if (int rc = retime_lay_out_samples(T, offsets, S, "vmv_retime_multi", res, Y); rc != VMV_OK) return rc;
                const uint64_t rows = Y.rows;
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

        // ---- vmv_retime_multi_constrained ----------------------------------------------------------------
        constexpr uint32_t kRetimeMarkWords = 64;  // one bit per piece: a path has at most kRetimeMaxGrid / 2 = 2,048
        static_assert(kRetimeMarkWords * 32u * kRetimeMinIntervals >= kRetimeMaxGrid, "a mark bit for every piece of a path");

        struct RetimeRound  // what a round says about one path
        {
            uint32_t first_fail;  // the first failing sample pair, VMV_RETIME_NONE: none fails
            uint32_t flags;       // bit 0: that pair's validity answer is 0; bit 1: some failing pair blames no blend
        };

        // Rows 0 and last of every listed path's samples become its end waypoints at rest, on the device: lane 2 a + end.
        // ends [n_paths][2]: the packed index of the path's first and last input waypoint.  A path of one sample keeps
        // its first waypoint.
        __global__ __launch_bounds__(256) void retime_ends_kernel(const uint32_t *__restrict__ sample_lo, uint32_t n_paths, uint32_t dim,
                                                                   const float *__restrict__ points, const uint32_t *__restrict__ ends,
                                                                   float *__restrict__ pos, float *__restrict__ vel)
        {
            const uint32_t g = blockIdx.x * 256u + threadIdx.x;
            if (g >= 2u * n_paths) return;
            const uint32_t a = g >> 1, end = g & 1u;
            const uint32_t lo = sample_lo[a], hi = sample_lo[a + 1u];
            if (hi == lo || (end && hi - lo == 1u)) return;
            const size_t row = (size_t) (end ? hi - 1u : lo) * dim, src = (size_t) ends[g] * dim;
            for (uint32_t j = 0; j < dim; ++j) pos[row + j] = points[src + j], vel[row + j] = 0.0f;
        }

        // One wave per listed path, lanes striding over its sample pairs.  valid: vmv_validate_motion_batch_multi's bits,
        // band: retime_band_kernel's bytes, both indexed by the packed row of the pair's first sample; either may be NULL
        // (all 1).  A failing pair (valid AND band is 0) blames the blend pieces from its first sample's piece to its
        // second's (vmv_retime_path.h).  marks [n_paths][kRetimeMarkWords]: one bit per blamed piece.  The outer trip count
        // comes from the host's sample layout and the inner one is the wave's largest range, so every lane reaches every
        // shuffle; the marks are ORed into LDS words and leave by plain stores, as the round record does by lane 0.
        __global__ __launch_bounds__(64) void retime_blame_kernel(const RetimePathDev *__restrict__ paths,
                                                                  const RetimePiece *__restrict__ pieces,
                                                                  const uint32_t *__restrict__ sample_lo, float dt,
                                                                  const float *__restrict__ gT, const uint64_t *__restrict__ valid,
                                                                  const uint8_t *__restrict__ band, RetimeRound *__restrict__ rounds,
                                                                  uint32_t *__restrict__ marks)
        {
            __shared__ uint32_t mark[kRetimeMarkWords];
            const uint32_t a = blockIdx.x, lane = threadIdx.x;
            const RetimePathDev P = paths[a];
            const uint32_t lo = sample_lo[a], count = sample_lo[a + 1u] - lo, pairs = count ? count - 1u : 0u;
            const RetimePiece *pc = pieces + P.piece_lo;
            const float *pT = gT + P.grid_lo;
            mark[lane] = 0u;
            __syncthreads();
            uint32_t best = 0xffffffffu;  // (pair << 1) | its validity answer, the smallest over the failing pairs
            bool orphan = false;
            for (uint32_t base = 0; base < pairs; base += 64u)
            {
                const uint32_t k = base + lane;
                const bool in = k < pairs;
                const uint32_t g = lo + (in ? k : 0u);
                const bool ok_v = valid == nullptr || ((valid[g >> 6] >> (g & 63u)) & 1ull) != 0ull;
                const bool ok_b = band == nullptr || band[g] != 0u;
                const bool fails = in && !(ok_v && ok_b);
                uint32_t pa = 0u, pb = 0u;
                if (fails)
                {
                    pa = retime_sample_piece(pc, P.n_pieces, pT, P.N, k, dt);
                    pb = retime_sample_piece(pc, P.n_pieces, pT, P.N, k + 1u, dt);
                }
                uint32_t range = (fails && pb >= pa) ? pb - pa + 1u : 0u, longest = range;
                for (int m = 1; m < 64; m <<= 1) longest = max(longest, (uint32_t) __shfl_xor((int) longest, m));
                bool any = false;
                for (uint32_t r = 0; r < longest; ++r)
                {
                    uint32_t piece;
                    if (r < range && retime_blame_step(pc, pa, pb, r, piece))
                    {
                        atomicOr(&mark[piece >> 5], 1u << (piece & 31u));
                        any = true;
                    }
                }
                orphan = orphan || (fails && !any);
                if (fails) best = min(best, (k << 1) | (ok_v ? 1u : 0u));
            }
            for (int m = 1; m < 64; m <<= 1) best = min(best, (uint32_t) __shfl_xor((int) best, m));
            const bool ended = __ballot(orphan) != 0ull;
            __syncthreads();
            marks[(size_t) a * kRetimeMarkWords + lane] = mark[lane];
            if (lane == 0u)
            {
                RetimeRound out;
                out.first_fail = best == 0xffffffffu ? VMV_RETIME_NONE : best >> 1;
                out.flags = (best != 0xffffffffu && (best & 1u) == 0u ? 1u : 0u) | (ended ? 2u : 0u);
                rounds[a] = out;
            }
        }

        struct RetimeConstrained  // the constrained call's own settings, resolved, and the caller's constraints (0, 1 or n)
        {
            ConstraintBand band;
            uint32_t halvings, max_rounds;
        };

        // The caller has checked every argument, n > 0, and (with envs) every environment is finalized on the current
        // device with the robot's part built.
        int retime_constrained_run(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                                   const float *vel_limits, const float *acc_limits, const RetimeHostSettings &S, const RetimeConstrained &C,
                                   vmv_trajectories *res)
        {
            const size_t dim = (size_t) res->dim;
            const RobotLaunchers &L = robot_launchers(robot);
            const ConstraintBand &band = C.band;
            const bool asks = envs != nullptr || band.count != 0;
            const uint8_t stop_level = (uint8_t) (C.halvings + 1u);
            hipStream_t stream = nullptr;
            res->n = n;
            res->status.assign(n, VMV_RETIME_COMPLETE), res->intervals.assign(n, 0), res->samples.assign(n, 0);
            res->first_invalid.assign(n, VMV_RETIME_NONE), res->duration.assign(n, 0.0f);
            res->levels.assign(offsets[n], 0), res->rounds.assign(n, 0), res->repaired.assign(n, 0), res->stops.assign(n, 0);

            int device = 0;
            VMV_LOCKSTEP_HIP(hipGetDevice(&device));
            DeviceBuffers call;  // what lives through the rounds: the waypoints, the limits, the constraints' records
            float *d_points = nullptr, *d_limits = nullptr;
            ConstraintDev *d_recs = nullptr;
            VMV_LOCKSTEP_HIP(call.alloc(&d_points, offsets[n] * dim));
            VMV_LOCKSTEP_HIP(call.alloc(&d_limits, 32));
            float limits[32] = {};
            for (size_t j = 0; j < dim; ++j) limits[j] = vel_limits[j], limits[16 + j] = acc_limits[j];
            if (offsets[n]) VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_points, points, offsets[n] * dim * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_limits, limits, sizeof(limits), hipMemcpyHostToDevice, stream));
            std::vector<ConstraintDev> cons(band.count);
            if (band.count)
            {
                constraint_band_records(band, cons.data());
                if (int rc = upload_records(call, cons.data(), band.count, &d_recs); rc != VMV_OK) return rc;
            }
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));

            // per path: the level of every distinct waypoint (its input count of bytes suffices), the samples it ended with
            std::vector<std::vector<uint8_t>> level(n);
            std::vector<std::vector<uint32_t>> kept(n);
            std::vector<std::vector<float>> o_t(n), o_p(n), o_v(n), o_a(n);
            std::vector<uint32_t> live(n);
            for (size_t p = 0; p < n; ++p)
                live[p] = (uint32_t) p, level[p].assign(offsets[p + 1] - offsets[p], S.stop_at_waypoints ? stop_level : (uint8_t) 0);

            for (uint32_t round = 1; !live.empty(); ++round)
            {
                // 1. set up, profile, sample
                RetimeLayout Y;
                if (int rc = retime_lay_out_paths(
                        live, points, offsets, dim, S, false, C.halvings, "vmv_retime_multi_constrained",
                        [&](uint32_t p) -> const uint8_t * { return level[p].data(); },
                        [&](uint32_t p, RetimePath &H) {
                            res->rounds[p] = round, res->status[p] = VMV_RETIME_COMPLETE, res->samples[p] = 0, res->duration[p] = 0.0f;
                            kept[p].swap(H.kept);
                            if (H.what == kRetimeTrivial && H.distinct)
                            {
                                o_t[p].assign(1, 0.0f), o_v[p].assign(dim, 0.0f), o_a[p].assign(dim, 0.0f);
                                o_p[p].assign(points + offsets[p] * dim, points + (offsets[p] + 1) * dim);
                            }
                        },
                        res, Y);
                    rc != VMV_OK)
                    return rc;
                const std::vector<RetimePiece> &pieces = Y.pieces;
                const std::vector<uint32_t> &corner = Y.corner, &part = Y.part, &sampled = Y.sampled, &sample_lo = Y.sample_lo, &ends = Y.ends;
                const std::vector<RetimePathDev> &recs = Y.recs, &srecs = Y.srecs;
                const uint64_t grid = Y.grid;
                live.clear();
                if (part.empty()) break;

                const size_t np = part.size();
                DeviceBuffers mem;  // the round's: a level changes the grid and the sample count either way, so no round bounds the next
                RetimePathDev *d_paths = nullptr;
                RetimePiece *d_pieces = nullptr;
                float *d_x = nullptr, *d_u = nullptr, *d_T = nullptr;
                VMV_LOCKSTEP_HIP(mem.alloc(&d_paths, np));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_pieces, pieces.size()));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_x, grid));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_u, grid));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_T, grid));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_paths, recs.data(), np * sizeof(RetimePathDev), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(RetimePiece), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemsetAsync(d_T, 0, grid * 4, stream));
                hipLaunchKernelGGL(retime_profile_kernel, dim3((uint32_t) np), dim3(64), 0, stream, d_paths, d_pieces, d_limits,
                                   (uint32_t) dim, d_x, d_u, d_T);
                VMV_LOCKSTEP_HIP(hipGetLastError());
                std::vector<float> T(grid);
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(T.data(), d_T, grid * 4, hipMemcpyDeviceToHost, stream));
                VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));

                if (int rc = retime_lay_out_samples(T, offsets, S, "vmv_retime_multi_constrained", res, Y); rc != VMV_OK) return rc;
                const uint64_t rows = Y.rows;
                if (sampled.empty()) break;

                const size_t ns = sampled.size();
                uint32_t *d_slo = nullptr, *d_ends = nullptr, *d_rec_of = nullptr, *d_marks = nullptr;
                float *d_t = nullptr, *d_p = nullptr, *d_v = nullptr, *d_a = nullptr;
                uint64_t *d_bits = nullptr;
                uint8_t *d_band = nullptr;
                RetimeRound *d_rounds = nullptr;
                VMV_LOCKSTEP_HIP(mem.alloc(&d_slo, ns + 1));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_ends, 2 * ns));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_t, rows));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_p, rows * dim));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_v, rows * dim));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_a, rows * dim));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_paths, srecs.data(), ns * sizeof(RetimePathDev), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_slo, sample_lo.data(), (ns + 1) * 4, hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_ends, ends.data(), 2 * ns * 4, hipMemcpyHostToDevice, stream));
                hipLaunchKernelGGL(retime_sample_kernel, dim3((uint32_t) ((rows + 255) / 256)), dim3(256), 0, stream, d_paths, d_pieces,
                                   d_slo, (uint32_t) ns, (uint32_t) dim, S.dt, d_x, d_u, d_T, d_t, d_p, d_v, d_a);
                VMV_LOCKSTEP_HIP(hipGetLastError());
                hipLaunchKernelGGL(retime_ends_kernel, dim3((uint32_t) ((2 * ns + 255) / 256)), dim3(256), 0, stream, d_slo, (uint32_t) ns,
                                   (uint32_t) dim, d_points, d_ends, d_p, d_v);
                VMV_LOCKSTEP_HIP(hipGetLastError());

                // 2. ask every consecutive sample pair, in place: pair g is rows g -> g + 1.  The pair behind a path's last
                // row runs into the next path; it is asked in the path's environment like the others and never looked at.
                std::vector<RetimeRound> rr(ns, RetimeRound{VMV_RETIME_NONE, 0u});
                std::vector<uint32_t> marks(ns * kRetimeMarkWords, 0u);
                uint64_t pairs = 0;
                for (size_t a = 0; a < ns; ++a) pairs += res->samples[sampled[a]] - 1u;
                if (asks && rows > 1)
                {
                    if (envs)
                    {
                        std::vector<const vmv_env *> seg_envs(ns);
                        std::vector<size_t> edge_seg(sample_lo.begin(), sample_lo.end());
                        edge_seg[ns] = rows - 1;
                        for (size_t a = 0; a < ns; ++a) seg_envs[a] = envs[sampled[a]];
                        VMV_LOCKSTEP_HIP(mem.alloc(&d_bits, (rows + 63) / 64 + 1));
                        if (int rc = vmv_validate_motion_batch_multi(robot, seg_envs.data(), edge_seg.data(), ns, d_p, d_p + dim, d_bits, stream);
                            rc != VMV_OK)
                            return rc;
                        ++res->validation_calls;
                    }
                    if (band.count)
                    {
                        VMV_LOCKSTEP_HIP(mem.alloc(&d_band, rows));
                        if (!band.P.shared)
                        {
                            VMV_LOCKSTEP_HIP(mem.alloc(&d_rec_of, ns));
                            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_rec_of, sampled.data(), ns * 4, hipMemcpyHostToDevice, stream));
                        }
                        if (int rc = L.retime_band(band.P, d_recs, d_rec_of, d_slo, (uint32_t) ns, d_p, (uint32_t) rows, d_band, stream); rc != VMV_OK)
                            return rc;
                    }
                    res->questions += pairs;

                    // 3. blame
                    VMV_LOCKSTEP_HIP(mem.alloc(&d_rounds, ns));
                    VMV_LOCKSTEP_HIP(mem.alloc(&d_marks, ns * kRetimeMarkWords));
                    hipLaunchKernelGGL(retime_blame_kernel, dim3((uint32_t) ns), dim3(64), 0, stream, d_paths, d_pieces, d_slo, S.dt, d_T,
                                       d_bits, d_band, d_rounds, d_marks);
                    VMV_LOCKSTEP_HIP(hipGetLastError());
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(rr.data(), d_rounds, ns * sizeof(RetimeRound), hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(marks.data(), d_marks, marks.size() * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
                }

                // 4. the outcome of every path; the samples of those that end come to the host, runs of neighbours together
                std::vector<uint8_t> ends_now(ns, 0);
                for (size_t a = 0; a < ns; ++a)
                {
                    const uint32_t p = sampled[a];
                    const RetimeRound &Q = rr[a];
                    if (Q.first_fail == VMV_RETIME_NONE) ends_now[a] = 1;
                    else if ((Q.flags & 2u) || round >= C.max_rounds)
                    {
                        ends_now[a] = 1;
                        res->status[p] = (Q.flags & 1u) ? VMV_RETIME_COLLISION : VMV_RETIME_OUT_OF_BAND;
                        res->first_invalid[p] = Q.first_fail;
                    }
                    else
                    {
                        const uint32_t *w = marks.data() + a * kRetimeMarkWords;
                        for (uint32_t q = 0; q < srecs[a].n_pieces; ++q)
                            if ((w[q >> 5] >> (q & 31u)) & 1u) ++level[p][corner[srecs[a].piece_lo + q]];
                        live.push_back(p);
                    }
                }
                // (each run of neighbours into its place in one host buffer per array, ONE wait for all of them, then the
                // rows go to their paths)
                std::vector<size_t> stage_at(ns + 1, 0);
                for (size_t a = 0; a < ns; ++a) stage_at[a + 1] = stage_at[a] + (ends_now[a] ? sample_lo[a + 1] - sample_lo[a] : 0u);
                const size_t staged = stage_at[ns];
                std::vector<float> t(staged), pp(staged * dim), vv(staged * dim), aa(staged * dim);
                for (size_t a = 0; a < ns;)
                {
                    if (!ends_now[a])
                    {
                        ++a;
                        continue;
                    }
                    size_t b = a;
                    while (b < ns && ends_now[b]) ++b;
                    const size_t from = sample_lo[a], count = sample_lo[b] - from, to = stage_at[a];
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(t.data() + to, d_t + from, count * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(pp.data() + to * dim, d_p + from * dim, count * dim * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(vv.data() + to * dim, d_v + from * dim, count * dim * 4, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(aa.data() + to * dim, d_a + from * dim, count * dim * 4, hipMemcpyDeviceToHost, stream));
                    a = b;
                }
                VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
                for (size_t c = 0; c < ns; ++c)
                {
                    if (!ends_now[c]) continue;
                    const uint32_t p = sampled[c];
                    const size_t at = stage_at[c], m = stage_at[c + 1] - at;
                    o_t[p].assign(t.begin() + at, t.begin() + at + m);
                    o_p[p].assign(pp.begin() + at * dim, pp.begin() + (at + m) * dim);
                    o_v[p].assign(vv.begin() + at * dim, vv.begin() + (at + m) * dim);
                    o_a[p].assign(aa.begin() + at * dim, aa.begin() + (at + m) * dim);
                }
            }

            // the packed result; the levels per input waypoint (0 for the ends and for dropped duplicates)
            size_t total = 0;
            for (size_t p = 0; p < n; ++p) total += res->samples[p];
            res->times.reserve(total), res->positions.reserve(total * dim), res->velocities.reserve(total * dim);
            res->accelerations.reserve(total * dim);
            for (size_t p = 0; p < n; ++p)
            {
                if (res->samples[p])
                {
                    res->times.insert(res->times.end(), o_t[p].begin(), o_t[p].end());
                    res->positions.insert(res->positions.end(), o_p[p].begin(), o_p[p].end());
                    res->velocities.insert(res->velocities.end(), o_v[p].begin(), o_v[p].end());
                    res->accelerations.insert(res->accelerations.end(), o_a[p].begin(), o_a[p].end());
                }
                for (size_t i = 1; i + 1 < kept[p].size(); ++i)
                {
                    const uint8_t h = level[p][i];
                    res->levels[offsets[p] + kept[p][i]] = h;
                    res->repaired[p] += h > 0 ? 1u : 0u, res->stops[p] += h == stop_level ? 1u : 0u;
                }
            }
            return VMV_OK;
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    // The checks both retiming calls make before anything is launched, in the header's order; `who` names the call in
    // the messages.  -> VMV_OK with the robot's dimension and the resolved settings, or the first failing check's code.
    static int retime_checks(const std::string &who, int robot, const vmv_env *const *envs, size_t n, const float *points,
                             const size_t *offsets, const float *vel_limits, const float *acc_limits, const vmv_retime_settings *settings,
                             const void *out, int &dim, vmv::RetimeHostSettings &H)
    {
        const auto refuse_argument = [&](const std::string &what) { return vmv::refuse_argument((who + ": " + what).c_str()); };
        dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kRetimeMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings) return refuse_argument("settings is NULL");
        if (!out) return refuse_argument("out is NULL");
        if (!vel_limits) return refuse_argument("vel_limits is NULL");
        if (!acc_limits) return refuse_argument("acc_limits is NULL");
        if (n > 0 && !offsets) return refuse_argument("offsets is NULL");
        const vmv_retime_settings &S = *settings;
        if (!std::isfinite(S.blend)) return refuse_argument("blend is not finite");
        if (!std::isfinite(S.grid_step)) return refuse_argument("grid_step is not finite");
        if (!std::isfinite(S.dt)) return refuse_argument("dt is not finite");
        if (S.grid_step > 0.0f && S.grid_step < 1e-6f) return refuse_argument("grid_step is below 1e-6");
        if (S.dt > 0.0f && S.dt < 1e-6f) return refuse_argument("dt is below 1e-6");
        if (S.max_grid > vmv::kRetimeMaxGrid) return refuse_argument("max_grid is above 4,096");
        if (S.stop_at_waypoints != 0 && S.stop_at_waypoints != 1) return refuse_argument("stop_at_waypoints is neither 0 nor 1");
        for (int j = 0; j < dim; ++j)
        {
            if (!(std::isfinite(vel_limits[j]) && vel_limits[j] > 0.0f))
                return refuse_argument("vel_limits[" + std::to_string(j) + "] is not finite and positive");
            if (!(std::isfinite(acc_limits[j]) && acc_limits[j] > 0.0f))
                return refuse_argument("acc_limits[" + std::to_string(j) + "] is not finite and positive");
        }
        if (n >= vmv::kMultiMaxConfigs) return refuse_argument("n is 2^31 or more");
        if (n > 0 && offsets[0] != 0) return refuse_argument("offsets[0] is not 0");
        for (size_t k = 0; k < n; ++k)
            if (offsets[k + 1] < offsets[k]) return refuse_argument("offsets decrease at " + std::to_string(k + 1));
        if (n > 0 && offsets[n] >= vmv::kMultiMaxConfigs) return refuse_argument("2^31 waypoints or more");
        if (n > 0 && offsets[n] > 0 && !points) return refuse_argument("points is NULL");
        if (int rc = vmv::check_env_kinds(robot, envs, n, false); rc != VMV_OK) return rc;
        const auto or_default = [](float v, float d) { return v > 0.0f ? v : d; };
        H = vmv::RetimeHostSettings{(double) or_default(S.blend, 0.1f), (double) or_default(S.grid_step, 0.02f), or_default(S.dt, 0.01f),
                                    S.max_grid ? S.max_grid : vmv::kRetimeMaxGrid, S.max_samples ? S.max_samples : 65536u,
                                    S.stop_at_waypoints != 0};
        return VMV_OK;
    }

    int vmv_retime_multi(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                         const float *vel_limits, const float *acc_limits, const vmv_retime_settings *settings, vmv_trajectories **out)
    {
        int dim = 0;
        vmv::RetimeHostSettings H;
        if (int rc = retime_checks("vmv_retime_multi", robot, envs, n, points, offsets, vel_limits, acc_limits, settings, out, dim, H); rc != VMV_OK)
            return rc;
        return vmv::lockstep_call(robot, envs, n, dim, out, [&](vmv_trajectories *result) {
            return vmv::retime_multi_run(robot, envs, n, points, offsets, vel_limits, acc_limits, H, result);
        });
    }

    int vmv_retime_multi_constrained(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                                     const float *vel_limits, const float *acc_limits, const vmv_ee_constraint *constraints,
                                     size_t n_constraints, const vmv_retime_constrained_settings *settings,
                                     const vmv_constraint_settings *constraint_settings, vmv_trajectories **out)
    {
        // vmv_retime_multi's checks in its order, then this call's own, then the constraint's in vmv_constraint_project_batch's
        // order; none needs a device
        const std::string who = "vmv_retime_multi_constrained";
        const auto refuse_argument = [&](const std::string &what) { return vmv::refuse_argument((who + ": " + what).c_str()); };
        int dim = 0;
        vmv::RetimeHostSettings H;
        if (int rc = retime_checks(who, robot, envs, n, points, offsets, vel_limits, acc_limits, settings ? &settings->base : nullptr, out, dim, H);
            rc != VMV_OK)
            return rc;
        if (settings->blend_halvings > vmv::kRetimeMaxHalvings) return refuse_argument("blend_halvings is above 8");
        vmv::RetimeConstrained C{};
        C.halvings = settings->blend_halvings ? settings->blend_halvings : 3u;
        C.max_rounds = settings->max_rounds ? settings->max_rounds : 8u;
        if (n_constraints != 0 && n_constraints != 1 && n_constraints != n) return refuse_argument("n_constraints is neither 0, 1 nor n");
        if (n_constraints)  // (this call's words for the pointers and the count, the band's for the rest)
        {
            if (!constraints) return refuse_argument("constraints is NULL");
            if (!constraint_settings) return refuse_argument("constraint_settings is NULL");
            const std::string err = vmv::constraint_band_resolve(constraints, n_constraints, *constraint_settings, nullptr, C.band);
            if (!err.empty()) return refuse_argument(err);
            float lower[16], span[16], descale[16];
            if (int rb = vmv_robot_bounds(robot, lower, span, descale); rb != VMV_OK) return rb;
            vmv::constraint_band_bounds(C.band, lower, span, dim);
        }
        const int rc = vmv::lockstep_call(robot, envs, n, dim, out, [&](vmv_trajectories *result) {
            return vmv::retime_constrained_run(robot, envs, n, points, offsets, vel_limits, acc_limits, H, C, result);
        });
        if (rc == VMV_OK) (*out)->levelled = true;
        return rc;
    }

    // NOT part of the supported interface and not in the public header: retime_band_kernel on its own, for the test that
    // compares its answers with vmv_constraint_check_motion_batch.  The band answers of the consecutive pairs of n_paths
    // packed sample lists, list a = positions rows [sample_offsets[a], sample_offsets[a + 1]) under constraint 0
    // (n_constraints 1) or a.  ok: one byte per ROW, 1 in a list's last row.  Synchronous, host buffers.
    int vmv_retime_band_pairs_host(int robot, const float *positions, const size_t *sample_offsets, size_t n_paths,
                                   const vmv_ee_constraint *constraints, size_t n_constraints, const vmv_constraint_settings *settings,
                                   uint8_t *ok)
    {
        using vmv::hip_status;
        const auto refuse_argument = [](const std::string &what) { return vmv::refuse_argument(("vmv_retime_band_pairs_host: " + what).c_str()); };
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0) return VMV_ERR_UNKNOWN_ROBOT;
        if (!positions || !sample_offsets || !constraints || !settings || !ok) return refuse_argument("null pointer");
        if (n_paths == 0 || n_paths >= vmv::kMultiMaxConfigs) return refuse_argument("n_paths must be 1 .. 2^31 - 1");
        if (n_constraints != 1 && n_constraints != n_paths) return refuse_argument("n_constraints must be 1 or n_paths");
        if (sample_offsets[0] != 0) return refuse_argument("sample_offsets[0] is not 0");
        for (size_t a = 0; a < n_paths; ++a)
            if (sample_offsets[a + 1] <= sample_offsets[a]) return refuse_argument("every list needs a row");
        const size_t rows = sample_offsets[n_paths];
        if (rows >= vmv::kMultiMaxConfigs) return refuse_argument("2^31 rows or more");
        vmv::ConstraintBand band{};  // (the band kernel reads no joint bounds: they stay 0)
        const std::string err = vmv::constraint_band_resolve(constraints, n_constraints, *settings, nullptr, band);
        if (!err.empty()) return refuse_argument(err);
        const vmv::ConstraintParams &P = band.P;
        std::vector<vmv::ConstraintDev> cons(n_constraints);
        vmv::constraint_band_records(band, cons.data());
        std::vector<uint32_t> slo(n_paths + 1), rec_of(n_paths);
        for (size_t a = 0; a <= n_paths; ++a) slo[a] = (uint32_t) sample_offsets[a];
        for (size_t a = 0; a < n_paths; ++a) rec_of[a] = (uint32_t) a;
        int device = 0;
        VMV_LOCKSTEP_HIP(hipGetDevice(&device));
        vmv::DeviceBuffers mem;
        vmv::ConstraintDev *d_recs = nullptr;
        uint32_t *d_slo = nullptr, *d_rec_of = nullptr;
        float *d_p = nullptr;
        uint8_t *d_ok = nullptr;
        if (int rc = vmv::upload_records(mem, cons.data(), n_constraints, &d_recs); rc != VMV_OK) return rc;
        VMV_LOCKSTEP_HIP(mem.alloc(&d_slo, n_paths + 1));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_rec_of, n_paths));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_p, rows * (size_t) dim));
        VMV_LOCKSTEP_HIP(mem.alloc(&d_ok, rows));
        VMV_LOCKSTEP_HIP(hipMemcpy(d_slo, slo.data(), (n_paths + 1) * 4, hipMemcpyHostToDevice));
        VMV_LOCKSTEP_HIP(hipMemcpy(d_rec_of, rec_of.data(), n_paths * 4, hipMemcpyHostToDevice));
        VMV_LOCKSTEP_HIP(hipMemcpy(d_p, positions, rows * (size_t) dim * 4, hipMemcpyHostToDevice));
        if (int rc = vmv::robot_launchers(robot).retime_band(P, d_recs, d_rec_of, d_slo, (uint32_t) n_paths, d_p, (uint32_t) rows, d_ok, nullptr);
            rc != VMV_OK)
            return rc;
        VMV_LOCKSTEP_HIP(hipMemcpy(ok, d_ok, rows, hipMemcpyDeviceToHost));
        return VMV_OK;
    }

    int vmv_retime_levels(const vmv_trajectories *result, uint8_t *levels, uint32_t *rounds, uint32_t *repaired, uint32_t *stops)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        if (!result->levelled) return vmv::refuse_argument("vmv_retime_levels: the result is not vmv_retime_multi_constrained's");
        const size_t n = result->n;
        if (levels && !result->levels.empty()) std::memcpy(levels, result->levels.data(), result->levels.size());
        if (rounds && n) std::memcpy(rounds, result->rounds.data(), n * 4);
        if (repaired && n) std::memcpy(repaired, result->repaired.data(), n * 4);
        if (stops && n) std::memcpy(stops, result->stops.data(), n * 4);
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
