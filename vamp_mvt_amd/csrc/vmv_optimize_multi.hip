// vmv_optimize_multi.hip — clearance-aware path optimisation over many independent paths (vmv_optimize_multi).
//
// A covariant gradient iteration (CHOMP's update without its velocity-projection terms) on the waypoints of every path, in
// lockstep: per iteration ONE vmv_clearance_grad_batch_multi call answers the two clearances and their gradients at the
// waypoints of all unfinished paths, opt_step_kernel (one workgroup per unfinished path) turns them into the cost of the
// iterate, the gradient, the tridiagonal solve, the capped and clipped update and the next iterate.  Every validate_every
// iterations the iterate's consecutive edges go through ONE vmv_validate_motion_batch_multi call and opt_accept_kernel (one
// wave per unfinished path) keeps the cheapest valid iterate and decides whether the path ends.  The host looks at the
// finished flags only there.  The contract, with every operation's order, is in include/vamp_mvt_amd.h.
//
// Decisions:
//  * The gradient / the step of a path live in LDS (free waypoints x dim floats, plus one float per waypoint for the cost
//    terms; dynamic, sized by the call's longest path).  The solve is a dependent chain per joint column whose loads the
//    compiler does not hoist far: LDS latency instead of L2 latency per link.  At the densified lengths the flow produces
//    (<= 130 waypoints x 7 joints: 4 KiB) LDS does not limit occupancy; at the cap (1,024 x 16: 68 KiB) two workgroups fit
//    a CU's 160 KiB, 512 on the chip, which is accepted for a call of 1,300 such paths.
//  * The step kernel writes the edges of the next validated iterate (it holds the new waypoints), the accept kernel only
//    reads answers.  The waypoints are double-buffered so that the accept kernel, which runs after the step kernel of the
//    same iteration, still finds the validated iterate.
//  * The active paths' waypoints are also kept packed (q), which is what the clearance call reads; the step kernel writes
//    both copies, opt_pack_kernel rebuilds the packed copy after the host compacted the active list.
// Every store is a plain vector store by the owning workgroup; the only atomics are on LDS words (order-independent
// minima / maxima of integer keys).  Every loop is bounded by a waypoint count the host checked against max_waypoints.
//
// vmv_optimize_multi_constrained (include/vamp_mvt_amd.h states the contract in full) runs the same iteration
// inside the band of an end-effector constraint.  The input's ends are band-tested and its inner waypoints projected
// before the first iteration; per iteration the robot's opt_band_kernel (vmv_robot_tu.inc), one lane per packed waypoint,
// follows the step kernel and replaces every inner waypoint of the new iterate by its projection, or by its value in the
// current iterate where the projection does not converge; at validated iterates ONE launch of the edge band test runs
// next to the validation call and opt_accept_kernel<true> ANDs its answers into the edge test.  The step kernel is the
// same for both calls: the cost of an iterate is computed from x[cur], which the band kernel has already written.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_lockstep.h"

#include <cmath>
#include <cstring>

struct vmv_optimized
{
    size_t n = 0;
    int dim = 0;
    std::vector<uint8_t> status;
    std::vector<uint32_t> iterations, best_iteration;
    std::vector<float> cost_first, cost, clearance_first, clearance;  // clearances: [n][2] = env, self
    std::vector<float> points;                                        // packed in path order, the input's layout
    uint64_t clearance_calls = 0, validation_calls = 0;
    bool constrained = false;    // made by vmv_optimize_multi_constrained
    std::vector<uint32_t> held;  // [n] its projections that did not converge
};

namespace vmv
{
    namespace
    {
        constexpr uint32_t kOptBlock = 256;
        constexpr uint32_t kOptAcceptBlock = kWave;
        constexpr uint32_t kOptDefaultIterations = 64;
        constexpr uint32_t kOptDefaultWaypoints = 1024;
        constexpr uint32_t kOptMaxWaypoints = 1024;
        constexpr uint32_t kKeyInf = 0xff800000u;  // order_key(+inf)

        struct OptParams
        {
            uint32_t dim, max_iterations;
            float step, max_step, min_change, w_smooth, w_env, w_self, eps_env, eps_self;
            float lower[kPlanMaxDim], upper[kPlanMaxDim];
        };

        struct OptState  // per path
        {
            uint32_t status, iterations, best_iteration, has_best;
            float u_first, u_best, u_cur;
            float env_first, self_first, env_best, self_best, env_cur, self_cur;
            float change_in, change_out;  // |scaled step|_inf of the step into the current iterate / out of it
            uint32_t pad;
        };
        static_assert(sizeof(OptState) == 64, "one cache line half per path");

        struct OptArrays
        {
            OptState *state;           // [n_paths]
            float *x;                  // [2][total][dim] the iterates in the input's layout, double-buffered
            float *best;               // [total][dim]
            const uint64_t *offsets;   // [n_paths + 1] in waypoints
            const uint32_t *active;    // [n_active] path of each workgroup
            const uint64_t *act_off;   // [n_active] first waypoint of the path in q / clr / grad
            const uint64_t *edge_off;  // [n_active] first edge of the path in e_start / e_goal / bits
            float *q;                  // [active waypoints][dim] the iterate the clearance call reads
            const float *clr;          // [active waypoints][2]
            const float *grad;         // [active waypoints][2][dim]
            float *e_start, *e_goal;   // [edges][dim]
            const uint64_t *bits;      // answers of the validated iterate
            const uint8_t *band_ok;    // [edges] vmv_optimize_multi_constrained: the band's answers (NULL otherwise, never read)
            const float *recip;        // [longest - 2] reciprocals of the solve's pivots
            uint8_t *done;             // [n_paths]
            size_t total;              // waypoints of the call
        };

        // a total order on floats as unsigned integers (-0 below +0), so that a minimum does not depend on the order it
        // is taken in; NaN never enters
        __device__ __forceinline__ uint32_t order_key(float v)
        {
            const uint32_t b = __float_as_uint(v);
            return (b >> 31) ? ~b : (b | 0x80000000u);
        }
        __device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

        // CHOMP's hinge and its derivative; +inf and NaN give 0
        __device__ __forceinline__ float hinge(float v, float eps)
        {
            if (v < 0.f) return (0.f - v) + 0.5f * eps;
            if (v <= eps)
            {
                const float d = v - eps;
                return (d * d) / (2.0f * eps);
            }
            return 0.f;
        }
        __device__ __forceinline__ float hinge_slope(float v, float eps)
        {
            if (v < 0.f) return -1.0f;
            if (v <= eps) return (v - eps) / eps;
            return 0.f;
        }

        // One workgroup per active path: iterate k in x[cur] -> its cost and clearance minima, and (update) iterate k + 1
        // in x[cur ^ 1] and q, with its edges if `edges`.
        __global__ __launch_bounds__(kOptBlock) void opt_step_kernel(const OptParams P, const OptArrays D, const uint32_t cur,
                                                                     const uint32_t k, const uint32_t update, const uint32_t edges)
        {
            extern __shared__ float s_mem[];
            __shared__ uint32_t s_key[3];  // min key of env, of self; max bits of |step|
            __shared__ float s_u;
            const uint32_t a = blockIdx.x, p = D.active[a], lane = threadIdx.x, dim = P.dim;
            if (D.done[p]) return;  // (the host removes a finished path before the next launch; whole workgroup alike)
            const uint64_t lo = D.offsets[p];
            const uint32_t N = (uint32_t) (D.offsets[p + 1] - lo), n = N - 2u;  // N >= 3 for an active path
            const float *x = D.x + ((size_t) cur * D.total + lo) * dim;
            float *xn = D.x + ((size_t) (cur ^ 1u) * D.total + lo) * dim;
            const uint64_t ao = D.act_off[a];
            const float *clr = D.clr + ao * 2u;
            const float *grad = D.grad + ao * 2u * dim;
            float *g = s_mem;                    // [n][dim]
            float *t = s_mem + (size_t) n * dim;  // [N - 1] cost terms

            if (lane < 3) s_key[lane] = lane < 2 ? kKeyInf : 0u;
            __syncthreads();

            // phase 1: cost terms and clearance minima per waypoint, the gradient per (free waypoint, joint)
            uint32_t ke = kKeyInf, ks = kKeyInf;
            for (uint32_t i = lane; i < N; i += kOptBlock)
            {
                const float env = clr[2u * i], self = clr[2u * i + 1u];
                if (env == env) ke = min(ke, order_key(env));
                if (self == self) ks = min(ks, order_key(self));
                if (i + 1u < N)
                {
                    float s = 0.f;
                    for (uint32_t j = 0; j < dim; ++j)
                    {
                        const float d = x[(size_t) (i + 1u) * dim + j] - x[(size_t) i * dim + j];
                        s = s + d * d;
                    }
                    const float sm = P.w_smooth * (0.5f * s);
                    const float ob = i >= 1u ? P.w_env * hinge(env, P.eps_env) + P.w_self * hinge(self, P.eps_self) : 0.f;
                    t[i] = sm + ob;
                }
            }
            atomicMin(&s_key[0], ke);
            atomicMin(&s_key[1], ks);
            if (update)
                for (uint32_t e = lane; e < n * dim; e += kOptBlock)
                {
                    const uint32_t i = e / dim + 1u, j = e - (i - 1u) * dim;
                    const float xi = x[(size_t) i * dim + j];
                    const float sm = ((2.0f * xi) - x[(size_t) (i - 1u) * dim + j]) - x[(size_t) (i + 1u) * dim + j];
                    const float de = P.w_env * hinge_slope(clr[2u * i], P.eps_env);
                    const float ds = P.w_self * hinge_slope(clr[2u * i + 1u], P.eps_self);
                    float v = P.w_smooth * sm;
                    v = v + de * grad[((size_t) i * 2u) * dim + j];
                    v = v + ds * grad[((size_t) i * 2u + 1u) * dim + j];
                    g[e] = v;
                }
            __syncthreads();

            // phase 2: the solve along i, one lane per joint column (lanes of wave 0), and the cost's ordered sum (one lane
            // of wave 1), side by side
            if (update && lane < dim)
            {
                const float *__restrict__ r = D.recip;
                float prev = g[lane];
                for (uint32_t i = 1; i < n; ++i)
                {
                    prev = g[(size_t) i * dim + lane] + r[i - 1u] * prev;
                    g[(size_t) i * dim + lane] = prev;
                }
                float z = prev * r[n - 1u];
                g[(size_t) (n - 1u) * dim + lane] = z;
                for (uint32_t i = n - 1u; i-- > 0u;)
                {
                    z = (g[(size_t) i * dim + lane] + z) * r[i];
                    g[(size_t) i * dim + lane] = z;
                }
            }
            if (lane == kWave)
            {
                float u = 0.f;
                for (uint32_t i = 0; i + 1u < N; ++i) u = u + t[i];
                s_u = u;
            }
            __syncthreads();

            // phase 3: the step, its path-wide norm, the scale, the clipped update
            float change = 0.f;
            if (update)
            {
                const float neg = 0.f - P.step;
                uint32_t km = 0u;
                for (uint32_t e = lane; e < n * dim; e += kOptBlock)
                {
                    const float d = neg * g[e];
                    g[e] = d;  // (element e is this lane's alone)
                    const float ad = fabsf(d);
                    if (ad == ad) km = max(km, __float_as_uint(ad));
                }
                atomicMax(&s_key[2], km);
                __syncthreads();
                const float m = __uint_as_float(s_key[2]);
                const float scale = P.max_step / (m > P.max_step ? m : P.max_step);
                change = m * scale;
                float *q = D.q + ao * dim;
                const uint64_t eo = D.edge_off[a];
                float *es = D.e_start + eo * dim, *eg = D.e_goal + eo * dim;
                for (uint32_t e = lane; e < N * dim; e += kOptBlock)
                {
                    const uint32_t i = e / dim, j = e - i * dim;
                    float v = x[e];
                    if (i >= 1u && i + 1u < N)
                    {
                        v = v + g[e - dim] * scale;
                        v = v < P.lower[j] ? P.lower[j] : (v > P.upper[j] ? P.upper[j] : v);  // (NaN stays NaN)
                    }
                    xn[e] = v;
                    q[e] = v;
                    if (edges)
                    {
                        if (i + 1u < N) es[e] = v;
                        if (i >= 1u) eg[e - dim] = v;
                    }
                }
            }
            if (lane == 0)
            {
                OptState st = D.state[p];
                st.u_cur = s_u, st.env_cur = key_value(s_key[0]), st.self_cur = key_value(s_key[1]);
                if (k == 0) st.u_first = st.u_cur, st.env_first = st.env_cur, st.self_first = st.self_cur;
                st.change_in = st.change_out, st.change_out = change;
                D.state[p] = st;
            }
        }

        // One wave per active path, after the step kernel of validated iterate k (in x[cur]) and its validation.
        // Constrained: an edge counts where the band's answer is 1 as well.
        template <bool Constrained>
        __global__ __launch_bounds__(kOptAcceptBlock) void opt_accept_kernel(const OptParams P, const OptArrays D, const uint32_t cur,
                                                                             const uint32_t k)
        {
            const uint32_t a = blockIdx.x, p = D.active[a], lane = threadIdx.x, dim = P.dim;
            if (D.done[p]) return;
            const uint64_t lo = D.offsets[p], eo = D.edge_off[a];
            const uint32_t N = (uint32_t) (D.offsets[p + 1] - lo);
            bool ok = true;
            for (uint32_t e = lane; e + 1u < N; e += kOptAcceptBlock)
            {
                const uint64_t b = eo + e;
                ok = ok && ((D.bits[b >> 6] >> (b & 63u)) & 1ull);
                if constexpr (Constrained) ok = ok && D.band_ok[b] != 0u;
            }
            const bool valid = __ballot(!ok) == 0ull;
            OptState st = D.state[p];
            const bool better = valid && (!st.has_best || st.u_cur < st.u_best);  // the first of equal costs stays
            if (better)
            {
                const float *x = D.x + ((size_t) cur * D.total + lo) * dim;
                float *b = D.best + lo * dim;
                for (uint32_t e = dim + lane; e < (N - 1u) * dim; e += kOptAcceptBlock) b[e] = x[e];  // (the ends never move)
            }
            if (lane == 0)
            {
                if (better)
                    st.has_best = 1u, st.best_iteration = k, st.u_best = st.u_cur, st.env_best = st.env_cur, st.self_best = st.self_cur;
                st.iterations = k;
                st.status = st.has_best ? VMV_OPT_OK : VMV_OPT_NO_VALID;
                D.state[p] = st;
                if (k >= P.max_iterations || (k > 0u && st.change_in < P.min_change)) D.done[p] = 1;
            }
        }

        // the packed copy of the active paths' current iterate (x[cur]) and, with `edges`, its edges
        __global__ __launch_bounds__(kOptBlock) void opt_pack_kernel(const OptParams P, const OptArrays D, const uint32_t cur,
                                                                     const uint32_t edges)
        {
            const uint32_t a = blockIdx.x, p = D.active[a], lane = threadIdx.x, dim = P.dim;
            const uint64_t lo = D.offsets[p], eo = D.edge_off[a];
            const uint32_t N = (uint32_t) (D.offsets[p + 1] - lo);
            const float *x = D.x + ((size_t) cur * D.total + lo) * dim;
            float *q = D.q + D.act_off[a] * dim, *es = D.e_start + eo * dim, *eg = D.e_goal + eo * dim;
            for (uint32_t e = lane; e < N * dim; e += kOptBlock)
            {
                const uint32_t i = e / dim;
                const float v = x[e];
                q[e] = v;
                if (edges)
                {
                    if (i + 1u < N) es[e] = v;
                    if (i >= 1u) eg[e - dim] = v;
                }
            }
        }

        int launched(hipError_t e, const char *what)
        {
            if (e == hipSuccess) return VMV_OK;
            (void) hipDeviceSynchronize();
            return hip_status(e, what);
        }

        // row -> active index of the packed waypoints of `active` (OptBand::row_path)
        std::vector<uint32_t> rows_of(const std::vector<uint32_t> &active, const size_t *offsets)
        {
            std::vector<uint32_t> rows;
            for (size_t a = 0; a < active.size(); ++a) rows.insert(rows.end(), offsets[active[a] + 1] - offsets[active[a]], (uint32_t) a);
            return rows;
        }

        // The constrained call's look at its input, before the iterations.  ONE band test over both ends of every path in
        // `finite` (finite paths of 2 waypoints and more), each with its path's record; then ONE launch of the band kernel
        // in its initial mode over the waypoints of the paths of 3 and more whose ends passed, which projects their inner
        // waypoints in place.  out_of_band[p] = 1: an end out of band or a projection that did not converge.  x0: the
        // input with the inner waypoints of the other paths projected (iterate 0).  d_recs: one record (shared) or one per path.
        int optimize_band_input(int robot, const ConstraintBand &cb, const ConstraintDev *d_recs, const std::vector<ConstraintDev> &recs,
                                const std::vector<uint32_t> &finite, size_t n, const float *points, const size_t *offsets,
                                const std::vector<uint64_t> &offsets64, size_t dim, hipStream_t stream, std::vector<uint8_t> &out_of_band,
                                std::vector<float> &x0)
        {
            const RobotLaunchers &L = robot_launchers(robot);
            const size_t total = offsets[n], m = finite.size();
            out_of_band.assign(n, 0);
            x0.assign(points, points + total * dim);
            if (m == 0) return VMV_OK;

            DeviceBuffers tmp;  // what only this look needs
            std::vector<float> ends(2 * m * dim);
            for (size_t s = 0; s < m; ++s)
            {
                std::memcpy(&ends[2 * s * dim], points + offsets[finite[s]] * dim, dim * 4);
                std::memcpy(&ends[(2 * s + 1) * dim], points + (offsets[finite[s] + 1] - 1) * dim, dim * 4);
            }
            float *d_ends = nullptr;
            uint64_t *d_bits = nullptr;
            const ConstraintDev *d_end_recs = d_recs;
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_ends, ends.size()));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_bits, (2 * m + 63) / 64));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_ends, ends.data(), ends.size() * 4, hipMemcpyHostToDevice, stream));
            if (!cb.P.shared)
            {
                std::vector<uint32_t> owner(2 * m);
                for (size_t s = 0; s < m; ++s) owner[2 * s] = owner[2 * s + 1] = finite[s];
                ConstraintDev *d = nullptr;
                if (int rc = upload_records(tmp, constraint_band_expand(recs.data(), owner).data(), 2 * m, &d); rc != VMV_OK) return rc;
                d_end_recs = d;
            }
            if (int rc = L.constraint_check(cb.P, d_end_recs, d_ends, 2 * m, d_bits, nullptr, stream); rc != VMV_OK) return rc;
            std::vector<uint64_t> bits((2 * m + 63) / 64);
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(bits.data(), d_bits, bits.size() * 8, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
            std::vector<uint32_t> inner;  // the paths whose inner waypoints are projected
            for (size_t s = 0; s < m; ++s)
            {
                const uint32_t p = finite[s];
                if (((bits[s >> 5] >> (2 * (s & 31u))) & 3ull) != 3ull)
                    out_of_band[p] = 1;
                else if (offsets[p + 1] - offsets[p] > 2)
                    inner.push_back(p);
            }
            if (inner.empty()) return VMV_OK;

            const std::vector<uint32_t> rows = rows_of(inner, offsets);
            std::vector<uint64_t> act_off(inner.size());
            for (size_t a = 0, at = 0; a < inner.size(); ++a) act_off[a] = at, at += offsets[inner[a] + 1] - offsets[inner[a]];
            OptBand B{};
            uint32_t *d_rows = nullptr, *d_active = nullptr;
            uint64_t *d_act_off = nullptr, *d_offsets = nullptr;
            float *d_scratch = nullptr;  // the packed copy and the edges of this launch, which nobody reads
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_rows, rows.size()));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_active, inner.size()));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_act_off, inner.size()));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_offsets, n + 1));
            VMV_LOCKSTEP_HIP(tmp.alloc(&B.x, total * dim));
            VMV_LOCKSTEP_HIP(tmp.alloc(&d_scratch, rows.size() * dim));
            VMV_LOCKSTEP_HIP(tmp.alloc(&B.unconverged, n));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(B.unconverged, 0, std::max<size_t>(n, 16), stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(B.x, points, total * dim * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_active, inner.data(), inner.size() * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_act_off, act_off.data(), inner.size() * 8, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_offsets, offsets64.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
            B.row_path = d_rows, B.active = d_active, B.act_off = d_act_off, B.edge_off = d_act_off, B.offsets = d_offsets;
            B.q = d_scratch, B.e_start = d_scratch, B.e_goal = d_scratch, B.change_in = B.x, B.state_stride = 0, B.held = nullptr;
            B.total = total;
            if (int rc = L.opt_band(cb.P, d_recs, B, (uint32_t) rows.size(), 0u, 1u, 0u, 0u, 0.f, stream); rc != VMV_OK) return rc;
            std::vector<uint8_t> unconverged(n);
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(x0.data(), B.x, total * dim * 4, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(unconverged.data(), B.unconverged, n, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
            for (const uint32_t p : inner) out_of_band[p] = unconverged[p];
            return VMV_OK;
        }

        // The caller has checked every argument, n > 0, and every environment is finalized on the current device with the
        // robot's part built.
        // cb: vmv_optimize_multi_constrained's constraints and resolved settings (NULL: vmv_optimize_multi).
        int optimize_multi_run(int robot, const vmv_env *const *envs, size_t n, const float *points, const size_t *offsets,
                               const OptParams &P, uint32_t validate_every, vmv_optimized *res, const ConstraintBand *cb = nullptr)
        {
            const size_t dim = P.dim, total = offsets[n];
            hipStream_t stream = nullptr;

            res->n = n;
            res->status.assign(n, VMV_OPT_OK), res->iterations.assign(n, 0), res->best_iteration.assign(n, 0);
            res->cost_first.assign(n, 0.f), res->cost.assign(n, 0.f);
            res->clearance_first.assign(2 * n, std::nanf("")), res->clearance.assign(2 * n, std::nanf(""));
            res->points.assign(points, points + total * dim);

            // who takes part: paths of 3 and more finite waypoints iterate; a finite path of 2 asks its one edge
            std::vector<uint32_t> active, two;
            std::vector<const vmv_env *> active_envs;
            std::vector<uint64_t> offsets64(n + 1);
            size_t longest = 0;
            for (size_t k = 0; k < n; ++k)
            {
                const size_t len = offsets[k + 1] - offsets[k];
                offsets64[k] = offsets[k];
                bool finite = true;
                for (size_t e = offsets[k] * dim; e < offsets[k + 1] * dim && finite; ++e) finite = std::isfinite(points[e]);
                if (!finite)
                    res->status[k] = VMV_OPT_NONFINITE;
                else if (len == 2)
                    two.push_back((uint32_t) k);
                else if (len > 2)
                    active.push_back((uint32_t) k), active_envs.push_back(envs[k]), longest = std::max(longest, len);
            }
            offsets64[n] = total;

            // the constrained call's look at the input: the paths out of band leave, the others start from iterate 0
            DeviceBuffers mem;
            ConstraintDev *d_recs = nullptr;
            std::vector<ConstraintDev> recs;
            std::vector<float> x0;
            if (cb)
            {
                res->held.assign(n, 0);
                recs.resize(cb->count);
                constraint_band_records(*cb, recs.data());
                if (int rc = upload_records(mem, recs.data(), cb->count, &d_recs); rc != VMV_OK) return rc;
                std::vector<uint32_t> finite(two);
                finite.insert(finite.end(), active.begin(), active.end());
                std::vector<uint8_t> out_of_band;
                if (int rc = optimize_band_input(robot, *cb, d_recs, recs, finite, n, points, offsets, offsets64, dim, stream, out_of_band, x0);
                    rc != VMV_OK)
                    return rc;
                const auto stays = [&](std::vector<uint32_t> &list) {
                    size_t kept = 0;
                    for (const uint32_t p : list)
                        if (out_of_band[p])
                            res->status[p] = VMV_OPT_OUT_OF_BAND;
                        else
                            list[kept++] = p;
                    list.resize(kept);
                };
                stays(two), stays(active);
                active_envs.clear(), longest = 0;
                for (const uint32_t p : active) active_envs.push_back(envs[p]), longest = std::max(longest, offsets[p + 1] - offsets[p]);
            }
            const float *first = cb ? x0.data() : points;  // iterate 0
            const size_t na0 = active.size();
            if (na0 == 0 && two.empty()) return VMV_OK;

            // the active list's offsets: waypoints (q, clr, grad) and edges; the 2-waypoint paths' edges follow the
            // active paths' in the first validation only
            std::vector<size_t> wp_seg(na0 + 1, 0), edge_seg(na0 + two.size() + 1, 0);
            std::vector<uint64_t> act_off(std::max<size_t>(na0, 1)), edge_off(std::max<size_t>(na0, 1));
            std::vector<const vmv_env *> edge_envs(active_envs);
            const auto lay_out = [&]() {
                for (size_t a = 0; a < active.size(); ++a)
                {
                    const size_t len = offsets[active[a] + 1] - offsets[active[a]];
                    act_off[a] = wp_seg[a], edge_off[a] = edge_seg[a];
                    wp_seg[a + 1] = wp_seg[a] + len, edge_seg[a + 1] = edge_seg[a] + len - 1;
                }
            };
            lay_out();
            const size_t act_total = wp_seg[na0], act_edges = edge_seg[na0], all_edges = act_edges + two.size();
            for (size_t s = 0; s < two.size(); ++s) edge_seg[na0 + s + 1] = act_edges + s + 1, edge_envs.push_back(envs[two[s]]);

            std::vector<float> recip(longest > 2 ? longest - 2 : 1);
            {
                float r = 0.5f;  // pivot 0 is 2
                recip[0] = r;
                for (size_t i = 1; i < recip.size(); ++i) r = 1.0f / (2.0f - r), recip[i] = r;
            }
            const size_t lds = ((longest > 2 ? longest - 2 : 0) * dim + longest) * sizeof(float);
            if (lds > 32u * 1024u)
                VMV_LOCKSTEP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(opt_step_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));

            OptArrays D{};
            uint64_t *d_offsets = nullptr, *d_act_off = nullptr, *d_edge_off = nullptr, *d_bits = nullptr;
            uint32_t *d_active = nullptr;
            float *d_clr = nullptr, *d_grad = nullptr, *d_recip = nullptr;
            const size_t words = (all_edges + 63) / 64 + 1;
            // the constrained call's own: the band's answer per edge, the row -> active-path index of the band kernel, the
            // counts of held waypoints and, with one record per path, the record of every edge for the edge band test
            uint8_t *d_band_ok = nullptr;
            uint32_t *d_rows = nullptr, *d_held = nullptr;
            ConstraintDev *d_edge_recs = nullptr;
            if (cb)
            {
                VMV_LOCKSTEP_HIP(mem.alloc(&d_band_ok, all_edges));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_rows, act_total));
                VMV_LOCKSTEP_HIP(mem.alloc(&d_held, n));
                VMV_LOCKSTEP_HIP(hipMemsetAsync(d_held, 0, std::max<size_t>(n * 4, 16), stream));
                if (!cb->P.shared) VMV_LOCKSTEP_HIP(mem.alloc(&d_edge_recs, all_edges));
            }
            VMV_LOCKSTEP_HIP(mem.alloc(&D.state, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.x, 2 * total * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.best, total * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_offsets, n + 1));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_active, std::max<size_t>(na0, 1)));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_act_off, std::max<size_t>(na0, 1)));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_edge_off, std::max<size_t>(na0, 1)));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.q, act_total * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_clr, act_total * 2));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_grad, act_total * 2 * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.e_start, all_edges * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.e_goal, all_edges * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_bits, words));
            VMV_LOCKSTEP_HIP(mem.alloc(&d_recip, recip.size()));
            VMV_LOCKSTEP_HIP(mem.alloc(&D.done, n));
            VMV_LOCKSTEP_HIP(hipHostMalloc(&mem.pinned, std::max<size_t>(n, 16), hipHostMallocDefault));
            uint8_t *h_done = static_cast<uint8_t *>(mem.pinned);
            D.offsets = d_offsets, D.active = d_active, D.act_off = d_act_off, D.edge_off = d_edge_off, D.clr = d_clr, D.grad = d_grad;
            D.bits = d_bits, D.recip = d_recip, D.total = total, D.band_ok = d_band_ok;

            VMV_LOCKSTEP_HIP(hipMemsetAsync(D.state, 0, n * sizeof(OptState), stream));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(D.done, 0, std::max<size_t>(n, 16), stream));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(d_bits, 0, words * 8, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.x, first, total * dim * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.best, points, total * dim * 4, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_offsets, offsets64.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream));
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_recip, recip.data(), recip.size() * 4, hipMemcpyHostToDevice, stream));
            for (size_t s = 0; s < two.size(); ++s)  // the one edge of a 2-waypoint path
            {
                const float *w = points + offsets[two[s]] * dim;
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.e_start + (act_edges + s) * dim, w, dim * 4, hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.e_goal + (act_edges + s) * dim, w + dim, dim * 4, hipMemcpyHostToDevice, stream));
            }
            const auto upload_active = [&]() -> int {  // (synchronous: the vectors change at the next compaction)
                const size_t na = active.size();
                VMV_LOCKSTEP_HIP(hipMemcpy(d_active, active.data(), na * 4, hipMemcpyHostToDevice));
                VMV_LOCKSTEP_HIP(hipMemcpy(d_act_off, act_off.data(), na * 8, hipMemcpyHostToDevice));
                VMV_LOCKSTEP_HIP(hipMemcpy(d_edge_off, edge_off.data(), na * 8, hipMemcpyHostToDevice));
                if (cb && na)
                {
                    const std::vector<uint32_t> rows = rows_of(active, offsets);
                    VMV_LOCKSTEP_HIP(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
                }
                if (d_edge_recs)  // edge e of active path a: the path's record; behind them the 2-waypoint paths' (first validation)
                {
                    std::vector<uint32_t> owner;
                    for (size_t a = 0; a < na; ++a) owner.insert(owner.end(), offsets[active[a] + 1] - offsets[active[a]] - 1, active[a]);
                    if (na == na0) owner.insert(owner.end(), two.begin(), two.end());
                    if (!owner.empty())
                        VMV_LOCKSTEP_HIP(hipMemcpy(d_edge_recs, constraint_band_expand(recs.data(), owner).data(),
                                                   owner.size() * sizeof(ConstraintDev), hipMemcpyHostToDevice));
                }
                return VMV_OK;
            };
            const auto validated = [&](uint32_t k) { return k % validate_every == 0 || k == P.max_iterations; };
            OptBand band{};
            if (cb)
            {
                band.row_path = d_rows, band.active = d_active, band.act_off = d_act_off, band.edge_off = d_edge_off, band.offsets = d_offsets;
                band.x = D.x, band.q = D.q, band.e_start = D.e_start, band.e_goal = D.e_goal;
                band.change_in = reinterpret_cast<const float *>(reinterpret_cast<const char *>(D.state) + offsetof(OptState, change_in));
                band.state_stride = (uint32_t) (sizeof(OptState) / sizeof(float));
                band.held = d_held, band.unconverged = nullptr, band.total = total;
            }

            uint32_t cur = 0;
            if (na0 == 0 && d_edge_recs)  // (the 2-waypoint paths' records)
                if (int rc = upload_active(); rc != VMV_OK) return rc;
            if (na0)
            {
                if (int rc = upload_active(); rc != VMV_OK) return rc;
                hipLaunchKernelGGL(opt_pack_kernel, dim3((uint32_t) na0), dim3(kOptBlock), 0, stream, P, D, cur, 1u);
                if (int rc = launched(hipGetLastError(), "opt_pack_kernel"); rc != VMV_OK) return rc;
            }
            std::vector<uint64_t> h_bits;
            std::vector<uint8_t> h_band;
            for (uint32_t k = 0; k <= P.max_iterations && (!active.empty() || (k == 0 && !two.empty())); ++k)
            {
                const size_t na = active.size();
                const bool check = validated(k), update = k < P.max_iterations;
                if (na)
                {
                    if (int rc = vmv_clearance_grad_batch_multi(robot, active_envs.data(), wp_seg.data(), na, D.q, d_clr, d_grad, nullptr,
                                                                stream);
                        rc != VMV_OK)
                        return (void) hipDeviceSynchronize(), rc;
                    ++res->clearance_calls;
                }
                if (check)
                {
                    const size_t segs = k == 0 ? na + two.size() : na;
                    if (int rc = vmv_validate_motion_batch_multi(robot, edge_envs.data(), edge_seg.data(), segs, D.e_start, D.e_goal,
                                                                 d_bits, stream);
                        rc != VMV_OK)
                        return (void) hipDeviceSynchronize(), rc;
                    ++res->validation_calls;
                    if (cb)  // the band's answer for the same edges, next to the validation
                        if (int rc = robot_launchers(robot).constraint_edges(cb->P, d_edge_recs ? d_edge_recs : d_recs, D.e_start, D.e_goal,
                                                                             edge_seg[segs], d_band_ok, stream);
                            rc != VMV_OK)
                            return (void) hipDeviceSynchronize(), rc;
                }
                if (na)
                {
                    hipLaunchKernelGGL(opt_step_kernel, dim3((uint32_t) na), dim3(kOptBlock), lds, stream, P, D, cur, k,
                                       update ? 1u : 0u, update && validated(k + 1u) ? 1u : 0u);
                    if (int rc = launched(hipGetLastError(), "opt_step_kernel"); rc != VMV_OK) return rc;
                    if (cb && update)  // every inner waypoint of iterate k + 1 becomes its projection, or stays as in iterate k
                        if (int rc = robot_launchers(robot).opt_band(cb->P, d_recs, band, (uint32_t) wp_seg[na], cur, 0u,
                                                                     validated(k + 1u) ? 1u : 0u, check && k > 0u ? 1u : 0u, P.min_change,
                                                                     stream);
                            rc != VMV_OK)
                            return (void) hipDeviceSynchronize(), rc;
                }
                if (check)
                {
                    if (na)
                    {
                        if (cb)
                            hipLaunchKernelGGL(opt_accept_kernel<true>, dim3((uint32_t) na), dim3(kOptAcceptBlock), 0, stream, P, D, cur, k);
                        else
                            hipLaunchKernelGGL(opt_accept_kernel<false>, dim3((uint32_t) na), dim3(kOptAcceptBlock), 0, stream, P, D, cur, k);
                        if (int rc = launched(hipGetLastError(), "opt_accept_kernel"); rc != VMV_OK) return rc;
                    }
                    if (k == 0 && !two.empty())
                    {
                        h_bits.resize(words);
                        VMV_LOCKSTEP_HIP(hipMemcpyAsync(h_bits.data(), d_bits, words * 8, hipMemcpyDeviceToHost, stream));
                        if (cb)
                        {
                            h_band.resize(two.size());
                            VMV_LOCKSTEP_HIP(hipMemcpyAsync(h_band.data(), d_band_ok + act_edges, two.size(), hipMemcpyDeviceToHost, stream));
                        }
                    }
                    VMV_LOCKSTEP_HIP(hipMemcpyAsync(h_done, D.done, n, hipMemcpyDeviceToHost, stream));
                    VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
                    if (k == 0)
                        for (size_t s = 0; s < two.size(); ++s)
                        {
                            const size_t b = act_edges + s;
                            const bool ok = ((h_bits[b >> 6] >> (b & 63)) & 1ull) != 0 && (!cb || h_band[s] != 0);
                            res->status[two[s]] = ok ? VMV_OPT_OK : VMV_OPT_NO_VALID;
                        }
                    size_t kept = 0;
                    for (size_t a = 0; a < na; ++a)
                        if (!h_done[active[a]]) active[kept] = active[a], active_envs[kept] = active_envs[a], ++kept;
                    if (kept != na || (k == 0 && !two.empty()))
                    {
                        active.resize(kept), active_envs.resize(kept);
                        edge_envs = active_envs;
                        lay_out();
                    }
                    if (update) cur ^= 1u;
                    if (kept != na && kept && update)  // the packed copy of iterate k + 1 in the new layout
                    {
                        if (int rc = upload_active(); rc != VMV_OK) return rc;
                        hipLaunchKernelGGL(opt_pack_kernel, dim3((uint32_t) kept), dim3(kOptBlock), 0, stream, P, D, cur,
                                           validated(k + 1u) ? 1u : 0u);
                        if (int rc = launched(hipGetLastError(), "opt_pack_kernel"); rc != VMV_OK) return rc;
                    }
                }
                else if (update)
                    cur ^= 1u;
            }

            // results: the states, and the best iterates in the input's layout
            if (na0)
            {
                std::vector<OptState> states(n);
                VMV_LOCKSTEP_HIP(hipMemcpy(states.data(), D.state, n * sizeof(OptState), hipMemcpyDeviceToHost));
                VMV_LOCKSTEP_HIP(hipMemcpy(res->points.data(), D.best, total * dim * 4, hipMemcpyDeviceToHost));
                if (cb) VMV_LOCKSTEP_HIP(hipMemcpy(res->held.data(), d_held, n * 4, hipMemcpyDeviceToHost));
                for (size_t k = 0; k < n; ++k)
                {
                    if (offsets[k + 1] - offsets[k] < 3 || res->status[k] == VMV_OPT_NONFINITE || res->status[k] == VMV_OPT_OUT_OF_BAND) continue;
                    const OptState &st = states[k];
                    res->status[k] = (uint8_t) st.status;
                    res->iterations[k] = st.iterations, res->best_iteration[k] = st.best_iteration;
                    res->cost_first[k] = st.u_first, res->cost[k] = st.has_best ? st.u_best : st.u_first;
                    res->clearance_first[2 * k] = st.env_first, res->clearance_first[2 * k + 1] = st.self_first;
                    res->clearance[2 * k] = st.has_best ? st.env_best : st.env_first;
                    res->clearance[2 * k + 1] = st.has_best ? st.self_best : st.self_first;
                }
            }
            return VMV_OK;
        }

        // The checks of both entry points, none of which needs a device, in the header's order -> the resolved settings
        int optimize_checks(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                            const vmv_optimize_settings *settings, vmv_optimized *const *out, OptParams &P)
        {
            // device-free checks, in vmv_simplify_multi's order; the refused kinds follow (check_env_kinds), the rest of
            // the environments' checks are vmv_env_prepare_multi's
            const int dim = vmv_robot_dimension(robot);
            if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
            if (!settings || !out || (n_paths > 0 && (!envs || !offsets))) return VMV_ERR_INVALID_ARGUMENT;
            const vmv_optimize_settings &S = *settings;
            if (n_paths >= kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
            const uint32_t max_waypoints = S.max_waypoints ? S.max_waypoints : kOptDefaultWaypoints;
            if (max_waypoints > kOptMaxWaypoints) return VMV_ERR_INVALID_ARGUMENT;
            if (n_paths > 0 && offsets[0] != 0) return VMV_ERR_INVALID_ARGUMENT;
            for (size_t k = 0; k < n_paths; ++k)
            {
                if (offsets[k + 1] < offsets[k]) return VMV_ERR_INVALID_ARGUMENT;
                if (offsets[k + 1] - offsets[k] > max_waypoints) return VMV_ERR_INVALID_ARGUMENT;
            }
            if (n_paths > 0 && offsets[n_paths] > 0 && !points) return VMV_ERR_INVALID_ARGUMENT;
            for (size_t k = 0; k < n_paths; ++k)
                if (!envs[k]) return VMV_ERR_INVALID_ARGUMENT;
            const auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
            const auto weight = [](float v) { return std::isfinite(v) && v >= 0.f; };
            if (!positive(S.step) || !positive(S.max_step) || !positive(S.env_margin) || !positive(S.self_margin))
                return VMV_ERR_INVALID_ARGUMENT;
            if (!weight(S.smooth_weight) || !weight(S.env_weight) || !weight(S.self_weight)) return VMV_ERR_INVALID_ARGUMENT;
            if (std::isnan(S.min_change)) return VMV_ERR_INVALID_ARGUMENT;
            if (S.validate_every == 0) return VMV_ERR_INVALID_ARGUMENT;
            if (n_paths > 0 && offsets[n_paths] >= kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
            P.dim = (uint32_t) dim, P.max_iterations = S.max_iterations ? S.max_iterations : kOptDefaultIterations;
            P.step = S.step, P.max_step = S.max_step, P.min_change = S.min_change;
            P.w_smooth = S.smooth_weight, P.w_env = S.env_weight, P.w_self = S.self_weight;
            P.eps_env = S.env_margin, P.eps_self = S.self_margin;
            {
                float lower[kPlanMaxDim] = {}, span[kPlanMaxDim] = {}, descale[kPlanMaxDim] = {};
                if (int rc = vmv_robot_bounds(robot, lower, span, descale); rc != VMV_OK) return rc;
                for (int j = 0; j < dim; ++j) P.lower[j] = lower[j], P.upper[j] = lower[j] + span[j];
            }
            return VMV_OK;
        }

    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_optimize_multi(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                           const vmv_optimize_settings *settings, vmv_optimized **out)
    {
        vmv::OptParams P{};
        if (int rc = vmv::optimize_checks(robot, envs, n_paths, points, offsets, settings, out, P); rc != VMV_OK) return rc;
        if (int rc = vmv::check_env_kinds(robot, envs, n_paths, true); rc != VMV_OK) return rc;
        return vmv::lockstep_call(robot, envs, n_paths, (int) P.dim, out, [&](vmv_optimized *res) {
            return vmv::optimize_multi_run(robot, envs, n_paths, points, offsets, P, settings->validate_every, res);
        });
    }

    int vmv_optimize_multi_constrained(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                                       const vmv_optimize_settings *settings, const vmv_ee_constraint *constraints, size_t n_constraints,
                                       const vmv_constraint_settings *constraint_settings, vmv_optimized **out)
    {
        // vmv_optimize_multi's checks in its order, then the constraint's own in vmv_constraint_project_batch's; none needs a device
        vmv::OptParams P{};
        if (int rc = vmv::optimize_checks(robot, envs, n_paths, points, offsets, settings, out, P); rc != VMV_OK) return rc;
        vmv::ConstraintBand cb{};
        const std::string err = vmv::constraint_band_checks(constraints, n_constraints, constraint_settings, n_paths, "n_paths", nullptr, cb);
        if (!err.empty()) return vmv::refuse_argument(err.c_str());
        for (uint32_t j = 0; j < 16; ++j) cb.P.lower[j] = j < P.dim ? P.lower[j] : 0.f, cb.P.upper[j] = j < P.dim ? P.upper[j] : 0.f;
        if (int rc = vmv::check_env_kinds(robot, envs, n_paths, true); rc != VMV_OK) return rc;
        const int rc = vmv::lockstep_call(robot, envs, n_paths, (int) P.dim, out, [&](vmv_optimized *res) {
            return vmv::optimize_multi_run(robot, envs, n_paths, points, offsets, P, settings->validate_every, res, &cb);
        });
        if (rc == VMV_OK) (*out)->constrained = true, (*out)->held.resize(n_paths);
        return rc;
    }

    int vmv_optimized_held(const vmv_optimized *result, uint32_t *held)
    {
        if (!result || !result->constrained) return VMV_ERR_INVALID_ARGUMENT;
        if (held && result->n) std::memcpy(held, result->held.data(), result->n * 4);
        return VMV_OK;
    }

    int vmv_optimized_summary(const vmv_optimized *result, uint8_t *status, uint32_t *iterations, uint32_t *best_iteration,
                              float *cost_first, float *cost, float *clearance_first, float *clearance, uint64_t *clearance_calls,
                              uint64_t *validation_calls)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = result->n;
        if (status && n) std::memcpy(status, result->status.data(), n);
        if (iterations && n) std::memcpy(iterations, result->iterations.data(), n * 4);
        if (best_iteration && n) std::memcpy(best_iteration, result->best_iteration.data(), n * 4);
        if (cost_first && n) std::memcpy(cost_first, result->cost_first.data(), n * 4);
        if (cost && n) std::memcpy(cost, result->cost.data(), n * 4);
        if (clearance_first && n) std::memcpy(clearance_first, result->clearance_first.data(), n * 8);
        if (clearance && n) std::memcpy(clearance, result->clearance.data(), n * 8);
        if (clearance_calls) *clearance_calls = result->clearance_calls;
        if (validation_calls) *validation_calls = result->validation_calls;
        return VMV_OK;
    }

    int vmv_optimized_points(const vmv_optimized *result, float *out, size_t capacity_floats)
    {
        if (!result || (!out && !result->points.empty())) return VMV_ERR_INVALID_ARGUMENT;
        if (capacity_floats < result->points.size()) return VMV_ERR_CAPACITY;
        if (!result->points.empty()) std::memcpy(out, result->points.data(), result->points.size() * 4);
        return VMV_OK;
    }

    int vmv_optimized_destroy(vmv_optimized *result)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        delete result;
        return VMV_OK;
    }
}
