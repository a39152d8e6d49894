// vmv_cartesian_multi.hip — straight-line end-effector motions for many independent problems (vmv_cartesian_multi,
// DESIGN §5m).  The host sets every line up in float64 from the fp32 frames (vmv_cartesian_line.h), so it knows each
// problem's segment count and the packed output's layout before anything is launched; ONE launch of the robot's
// cartesian_track_kernel (csrc/vmv_robot_tu.inc; one lane per problem) walks all lines; then the starts go through ONE
// vmv_validate_batch_multi call, the tracked edges through ONE vmv_validate_motion_batch_multi call, and the host cuts
// every path in front of its first invalid edge.  The contract is in include/vamp_mvt_amd.h.
//
// The prologue is the existing calls' own: the handles are checked by an empty vmv_validate_batch_multi batch (robot,
// NULL, finalized; no device), the device by vmv_eefk_batch_host, which also gives the start frames, and the
// environments' device and robot parts by vmv_env_prepare_multi.
#include "../../include/vamp_mvt_amd.h"

#include "vmv_cartesian_line.h"
#include "vmv_lockstep.h"

#include <cmath>
#include <cstring>

struct vmv_cartesian
{
    size_t n = 0;
    int dim = 0;
    std::vector<uint8_t> status;
    std::vector<uint32_t> segments, achieved, evaluations;
    std::vector<float> points;  // achieved + 1 waypoints per problem, packed in problem order
    uint64_t validation_calls = 0, questions = 0;
};

namespace vmv
{
    namespace
    {
        constexpr uint32_t kCartMaxWaypoints = 1024;

        struct CartHostSettings
        {
            double pos_step, rot_step;
            uint32_t max_waypoints;
            bool position_only;
        };

        bool finite_all(const float *v, size_t count)
        {
            for (size_t k = 0; k < count; ++k)
                if (!std::isfinite(v[k])) return false;
            return true;
        }

        // The caller has checked every argument, n > 0, and (with envs) every environment is finalized on the current
        // device with the robot's part built.
        int cartesian_multi_run(int robot, const vmv_env *const *envs, size_t n, const float *starts, const float *targets,
                                CartParams P, const CartHostSettings &S, vmv_cartesian *res)
        {
            const size_t dim = (size_t) res->dim;
            hipStream_t stream = nullptr;
            res->n = n;
            res->status.assign(n, VMV_CART_COMPLETE), res->segments.assign(n, 0), res->achieved.assign(n, 0);
            res->evaluations.assign(n, 0);

            // the starts the device sees (a non-finite problem's are zeros) and their frames
            std::vector<float> clean(starts, starts + n * dim), frames(n * 16);
            std::vector<uint8_t> finite(n);
            for (size_t p = 0; p < n; ++p)
            {
                finite[p] = finite_all(starts + p * dim, dim) && finite_all(targets + p * 16, 16);
                if (!finite[p])
                {
                    res->status[p] = VMV_CART_NON_FINITE;
                    std::fill(clean.begin() + p * dim, clean.begin() + (p + 1) * dim, 0.0f);
                }
            }
            if (int rc = vmv_eefk_batch_host(robot, clean.data(), n, frames.data()); rc != VMV_OK) return rc;
            for (size_t p = 0; p < n; ++p)  // a finite start of huge entries may have no finite frame: no line to set up
                if (finite[p] && !finite_all(frames.data() + p * 16, 16))
                {
                    finite[p] = 0, res->status[p] = VMV_CART_NON_FINITE;
                    std::fill(clean.begin() + p * dim, clean.begin() + (p + 1) * dim, 0.0f);
                }

            // the lines: every m, the packed layout, who takes part
            std::vector<CartLine> lines(n);
            std::vector<uint32_t> part;
            uint64_t rows = 0;
            uint32_t longest = 0;
            for (size_t p = 0; p < n; ++p)
            {
                CartLine &L = lines[p];
                std::memset(&L, 0, sizeof(L));
                L.offset = rows;
                if (!finite[p]) continue;
                const CartLineSetup H = cart_line(frames.data() + p * 16, targets + p * 16, S.pos_step, S.rot_step, S.position_only);
                res->segments[p] = (uint32_t) H.m;
                if (H.m + 1 > S.max_waypoints)
                {
                    res->status[p] = VMV_CART_TOO_LONG;
                    continue;
                }
                for (int k = 0; k < 3; ++k) L.p0[k] = (float) H.p0[k], L.dp[k] = (float) H.dp[k], L.axis[k] = (float) H.axis[k];
                for (int k = 0; k < 9; ++k) L.R0[k] = (float) H.R0[k];
                L.theta = (float) H.theta, L.m = (uint32_t) H.m;
                rows += H.m + 1;
                longest = std::max(longest, L.m);
                part.push_back((uint32_t) p);
            }
            P.max_k = longest;

            std::vector<float> tracked_rows(rows * dim);
            std::vector<CartResult> results(n, CartResult{0u, (uint32_t) VMV_CART_COMPLETE, 0u, 0u});
            if (!part.empty())
            {
                // one allocation for the four arrays, each at a 256-byte boundary
                const auto padded = [](size_t bytes) { return (bytes + 255) & ~size_t{255}; };
                const size_t at_results = padded(n * sizeof(CartLine)), at_starts = at_results + padded(n * sizeof(CartResult));
                const size_t at_points = at_starts + padded(n * dim * 4);
                DeviceBuffers mem;
                char *base = nullptr;
                VMV_LOCKSTEP_HIP(mem.alloc(&base, at_points + rows * dim * 4));
                CartLine *d_lines = reinterpret_cast<CartLine *>(base);
                CartResult *d_results = reinterpret_cast<CartResult *>(base + at_results);
                float *d_starts = reinterpret_cast<float *>(base + at_starts), *d_points = reinterpret_cast<float *>(base + at_points);
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_lines, lines.data(), n * sizeof(CartLine), hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_starts, clean.data(), n * dim * 4, hipMemcpyHostToDevice, stream));
                VMV_LOCKSTEP_HIP(hipMemsetAsync(d_points, 0, rows * dim * 4, stream));
                if (int rc = robot_launchers(robot).cartesian(P, d_lines, d_starts, n, d_points, d_results, stream); rc != VMV_OK)
                    return (void) hipDeviceSynchronize(), rc;
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(results.data(), d_results, n * sizeof(CartResult), hipMemcpyDeviceToHost, stream));
                VMV_LOCKSTEP_HIP(hipMemcpyAsync(tracked_rows.data(), d_points, rows * dim * 4, hipMemcpyDeviceToHost, stream));
                VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
            }
            for (const uint32_t p : part)  // row 0 is the start's bits, whatever the clip made of it on the device
            {
                std::memcpy(tracked_rows.data() + lines[p].offset * dim, starts + (size_t) p * dim, dim * 4);
                const CartResult &r = results[p];
                res->status[p] = (uint8_t) r.status, res->achieved[p] = std::min(r.tracked, lines[p].m), res->evaluations[p] = r.evaluations;
            }

            // validation: the starts, then the tracked edges, a segment per taking-part problem as vmv_optimize_multi lays
            // its paths' edges out; the cut reads the answers here
            if (envs && !part.empty())
            {
                const size_t np = part.size();
                std::vector<const vmv_env *> part_envs(np);
                std::vector<size_t> start_seg(np + 1), edge_seg(np + 1, 0);
                std::vector<float> q0(np * dim);
                for (size_t a = 0; a < np; ++a)
                {
                    part_envs[a] = envs[part[a]], start_seg[a] = a;
                    std::memcpy(q0.data() + a * dim, starts + (size_t) part[a] * dim, dim * 4);
                    edge_seg[a + 1] = edge_seg[a] + res->achieved[part[a]];
                }
                start_seg[np] = np;
                const size_t n_edges = edge_seg[np];
                std::vector<uint64_t> start_bits((np + 63) / 64 + 1, 0), edge_bits((n_edges + 63) / 64 + 1, 0);
                if (int rc = vmv_validate_batch_multi_host(robot, part_envs.data(), start_seg.data(), np, q0.data(), start_bits.data());
                    rc != VMV_OK)
                    return rc;
                ++res->validation_calls, res->questions += np;
                if (n_edges)
                {
                    std::vector<float> e_start(n_edges * dim), e_goal(n_edges * dim);
                    for (size_t a = 0; a < np; ++a)
                    {
                        const float *w = tracked_rows.data() + lines[part[a]].offset * dim;
                        const size_t t = res->achieved[part[a]];
                        if (!t) continue;
                        std::memcpy(e_start.data() + edge_seg[a] * dim, w, t * dim * 4);
                        std::memcpy(e_goal.data() + edge_seg[a] * dim, w + dim, t * dim * 4);
                    }
                    if (int rc = vmv_validate_motion_batch_multi_host(robot, part_envs.data(), edge_seg.data(), np, e_start.data(),
                                                                      e_goal.data(), edge_bits.data());
                        rc != VMV_OK)
                        return rc;
                    ++res->validation_calls, res->questions += n_edges;
                }
                for (size_t a = 0; a < np; ++a)
                {
                    const uint32_t p = part[a];
                    if (!((start_bits[a >> 6] >> (a & 63u)) & 1ull))
                    {
                        res->status[p] = VMV_CART_INVALID_START, res->achieved[p] = 0;
                        continue;
                    }
                    const uint32_t kept = cart_cut(edge_bits.data(), edge_seg[a], res->achieved[p]);
                    if (kept < res->achieved[p]) res->status[p] = VMV_CART_COLLISION, res->achieved[p] = kept;
                }
            }

            // the packed result: achieved + 1 waypoints per problem; a problem that took no part gives its start as passed
            size_t total = 0;
            for (size_t p = 0; p < n; ++p) total += res->achieved[p] + 1u;
            res->points.resize(total * dim);
            float *o = res->points.data();
            for (size_t p = 0; p < n; ++p)
            {
                const bool took = lines[p].m != 0u;
                const float *w = took ? tracked_rows.data() + lines[p].offset * dim : starts + p * dim;
                const size_t count = ((size_t) res->achieved[p] + 1u) * dim;
                std::memcpy(o, w, count * 4);
                o += count;
            }
            return VMV_OK;
        }
    }  // namespace
}  // namespace vmv

extern "C"
{
    int vmv_cartesian_multi(int robot, const vmv_env *const *envs, size_t n, const float *starts, const float *targets,
                            const vmv_cartesian_settings *settings, vmv_cartesian **out)
    {
        const int dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || dim <= 0 || dim > (int) vmv::kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n > 0 && (!starts || !targets))) return VMV_ERR_INVALID_ARGUMENT;
        const vmv_cartesian_settings &S = *settings;
        const float values[] = {S.pos_step, S.rot_step, S.pos_tol, S.rot_tol, S.rot_weight, S.damping, S.max_step, S.max_joint_step};
        for (const float v : values)
            if (!std::isfinite(v)) return VMV_ERR_INVALID_ARGUMENT;
        if (S.max_iterations >= (1u << 30)) return VMV_ERR_INVALID_ARGUMENT;
        if (S.max_waypoints > vmv::kCartMaxWaypoints) return VMV_ERR_INVALID_ARGUMENT;
        if (S.position_only != 0 && S.position_only != 1) return VMV_ERR_INVALID_ARGUMENT;
        if (n >= vmv::kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        if (int rc = vmv::check_env_kinds(robot, envs, n, false); rc != VMV_OK) return rc;
        const auto or_default = [](float v, float d) { return v > 0.0f ? v : d; };
        vmv::CartParams P{};
        P.max_iterations = S.max_iterations ? S.max_iterations : 16u;
        P.pos_tol = or_default(S.pos_tol, 1e-4f), P.rot_tol = or_default(S.rot_tol, 1e-3f);
        P.rot_weight = S.position_only ? 0.0f : or_default(S.rot_weight, 0.25f);
        P.damping = or_default(S.damping, 1e-2f), P.max_step = or_default(S.max_step, 0.5f);
        P.max_joint_step = or_default(S.max_joint_step, 0.3f);
        P.position_only = (uint32_t) S.position_only;
        {
            float lower[vmv::kPlanMaxDim] = {}, span[vmv::kPlanMaxDim] = {}, descale[vmv::kPlanMaxDim] = {};
            if (int rc = vmv_robot_bounds(robot, lower, span, descale); rc != VMV_OK) return rc;
            for (int j = 0; j < dim; ++j) P.lower[j] = lower[j], P.upper[j] = lower[j] + span[j];
        }
        const vmv::CartHostSettings H{(double) or_default(S.pos_step, 0.01f), (double) or_default(S.rot_step, 0.05f),
                                      S.max_waypoints ? S.max_waypoints : vmv::kCartMaxWaypoints, S.position_only != 0};
        return vmv::lockstep_call(robot, envs, n, dim, out, [&](vmv_cartesian *result) {
            return vmv::cartesian_multi_run(robot, envs, n, starts, targets, P, H, result);
        });
    }

    int vmv_cartesian_summary(const vmv_cartesian *result, uint8_t *status, uint32_t *segments, uint32_t *achieved,
                              uint32_t *evaluations, uint64_t *validation_calls, uint64_t *questions)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        const size_t n = result->n;
        if (status && n) std::memcpy(status, result->status.data(), n);
        if (segments && n) std::memcpy(segments, result->segments.data(), n * 4);
        if (achieved && n) std::memcpy(achieved, result->achieved.data(), n * 4);
        if (evaluations && n) std::memcpy(evaluations, result->evaluations.data(), n * 4);
        if (validation_calls) *validation_calls = result->validation_calls;
        if (questions) *questions = result->questions;
        return VMV_OK;
    }

    int vmv_cartesian_points(const vmv_cartesian *result, float *out, size_t capacity_floats)
    {
        if (!result || (!out && !result->points.empty())) return VMV_ERR_INVALID_ARGUMENT;
        if (capacity_floats < result->points.size()) return VMV_ERR_CAPACITY;
        if (!result->points.empty()) std::memcpy(out, result->points.data(), result->points.size() * 4);
        return VMV_OK;
    }

    int vmv_cartesian_destroy(vmv_cartesian *result)
    {
        if (!result) return VMV_ERR_INVALID_ARGUMENT;
        delete result;
        return VMV_OK;
    }
}
