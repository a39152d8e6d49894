// vmv_constraint.h — end-effector constraints (include/vamp_mvt_amd.h: vmv_ee_constraint): the host set-up
// that turns a caller's constraint and settings into the records the device reads, and the full statement of what the
// device computes from them.  Plain C++ without a HIP header, so that tests/native/constraint_sanitize.cc compiles it on
// its own.
//
// THE CONSTRAINT.  C = (C_R, C_t) is a rigid frame in the world, (R, t) the end-effector frame of a configuration q.
//   position   p = C_R^T (t - C_t); the nominal band is lo_k <= p_k <= hi_k for k = 0, 1, 2 (-inf / +inf: free; lo == hi:
//              a plane or a line);
//   axis       a = R u (u = tool_axis, unit, in the end-effector frame), d = C_R ref_axis (unit, in the world); the
//              nominal band is angle(a, d) <= max_angle; max_angle == 0 leaves the orientation free.
// Set-up (constraint_refusal, then constraint_record below) normalises u and ref_axis in float64, rotates ref_axis into the world, computes
// cos_m = cos(max_angle), sin_m = sin(max_angle), cos_band = cos(max_angle + rot_tol), lo_band = lo - pos_tol and
// hi_band = hi + pos_tol in float64, and rounds each value once to fp32 into a ConstraintDev.
//
// THE RESIDUAL (device, fp32, one rounding per written operation, every 3-term sum as ((a0 b0 + a1 b1) + a2 b2)).
//   dt = t - C_t; p_k = column k of C_R . dt; v_k = p_k - min(max(p_k, lo_k), hi_k); e_p = -C_R v in the world, |e_p| = |v|.
//   a_r = row r of R . u; c = a x d; sin = sqrt(c . c); cos = a . d; n = c / (sin > 0 ? sin : 1).
//   excess s = sin cos_m - cos sin_m (the sine of angle - max_angle); where cos cos_m + sin sin_m <= 0 (the excess is
//   90 degrees or more) s = 1, as the pose error of vmv_ik_batch does beyond 90 degrees.
//   The axis part is active ("tilted") iff the constraint has an axis and cos < cos_m; e_w = rot_weight s n then, else 0.
//   E = 1/2 (|v|^2 + (rot_weight s)^2 [tilted]).
//   Antiparallel axes (sin == 0 and cos < 0) have no direction n: see the projection.
// THE BAND TEST: lo_band_k <= p_k <= hi_band_k for every k, and (no axis or cos >= cos_band).  A configuration with a
// non-finite joint is out of band.  Every kernel asks this one function (constraint_residual in vmv_robot_tu.inc).
// The residual pair reported to the caller: |v| in metres and, where tilted, atan2(sin cos_m - cos sin_m, cos cos_m + sin
// sin_m) = angle - max_angle in radians, else 0.
//
// THE PROJECTION is vmv_ik_batch's iteration with this residual in place of the pose error.  With J the geometric
// Jacobian of vmv_eefk_jacobian_batch (rows 0-2 dt/dq_j, rows 3-5 the angular velocity), the six rows of the step are
//   rows 0-2   column k of C_R . (dt/dq_j), right-hand side -v_k; a row whose v_k == 0 is zero;
//   row 3      rot_weight n . omega_j, right-hand side rot_weight s   (turns a towards d);
//   row 4      rot_weight (a x n) . omega_j, right-hand side 0        (holds a in the plane of a and d);
//   row 5      zero (rotation about the tool axis stays free);
// rows 3 and 4 are zero unless tilted.  The input is clipped to the joint bounds and evaluated; then per iteration the
// column of every joint that sits at a bound while the descent direction points outward is set to zero (the bound-hold
// rule), A = Jm Jm^T + lambda I, A y = e by the 6 x 6 Cholesky, delta = Jm^T y scaled so that max_j |delta_j| <= max_step,
// q' = q + delta clipped to the bounds; q' is evaluated and accepted iff E' < E, with lambda = max(lambda / 4, 1e-5) on
// acceptance and min(4 lambda, 1e6) otherwise, from lambda = damping.  The band test runs on the accepted state after
// every evaluation; a state in the band is converged and stops changing; a wave stops when its lanes are done or after
// max_iterations evaluations beyond the first.  Only joints in the robot's kEeJointMask move.  Hence:
//   * an input inside the joint bounds and in the band comes back bit for bit, converged, with 0 evaluations;
//   * an input whose axes are antiparallel is not converged and comes back as given, with 0 evaluations (there is no
//     direction to turn in);
//   * an input with a non-finite joint comes back as given with NaN residuals and status bit 30;
//   * every other output is the accepted state of smallest E: never worse than the clipped input, inside the bounds.  The
//     two kinds of rows that come back as given are NOT clipped: such a row lies outside the bounds if its input did.
// Status word: bit 31 converged, bit 30 non-finite input, the low bits the evaluations after the first.
//
// AN EDGE a -> b: n_c = max(1, ceil(|b - a| / check_step)) with |b - a| = sqrt of the squares summed in joint order, all
// fp32; an edge with n_c > 1,024 or a non-finite length fails; else the samples are a + (b - a) * (i / n_c), i = 1 .. n_c
// (the quotient, the product and the sum rounded once each), and the edge is in band iff every sample passes the band test.
#pragma once

#include "../../include/vamp_mvt_amd.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vmv
{
    constexpr uint32_t kConstraintMaxSamples = 1024;  // band samples of one edge at most

    struct ConstraintDev  // one constraint as the device reads it
    {
        float t[3], R[9];  // C_t, C_R row-major
        float lo[3], hi[3], lo_band[3], hi_band[3];
        float u[3], d[3];  // unit tool axis in the end-effector frame, unit reference axis in the world
        float cos_m, sin_m, cos_band;
        uint32_t axis;  // 0: the orientation is free
    };
    static_assert(sizeof(ConstraintDev) == 34 * 4, "33 floats and the flag");

    struct ConstraintParams  // vmv_constraint_settings as resolved, the robot's bounds [lower, lower + span]
    {
        uint32_t max_iterations;
        float pos_tol, rot_tol, rot_weight, damping, max_step, check_step;
        uint32_t shared;  // 1: one ConstraintDev for every lane, 0: one per lane
        float lower[16], upper[16];
    };

    // The settings with their defaults in place; -> nullptr or what is wrong (names the field).
    inline const char *constraint_settings(const vmv_constraint_settings &s, ConstraintParams &P)
    {
        const auto bad = [](float v) { return !(std::isfinite(v) && v >= 0.0f); };
        if (s.max_iterations >= (1u << 30)) return "max_iterations must be 0 (default) .. 2^30 - 1";
        if (bad(s.pos_tol)) return "pos_tol must be finite and not negative (0 = default)";
        if (bad(s.rot_tol)) return "rot_tol must be finite and not negative (0 = default)";
        if (bad(s.rot_weight)) return "rot_weight must be finite and not negative (0 = default)";
        if (bad(s.damping)) return "damping must be finite and not negative (0 = default)";
        if (bad(s.max_step)) return "max_step must be finite and not negative (0 = default)";
        if (bad(s.check_step)) return "check_step must be finite and not negative (0 = default)";
        const auto or_default = [](float v, float d) { return v > 0.0f ? v : d; };
        P.max_iterations = s.max_iterations ? s.max_iterations : 16u;
        P.pos_tol = or_default(s.pos_tol, 1e-4f), P.rot_tol = or_default(s.rot_tol, 1e-3f);
        P.rot_weight = or_default(s.rot_weight, 0.25f), P.damping = or_default(s.damping, 1e-2f);  // vmv_ik_settings' defaults
        P.max_step = or_default(s.max_step, 0.5f);
        P.check_step = or_default(s.check_step, 0.05f);
        return nullptr;
    }

    // What is wrong with a constraint, or nullptr: the checks alone, so that a call can refuse before it holds any
    // device resource and then build its records in place (constraint_record).
    inline const char *constraint_refusal(const vmv_ee_constraint &c)
    {
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(c.frame[k])) return "frame must be finite";
        for (int k = 0; k < 3; ++k)
        {
            if (std::isnan(c.pos_lo[k]) || std::isnan(c.pos_hi[k])) return "pos_lo / pos_hi must not be NaN";
            if (c.pos_lo[k] > c.pos_hi[k]) return "pos_lo must not exceed pos_hi";
            if (c.pos_lo[k] == INFINITY || c.pos_hi[k] == -INFINITY) return "pos_lo must be below +inf and pos_hi above -inf";
            if (!std::isfinite(c.tool_axis[k]) || !std::isfinite(c.ref_axis[k])) return "tool_axis / ref_axis must be finite";
        }
        if (std::isnan(c.max_angle)) return "max_angle must not be NaN";
        double Rm[9];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) Rm[3 * r + k] = (double) c.frame[4 * r + k];
        for (int i = 0; i < 3; ++i)  // R^T R = I within 1e-4, a proper rotation, the last row (0, 0, 0, 1)
            for (int j = 0; j < 3; ++j)
            {
                const double g = Rm[i] * Rm[j] + Rm[3 + i] * Rm[3 + j] + Rm[6 + i] * Rm[6 + j];
                if (std::fabs(g - (i == j ? 1.0 : 0.0)) > 1e-4) return "frame must be rigid (R^T R = I within 1e-4)";
            }
        const double det = Rm[0] * (Rm[4] * Rm[8] - Rm[5] * Rm[7]) - Rm[1] * (Rm[3] * Rm[8] - Rm[5] * Rm[6]) +
                           Rm[2] * (Rm[3] * Rm[7] - Rm[4] * Rm[6]);
        if (det < 0.0) return "frame must be rigid (a reflection)";
        for (int k = 0; k < 4; ++k)
            if (std::fabs((double) c.frame[12 + k] - (k == 3 ? 1.0 : 0.0)) > 1e-4) return "frame must be rigid (last row 0 0 0 1)";
        if (!(c.max_angle >= 0.0f && c.max_angle <= 1.57079637f)) return "max_angle must be in [0, pi/2]";
        const auto zero = [](const float (&v)[3]) { return v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f; };
        if (c.max_angle > 0.0f && (zero(c.tool_axis) || zero(c.ref_axis))) return "tool_axis and ref_axis must not be zero while max_angle > 0";
        return nullptr;
    }

    // The device record of a constraint that constraint_refusal passes.
    inline void constraint_record(const vmv_ee_constraint &c, double pos_tol, double rot_tol, ConstraintDev &out)
    {
        double Rm[9];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) Rm[3 * r + k] = (double) c.frame[4 * r + k];
        const bool axis = c.max_angle > 0.0f;
        double u[3] = {0.0, 0.0, 1.0}, d[3] = {0.0, 0.0, 1.0};
        if (axis)
        {
            const double lu = std::sqrt((double) c.tool_axis[0] * c.tool_axis[0] + (double) c.tool_axis[1] * c.tool_axis[1] +
                                        (double) c.tool_axis[2] * c.tool_axis[2]);
            const double lr = std::sqrt((double) c.ref_axis[0] * c.ref_axis[0] + (double) c.ref_axis[1] * c.ref_axis[1] +
                                        (double) c.ref_axis[2] * c.ref_axis[2]);
            for (int r = 0; r < 3; ++r)
            {
                u[r] = (double) c.tool_axis[r] / lu;
                d[r] = (Rm[3 * r] * c.ref_axis[0] + Rm[3 * r + 1] * c.ref_axis[1] + Rm[3 * r + 2] * c.ref_axis[2]) / lr;
            }
            const double ld = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);  // (the frame is rigid within 1e-4 only)
            for (double &x : d) x /= ld;
        }
        for (int r = 0; r < 3; ++r)
        {
            out.t[r] = c.frame[4 * r + 3];
            for (int k = 0; k < 3; ++k) out.R[3 * r + k] = c.frame[4 * r + k];
            out.lo[r] = c.pos_lo[r], out.hi[r] = c.pos_hi[r];
            out.lo_band[r] = (float) ((double) c.pos_lo[r] - pos_tol), out.hi_band[r] = (float) ((double) c.pos_hi[r] + pos_tol);
            out.u[r] = (float) u[r], out.d[r] = (float) d[r];
        }
        out.cos_m = (float) std::cos((double) c.max_angle), out.sin_m = (float) std::sin((double) c.max_angle);
        out.cos_band = axis ? (float) std::cos((double) c.max_angle + rot_tol) : -2.0f;
        out.axis = axis ? 1u : 0u;
    }

    // One constraint -> its device record; -> nullptr or what is wrong.  `out` is written only on success.
    inline const char *constraint_setup(const vmv_ee_constraint &c, double pos_tol, double rot_tol, ConstraintDev &out)
    {
        if (const char *err = constraint_refusal(c)) return err;
        constraint_record(c, pos_tol, rot_tol, out);
        return nullptr;
    }

    // THE BAND OF ONE CALL on the host, as every constraint-taking entry point sets it up: the resolved settings and the
    // robot's bounds (P), and the caller's constraints - one for every item of the call (P.shared) or one per item; none
    // (count 0) only where the call allows it (vmv_retime_multi_constrained).
    struct ConstraintBand
    {
        ConstraintParams P;
        const vmv_ee_constraint *constraints;
        size_t count;
    };

    // The checks behind a call's NULL and count checks, in the order every call makes them: the settings, the call's own
    // check (own_refusal: what it found, nullptr = nothing), every constraint in order.  -> "" with B filled but for its
    // bounds, or what is wrong; the caller puts its own prefix in front and refuses.
    inline std::string constraint_band_resolve(const vmv_ee_constraint *constraints, size_t n_constraints,
                                               const vmv_constraint_settings &settings, const char *own_refusal, ConstraintBand &B)
    {
        if (const char *err = constraint_settings(settings, B.P)) return err;
        if (own_refusal) return own_refusal;
        for (size_t k = 0; k < n_constraints; ++k)
            if (const char *err = constraint_refusal(constraints[k])) return "constraints[" + std::to_string(k) + "]: " + err;
        B.constraints = constraints, B.count = n_constraints, B.P.shared = n_constraints == 1 ? 1u : 0u;
        return std::string();
    }
    // The whole of it for a call whose words are the common ones: "null pointer", then "n_constraints must be 1 or
    // <items>" (items: the header's name of the call's count n), then constraint_band_resolve.
    inline std::string constraint_band_checks(const vmv_ee_constraint *constraints, size_t n_constraints,
                                              const vmv_constraint_settings *settings, size_t n, const char *items,
                                              const char *own_refusal, ConstraintBand &B)
    {
        if (!constraints || !settings) return "null pointer";
        if (n_constraints != 1 && n_constraints != n) return std::string("n_constraints must be 1 or ") + items;
        return constraint_band_resolve(constraints, n_constraints, *settings, own_refusal, B);
    }

    // The robot's joint bounds [lower, lower + span] into the band; the entries from `dim` on are 0.
    inline void constraint_band_bounds(ConstraintBand &B, const float *lower, const float *span, int dim)
    {
        for (int j = 0; j < 16; ++j) B.P.lower[j] = j < dim ? lower[j] : 0.f, B.P.upper[j] = j < dim ? lower[j] + span[j] : 0.f;
    }

    // The band's records into out [B.count], which the caller provides: pinned memory, a vector's storage.
    inline void constraint_band_records(const ConstraintBand &B, ConstraintDev *out)
    {
        for (size_t k = 0; k < B.count; ++k) constraint_record(B.constraints[k], (double) B.P.pos_tol, (double) B.P.rot_tol, out[k]);
    }

    // One record per lane from one per item: lane i gets the record of item owner[i].  What a kernel that reads "one record
    // or one per lane" needs where an item has several lanes (its goals, its edges, its two ends).
    inline std::vector<ConstraintDev> constraint_band_expand(const ConstraintDev *records, const std::vector<uint32_t> &owner)
    {
        std::vector<ConstraintDev> out(owner.size());
        for (size_t i = 0; i < owner.size(); ++i) out[i] = records[owner[i]];
        return out;
    }
}  // namespace vmv
