// vmv_cartesian_line.h — the host steps of vmv_cartesian_multi that make no device call (include/vamp_mvt_amd.h, DESIGN
// §5m): the float64 set-up of a line from two fp32 frames, and the cut of a tracked path at its first invalid edge.
// Plain C++ without a HIP header, so that tests/native/cartesian_sanitize.cc compiles it on its own.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vmv
{
    constexpr uint64_t kCartMaxSegments = 0x7fffffffull;  // what `segments` reports at most

    struct CartLineSetup
    {
        double p0[3], dp[3], R0[9], axis[3], theta;  // R0 row-major
        uint64_t m;
    };

    // Axis and angle, theta in [0, pi], of the rotation R (row-major; orthonormal up to fp32 rounding).
    inline void cart_axis_angle(const double (&R)[9], double (&axis)[3], double &theta)
    {
        const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
        const double s = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
        theta = std::atan2(s, c);
        if (c >= -0.5)
        {
            if (s < 1e-12)
                axis[0] = 0.0, axis[1] = 0.0, axis[2] = 1.0;
            else
                for (int k = 0; k < 3; ++k) axis[k] = v[k] / s;
            return;
        }
        // near pi the skew part vanishes: 1/2 (R + R^T) = cos I + (1 - cos) a a^T holds the axis up to its sign
        const double ct = std::cos(theta);
        double S[9];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) S[3 * r + k] = 0.5 * (R[3 * r + k] + R[3 * k + r]) - (r == k ? ct : 0.0);
        int col = 0;
        for (int k = 1; k < 3; ++k)
            if (S[4 * k] > S[4 * col]) col = k;
        double a[3] = {S[col], S[3 + col], S[6 + col]};
        const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        const double sign = (a[0] * v[0] + a[1] * v[1] + a[2] * v[2]) < 0.0 ? -1.0 : 1.0;
        for (int k = 0; k < 3; ++k) axis[k] = len > 0.0 ? sign * a[k] / len : (k == 2 ? 1.0 : 0.0);
    }

    // The line from frame T0 to frame T1 (16 floats each, row-major 4 x 4, finite); the steps are positive and finite.
    inline CartLineSetup cart_line(const float *T0, const float *T1, double pos_step, double rot_step, bool position_only)
    {
        CartLineSetup L{};
        double R1[9], D[9];
        for (int r = 0; r < 3; ++r)
        {
            L.p0[r] = (double) T0[4 * r + 3];
            L.dp[r] = (double) T1[4 * r + 3] - L.p0[r];
            for (int k = 0; k < 3; ++k) L.R0[3 * r + k] = (double) T0[4 * r + k], R1[3 * r + k] = (double) T1[4 * r + k];
        }
        for (int r = 0; r < 3; ++r)  // D = R0^T R1
            for (int k = 0; k < 3; ++k) D[3 * r + k] = L.R0[r] * R1[k] + L.R0[3 + r] * R1[3 + k] + L.R0[6 + r] * R1[6 + k];
        cart_axis_angle(D, L.axis, L.theta);
        if (position_only) L.theta = 0.0;
        const double len = std::sqrt(L.dp[0] * L.dp[0] + L.dp[1] * L.dp[1] + L.dp[2] * L.dp[2]);
        const double need = std::fmax(1.0, std::fmax(std::ceil(len / pos_step), std::ceil(L.theta / rot_step)));
        L.m = need < (double) kCartMaxSegments ? (uint64_t) need : kCartMaxSegments;  // (the ratio may be huge; never NaN)
        return L;
    }

    // How many of the `tracked` edges [first, first + tracked) of a problem come before its first invalid one; bits: the
    // packed answers of vmv_validate_motion_batch_multi.
    inline uint32_t cart_cut(const uint64_t *bits, uint64_t first, uint32_t tracked)
    {
        for (uint32_t e = 0; e < tracked; ++e)
        {
            const uint64_t b = first + e;
            if (!((bits[b >> 6] >> (b & 63u)) & 1ull)) return e;
        }
        return tracked;
    }
}  // namespace vmv
