// Test program: the host steps of vmv_cartesian_multi that make no device call (vamp_mvt_amd/csrc/vmv_cartesian_line.h:
// the float64 line set-up and the cut) under AddressSanitizer + UBSan.  Built and run by tests/test_cartesian.py (CPU only).
#include "../../vamp_mvt_amd/csrc/vmv_cartesian_line.h"

#include <cstdio>
#include <limits>
#include <random>
#include <vector>

static int fail(const char *what)
{
    std::printf("FAIL: %s\n", what);
    return 1;
}

static void rodrigues(const double (&a)[3], double t, double (&R)[9])
{
    const double c = std::cos(t), s = std::sin(t), v = 1.0 - c;
    R[0] = c + v * a[0] * a[0], R[1] = v * a[0] * a[1] - s * a[2], R[2] = v * a[0] * a[2] + s * a[1];
    R[3] = v * a[1] * a[0] + s * a[2], R[4] = c + v * a[1] * a[1], R[5] = v * a[1] * a[2] - s * a[0];
    R[6] = v * a[2] * a[0] - s * a[1], R[7] = v * a[2] * a[1] + s * a[0], R[8] = c + v * a[2] * a[2];
}

static void frame(const double (&R)[9], const double (&p)[3], float *T)
{
    for (int r = 0; r < 3; ++r)
    {
        for (int k = 0; k < 3; ++k) T[4 * r + k] = (float) R[3 * r + k];
        T[4 * r + 3] = (float) p[r];
    }
    T[12] = T[13] = T[14] = 0.f, T[15] = 1.f;
}

int main()
{
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    const double pi = 3.14159265358979323846;
    // axis and angle round trip, the angles at both ends included
    for (const double t : {0.0, 1e-4, 0.3, 1.0, 2.0, 2.2, 3.0, 3.14, pi})
        for (int rep = 0; rep < 50; ++rep)
        {
            double a[3] = {u(rng), u(rng), u(rng)}, R[9], b[3], got = -1.0;
            const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            if (len < 0.1) continue;
            for (double &x : a) x /= len;
            rodrigues(a, t, R);
            vmv::cart_axis_angle(R, b, got);
            if (std::fabs(got - t) > 1e-7) return fail("angle");
            double dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
            if (t == pi) dot = std::fabs(dot);  // (either sign is the same rotation)
            if (t > 0.0 && dot < 1.0 - 1e-6) return fail("axis");
            if (std::fabs(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] - 1.0) > 1e-12) return fail("unit axis");
        }
    // lines: segment counts, huge quotients, a target equal to the start
    for (int rep = 0; rep < 200; ++rep)
    {
        double a[3] = {0.0, 0.6, 0.8}, R0[9], R1[9], p0[3] = {u(rng), u(rng), u(rng)}, p1[3] = {u(rng), u(rng), u(rng)};
        rodrigues(a, u(rng) * 3.0, R0);
        rodrigues(a, u(rng) * 3.0, R1);
        float T0[16], T1[16];
        frame(R0, p0, T0), frame(R1, p1, T1);
        const vmv::CartLineSetup L = vmv::cart_line(T0, T1, 0.01, 0.05, rep % 2 == 1);
        const double len = std::sqrt(L.dp[0] * L.dp[0] + L.dp[1] * L.dp[1] + L.dp[2] * L.dp[2]);
        if (L.m < 1 || (double) L.m < len / 0.01 || (double) L.m < L.theta / 0.05) return fail("too few segments");
        if ((double) L.m >= len / 0.01 + 1.0 && (double) L.m >= L.theta / 0.05 + 1.0 && L.m > 1) return fail("too many segments");
        if (rep % 2 == 1 && L.theta != 0.0) return fail("position_only");
        const vmv::CartLineSetup same = vmv::cart_line(T0, T0, 0.01, 0.05, false);
        if (same.m != 1 || same.theta > 1e-6) return fail("a line to the start's own frame");
        const vmv::CartLineSetup tiny = vmv::cart_line(T0, T1, std::numeric_limits<double>::denorm_min(), 0.05, false);
        if (tiny.m != vmv::kCartMaxSegments && len > 0.0) return fail("a huge quotient");
    }
    // the cut: every position of the first invalid edge, across word boundaries
    for (const uint32_t tracked : {0u, 1u, 63u, 64u, 65u, 200u})
        for (const uint64_t first : {uint64_t{0}, uint64_t{1}, uint64_t{63}, uint64_t{64}, uint64_t{130}})
        {
            const size_t words = (first + tracked + 63) / 64;
            for (uint32_t bad = 0; bad <= tracked; ++bad)
            {
                std::vector<uint64_t> bits(words, ~uint64_t{0});  // exactly the words the call owns
                if (bad < tracked) bits[(first + bad) >> 6] &= ~(uint64_t{1} << ((first + bad) & 63u));
                if (vmv::cart_cut(bits.data(), first, tracked) != bad) return fail("cut");
            }
        }
    std::printf("OK\n");
    return 0;
}
