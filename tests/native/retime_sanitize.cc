// Test program: the host steps of vmv_retime_multi that make no device call (vamp_mvt_amd/csrc/vmv_retime_path.h: the
// float64 set-up of a blended path, the sample count, the first invalid edge) under AddressSanitizer + UBSan.  Built and
// run by tests/test_retime.py (CPU only).
#include "../../vamp_mvt_amd/csrc/vmv_retime_path.h"

#include <cstdio>
#include <limits>
#include <random>
#include <vector>

static int fail(const char *what)
{
    std::printf("FAIL: %s\n", what);
    return 1;
}

// the pieces tile the grid, every piece has at least two intervals, tangents are unit vectors, and consecutive pieces
// meet in position and tangent unless a stop point lies between them
static int check(const vmv::RetimePath &P, size_t dim, uint32_t max_grid)
{
    if (P.what != vmv::kRetimeOk) return 0;
    uint64_t grid = 0;
    for (size_t a = 0; a < P.pieces.size(); ++a)
    {
        const vmv::RetimePiece &R = P.pieces[a];
        if (R.first != grid) return fail("first grid index");
        if (R.n < 2) return fail("fewer than two intervals");
        if (!(R.span > 0.f) || !(R.d >= 0.f)) return fail("span or d");
        if (a == 0 && !R.stop) return fail("the first point is a stop point");
        double in = 0.0, out = 0.0;
        for (size_t j = 0; j < dim; ++j) in += (double) R.u_in[j] * R.u_in[j], out += (double) R.u_out[j] * R.u_out[j];
        if (std::fabs(in - 1.0) > 1e-5 || std::fabs(out - 1.0) > 1e-5) return fail("unit tangents");
        if (a + 1 < P.pieces.size() && !P.pieces[a + 1].stop)
            for (size_t j = 0; j < dim; ++j)
            {
                const double c = R.d > 0.f ? ((double) R.u_out[j] - R.u_in[j]) / (2.0 * R.d) : 0.0;
                const double end = R.base[j] + R.u_in[j] * (double) R.span + 0.5 * c * (double) R.span * R.span;
                if (std::fabs(end - P.pieces[a + 1].base[j]) > 1e-5) return fail("pieces do not meet");
                if (std::fabs((double) R.u_out[j] - P.pieces[a + 1].u_in[j]) > 1e-6) return fail("tangents do not meet");
            }
        grid += R.n;
    }
    if (grid != P.intervals || grid > max_grid) return fail("interval count");
    return 0;
}

int main()
{
    std::mt19937 rng(26);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    for (const size_t dim : {size_t{1}, size_t{6}, size_t{7}, size_t{14}, size_t{16}})
        for (int rep = 0; rep < 200; ++rep)
        {
            const size_t count = (size_t) (rep % 9);
            std::vector<float> w(count * dim);  // exactly the floats the call owns
            for (float &x : w) x = u(rng);
            if (rep % 5 == 0 && count > 2)  // a duplicate waypoint
                for (size_t j = 0; j < dim; ++j) w[2 * dim + j] = w[dim + j];
            const bool stop = rep % 3 == 0;
            const double blend = rep % 4 == 0 ? 5.0 : 0.1;  // (a blend above every L / 2: no line is left)
            const vmv::RetimePath P = vmv::retime_path(w.data(), count, dim, blend, 0.02, 4096, stop);
            const bool trivial = count < 2;
            if (trivial != (P.what == vmv::kRetimeTrivial)) return fail("trivial");
            if (trivial && P.distinct != count) return fail("distinct");
            if (int rc = check(P, dim, 4096)) return rc;
            if (stop && P.what == vmv::kRetimeOk)
                for (const vmv::RetimePiece &R : P.pieces)
                    if (R.d != 0.f || !R.stop) return fail("stop_at_waypoints leaves a blend or a corner without a stop");
            const vmv::RetimePath capped = vmv::retime_path(w.data(), count, dim, blend, 0.02, 3, stop);
            if (!trivial && capped.what != vmv::kRetimeTooLong && capped.intervals > 3) return fail("max_grid");
            if (capped.what == vmv::kRetimeTooLong && (!capped.pieces.empty() || capped.intervals <= 3)) return fail("too_long");
            // a huge quotient: the interval count saturates, nothing overflows
            const vmv::RetimePath huge = vmv::retime_path(w.data(), count, dim, blend, std::numeric_limits<double>::denorm_min(), 4096, stop);
            if (!trivial && huge.what != vmv::kRetimeTooLong) return fail("a huge quotient");
            if (count)
            {
                std::vector<float> bad(w);
                bad[(size_t) rep % bad.size()] = rep % 2 ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity();
                if (vmv::retime_path(bad.data(), count, dim, blend, 0.02, 4096, stop).what != vmv::kRetimeNonFinite) return fail("non-finite");
            }
        }
    {
        // all waypoints equal; a 1 mm line (two intervals between two stops); lines at most 1e-9 long
        const float same[6] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f};
        const vmv::RetimePath one = vmv::retime_path(same, 3, 2, 0.1, 0.02, 4096, false);
        if (one.what != vmv::kRetimeTrivial || one.distinct != 1) return fail("equal waypoints");
        const float mm[2] = {0.f, 0.001f};
        const vmv::RetimePath line = vmv::retime_path(mm, 2, 1, 0.1, 0.02, 4096, false);
        if (line.what != vmv::kRetimeOk || line.intervals != 2 || line.pieces.size() != 1) return fail("1 mm line");
        const float tiny[2] = {0.f, 1e-12f};
        const vmv::RetimePath none = vmv::retime_path(tiny, 2, 1, 0.1, 0.02, 4096, true);
        if (none.what != vmv::kRetimeTrivial || none.distinct != 1) return fail("a line below 1e-9");
        if (vmv::retime_path(nullptr, 0, 7, 0.1, 0.02, 4096, false).distinct != 0) return fail("no waypoints");
    }
    if (vmv::retime_samples(0.f, 0.01f) != 1 || vmv::retime_samples(1.f, 0.5f) != 3 || vmv::retime_samples(1.01f, 0.5f) != 4) return fail("samples");
    if (vmv::retime_samples(3e38f, 1e-6f) != 4294967295ull) return fail("samples saturate");
    for (const uint32_t edges : {0u, 1u, 63u, 64u, 65u, 200u})
        for (const uint64_t first : {uint64_t{0}, uint64_t{1}, uint64_t{63}, uint64_t{64}, uint64_t{130}})
        {
            const size_t words = (first + edges + 63) / 64;
            for (uint32_t bad = 0; bad <= edges; ++bad)
            {
                std::vector<uint64_t> bits(words, ~uint64_t{0});  // exactly the words the call owns
                if (bad < edges) bits[(first + bad) >> 6] &= ~(uint64_t{1} << ((first + bad) & 63u));
                if (vmv::retime_first_invalid(bits.data(), first, edges, 0xffffffffu) != (bad < edges ? bad : 0xffffffffu)) return fail("first invalid");
            }
        }
    std::printf("OK\n");
    return 0;
}
