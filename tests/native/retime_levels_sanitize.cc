// Test program: the host steps of vmv_retime_multi_constrained that make no device call (vamp_mvt_amd/csrc/vmv_retime_path.h:
// the set-up with a level per corner, the two searches that place a sample, the blame rule of a failing pair) under
// AddressSanitizer + UBSan.  Built and run by tests/test_retime_levels_native.py (CPU only).
//
//   retime_levels_sanitize                 the checks below; prints OK
//   retime_levels_sanitize dump < input    the pieces of one levelled set-up as text, for the comparison with the serial
//                                          statement: input "dim count blend grid_step max_grid H", then `count` levels,
//                                          then count * dim waypoints as the hexadecimal bits of their floats
#include "../../vamp_mvt_amd/csrc/vmv_retime_path.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int fail(const char *what)
{
    std::printf("FAIL: %s\n", what);
    return 1;
}

static uint32_t bits_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

// the pieces tile the grid; a blend has its corner and the corner's half-length, a line has none; a corner without a
// blend makes the next piece begin with a stop
static int check(const vmv::RetimePath &P, const uint8_t *levels, uint32_t H, uint32_t max_grid)
{
    if (P.what != vmv::kRetimeOk) return P.pieces.empty() && P.corner.empty() ? 0 : fail("pieces without a set-up");
    if (P.corner.size() != P.pieces.size()) return fail("corner is not parallel to pieces");
    uint64_t grid = 0;
    uint32_t last_corner = 0;
    for (size_t a = 0; a < P.pieces.size(); ++a)
    {
        const vmv::RetimePiece &R = P.pieces[a];
        if (R.first != grid || R.n < 2) return fail("grid");
        if ((R.d > 0.f) != (P.corner[a] != 0)) return fail("a blend has a corner, a line has none");
        if (P.corner[a])
        {
            if (P.corner[a] <= last_corner || P.corner[a] + 1 >= P.kept.size()) return fail("corner order");
            if (levels && levels[P.corner[a]] > H) return fail("a stop corner has a blend");
            last_corner = P.corner[a];
        }
        grid += R.n;
    }
    if (grid != P.intervals || grid > max_grid) return fail("interval count");
    return 0;
}

static bool same_pieces(const vmv::RetimePath &A, const vmv::RetimePath &B)
{
    return A.what == B.what && A.intervals == B.intervals && A.distinct == B.distinct && A.pieces.size() == B.pieces.size() &&
           (A.pieces.empty() || std::memcmp(A.pieces.data(), B.pieces.data(), A.pieces.size() * sizeof(vmv::RetimePiece)) == 0);
}

static int dump()
{
    unsigned long dim, count, max_grid, H;
    double blend, grid_step;
    if (std::scanf("%lu %lu %lf %lf %lu %lu", &dim, &count, &blend, &grid_step, &max_grid, &H) != 6) return fail("header");
    std::vector<uint8_t> levels(count);  // exactly the bytes the call may read
    for (auto &l : levels)
    {
        unsigned v;
        if (std::scanf("%u", &v) != 1) return fail("levels");
        l = (uint8_t) v;
    }
    std::vector<float> w(count * dim);
    for (float &x : w)
    {
        uint32_t b;
        if (std::scanf("%" SCNx32, &b) != 1) return fail("waypoints");
        std::memcpy(&x, &b, 4);
    }
    const vmv::RetimePath P = vmv::retime_path(w.data(), count, dim, blend, grid_step, (uint32_t) max_grid, false, levels.data(), (uint32_t) H);
    std::printf("%d %u %" PRIu64 " %zu\n", (int) P.what, P.distinct, P.intervals, P.pieces.size());
    for (size_t a = 0; a < P.pieces.size(); ++a)
    {
        const vmv::RetimePiece &R = P.pieces[a];
        std::printf("%u %u %u %u %08x %08x", P.corner[a], R.n, R.first, R.stop, bits_of(R.d), bits_of(R.span));
        for (size_t j = 0; j < dim; ++j) std::printf(" %08x %08x %08x", bits_of(R.base[j]), bits_of(R.u_in[j]), bits_of(R.u_out[j]));
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "dump") == 0) return dump();
    std::mt19937 rng(31);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    const uint32_t H = 3;
    for (const size_t dim : {size_t{1}, size_t{7}, size_t{14}, size_t{16}})
        for (int rep = 0; rep < 200; ++rep)
        {
            const size_t count = (size_t) (rep % 9);  // 0, 1 and 2 waypoints among them
            std::vector<float> w(count * dim);         // exactly the floats the call owns
            for (float &x : w) x = u(rng);
            if (rep % 5 == 0 && count > 2)  // a duplicate waypoint
                for (size_t j = 0; j < dim; ++j) w[2 * dim + j] = w[dim + j];
            if (rep % 11 == 0 && count > 0) w[rng() % w.size()] = std::numeric_limits<float>::quiet_NaN();
            std::vector<uint8_t> levels(count);  // exactly `count` bytes
            for (auto &l : levels) l = (uint8_t) (rep % 4 == 0 ? 0 : rep % 4 == 1 ? H : rep % 4 == 2 ? H + 1 : rng() % (H + 2));
            const double blend = rep % 3 == 0 ? 5.0 : 0.1;  // (a blend above every L / 2: the blends abut, no line is left)
            const vmv::RetimePath P = vmv::retime_path(w.data(), count, dim, blend, 0.02, 4096, false, levels.data(), H);
            if (check(P, levels.data(), H, 4096)) return 1;
            if (rep % 11 == 0 && count > 0 && P.what != vmv::kRetimeNonFinite) return fail("NaN waypoint");
            if (rep % 4 == 0 && !same_pieces(P, vmv::retime_path(w.data(), count, dim, blend, 0.02, 4096, false)))
                return fail("levels 0 are not the plain set-up");
            if (rep % 4 == 2 && !same_pieces(P, vmv::retime_path(w.data(), count, dim, blend, 0.02, 4096, true)))
                return fail("levels H + 1 are not the set-up that stops at waypoints");
            if (rep % 4 == 1 && blend > 1.0 && P.what == vmv::kRetimeOk)  // level H of abutting blends: lines appear between them
                for (size_t a = 0; a < P.pieces.size(); ++a)
                    if (P.corner[a] && a + 1 < P.pieces.size() && P.corner[a + 1]) return fail("blends at level H still abut");
        }

    // abutting blends with no line between them: the middle edge is the shortest, both corners take half of it
    {
        const float w[8] = {0.f, 0.f, 1.f, 0.f, 1.f, 0.5f, 2.f, 0.5f};
        uint8_t levels[4] = {0, 0, 0, 0};
        const vmv::RetimePath P = vmv::retime_path(w, 4, 2, 5.0, 0.02, 4096, false, levels, H);
        if (check(P, levels, H, 4096) || P.pieces.size() != 4 || P.corner[1] != 1 || P.corner[2] != 2) return fail("abutting blends");
        levels[2] = 1;  // one of them halved: a line appears
        const vmv::RetimePath Q = vmv::retime_path(w, 4, 2, 5.0, 0.02, 4096, false, levels, H);
        if (check(Q, levels, H, 4096) || Q.pieces.size() != 5 || Q.corner[2] != 0 || Q.corner[3] != 2) return fail("a line between halved blends");
    }

    // exactly at and one over max_grid after a level change: halving a blend changes the interval count
    {
        const float w[6] = {0.f, 0.f, 1.f, 0.f, 1.f, 1.f};
        uint8_t levels[3] = {0, 0, 0};
        const uint64_t n0 = vmv::retime_path(w, 3, 2, 0.3, 0.023, 4096, false, levels, H).intervals;
        levels[1] = 1;
        const uint64_t n1 = vmv::retime_path(w, 3, 2, 0.3, 0.023, 4096, false, levels, H).intervals;
        if (n0 == n1) return fail("the level does not change the interval count");
        const vmv::RetimePath at = vmv::retime_path(w, 3, 2, 0.3, 0.023, (uint32_t) n1, false, levels, H);
        const vmv::RetimePath over = vmv::retime_path(w, 3, 2, 0.3, 0.023, (uint32_t) n1 - 1, false, levels, H);
        if (at.what != vmv::kRetimeOk || at.intervals != n1 || check(at, levels, H, (uint32_t) n1)) return fail("exactly at max_grid");
        if (over.what != vmv::kRetimeTooLong || over.intervals != n1 || !over.pieces.empty() || !over.corner.empty()) return fail("one over max_grid");
        const float d0 = vmv::retime_path(w, 3, 2, 0.3, 0.023, 4096, false).pieces[1].d;
        if (at.pieces[1].d != 0.5f * d0 || at.corner[1] != 1) return fail("level 1 halves the blend");
    }

    // the searches and the blame rule on a path line | blend | blend | line | small blend | line (the first two abut)
    {
        std::vector<vmv::RetimePiece> pc(6);
        const float d[6] = {0.f, 0.1f, 0.1f, 0.f, 0.0125f, 0.f};
        uint32_t first = 0;
        for (size_t a = 0; a < 6; ++a) pc[a].d = d[a], pc[a].n = 2, pc[a].first = first, first += 2;
        const uint32_t N = first;
        std::vector<float> T(N + 1);  // exactly N + 1 times
        for (uint32_t i = 0; i <= N; ++i) T[i] = 0.1f * (float) i;
        const float dt = 0.05f;
        const auto piece = [&](uint32_t k) { return vmv::retime_sample_piece(pc.data(), 6, T.data(), N, k, dt); };
        if (piece(0) != 0 || piece(3) != 0 || piece(4) != 1 || piece(23) != 5 || piece(24) != 5 || piece(1000) != 5) return fail("sample_piece");
        std::vector<uint32_t> marks(1, 0u);  // ceil(6 / 32) words
        if (vmv::retime_blame_pair(pc.data(), 0, 0, marks.data()) || marks[0]) return fail("a pair on a line blames nothing");
        if (!vmv::retime_blame_pair(pc.data(), 0, 1, marks.data()) || marks[0] != 2u) return fail("a pair that straddles a line and a blend");
        marks[0] = 0;
        if (!vmv::retime_blame_pair(pc.data(), 1, 2, marks.data()) || marks[0] != 6u) return fail("a pair that straddles two abutting blends");
        marks[0] = 0;
        if (!vmv::retime_blame_pair(pc.data(), 3, 5, marks.data()) || marks[0] != 16u) return fail("a pair that jumps over a whole small blend");
        marks[0] = 0;
        if (vmv::retime_blame_pair(pc.data(), 5, 5, marks.data()) || vmv::retime_blame_pair(pc.data(), 3, 3, marks.data()) || marks[0])
            return fail("lines only");
        uint32_t q;
        if (vmv::retime_blame_step(pc.data(), 4, 4, 1, q) || q != 5) return fail("a step past the range");
        std::vector<vmv::RetimePiece> many(65);  // the last bit of the last word
        for (size_t a = 0; a < 65; ++a) many[a].d = a == 64 ? 0.1f : 0.f;
        std::vector<uint32_t> wide(3, 0u);
        if (!vmv::retime_blame_pair(many.data(), 0, 64, wide.data()) || wide[0] || wide[1] || wide[2] != 1u) return fail("65 pieces");
    }
    std::printf("OK\n");
    return 0;
}
