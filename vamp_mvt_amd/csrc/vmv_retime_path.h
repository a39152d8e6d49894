// vmv_retime_path.h — the host steps of vmv_retime_multi that make no device call (include/vamp_mvt_amd.h):
// the float64 set-up of a blended path from fp32 waypoints (its pieces, their grid) and the sample count of a duration.
// For vmv_retime_multi_constrained the set-up takes a level per corner, and the two searches that place a
// sample on the grid and the blame rule of one failing sample pair stand here as host-and-device functions, so that
// retime_blame_kernel and a host program run the same text.
// Plain C++ without a HIP header, so that tests/native/retime_sanitize.cc compiles it on its own.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VMV_RETIME_HD __host__ __device__
#else
#define VMV_RETIME_HD
#endif

namespace vmv
{
    constexpr uint32_t kRetimeMaxDim = 16;
    constexpr uint32_t kRetimeMaxGrid = 4096;        // the cap of max_grid: K of a whole path fits the profile kernel's LDS
    constexpr double kRetimeMinSpan = 1e-9;          // a line that is not longer is left out
    constexpr uint32_t kRetimeMinIntervals = 2;      // per piece: a stretch between two stops needs an inner grid point

    // One piece of the blended path as the kernels read it (fp32): q(s) = base + u_in s + 1/2 q'' s^2 for s in [0, span],
    // q'' = (u_out - u_in) / (2 d) on a blend (d > 0) and 0 on a line (d == 0, u_in == u_out).
    struct RetimePiece
    {
        float base[kRetimeMaxDim], u_in[kRetimeMaxDim], u_out[kRetimeMaxDim];
        float d, span;
        uint32_t n;      // equal intervals of the piece, at least 2
        uint32_t first;  // grid index of its first point within the path
        uint32_t stop;   // 1: its first point is a stop point
        uint32_t pad;
    };
    static_assert(sizeof(RetimePiece) == 216, "48 floats, d, span, n, first, stop, pad");

    enum RetimeSetup
    {
        kRetimeOk = 0,       // pieces and intervals are set
        kRetimeTrivial = 1,  // fewer than two distinct waypoints, or no piece: `distinct` says how many samples (0 or 1)
        kRetimeTooLong = 2,  // more than max_grid intervals: `intervals` is set, no pieces
        kRetimeNonFinite = 3
    };

    struct RetimePath
    {
        RetimeSetup what = kRetimeTrivial;
        uint32_t distinct = 0;   // distinct waypoints
        uint64_t intervals = 0;  // N
        std::vector<RetimePiece> pieces;
        std::vector<uint32_t> corner;  // per piece: the distinct waypoint a blend rounds; 0 for a line
        std::vector<uint32_t> kept;    // per distinct waypoint: its index among the input waypoints
    };

    constexpr uint32_t kRetimeMaxHalvings = 8;  // the cap of blend_halvings

    // waypoints [count][dim] (fp32, any values); blend, grid_step positive and finite; dim <= 16.
    // levels (may be nullptr: every corner at level 0, or a stop with stop_at_waypoints): one byte per DISTINCT waypoint,
    // so `count` bytes always suffice; corner i has the half-length min(blend, L_{i-1} / 2, L_i / 2) * 2^-levels[i] up to
    // level `halvings` (the scaling is exact) and 0, a stop, above it.  With levels, stop_at_waypoints is not looked at.
    inline RetimePath retime_path(const float *waypoints, size_t count, size_t dim, double blend, double grid_step,
                                  uint32_t max_grid, bool stop_at_waypoints, const uint8_t *levels, uint32_t halvings)
    {
        RetimePath P;
        for (size_t k = 0; k < count * dim; ++k)
            if (!std::isfinite(waypoints[k]))
            {
                P.what = kRetimeNonFinite;
                return P;
            }
        std::vector<size_t> keep;  // a waypoint equal to its predecessor is dropped
        for (size_t i = 0; i < count; ++i)
        {
            bool same = !keep.empty();
            for (size_t j = 0; same && j < dim; ++j) same = waypoints[i * dim + j] == waypoints[keep.back() * dim + j];
            if (!same) keep.push_back(i);
        }
        const size_t m = keep.size();
        P.distinct = (uint32_t) (m < 2 ? m : 2);
        P.kept.assign(keep.begin(), keep.end());
        if (m < 2) return P;

        const size_t edges = m - 1;
        std::vector<double> L(edges), u(edges * dim), d(m, 0.0);
        for (size_t e = 0; e < edges; ++e)
        {
            const float *a = waypoints + keep[e] * dim, *b = waypoints + keep[e + 1] * dim;
            double sum = 0.0;
            for (size_t j = 0; j < dim; ++j)
            {
                const double diff = (double) b[j] - (double) a[j];
                u[e * dim + j] = diff;
                sum += diff * diff;
            }
            L[e] = std::sqrt(sum);
            for (size_t j = 0; j < dim; ++j) u[e * dim + j] /= L[e];
        }
        if (levels)
        {
            for (size_t i = 1; i + 1 < m; ++i)
                if (levels[i] <= halvings) d[i] = std::ldexp(std::fmin(blend, std::fmin(0.5 * L[i - 1], 0.5 * L[i])), -(int) levels[i]);
        }
        else if (!stop_at_waypoints)
            for (size_t i = 1; i + 1 < m; ++i) d[i] = std::fmin(blend, std::fmin(0.5 * L[i - 1], 0.5 * L[i]));

        uint64_t grid = 0;
        bool stop_next = true;  // the first grid point is a stop point
        const auto add = [&](const double *base, const double *uin, const double *uout, double half, double span, size_t corner) {
            RetimePiece R{};
            for (size_t j = 0; j < dim; ++j) R.base[j] = (float) base[j], R.u_in[j] = (float) uin[j], R.u_out[j] = (float) uout[j];
            R.d = (float) half, R.span = (float) span;
            const double need = std::ceil(span / grid_step);
            const uint64_t n = need < (double) kRetimeMinIntervals ? kRetimeMinIntervals :
                               need < 4294967295.0 ? (uint64_t) need : 4294967295ull;  // (the quotient may be huge; never NaN)
            R.n = (uint32_t) n, R.first = (uint32_t) (grid < 4294967295ull ? grid : 4294967295ull), R.stop = stop_next ? 1u : 0u;
            grid += n, stop_next = false;
            if (grid <= max_grid) P.pieces.push_back(R), P.corner.push_back((uint32_t) corner);
        };
        std::vector<double> base(dim);
        for (size_t e = 0; e < edges; ++e)
        {
            const double *ue = u.data() + e * dim;
            const float *w = waypoints + keep[e] * dim, *w1 = waypoints + keep[e + 1] * dim;
            const double span = L[e] - d[e] - d[e + 1];
            if (span > kRetimeMinSpan)
            {
                for (size_t j = 0; j < dim; ++j) base[j] = (double) w[j] + d[e] * ue[j];
                add(base.data(), ue, ue, 0.0, span, 0);
            }
            if (e + 1 < edges)
            {
                if (d[e + 1] > 0.0)
                {
                    for (size_t j = 0; j < dim; ++j) base[j] = (double) w1[j] - d[e + 1] * ue[j];
                    add(base.data(), ue, ue + dim, d[e + 1], 2.0 * d[e + 1], e + 1);
                }
                else
                    stop_next = true;  // a corner without a blend
            }
        }
        P.intervals = grid;
        if (grid > max_grid)
        {
            P.what = kRetimeTooLong;
            P.pieces.clear(), P.corner.clear();
            return P;
        }
        if (P.pieces.empty())  // every line at most 1e-9 long and no blend: the path is its first waypoint
        {
            P.distinct = 1;
            return P;
        }
        P.what = kRetimeOk;
        return P;
    }

    inline RetimePath retime_path(const float *waypoints, size_t count, size_t dim, double blend, double grid_step,
                                  uint32_t max_grid, bool stop_at_waypoints)
    {
        return retime_path(waypoints, count, dim, blend, grid_step, max_grid, stop_at_waypoints, nullptr, 0u);
    }

    // samples of a trajectory of duration T sampled every dt (both fp32 values, T >= 0 finite, dt > 0): ceil(T / dt) + 1 in
    // float64, saturated at 2^32 - 1
    inline uint64_t retime_samples(float T, float dt)
    {
        const double need = std::ceil((double) T / (double) dt) + 1.0;
        return need < 4294967295.0 ? (uint64_t) need : 4294967295ull;
    }

    // The first invalid edge [first, first + edges) of a path among the packed answers of vmv_validate_motion_batch_multi,
    // or `none`.
    inline uint32_t retime_first_invalid(const uint64_t *bits, uint64_t first, uint32_t edges, uint32_t none)
    {
        for (uint32_t e = 0; e < edges; ++e)
        {
            const uint64_t b = first + e;
            if (!((bits[b >> 6] >> (b & 63u)) & 1ull)) return e;
        }
        return none;
    }

    // ---- vmv_retime_multi_constrained: where a sample lies, and what a failing sample pair blames ---------------------
    // The time of sample k and the two searches of retime_sample_kernel (vmv_retime_multi.hip), which keeps its own text
    // because its code is not to change: the two must STAY word for word, or piece(k) differs from the piece the sample
    // was evaluated on.  T [N + 1] the grid times of the path, pieces [n_pieces] its records.  -> the piece of sample k.
    VMV_RETIME_HD inline uint32_t retime_sample_piece(const RetimePiece *pieces, uint32_t n_pieces, const float *T, uint32_t N,
                                                      uint32_t k, float dt)
    {
        const float t = fminf((float) k * dt, T[N]);
        uint32_t i = 0u, hi = N - 1u;  // the last interval that starts at or before t
        while (i < hi)
        {
            const uint32_t mid = (i + hi + 1u) >> 1;
            if (T[mid] <= t) i = mid;
            else hi = mid - 1u;
        }
        uint32_t a = 0u;  // its piece
        hi = n_pieces - 1u;
        while (a < hi)
        {
            const uint32_t mid = (a + hi + 1u) >> 1;
            if (pieces[mid].first <= i) a = mid;
            else hi = mid - 1u;
        }
        return a;
    }

    // The blame rule.  A failing pair whose samples lie on the pieces pa <= pb blames every blend piece in [pa, pb]; this
    // is step r of the walk over that range: -> true where piece pa + r is in the range and is a blend (`piece` is set to
    // it either way).  The steps r = 0 .. pb - pa make the whole rule; retime_blame_kernel runs them in a loop whose trip
    // count is the wave's largest range, a host program in retime_blame_pair below.
    VMV_RETIME_HD inline bool retime_blame_step(const RetimePiece *pieces, uint32_t pa, uint32_t pb, uint32_t r, uint32_t &piece)
    {
        piece = pa + r;
        return piece <= pb && pieces[piece].d > 0.0f;
    }

    // marks [ceil(n_pieces / 32)] words, one bit per piece, ORed into.  -> whether the pair blames any blend.
    inline bool retime_blame_pair(const RetimePiece *pieces, uint32_t pa, uint32_t pb, uint32_t *marks)
    {
        bool any = false;
        for (uint32_t r = 0; pa + r <= pb; ++r)
        {
            uint32_t piece;
            if (retime_blame_step(pieces, pa, pb, r, piece)) marks[piece >> 5] |= 1u << (piece & 31u), any = true;
        }
        return any;
    }
}  // namespace vmv
