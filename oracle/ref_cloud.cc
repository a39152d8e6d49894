// TEST INFRASTRUCTURE ONLY (oracle/_ref): thin extern "C" exports over the reference's point-cloud headers,
// compiled from where they lie (never copied): collision/mvt.hh, collision/capt.hh, collision/filter.hh and
// collision/filter_centervox.hh.  mvt.hh and filter_centervox.hh need only the standard library, vamp/vector.hh and
// collision/math.hh; capt.hh and filter.hh also name <pdqsort.h>, which oracle/shim/pdqsort.h supplies (our own
// text; -DREF_TIES_REVERSED builds the variant with the opposite order of equal keys).
//
// Nothing is caught here: where the reference throws (the noexcept MVT constructor, the centervox pools) the process
// terminates as the reference's would.  tools/make_cloud_golden.py runs those cases in a child process.
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include <vamp/vector.hh>
#include <vamp/collision/math.hh>
#include <vamp/collision/mvt.hh>
#include <vamp/collision/capt.hh>
#include <vamp/collision/filter.hh>
#include <vamp/collision/filter_centervox.hh>

using vamp::collision::CAPT;
using vamp::collision::MVT;
using vamp::collision::Point;
using V8 = vamp::FloatVector<>;
static_assert(V8::num_scalars == 8, "the rake exports assume 8 lanes");

namespace
{
    std::vector<Point> cloud(const float *xyz, std::size_t n)
    {
        std::vector<Point> pts(n);
        for (std::size_t i = 0; i < n; ++i) pts[i] = Point{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        return pts;
    }

    Point point(const float *p)
    {
        return Point{p[0], p[1], p[2]};
    }

    std::size_t put(const std::vector<Point> &pts, float *out)
    {
        for (std::size_t i = 0; i < pts.size(); ++i)
            for (int k = 0; k < 3; ++k) out[3 * i + k] = pts[i][k];
        return pts.size();
    }

    // spheres [m][8][4] (x y z r per lane) -> the four lane vectors of rake j
    void rake(const float *spheres, std::size_t j, std::array<V8, 3> &c, V8 &r)
    {
        alignas(32) float a[4][8];
        for (int l = 0; l < 8; ++l)
            for (int k = 0; k < 4; ++k) a[k][l] = spheres[(j * 8 + l) * 4 + k];
        c = {V8(a[0]), V8(a[1]), V8(a[2])};
        r = V8(a[3]);
    }
}  // namespace

extern "C"
{
    int ref_ties_reversed(void)
    {
#ifdef REF_TIES_REVERSED
        return 1;
#else
        return 0;
#endif
    }

    // ---- MVT (collision/mvt.hh) ----
    void *ref_mvt_create(const float *xyz, std::size_t n, float r_min, float r_max, const float *ws_min,
                         const float *ws_max, float r_point)
    {
        return new MVT(cloud(xyz, n), r_min, r_max, point(ws_min), point(ws_max), r_point);
    }
    void ref_mvt_destroy(void *h)
    {
        delete static_cast<MVT *>(h);
    }
    // u32[3] = grid_width, estimated_max_point_per_voxel, voxel_storage.size(); f32[7] = inverse_scale_factor, global box
    void ref_mvt_info(const void *h, uint32_t *u3, float *f7)
    {
        const auto *m = static_cast<const MVT *>(h);
        u3[0] = m->grid_width;
        u3[1] = static_cast<uint32_t>(m->estimated_max_point_per_voxel);
        u3[2] = static_cast<uint32_t>(m->voxel_storage.size());
        f7[0] = m->inverse_scale_factor;
        for (int k = 0; k < 3; ++k)
        {
            f7[1 + k] = m->global_aabb_min[k];
            f7[4 + k] = m->global_aabb_max[k];
        }
    }
    void ref_mvt_collides(const void *h, const float *spheres4, std::size_t n, uint8_t *out)
    {
        const auto *m = static_cast<const MVT *>(h);
        for (std::size_t i = 0; i < n; ++i) out[i] = m->collides(point(spheres4 + 4 * i), spheres4[4 * i + 3]);
    }
    void ref_mvt_collides_simd(const void *h, const float *spheres4, std::size_t n_rakes, uint8_t *out)
    {
        const auto *m = static_cast<const MVT *>(h);
        std::array<V8, 3> c;
        V8 r;
        for (std::size_t j = 0; j < n_rakes; ++j)
        {
            rake(spheres4, j, c, r);
            out[j] = m->collides_simd(c, r);
        }
    }

    // ---- CAPT (collision/capt.hh) ----
    void *ref_capt_create(const float *xyz, std::size_t n, float r_min, float r_max, float r_point)
    {
        return new CAPT(cloud(xyz, n), r_min, r_max, r_point);
    }
    void ref_capt_destroy(void *h)
    {
        delete static_cast<CAPT *>(h);
    }
    // u32[5] = nlog2, tests.size(), aff_starts.size(), aabbs.size(), affordances[0].size()
    void ref_capt_sizes(const void *h, uint32_t *u5)
    {
        const auto *c = static_cast<const CAPT *>(h);
        u5[0] = c->nlog2;
        u5[1] = static_cast<uint32_t>(c->tests.size());
        u5[2] = static_cast<uint32_t>(c->aff_starts.size());
        u5[3] = static_cast<uint32_t>(c->aabbs.size());
        u5[4] = static_cast<uint32_t>(c->affordances[0].size());
    }
    // raw bytes of tests, aff_starts, aabbs [leaves][6], the three affordance arrays [vectors][8] and the top box [6]
    void ref_capt_arrays(const void *h, float *tests, uint32_t *aff_starts, float *aabbs, float *ax, float *ay,
                         float *az, float *top6)
    {
        const auto *c = static_cast<const CAPT *>(h);
        std::memcpy(tests, c->tests.data(), c->tests.size() * sizeof(float));
        std::memcpy(aff_starts, c->aff_starts.data(), c->aff_starts.size() * sizeof(uint32_t));
        static_assert(sizeof(vamp::collision::Volume) == 6 * sizeof(float), "Volume is two Points");
        std::memcpy(aabbs, c->aabbs.data(), c->aabbs.size() * 6 * sizeof(float));
        float *dst[3] = {ax, ay, az};
        alignas(32) float lanes[8];
        for (int k = 0; k < 3; ++k)
            for (std::size_t i = 0; i < c->affordances[k].size(); ++i)
            {
                c->affordances[k][i].to_array(lanes);
                std::memcpy(dst[k] + 8 * i, lanes, sizeof(lanes));
            }
        std::memcpy(top6, &c->aabb_top, 6 * sizeof(float));
    }
    void ref_capt_collides(const void *h, const float *spheres4, std::size_t n, uint8_t *out)
    {
        const auto *c = static_cast<const CAPT *>(h);
        for (std::size_t i = 0; i < n; ++i) out[i] = c->collides(point(spheres4 + 4 * i), spheres4[4 * i + 3]);
    }
    void ref_capt_collides_simd(const void *h, const float *spheres4, std::size_t n_rakes, uint8_t *out)
    {
        const auto *t = static_cast<const CAPT *>(h);
        std::array<V8, 3> c;
        V8 r;
        for (std::size_t j = 0; j < n_rakes; ++j)
        {
            rake(spheres4, j, c, r);
            out[j] = t->collides_simd(c, r);
        }
    }

    // ---- filters (collision/filter.hh, collision/filter_centervox.hh) over std::vector<Point>; out holds n points ----
    std::size_t ref_filter_scdf(const float *xyz, std::size_t n, float min_dist, float max_range, const float *origin,
                                const float *ws_min, const float *ws_max, int cull, float *out)
    {
        return put(vamp::collision::filter_pointcloud(cloud(xyz, n), min_dist, max_range, point(origin), point(ws_min),
                                                      point(ws_max), cull != 0), out);
    }
    std::size_t ref_filter_centervox(const float *xyz, std::size_t n, float voxel_size, float max_range,
                                     const float *origin, const float *ws_min, const float *ws_max, float *out)
    {
        return put(vamp::collision::filter_pointcloud_centervox(cloud(xyz, n), voxel_size, max_range, point(origin),
                                                                point(ws_min), point(ws_max)), out);
    }
}
