// TEST INFRASTRUCTURE ONLY (oracle/_ref): thin extern "C" exports over the reference's primitive narrow phase and
// environment loop, compiled from where they lie (never copied): collision/validity.hh, which brings in shapes.hh,
// environment.hh, attachments.hh and the sphere_*.hh predicates.  environment.hh and attachments.hh name
// <Eigen/Dense> and <Eigen/Geometry>; oracle/shim/Eigen supplies stand-ins of our own text whose members are never
// called (no Attachment is ever constructed here, so attachments and fkcc_attach stay outside these pins).
//
// Three answers per query (a sphere broadcast to the 8 lanes, or a rake of 8 distinct spheres):
//   ref      vamp::sphere_environment_in_collision on Environment<FloatVector<8>>, as compiled
//   nobreak  the OR over EVERY primitive of the reference's own predicate, with no sorted early break
//   exact    the loop of collision/validity.hh:47-158 restated below in our own text: the reference's predicates and
//            the reference's min_distance, but max_extent from the correctly rounded sqrtf instead of the vector
//            type's v * rsqrt(v) (the one deliberate deviation, written once next to the reference)
// Lists follow bindings/environment.cc:111-151: z-aligned cuboid iff axis_3_z == 1, z-aligned capsule iff
// xv == 0 and yv == 0, sort() after every insertion; a heightfield is HeightField<float>(c, 1 / scale, xd, yd, data),
// which is what collision/factory.hh:365-386 builds.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include <vamp/vector.hh>
#include <vamp/collision/validity.hh>

namespace vc = vamp::collision;
using V8 = vamp::FloatVector<8>;
static_assert(V8::num_scalars == 8, "the rake exports assume 8 lanes");

namespace
{
    struct Env
    {
        vc::Environment<float> f;
        vc::Environment<V8> v;
        bool stale = true;

        const vc::Environment<V8> &vec()
        {
            if (stale)
            {
                v = vc::Environment<V8>(f);
                stale = false;
            }
            return v;
        }
    };

    struct Query
    {
        V8 x, y, z, r;
    };

    // spheres [..][4] = x y z r: one sphere on all lanes, or the 8 spheres of rake j
    Query broadcast(const float *s) { return {V8(s[0]), V8(s[1]), V8(s[2]), V8(s[3])}; }
    Query rake(const float *spheres, std::size_t j)
    {
        alignas(32) float a[4][8];
        for (int l = 0; l < 8; ++l)
            for (int k = 0; k < 4; ++k) a[k][l] = spheres[(j * 8 + l) * 4 + k];
        return {V8(a[0]), V8(a[1]), V8(a[2]), V8(a[3])};
    }

    bool hit(const V8 &v) { return not v.test_zero(); }

    bool nobreak(const vc::Environment<V8> &e, const Query &q)
    {
        const V8 rsq = q.r * q.r;
        bool any = false;
        for (const auto &s : e.spheres) any |= hit(vc::sphere_sphere_sql2(s, q.x, q.y, q.z, q.r));
        for (const auto &c : e.capsules) any |= hit(vc::sphere_capsule(c, q.x, q.y, q.z, q.r));
        for (const auto &c : e.z_aligned_capsules) any |= hit(vc::sphere_z_aligned_capsule(c, q.x, q.y, q.z, q.r));
        for (const auto &c : e.cuboids) any |= hit(vc::sphere_cuboid(c, q.x, q.y, q.z, rsq));
        for (const auto &c : e.z_aligned_cuboids) any |= hit(vc::sphere_z_aligned_cuboid(c, q.x, q.y, q.z, rsq));
        for (const auto &h : e.heightfields) any |= hit(vc::sphere_heightfield(h, q.x, q.y, q.z, q.r));
        return any;
    }

    // our own restatement of the sorted loop; the break is the reference's (no lane of min_distance - max_extent has
    // its sign bit set), max_extent is not
    template <typename List, typename Test>
    bool sorted_list_hits(const List &list, const V8 &max_extent, Test test)
    {
        for (const auto &p : list)
        {
            if ((p.min_distance - max_extent).test_zero()) break;
            if (hit(test(p))) return true;
        }
        return false;
    }

    bool exact(const vc::Environment<V8> &e, const Query &q)
    {
        alignas(32) float sq[8];
        vc::dot_3(q.x, q.y, q.z, q.x, q.y, q.z).to_array(sq);
        for (float &v : sq) v = std::sqrt(v);
        const V8 max_extent = V8(sq) + q.r;
        const V8 rsq = q.r * q.r;
        if (sorted_list_hits(e.spheres, max_extent,
                             [&](const auto &p) { return vc::sphere_sphere_sql2(p, q.x, q.y, q.z, q.r); }))
            return true;
        if (sorted_list_hits(e.capsules, max_extent, [&](const auto &p) { return vc::sphere_capsule(p, q.x, q.y, q.z, q.r); }))
            return true;
        if (sorted_list_hits(e.z_aligned_capsules, max_extent,
                             [&](const auto &p) { return vc::sphere_z_aligned_capsule(p, q.x, q.y, q.z, q.r); }))
            return true;
        if (sorted_list_hits(e.cuboids, max_extent, [&](const auto &p) { return vc::sphere_cuboid(p, q.x, q.y, q.z, rsq); }))
            return true;
        if (sorted_list_hits(e.z_aligned_cuboids, max_extent,
                             [&](const auto &p) { return vc::sphere_z_aligned_cuboid(p, q.x, q.y, q.z, rsq); }))
            return true;
        for (const auto &h : e.heightfields)
            if (hit(vc::sphere_heightfield(h, q.x, q.y, q.z, q.r))) return true;
        return false;
    }

    void answer(Env *env, const Query &q, uint8_t *out3)
    {
        const auto &e = env->vec();
        out3[0] = vamp::sphere_environment_in_collision(e, q.x, q.y, q.z, q.r);
        out3[1] = nobreak(e, q);
        out3[2] = exact(e, q);
    }

    float lane0(const V8 &v)
    {
        alignas(32) float a[8];
        v.to_array(a);
        return a[0];
    }
}  // namespace

extern "C"
{
    void *ref_env_create(void) { return new Env; }
    void ref_env_destroy(void *h) { delete static_cast<Env *>(h); }

    void ref_env_add_sphere(void *h, float x, float y, float z, float r)
    {
        auto *e = static_cast<Env *>(h);
        e->f.spheres.emplace_back(vc::Sphere<float>(x, y, z, r));
        e->f.sort();
        e->stale = true;
    }
    void ref_env_add_cuboid(void *h, const float *p)
    {
        auto *e = static_cast<Env *>(h);
        vc::Cuboid<float> c(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14]);
        (c.axis_3_z == 1. ? e->f.z_aligned_cuboids : e->f.cuboids).emplace_back(c);
        e->f.sort();
        e->stale = true;
    }
    void ref_env_add_capsule(void *h, const float *p)
    {
        auto *e = static_cast<Env *>(h);
        vc::Cylinder<float> c(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
        ((c.xv == 0. and c.yv == 0.) ? e->f.z_aligned_capsules : e->f.capsules).emplace_back(c);
        e->f.sort();
        e->stale = true;
    }
    void ref_env_add_heightfield(void *h, const float *c, const float *scale, std::size_t xd, std::size_t yd, const float *data)
    {
        auto *e = static_cast<Env *>(h);
        e->f.heightfields.emplace_back(vc::HeightField<float>(c[0], c[1], c[2], 1.F / scale[0], 1.F / scale[1], 1.F / scale[2],
                                                              xd, yd, std::vector<float>(data, data + xd * yd)));
        e->f.sort();
        e->stale = true;
    }

    // spheres, capsules, z-aligned capsules, cuboids, z-aligned cuboids, heightfields
    void ref_env_counts(const void *h, std::size_t *n6)
    {
        const auto &f = static_cast<const Env *>(h)->f;
        n6[0] = f.spheres.size();
        n6[1] = f.capsules.size();
        n6[2] = f.z_aligned_capsules.size();
        n6[3] = f.cuboids.size();
        n6[4] = f.z_aligned_cuboids.size();
        n6[5] = f.heightfields.size();
    }
    // the sorted lists: x y z r min_distance | 15 parameters + min_distance | 8 parameters + min_distance
    void ref_env_get_spheres(const void *h, float *out5)
    {
        for (const auto &s : static_cast<const Env *>(h)->f.spheres)
        {
            const float row[5] = {s.x, s.y, s.z, s.r, s.min_distance};
            std::memcpy(out5, row, sizeof(row));
            out5 += 5;
        }
    }
    void ref_env_get_cuboids(const void *h, int z_aligned, float *out16)
    {
        const auto &f = static_cast<const Env *>(h)->f;
        for (const auto &c : z_aligned ? f.z_aligned_cuboids : f.cuboids)
        {
            const float row[16] = {c.x,        c.y,        c.z,        c.axis_1_x, c.axis_1_y, c.axis_1_z, c.axis_2_x, c.axis_2_y,
                                   c.axis_2_z, c.axis_3_x, c.axis_3_y, c.axis_3_z, c.axis_1_r, c.axis_2_r, c.axis_3_r, c.min_distance};
            std::memcpy(out16, row, sizeof(row));
            out16 += 16;
        }
    }
    void ref_env_get_capsules(const void *h, int z_aligned, float *out9)
    {
        const auto &f = static_cast<const Env *>(h)->f;
        for (const auto &c : z_aligned ? f.z_aligned_capsules : f.capsules)
        {
            const float row[9] = {c.x1, c.y1, c.z1, c.xv, c.yv, c.zv, c.r, c.rdv, c.min_distance};
            std::memcpy(out9, row, sizeof(row));
            out9 += 9;
        }
    }

    // out[n][3] = ref, nobreak, exact for spheres[n][4], each broadcast to 8 lanes
    void ref_env_query(void *h, const float *spheres4, std::size_t n, uint8_t *out)
    {
        for (std::size_t i = 0; i < n; ++i) answer(static_cast<Env *>(h), broadcast(spheres4 + 4 * i), out + 3 * i);
    }
    // the same for rakes: spheres[n_rakes][8][4]
    void ref_env_query_rakes(void *h, const float *spheres4, std::size_t n_rakes, uint8_t *out)
    {
        for (std::size_t j = 0; j < n_rakes; ++j) answer(static_cast<Env *>(h), rake(spheres4, j), out + 3 * j);
    }

    // the signed value the predicate returns for (primitive `index` of sorted list `kind`, sphere i); its sign bit is
    // the answer.  kind: 0 sphere, 1 capsule, 2 z-aligned capsule, 3 cuboid, 4 z-aligned cuboid, 5 heightfield
    int ref_env_values(void *h, int kind, std::size_t index, const float *spheres4, std::size_t n, float *out)
    {
        const auto &e = static_cast<Env *>(h)->vec();
        const std::size_t sizes[6] = {e.spheres.size(),          e.capsules.size(),          e.z_aligned_capsules.size(),
                                      e.cuboids.size(),          e.z_aligned_cuboids.size(), e.heightfields.size()};
        if (kind < 0 or kind > 5 or index >= sizes[kind]) return -1;
        for (std::size_t i = 0; i < n; ++i)
        {
            const Query q = broadcast(spheres4 + 4 * i);
            const V8 rsq = q.r * q.r;
            switch (kind)
            {
                case 0: out[i] = lane0(vc::sphere_sphere_sql2(e.spheres[index], q.x, q.y, q.z, q.r)); break;
                case 1: out[i] = lane0(vc::sphere_capsule(e.capsules[index], q.x, q.y, q.z, q.r)); break;
                case 2: out[i] = lane0(vc::sphere_z_aligned_capsule(e.z_aligned_capsules[index], q.x, q.y, q.z, q.r)); break;
                case 3: out[i] = lane0(vc::sphere_cuboid(e.cuboids[index], q.x, q.y, q.z, rsq)); break;
                case 4: out[i] = lane0(vc::sphere_z_aligned_cuboid(e.z_aligned_cuboids[index], q.x, q.y, q.z, rsq)); break;
                default: out[i] = lane0(vc::sphere_heightfield(e.heightfields[index], q.x, q.y, q.z, q.r)); break;
            }
        }
        return 0;
    }
}
