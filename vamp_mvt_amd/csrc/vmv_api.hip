// vmv_api.hip — C ABI (include/vamp_mvt_amd.h): environment builder/upload, robot table, dispatch to the
// per-robot kernel translation units (gen/tu_<robot>.hip).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see __graft_entry__.build()).  There is no CPU
// fallback anywhere in this library: every compute entry point needs a HIP device.
#include "../../include/vamp_mvt_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vmv_capt_build.h"
#include "vmv_mvt_build.h"
#include "vmv_grid_build.h"
#include "vmv_common.h"

// ---------------------------------------------------------------------------------------------------------
// host-side robot table
// ---------------------------------------------------------------------------------------------------------
struct vmv_link_reach  // reach certificate of one link (tools/gen_hip.py: link_samples)
{
    int group;       // index of the link's environment group = bit in EnvDev::link_skip
    int n;           // sample centres
    float slack;     // every centre the link can have lies within `slack` of a sample
    float radius;    // the link's bounding-sphere radius
    const float (*samples)[3];
};
struct vmv_robot_info
{
    const char *name;
    int dimension, n_spheres, resolution;
    float min_radius, max_radius, max_bounding_radius;
    float grid_radius[4];  // largest bounding radius of each broad-phase grid class (vmv::kGridClasses)
    float lower[16], span[16], descale[16];
    const char *end_effector;
    const char *joint_names[16];
    int n_self_pairs;
    const uint16_t (*self_pairs)[2];  // fine pairs of the self-collision groups, in group order
    int n_reach;
    const vmv_link_reach *reach;
};
#include "gen/robots_host.inc"

namespace
{
    thread_local std::string g_last_error;

    int hip_fail(hipError_t e, const char *what)
    {
        g_last_error = std::string(what) + ": " + hipGetErrorString(e);
        return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ?
                   VMV_ERR_NO_DEVICE :
                   VMV_ERR_HIP;
    }
#define VMV_HIP(call)                                  \
    do                                                 \
    {                                                  \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

    int require_device()
    {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0)
        {
            g_last_error = "no HIP device (this library has no CPU path)";
            return VMV_ERR_NO_DEVICE;
        }
        return VMV_OK;
    }

    using vmv::kMaxPrimFloats;
    using vmv::robot_launchers;
}  // namespace

namespace vmv
{
    int hip_status(hipError_t e, const char *what) { return hip_fail(e, what); }

    int refuse_argument(const char *message)
    {
        g_last_error = message;
        return VMV_ERR_INVALID_ARGUMENT;
    }

    // ---- per-(device, stream) tables of vmv_validate_batch_multi (vmv_common.h: MultiTableLease) ----
    namespace
    {
        struct MultiHostSlot
        {
            void *p = nullptr;
            size_t bytes = 0;
            hipEvent_t copied = nullptr;  // recorded after the slot's last copy
        };
        struct MultiTables
        {
            void *dev = nullptr;
            size_t bytes = 0;
            std::vector<MultiHostSlot> host;
        };
        std::mutex g_multi_mutex;
        std::map<std::pair<int, hipStream_t>, MultiTables> g_multi;  // never freed at exit (see vmv_release_staging)
    }  // namespace

    MultiTableLease::MultiTableLease() : lock_(g_multi_mutex, std::defer_lock) {}

    int MultiTableLease::acquire(hipStream_t stream, size_t bytes)
    {
        int dev = -1;
        VMV_HIP(hipGetDevice(&dev));
        const size_t want = std::max<size_t>(bytes, size_t{1} << 16);
        lock_.lock();
        MultiTables &m = g_multi[{dev, stream}];
        entry_ = &m;
        if (m.bytes < bytes)
        {
            if (m.dev) (void) hipFree(m.dev);  // (waits for the calls still using it)
            m.dev = nullptr, m.bytes = 0;
            VMV_HIP(hipMalloc(&m.dev, want));
            m.bytes = want;
        }
        // a host slot whose last copy has run (hipEventQuery: never waits), else a new one
        slot_ = m.host.size();
        for (size_t i = 0; i < m.host.size() && slot_ == m.host.size(); ++i)
            if (m.host[i].bytes >= bytes && hipEventQuery(m.host[i].copied) == hipSuccess) slot_ = i;
        if (slot_ == m.host.size())
        {
            MultiHostSlot s;
            VMV_HIP(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
            if (hipError_t e = hipHostMalloc(&s.p, want, hipHostMallocDefault); e != hipSuccess)
            {
                (void) hipEventDestroy(s.copied);
                return hip_fail(e, "hipHostMalloc(multi-environment tables)");
            }
            s.bytes = want;
            m.host.push_back(s);
        }
        host = m.host[slot_].p;
        this->dev = m.dev;
        return VMV_OK;
    }

    int MultiTableLease::upload(hipStream_t stream, size_t bytes)
    {
        VMV_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
        VMV_HIP(hipEventRecord(static_cast<MultiTables *>(entry_)->host[slot_].copied, stream));
        return VMV_OK;
    }

    void release_multi_tables()
    {
        std::lock_guard<std::mutex> g(g_multi_mutex);
        for (auto &kv : g_multi)
        {
            if (kv.second.dev) (void) hipFree(kv.second.dev);
            for (MultiHostSlot &s : kv.second.host)
            {
                (void) hipEventSynchronize(s.copied);
                (void) hipHostFree(s.p);
                (void) hipEventDestroy(s.copied);
            }
        }
        g_multi.clear();
    }

    // uniform configurations inside the joint bounds (bench input generator, counter based)
    __global__ void fill_uniform_kernel(float *q, size_t total, int dim, uint64_t seed, const float *lower,
                                        const float *span)
    {
        const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= total) return;
        uint64_t z = seed + 0x9e3779b97f4a7c15ull * (uint64_t) (i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z = z ^ (z >> 31);
        const float u = (float) (z >> 40) * (1.0f / 16777216.0f);
        const int j = (int) (i % (size_t) dim);
        q[i] = lower[j] + span[j] * u;
    }

    // vmv_bare_trig_error: the workgroups stride over the fp32 bit patterns lo .. hi (positive floats) and take each with
    // both signs; per lane the maxima of |bare_sin - vsin| and |bare_cos - vcos| (a NaN difference wins and stays),
    // reduced over the wave by shuffles, over the workgroup through LDS, and stored as partial[2 * block + {0, 1}];
    // trig_error_final_kernel (one workgroup) folds the `blocks` partials into out[0..1].
    constexpr uint32_t kTrigBlocks = 2048;
    __device__ __forceinline__ float nan_max(float m, float d) { return (d > m || d != d) ? d : m; }
    __device__ __forceinline__ void trig_block_max(float &ms, float &mc, float (&part)[2][kBlock / kWave])
    {
        for (int o = kWave / 2; o > 0; o /= 2)
        {
            ms = nan_max(ms, __shfl_xor(ms, o));
            mc = nan_max(mc, __shfl_xor(mc, o));
        }
        if (threadIdx.x % kWave == 0) part[0][threadIdx.x / kWave] = ms, part[1][threadIdx.x / kWave] = mc;
        __syncthreads();
        for (int w = 0; w < kBlock / kWave; ++w) ms = nan_max(ms, part[0][w]), mc = nan_max(mc, part[1][w]);
    }
    __global__ __launch_bounds__(kBlock) void trig_error_kernel(const uint32_t lo, const uint32_t hi, float *__restrict__ partial)
    {
        __shared__ float part[2][kBlock / kWave];
        float ms = 0.0f, mc = 0.0f;
        for (uint64_t b = (uint64_t) lo + blockIdx.x * (uint64_t) kBlock + threadIdx.x; b <= (uint64_t) hi;
             b += (uint64_t) gridDim.x * kBlock)
            for (uint32_t sign = 0u; sign < 2u; ++sign)
            {
                const float x = u2f((uint32_t) b | sign << 31);
                ms = nan_max(ms, vabs(bare_sin(x) - vsin(x)));
                mc = nan_max(mc, vabs(bare_cos(x) - vcos(x)));
            }
        trig_block_max(ms, mc, part);
        if (threadIdx.x == 0) partial[2 * blockIdx.x] = ms, partial[2 * blockIdx.x + 1] = mc;
    }
    __global__ __launch_bounds__(kBlock) void trig_error_final_kernel(const float *__restrict__ partial, const uint32_t blocks,
                                                                       float *__restrict__ out)
    {
        __shared__ float part[2][kBlock / kWave];
        float ms = 0.0f, mc = 0.0f;
        for (uint32_t i = threadIdx.x; i < blocks; i += kBlock) ms = nan_max(ms, partial[2 * i]), mc = nan_max(mc, partial[2 * i + 1]);
        trig_block_max(ms, mc, part);
        if (threadIdx.x == 0) out[0] = ms, out[1] = mc;
    }

    // Halton sample (skip + 1 + row) of the reference's sequence, element j (halton_element, vmv_common.h)
    __global__ void halton_kernel(float *q, size_t total, int dim, uint64_t skip, const float *lower, const float *span)
    {
        const size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
        if (idx >= total) return;
        const int j = (int) (idx % (size_t) dim);
        q[idx] = halton_element(skip + idx / (size_t) dim + 1, j, lower[j], span[j]);
    }

    // sphere_environment_in_collision (collision/validity.hh:47-158) for a batch of free spheres, one lane per sphere
    // (each sphere is its own replicated rake): the primitive lists with their sorted early-break, heightfields,
    // CAPT and MVT clouds, through the same device functions the robot kernels use (counted loops, no grid).
    // robot_spheres (optional, [n_robot] x y z r of one configuration, <robot>.filter_self_from_pointcloud): a sphere
    // also "hits" when it overlaps one of them (sphere_sphere_sql2 < 0, strict, robot_helper.hh:306-307)
    __global__ __launch_bounds__(kBlock) void spheres_env_kernel(const EnvDev *__restrict__ env, const float4 *__restrict__ spheres,
                                                                  const size_t n, uint8_t *__restrict__ hits,
                                                                  const float4 *__restrict__ robot_spheres, const int n_robot)
    {
        extern __shared__ __align__(16) float smem[];
        const uint32_t n_floats = env->n_floats;  // a multiple of 4
        for (uint32_t i = threadIdx.x; i < n_floats; i += blockDim.x) smem[i] = env->prims[i];
        __syncthreads();
        // [primitive block | CAPT hit-flag rows]; no radius table (free spheres bring their own radius)
        const EnvView E{(env_cptr) env, (lds_cptr) smem, 0u, (lds_cptr) smem + n_floats + kCaptFlagWords};
        const size_t rounds = (n + (size_t) gridDim.x * kBlock - 1) / ((size_t) gridDim.x * kBlock);
        for (size_t k = 0; k < rounds; ++k)  // every wave runs every round: env_hit uses wave-wide votes
        {
            const size_t i = (k * gridDim.x + blockIdx.x) * (size_t) kBlock + threadIdx.x;
            const bool active = i < n;
            const float4 s = active ? spheres[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            bool hit = env_hit<1, 0, kEnvFull>(E, s.x, s.y, s.z, s.w, active, nullptr);
            for (int k = 0; k < n_robot; ++k)  // wave-uniform records (scalar loads)
            {
                const float4 a = robot_spheres[k];
                hit |= neg(sphere_sphere_sql2(a.x, a.y, a.z, a.w, s.x, s.y, s.z, s.w));
            }
            if (active) hits[i] = hit ? 1 : 0;
        }
    }
}  // namespace vmv

// ---------------------------------------------------------------------------------------------------------
// environment (host builder + device image)
// ---------------------------------------------------------------------------------------------------------
struct vmv_env
{
    struct Sphere
    {
        float x, y, z, r, min_d;
    };
    struct Cuboid
    {
        float p[15];
        float min_d;
    };
    struct Capsule
    {
        float p[8];
        float min_d;
    };
    std::vector<Sphere> spheres;
    std::vector<Capsule> capsules, z_capsules;
    std::vector<Cuboid> cuboids, z_cuboids;
    std::vector<vmv::CaptArrays> capts;
    std::vector<vmv::MvtArrays> mvts;
    struct HeightField
    {
        float c[3], inv[3];
        size_t xd, yd;
        std::vector<float> data;
    };
    std::vector<HeightField> heightfields;
    bool attached = false;
    float attach_tf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // row-major 3 x 4 (R | t), relative to the end effector
    std::vector<float> attach_spheres;                            // [n][4] = x y z r in that frame

    bool finalized = false;
    int device = -1;
    vmv::EnvLaunch launch[8]{};  // per robot: host + device copies of the kernel-side description (grids differ)
    // the robot-specific part (broad-phase grids, static links) is built on the robot's first use
    vmv::EnvDev base{};
    std::vector<vmv::GridPrim> grid_prims;
    uint32_t grid_words = 0;
    // per robot: kRobotNone -> kRobotBuilding (claimed by one lazy build or one vmv_env_prepare_multi call, under
    // robot_mutex) -> kRobotBuilt (launch[r], robot_status[r], robot_error[r] final; released with robot_cv)
    std::atomic<int> robot_state[8] = {};
    std::mutex robot_mutex;  // guards the state changes and `allocations` / `shared_allocations`
    std::condition_variable robot_cv;
    int robot_status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string robot_error[8];
    std::vector<void *> allocations;
    std::vector<std::shared_ptr<void>> shared_allocations;  // device memory of a batch preparation, freed by its last holder
};
enum
{
    kRobotNone = 0,
    kRobotBuilding = 1,
    kRobotBuilt = 2
};

namespace
{
    float dot3h(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx) + (ay * by) + (az * bz); }
    // collision/math.hh:47-51: std::max(std::min(v, upper), lower) of the C++ library, written out: a NaN comes back as
    // NaN (in a HIP translation unit std::min / std::max on floats may resolve to fminf / fmaxf, which drop it)
    float clamp_scalar(float v, float lo, float hi)
    {
        const float m = (hi < v) ? hi : v;
        return (m < lo) ? lo : m;
    }

    // collision/shapes.hh:52-67
    float cuboid_min_distance(const float *p)
    {
        const float x = p[0], y = p[1], z = p[2];
        const float d1 = dot3h(-x, -y, -z, p[3], p[4], p[5]);
        const float d2 = dot3h(-x, -y, -z, p[6], p[7], p[8]);
        const float d3 = dot3h(-x, -y, -z, p[9], p[10], p[11]);
        const float v1 = clamp_scalar(d1, -p[12], p[12]);
        const float v2 = clamp_scalar(d2, -p[13], p[13]);
        const float v3 = clamp_scalar(d3, -p[14], p[14]);
        const float xn = x + p[3] * v1 + p[6] * v2 + p[9] * v3;
        const float yn = y + p[4] * v1 + p[7] * v2 + p[10] * v3;
        const float zn = z + p[5] * v1 + p[8] * v2 + p[11] * v3;
        return std::sqrt(xn * xn + yn * yn + zn * zn);
    }

    // collision/shapes.hh:165-189.  Where the reference divides 0 by 0 (ol == 0: the origin lies on the capsule's axis) the
    // true distance is 0, and that is what is stored; so is any value that is still not finite (a zero-length capsule
    // with rdv = inf).  Such an entry sorts first and never triggers the sorted early break (include/vamp_mvt_amd.h).
    float capsule_min_distance(const float *p)
    {
        const float x1 = p[0], y1 = p[1], z1 = p[2], xv = p[3], yv = p[4], zv = p[5], r = p[6], rdv = p[7];
        const float t = clamp_scalar(dot3h(-x1, -y1, -z1, xv, yv, zv) * rdv, 0.F, 1.F);
        const float xp = x1 + xv * t, yp = y1 + yv * t, zp = z1 + zv * t;
        float xo = -xp, yo = -yp, zo = -zp;
        const float ol = std::sqrt(dot3h(xo, yo, zo, xo, yo, zo));
        if (ol == 0.F) return 0.F;
        xo = xo / ol;
        yo = yo / ol;
        zo = zo / ol;
        const float ro = clamp_scalar(ol, 0.F, r);
        const float xn = xp + ro * xo, yn = yp + ro * yo, zn = zp + ro * zo;
        const float d = std::sqrt(xn * xn + yn * yn + zn * zn);
        return std::isfinite(d) ? d : 0.F;
    }

    template <typename T>
    void sort_by_min_distance(std::vector<T> &v)
    {
        std::stable_sort(v.begin(), v.end(), [](const T &a, const T &b) { return a.min_d < b.min_d; });
    }

    // the getters return the lists as the kernels will see them: sorted by min_distance (stable), finalized or not
    template <typename T>
    std::vector<T> sorted_copy(const std::vector<T> &v)
    {
        std::vector<T> c(v);
        sort_by_min_distance(c);
        return c;
    }

    template <typename T>
    int upload(vmv_env *env, const std::vector<T> &host, const T **dev_ptr)
    {
        void *d = nullptr;
        const size_t bytes = std::max<size_t>(host.size() * sizeof(T), 16);
        VMV_HIP(hipMalloc(&d, bytes));
        env->allocations.push_back(d);
        if (!host.empty()) VMV_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        *dev_ptr = static_cast<const T *>(d);
        return VMV_OK;
    }
}  // namespace

extern "C"
{
    const char *vmv_status_string(int status)
    {
        switch (status)
        {
            case VMV_OK: return "ok";
            case VMV_ERR_INVALID_ARGUMENT: return "invalid argument";
            case VMV_ERR_NO_DEVICE: return "no HIP device";
            case VMV_ERR_HIP: return "HIP runtime error";
            case VMV_ERR_CAPACITY: return "environment exceeds on-chip staging capacity";
            case VMV_ERR_NOT_FINALIZED: return "environment not finalized";
            case VMV_ERR_UNKNOWN_ROBOT: return "unknown robot";
            case VMV_ERR_FINALIZED: return "environment already finalized";
            default: return "unknown status";
        }
    }
    int vmv_abi_version(void) { return 1; }
    const char *vmv_last_error(void) { return g_last_error.c_str(); }

    int vmv_device_count(int *count)
    {
        if (!count) return VMV_ERR_INVALID_ARGUMENT;
        *count = 0;
        hipError_t e = hipGetDeviceCount(count);
        if (e != hipSuccess)
        {
            *count = 0;
            return hip_fail(e, "hipGetDeviceCount");
        }
        return VMV_OK;
    }
    int vmv_set_device(int device)
    {
        VMV_HIP(hipSetDevice(device));
        return VMV_OK;
    }
    int vmv_get_device(int *device)
    {
        if (!device) return VMV_ERR_INVALID_ARGUMENT;
        VMV_HIP(hipGetDevice(device));
        return VMV_OK;
    }

    // ---- robots ----
    int vmv_num_robots(void) { return kNumRobots; }
    static bool robot_ok(int r) { return r >= 0 && r < kNumRobots; }
    const char *vmv_robot_name(int r) { return robot_ok(r) ? kRobots[r].name : nullptr; }
    int vmv_robot_id(const char *name)
    {
        if (!name) return -1;
        for (int i = 0; i < kNumRobots; ++i)
            if (std::strcmp(kRobots[i].name, name) == 0) return i;
        return -1;
    }
    int vmv_robot_dimension(int r) { return robot_ok(r) ? kRobots[r].dimension : -1; }
    int vmv_robot_n_spheres(int r) { return robot_ok(r) ? kRobots[r].n_spheres : -1; }
    int vmv_robot_resolution(int r) { return robot_ok(r) ? kRobots[r].resolution : -1; }
    int vmv_robot_min_max_radii(int r, float *mn, float *mx)
    {
        if (!robot_ok(r)) return VMV_ERR_UNKNOWN_ROBOT;
        if (mn) *mn = kRobots[r].min_radius;
        if (mx) *mx = kRobots[r].max_radius;
        return VMV_OK;
    }
    int vmv_robot_bounds(int r, float *lower, float *span, float *descale)
    {
        if (!robot_ok(r)) return VMV_ERR_UNKNOWN_ROBOT;
        const size_t b = sizeof(float) * (size_t) kRobots[r].dimension;
        if (lower) std::memcpy(lower, kRobots[r].lower, b);
        if (span) std::memcpy(span, kRobots[r].span, b);
        if (descale) std::memcpy(descale, kRobots[r].descale, b);
        return VMV_OK;
    }
    const char *vmv_robot_joint_name(int r, int j)
    {
        return (robot_ok(r) && j >= 0 && j < kRobots[r].dimension) ? kRobots[r].joint_names[j] : nullptr;
    }
    const char *vmv_robot_end_effector(int r) { return robot_ok(r) ? kRobots[r].end_effector : nullptr; }

    // ---- environment ----
    int vmv_env_create(vmv_env **out)
    {
        if (!out) return VMV_ERR_INVALID_ARGUMENT;
        *out = new (std::nothrow) vmv_env();
        return *out ? VMV_OK : VMV_ERR_INVALID_ARGUMENT;
    }
    int vmv_env_destroy(vmv_env *env)
    {
        if (!env) return VMV_OK;
        for (void *p : env->allocations) (void) hipFree(p);
        delete env;
        return VMV_OK;
    }
#define VMV_MUTABLE(env)                                  \
    if (!(env)) return VMV_ERR_INVALID_ARGUMENT;          \
    if ((env)->finalized) return VMV_ERR_FINALIZED;

    int vmv_env_add_sphere(vmv_env *env, float x, float y, float z, float r)
    {
        VMV_MUTABLE(env)
        // collision/shapes.hh:236-239
        env->spheres.push_back({x, y, z, r, std::sqrt(x * x + y * y + z * z) - r});
        return VMV_OK;
    }
    int vmv_env_add_cuboid(vmv_env *env, const float *p)
    {
        VMV_MUTABLE(env)
        if (!p) return VMV_ERR_INVALID_ARGUMENT;
        vmv_env::Cuboid c;
        std::memcpy(c.p, p, sizeof(c.p));
        c.min_d = cuboid_min_distance(p);
        (p[11] == 1.0f ? env->z_cuboids : env->cuboids).push_back(c);  // environment.cc:123-130
        return VMV_OK;
    }
    int vmv_env_add_capsule(vmv_env *env, const float *p)
    {
        VMV_MUTABLE(env)
        if (!p) return VMV_ERR_INVALID_ARGUMENT;
        vmv_env::Capsule c;
        std::memcpy(c.p, p, sizeof(c.p));
        c.min_d = capsule_min_distance(p);
        ((p[3] == 0.0f && p[4] == 0.0f) ? env->z_capsules : env->capsules).push_back(c);  // environment.cc:137-144
        return VMV_OK;
    }
    int vmv_env_add_heightfield(vmv_env *env, const float *center, const float *scale, size_t xd, size_t yd,
                                const float *data)
    {
        VMV_MUTABLE(env)
        if (!center || !scale || !data || xd == 0 || yd == 0 || xd * yd > (size_t) 1 << 30) return VMV_ERR_INVALID_ARGUMENT;
        if (env->heightfields.size() >= (size_t) vmv::kMaxHeightFields) return VMV_ERR_CAPACITY;
        vmv_env::HeightField h;
        for (int k = 0; k < 3; ++k)
        {
            h.c[k] = center[k];
            h.inv[k] = 1.F / scale[k];  // factory.hh:376-386
        }
        h.xd = xd;
        h.yd = yd;
        h.data.assign(data, data + xd * yd);
        env->heightfields.push_back(std::move(h));
        return VMV_OK;
    }
    int vmv_env_attach(vmv_env *env, const float *tf16, const float *spheres, size_t n)
    {
        VMV_MUTABLE(env)
        if (!tf16 || (n && !spheres)) return VMV_ERR_INVALID_ARGUMENT;
        if (n > (size_t) vmv::kMaxAttachSpheres) return VMV_ERR_CAPACITY;
        env->attached = true;
        for (int i = 0; i < 12; ++i) env->attach_tf[i] = tf16[i];  // the first three rows of the row-major 4 x 4
        env->attach_spheres.assign(spheres, spheres + 4 * n);
        return VMV_OK;
    }
    int vmv_env_detach(vmv_env *env)
    {
        VMV_MUTABLE(env)
        env->attached = false;
        env->attach_spheres.clear();
        return VMV_OK;
    }
    int vmv_env_heightfield_count(const vmv_env *env, size_t *count)
    {
        if (!env || !count) return VMV_ERR_INVALID_ARGUMENT;
        *count = env->heightfields.size();
        return VMV_OK;
    }
    int vmv_env_add_capt_pointcloud(vmv_env *env, const float *pts, size_t n, float r_min, float r_max, float r_point,
                                    uint64_t *build_ns)
    {
        VMV_MUTABLE(env)
        if (!pts || n < 2) return VMV_ERR_INVALID_ARGUMENT;
        if (env->capts.size() >= (size_t) vmv::kMaxCapt) return VMV_ERR_CAPACITY;
        const auto t0 = std::chrono::steady_clock::now();
        vmv::CaptArrays arrays;
        if (!vmv::build_capt(pts, n, r_min, r_max, r_point, arrays)) return VMV_ERR_INVALID_ARGUMENT;
        env->capts.push_back(std::move(arrays));
        if (build_ns)
            *build_ns = (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now() - t0)
                            .count();
        return VMV_OK;
    }

    int vmv_env_add_capt_pointcloud_gpu(vmv_env *env, const float *pts, size_t n, float r_min, float r_max, float r_point,
                                        uint64_t *build_ns, uint64_t *device_ns)
    {
        VMV_MUTABLE(env)
        if (!pts || n < 2) return VMV_ERR_INVALID_ARGUMENT;
        if (env->capts.size() >= (size_t) vmv::kMaxCapt) return VMV_ERR_CAPACITY;
        int rc = require_device();
        if (rc != VMV_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        vmv::CaptArrays arrays;
        rc = vmv::build_capt_device(pts, n, r_min, r_max, r_point, arrays, device_ns);
        if (rc != VMV_OK) return rc;
        for (void *p : {(void *) arrays.dev.tests, (void *) arrays.dev.aff_starts, (void *) arrays.dev.aabbs, (void *) arrays.dev.aff})
            if (p) env->allocations.push_back(p);  // freed with the environment
        env->capts.push_back(std::move(arrays));
        if (build_ns)
            *build_ns = (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now() - t0)
                            .count();
        return VMV_OK;
    }

    int vmv_env_add_mvt_pointcloud(vmv_env *env, const float *pts, size_t n, float r_min, float r_max,
                                   const float *ws_min, const float *ws_max, float r_point, uint64_t *build_ns,
                                   int *reason)
    {
        VMV_MUTABLE(env)
        if (reason) *reason = 0;
        if (!pts || !ws_min || !ws_max) return VMV_ERR_INVALID_ARGUMENT;
        if (env->mvts.size() >= (size_t) vmv::kMaxMvt) return VMV_ERR_CAPACITY;
        const auto t0 = std::chrono::steady_clock::now();
        vmv::MvtArrays arrays;
        const vmv::MvtStatus st = vmv::build_mvt(pts, n, r_min, r_max, ws_min, ws_max, r_point, arrays);
        if (st != vmv::MvtStatus::ok)
        {
            if (reason) *reason = (int) st;
            g_last_error = "MVT: a pool the reference sizes up front would be exhausted (see vmv_mvt_build.h)";
            return VMV_ERR_CAPACITY;
        }
        env->mvts.push_back(std::move(arrays));
        if (build_ns)
            *build_ns = (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now() - t0)
                            .count();
        return VMV_OK;
    }

    int vmv_env_mvt_count(const vmv_env *env, size_t *count)
    {
        if (!env || !count) return VMV_ERR_INVALID_ARGUMENT;
        *count = env->mvts.size();
        return VMV_OK;
    }
    int vmv_env_mvt_info(const vmv_env *env, size_t index, uint32_t *gw, uint32_t *cap, uint32_t *nv, float *isf, float *box)
    {
        if (!env || index >= env->mvts.size()) return VMV_ERR_INVALID_ARGUMENT;
        const vmv::MvtArrays &m = env->mvts[index];
        if (gw) *gw = m.grid_width;
        if (cap) *cap = m.capacity;
        if (nv) *nv = m.n_voxels();
        if (isf) *isf = m.inv_scale;
        if (box)
        {
            std::memcpy(box, m.gmin, 12);
            std::memcpy(box + 3, m.gmax, 12);
        }
        return VMV_OK;
    }

    int vmv_env_finalize(vmv_env *env)
    {
        VMV_MUTABLE(env)
        int rc = require_device();
        if (rc != VMV_OK) return rc;
        sort_by_min_distance(env->spheres);
        sort_by_min_distance(env->capsules);
        sort_by_min_distance(env->z_capsules);
        sort_by_min_distance(env->cuboids);
        sort_by_min_distance(env->z_cuboids);

        // pack the LDS primitive block (record layouts: vmv_device.h)
        std::vector<float> block;
        vmv::EnvDev D_base{};
        vmv::EnvDev &D = D_base;
        D.n_sphere = (uint32_t) env->spheres.size();
        D.off_sphere = (uint32_t) block.size();
        for (const auto &s : env->spheres)
        {
            block.insert(block.end(), {s.x, s.y, s.z, s.r, s.min_d});
            block.insert(block.end(), (size_t) vmv::kSphereRec - 5, 0.f);
        }
        D.n_capsule = (uint32_t) env->capsules.size();
        D.off_capsule = (uint32_t) block.size();
        for (const auto &c : env->capsules)
            block.insert(block.end(),
                         {c.p[0], c.p[1], c.p[2], c.p[3], c.p[4], c.p[5], c.p[6], c.p[7], c.min_d, 0.f, 0.f, 0.f});
        D.n_zcapsule = (uint32_t) env->z_capsules.size();
        D.off_zcapsule = (uint32_t) block.size();
        for (const auto &c : env->z_capsules)
            block.insert(block.end(), {c.p[0], c.p[1], c.p[2], c.p[5], c.p[6], c.p[7], c.min_d, 0.f});
        D.n_cuboid = (uint32_t) env->cuboids.size();
        D.off_cuboid = (uint32_t) block.size();
        for (const auto &c : env->cuboids)
        {
            block.insert(block.end(), c.p, c.p + 15);
            block.push_back(c.min_d);
        }
        D.n_zcuboid = (uint32_t) env->z_cuboids.size();
        D.off_zcuboid = (uint32_t) block.size();
        for (const auto &c : env->z_cuboids)
            block.insert(block.end(), {c.p[0], c.p[1], c.p[2], c.p[3], c.p[4], c.p[6], c.p[7], c.p[12], c.p[13],
                                       c.p[14], c.min_d, 0.f});
        // compact min_distance arrays (one per list) for the wave-wide live-prefix count
        auto md_array = [&](auto &list, uint32_t &off)
        {
            while (block.size() % 4) block.push_back(0.f);
            off = (uint32_t) block.size();
            for (const auto &s : list) block.push_back(s.min_d);
        };
        md_array(env->spheres, D.off_md_sphere);
        md_array(env->capsules, D.off_md_capsule);
        md_array(env->z_capsules, D.off_md_zcapsule);
        md_array(env->cuboids, D.off_md_cuboid);
        md_array(env->z_cuboids, D.off_md_zcuboid);
        uint32_t total_words = 0;
        {  // candidate words of the fine phase (vmv_device.h, kCandidateMargin): 32 primitives per word, per list
            uint32_t *const base[5] = {&D.wbase_sphere, &D.wbase_capsule, &D.wbase_zcapsule, &D.wbase_cuboid, &D.wbase_zcuboid};
            uint32_t *const shift[5] = {&D.wshift_sphere, &D.wshift_capsule, &D.wshift_zcapsule, &D.wshift_cuboid, &D.wshift_zcuboid};
            const uint32_t count[5] = {D.n_sphere, D.n_capsule, D.n_zcapsule, D.n_cuboid, D.n_zcuboid};
            uint32_t w = 0;
            for (int t = 0; t < 5; ++t)
            {
                *base[t] = w, *shift[t] = 0u;
                w += (count[t] + 31u) / 32u;
            }
            // More lists than words (all five kinds present, say): lists of at most 32 primitives share words — a list
            // starts at the next free bit when it fits into what is left of the word, else (and always when it is
            // longer than a word) at bit 0 of the next one.  Not for the environments the three-list kernel variant
            // serves (well-formed primitives without general cuboids / capsules, nothing else): it reads no shifts.
            const bool three_lists = env->capsules.empty() && env->cuboids.empty() && env->capts.empty() && env->mvts.empty() &&
                                     env->heightfields.empty();
            if (w > (uint32_t) vmv::kMaskWords && !three_lists)
            {
                uint32_t pos = 0;  // next free bit
                for (int t = 0; t < 5; ++t)
                {
                    if (count[t] == 0u) continue;
                    if (count[t] > 32u || (pos % 32u) + count[t] > 32u) pos = (pos + 31u) & ~31u;
                    *base[t] = pos / 32u, *shift[t] = pos % 32u;
                    pos += count[t];
                    if (count[t] > 32u) pos = (pos + 31u) & ~31u;
                }
                w = (pos + 31u) / 32u;
            }
            D.masked_fine = (w <= (uint32_t) vmv::kMaskWords) ? 1u : 0u;
            total_words = w;
        }
        {
            // The candidate pruning (fine-phase margin, broad-phase grid) assumes 1-Lipschitz primitive distances, which
            // holds for orthonormal cuboid axes and a capsule whose rdv is 1 / |v|^2.  The ABI accepts arbitrary
            // canonical parameters (as the reference does), so environments with an ill-formed primitive run the full
            // sorted loops instead: same answers as the reference's loop, no pruning.
            bool well_formed = true;
            const double origin[3] = {0, 0, 0};
            for (const auto *list : {&env->cuboids, &env->z_cuboids})
                for (const auto &c : *list)
                {
                    double lip = 1.0;
                    (void) vmv::grid_detail::cuboid_g(c.p, origin, list == &env->z_cuboids, lip);
                    well_formed = well_formed && std::isfinite(lip) && lip <= 1.0 + 1e-4;
                }
            for (const auto *list : {&env->capsules, &env->z_capsules})
                for (const auto &c : *list)
                {
                    const bool z = list == &env->z_capsules;
                    const double vv = (z ? 0.0 : (double) c.p[3] * c.p[3] + (double) c.p[4] * c.p[4]) + (double) c.p[5] * c.p[5];
                    const double k = vv * (double) c.p[7];
                    well_formed = well_formed && std::isfinite(k) && std::fabs(k - 1.0) <= 1e-3;
                }
            D.ill_formed = well_formed ? 0u : 1u;
            if (!well_formed) D.masked_fine = 0u;
        }
        while (block.size() % 4) block.push_back(0.f);
        if (block.size() > kMaxPrimFloats)
        {
            g_last_error = "more primitive records than the LDS staging budget (48 KiB)";
            return VMV_ERR_CAPACITY;
        }
        D.n_floats = (uint32_t) block.size();
        VMV_HIP(hipGetDevice(&env->device));
        rc = upload(env, block, &D.prims);
        if (rc != VMV_OK) return rc;

        D.n_capt = (uint32_t) env->capts.size();
        // the query copy of a cloud (blocked planes, leaf records, points sorted by distance to the leaf cell)
        auto query_copy = [&](const vmv::CaptArrays &a, vmv::CaptDev &c, uint32_t n_vectors) -> int
        {
            bool prune = true;
            if (const char *e = std::getenv("VMV_CAPT_NO_PREFIX")) prune = e[0] != '1';  // measurement / test aid
            for (int k = 0; k < 6; ++k)
                if (!(std::fabs(a.aabb_top[k]) <= 1e2f)) prune = false;  // the 1e-4 m margin is 13 fp32 ulps at 100 m; beyond: walk everything
            vmv::CaptQueryDev q;
            const int rc = vmv::build_capt_query(c.tests, c.aff_starts, c.aabbs, c.aff_x, c.aff_y, c.aff_z, a.nlog2, n_vectors,
                                                 a.r_min, a.r_max, a.r_point, prune, a.aabb_top, q);
            if (rc != VMV_OK)
            {
                if (rc == VMV_ERR_CAPACITY) g_last_error = "point cloud too large for the device query copy";
                return rc;
            }
            env->allocations.push_back(q.points);
            env->allocations.push_back(q.leaves);
            env->allocations.push_back(q.planes);
            c.q_x = q.points, c.q_y = q.points + (size_t) n_vectors * 8, c.q_z = q.points + 2 * (size_t) n_vectors * 8;
            c.q_leaves = q.leaves;
            c.q_planes = q.planes;
            c.cut_t0 = q.t0, c.cut_inv_step = q.inv_step;
            c.q_dist = q.dist;
            if (q.dist) env->allocations.push_back(q.dist);
            for (int k = 0; k < 3; ++k) c.dist_dims[k] = q.dist_dims[k], c.dist_origin[k] = q.dist_origin[k];
            c.dist_inv_cell = q.dist_inv_cell;
            return VMV_OK;
        };
        for (size_t i = 0; i < env->capts.size(); ++i)
        {
            vmv::CaptArrays &a = env->capts[i];
            vmv::CaptDev &c = D.capt[i];
            if (a.dev.tests && a.dev.device == env->device)
            {
                // built on this device: use the arrays where they are
                const size_t nv = a.dev.n_vectors;
                c.tests = a.dev.tests;
                c.aff_starts = a.dev.aff_starts;
                c.aabbs = a.dev.aabbs;
                c.aff_x = a.dev.aff;
                c.aff_y = a.dev.aff + nv * 8;
                c.aff_z = a.dev.aff + 2 * nv * 8;
                std::memcpy(c.aabb_top, a.aabb_top, sizeof(c.aabb_top));
                c.r_point = a.r_point;
                c.nlog2 = a.nlog2;
                c.n_tests = a.n_tests();
                if ((rc = query_copy(a, c, (uint32_t) nv)) != VMV_OK) return rc;
                continue;
            }
            if ((rc = vmv::download_capt(a)) != VMV_OK) return rc;  // built on another device: go through the host
            if ((rc = upload(env, a.tests, &c.tests)) != VMV_OK) return rc;
            if ((rc = upload(env, a.aff_starts, &c.aff_starts)) != VMV_OK) return rc;
            if ((rc = upload(env, a.aabbs, &c.aabbs)) != VMV_OK) return rc;
            if ((rc = upload(env, a.aff[0], &c.aff_x)) != VMV_OK) return rc;
            if ((rc = upload(env, a.aff[1], &c.aff_y)) != VMV_OK) return rc;
            if ((rc = upload(env, a.aff[2], &c.aff_z)) != VMV_OK) return rc;
            std::memcpy(c.aabb_top, a.aabb_top, sizeof(c.aabb_top));
            c.r_point = a.r_point;
            c.nlog2 = a.nlog2;
            c.n_tests = (uint32_t) a.tests.size();
            if ((rc = query_copy(a, c, (uint32_t) (a.aff[0].size() / 8))) != VMV_OK) return rc;
        }
        D.capt0_n_tests = D.n_capt ? env->capts[0].n_tests() : 0u;
        D.n_mvt = (uint32_t) env->mvts.size();
        for (size_t i = 0; i < env->mvts.size(); ++i)
        {
            const vmv::MvtArrays &m = env->mvts[i];
            vmv::MvtDev &d = D.mvt[i];
            if ((rc = upload(env, m.cells, &d.cells)) != VMV_OK) return rc;
            if ((rc = upload(env, m.vox_bbox, &d.vox_bbox)) != VMV_OK) return rc;
            if ((rc = upload(env, m.vox_offset, &d.vox_offset)) != VMV_OK) return rc;
            if ((rc = upload(env, m.px, &d.px)) != VMV_OK) return rc;
            if ((rc = upload(env, m.py, &d.py)) != VMV_OK) return rc;
            if ((rc = upload(env, m.pz, &d.pz)) != VMV_OK) return rc;
            std::memcpy(d.gmin, m.gmin, 12);
            std::memcpy(d.gmax, m.gmax, 12);
            std::memcpy(d.ws_min, m.ws_min, 12);
            d.inv_scale = m.inv_scale;
            d.r_point = m.r_point;
            d.grid_width = m.grid_width;
        }
        D.n_attach = 0;
        if (env->attached && !env->attach_spheres.empty())
        {
            // (an attachment without spheres poses nothing and tests nothing: plain fkcc gives the same answers)
            D.n_attach = (uint32_t) (env->attach_spheres.size() / 4);
            std::memcpy(D.attach_tf, env->attach_tf, sizeof(D.attach_tf));
            if ((rc = upload(env, env->attach_spheres, &D.attach_spheres)) != VMV_OK) return rc;
        }
        D.n_heightfield = (uint32_t) env->heightfields.size();
        for (size_t i = 0; i < env->heightfields.size(); ++i)
        {
            const vmv_env::HeightField &h = env->heightfields[i];
            vmv::HeightFieldDev &d = D.heightfield[i];
            if ((rc = upload(env, h.data, &d.data)) != VMV_OK) return rc;
            d.x = h.c[0], d.y = h.c[1], d.z = h.c[2];
            d.xs = h.inv[0], d.ys = h.inv[1], d.zs = h.inv[2];
            d.xd = (float) h.xd, d.yd = (float) h.yd;
            d.xd2 = (float) (h.xd / 2), d.yd2 = (float) (h.yd / 2);  // shapes.hh:289-290
            d.last = (uint32_t) (h.xd * h.yd - 1);
        }
        // broad-phase grid of the gate pass, one per robot (its reach is the robot's largest bounding radius)
        std::vector<vmv::GridPrim> gp;
        if (D.masked_fine)
        {
            auto add = [&](int type, const float *p, uint32_t wbase, uint32_t shift, size_t i)
            { gp.push_back(vmv::GridPrim{type, p, wbase + (uint32_t) ((shift + i) / 32), (uint32_t) ((shift + i) % 32)}); };
            for (size_t i = 0; i < env->spheres.size(); ++i) add(0, &env->spheres[i].x, D.wbase_sphere, D.wshift_sphere, i);
            for (size_t i = 0; i < env->capsules.size(); ++i) add(1, env->capsules[i].p, D.wbase_capsule, D.wshift_capsule, i);
            for (size_t i = 0; i < env->z_capsules.size(); ++i) add(2, env->z_capsules[i].p, D.wbase_zcapsule, D.wshift_zcapsule, i);
            for (size_t i = 0; i < env->cuboids.size(); ++i) add(3, env->cuboids[i].p, D.wbase_cuboid, D.wshift_cuboid, i);
            for (size_t i = 0; i < env->z_cuboids.size(); ++i) add(4, env->z_cuboids[i].p, D.wbase_zcuboid, D.wshift_zcuboid, i);
        }
        env->base = D_base;
        env->grid_prims = std::move(gp);
        env->grid_words = total_words;
        env->finalized = true;
        return VMV_OK;
    }

    int vmv_env_counts(const vmv_env *env, size_t *c)
    {
        if (!env || !c) return VMV_ERR_INVALID_ARGUMENT;
        c[0] = env->spheres.size();
        c[1] = env->capsules.size();
        c[2] = env->z_capsules.size();
        c[3] = env->cuboids.size();
        c[4] = env->z_cuboids.size();
        c[5] = env->capts.size();
        return VMV_OK;
    }
    int vmv_env_get_spheres(const vmv_env *env, float *out, size_t cap, size_t *n)
    {
        if (!env || !n) return VMV_ERR_INVALID_ARGUMENT;
        const auto v = sorted_copy(env->spheres);
        *n = v.size();
        if (out)
            for (size_t i = 0; i < std::min(cap, *n); ++i) std::memcpy(out + 5 * i, &v[i], 5 * sizeof(float));
        return VMV_OK;
    }
    int vmv_env_get_cuboids(const vmv_env *env, int z, float *out, size_t cap, size_t *n)
    {
        if (!env || !n) return VMV_ERR_INVALID_ARGUMENT;
        const auto v = sorted_copy(z ? env->z_cuboids : env->cuboids);
        *n = v.size();
        if (out)
            for (size_t i = 0; i < std::min(cap, *n); ++i) std::memcpy(out + 16 * i, &v[i], 16 * sizeof(float));
        return VMV_OK;
    }
    int vmv_env_get_capsules(const vmv_env *env, int z, float *out, size_t cap, size_t *n)
    {
        if (!env || !n) return VMV_ERR_INVALID_ARGUMENT;
        const auto v = sorted_copy(z ? env->z_capsules : env->capsules);
        *n = v.size();
        if (out)
            for (size_t i = 0; i < std::min(cap, *n); ++i) std::memcpy(out + 9 * i, &v[i], 9 * sizeof(float));
        return VMV_OK;
    }
    int vmv_env_capt_sizes(const vmv_env *env, size_t index, uint32_t *nlog2, uint32_t *n_aff)
    {
        if (!env || index >= env->capts.size()) return VMV_ERR_INVALID_ARGUMENT;
        if (nlog2) *nlog2 = env->capts[index].nlog2;
        if (n_aff) *n_aff = env->capts[index].n_aff_vectors();
        return VMV_OK;
    }
    int vmv_env_capt_arrays(const vmv_env *env, size_t index, float *tests, uint32_t *aff_starts, float *aabbs,
                            float *ax, float *ay, float *az, float *top)
    {
        if (!env || index >= env->capts.size()) return VMV_ERR_INVALID_ARGUMENT;
        vmv::CaptArrays &a = const_cast<vmv_env *>(env)->capts[index];  // a GPU-built cloud is downloaded on first look
        const int rc = vmv::download_capt(a);
        if (rc != VMV_OK) return rc;
        if (tests) std::memcpy(tests, a.tests.data(), a.tests.size() * 4);
        if (aff_starts) std::memcpy(aff_starts, a.aff_starts.data(), a.aff_starts.size() * 4);
        if (aabbs) std::memcpy(aabbs, a.aabbs.data(), a.aabbs.size() * 4);
        if (ax) std::memcpy(ax, a.aff[0].data(), a.aff[0].size() * 4);
        if (ay) std::memcpy(ay, a.aff[1].data(), a.aff[1].size() * 4);
        if (az) std::memcpy(az, a.aff[2].data(), a.aff[2].size() * 4);
        if (top) std::memcpy(top, a.aabb_top, sizeof(a.aabb_top));
        return VMV_OK;
    }
}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// robot-specific part of a finalized environment, built on first use (thread safe; environments stay immutable
// from the caller's point of view)
// ---------------------------------------------------------------------------------------------------------
namespace
{
    int build_robot_part(vmv_env *env, int r)
    {
        int rc;
        int dev = -1;
        VMV_HIP(hipGetDevice(&dev));
        if (dev != env->device) VMV_HIP(hipSetDevice(env->device));
        vmv::EnvDev Dr = env->base;
        const bool use_grid = std::getenv("VMV_NO_GRID") == nullptr;
        if (use_grid && !env->grid_prims.empty())
        {
            bool ok = true;
            std::vector<vmv::GridArrays> grids(vmv::kGridClasses);
            for (int c = 0; c < vmv::kGridClasses && ok; ++c)
            {
                if (c > 0 && kRobots[r].grid_radius[c] == kRobots[r].grid_radius[c - 1])
                    grids[c] = grids[c - 1];
                else
                    ok = vmv::build_grid(env->grid_prims, env->grid_words, (double) kRobots[r].grid_radius[c], grids[c]);
            }
            if (ok)
            {
                for (int c = 0; c < vmv::kGridClasses; ++c)
                {
                    vmv::GridDev &g = Dr.grid[c];
                    if ((rc = upload(env, grids[c].cells, &g.cells)) != VMV_OK) return rc;
                    for (int k = 0; k < 3; ++k)
                    {
                        g.dims[k] = grids[c].dims[k];
                        g.origin[k] = grids[c].origin[k];
                    }
                    g.inv_cell = grids[c].inv_cell;
                }
                Dr.grid_words = env->grid_words;
            }
        }
        // Reach certificates: a link whose bounding sphere cannot come within 1 mm of any primitive, whatever the
        // configuration, is skipped by the environment kernels (its gate could never fire).  Only for environments of
        // well-formed primitives (masked_fine: the distance expressions below are then exact and 1-Lipschitz) without
        // heightfields / point clouds; VMV_NO_LINK_SKIP=1 switches it off (A/B, tests).
        Dr.link_skip = 0ull;
        if (Dr.masked_fine && Dr.n_capt + Dr.n_mvt + Dr.n_heightfield == 0 && std::getenv("VMV_NO_LINK_SKIP") == nullptr)
            for (int k = 0; k < kRobots[r].n_reach; ++k)
            {
                const vmv_link_reach &lr = kRobots[r].reach[k];
                if (lr.n <= 0 || lr.group < 0 || lr.group >= 64) continue;
                const double need = (double) lr.radius + (double) lr.slack + 1e-3;
                bool free = true;
                for (int i = 0; i < lr.n && free; ++i)
                {
                    const double x[3] = {lr.samples[i][0], lr.samples[i][1], lr.samples[i][2]};
                    for (const auto &g : env->grid_prims)
                    {
                        double lip = 1.0, d;
                        if (g.type == 0)
                        {
                            const double dx = x[0] - g.p[0], dy = x[1] - g.p[1], dz = x[2] - g.p[2];
                            d = std::sqrt(dx * dx + dy * dy + dz * dz) - g.p[3];
                        }
                        else if (g.type <= 2)
                            d = vmv::grid_detail::capsule_g(g.p, x, g.type == 2, lip);
                        else
                            d = vmv::grid_detail::cuboid_g(g.p, x, g.type == 4, lip);
                        if (!(d > need * lip))
                        {
                            free = false;
                            break;
                        }
                    }
                }
                if (free) Dr.link_skip |= 1ull << lr.group;
            }
        env->launch[r].host = Dr;
        std::vector<vmv::EnvDev> one(1, Dr);
        const vmv::EnvDev *d_env = nullptr;
        if ((rc = upload(env, one, &d_env)) != VMV_OK) return rc;
        env->launch[r].d_env = d_env;
        rc = robot_launchers(r).prepare(env->launch[r], const_cast<vmv::EnvDev *>(d_env));
        if (dev != env->device) (void) hipSetDevice(dev);
        return rc;
    }

    // A finalized environment lives on ONE device (its primitive block, point clouds, grids).  The batched entry
    // points launch on the caller's current device and stream, so that device must be the environment's.
    int check_device(const vmv_env *env)
    {
        int dev = -1;
        VMV_HIP(hipGetDevice(&dev));
        if (dev != env->device)
        {
            g_last_error = "environment was finalized on device " + std::to_string(env->device) + ", current device is " +
                           std::to_string(dev) + " (finalize one environment per device)";
            return VMV_ERR_INVALID_ARGUMENT;
        }
        return VMV_OK;
    }

    int robot_result(const vmv_env *env, int r)  // of a built part
    {
        if (env->robot_status[r] != VMV_OK) g_last_error = env->robot_error[r];
        return env->robot_status[r];
    }

    // the lazy path: the first caller builds on the host (holding robot_mutex, as builds of other robots for this
    // environment append to the same lists), everybody else waits for whoever has claimed the part
    int ensure_robot(const vmv_env *cenv, int r)
    {
        vmv_env *env = const_cast<vmv_env *>(cenv);
        if (env->robot_state[r].load(std::memory_order_acquire) != kRobotBuilt)
        {
            std::unique_lock<std::mutex> lock(env->robot_mutex);
            env->robot_cv.wait(lock, [&]() { return env->robot_state[r].load(std::memory_order_relaxed) != kRobotBuilding; });
            if (env->robot_state[r].load(std::memory_order_relaxed) == kRobotNone)
            {
                env->robot_state[r].store(kRobotBuilding, std::memory_order_relaxed);
                env->robot_status[r] = build_robot_part(env, r);
                if (env->robot_status[r] != VMV_OK) env->robot_error[r] = g_last_error;
                env->robot_state[r].store(kRobotBuilt, std::memory_order_release);
                env->robot_cv.notify_all();
            }
        }
        return robot_result(env, r);
    }

    struct DeviceFree
    {
        void operator()(void *p) const { (void) hipFree(p); }
    };

    // The batch path (vmv_env_prepare_multi and the multi-environment validate calls): claims every environment of
    // `envs` whose part for robot r nobody has built or claimed, builds those parts together on the device, and waits
    // for the ones somebody else is building.  All environments are finalized on the current device.  Bit for bit what
    // build_robot_part makes.  The EnvDev images go up once, complete but for link_skip and static_hit, which the
    // reach and static-link kernels store into them in place.
    int build_robot_parts(const vmv_env *const *cenvs, size_t n_envs, int r)
    {
        std::vector<vmv_env *> mine, theirs;
        for (size_t k = 0; k < n_envs; ++k)
        {
            vmv_env *env = const_cast<vmv_env *>(cenvs[k]);
            if (env->robot_state[r].load(std::memory_order_acquire) == kRobotBuilt) continue;
            std::lock_guard<std::mutex> lock(env->robot_mutex);
            const int st = env->robot_state[r].load(std::memory_order_relaxed);
            if (st == kRobotNone)
            {
                env->robot_state[r].store(kRobotBuilding, std::memory_order_relaxed);
                mine.push_back(env);
            }
            else if (st == kRobotBuilding && std::find(mine.begin(), mine.end(), env) == mine.end())
                theirs.push_back(env);
        }
        const size_t n = mine.size();
        std::vector<int> status(n, VMV_OK);
        std::vector<vmv::EnvDev> images(n);
        std::shared_ptr<void> keep;  // [EnvDev images | cell words]
        vmv::EnvDev *d_images = nullptr;
        void *d_tables = nullptr;
        std::string error;
        const int rc = [&]() -> int
        {
            if (n == 0) return VMV_OK;
            const bool use_grid = std::getenv("VMV_NO_GRID") == nullptr, use_skip = std::getenv("VMV_NO_LINK_SKIP") == nullptr;
            std::vector<vmv::PrepPrim> prims;
            std::vector<vmv::PrepGridJob> grid_jobs;
            std::vector<vmv::PrepReachJob> reach_jobs;
            std::vector<size_t> reach_env;                           // the reach job's environment (index in `mine`)
            std::vector<int> grid_class(n * vmv::kGridClasses, -1);  // (environment, class) -> grid job
            size_t cell_words = 0;
            for (size_t k = 0; k < n; ++k)
            {
                const vmv_env *env = mine[k];
                images[k] = env->base;
                images[k].link_skip = 0ull;
                const bool grid = use_grid && !env->grid_prims.empty();
                // (an environment without primitives is certified too: no link can touch it)
                const bool reach = use_skip && env->base.masked_fine && kRobots[r].n_reach > 0 &&
                                   env->base.n_capt + env->base.n_mvt + env->base.n_heightfield == 0;
                if (!grid && !reach) continue;
                if (env->grid_prims.size() > vmv::kPrepMaxPrims)
                {
                    g_last_error = "more primitives with candidate bits than four words hold";
                    return VMV_ERR_CAPACITY;  // (finalize never makes such a list)
                }
                const uint32_t prim_lo = (uint32_t) prims.size();
                for (const vmv::GridPrim &g : env->grid_prims)
                {
                    vmv::PrepPrim q{g.type, g.word, g.bit, {}};
                    std::memcpy(q.p, g.p, sizeof(float) * (g.type == 0 ? 4 : g.type <= 2 ? 8 : 15));
                    prims.push_back(q);
                }
                if (reach)
                {
                    reach_jobs.push_back(vmv::PrepReachJob{prim_lo, (uint32_t) env->grid_prims.size(), nullptr, (uint32_t) reach_env.size()});
                    reach_env.push_back(k);
                }
                if (!grid) continue;
                vmv::GridGeometry geo[vmv::kGridClasses];
                bool ok = true;
                for (int c = 0; c < vmv::kGridClasses && ok; ++c)
                {
                    if (c > 0 && kRobots[r].grid_radius[c] == kRobots[r].grid_radius[c - 1])
                        geo[c] = geo[c - 1];
                    else
                        ok = vmv::grid_geometry(env->grid_prims, env->grid_words, (double) kRobots[r].grid_radius[c], geo[c]);
                }
                if (!ok) continue;
                for (int c = 0; c < vmv::kGridClasses; ++c)
                {
                    if (c > 0 && kRobots[r].grid_radius[c] == kRobots[r].grid_radius[c - 1])
                    {
                        grid_class[k * vmv::kGridClasses + c] = grid_class[k * vmv::kGridClasses + c - 1];
                        continue;
                    }
                    vmv::PrepGridJob j{};
                    j.prim_lo = prim_lo, j.n_prims = (uint32_t) env->grid_prims.size();
                    for (int a = 0; a < 3; ++a) j.dims[a] = geo[c].dims[a], j.origin[a] = geo[c].origin[a];
                    j.words = env->grid_words;
                    j.hf = geo[c].hf, j.half_diag = geo[c].half_diag, j.R = (double) kRobots[r].grid_radius[c];
                    j.cell_lo = cell_words;
                    cell_words += (size_t) j.dims[0] * j.dims[1] * j.dims[2] * j.words;
                    grid_class[k * vmv::kGridClasses + c] = (int) grid_jobs.size();
                    grid_jobs.push_back(j);
                }
                for (int c = 0; c < vmv::kGridClasses; ++c)
                {
                    vmv::GridDev &g = images[k].grid[c];
                    for (int a = 0; a < 3; ++a) g.dims[a] = geo[c].dims[a], g.origin[a] = geo[c].origin[a];
                    g.inv_cell = geo[c].inv_cell;
                }
                images[k].grid_words = env->grid_words;
            }
            // the allocation the environments keep: their images, then the cell words
            const size_t image_bytes = (n * sizeof(vmv::EnvDev) + 255) & ~size_t{255};
            void *d_keep = nullptr;
            VMV_HIP(hipMalloc(&d_keep, image_bytes + std::max<size_t>(cell_words, 4) * sizeof(uint32_t)));
            keep = std::shared_ptr<void>(d_keep, DeviceFree{});
            d_images = static_cast<vmv::EnvDev *>(d_keep);
            uint32_t *d_cells = reinterpret_cast<uint32_t *>(static_cast<char *>(d_keep) + image_bytes);
            for (size_t k = 0; k < n; ++k)
                for (int c = 0; c < vmv::kGridClasses; ++c)
                    if (const int j = grid_class[k * vmv::kGridClasses + c]; j >= 0)
                        images[k].grid[c].cells = d_cells + grid_jobs[(size_t) j].cell_lo;
            for (size_t i = 0; i < reach_jobs.size(); ++i) reach_jobs[i].image = d_images + reach_env[i];
            VMV_HIP(hipMemcpy(d_images, images.data(), n * sizeof(vmv::EnvDev), hipMemcpyHostToDevice));
            // the tables of this call: primitives, jobs, the robot's reach links and samples, the certificates' answers
            std::vector<vmv::PrepReachLink> links;
            std::vector<float> samples;
            for (int k = 0; k < kRobots[r].n_reach && !reach_jobs.empty(); ++k)
            {
                const vmv_link_reach &lr = kRobots[r].reach[k];
                if (lr.n <= 0 || lr.group < 0 || lr.group >= 64) continue;
                links.push_back(vmv::PrepReachLink{lr.group, (uint32_t) (samples.size() / 3), (uint32_t) lr.n,
                                                   (double) lr.radius + (double) lr.slack + 1e-3});
                samples.insert(samples.end(), &lr.samples[0][0], &lr.samples[0][0] + 3 * (size_t) lr.n);
            }
            std::vector<unsigned long long> skip(reach_jobs.size(), 0ull);
            if (!grid_jobs.empty() || !reach_jobs.empty())
            {
                size_t at = 0;
                auto place = [&](size_t bytes)
                {
                    const size_t o = at;
                    at += (bytes + 255) & ~size_t{255};
                    return o;
                };
                const size_t o_prims = place(prims.size() * sizeof(vmv::PrepPrim)), o_grid = place(grid_jobs.size() * sizeof(vmv::PrepGridJob)),
                             o_reach = place(reach_jobs.size() * sizeof(vmv::PrepReachJob)), o_links = place(links.size() * sizeof(vmv::PrepReachLink)),
                             o_samples = place(samples.size() * sizeof(float)), o_skip = place(skip.size() * sizeof(unsigned long long));
                std::vector<char> host(o_skip);
                std::memcpy(host.data() + o_prims, prims.data(), prims.size() * sizeof(vmv::PrepPrim));
                std::memcpy(host.data() + o_grid, grid_jobs.data(), grid_jobs.size() * sizeof(vmv::PrepGridJob));
                std::memcpy(host.data() + o_reach, reach_jobs.data(), reach_jobs.size() * sizeof(vmv::PrepReachJob));
                std::memcpy(host.data() + o_links, links.data(), links.size() * sizeof(vmv::PrepReachLink));
                std::memcpy(host.data() + o_samples, samples.data(), samples.size() * sizeof(float));
                VMV_HIP(hipMalloc(&d_tables, std::max<size_t>(at, 256)));
                char *t = static_cast<char *>(d_tables);
                if (!host.empty()) VMV_HIP(hipMemcpy(t, host.data(), host.size(), hipMemcpyHostToDevice));
                const vmv::PrepPrim *d_prims = reinterpret_cast<const vmv::PrepPrim *>(t + o_prims);
                if (!grid_jobs.empty())
                    if (int rc = vmv::launch_grid_fill(d_prims, reinterpret_cast<const vmv::PrepGridJob *>(t + o_grid), grid_jobs.data(),
                                                       grid_jobs.size(), d_cells, nullptr);
                        rc != VMV_OK)
                        return rc;
                if (!reach_jobs.empty() && !links.empty())
                {
                    unsigned long long *d_skip = reinterpret_cast<unsigned long long *>(t + o_skip);
                    if (int rc = vmv::launch_reach(d_prims, reinterpret_cast<const vmv::PrepReachJob *>(t + o_reach), reach_jobs.size(),
                                                   reinterpret_cast<const vmv::PrepReachLink *>(t + o_links), (uint32_t) links.size(),
                                                   reinterpret_cast<const float *>(t + o_samples), d_skip, nullptr);
                        rc != VMV_OK)
                        return rc;
                    VMV_HIP(hipMemcpy(skip.data(), d_skip, skip.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                    for (size_t i = 0; i < skip.size(); ++i) images[reach_env[i]].link_skip = skip[i];
                }
            }
            // static links (after the grids and certificates on the same stream: the kernel reads both)
            std::vector<vmv::EnvLaunch> launch(n);
            std::vector<const vmv::EnvLaunch *> launch_p(n);
            std::vector<vmv::EnvDev *> image_p(n);
            for (size_t k = 0; k < n; ++k)
            {
                launch[k].d_env = d_images + k, launch[k].host = images[k];
                launch_p[k] = &launch[k], image_p[k] = d_images + k;
            }
            if (int rc = robot_launchers(r).prepare_multi(launch_p.data(), image_p.data(), n, status.data()); rc != VMV_OK) return rc;
            VMV_HIP(hipDeviceSynchronize());
            return VMV_OK;
        }();
        if (rc != VMV_OK) error = g_last_error;
        if (d_tables)
        {
            (void) hipDeviceSynchronize();  // (a failed call may have kernels in flight that read the tables)
            (void) hipFree(d_tables);
        }
        for (size_t k = 0; k < n; ++k)
        {
            vmv_env *env = mine[k];
            std::lock_guard<std::mutex> lock(env->robot_mutex);
            const int st = rc != VMV_OK ? rc : status[k];
            env->launch[r].host = images[k];
            env->launch[r].d_env = d_images ? d_images + k : nullptr;
            if (keep) env->shared_allocations.push_back(keep);
            env->robot_status[r] = st;
            if (st != VMV_OK)
                env->robot_error[r] = rc != VMV_OK ? error : std::string("the environment exceeds the on-chip staging capacity");
            env->robot_state[r].store(kRobotBuilt, std::memory_order_release);
            env->robot_cv.notify_all();
        }
        for (vmv_env *env : theirs)
        {
            std::unique_lock<std::mutex> lock(env->robot_mutex);
            env->robot_cv.wait(lock, [&]() { return env->robot_state[r].load(std::memory_order_relaxed) == kRobotBuilt; });
        }
        for (size_t k = 0; k < n_envs; ++k)
            if (int st = robot_result(cenvs[k], r); st != VMV_OK) return st;
        return VMV_OK;
    }

    // vmv_clearance_batch*: the kinds a clearance is not defined for (include/vamp_mvt_amd.h), read from the host
    // builder, so the refusal needs neither a device nor a finalized environment; `who` names the argument
    int clearance_kinds(const vmv_env *env, const std::string &who)
    {
        const char *kind = !env->capts.empty() ? "a CAPT point cloud" :
                           !env->mvts.empty() ? "an MVT point cloud" :
                           (env->attached && !env->attach_spheres.empty()) ? "an attachment" : nullptr;
        if (!kind) return VMV_OK;
        g_last_error = who + " holds " + kind + ": a clearance is defined against primitives and heightfields only";
        return VMV_ERR_INVALID_ARGUMENT;
    }

    int refuse(int status, const std::string &message)
    {
        g_last_error = message;
        return status;
    }

    // What a prologue hands its entry point: `run` = launch; else return `rc` (an error, or VMV_OK: an empty batch).
    struct EnvCall
    {
        int rc = VMV_OK;
        bool run = false;
        const vmv::EnvLaunch *launch = nullptr;  // nullptr: no environment
    };
    enum CallKind
    {
        kInspect,  // reads the robot's part of the environment: no batch, any current device
        kDevice,   // device arrays in, launched on the caller's stream
        kHost      // host arrays in: asks for a device at all before the environment's is compared
    };

    // The single-environment prologue, in this order: robot, NULL pointers (`pointers`: the entry point's own arrays are
    // all there; a NULL `env` unless `optional`), finalized, n == 0, [kHost: a device at all,] the environment's device,
    // the robot's part of the environment.  `clearance`: the clearance calls' messages, and clearance_kinds before the
    // finalized check.
    EnvCall env_call(int robot, const vmv_env *env, bool optional, bool pointers, size_t n, CallKind kind, bool clearance = false)
    {
        if (!robot_ok(robot)) return {VMV_ERR_UNKNOWN_ROBOT};
        if (!pointers || (!env && !optional)) return {clearance ? refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer") : VMV_ERR_INVALID_ARGUMENT};
        if (env && clearance)
            if (int rc = clearance_kinds(env, "the environment"); rc != VMV_OK) return {rc};
        if (env && !env->finalized)
            return {clearance ? refuse(VMV_ERR_NOT_FINALIZED, "the environment is not finalized") : VMV_ERR_NOT_FINALIZED};
        if (n == 0) return {VMV_OK};
        if (kind == kHost)
            if (int rc = require_device(); rc != VMV_OK) return {rc};
        if (env && kind != kInspect)
            if (int rc = check_device(env); rc != VMV_OK) return {rc};
        if (env)
            if (int rc = ensure_robot(env, robot); rc != VMV_OK) return {rc};
        return {VMV_OK, true, env ? &env->launch[robot] : nullptr};
    }

    // per handle of a multi-environment call: NULL (and, given `offsets`, that they do not decrease), then for all of
    // them the kinds a clearance refuses, then finalized; each names the index
    int env_handles(const vmv_env *const *envs, size_t n_envs, const size_t *offsets, bool clearance)
    {
        for (size_t k = 0; k < n_envs; ++k)
            if (offsets && offsets[k + 1] < offsets[k])
                return refuse(VMV_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (offsets[" + std::to_string(k + 1) +
                                                            "] < offsets[" + std::to_string(k) + "])");
            else if (!envs[k])
                return refuse(VMV_ERR_INVALID_ARGUMENT, "envs[" + std::to_string(k) + "] is NULL");
        for (size_t k = 0; clearance && k < n_envs; ++k)
            if (int rc = clearance_kinds(envs[k], "envs[" + std::to_string(k) + "]"); rc != VMV_OK) return rc;
        for (size_t k = 0; k < n_envs; ++k)
            if (!envs[k]->finalized) return refuse(VMV_ERR_NOT_FINALIZED, "envs[" + std::to_string(k) + "] is not finalized");
        return VMV_OK;
    }

    // every environment on the current device, then the robot's parts of all of them (once per environment and robot)
    int prepare_parts(int robot, const vmv_env *const *envs, size_t n_envs)
    {
        for (size_t k = 0; k < n_envs; ++k)
            if (int rc = check_device(envs[k]); rc != VMV_OK) return rc;
        return build_robot_parts(envs, n_envs, robot);
    }

    struct MultiCall
    {
        int rc = VMV_OK;
        bool run = false;
        size_t n = 0;  // offsets[n_envs]
        std::vector<const vmv::EnvLaunch *> launch;
    };

    // The multi-environment prologue: robot, NULL arrays (q, q2: the inputs; out: the required output), the offsets,
    // env_handles, an empty batch; then the environments' device, the robot's parts and the launch vector - or, for a
    // `host` form, a device at all (it runs the device form once its arrays are up).
    MultiCall multi_call(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs, const void *q,
                         const void *q2, const void *out, bool host, bool clearance = false)
    {
        MultiCall c;
        if (!robot_ok(robot)) return c.rc = VMV_ERR_UNKNOWN_ROBOT, c;
        const char *err = (!envs || !offsets || !q || !q2 || !out) ? "null pointer" :
                          n_envs >= vmv::kMultiMaxConfigs ? "n_envs must be below 2^31" :
                          offsets[0] != 0 ? "offsets[0] must be 0" :
                          offsets[n_envs] >= vmv::kMultiMaxConfigs ? "offsets[n_envs] (the batch size) must be below 2^31" : nullptr;
        c.rc = err ? refuse(VMV_ERR_INVALID_ARGUMENT, err) : env_handles(envs, n_envs, offsets, clearance);
        if (c.rc != VMV_OK || (c.n = offsets[n_envs]) == 0) return c;
        if ((c.rc = host ? require_device() : prepare_parts(robot, envs, n_envs)) != VMV_OK) return c;
        for (size_t k = 0; !host && k < n_envs; ++k) c.launch.push_back(&envs[k]->launch[robot]);
        c.run = true;
        return c;
    }
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// device memory of the host-buffer entry points, and the gradient calls' witness scratch
// ---------------------------------------------------------------------------------------------------------
namespace
{
    // Device staging of the *_host entry points: one grow-only arena per thread, so that a planner's many small calls
    // (one configuration, a handful of edges) do not pay hipMalloc / hipFree pairs each.  Never freed from a
    // destructor: a thread_local of the main thread is destroyed during static destruction, possibly after the HIP
    // runtime is gone (the memory goes back with the process).  Long-lived callers release it with
    // vmv_release_staging(); a request above kStagingKeepBytes is not kept beyond its call, so one huge batch does not
    // pin its memory for the thread's life.
    constexpr size_t kStagingKeepBytes = size_t{64} << 20;
    struct StagingArena
    {
        void *base = nullptr;
        size_t capacity = 0;
        int device = -1;
        void release()
        {
            if (base) (void) hipFree(base);
            base = nullptr;
            capacity = 0;
        }
        void *get(size_t bytes)
        {
            int dev = -1;
            if (hipGetDevice(&dev) != hipSuccess) return nullptr;
            if (base && (dev != device || bytes > capacity)) release();
            if (!base)
            {
                const size_t want = std::max<size_t>(bytes, 1u << 16);
                if (hipMalloc(&base, want) != hipSuccess)
                {
                    base = nullptr;
                    return nullptr;
                }
                capacity = want;
                device = dev;
            }
            return base;
        }
        void trim()
        {
            if (capacity > kStagingKeepBytes) release();
        }
    };
    thread_local StagingArena g_staging;

    // One host round trip through the arena.  The caller declares its device regions: in() is uploaded from host
    // memory, out() is downloaded once the call has returned VMV_OK (dst NULL: a plain temporary; `room`: laid out,
    // and with `zero` cleared, at least this large).  run() lays them out at 256-byte alignment in one arena request,
    // uploads, runs `call` - which reads the device pointers with at() and launches on the null stream, so that the
    // synchronous copies order with it - downloads, and trims the arena on every path.  A region without bytes is NULL.
    struct Staged
    {
        struct Region
        {
            const void *src;
            void *dst;
            size_t bytes, room;
            bool zero;
            void *ptr;
        };
        Region regions[6];
        int count = 0;
        int add(const void *src, void *dst, size_t bytes, size_t room, bool zero)
        {
            regions[count] = {src, dst, bytes, std::max(bytes, room), zero, nullptr};
            return count++;
        }
        int in(const void *src, size_t bytes) { return add(src, nullptr, bytes, 0, false); }
        int out(void *dst, size_t bytes, size_t room = 0, bool zero = false) { return add(nullptr, dst, bytes, room, zero); }
        template <typename T>
        T *at(int region) const
        {
            return static_cast<T *>(regions[region].ptr);
        }
        template <typename F>
        int run(F &&call)
        {
            const auto padded = [](const Region &r) { return (r.room + 255) & ~size_t{255}; };
            size_t total = 0;
            for (int i = 0; i < count; ++i) total += padded(regions[i]);
            char *p = static_cast<char *>(g_staging.get(total));
            if (!p) return hip_fail(hipErrorOutOfMemory, "staging arena");
            bool ok = true;
            for (int i = 0; i < count && ok; ++i)
            {
                Region &r = regions[i];
                r.ptr = r.room ? p : nullptr;
                p += padded(r);
                if (r.src && r.bytes) ok = hipMemcpy(r.ptr, r.src, r.bytes, hipMemcpyHostToDevice) == hipSuccess;
                if (r.zero && r.room) ok = ok && hipMemset(r.ptr, 0, r.room) == hipSuccess;
            }
            int rc = ok ? call() : VMV_ERR_HIP;
            for (int i = 0; i < count && rc == VMV_OK; ++i)
                if (const Region &r = regions[i]; r.dst && r.bytes && hipMemcpy(r.dst, r.ptr, r.bytes, hipMemcpyDeviceToHost) != hipSuccess)
                    rc = VMV_ERR_HIP;
            g_staging.trim();
            return rc;
        }
    };

    size_t config_bytes(int robot, size_t n) { return n * (size_t) kRobots[robot].dimension * sizeof(float); }

    // The gradient kernel reads the witness the clearance kernel wrote.  A caller without a witness buffer is lent scratch
    // per (device, stream): calls on one stream run in order, so they share it; grow-only, a larger request frees the old
    // buffer (hipFree waits for the calls still using it).  The lease holds the pool's lock until the call is enqueued.
    struct WitnessScratch
    {
        void *p = nullptr;
        size_t bytes = 0;
    };
    std::mutex g_witness_mutex;
    std::map<std::pair<int, hipStream_t>, WitnessScratch> g_witness;  // never freed at exit (see vmv_release_staging)
    struct WitnessLease
    {
        std::unique_lock<std::mutex> lock{g_witness_mutex, std::defer_lock};
        int acquire(hipStream_t stream, size_t n, uint32_t **out)
        {
            int dev = -1;
            VMV_HIP(hipGetDevice(&dev));
            lock.lock();
            WitnessScratch &w = g_witness[{dev, stream}];
            if (w.bytes < n * 16)
            {
                if (w.p) (void) hipFree(w.p);
                w.p = nullptr, w.bytes = 0;
                const size_t want = std::max<size_t>(n * 16, size_t{1} << 16);
                VMV_HIP(hipMalloc(&w.p, want));
                w.bytes = want;
            }
            *out = static_cast<uint32_t *>(w.p);
            return VMV_OK;
        }
    };
    void release_witness_scratch()
    {
        std::lock_guard<std::mutex> g(g_witness_mutex);
        for (auto &kv : g_witness)
            if (kv.second.p) (void) hipFree(kv.second.p);
        g_witness.clear();
    }
    // the round trip of the four clearance host forms: [configurations | clearances | gradients | witness]; grad NULL: the values
    // alone, and a witness only where the caller wants one; launch(d_q, d_clearance, d_grad, d_witness)
    template <typename F>
    int clearance_staged(int robot, const float *q, size_t n, float *clearance, float *grad, uint32_t *witness, F &&launch)
    {
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), dc = s.out(clearance, n * 8), dg = s.out(grad, grad ? 2 * config_bytes(robot, n) : 0),
                  dw = s.out(witness, grad || witness ? n * 16 : 0);
        return s.run([&] { return launch(s.at<float>(dq), s.at<float>(dc), s.at<float>(dg), s.at<uint32_t>(dw)); });
    }

    // launch(the caller's witness buffer, or one lent until the call is enqueued)
    template <typename F>
    int with_witness(uint32_t *d_witness, size_t n, void *stream, F &&launch)
    {
        WitnessLease lease;
        if (!d_witness)
            if (int rc = lease.acquire(static_cast<hipStream_t>(stream), n, &d_witness); rc != VMV_OK) return rc;
        return launch(d_witness);
    }

    // free spheres (and, given robot_spheres, one configuration's) against the environment: vmv::spheres_env_kernel
    int launch_spheres(const vmv_env *env, const float *d_spheres, size_t n, uint8_t *d_hits, const float *d_robot_spheres,
                       int n_robot, void *stream)
    {
        const size_t blocks = (n + vmv::kBlock - 1) / vmv::kBlock;
        hipLaunchKernelGGL(vmv::spheres_env_kernel, dim3((unsigned) std::min<size_t>(blocks, 4096)), dim3(vmv::kBlock),
                           (env->base.n_floats + vmv::kCaptFlagWords) * sizeof(float), static_cast<hipStream_t>(stream), env->launch[0].d_env,
                           reinterpret_cast<const float4 *>(d_spheres), n, d_hits, reinterpret_cast<const float4 *>(d_robot_spheres), n_robot);
        VMV_HIP(hipGetLastError());
        return VMV_OK;
    }

    // vmv_ik_batch without the caller's seeds: the robot's bounds and n_seeds Halton samples in scratch per (device,
    // stream), [lower 16 | span 16 | seeds 1,024 x 16 floats] - its full size from the start, so it never moves.  Calls on
    // one stream run in order and share it; the bounds are uploaded when the entry last served another robot.  The lease
    // holds the pool's lock until the call is enqueued.
    constexpr size_t kIkMaxSeeds = 1024;
    struct IkSeedScratch
    {
        float *p = nullptr;
        int robot = -1;
    };
    std::mutex g_ik_mutex;
    std::map<std::pair<int, hipStream_t>, IkSeedScratch> g_ik_seeds;  // never freed at exit (see vmv_release_staging)
    struct IkSeedLease
    {
        std::unique_lock<std::mutex> lock{g_ik_mutex, std::defer_lock};
        int acquire(hipStream_t stream, int robot, float **out)
        {
            int dev = -1;
            VMV_HIP(hipGetDevice(&dev));
            lock.lock();
            IkSeedScratch &w = g_ik_seeds[{dev, stream}];
            if (!w.p) VMV_HIP(hipMalloc((void **) &w.p, (32 + kIkMaxSeeds * 16) * sizeof(float)));
            if (w.robot != robot)
            {
                w.robot = -1;
                VMV_HIP(hipMemcpyAsync(w.p, kRobots[robot].lower, 16 * sizeof(float), hipMemcpyHostToDevice, stream));
                VMV_HIP(hipMemcpyAsync(w.p + 16, kRobots[robot].span, 16 * sizeof(float), hipMemcpyHostToDevice, stream));
                w.robot = robot;
            }
            *out = w.p;
            return VMV_OK;
        }
    };
    void release_ik_scratch()
    {
        std::lock_guard<std::mutex> g(g_ik_mutex);
        for (auto &kv : g_ik_seeds)
            if (kv.second.p) (void) hipFree(kv.second.p);
        g_ik_seeds.clear();
    }

    // The checks of vmv_ik_batch that need no device, in the header's order; fills the kernel's parameter block.
    int ik_checks(int robot, const float *targets, size_t n_targets, const float *seeds, uint64_t halton_skip,
                  const vmv_ik_settings *s, const float *q, const uint32_t *status, vmv::IkParams &P)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!targets || !s || !q || !status) return refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer");
        const auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
        const char *err = (s->n_seeds < 1u || s->n_seeds > (uint32_t) kIkMaxSeeds) ? "n_seeds must be 1 .. 1024" :
                          (s->max_iterations < 1u || s->max_iterations >= (1u << 30)) ? "max_iterations must be 1 .. 2^30 - 1" :
                          !positive(s->pos_tol) ? "pos_tol must be finite and positive" :
                          !positive(s->rot_tol) ? "rot_tol must be finite and positive" :
                          !positive(s->rot_weight) ? "rot_weight must be finite and positive" :
                          !positive(s->damping) ? "damping must be finite and positive" :
                          !positive(s->max_step) ? "max_step must be finite and positive" :
                          (s->position_only != 0 && s->position_only != 1) ? "position_only must be 0 or 1" :
                          (!seeds && (halton_skip > 1000000ull || halton_skip + s->n_seeds > 1000000ull)) ?
                          "halton_skip + n_seeds must not exceed 1,000,000" :
                          n_targets > (vmv::kMultiMaxConfigs - 1) / s->n_seeds ? "n_targets * n_seeds must be below 2^31" : nullptr;
        if (err) return refuse(VMV_ERR_INVALID_ARGUMENT, err);
        P.n_seeds = s->n_seeds, P.max_iterations = s->max_iterations;
        P.pos_tol = s->pos_tol, P.rot_tol = s->rot_tol, P.rot_weight = s->position_only ? 0.0f : s->rot_weight;
        P.damping = s->damping, P.max_step = s->max_step;
        P.position_only = (uint32_t) s->position_only, P.seeds_shared = seeds ? 0u : 1u;
        for (int j = 0; j < 16; ++j) P.lower[j] = kRobots[robot].lower[j], P.upper[j] = kRobots[robot].lower[j] + kRobots[robot].span[j];
        return VMV_OK;
    }

    // The checks of the vmv_constraint_*_batch calls, none of which needs a device, in the header's order; fills the
    // kernels' parameter block; the device records (one, or one per lane) are built once the call holds its pinned table.
    int constraint_checks(int robot, bool arrays, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                          const vmv_constraint_settings *settings, vmv::ConstraintBand &c)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!arrays) return refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer");
        const std::string err = vmv::constraint_band_checks(constraints, n_constraints, settings, n, "n",
                                                            n >= vmv::kMultiMaxConfigs ? "n must be below 2^31" : nullptr, c);
        if (!err.empty()) return refuse(VMV_ERR_INVALID_ARGUMENT, err);
        vmv::constraint_band_bounds(c, kRobots[robot].lower, kRobots[robot].span, kRobots[robot].dimension);
        return VMV_OK;
    }
    // the records built straight into the stream's pinned table, uploaded, then launch(d_records, stream); the _host forms
    // come here after their own prologue (the null stream, so that the staged copies order with the launch)
    template <typename F>
    int constraint_launch(const vmv::ConstraintBand &c, hipStream_t stream, F &&launch)
    {
        vmv::MultiTableLease lease;
        const size_t bytes = c.count * sizeof(vmv::ConstraintDev);
        if (int rc = lease.acquire(stream, bytes); rc != VMV_OK) return rc;
        vmv::constraint_band_records(c, static_cast<vmv::ConstraintDev *>(lease.host));
        if (int rc = lease.upload(stream, bytes); rc != VMV_OK) return rc;
        return launch(static_cast<const vmv::ConstraintDev *>(lease.dev), stream);
    }

    // bench / sampling input generators: uploads the robot's bounds, launches `kernel` on the stream, waits for it
    using ConfigKernel = void (*)(float *, size_t, int, uint64_t, const float *, const float *);
    int generate_configs(int robot, ConfigKernel kernel, uint64_t seed_or_skip, float *d_q, size_t n, void *stream)
    {
        const int dim = kRobots[robot].dimension;
        float *d_bounds = nullptr;
        VMV_HIP(hipMalloc((void **) &d_bounds, 32 * sizeof(float)));
        const int rc = [&]() -> int
        {
            VMV_HIP(hipMemcpy(d_bounds, kRobots[robot].lower, 16 * sizeof(float), hipMemcpyHostToDevice));
            VMV_HIP(hipMemcpy(d_bounds + 16, kRobots[robot].span, 16 * sizeof(float), hipMemcpyHostToDevice));
            const size_t total = n * (size_t) dim;
            hipLaunchKernelGGL(kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_q,
                               total, dim, seed_or_skip, d_bounds, d_bounds + 16);
            VMV_HIP(hipGetLastError());
            VMV_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
            return VMV_OK;
        }();
        (void) hipFree(d_bounds);
        return rc;
    }
}  // namespace

// ---------------------------------------------------------------------------------------------------------
// batched entry points
// ---------------------------------------------------------------------------------------------------------
extern "C"
{
    static int validate_parts(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, void *stream, int parts)
    {
        const EnvCall c = env_call(robot, env, false, d_q && d_bits, n, kDevice);
        if (!c.run) return c.rc;
        return robot_launchers(robot).validate(*c.launch, d_q, n, d_bits, static_cast<hipStream_t>(stream), parts);
    }
    int vmv_validate_batch(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, void *stream)
    {
        return validate_parts(robot, env, d_q, n, d_bits, stream, 7);
    }
    int vmv_validate_batch_env(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, void *stream)
    {
        return validate_parts(robot, env, d_q, n, d_bits, stream, 1);
    }

    int vmv_validate_batch_self(int robot, const float *d_q, size_t n, uint64_t *d_bits, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || !d_bits) return VMV_ERR_INVALID_ARGUMENT;
        if (n == 0) return VMV_OK;
        return robot_launchers(robot).validate(vmv::EnvLaunch{}, d_q, n, d_bits, static_cast<hipStream_t>(stream), 2);
    }

    int vmv_self_screen_flags(int robot, const float *d_q, size_t n, int mode, uint64_t *d_words, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || !d_words || (mode != 0 && mode != 1) || n >= (size_t{1} << 31)) return VMV_ERR_INVALID_ARGUMENT;
        if (n == 0) return VMV_OK;
        return robot_launchers(robot).self_screen_flags(d_q, n, mode, d_words, static_cast<hipStream_t>(stream));
    }

    int vmv_bare_trig_error(uint32_t lo_bits, uint32_t hi_bits, float *out2, void *stream)
    {
        // positive, finite, ordered: the bit patterns of positive floats are ordered as the floats are
        if (!out2 || lo_bits > hi_bits || hi_bits >= 0x7f800000u) return VMV_ERR_INVALID_ARGUMENT;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        const uint64_t count = (uint64_t) hi_bits - lo_bits + 1u;
        const uint32_t blocks = (uint32_t) std::min<uint64_t>((count + vmv::kBlock - 1) / vmv::kBlock, vmv::kTrigBlocks);
        float *d = nullptr;  // [2 * blocks] partials, then the two results
        VMV_HIP(hipMalloc((void **) &d, (2 * (size_t) blocks + 2) * sizeof(float)));
        const int rc = [&]() -> int
        {
            hipLaunchKernelGGL(vmv::trig_error_kernel, dim3(blocks), dim3(vmv::kBlock), 0, s, lo_bits, hi_bits, d);
            hipLaunchKernelGGL(vmv::trig_error_final_kernel, dim3(1), dim3(vmv::kBlock), 0, s, (const float *) d, blocks, d + 2 * (size_t) blocks);
            VMV_HIP(hipGetLastError());
            VMV_HIP(hipMemcpyAsync(out2, d + 2 * (size_t) blocks, 2 * sizeof(float), hipMemcpyDeviceToHost, s));
            VMV_HIP(hipStreamSynchronize(s));
            return VMV_OK;
        }();
        (void) hipFree(d);
        return rc;
    }

    int vmv_validate_motion_batch(int robot, const vmv_env *env, const float *d_a, const float *d_b, size_t n,
                                  uint64_t *d_bits, void *stream)
    {
        const EnvCall c = env_call(robot, env, false, d_a && d_b && d_bits, n, kDevice);
        if (!c.run) return c.rc;
        return robot_launchers(robot).validate_motion(*c.launch, d_a, d_b, n, d_bits, static_cast<hipStream_t>(stream));
    }

    int vmv_validate_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                 const float *d_q, uint64_t *d_bits, void *stream)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, d_q, d_q, d_bits, false);
        if (!c.run) return c.rc;
        return robot_launchers(robot).validate_multi(c.launch.data(), offsets, n_envs, d_q, d_bits, static_cast<hipStream_t>(stream));
    }

    int vmv_validate_motion_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                        const float *d_start, const float *d_goal, uint64_t *d_bits, void *stream)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, d_start, d_goal, d_bits, false);
        if (!c.run) return c.rc;
        return robot_launchers(robot).validate_motion_multi(c.launch.data(), offsets, n_envs, d_start, d_goal, d_bits,
                                                            static_cast<hipStream_t>(stream));
    }

    int vmv_env_prepare_multi(int robot, const vmv_env *const *envs, size_t n_envs)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (n_envs == 0) return VMV_OK;
        if (!envs) return refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer");
        if (int rc = env_handles(envs, n_envs, nullptr, false); rc != VMV_OK) return rc;
        return prepare_parts(robot, envs, n_envs);
    }

    int vmv_env_grid_info(const vmv_env *env, int robot, int grid_class, uint32_t *dims3, float *origin3, float *inv_cell,
                          uint32_t *words)
    {
        const EnvCall c = env_call(robot, env, false, grid_class >= 0 && grid_class < vmv::kGridClasses, 1, kInspect);
        if (!c.run) return c.rc;
        const vmv::EnvDev &D = c.launch->host;
        const vmv::GridDev &g = D.grid[grid_class];
        const bool has = g.cells != nullptr;
        for (int k = 0; k < 3; ++k)
        {
            if (dims3) dims3[k] = has ? g.dims[k] : 0u;
            if (origin3) origin3[k] = has ? g.origin[k] : 0.f;
        }
        if (inv_cell) *inv_cell = has ? g.inv_cell : 0.f;
        if (words) *words = has ? D.grid_words : 0u;
        return VMV_OK;
    }
    int vmv_env_grid_cells(const vmv_env *env, int robot, int grid_class, uint32_t *out, size_t capacity, size_t *n)
    {
        const EnvCall c = env_call(robot, env, false, n && grid_class >= 0 && grid_class < vmv::kGridClasses, 1, kInspect);
        if (!c.run) return c.rc;
        const vmv::EnvDev &D = c.launch->host;
        const vmv::GridDev &g = D.grid[grid_class];
        *n = g.cells ? (size_t) g.dims[0] * g.dims[1] * g.dims[2] * D.grid_words : 0;
        const size_t m = std::min(capacity, *n);
        if (out && m) VMV_HIP(hipMemcpy(out, g.cells, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return VMV_OK;
    }
    int vmv_env_robot_flags(const vmv_env *env, int robot, uint64_t *link_skip, uint32_t *static_hit)
    {
        const EnvCall c = env_call(robot, env, false, true, 1, kInspect);
        if (!c.run) return c.rc;
        if (link_skip) *link_skip = c.launch->host.link_skip;
        if (static_hit)  // (the kernel's answer lives in the device image only)
            VMV_HIP(hipMemcpy(static_hit, &c.launch->d_env->static_hit, sizeof(uint32_t), hipMemcpyDeviceToHost));
        return VMV_OK;
    }

    int vmv_robot_self_pairs(int robot, size_t *n_pairs, uint16_t *pairs2)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!n_pairs) return VMV_ERR_INVALID_ARGUMENT;
        *n_pairs = (size_t) kRobots[robot].n_self_pairs;
        if (pairs2) std::memcpy(pairs2, kRobots[robot].self_pairs, *n_pairs * 4);
        return VMV_OK;
    }
    int vmv_env_report_layout(const vmv_env *env, uint32_t *w)
    {
        if (!env || !w) return VMV_ERR_INVALID_ARGUMENT;
        if (!env->finalized) return VMV_ERR_NOT_FINALIZED;
        const vmv::EnvDev &D = env->base;
        uint32_t base = 0;
        const uint32_t counts[5] = {D.n_sphere, D.n_capsule, D.n_zcapsule, D.n_cuboid, D.n_zcuboid};
        for (int i = 0; i < 5; ++i)
        {
            w[i] = base;
            base += (counts[i] + 31u) / 32u;
        }
        return VMV_OK;
    }

    int vmv_fk_batch(int robot, const float *d_q, size_t n, float *d_out, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || !d_out) return VMV_ERR_INVALID_ARGUMENT;
        if (n == 0) return VMV_OK;
        return robot_launchers(robot).fk(d_q, n, d_out, static_cast<hipStream_t>(stream));
    }
    int vmv_eefk_batch(int robot, const float *d_q, size_t n, float *d_out, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || !d_out) return VMV_ERR_INVALID_ARGUMENT;
        if (n == 0) return VMV_OK;
        return robot_launchers(robot).eefk(d_q, n, d_out, static_cast<hipStream_t>(stream));
    }

    // ---- host-buffer variants: their own arrays and a device are checked here, the rest by the device form they run ----
    int vmv_fk_batch_host(int robot, const float *q, size_t n, float *out)
    {
        const EnvCall c = env_call(robot, nullptr, true, q && out, n, kHost);
        if (!c.run) return c.rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), dout = s.out(out, n * (size_t) kRobots[robot].n_spheres * 16);
        return s.run([&] { return vmv_fk_batch(robot, s.at<float>(dq), n, s.at<float>(dout), nullptr); });
    }
    int vmv_eefk_batch_host(int robot, const float *q, size_t n, float *out)
    {
        const EnvCall c = env_call(robot, nullptr, true, q && out, n, kHost);
        if (!c.run) return c.rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), dout = s.out(out, n * 64);
        return s.run([&] { return vmv_eefk_batch(robot, s.at<float>(dq), n, s.at<float>(dout), nullptr); });
    }
    int vmv_validate_batch_host(int robot, const vmv_env *env, const float *q, size_t n, uint64_t *bits)
    {
        const EnvCall c = env_call(robot, nullptr, true, q && bits, n, kHost);
        if (!c.run) return c.rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), dbits = s.out(bits, (n + 63) / 64 * 8);
        return s.run([&] { return vmv_validate_batch(robot, env, s.at<float>(dq), n, s.at<uint64_t>(dbits), nullptr); });
    }
    int vmv_validate_motion_batch_host(int robot, const vmv_env *env, const float *a, const float *b, size_t n,
                                       uint64_t *bits)
    {
        if (!b) return VMV_ERR_INVALID_ARGUMENT;
        const EnvCall c = env_call(robot, nullptr, true, a && bits, n, kHost);
        if (!c.run) return c.rc;
        Staged s;
        const int da = s.in(a, config_bytes(robot, n)), db = s.in(b, config_bytes(robot, n)), dbits = s.out(bits, (n + 63) / 64 * 8);
        return s.run([&]
                     { return vmv_validate_motion_batch(robot, env, s.at<float>(da), s.at<float>(db), n, s.at<uint64_t>(dbits), nullptr); });
    }
    int vmv_validate_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                      const float *q, uint64_t *bits)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, q, q, bits, true);
        if (!c.run) return c.rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, c.n)), dbits = s.out(bits, (c.n + 63) / 64 * 8);
        return s.run([&]
                     { return vmv_validate_batch_multi(robot, envs, offsets, n_envs, s.at<float>(dq), s.at<uint64_t>(dbits), nullptr); });
    }
    int vmv_validate_motion_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                             const float *start, const float *goal, uint64_t *bits)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, start, goal, bits, true);
        if (!c.run) return c.rc;
        Staged s;
        const int da = s.in(start, config_bytes(robot, c.n)), db = s.in(goal, config_bytes(robot, c.n)),
                  dbits = s.out(bits, (c.n + 63) / 64 * 8);
        return s.run([&]
                     {
                         return vmv_validate_motion_batch_multi(robot, envs, offsets, n_envs, s.at<float>(da), s.at<float>(db),
                                                                s.at<uint64_t>(dbits), nullptr);
                     });
    }
    int vmv_contacts_batch_host(int robot, const vmv_env *env, const float *q, size_t n, uint32_t *env_words,
                                uint32_t *pair_words)
    {
        const EnvCall c = env_call(robot, env, false, q && env_words && pair_words, n, kHost);
        if (!c.run) return c.rc;
        const size_t ns = (size_t) kRobots[robot].n_spheres, npw = ((size_t) robot_launchers(robot).n_self_pairs + 31) / 32;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), ds = s.out(nullptr, n * ns * 16),
                  de = s.out(env_words, n * ns * (vmv::kReportWords + 1) * 4), dp = s.out(pair_words, n * npw * 4, 4, true);
        return s.run([&]
                     {
                         const int rc = robot_launchers(robot).fk(s.at<float>(dq), n, s.at<float>(ds), nullptr);
                         return rc != VMV_OK ? rc : robot_launchers(robot).contacts(*c.launch, s.at<float>(ds), n, s.at<uint32_t>(de),
                                                                                  s.at<uint32_t>(dp), nullptr);
                     });
    }

    int vmv_release_staging(void)
    {
        g_staging.release();
        release_witness_scratch();
        release_ik_scratch();
        vmv::release_edge_scratch();  // (waits for the edge batches still in flight: hipFree synchronizes)
        vmv::release_multi_tables();
        return VMV_OK;
    }

    // ---- clearances and their gradients (include/vamp_mvt_amd.h: vmv_clearance_batch, vmv_clearance_grad_batch) ----
    int vmv_clearance_batch(int robot, const vmv_env *env, const float *d_q, size_t n, float *d_clearance, uint32_t *d_witness,
                            void *stream)
    {
        const EnvCall c = env_call(robot, env, true, d_q && d_clearance, n, kDevice, true);
        if (!c.run) return c.rc;
        return robot_launchers(robot).clearance(c.launch, d_q, n, d_clearance, d_witness, static_cast<hipStream_t>(stream));
    }
    int vmv_clearance_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                                  float *d_clearance, uint32_t *d_witness, void *stream)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, d_q, d_q, d_clearance, false, true);
        if (!c.run) return c.rc;
        return robot_launchers(robot).clearance_multi(c.launch.data(), offsets, n_envs, d_q, d_clearance, d_witness,
                                                      static_cast<hipStream_t>(stream));
    }
    int vmv_clearance_grad_batch(int robot, const vmv_env *env, const float *d_q, size_t n, float *d_clearance, float *d_grad,
                                 uint32_t *d_witness, void *stream)
    {
        const EnvCall c = env_call(robot, env, true, d_q && d_grad && d_clearance, n, kDevice, true);
        if (!c.run) return c.rc;
        return with_witness(d_witness, n, stream, [&](uint32_t *witness)
                            {
                                return robot_launchers(robot).clearance_grad(c.launch, d_q, n, d_clearance, d_grad, witness,
                                                                             static_cast<hipStream_t>(stream));
                            });
    }
    int vmv_clearance_grad_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                       const float *d_q, float *d_clearance, float *d_grad, uint32_t *d_witness, void *stream)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, d_q, d_grad, d_clearance, false, true);
        if (!c.run) return c.rc;
        return with_witness(d_witness, c.n, stream, [&](uint32_t *witness)
                            {
                                return robot_launchers(robot).clearance_grad_multi(c.launch.data(), offsets, n_envs, d_q, d_clearance,
                                                                                   d_grad, witness, static_cast<hipStream_t>(stream));
                            });
    }
    int vmv_clearance_batch_host(int robot, const vmv_env *env, const float *q, size_t n, float *clearance, uint32_t *witness)
    {
        const EnvCall c = env_call(robot, env, true, q && clearance, n, kHost, true);
        if (!c.run) return c.rc;
        return clearance_staged(robot, q, n, clearance, nullptr, witness, [&](float *dq, float *dc, float *, uint32_t *dw)
                                { return robot_launchers(robot).clearance(c.launch, dq, n, dc, dw, nullptr); });
    }
    int vmv_clearance_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs, const float *q,
                                       float *clearance, uint32_t *witness)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, q, q, clearance, true, true);
        if (!c.run) return c.rc;
        return clearance_staged(robot, q, c.n, clearance, nullptr, witness, [&](float *dq, float *dc, float *, uint32_t *dw)
                                { return vmv_clearance_batch_multi(robot, envs, offsets, n_envs, dq, dc, dw, nullptr); });
    }
    int vmv_clearance_grad_batch_host(int robot, const vmv_env *env, const float *q, size_t n, float *clearance, float *grad,
                                      uint32_t *witness)
    {
        const EnvCall c = env_call(robot, env, true, q && grad && clearance, n, kHost, true);
        if (!c.run) return c.rc;
        return clearance_staged(robot, q, n, clearance, grad, witness, [&](float *dq, float *dc, float *dg, uint32_t *dw)
                                { return robot_launchers(robot).clearance_grad(c.launch, dq, n, dc, dg, dw, nullptr); });
    }
    int vmv_clearance_grad_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                            const float *q, float *clearance, float *grad, uint32_t *witness)
    {
        const MultiCall c = multi_call(robot, envs, offsets, n_envs, q, grad, clearance, true, true);
        if (!c.run) return c.rc;
        return clearance_staged(robot, q, c.n, clearance, grad, witness, [&](float *dq, float *dc, float *dg, uint32_t *dw)
                                { return vmv_clearance_grad_batch_multi(robot, envs, offsets, n_envs, dq, dc, dg, dw, nullptr); });
    }

    // ---- end-effector Jacobian and inverse kinematics (include/vamp_mvt_amd.h: vmv_eefk_jacobian_batch, vmv_ik_batch) ----
    int vmv_eefk_jacobian_batch(int robot, const float *d_q, size_t n, float *d_frames, float *d_jac, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || !d_jac) return refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer");
        if (n == 0) return VMV_OK;
        return robot_launchers(robot).eefk_jacobian(d_q, n, d_frames, d_jac, static_cast<hipStream_t>(stream));
    }
    int vmv_eefk_jacobian_batch_host(int robot, const float *q, size_t n, float *frames, float *jac)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!q || !jac) return refuse(VMV_ERR_INVALID_ARGUMENT, "null pointer");
        if (n == 0) return VMV_OK;
        if (int rc = require_device(); rc != VMV_OK) return rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), df = s.out(frames, frames ? n * 64 : 0), dj = s.out(jac, 6 * config_bytes(robot, n));
        return s.run([&] { return vmv_eefk_jacobian_batch(robot, s.at<float>(dq), n, s.at<float>(df), s.at<float>(dj), nullptr); });
    }
    int vmv_ik_batch(int robot, const float *d_targets, size_t n_targets, const float *d_seeds, uint64_t halton_skip,
                     const vmv_ik_settings *settings, float *d_q, float *d_err, uint32_t *d_status, void *stream)
    {
        vmv::IkParams P;
        if (int rc = ik_checks(robot, d_targets, n_targets, d_seeds, halton_skip, settings, d_q, d_status, P); rc != VMV_OK) return rc;
        if (n_targets == 0) return VMV_OK;
        const hipStream_t st = static_cast<hipStream_t>(stream);
        const size_t n = n_targets * (size_t) P.n_seeds;
        if (d_seeds) return robot_launchers(robot).ik(P, d_targets, d_seeds, n, d_q, d_err, d_status, st);
        IkSeedLease lease;
        float *scratch = nullptr;
        if (int rc = lease.acquire(st, robot, &scratch); rc != VMV_OK) return rc;
        const size_t total = (size_t) P.n_seeds * (size_t) kRobots[robot].dimension;
        hipLaunchKernelGGL(vmv::halton_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, scratch + 32, total,
                           kRobots[robot].dimension, halton_skip, scratch, scratch + 16);
        VMV_HIP(hipGetLastError());
        return robot_launchers(robot).ik(P, d_targets, scratch + 32, n, d_q, d_err, d_status, st);
    }
    int vmv_ik_batch_host(int robot, const float *targets, size_t n_targets, const float *seeds, uint64_t halton_skip,
                          const vmv_ik_settings *settings, float *q, float *err, uint32_t *status)
    {
        vmv::IkParams P;
        if (int rc = ik_checks(robot, targets, n_targets, seeds, halton_skip, settings, q, status, P); rc != VMV_OK) return rc;
        if (n_targets == 0) return VMV_OK;
        if (int rc = require_device(); rc != VMV_OK) return rc;
        const size_t n = n_targets * (size_t) P.n_seeds;
        Staged s;
        const int dt = s.in(targets, n_targets * 64), ds = s.in(seeds, seeds ? config_bytes(robot, n) : 0), dq = s.out(q, config_bytes(robot, n)),
                  de = s.out(err, err ? n * 8 : 0), dst = s.out(status, n * 4);
        return s.run([&]
                     {
                         return vmv_ik_batch(robot, s.at<float>(dt), n_targets, s.at<float>(ds), halton_skip, settings, s.at<float>(dq),
                                             s.at<float>(de), s.at<uint32_t>(dst), nullptr);
                     });
    }

    // ---- end-effector constraints (include/vamp_mvt_amd.h: vmv_constraint_*_batch; csrc/vmv_constraint.h) ----
    int vmv_constraint_project_batch(int robot, const float *d_q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                                     const vmv_constraint_settings *settings, float *d_q_out, float *d_residuals, uint32_t *d_status,
                                     void *stream)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, d_q && d_q_out && d_status, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        return constraint_launch(c, static_cast<hipStream_t>(stream), [&](const vmv::ConstraintDev *d_cons, hipStream_t st)
                                 { return robot_launchers(robot).constraint_project(c.P, d_cons, d_q, n, d_q_out, d_residuals, d_status, st); });
    }
    int vmv_constraint_project_batch_host(int robot, const float *q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                                          const vmv_constraint_settings *settings, float *q_out, float *residuals, uint32_t *status)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, q && q_out && status, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        if (int rc = require_device(); rc != VMV_OK) return rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), dout = s.out(q_out, config_bytes(robot, n)),
                  dr = s.out(residuals, residuals ? n * 8 : 0), dst = s.out(status, n * 4);
        return s.run([&]
                     {
                         return constraint_launch(c, nullptr, [&](const vmv::ConstraintDev *d_cons, hipStream_t st) {
                             return robot_launchers(robot).constraint_project(c.P, d_cons, s.at<float>(dq), n, s.at<float>(dout), s.at<float>(dr),
                                                                              s.at<uint32_t>(dst), st);
                         });
                     });
    }
    int vmv_constraint_check_batch(int robot, const float *d_q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                                   const vmv_constraint_settings *settings, uint64_t *d_bits, float *d_residuals, void *stream)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, d_q && d_bits, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        return constraint_launch(c, static_cast<hipStream_t>(stream), [&](const vmv::ConstraintDev *d_cons, hipStream_t st)
                                 { return robot_launchers(robot).constraint_check(c.P, d_cons, d_q, n, d_bits, d_residuals, st); });
    }
    int vmv_constraint_check_batch_host(int robot, const float *q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                                        const vmv_constraint_settings *settings, uint64_t *bits, float *residuals)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, q && bits, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        if (int rc = require_device(); rc != VMV_OK) return rc;
        Staged s;
        const int dq = s.in(q, config_bytes(robot, n)), db = s.out(bits, (n + 63) / 64 * 8), dr = s.out(residuals, residuals ? n * 8 : 0);
        return s.run([&]
                     {
                         return constraint_launch(c, nullptr, [&](const vmv::ConstraintDev *d_cons, hipStream_t st) {
                             return robot_launchers(robot).constraint_check(c.P, d_cons, s.at<float>(dq), n, s.at<uint64_t>(db), s.at<float>(dr), st);
                         });
                     });
    }
    int vmv_constraint_check_motion_batch(int robot, const float *d_a, const float *d_b, size_t n, const vmv_ee_constraint *constraints,
                                          size_t n_constraints, const vmv_constraint_settings *settings, uint8_t *d_ok, void *stream)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, d_a && d_b && d_ok, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        return constraint_launch(c, static_cast<hipStream_t>(stream), [&](const vmv::ConstraintDev *d_cons, hipStream_t st)
                                 { return robot_launchers(robot).constraint_edges(c.P, d_cons, d_a, d_b, n, d_ok, st); });
    }
    int vmv_constraint_check_motion_batch_host(int robot, const float *a, const float *b, size_t n, const vmv_ee_constraint *constraints,
                                               size_t n_constraints, const vmv_constraint_settings *settings, uint8_t *ok)
    {
        vmv::ConstraintBand c;
        if (int rc = constraint_checks(robot, a && b && ok, n, constraints, n_constraints, settings, c); rc != VMV_OK) return rc;
        if (n == 0) return VMV_OK;
        if (int rc = require_device(); rc != VMV_OK) return rc;
        Staged s;
        const int da = s.in(a, config_bytes(robot, n)), db = s.in(b, config_bytes(robot, n)), dk = s.out(ok, n);
        return s.run([&]
                     {
                         return constraint_launch(c, nullptr, [&](const vmv::ConstraintDev *d_cons, hipStream_t st) {
                             return robot_launchers(robot).constraint_edges(c.P, d_cons, s.at<float>(da), s.at<float>(db), n, s.at<uint8_t>(dk), st);
                         });
                     });
    }

    // ---- multi-GPU sharding arithmetic (vamp_mvt_amd/sharding.py: shard_range) ----
    size_t vmv_shard_words(size_t n, int world)
    {
        if (world < 1) return 0;
        const size_t words = (n + 63) / 64;
        return (words + (size_t) world - 1) / (size_t) world;
    }
    int vmv_shard_range(size_t n, int rank, int world, size_t *lo, size_t *hi)
    {
        if (!lo || !hi || world < 1 || rank < 0 || rank >= world) return VMV_ERR_INVALID_ARGUMENT;
        const size_t per = vmv_shard_words(n, world) * 64;
        *lo = std::min((size_t) rank * per, n);
        *hi = std::min(((size_t) rank + 1) * per, n);
        return VMV_OK;
    }

    // ---- free spheres against the environment (any robot's image will do: the counted loops use no grid) ----
    int vmv_spheres_in_collision_batch(const vmv_env *env, const float *d_spheres, size_t n, uint8_t *d_hits, void *stream)
    {
        const EnvCall c = env_call(0, env, false, d_spheres && d_hits, n, kDevice);
        if (!c.run) return c.rc;
        return launch_spheres(env, d_spheres, n, d_hits, nullptr, 0, stream);
    }
    int vmv_spheres_in_collision_batch_host(const vmv_env *env, const float *spheres, size_t n, uint8_t *hits)
    {
        const EnvCall c = env_call(0, nullptr, true, env && spheres && hits, n, kHost);
        if (!c.run) return c.rc;
        Staged s;
        const int ds = s.in(spheres, n * 16), dh = s.out(hits, n);
        return s.run([&] { return vmv_spheres_in_collision_batch(env, s.at<float>(ds), n, s.at<uint8_t>(dh), nullptr); });
    }
    int vmv_filter_self_from_pointcloud(int robot, const vmv_env *env, const float *q, const float *points_xyz, size_t n,
                                        float point_radius, float *out_xyz, size_t capacity, size_t *n_out)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        const EnvCall c = env_call(0, env, false, q && (!n || points_xyz) && n_out, n, kHost);
        if (!c.run && c.rc != VMV_OK) return c.rc;
        *n_out = 0;
        if (!c.run) return VMV_OK;
        const size_t ns = (size_t) kRobots[robot].n_spheres;
        std::vector<float> spheres(4 * n);
        for (size_t i = 0; i < n; ++i)
        {
            std::memcpy(&spheres[4 * i], points_xyz + 3 * i, 12);
            spheres[4 * i + 3] = point_radius;
        }
        std::vector<uint8_t> hits(n);
        Staged s;
        const int dq = s.in(q, config_bytes(robot, 1)), drs = s.out(nullptr, ns * 16), ds = s.in(spheres.data(), n * 16),
                  dh = s.out(hits.data(), n);
        const int rc = s.run([&]
                             {
                                 // Robot::sphere_fk of the one configuration
                                 const int fk = robot_launchers(robot).fk(s.at<float>(dq), 1, s.at<float>(drs), nullptr);
                                 return fk != VMV_OK ? fk : launch_spheres(env, s.at<float>(ds), n, s.at<uint8_t>(dh), s.at<float>(drs),
                                                                           (int) ns, nullptr);
                             });
        if (rc != VMV_OK) return rc;
        size_t m = 0;
        for (size_t i = 0; i < n; ++i)
            if (!hits[i])
            {
                if (out_xyz && m < capacity) std::memcpy(out_xyz + 3 * m, points_xyz + 3 * i, 12);
                ++m;
            }
        *n_out = m;
        return (out_xyz && m > capacity) ? VMV_ERR_CAPACITY : VMV_OK;
    }

    // ---- measurement support ----
    int vmv_time_validate_batch(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, int iters,
                                void *stream, float *avg_ms)
    {
        if (!avg_ms || iters < 1) return VMV_ERR_INVALID_ARGUMENT;
        hipStream_t s = static_cast<hipStream_t>(stream);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        VMV_HIP(hipEventCreate(&e0));
        hipError_t he = hipEventCreate(&e1);
        int rc = VMV_OK;
        float ms = 0.f;
        if (he == hipSuccess) he = hipEventRecord(e0, s);
        for (int i = 0; he == hipSuccess && i < iters && rc == VMV_OK; ++i)
            rc = vmv_validate_batch(robot, env, d_q, n, d_bits, stream);
        if (he == hipSuccess) he = hipEventRecord(e1, s);
        if (he == hipSuccess) he = hipEventSynchronize(e1);
        if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
        (void) hipEventDestroy(e0);  // on every exit path
        if (e1) (void) hipEventDestroy(e1);
        if (he != hipSuccess) return hip_fail(he, "vmv_time_validate_batch");
        *avg_ms = ms / (float) iters;
        return rc;
    }

    int vmv_fill_uniform_configs(int robot, float *d_q, size_t n, uint64_t seed, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q) return VMV_ERR_INVALID_ARGUMENT;
        return generate_configs(robot, vmv::fill_uniform_kernel, seed, d_q, n, stream);
    }
    int vmv_halton_configs(int robot, uint64_t skip, float *d_q, size_t n, void *stream)
    {
        if (!robot_ok(robot)) return VMV_ERR_UNKNOWN_ROBOT;
        if (!d_q || skip + n > 1000000ull) return VMV_ERR_INVALID_ARGUMENT;
        if (n == 0) return VMV_OK;
        return generate_configs(robot, vmv::halton_kernel, skip, d_q, n, stream);
    }

    const char *vmv_kernel_name(int robot, const char *entry_point)
    {
        static thread_local std::string name;
        if (!robot_ok(robot) || !entry_point) return nullptr;
        // validate_batch / validate_motion_batch run as two kernels (environment half, self-collision half);
        // the environment kernel dominates
        std::string ep(entry_point);
        if (ep == "validate_batch") ep = "validate_env";
        if (ep == "validate_motion_batch") ep = "rake_tasks_env";
        name = std::string("vmv::") + kRobots[robot].name + "::" + ep + "_kernel";
        return name.c_str();
    }
}  // extern "C"
