// vmv_robot_tu.inc — kernels of ONE robot; its launchers follow in vmv_robot_launch.inc.  Included by gen/tu_<robot>.hip with
//   VMV_ROBOT_NS      robot namespace / traits prefix (panda, ur5, fetch, baxter)
//   VMV_ROBOT_LAUNCH  name of the exported RobotLaunchers object
// One translation unit per robot keeps hipcc's compile time parallel (the generated FK programs are large).
#include "../../include/vamp_mvt_amd.h"
#include "vmv_common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifdef VMV_SELF_STAMP
#include <cstdio>
#endif

// workgroups per CU the edge kernels are compiled for (tuning knobs; tools/build_variant.py)
#ifndef VMV_MOTION_ENV_BLOCKS
#define VMV_MOTION_ENV_BLOCKS 4  // (the variants with point-cloud code: 128 VGPRs and 9 - 19 spilled beat 151 VGPRs at 3: config 5 18.4 -> 16.2 ms)
#endif
#ifndef VMV_MOTION_PRIMS_BLOCKS  // rake_tasks_env_kernel of the primitive-only variants
#define VMV_MOTION_PRIMS_BLOCKS 5  // (96 VGPRs, 0 - 6 spilled: Panda's roadmap-shaped edges 1.57 -> 1.45 ms per 262,144, Baxter's -3 %)
#endif
#ifndef VMV_CLOUDS_BLOCKS  // validate_env_kernel<kEnvClouds>
#define VMV_CLOUDS_BLOCKS 4
#endif
#ifndef VMV_PRIMS_BLOCKS  // validate_env_kernel<kEnvPrims>
#define VMV_PRIMS_BLOCKS R::kEnvBlocks
#endif
#ifndef VMV_MOTION_SELF_BLOCKS
// (what the configuration kernel of the robot is compiled for: Panda 4, UR5 4, Fetch 2, Baxter 3.  Baxter: 168 VGPRs with 5
// spilled instead of 186 at two workgroups: config 5 16.2 -> 15.1 ms; Panda: 128 with 7 spilled instead of 143 at three:
// 262,144 roadmap-shaped edges 1.455 -> 1.38 ms)
#define VMV_MOTION_SELF_BLOCKS R::kMotionSelfBlocks  // (UR5: 5, tools/gen_hip.py MOTION_SELF_BLOCKS)
#endif
// batches below this many edges take the fused task kernel where the robot has one (Panda, UR5; primitives only).  Measured
// (profiles/r03_edge_schedules.txt, UR5): 256 edges 0.148 -> 0.128 ms, 2,048: 0.165 -> 0.144, 8,192: 0.179 -> 0.158, level at
// 16,384, slower beyond (32,768: 0.29 -> 0.36)
#ifndef VMV_EDGE_FUSED_BELOW
#define VMV_EDGE_FUSED_BELOW 16384
#endif
#define VMV_CAT_(a, b) a##b
#define VMV_CAT(a, b) VMV_CAT_(a, b)
#define VMV_TRAITS VMV_CAT(VMV_ROBOT_NS, _traits)

namespace vmv
{
namespace VMV_ROBOT_NS
{
    using R = VMV_TRAITS;

    // LDS image of the environment kernels: [primitive block | CAPT split planes (optional) | radius table |
    // one slab per wave]; of the self-collision kernels: [radius table | one slab per wave].
    __host__ __device__ constexpr uint32_t slab_spheres_floats()
    {
        constexpr uint32_t a = (uint32_t) R::kSlabSpheres * 3u * kRow;
        constexpr uint32_t b = (uint32_t) R::kDim * kWave;
        return a > b ? a : b;
    }
    __host__ __device__ constexpr uint32_t slab_floats() { return slab_spheres_floats() + (uint32_t) kScratchWords; }
    __host__ __device__ constexpr uint32_t self_slab_floats()
    {
        constexpr uint32_t a = (uint32_t) R::kSelfSlabSpheres * 3u * kRow;
        constexpr uint32_t b = (uint32_t) R::kDim * kWave;
        return (a > b ? a : b) + (uint32_t) kSelfScratchWords;
    }
    // radius table in LDS: the robot's radii, then (environment kernels) the radii of the attached spheres
    constexpr uint32_t kRadiiFloats = ((uint32_t) R::kNRadii + (uint32_t) kMaxAttachSpheres + 3u) & ~3u;
    // (the self-collision kernels pose no attachments: without those 1 KiB UR5's kernel fits four workgroups per CU)
    constexpr uint32_t kSelfRadiiFloats = ((uint32_t) R::kNRadii + 3u) & ~3u;
    // environment kernels: [.. | CAPT hit-flag rows (kCaptFlagWords) | radius table | slabs ..]
    constexpr uint32_t kEnvRadiiFloats = kRadiiFloats + (uint32_t) kCaptFlagWords;

    __device__ __forceinline__ void stage_radii(float *dst, const EnvDev *__restrict__ env = nullptr)
    {
        for (uint32_t i = threadIdx.x; i < (uint32_t) R::kNRadii; i += blockDim.x) dst[i] = VMV_ROBOT_NS::kRadii[i];
        if (env)
            for (uint32_t i = threadIdx.x; i < env->n_attach; i += blockDim.x)
                dst[R::kNRadii + i] = env->attach_spheres[4 * i + 3];
    }

    // Copies the primitive block (and optionally the top of point cloud 0's blocked split planes) into LDS; returns the view.
    __device__ __forceinline__ EnvView
    stage_environment(const EnvDev *__restrict__ env, const uint32_t tests_in_lds, float *smem)
    {
        // (smem is the workgroup's dynamic LDS; the view carries it with its explicit address space)
        const uint32_t tid = threadIdx.x;
        const uint32_t n_floats = env->n_floats;
        const float4 *src = reinterpret_cast<const float4 *>(env->prims);
        float4 *dst = reinterpret_cast<float4 *>(smem);
        for (uint32_t i = tid; i < n_floats / 4; i += blockDim.x) dst[i] = src[i];
        if (tests_in_lds)
        {
            const float *planes = env->capt[0].q_planes;  // the leading groups of the blocked copy (vmv_device.h)
            for (uint32_t i = tid; i < tests_in_lds; i += blockDim.x) smem[n_floats + i] = planes[i];
        }
        float *radii = smem + ((n_floats + tests_in_lds + 3u) & ~3u) + kCaptFlagWords;
        stage_radii(radii, env);
        __syncthreads();
        return EnvView{(env_cptr) env, (lds_cptr) smem, tests_in_lds, (lds_cptr) radii};
    }

    // the lane number, recomputed where it is asked for (volatile: never hoisted out of a loop, never merged)
    __device__ __forceinline__ uint32_t opaque_lane_id()
    {
        uint32_t lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        return lane;
    }

    // Coalesced load of 64 consecutive configurations ([64][DIM] floats) and LDS transpose into registers.
    template <int DIM>
    __device__ __forceinline__ void
    load_configs(const float *__restrict__ q, size_t first_cfg, size_t n_cfg, lds_ptr wave_slab, float (&out)[DIM],
                 const uint32_t lane = __lane_id())
    {
        const size_t base = first_cfg * DIM;
        const size_t total = n_cfg * DIM;
#pragma unroll
        for (int k = 0; k < DIM; ++k)
        {
            const size_t idx = base + (size_t) k * kWave + lane;
            wave_slab[k * kWave + lane] = (idx < total) ? q[idx] : 0.0f;
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < DIM; ++j) out[j] = wave_slab[lane * DIM + j];
        wave_lds_sync();
    }

    // Boundary rule for non-finite input (include/vamp_mvt_amd.h): a configuration with a NaN or +-inf joint is INVALID,
    // an edge with such an endpoint likewise.  (The reference's sign-bit predicates would read the sign of whichever NaN
    // each instruction happens to propagate — an artefact, and a different one per instruction set.)  One v_cmp_class per
    // joint at load; the lane is switched off and its joints zeroed, so nothing downstream ever sees the NaN.
    template <int DIM>
    __device__ __forceinline__ bool sanitize_config(float (&cfg)[DIM])
    {
        bool finite = true;
#pragma unroll
        for (int j = 0; j < DIM; ++j) finite = finite && __builtin_isfinite(cfg[j]);
#pragma unroll
        for (int j = 0; j < DIM; ++j) cfg[j] = finite ? cfg[j] : 0.0f;
        return finite;
    }

    // <robot>.validate over a batch: one lane = one configuration (= one reference rake whose 8 lanes all hold
    // that configuration).  Bit i of the output = configuration i is collision free.
    //
    // Robot::fkcc is the OR of an environment half and a self-collision half.  They run as two kernels because
    // their resource profiles differ (see tools/gen_hip.py): the environment kernel is LDS-latency bound and wants
    // 4+ waves per SIMD (<= 128 VGPRs, small slab); the self-collision kernel is pure register arithmetic.
    // kernel 1 writes the validity words, kernel 2 ANDs into them (same stream, in order).
    // V: what the variant compiles in (vmv_device.h kEnvFull / kEnvPrims / kEnvZOnly; the launcher picks).
    // PAIRS (primitive-only variants): the fine phase deals (item, candidate) pairs (vmv_device.h env_fine_pairs).
    template <int V, bool PAIRS = false>
    __global__ __launch_bounds__(kBlock, (V == kEnvFull) ? 4 : (V == kEnvClouds) ? VMV_CLOUDS_BLOCKS : (V == kEnvPrims) ? VMV_PRIMS_BLOCKS : R::kEnvBlocks) void validate_env_kernel(const EnvDev *__restrict__ env,
                                                                      const uint32_t tests_in_lds,
                                                                      const float *__restrict__ q, const uint32_t n,
                                                                      uint64_t *__restrict__ bits)
    {
        // (n is 32-bit: the launcher cuts larger batches into slices.  A 64-bit bound has no scalar ordered compare on
        // gfx950, so it was copied to a VGPR pair, hoisted out of the loop and spilled.)
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        const uint32_t wave = uniform(threadIdx.x / kWave);  // wave-uniform by construction: an SGPR, like all it feeds
        lds_ptr wave_slab =
            (lds_ptr) smem + ((env->n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats + wave * slab_floats();

        for (uint32_t base = blockIdx.x * (uint32_t) kBlock; base < n; base += gridDim.x * (uint32_t) kBlock)
        {
            const uint32_t first = base + wave * (uint32_t) kWave;
            if (first >= n) continue;  // wave-uniform
            // the lane number is re-derived inside the loop, opaquely: as a loop invariant the per-lane LDS addresses built
            // from it were hoisted and spilled (36 B of scratch per lane, 38 MB of HBM writes per 1M-configuration launch)
            const uint32_t lane = opaque_lane_id();
            lds_ptr slab = wave_slab + lane;
            float cfg[R::kDim];
            load_configs<R::kDim>(q, first, n, wave_slab, cfg, lane);
            const bool finite = sanitize_config<R::kDim>(cfg);
            const bool in_range = first + lane < n && finite;
            const bool bad = R::template fkcc_env<1, V, PAIRS>(E, cfg, slab, !in_range);
            const uint64_t word = __ballot(in_range && !bad);
            if (opaque_lane_id() == 0u) bits[first / kWave] = word;  // (not `lane`: it would stay live across the whole body)
        }
    }

    // Per-wave LDS region of the fused task kernel (both halves of Robot::fkcc along one FK, robots with R::kHasFused):
    // the larger of the two halves' (they use it one after the other).
    __host__ __device__ constexpr uint32_t fused_slab_floats()
    {
        return slab_floats() > self_slab_floats() ? slab_floats() : self_slab_floats();
    }

    // One workgroup, every lane alike: the environment groups of the robot's static links (gen: static_env_hit).
    __global__ __launch_bounds__(kBlock) void static_links_kernel(EnvDev *__restrict__ env, const uint32_t tests_in_lds)
    {
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        const bool hit = R::static_env_hit(E);
        if (threadIdx.x == 0) env->static_hit = hit ? 1u : 0u;
    }

    // The same for many environments (vmv_env_prepare_multi): workgroup b stages environment b with its own LDS plan.
    struct StaticJob
    {
        EnvDev *env;
        uint32_t tests_in_lds;
    };
    __global__ __launch_bounds__(kBlock) void static_links_multi_kernel(const StaticJob *__restrict__ jobs)
    {
        extern __shared__ __align__(16) float smem[];
        const StaticJob J = jobs[blockIdx.x];
        const EnvView E = stage_environment(J.env, J.tests_in_lds, smem);
        const bool hit = R::static_env_hit(E);
        if (threadIdx.x == 0) J.env->static_hit = hit ? 1u : 0u;
    }

    // Attachment part of Robot::fkcc_attach (only launched for environments with an attachment): ANDs into the words.
    __global__ __launch_bounds__(kBlock, 2) void validate_attach_kernel(const EnvDev *__restrict__ env,
                                                                       const uint32_t tests_in_lds,
                                                                       const float *__restrict__ q, const size_t n,
                                                                       uint64_t *__restrict__ bits)
    {
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        const uint32_t lane = __lane_id();
        const uint32_t wave = threadIdx.x / kWave;
        lds_ptr wave_slab =
            (lds_ptr) smem + ((env->n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats + wave * slab_floats();
        for (size_t base = (size_t) blockIdx.x * kBlock; base < n; base += (size_t) gridDim.x * kBlock)
        {
            const size_t first = base + (size_t) wave * kWave;
            if (first >= n) continue;  // wave-uniform
            const uint64_t before = bits[first / kWave];
            if (before == 0ull) continue;
            float cfg[R::kDim];
            load_configs<R::kDim>(q, first, n, wave_slab, cfg);
            const bool todo = (first + lane < n) && ((before >> lane) & 1ull);
            const bool bad = R::template fkcc_attach<1>(E, cfg, wave_slab + lane, !todo);
            const uint64_t word = __ballot(todo && !bad);
            if (lane == 0) bits[first / kWave] = word;
        }
    }

    // vmv_validate_batch_multi: the segmented twins of validate_env_kernel / validate_attach_kernel.  Workgroup b takes
    // tile b of its launch's table and stages that tile's environment; wave w owns the GLOBAL validity word tile.word + w,
    // and the lanes of that word outside the tile's segment are out of range, as lanes beyond n are in the
    // single-environment kernels (zeroed joints, skipped).  The per-lane body is the single-environment one, so every bit
    // is the one a call for that environment alone computes.  A word that holds configurations of two segments is shared:
    // the launcher zeroed it and each segment ORs (environment half) or ANDs (attachment) its bits in with a 64-bit
    // atomic, possibly from two launches; every other word has one writer and is stored as in the single-environment
    // kernels.  (One tile per workgroup, no loop: a loop over tiles that restages on a change of segment carried enough
    // scalar state across the body to spill on every robot.)
    __device__ __forceinline__ bool multi_shared_word(const uint32_t first, const uint32_t lo, const uint32_t hi, const uint32_t n)
    {
        return first < lo || (hi < n && first + (uint32_t) kWave > hi);
    }

    template <int V, bool PAIRS = false>
    __global__ __launch_bounds__(kBlock, (V == kEnvFull) ? 4 : (V == kEnvClouds) ? VMV_CLOUDS_BLOCKS : (V == kEnvPrims) ? VMV_PRIMS_BLOCKS : R::kEnvBlocks) void validate_env_multi_kernel(
        const MultiSeg *__restrict__ segs, const MultiTile *__restrict__ tiles, const float *__restrict__ q, const uint32_t n,
        uint64_t *__restrict__ bits)
    {
        extern __shared__ __align__(16) float smem[];
        const MultiTile tile = tiles[blockIdx.x];
        const MultiSeg S = segs[tile.seg];
        const EnvView E = stage_environment(S.env, S.tests_in_lds, smem);
        const uint32_t wave = uniform(threadIdx.x / kWave);
        const uint32_t word = tile.word + wave, first = word * (uint32_t) kWave;
        if (first >= S.hi) return;  // wave-uniform
        lds_ptr wave_slab = (lds_ptr) smem + S.slab + wave * slab_floats();
        const uint32_t lane = opaque_lane_id();
        float cfg[R::kDim];
        load_configs<R::kDim>(q, first, n, wave_slab, cfg, lane);
        const bool in_seg = first + lane >= S.lo && first + lane < S.hi;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = in_seg ? cfg[j] : 0.0f;
        const bool finite = sanitize_config<R::kDim>(cfg);
        const bool in_range = in_seg && finite;
        const bool bad = R::template fkcc_env<1, V, PAIRS>(E, cfg, wave_slab + lane, !in_range);
        const uint64_t w = __ballot(in_range && !bad);
        if (opaque_lane_id() == 0u)
        {
            if (multi_shared_word(first, S.lo, S.hi, n))
                atomicOr(reinterpret_cast<unsigned long long *>(bits + word), (unsigned long long) w);
            else
                bits[word] = w;
        }
    }

    __global__ __launch_bounds__(kBlock, 2) void validate_attach_multi_kernel(const MultiSeg *__restrict__ segs,
                                                                             const MultiTile *__restrict__ tiles,
                                                                             const float *__restrict__ q, const uint32_t n,
                                                                             uint64_t *__restrict__ bits)
    {
        extern __shared__ __align__(16) float smem[];
        const MultiTile tile = tiles[blockIdx.x];
        const MultiSeg S = segs[tile.seg];
        const EnvView E = stage_environment(S.env, S.tests_in_lds, smem);
        const uint32_t lane = __lane_id();
        const uint32_t wave = threadIdx.x / kWave;
        const uint32_t word = tile.word + wave, first = word * (uint32_t) kWave;
        if (first >= S.hi) return;  // wave-uniform
        // (a shared word's bits of the other segment may change meanwhile; this segment's bits are this wave's alone)
        const uint64_t before = bits[word];
        if (before == 0ull) return;
        lds_ptr wave_slab = (lds_ptr) smem + S.slab + wave * slab_floats();
        float cfg[R::kDim];
        load_configs<R::kDim>(q, first, n, wave_slab, cfg);
        const bool in_seg = first + lane >= S.lo && first + lane < S.hi;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = in_seg ? cfg[j] : 0.0f;
        const bool todo = in_seg && ((before >> lane) & 1ull);
        const bool bad = R::template fkcc_attach<1>(E, cfg, wave_slab + lane, !todo);
        if (multi_shared_word(first, S.lo, S.hi, n))
        {
            const uint64_t keep = __ballot(!(todo && bad));  // lanes outside the segment keep their bits
            if (lane == 0) atomicAnd(reinterpret_cast<unsigned long long *>(bits + word), (unsigned long long) keep);
        }
        else
        {
            const uint64_t w = __ballot(todo && !bad);
            if (lane == 0) bits[word] = w;
        }
    }

    // Contact report (Robot::fkcc_debug): spheres = sphere_fk of the batch ([n][kNSpheres] float4).  One lane per
    // (configuration, fine sphere): the primitives it collides with, kReportWords + 1 words per item.
    __global__ __launch_bounds__(kBlock) void contacts_env_kernel(const EnvDev *__restrict__ env, const uint32_t tests_in_lds,
                                                                   const float4 *__restrict__ spheres, const size_t items,
                                                                   uint32_t *__restrict__ out)
    {
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        for (size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x; i < items; i += (size_t) gridDim.x * kBlock)
        {
            const float4 s = spheres[i];
            uint32_t words[kReportWords + 1];
            sphere_hit_words(E, s.x, s.y, s.z, s.w, words);
#pragma unroll
            for (int w = 0; w <= kReportWords; ++w) out[i * (kReportWords + 1) + w] = words[w];
        }
    }
    // ... and one lane per (configuration, fine pair): bit p of the configuration's pair words = pair p overlaps
    __global__ __launch_bounds__(kBlock) void contacts_self_kernel(const float4 *__restrict__ spheres, const size_t n,
                                                                    uint32_t *__restrict__ out, const uint32_t pair_words)
    {
        const size_t total = n * (size_t) R::kNSelfPairs;
        for (size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t) gridDim.x * kBlock)
        {
            const size_t c = i / R::kNSelfPairs;
            const uint32_t p = (uint32_t) (i % R::kNSelfPairs);
            const float4 a = spheres[c * R::kNSpheres + VMV_ROBOT_NS::kSelfPairs[p][0]];
            const float4 b = spheres[c * R::kNSpheres + VMV_ROBOT_NS::kSelfPairs[p][1]];
            const float rs = a.w + b.w;  // collision/sphere_sphere.hh:9-23
            if (neg(sql2_3(a.x, a.y, a.z, b.x, b.y, b.z) - rs * rs)) atomicOr(&out[c * pair_words + (p >> 5)], 1u << (p & 31u));
        }
    }

    // <robot>.eefk over a batch: out[i] = 4 x 4 row-major end-effector frame (bindings/robot_helper.hh:279-282)
    __global__ __launch_bounds__(kBlock) void eefk_batch_kernel(const float *__restrict__ q, const size_t n,
                                                                 float *__restrict__ out)
    {
        const size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x;
        if (i >= n) return;
        float cfg[R::kDim], f[12];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = q[i * R::kDim + j];
        R::ee_frame(cfg, f);
        float *o = out + 16 * i;
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
#pragma unroll
            for (int k = 0; k < 3; ++k) o[4 * r + k] = f[3 + 3 * k + r];
            o[4 * r + 3] = f[r];
        }
        o[12] = o[13] = o[14] = 0.0f;
        o[15] = 1.0f;
    }

#ifdef VMV_SELF_STAMP
    // Measurement build only (tools/build_variant.py NAME -DVMV_SELF_STAMP; never in the default library): every wave of
    // the self-collision kernels writes one record of 4 words to self_stamp[global wave]: s_memrealtime (100 MHz) at
    // entry, at the end of its last pass and at exit; passes | XCC_ID << 16 | HW_ID << 32 (tools/self_stamp_summary.py).
    __device__ uint64_t *self_stamp;
    __device__ __forceinline__ uint64_t stamp_now() { return __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void stamp_write(const uint64_t t0, const uint64_t t1, const uint32_t passes)
    {
        const uint64_t t2 = stamp_now();
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        uint64_t *r = self_stamp + 4 * ((size_t) blockIdx.x * kWavesPerBlock + threadIdx.x / kWave);
        const uint32_t lane = __lane_id();
        if (lane < 4u)
            r[lane] = lane == 0u ? t0 : lane == 1u ? t1 : lane == 2u ? t2 :
                      ((uint64_t) (passes & 0xffffu) | (uint64_t) (xcc & 0xfu) << 16 | (uint64_t) hw << 32);
    }
#define VMV_STAMP_START const uint64_t stamp_t0_ = stamp_now(); uint64_t stamp_t1_ = 0; uint32_t stamp_passes_ = 0
#define VMV_STAMP_PASS ++stamp_passes_
#define VMV_STAMP_WORK_DONE stamp_t1_ = stamp_now()
#define VMV_STAMP_END stamp_write(stamp_t0_, stamp_t1_, stamp_passes_)
#else
#define VMV_STAMP_START
#define VMV_STAMP_PASS
#define VMV_STAMP_WORK_DONE
#define VMV_STAMP_END
#endif

    // The self-collision half ANDs into the validity words the environment kernel wrote.  A workgroup owns
    // kWavesPerBlock x `group` (group 1..8) consecutive words and its waves work through the configurations that are
    // still valid in them, 64 per pass: with 62.5 % of a 16-word share valid that is 10 passes of FK + self-collision
    // groups instead of 16 (12 with 4-word shares per wave) — what the environment half already rejected costs nothing.  Passes are
    // claimed from an LDS counter, so a wave whose passes ran long does not hold up the workgroup's other waves, and only
    // the last pass of the share runs partly empty (per-wave shares of 4 words left every wave a part-empty third pass,
    // and the kernel lasted 1.6 mean wave lives: profiles/r04_self_stamp_summary.txt).  Nothing is exchanged but the
    // words themselves (no list in memory, no device-scope atomics: the words are edited in LDS and stored once).  The
    // launcher picks `group` so that the grid is one round of resident workgroups.
    //
    // SCREEN != kSelfUnscreened (robots with R::kSelfScreen): a share runs two rounds of passes.  The first runs a screen -
    // table bits, the FK of the bounding centres, every group's gate - on the valid configurations and collects the
    // flagged ones in flag words (LDS atomicOr); one wave then makes the flag words the enumeration, and the second round
    // runs fkcc_self on the flagged configurations alone, packed 64 to a pass.  An unflagged configuration has every gate
    // of fkcc_self false, so fkcc_self would have returned `skip` for it: the words are the same.  The flag words lie in
    // wave 0's slab, which no wave touches before the second round.  The second round deals the flagged configurations
    // evenly over the workgroup's waves (at most 64 per pass).
    // The screen of kSelfExactScreen is R::fkcc_self_screen, the gates' own arithmetic.  That of kSelfPrescreen, the
    // default, is R::fkcc_self_prescreen: the hardware's sine and cosine, fused multiply-adds, and thresholds widened by a
    // margin the generator computes from the measured error of those instructions, so that it flags a superset of what the
    // exact screen flags (and every configuration with a joint outside |q| <= Q_MAX).  Which configurations run fkcc_self
    // changes, what fkcc_self answers does not.  VMV_SELF_SCREEN = 2 / 0 selects the exact screen / no screen
    // (measurement and test aid).
    enum SelfScreenMode : int
    {
        kSelfUnscreened = 0,
        kSelfPrescreen = 1,
        kSelfExactScreen = 2
    };
    static_assert(kSelfShareWords == (uint32_t) kWavesPerBlock * 8u, "a share holds group <= 8 words per wave");
    template <int SCREEN>
    __global__ __launch_bounds__(kBlock, R::kSelfBlocks) void validate_self_kernel(const float *__restrict__ q, const uint32_t n,
                                                                    uint64_t *__restrict__ bits, const uint32_t group)
    {
        VMV_STAMP_START;
        __shared__ __align__(16) float stage[kSelfRadiiFloats + kWavesPerBlock * self_slab_floats()];
        __shared__ SelfShare S;
        stage_radii(stage);
        const uint32_t wave = uniform(threadIdx.x / kWave);
        lds_ptr wave_slab = (lds_ptr) stage + kSelfRadiiFloats + wave * self_slab_floats();
        static_assert(kSelfRadiiFloats % 2u == 0u && self_slab_floats() >= 2u * kSelfShareWords, "the flag words fit a slab");
        unsigned long long *const flag = (unsigned long long *) (stage + kSelfRadiiFloats);  // [kSelfShareWords], screened instances only
        const uint32_t words = (n + (uint32_t) kWave - 1u) / (uint32_t) kWave;
        const uint32_t share = group * (uint32_t) kWavesPerBlock;  // <= kSelfShareWords (the launcher clamps group)
        const uint32_t tail = n % (uint32_t) kWave;
        for (uint32_t w0 = blockIdx.x * share; w0 < words; w0 += gridDim.x * share)  // workgroup-uniform
        {
            const uint32_t nw = (words - w0 < share) ? words - w0 : share;
            // (lane numbers re-derived opaquely: the table addresses built from threadIdx were hoisted out of the loop and
            // spilled)
            if (wave == 0u)
            {
                self_share_load(S, bits, w0, nw, words - 1u, tail, opaque_lane_id());
                if (SCREEN != kSelfUnscreened && opaque_lane_id() < kSelfShareWords) flag[opaque_lane_id()] = 0ull;
            }
            __syncthreads();
            uint32_t total = uniform(S.before[nw]);
            uint32_t width = (uint32_t) kWave;  // configurations per pass of the (second) round
            if constexpr (SCREEN != kSelfUnscreened)
            {
                for (;;)
                {
                    const uint32_t pass = self_share_claim(S, opaque_lane_id());
                    if (pass >= total) break;  // wave-uniform
                    const uint32_t at = self_share_locate(S, nw, pass + opaque_lane_id(), total);
                    const uint32_t idx = w0 * (uint32_t) kWave + (at != ~0u ? at : 0u);
                    float cfg[R::kDim];
#pragma unroll
                    for (int d = 0; d < R::kDim; ++d) cfg[d] = q[(size_t) idx * R::kDim + d];
                    const bool flagged = SCREEN == kSelfPrescreen ? R::fkcc_self_prescreen(cfg) : R::fkcc_self_screen(cfg);
                    if (flagged && at != ~0u)
                        atomicOr(&flag[at / (uint32_t) kWave], 1ull << (at % (uint32_t) kWave));  // LDS atomic
                }
                __syncthreads();
                if (wave == 0u) self_share_enumerate(S, opaque_lane_id() < nw ? flag[opaque_lane_id()] : 0ull, opaque_lane_id());
                __syncthreads();  // (also: wave 0 has read the flag words before its slab is written)
                total = uniform(S.before[nw]);
                // the flagged configurations of a share rarely fill one pass per wave: dealt evenly, no wave waits at the
                // barrier for another's pass (a pass is a long dependent chain whatever its lanes; self kernel 0.0634 -> 0.0608 ms)
                width = (total + (uint32_t) kWavesPerBlock - 1u) / (uint32_t) kWavesPerBlock;
                width = width < 1u ? 1u : (width > (uint32_t) kWave ? (uint32_t) kWave : width);
            }
            for (;;)
            {
                const uint32_t pass = self_share_claim(S, opaque_lane_id(), width);
                if (pass >= total) break;  // wave-uniform: the share is used up
                VMV_STAMP_PASS;
                const uint32_t lane = opaque_lane_id();
                const uint32_t at = (SCREEN == kSelfUnscreened || lane < width) ? self_share_locate(S, nw, pass + lane, total) : ~0u;
                const uint32_t idx = w0 * (uint32_t) kWave + (at != ~0u ? at : 0u);  // (a valid bit always lies below n <= 2^31)
                float cfg[R::kDim];
#pragma unroll
                for (int d = 0; d < R::kDim; ++d) cfg[d] = q[(size_t) idx * R::kDim + d];
                const bool bad = R::template fkcc_self<1>(cfg, wave_slab + lane, (lds_cptr) stage, at == ~0u);
                if (bad && at != ~0u) atomicAnd(&S.result[at / (uint32_t) kWave], ~(1ull << (at % (uint32_t) kWave)));  // LDS atomic
            }
            VMV_STAMP_WORK_DONE;
            __syncthreads();
            if (wave == 0u && opaque_lane_id() < nw) bits[w0 + opaque_lane_id()] = S.result[opaque_lane_id()];
            __syncthreads();  // (the next share rewrites the tables)
        }
        VMV_STAMP_END;
    }

    // vmv_self_screen_flags: bit i of the words = the exact screen (EXACT) or the prescreen flags row i; one lane per
    // row, one word per wave, whatever the validity of the row (probe of the screens: tests/test_self_prescreen_gpu.py).
    // The grid covers n; n >= 1.
    template <bool EXACT>
    __global__ __launch_bounds__(kBlock) void self_screen_flags_kernel(const float *__restrict__ q, const uint32_t n,
                                                                        uint64_t *__restrict__ words)
    {
        const uint32_t i = blockIdx.x * (uint32_t) kBlock + threadIdx.x;
        const uint32_t row = i < n ? i : 0u;
        float cfg[R::kDim];
#pragma unroll
        for (int d = 0; d < R::kDim; ++d) cfg[d] = q[(size_t) row * R::kDim + d];
        const bool flagged = EXACT ? R::fkcc_self_screen(cfg) : R::fkcc_self_prescreen(cfg);
        const uint64_t word = __ballot(flagged && i < n);
        if (__lane_id() == 0u && i < n) words[i / (uint32_t) kWave] = word;  // (lane 0 of a wave below n: word <= (n - 1) / 64)
    }

    // hsum + exact sqrt of a configuration-sized vector (vector/avx.hh:441-452, interface.hh:397-410)
    template <int DIM>
    __device__ __forceinline__ float l2_norm(const float (&v)[DIM])
    {
        float sq[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) sq[i] = (i < DIM) ? v[i < DIM ? i : 0] * v[i < DIM ? i : 0] : 0.0f;
        float row[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = (DIM > 8) ? sq[k] + sq[8 + k] : sq[k];
        const float s0 = row[4] + row[0], s1 = row[5] + row[1], s2 = row[6] + row[2], s3 = row[7] + row[3];
        const float a = s0 + s2, b = s1 + s3;
        return sqrtf(a + b);
    }

    // Attachment part of validate_motion<Robot, 8, Robot::resolution> over a batch of edges (planning/validate.hh:24-77),
    // after the (edge, rake) task passes: an edge is valid iff fkcc and fkcc_attach are clear on every rake (the
    // reference's early-out only skips work, so the parts may walk the edge independently); this walk continues only the
    // edges the task passes left valid and clears the bit of an edge one of whose rakes collides.
    //
    // Lanes 8g..8g+7 of a wave are the 8 lanes of one reference rake (G = 8: the reference's "any lane of the rake"
    // gating is reproduced with ballots).  Edges have very different lengths (n = ceil(distance * resolution / 8)
    // rakes) and stop at their first colliding rake, so rakes are scheduled dynamically: a workgroup owns a chunk
    // of kChunkEdges consecutive edges, and each of its 32 rake groups pulls the next edge of the chunk from an LDS
    // counter as soon as its current edge is decided.  Per edge the arithmetic is the reference's, in its order:
    // block = start + vector * percent for the first rake, then block -= backstep, n and backstep from the
    // hsum-ordered l2 norm.  Validity bits of the chunk are assembled in LDS and stored once.
#ifndef VMV_CHUNK_EDGES
#define VMV_CHUNK_EDGES 512
#endif
    constexpr uint32_t kChunkEdges = VMV_CHUNK_EDGES;     // multiple of 64: chunks own whole validity words
    constexpr uint32_t kCtrlWords = 4 + kChunkEdges / 32; // [0] next edge, [4..] validity bits of the chunk

    // SEG (vmv_validate_motion_batch_multi): one chunk, the one from edge seg_begin, and only the edges of the segment
    // [seg_lo, seg_hi) in it; the others are dead on arrival, and a word shared with another segment is ANDed in.
    __device__ __forceinline__ uint32_t segment_mask32(const size_t first, const uint32_t lo, const uint32_t hi)
    {
        const size_t a = lo > first ? lo - first : 0u, b = hi > first ? (hi - first < 32u ? hi - first : 32u) : 0u;
        if (b <= a) return 0u;
        return (b == 32u ? ~0u : (1u << b) - 1u) & ~((1u << a) - 1u);
    }

    template <bool SEG = false>
    __device__ __forceinline__ void motion_body(const EnvView &E, lds_ptr slab, lds_u32 *ctrl,
                                                const float *__restrict__ start, const float *__restrict__ goal,
                                                const size_t n, uint32_t *__restrict__ bits32, const uint32_t chunk,
                                                const uint32_t seg_lo = 0u, const uint32_t seg_hi = 0u,
                                                const uint32_t seg_begin = 0u)
    {
        // chunk: edges per workgroup pass, a multiple of 64 and at most kChunkEdges (the launcher shrinks it for small
        // batches so that the grid still fills the chip: a 2,000-edge planner batch is 32 workgroups at 64, 4 at 512)
        const uint32_t lane = __lane_id();
        const uint32_t tid = threadIdx.x;
        const uint32_t group = tid / 8;  // rake group within the workgroup
        const int k = lane & 7;
        const uint32_t leader = lane & ~7u;
        constexpr uint32_t kGroups = kBlock / 8;
        const size_t n_words = ((n + 63) / 64) * 2;  // 32-bit words of the validity array
        lds_u32 *chunk_bits = ctrl + 4;
        const float percent = (float) (k + 1) / 8.0f;  // validate.hh:12-21

        for (size_t begin = SEG ? (size_t) seg_begin : (size_t) blockIdx.x * chunk; begin < n;
             begin += SEG ? n : (size_t) gridDim.x * chunk)  // (SEG: one chunk)
        {
            const size_t end = (begin + chunk < n) ? begin + chunk : n;
            if (tid < chunk / 32)
            {
                const size_t w = begin / 32 + tid;
                uint32_t in = (w < n_words) ? bits32[w] : 0u;
                const size_t first_edge = w * 32;  // bits at or beyond n are never continued (and come back as 0)
                if (first_edge + 32 > n) in &= (first_edge < n) ? ((1u << (uint32_t) (n - first_edge)) - 1u) : 0u;
                if constexpr (SEG) in &= segment_mask32(first_edge, seg_lo, seg_hi);
                chunk_bits[tid] = in;
            }
            if (tid == 0) ctrl[0] = (uint32_t) (begin + kGroups);
            __syncthreads();

            // per-rake-group state (identical in the 8 lanes of a group except block[])
            size_t e = begin + group;
            bool fresh = true;  // e was just assigned and has not been set up yet
            uint32_t step = 0, steps = 1;
            float block[R::kDim], backstep[R::kDim];
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) block[j] = backstep[j] = 0.0f;

            while (true)
            {
                // (re)assign: groups whose edge is decided, or dead on arrival, pull the next edge of the chunk
                while (true)
                {
                    const bool dead = fresh && e < end &&
                                      ((chunk_bits[(e - begin) / 32] >> ((e - begin) % 32)) & 1u) == 0u;
                    if (!wave_any(dead)) break;
                    uint32_t ne = (dead && k == 0) ? atomicAdd((uint32_t *) ctrl, 1u) : 0u;
                    ne = (uint32_t) __shfl((int) ne, (int) leader);
                    if (dead) e = ne;
                }
                const bool work = e < end;
                if (!wave_any(work)) break;
                if (wave_any(fresh && work))
                {
                    // set the edge up (validate.hh:31-41, :50): only the lanes of freshly assigned groups keep it
                    const size_t el = work ? e : begin;
                    float s[R::kDim], v[R::kDim];
                    bool finite = true;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j)
                    {
                        s[j] = start[el * R::kDim + j];
                        v[j] = goal[el * R::kDim + j];
                        finite = finite && __builtin_isfinite(s[j]) && __builtin_isfinite(v[j]);
                    }
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j)
                    {
                        s[j] = finite ? s[j] : 0.0f;  // (an edge with a non-finite endpoint is already invalid)
                        v[j] = finite ? v[j] - s[j] : 0.0f;
                    }
                    const float distance = l2_norm<R::kDim>(v);
                    const uint32_t st = (uint32_t) fmaxf(ceilf(distance / 8.0f * (float) R::kResolution), 1.F);
                    const float denom = (float) (8u * st);
                    const bool take = fresh && work;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j)
                    {
                        const float b0 = s[j] + (v[j] * percent);
                        const float bs = v[j] / denom;
                        block[j] = take ? b0 : block[j];
                        backstep[j] = take ? bs : backstep[j];
                    }
                    steps = take ? st : steps;
                    step = take ? 0u : step;
                    fresh = false;
                }

                const bool bad = R::template fkcc_attach<8>(E, block, slab, !work);

                // advance (validate.hh:43-64)
                const bool decided = work && (bad || step + 1 >= steps);
                if (work && !decided)
                {
                    step += 1;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j) block[j] = block[j] - backstep[j];
                }
                if (wave_any(decided))
                {
                    if (decided && k == 0)
                    {
                        const uint32_t bit = 1u << ((e - begin) % 32);
                        if (bad) atomicAnd((uint32_t *) &chunk_bits[(e - begin) / 32], ~bit);
                    }
                    uint32_t ne = (decided && k == 0) ? atomicAdd((uint32_t *) ctrl, 1u) : 0u;
                    ne = (uint32_t) __shfl((int) ne, (int) leader);
                    if (decided)
                    {
                        e = ne;
                        fresh = true;
                    }
                }
            }
            __syncthreads();
            if (tid < chunk / 32)
            {
                const size_t w = begin / 32 + tid;
                if constexpr (SEG)
                {
                    const uint32_t mask = segment_mask32(w * 32, seg_lo, seg_hi);
                    if (mask == ~0u)
                        bits32[w] = chunk_bits[tid];
                    else if (mask != 0u)  // (shared with another segment)
                        atomicAnd(bits32 + w, chunk_bits[tid] | ~mask);
                }
                else
                {
                    if (w < n_words) bits32[w] = chunk_bits[tid];
                }
            }
            __syncthreads();
        }
    }

    // ---------------------------------------------------------------------------------------------------------
    // (edge, rake) tasks.  The walk above gives a rake group one EDGE at a time and lets it walk the edge's rakes one
    // after the other: right for batches that oversubscribe the chip many times, but a planner-sized batch (hundreds
    // to tens of thousands of edges) then runs as deep as its longest edge, and a shard of the 1M-edge job is bounded by
    // the most loaded workgroup.  The task kernels give a rake group one RAKE at a time instead (vmv_edge_tasks.hip has
    // the rationale and the scan between passes): every task costs one fkcc, so a static assignment is balanced and the
    // depth of a batch that fits the chip is one fkcc per pass.
    //   first pass  (`first` = true): task t = rake 0 of edge t; the environment kernel WRITES the validity byte of the 8
    //               edges of a wave and each edge's rake count, the self-collision kernel clears bits in it;
    //   later pass: task t = rake lo_i + (t - excl[e]) of the edge e whose range of the pass's scan holds t (found by
    //               the group's 8 lanes together); an edge already invalid is skipped, a colliding rake clears the
    //               edge's bit with one atomic (failures only).
    // Per task the arithmetic is the reference's, in its order (validate.hh:31-64): block = start + vector * percent,
    // then `i` times block -= backstep — iterated, never multiplied.
    // ---------------------------------------------------------------------------------------------------------
    // largest e in [0, n) with excl[e] <= t: 8 probes per round, one per lane of the rake group (log9 n rounds)
    __device__ __forceinline__ uint32_t find_task_edge(const uint32_t *__restrict__ excl, const uint32_t n, const uint32_t t)
    {
        const uint32_t lane = __lane_id(), k = lane & 7u, leader = lane & ~7u;
        uint32_t lo = 0u, hi = n;  // excl[lo] <= t, and excl[hi] > t or hi == n
        while (wave_any(hi - lo > 1u))
        {
            const uint32_t p = lo + ((k + 1u) * (hi - lo)) / 9u;  // lo <= p < hi, non-decreasing in k
            const bool le = excl[p] <= t;                         // true for a prefix of the group's lanes
            const uint32_t m = (uint32_t) __popc((uint32_t) ((__ballot(le) >> leader) & 0xffull));
            const uint32_t p_lo = (uint32_t) __shfl((int) p, (int) (leader + (m > 0u ? m - 1u : 0u)));
            const uint32_t p_hi = (uint32_t) __shfl((int) p, (int) (leader + (m < 8u ? m : 7u)));
            lo = m > 0u ? p_lo : lo;
            hi = m < 8u ? p_hi : hi;
        }
        return lo;
    }

    // SEG (vmv_validate_motion_batch_multi, environment half): the workgroup's tasks are [t_begin, tasks) of the segment
    // [seg_lo, seg_hi), strided by its waves.  First pass: t_begin is a multiple of 32, the edges outside the segment are
    // out of range, the launcher zeroed the validity words, and a byte whose 32-bit word holds edges of another segment
    // is ORed in.  Later pass: the task's edge is searched among the segment's edges only.
    template <int PART, int V = kEnvFull, bool SEG = false>  // 0 environment half, 1 self-collision half, 3 both halves along one FK (fkcc_fused)
    __device__ __forceinline__ void rake_task_body(const EnvView &E, lds_ptr slab, const float *__restrict__ start,
                                                   const float *__restrict__ goal, const uint32_t n, uint8_t *__restrict__ bits8,
                                                   uint32_t *__restrict__ steps_out, const uint32_t *__restrict__ excl,
                                                   const uint32_t tasks, const uint32_t lo_i, const bool first,
                                                   const uint32_t seg_lo = 0u, const uint32_t seg_hi = 0u,
                                                   const uint32_t t_begin = 0u)
    {
        constexpr bool SELF = PART == 1;  // continues the edges the environment half left valid (PART 3 writes, like PART 0)
        const uint32_t lane = __lane_id();
        const uint32_t k = lane & 7u, g = lane >> 3;
        const float percent = (float) (k + 1u) / 8.0f;  // validate.hh:12-21
        const uint32_t stride = SEG ? (uint32_t) (kWavesPerBlock * 8) : gridDim.x * (uint32_t) (kWavesPerBlock * 8);
        const uint32_t t_first = SEG ? t_begin + (threadIdx.x / kWave) * 8u
                                     : (blockIdx.x * (uint32_t) kWavesPerBlock + threadIdx.x / kWave) * 8u;
        for (uint32_t t0 = t_first; t0 < tasks; t0 += stride)
        {
            const uint32_t t = t0 + g;
            uint32_t e = t, i = 0u, byte = 0u;
            bool work;
            if (first)
            {
                work = SEG ? (e >= seg_lo && e < seg_hi) : e < n;
                if constexpr (SELF)
                {
                    byte = bits8[t0 >> 3];
                    work = work && ((byte >> g) & 1u) != 0u;
                }
            }
            else
            {
                work = t < tasks;
                if constexpr (SEG)
                    e = seg_lo + find_task_edge(excl + seg_lo, seg_hi - seg_lo, work ? t : 0u);
                else
                    e = find_task_edge(excl, n, work ? t : 0u);
                i = lo_i + (t - excl[e]);
                work = work && ((bits8[e >> 3] >> (e & 7u)) & 1u) != 0u;  // already invalid: nothing to add
            }
            if (!wave_any(work))
            {
                if (first && !SELF && !SEG && lane == 0u) bits8[t0 >> 3] = 0u;
                continue;
            }
            // the edge (validate.hh:31-41, :50)
            const size_t el = work ? e : 0u;
            float block[R::kDim], backstep[R::kDim];
            bool finite = true;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
            {
                block[j] = start[el * R::kDim + j];
                backstep[j] = goal[el * R::kDim + j];
                finite = finite && __builtin_isfinite(block[j]) && __builtin_isfinite(backstep[j]);
            }
            float v[R::kDim];
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
            {
                block[j] = finite ? block[j] : 0.0f;  // a non-finite edge is one rake at the zero configuration, then invalid
                v[j] = finite ? backstep[j] - block[j] : 0.0f;
            }
            const float distance = l2_norm<R::kDim>(v);
            const uint32_t st = (uint32_t) fmaxf(ceilf(distance / 8.0f * (float) R::kResolution), 1.F);
            const float denom = (float) (8u * st);
            if constexpr (SEG && !SELF)  // (stored before the collision test: st is not kept alive across it)
                if (first && k == 0u && work) steps_out[e] = st;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
            {
                block[j] = block[j] + (v[j] * percent);
                backstep[j] = v[j] / denom;
            }
            if (!first)
            {
                uint32_t top = work ? i : 0u;  // the most subtractions any group of the wave needs
#pragma unroll
                for (int d = 32; d >= 8; d >>= 1)  // (i is uniform inside a group of 8)
                {
                    const uint32_t o = (uint32_t) __shfl_xor((int) top, d);
                    top = o > top ? o : top;
                }
                top = (uint32_t) __builtin_amdgcn_readfirstlane((int) top);
                for (uint32_t r = 0; r < top; ++r)
                {
                    const bool more = r < i && work;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j) block[j] = more ? block[j] - backstep[j] : block[j];
                }
            }
            bool bad;
            if constexpr (SELF)
                bad = R::template fkcc_self<8>(block, slab, E.radii, !work);
            else if constexpr (PART == 3)
                bad = R::template fkcc_fused<8, V>(E, block, slab, !work) || !finite;
            else
                bad = R::template fkcc_env<8, V>(E, block, slab, !work) || !finite;
            if (first)
            {
                const uint64_t ok = __ballot(work && !bad && k == 0u);  // bit 8 g = edge t0 + g is still valid
                const uint32_t out = (uint32_t) ((ok * 0x0102040810204080ull) >> 56);  // -> bit g
                if constexpr (SELF)
                {
                    if (lane == 0u && out != byte) bits8[t0 >> 3] = (uint8_t) out;
                }
                else if constexpr (SEG)
                {
                    const uint32_t d0 = t0 & ~31u;
                    if (lane == 0u)
                    {
                        if (d0 < seg_lo || (d0 + 32u > seg_hi && seg_hi < n))
                        {
                            if (out != 0u) atomicOr(reinterpret_cast<uint32_t *>(bits8) + (t0 >> 5), out << (t0 & 24u));
                        }
                        else
                            bits8[t0 >> 3] = (uint8_t) out;
                    }
                }
                else
                {
                    if (lane == 0u) bits8[t0 >> 3] = (uint8_t) out;
                    if (k == 0u && e < n) steps_out[e] = st;
                }
            }
            else if (work && bad && k == 0u)
                atomicAnd(reinterpret_cast<uint32_t *>(bits8) + (e >> 5), ~(1u << (e & 31u)));
        }
    }

    template <int V>
    __global__ __launch_bounds__(kBlock, (V == kEnvFull || V == kEnvClouds) ? VMV_MOTION_ENV_BLOCKS : VMV_MOTION_PRIMS_BLOCKS) void rake_tasks_env_kernel(
        const EnvDev *__restrict__ env, const uint32_t tests_in_lds, const float *__restrict__ start,
        const float *__restrict__ goal, const uint32_t n, uint8_t *__restrict__ bits8, uint32_t *__restrict__ steps_out,
        const uint32_t *__restrict__ excl, const uint32_t *__restrict__ total, const uint32_t lo_i, const uint32_t first)
    {
        // first pass: every byte of the validity words is written, also the ones past the last edge
        const uint32_t tasks = first ? ((n + 63u) & ~63u) : *total;
        if (blockIdx.x * (uint32_t) (kWavesPerBlock * 8) >= tasks) return;  // (before the environment is staged)
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        const uint32_t head = ((env->n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats;
        lds_ptr wave_slab = (lds_ptr) smem + head + (threadIdx.x / kWave) * slab_floats();
        rake_task_body<0, V>(E, wave_slab + __lane_id(), start, goal, n, bits8, steps_out, excl, tasks, lo_i, first != 0u);
    }

    // Both halves in one task kernel (robots with R::kHasFused, primitive-only environments): one FK and one launch per
    // pass instead of two.  The fused body is the slower one per unit of work (128 VGPRs, spills: DESIGN.md §6), so the
    // launcher uses it only for batches too small to fill the chip, where the depth — lone-wave latencies — is what counts.
    template <int V>
    __global__ __launch_bounds__(kBlock, R::kFusedBlocks) void rake_tasks_fused_kernel(
        const EnvDev *__restrict__ env, const uint32_t tests_in_lds, const float *__restrict__ start,
        const float *__restrict__ goal, const uint32_t n, uint8_t *__restrict__ bits8, uint32_t *__restrict__ steps_out,
        const uint32_t *__restrict__ excl, const uint32_t *__restrict__ total, const uint32_t lo_i, const uint32_t first)
    {
        if constexpr (R::kHasFused)
        {
            const uint32_t tasks = first ? ((n + 63u) & ~63u) : *total;
            if (blockIdx.x * (uint32_t) (kWavesPerBlock * 8) >= tasks) return;
            extern __shared__ __align__(16) float smem[];
            const EnvView E = stage_environment(env, tests_in_lds, smem);
            const uint32_t head = ((env->n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats;
            lds_ptr wave_slab = (lds_ptr) smem + head + (threadIdx.x / kWave) * fused_slab_floats();
            rake_task_body<3, V>(E, wave_slab + __lane_id(), start, goal, n, bits8, steps_out, excl, tasks, lo_i, first != 0u);
        }
    }

    __global__ __launch_bounds__(kBlock, VMV_MOTION_SELF_BLOCKS) void rake_tasks_self_kernel(
        const float *__restrict__ start, const float *__restrict__ goal, const uint32_t n, uint8_t *__restrict__ bits8,
        const uint32_t *__restrict__ excl, const uint32_t *__restrict__ total, const uint32_t lo_i, const uint32_t first)
    {
        const uint32_t tasks = first ? n : *total;
        if (blockIdx.x * (uint32_t) (kWavesPerBlock * 8) >= tasks) return;
        __shared__ __align__(16) float stage[kSelfRadiiFloats + kWavesPerBlock * self_slab_floats()];
        stage_radii(stage);
        __syncthreads();
        const EnvView E{nullptr, nullptr, 0u, (lds_cptr) stage};
        lds_ptr wave_slab = (lds_ptr) stage + kSelfRadiiFloats + (threadIdx.x / kWave) * self_slab_floats();
        rake_task_body<1>(E, wave_slab + __lane_id(), start, goal, n, bits8, nullptr, excl, tasks, lo_i, first != 0u);
    }

    __global__ __launch_bounds__(kBlock, 2) void validate_motion_attach_kernel(const EnvDev *__restrict__ env,
                                                                              const uint32_t tests_in_lds,
                                                                              const float *__restrict__ start,
                                                                              const float *__restrict__ goal,
                                                                              const size_t n, uint32_t *__restrict__ bits,
                                                                              const uint32_t chunk)
    {
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(env, tests_in_lds, smem);
        const uint32_t wave = threadIdx.x / kWave;
        const uint32_t head = ((env->n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats;
        lds_ptr wave_slab = (lds_ptr) smem + head + wave * slab_floats();
        lds_u32 *ctrl = (lds_u32 *) ((lds_ptr) smem + head + kWavesPerBlock * slab_floats());
        motion_body(E, wave_slab + __lane_id(), ctrl, start, goal, n, bits, chunk);
    }

    // vmv_validate_motion_batch_multi: the segmented twins of rake_tasks_env_kernel and validate_motion_attach_kernel
    // (the bodies' SEG forms); every workgroup stages exactly one environment.
    //   first pass: workgroup b takes tiles[b] = {segment, 32-bit validity word}: rake 0 of the segment's edges in that
    //               word, one validity byte per wave;
    //   later pass: workgroup b takes tile b of its class (launch_edge_multi_tiles): tile b - starts[j] of the segment
    //               entries[j], starts[j] <= b < starts[j + 1], i.e. `*chunk` consecutive tasks of that one segment.  The
    //               grid is sized for the most tiles there can be; the workgroups beyond the last one leave before they
    //               stage anything.  (One tile per workgroup, no loop over tiles: see validate_env_multi_kernel.)
    // The pass is a template argument, so that the later pass's tile search and segment bounds do not share one register
    // budget with pass 0's body (with a runtime `first`, up to 4 more VGPRs spilled than in rake_tasks_env_kernel).
    template <int V, bool FIRST>
    __global__ __launch_bounds__(kBlock, (V == kEnvFull || V == kEnvClouds) ? VMV_MOTION_ENV_BLOCKS : VMV_MOTION_PRIMS_BLOCKS) void rake_tasks_env_multi_kernel(
        const MultiSeg *__restrict__ segs, const MultiTile *__restrict__ tiles, const uint32_t *__restrict__ entries,
        const uint32_t m, const uint32_t *__restrict__ starts, const uint32_t *__restrict__ chunk,
        const float *__restrict__ start, const float *__restrict__ goal, const uint32_t n, uint8_t *__restrict__ bits8,
        uint32_t *__restrict__ steps_out, const uint32_t *__restrict__ excl, const uint32_t *__restrict__ total)
    {
        uint32_t seg, t_begin, t_end;
        if constexpr (FIRST)
        {
            const MultiTile tile = tiles[blockIdx.x];
            seg = tile.seg, t_begin = tile.word * 32u;
            const uint32_t top = (segs[seg].hi + 7u) & ~7u;  // (the waves whose byte lies past the segment have nothing to do)
            t_end = top - t_begin < 32u ? top : t_begin + 32u;
        }
        else
        {
            const uint32_t b = blockIdx.x;
            if (b >= starts[m]) return;  // (before the environment is staged)
            uint32_t lo = 0u, hi = m;    // starts[lo] <= b < starts[hi]: 64 probes per round, one per lane
            while (hi - lo > 1u)
            {
                const uint32_t p = lo + (uint32_t) (((uint64_t) (__lane_id() + 1u) * (hi - lo)) / (uint64_t) (kWave + 1));
                const uint32_t below = (uint32_t) __popcll(__ballot(starts[p] <= b));  // a prefix of the lanes
                const uint32_t p_lo = (uint32_t) __shfl((int) p, (int) (below > 0u ? below - 1u : 0u));
                const uint32_t p_hi = (uint32_t) __shfl((int) p, (int) (below < (uint32_t) kWave ? below : kWave - 1));
                lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (below > 0u ? p_lo : lo));
                hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (below < (uint32_t) kWave ? p_hi : hi));
            }
            seg = entries[lo];
            const uint32_t s_lo = segs[seg].lo, s_hi = segs[seg].hi, size = *chunk;
            const uint32_t end = s_hi < n ? excl[s_hi] : *total;
            t_begin = excl[s_lo] + (b - starts[lo]) * size;
            t_end = end - t_begin < size ? end : t_begin + size;
        }
        const MultiSeg S = segs[seg];
        extern __shared__ __align__(16) float smem[];
        const EnvView E = stage_environment(S.env, S.tests_in_lds, smem);
        lds_ptr wave_slab = (lds_ptr) smem + S.slab + (threadIdx.x / kWave) * slab_floats();
        rake_task_body<0, V, true>(E, wave_slab + __lane_id(), start, goal, n, bits8, steps_out, excl, t_end, FIRST ? 0u : 1u,
                                   FIRST, S.lo, S.hi, t_begin);
    }

    // workgroup b walks the edges of segment tiles[b].seg in the chunk that starts at edge 32 * tiles[b].word
    __global__ __launch_bounds__(kBlock, 2) void validate_motion_attach_multi_kernel(const MultiSeg *__restrict__ segs,
                                                                                    const MultiTile *__restrict__ tiles,
                                                                                    const float *__restrict__ start,
                                                                                    const float *__restrict__ goal,
                                                                                    const uint32_t n, uint32_t *__restrict__ bits,
                                                                                    const uint32_t chunk)
    {
        extern __shared__ __align__(16) float smem[];
        const MultiTile tile = tiles[blockIdx.x];
        const MultiSeg S = segs[tile.seg];
        const EnvView E = stage_environment(S.env, S.tests_in_lds, smem);
        const uint32_t wave = threadIdx.x / kWave;
        lds_ptr wave_slab = (lds_ptr) smem + S.slab + wave * slab_floats();
        lds_u32 *ctrl = (lds_u32 *) ((lds_ptr) smem + S.slab + kWavesPerBlock * slab_floats());
        motion_body<true>(E, wave_slab + __lane_id(), ctrl, start, goal, n, bits, chunk, S.lo, S.hi, tile.word * 32u);
    }

    __global__ __launch_bounds__(kBlock) void fk_batch_kernel(const float *__restrict__ q, const size_t n,
                                                               float4 *__restrict__ out)
    {
        const size_t i = (size_t) blockIdx.x * kBlock + threadIdx.x;
        if (i >= n) return;
        float cfg[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = q[i * R::kDim + j];
        R::sphere_fk(cfg, out + i * R::kNSpheres);
    }

    // ---------------------------------------------------------------------------------------------------------
    // vmv_clearance_batch: per configuration the smallest signed distance of a fine sphere to a contact of the
    // environment and of a fine self pair, with the witness (include/vamp_mvt_amd.h, DESIGN.md 5i).  Fused: a workgroup
    // takes a tile of kClrTile configurations; the first kClrTile lanes run Robot::sphere_fk, one configuration each, into
    // an LDS slab ([configuration][sphere] float4, rows of an odd number of float4 so that the lanes of a 128-bit read
    // fall into different bank groups) and the spheres never reach HBM.  Then lane = configuration, and the workgroup's
    // kClrStreams = kBlock / kClrTile streams share the configuration's spheres (stream t takes spheres t, t + streams,
    // ..) and then its self pairs the same way; with 64-configuration tiles a stream is a wave, and the sphere / pair
    // number and every record address are wave-uniform.  Each stream keeps (value, key) minima with a strict compare in
    // ascending key order; the streams' partial results meet in LDS and the configuration's first lane joins them, on
    // equal values the lower sphere (pair) index wins - the minimum of a total order, so it does not depend on the tile
    // size, on where the configuration sits in the batch, or on which kernel computed it.
    // LDS after the staged environment: [slab | 5 partial rows of kBlock words].
    // ---------------------------------------------------------------------------------------------------------
    constexpr uint32_t kClrRow = (uint32_t) R::kNSpheres | 1u;
    constexpr uint32_t kClrTile = (kClrRow * 64u * 16u <= 64u * 1024u) ? 64u : 32u;  // (Panda, UR5: 64; Fetch, Baxter: 32)
    constexpr uint32_t kClrStreams = (uint32_t) kBlock / kClrTile;
    constexpr uint32_t kClrSlabFloats = kClrTile * kClrRow * 4u;
    constexpr uint32_t kClrTailFloats = kClrSlabFloats + 5u * (uint32_t) kBlock;

    // configurations [first, min(first + kClrTile, hi)) of the batch; `tail` = the LDS behind the staged environment
    __device__ __forceinline__ void clearance_tile(const bool has_env, const EnvView &E, float *tail, const float *__restrict__ q,
                                                   const uint32_t first, const uint32_t hi, float *__restrict__ out,
                                                   uint32_t *__restrict__ witness)
    {
        constexpr uint32_t kNone = 0xffffffffu;
        float4 *slab = reinterpret_cast<float4 *>(tail);
        float *part_env = tail + kClrSlabFloats, *part_self = part_env + 3 * kBlock;
        uint32_t *part_key = reinterpret_cast<uint32_t *>(part_env) + kBlock, *part_sphere = part_key + kBlock;
        uint32_t *part_pair = reinterpret_cast<uint32_t *>(part_self) + kBlock;
        const uint32_t tid = threadIdx.x;
        const uint32_t c = tid % kClrTile;
        const uint32_t stream = kClrTile == (uint32_t) kWave ? uniform(tid / kClrTile) : tid / kClrTile;
        const uint32_t count = hi - first < kClrTile ? hi - first : kClrTile;
        const float4 *row = slab + c * kClrRow;
        bool finite = true;
        if (tid < kClrTile)
        {
            float cfg[R::kDim];
            const size_t at = (size_t) (c < count ? first + c : first) * R::kDim;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) cfg[j] = q[at + j];
            finite = sanitize_config<R::kDim>(cfg);  // (a non-finite configuration poses the zero configuration; its results are replaced below)
            R::sphere_fk(cfg, slab + c * kClrRow);
        }
        __syncthreads();

        float env_best = __builtin_inff();
        uint32_t env_key = kNone, env_sphere = kNone;
        if (has_env)
        {
            constexpr uint32_t kRounds = ((uint32_t) R::kNSpheres + kClrStreams - 1u) / kClrStreams;
            for (uint32_t k = 0; k < kRounds; ++k)
            {
                const uint32_t s = stream + k * kClrStreams;
                const bool live = s < (uint32_t) R::kNSpheres;
                const float4 sp = row[live ? s : 0u];
                float v = __builtin_inff();
                uint32_t key = kNone;
                sphere_clearance(E, sp.x, sp.y, sp.z, sp.w, v, key);
                const bool take = live && v < env_best;
                env_best = take ? v : env_best;
                env_key = take ? key : env_key;
                env_sphere = take ? s : env_sphere;
            }
        }
        float self_best = __builtin_inff();
        uint32_t self_pair = kNone;
        if constexpr (R::kNSelfPairs > 0)
        {
            constexpr uint32_t kRounds = ((uint32_t) R::kNSelfPairs + kClrStreams - 1u) / kClrStreams;
            for (uint32_t k = 0; k < kRounds; ++k)
            {
                const uint32_t p = stream + k * kClrStreams;
                const bool live = p < (uint32_t) R::kNSelfPairs;
                const float4 a = row[VMV_ROBOT_NS::kSelfPairs[live ? p : 0u][0]];
                const float4 b = row[VMV_ROBOT_NS::kSelfPairs[live ? p : 0u][1]];
                const float v = sqrtf(sql2_3(a.x, a.y, a.z, b.x, b.y, b.z)) - (a.w + b.w);
                const bool take = live && v < self_best;
                self_best = take ? v : self_best;
                self_pair = take ? p : self_pair;
            }
        }
        part_env[tid] = env_best, part_key[tid] = env_key, part_sphere[tid] = env_sphere;
        part_self[tid] = self_best, part_pair[tid] = self_pair;
        __syncthreads();
        if (tid < count)  // (stream 0 of configuration c: its own partial results are the start)
        {
            for (uint32_t t = 1; t < kClrStreams; ++t)
            {
                const uint32_t o = t * kClrTile + c;
                const float v = part_env[o];
                const uint32_t s = part_sphere[o];
                if (v < env_best || (v == env_best && s < env_sphere)) env_best = v, env_key = part_key[o], env_sphere = s;
                const float w = part_self[o];
                const uint32_t p = part_pair[o];
                if (w < self_best || (w == self_best && p < self_pair)) self_best = w, self_pair = p;
            }
            const size_t i = (size_t) first + c;
            const float nan = __builtin_nanf("");
            out[2 * i] = finite ? env_best : nan;
            out[2 * i + 1] = finite ? self_best : nan;
            if (witness)
            {
                const bool some = finite && env_key != kNone;
                witness[4 * i] = some ? env_sphere : kNone;
                witness[4 * i + 1] = some ? env_key >> kClearanceKindShift : kNone;
                witness[4 * i + 2] = some ? env_key & ((1u << kClearanceKindShift) - 1u) : kNone;
                witness[4 * i + 3] = finite ? self_pair : kNone;
            }
        }
    }

    // Workgroup b takes tile b.  n is 32-bit: the launcher cuts larger batches into slices.  env == nullptr: the self
    // clearance alone.  (Both kernels are templates for their place in the code object alone: instantiations are emitted
    // at the end of the translation unit, so every kernel that was there before keeps its address.)
    template <int = 0>
    __global__ __launch_bounds__(kBlock) void clearance_kernel(const EnvDev *__restrict__ env, const uint32_t head,
                                                                const float *__restrict__ q, const uint32_t n,
                                                                float *__restrict__ out, uint32_t *__restrict__ witness)
    {
        extern __shared__ __align__(16) float smem[];
        EnvView E{};
        if (env) E = stage_environment(env, 0u, smem);  // (workgroup-uniform)
        // one tile per workgroup, no loop: around a loop over tiles the FK's constants and the tile's addresses stayed live
        // (Fetch: 254 VGPRs against 169)
        clearance_tile(env != nullptr, E, smem + head, q, blockIdx.x * kClrTile, n, out, witness);
    }

    // vmv_clearance_batch_multi: workgroup b takes tile b of the table, MultiTile::word = the tile's first configuration,
    // and stages that tile's environment; the body is the single-environment one.
    template <int = 0>
    __global__ __launch_bounds__(kBlock) void clearance_multi_kernel(const MultiSeg *__restrict__ segs,
                                                                      const MultiTile *__restrict__ tiles,
                                                                      const float *__restrict__ q, float *__restrict__ out,
                                                                      uint32_t *__restrict__ witness)
    {
        extern __shared__ __align__(16) float smem[];
        const MultiTile tile = tiles[blockIdx.x];
        const MultiSeg S = segs[tile.seg];
        const EnvView E = stage_environment(S.env, 0u, smem);
        clearance_tile(true, E, smem + S.slab, q, tile.word, S.hi, out, witness);
    }

    // ---------------------------------------------------------------------------------------------------------
    // vmv_clearance_grad_batch: the joint-space gradients of the two clearances with the witness held fixed
    // (include/vamp_mvt_amd.h, DESIGN.md 5j).  Runs behind the unchanged clearance kernel on the same stream and reads the
    // witness that kernel wrote, so values and witness are the clearance call's by construction.  One lane = one
    // configuration: Robot::sphere_fk_grad gives the centres and 3 x dim Jacobians of the three witness spheres, the ONE
    // witness record is fetched per lane from the environment's HBM block (no staging, no LDS), the normal is
    // prim_offset's c - p, normalised, and grad[i] = [env | self][dim] leaves through plain vector stores.  A witness that names nothing
    // (and one that is out of range: never written by the clearance kernel, never followed) gives zeros; a non-finite
    // joint gives 2 * dim NaNs.  Workgroups of one wave: the Jacobians alone are 9 * dim registers.
    // ---------------------------------------------------------------------------------------------------------
    constexpr uint32_t kGradBlock = (uint32_t) kWave;

    __device__ __forceinline__ void clearance_grad_lane(const EnvDev *__restrict__ env, const float *__restrict__ q, const size_t i,
                                                        const uint32_t *__restrict__ witness, float *__restrict__ grad)
    {
        constexpr uint32_t kNone = 0xffffffffu;
        float cfg[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = q[i * R::kDim + j];
        const bool finite = sanitize_config<R::kDim>(cfg);
        const uint32_t w_sphere = witness[4 * i], w_kind = witness[4 * i + 1], w_index = witness[4 * i + 2];
        const uint32_t w_pair = witness[4 * i + 3];

        // which record, if any: kind and index checked against the environment's own counts; its float4s are fetched here,
        // in front of the kinematics
        const env_cptr D = (env_cptr) env;
        bool has_env = false;
        v4f ra = {0.f, 0.f, 0.f, 0.f}, rb = ra, rc = ra, rd = ra;
        if (env != nullptr && w_sphere < (uint32_t) R::kNSpheres)
        {
            const uint32_t n_kind = w_kind == (uint32_t) kSphere ? D->n_sphere : w_kind == (uint32_t) kCapsule ? D->n_capsule :
                                    w_kind == (uint32_t) kZCapsule ? D->n_zcapsule : w_kind == (uint32_t) kCuboid ? D->n_cuboid :
                                    w_kind == (uint32_t) kZCuboid ? D->n_zcuboid :
                                    w_kind == kClearanceHeightfield ? D->n_heightfield : 0u;
            has_env = w_index < n_kind;
            if (has_env && w_kind != kClearanceHeightfield)
            {
                const uint32_t off = w_kind == (uint32_t) kSphere ? D->off_sphere + w_index * (uint32_t) kSphereRec :
                                     w_kind == (uint32_t) kCapsule ? D->off_capsule + w_index * (uint32_t) kCapsuleRec :
                                     w_kind == (uint32_t) kZCapsule ? D->off_zcapsule + w_index * (uint32_t) kZCapsuleRec :
                                     w_kind == (uint32_t) kCuboid ? D->off_cuboid + w_index * (uint32_t) kCuboidRec :
                                                                    D->off_zcuboid + w_index * (uint32_t) kZCuboidRec;
                const g_v4f *rec = (const g_v4f *) ((gf_cptr) D->prims + off);
                ra = rec[0], rb = rec[1];  // (every record has two float4s)
                if (w_kind == (uint32_t) kCapsule || w_kind == (uint32_t) kCuboid || w_kind == (uint32_t) kZCuboid) rc = rec[2];
                if (w_kind == (uint32_t) kCuboid) rd = rec[3];
            }
        }
        uint32_t sa = kNone, sb = kNone;
        if constexpr (R::kNSelfPairs > 0)
        {
            const bool has_self = w_pair < (uint32_t) R::kNSelfPairs;
            sa = has_self ? (uint32_t) VMV_ROBOT_NS::kSelfPairs[has_self ? w_pair : 0u][0] : kNone;
            sb = has_self ? (uint32_t) VMV_ROBOT_NS::kSelfPairs[has_self ? w_pair : 0u][1] : kNone;
        }

        float c[3][3], J[3][3][R::kDim];
        R::sphere_fk_grad(cfg, has_env ? w_sphere : kNone, sa, sb, c, J);

        // c - p of every kind on the one record, the witness's kind picked by selects (vmv_device.h: prim_offset); a
        // heightfield's value is z - r - height(cell) with the cell held fixed: (0, 0, 1); no witness: 0
        float nx = 0.0f, ny = 0.0f, nz = has_env && w_kind == kClearanceHeightfield ? 1.0f : 0.0f;
        {
            const bool prim = has_env && w_kind != kClearanceHeightfield;
            float x, y, z;
            prim_offset<kSphere>(ra, rb, rc, rd, c[0][0], c[0][1], c[0][2], x, y, z);
            nx = prim && w_kind == (uint32_t) kSphere ? x : nx, ny = prim && w_kind == (uint32_t) kSphere ? y : ny;
            nz = prim && w_kind == (uint32_t) kSphere ? z : nz;
            prim_offset<kCapsule>(ra, rb, rc, rd, c[0][0], c[0][1], c[0][2], x, y, z);
            nx = prim && w_kind == (uint32_t) kCapsule ? x : nx, ny = prim && w_kind == (uint32_t) kCapsule ? y : ny;
            nz = prim && w_kind == (uint32_t) kCapsule ? z : nz;
            prim_offset<kZCapsule>(ra, rb, rc, rd, c[0][0], c[0][1], c[0][2], x, y, z);
            nx = prim && w_kind == (uint32_t) kZCapsule ? x : nx, ny = prim && w_kind == (uint32_t) kZCapsule ? y : ny;
            nz = prim && w_kind == (uint32_t) kZCapsule ? z : nz;
            prim_offset<kCuboid>(ra, rb, rc, rd, c[0][0], c[0][1], c[0][2], x, y, z);
            nx = prim && w_kind == (uint32_t) kCuboid ? x : nx, ny = prim && w_kind == (uint32_t) kCuboid ? y : ny;
            nz = prim && w_kind == (uint32_t) kCuboid ? z : nz;
            prim_offset<kZCuboid>(ra, rb, rc, rd, c[0][0], c[0][1], c[0][2], x, y, z);
            nx = prim && w_kind == (uint32_t) kZCuboid ? x : nx, ny = prim && w_kind == (uint32_t) kZCuboid ? y : ny;
            nz = prim && w_kind == (uint32_t) kZCuboid ? z : nz;
        }
        unit3(nx, ny, nz);
        float mx = c[1][0] - c[2][0], my = c[1][1] - c[2][1], mz = c[1][2] - c[2][2];  // (no self witness: both centres are 0)
        unit3(mx, my, mz);
        // g + 0 = g (and +0 for -0), g + NaN = NaN: the non-finite configuration's NaNs without a branch around the sums
        const float poison = finite ? 0.0f : __builtin_nanf("");
        float *out = grad + i * (size_t) (2 * R::kDim);
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) out[j] = dot3(nx, ny, nz, J[0][0][j], J[0][1][j], J[0][2][j]) + poison;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
            out[R::kDim + j] = dot3(mx, my, mz, J[1][0][j] - J[2][0][j], J[1][1][j] - J[2][1][j], J[1][2][j] - J[2][2][j]) + poison;
    }

    // n is 32-bit: the launcher cuts larger batches into the clearance kernel's slices.  (Templates for their place in the
    // code object, as the two kernels above.)
    template <int = 0>
    __global__ __launch_bounds__(kGradBlock) void clearance_grad_kernel(const EnvDev *__restrict__ env, const float *__restrict__ q,
                                                                        const uint32_t n, const uint32_t *__restrict__ witness,
                                                                        float *__restrict__ grad)
    {
        const uint32_t i = blockIdx.x * kGradBlock + threadIdx.x;
        if (i < n) clearance_grad_lane(env, q, i, witness, grad);
    }

    // vmv_clearance_grad_batch_multi: the (segment, first configuration) tiles of clearance_multi_kernel, kGradBlock /
    // kClrTile of them per workgroup; a lane finds its environment through its tile's segment.
    template <int = 0>
    __global__ __launch_bounds__(kGradBlock) void clearance_grad_multi_kernel(const MultiSeg *__restrict__ segs,
                                                                              const MultiTile *__restrict__ tiles,
                                                                              const uint32_t n_tiles, const float *__restrict__ q,
                                                                              const uint32_t *__restrict__ witness,
                                                                              float *__restrict__ grad)
    {
        const uint32_t t = blockIdx.x * (kGradBlock / kClrTile) + threadIdx.x / kClrTile;
        if (t >= n_tiles) return;
        const MultiTile tile = tiles[t];
        const MultiSeg S = segs[tile.seg];
        const uint32_t i = tile.word + threadIdx.x % kClrTile;
        if (i < S.hi) clearance_grad_lane(S.env, q, i, witness, grad);
    }

    // ---------------------------------------------------------------------------------------------------------
    // vmv_eefk_jacobian_batch and vmv_ik_batch (include/vamp_mvt_amd.h, DESIGN.md 5k).  One lane = one configuration
    // (one (target, seed) pair), workgroups of one wave, no LDS, no atomics; Robot::ee_frame_jac gives the frame and the
    // tangents of its twelve entries.  A joint outside R::kEeJointMask (Baxter's other arm) has literal-zero tangents and
    // is left out of every sum at compile time.  Both kernels are templates for their place in the code object, as the
    // clearance kernels above.
    // ---------------------------------------------------------------------------------------------------------
    constexpr uint32_t kIkBlock = (uint32_t) kWave;
    constexpr float kIkLambdaFactor = 4.0f, kIkLambdaFloor = 1e-5f, kIkLambdaCeil = 1e6f;  // tests/ik_serial.py states the same
    __host__ __device__ constexpr bool ee_joint(const int j) { return ((R::kEeJointMask >> j) & 1u) != 0u; }

    // The geometric Jacobian in the world frame from a frame f (ee_frame's layout: f[3 + 3 k + a] = R[a][k]) and its
    // tangents: rows 0-2 dt/dq_j, rows 3-5 the angular velocity omega_j = vee(A), A = (dR/dq_j) R^T, every entry of A as
    // ((a0 b0 + a1 b1) + a2 b2).
    __device__ __forceinline__ void ee_jacobian(const float (&f)[12], const float (&df)[12][R::kDim], float (&J)[6][R::kDim])
    {
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            if (ee_joint(j))
            {
                const auto A = [&](const int a, const int b)
                { return ((df[3 + a][j] * f[3 + b]) + (df[6 + a][j] * f[6 + b])) + (df[9 + a][j] * f[9 + b]); };
                J[0][j] = df[0][j], J[1][j] = df[1][j], J[2][j] = df[2][j];
                J[3][j] = 0.5f * (A(2, 1) - A(1, 2));
                J[4][j] = 0.5f * (A(0, 2) - A(2, 0));
                J[5][j] = 0.5f * (A(1, 0) - A(0, 1));
            }
            else
                J[0][j] = J[1][j] = J[2][j] = J[3][j] = J[4][j] = J[5][j] = 0.0f;
        }
    }

    // frames [n][16] (nullptr: not wanted) exactly as eefk_batch_kernel writes them - the same primal operations on the
    // same joints, so a non-finite joint gives that kernel's frame - and jac [n][6][dim]; a non-finite joint: 6 * dim NaNs
    // (J + 0 = J, J + NaN = NaN, as the clearance gradient's).
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void eefk_jacobian_kernel(const float *__restrict__ q, const uint32_t n,
                                                                     float *__restrict__ frames, float *__restrict__ jac)
    {
        const uint32_t i = blockIdx.x * kIkBlock + threadIdx.x;
        if (i >= n) return;
        float cfg[R::kDim], f[12], df[12][R::kDim], J[6][R::kDim];
        bool finite = true;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            cfg[j] = q[(size_t) i * R::kDim + j];
            finite = finite && __builtin_isfinite(cfg[j]);
        }
        R::ee_frame_jac(cfg, f, df);
        ee_jacobian(f, df, J);
        if (frames != nullptr)
        {
            float *o = frames + 16 * (size_t) i;
#pragma unroll
            for (int r = 0; r < 3; ++r)
            {
#pragma unroll
                for (int k = 0; k < 3; ++k) o[4 * r + k] = f[3 + 3 * k + r];
                o[4 * r + 3] = f[r];
            }
            o[12] = o[13] = o[14] = 0.0f;
            o[15] = 1.0f;
        }
        const float poison = finite ? 0.0f : __builtin_nanf("");
        float *out = jac + (size_t) i * (6 * R::kDim);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) out[r * R::kDim + j] = J[r][j] + poison;
    }

    // The pose error of frame f against the target T (both in ee_frame's layout): e[0..2] = t* - t; e_w = 1/2 sum_k R_k x
    // R*_k over the three columns, |e_w| = sin(theta); where tr(R*^T R) <= 1 (theta >= 90 degrees) the weighted error
    // carries e_w at unit length.  e[3..5] = w * e_w (rescaled); n_p = |e_p|, n_w = |e_w| unrescaled.  The quotient stands
    // outside the select (DESIGN.md 5j: a quotient on one side of a select makes a conditional region).
    __device__ __forceinline__ void ik_error(const float (&f)[12], const float (&T)[12], const float w, float (&e)[6], float &n_p,
                                             float &n_w, float &tr)
    {
        e[0] = T[0] - f[0], e[1] = T[1] - f[1], e[2] = T[2] - f[2];
        float cx[3], cy[3], cz[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            const float a0 = f[3 + 3 * k], a1 = f[4 + 3 * k], a2 = f[5 + 3 * k];
            const float b0 = T[3 + 3 * k], b1 = T[4 + 3 * k], b2 = T[5 + 3 * k];
            cx[k] = (a1 * b2) - (a2 * b1), cy[k] = (a2 * b0) - (a0 * b2), cz[k] = (a0 * b1) - (a1 * b0);
            d[k] = dot3(a0, a1, a2, b0, b1, b2);
        }
        const float wx = 0.5f * ((cx[0] + cx[1]) + cx[2]), wy = 0.5f * ((cy[0] + cy[1]) + cy[2]), wz = 0.5f * ((cz[0] + cz[1]) + cz[2]);
        tr = (d[0] + d[1]) + d[2];
        n_p = sqrtf(dot3(e[0], e[1], e[2], e[0], e[1], e[2]));
        n_w = sqrtf(dot3(wx, wy, wz, wx, wy, wz));
        const float s = w / ((tr <= 1.0f && n_w > 0.0f) ? n_w : 1.0f);
        e[3] = s * wx, e[4] = s * wy, e[5] = s * wz;
    }

    // the rows of ik_error's weighted error: the Jacobian's, the angular ones times w
    __device__ __forceinline__ void ik_weigh(const float w, float (&J)[6][R::kDim])
    {
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
            if (ee_joint(j))
            {
#pragma unroll
                for (int r = 3; r < 6; ++r) J[r][j] = w * J[r][j];
            }
    }

    // y = A^-1 b for the symmetric positive definite A = Jm Jm^T + lambda I (its lower triangle), by a Cholesky
    // factorisation in registers: every loop has constant bounds and unrolls.  A pivot that rounding took to zero or below
    // is raised to 1e-12 (lambda >= kIkLambdaFloor keeps it away from there but for rounding).
    __device__ __forceinline__ void chol6_solve(const float (&A)[6][6], const float (&b)[6], float (&y)[6])
    {
        float L[6][6], inv[6], z[6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j)
            {
                float s = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
                if (i == j)
                {
                    L[i][i] = sqrtf(fmaxf(s, 1e-12f));
                    inv[i] = 1.0f / L[i][i];
                }
                else
                    L[i][j] = s * inv[j];
            }
#pragma unroll
        for (int i = 0; i < 6; ++i)
        {
            float s = b[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
            z[i] = s * inv[i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i)
        {
            float s = z[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s -= L[k][i] * y[k];
            y[i] = s * inv[i];
        }
    }

    // The damped least-squares (Levenberg-Marquardt) iteration, stated once for ik_kernel and cartesian_track_kernel
    // (DESIGN.md 5k; constraint_project_lane writes the same out, see there); tests/ik_serial.py states it in float64
    // (step, damped).  A loop body is ONE evaluation of a candidate - the start first, then lm_step's - followed by
    // lm_accept's selects into the accepted state: a rejected step keeps the old rows in registers and nothing is
    // evaluated twice.  The three functions hold no branch, so with the caller's wave-uniform exit the compiler has no
    // conditional region to sink the tape into; every fp32 operation stands in the order the callers' results are
    // pinned to.
    struct LmState  // the accepted state
    {
        float q[R::kDim];      // the configuration
        float Jw[6][R::kDim];  // its weighted rows: the caller's error e has the Jacobian de/dq = -Jw
        float e[6], E, lam;    // the weighted error, E = 1/2 |e|^2, the damping lambda
    };

    // the start: the candidate clipped to the bounds; no rows, E = inf, lambda = damping
    template <class Params>
    __device__ __forceinline__ void lm_start(const Params &P, float (&cand)[R::kDim], LmState &S)
    {
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            cand[j] = fminf(fmaxf(cand[j], P.lower[j]), P.upper[j]);
            S.q[j] = cand[j];
#pragma unroll
            for (int r = 0; r < 6; ++r) S.Jw[r][j] = 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) S.e[r] = 0.0f;
        S.E = __builtin_inff(), S.lam = P.damping;
    }

    // the accept: the candidate (its weighted rows Jc, its error ec and Ec) is taken if it lowers E - the first whatever
    // it gives, which leaves lambda alone; a lane that is done takes nothing.  lambda falls by kIkLambdaFactor after a step
    // that was taken and rises after one that was not; evals counts the candidates after the first.  -> taken
    __device__ __forceinline__ bool lm_accept(const bool first, const bool done, const float (&cand)[R::kDim], const float (&Jc)[6][R::kDim],
                                              const float (&ec)[6], const float Ec, LmState &S, uint32_t &evals)
    {
        const bool take = !done && (first || Ec < S.E);
        const float lam_next = take ? fmaxf(S.lam * (1.0f / kIkLambdaFactor), kIkLambdaFloor) : fminf(S.lam * kIkLambdaFactor, kIkLambdaCeil);
        S.lam = (done || first) ? S.lam : lam_next;
        evals += (done || first) ? 0u : 1u;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            S.q[j] = take ? cand[j] : S.q[j];
            if (ee_joint(j))
            {
#pragma unroll
                for (int r = 0; r < 6; ++r) S.Jw[r][j] = take ? Jc[r][j] : S.Jw[r][j];
            }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) S.e[r] = take ? ec[r] : S.e[r];
        S.E = take ? Ec : S.E;
        return take;
    }

    // the step from the accepted state: A = Jm Jm^T + lambda I, A y = e, delta = Jm^T y, capped at max_step; the next
    // candidate is q + delta clipped to the bounds.  Jm: a joint that sits at a bound while the descent direction g = Jw^T e
    // points outward is left out of the step (its column of Jw reads as zero), so the other joints are not asked to make
    // up for a motion the clip will take away.
    template <class Params>
    __device__ __forceinline__ void lm_step(const Params &P, const LmState &S, float (&cand)[R::kDim])
    {
        float Jm[6][R::kDim], A[6][6], y[6], delta[R::kDim], big = 0.0f;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
            if (ee_joint(j))
            {
                float g = S.Jw[0][j] * S.e[0];
#pragma unroll
                for (int r = 1; r < 6; ++r) g += S.Jw[r][j] * S.e[r];
                const bool hold = (S.q[j] <= P.lower[j] && g < 0.0f) || (S.q[j] >= P.upper[j] && g > 0.0f);
#pragma unroll
                for (int r = 0; r < 6; ++r) Jm[r][j] = hold ? 0.0f : S.Jw[r][j];
            }
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b)
            {
                float s = a == b ? S.lam : 0.0f;
#pragma unroll
                for (int j = 0; j < R::kDim; ++j)
                    if (ee_joint(j)) s += Jm[a][j] * Jm[b][j];
                A[a][b] = s;
            }
        chol6_solve(A, S.e, y);
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            delta[j] = 0.0f;
            if (ee_joint(j))
            {
                float s = Jm[0][j] * y[0];
#pragma unroll
                for (int r = 1; r < 6; ++r) s += Jm[r][j] * y[r];
                delta[j] = s;
                big = fmaxf(big, fabsf(s));
            }
        }
        const float scale = P.max_step / fmaxf(big, P.max_step);  // 1 while the largest joint change is within max_step
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
            cand[j] = ee_joint(j) ? fminf(fmaxf(S.q[j] + delta[j] * scale, P.lower[j]), P.upper[j]) : S.q[j];
    }

    // vmv_ik_batch: the iteration above from one seed towards one target per lane (lane i: target i / n_seeds, seed i, or
    // seed i % n_seeds of the shared Halton seeds), its rows the Jacobian's with rot_weight on the angular ones.  There is
    // no branch in the loop but the wave-uniform exit.  A lane's result depends on its own target, seed and settings
    // alone.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void ik_kernel(const IkParams P, const float *__restrict__ targets,
                                                          const float *__restrict__ seeds, const uint32_t n,
                                                          float *__restrict__ q_out, float *__restrict__ err_out,
                                                          uint32_t *__restrict__ status_out)
    {
        const uint32_t i = blockIdx.x * kIkBlock + threadIdx.x;
        const bool in_range = i < n;
        const uint32_t row = in_range ? i : 0u;  // (a lane past the end works on row 0 and writes nothing)
        const float *const tp = targets + 16 * (size_t) (row / P.n_seeds);
        const float *const sp = seeds + (size_t) (P.seeds_shared != 0u ? row % P.n_seeds : row) * R::kDim;
        float T[12], cand[R::kDim];
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const float v = tp[4 * r + k];
                finite = finite && __builtin_isfinite(v);
                if (r < 3) T[k < 3 ? 3 + 3 * k + r : r] = v;
            }
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            cand[j] = sp[j];
            finite = finite && __builtin_isfinite(cand[j]);
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = finite ? T[k] : 0.0f;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cand[j] = finite ? cand[j] : 0.0f;

        LmState W;
        lm_start(P, cand, W);
        float err_p = 0.0f, err_w = 0.0f;
        bool done = !in_range || !finite, converged = false;
        uint32_t evals = 0;
        for (uint32_t it = 0;; ++it)
        {
            // ---- one evaluation: the candidate's frame, weighted Jacobian, error and E
            float f[12], df[12][R::kDim], Jc[6][R::kDim], ec[6], n_p, n_w, tr;
            R::ee_frame_jac(cand, f, df);
            ee_jacobian(f, df, Jc);
            ik_error(f, T, P.rot_weight, ec, n_p, n_w, tr);
            ik_weigh(P.rot_weight, Jc);
            const float Ec = 0.5f * (dot3(ec[0], ec[1], ec[2], ec[0], ec[1], ec[2]) + dot3(ec[3], ec[4], ec[5], ec[3], ec[4], ec[5]));
            const bool take = lm_accept(it == 0u, done, cand, Jc, ec, Ec, W, evals);
            const bool ok = n_p <= P.pos_tol && (P.position_only != 0u || (tr > 1.0f && n_w <= P.rot_tol));
            err_p = take ? n_p : err_p, err_w = take ? n_w : err_w;
            converged = converged || (take && ok);
            done = done || (take && ok);
            if (it == P.max_iterations || !wave_any(!done)) break;
            lm_step(P, W, cand);
        }
        if (!in_range) return;
        // invalid input: the seed as given, NaN errors, bit 30
        const float poison = finite ? 0.0f : __builtin_nanf("");
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) q_out[(size_t) i * R::kDim + j] = finite ? W.q[j] : sp[j];
        if (err_out != nullptr) err_out[2 * (size_t) i] = err_p + poison, err_out[2 * (size_t) i + 1] = err_w + poison;
        status_out[i] = (converged ? 0x80000000u : 0u) | (finite ? 0u : 0x40000000u) | evals;
    }

    // vmv_cartesian_multi's tracking (include/vamp_mvt_amd.h, DESIGN.md 5m): one lane walks one line.  The outer loop
    // runs over the poses k = 1 .. m of the lane's line, the inner loop is ik_kernel's from waypoint k - 1 towards pose
    // k: the same evaluation and the same lm_start, lm_accept and lm_step, so a waypoint is ik_kernel's answer.  Both loops
    // have bounds of their own (P.max_k <= 1,023 poses, P.max_iterations evaluations after the first) and both end on a
    // wave-uniform test; a lane whose line is shorter, has stopped or has converged rides along through selects, so a
    // lane's result depends on its own record, start and settings alone.  The host hands only finite records and starts
    // (a problem with a non-finite entry has m == 0), so there is nothing to poison.  The only conditional code is the
    // store of an accepted waypoint: plain vector stores under the lane mask, no form of the tape.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void cartesian_track_kernel(const CartParams P, const CartLine *__restrict__ lines,
                                                                       const float *__restrict__ starts, const uint32_t n,
                                                                       float *__restrict__ points, CartResult *__restrict__ results)
    {
        const uint32_t i = blockIdx.x * kIkBlock + threadIdx.x;
        const bool in_range = i < n;
        const uint32_t row = in_range ? i : 0u;  // (a lane past the end reads row 0 and writes nothing)
        const CartLine L = lines[row];
        const uint32_t m = in_range ? L.m : 0u;
        const float mf = (float) (m > 0u ? m : 1u);
        float *const out = points + (size_t) L.offset * R::kDim;
        float prev[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) prev[j] = starts[(size_t) row * R::kDim + j];
        const float ax = L.axis[0], ay = L.axis[1], az = L.axis[2];
        bool stopped = false;
        uint32_t tracked = 0u, status = (uint32_t) VMV_CART_COMPLETE, evals = 0u;

        for (uint32_t k = 1u; k <= P.max_k; ++k)
        {
            const bool active = !stopped && k <= m;
            if (!wave_any(active)) break;

            // ---- pose k of the line in ee_frame's layout: p0 + s dp, R0 Rot(axis, s theta) by Rodrigues' formula
            const float s = (float) k / mf;
            const float ang = s * L.theta, sn = vsin(ang), cs = vcos(ang), vs = 1.0f - cs;
            const float vx = vs * ax, vy = vs * ay, vz = vs * az;
            float Q[3][3], T[12];
            Q[0][0] = cs + vx * ax, Q[0][1] = vx * ay - sn * az, Q[0][2] = vx * az + sn * ay;
            Q[1][0] = vy * ax + sn * az, Q[1][1] = cs + vy * ay, Q[1][2] = vy * az - sn * ax;
            Q[2][0] = vz * ax - sn * ay, Q[2][1] = vz * ay + sn * ax, Q[2][2] = cs + vz * az;
#pragma unroll
            for (int a = 0; a < 3; ++a)
            {
                T[a] = L.p0[a] + s * L.dp[a];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    T[3 + 3 * c + a] = dot3(L.R0[3 * a], L.R0[3 * a + 1], L.R0[3 * a + 2], Q[0][c], Q[1][c], Q[2][c]);
            }

            // ---- ik_kernel's loop from waypoint k - 1 (clipped to the bounds, as a seed is)
            float cand[R::kDim];
            LmState W;
            bool done = !active, converged = false;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) cand[j] = prev[j];
            lm_start(P, cand, W);
            for (uint32_t it = 0;; ++it)
            {
                float f[12], df[12][R::kDim], Jc[6][R::kDim], ec[6], n_p, n_w, tr;
                R::ee_frame_jac(cand, f, df);
                ee_jacobian(f, df, Jc);
                ik_error(f, T, P.rot_weight, ec, n_p, n_w, tr);
                ik_weigh(P.rot_weight, Jc);
                const float Ec = 0.5f * (dot3(ec[0], ec[1], ec[2], ec[0], ec[1], ec[2]) + dot3(ec[3], ec[4], ec[5], ec[3], ec[4], ec[5]));
                const bool take = lm_accept(it == 0u, done, cand, Jc, ec, Ec, W, evals);
                const bool ok = n_p <= P.pos_tol && (P.position_only != 0u || (tr > 1.0f && n_w <= P.rot_tol));
                converged = converged || (take && ok);
                done = done || (take && ok);
                if (it == P.max_iterations || !wave_any(!done)) break;
                lm_step(P, W, cand);
            }

            // ---- the waypoint is accepted if it converged within max_joint_step of waypoint k - 1
            float jump = 0.0f;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) jump = fmaxf(jump, fabsf(W.q[j] - prev[j]));
            const bool good = converged && jump <= P.max_joint_step;
            const bool keep = active && good;
            status = (active && !good) ? (uint32_t) (converged ? VMV_CART_JOINT_JUMP : VMV_CART_IK_FAILED) : status;
            stopped = stopped || (active && !good);
            tracked += keep ? 1u : 0u;
            if (keep)  // k <= m: inside the problem's m + 1 rows
            {
#pragma unroll
                for (int j = 0; j < R::kDim; ++j) out[(size_t) k * R::kDim + j] = W.q[j];
            }
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) prev[j] = keep ? W.q[j] : prev[j];
        }
        if (in_range) results[i] = CartResult{tracked, status, evals, 0u};
    }

    // ---------------------------------------------------------------------------------------------------------
    // End-effector constraints (include/vamp_mvt_amd.h: vmv_constraint_*_batch, DESIGN.md 5o).  csrc/vmv_constraint.h
    // states the residual, the band test, the projection and the edge test; the functions below are that statement in
    // fp32, and every kernel asks them, so a question has one answer wherever it is asked.  Templates for their place in
    // the code object, as the kernels above.
    // ---------------------------------------------------------------------------------------------------------
    struct ConstraintState  // what constraint_residual reads off one frame
    {
        float v[3];        // p - clamp(p, lo, hi) along C's axes
        float a[3], n[3];  // the tool axis in the world; c / |c|, c = a x d
        float s;           // the excess: sin(angle - max_angle), 1 beyond 90 degrees of excess
        float sn, cs;      // |a x d|, a . d
        bool tilted;       // the axis part is active: cos < cos_m
        bool anti;         // antiparallel axes: no direction to turn in
        bool band;         // the band test
    };
    __device__ __forceinline__ void constraint_residual(const float (&f)[12], const ConstraintDev &C, ConstraintState &S)
    {
        const float d0 = f[0] - C.t[0], d1 = f[1] - C.t[1], d2 = f[2] - C.t[2];
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            const float p = dot3(C.R[k], C.R[3 + k], C.R[6 + k], d0, d1, d2);
            S.v[k] = p - fminf(fmaxf(p, C.lo[k]), C.hi[k]);
            in = in && p >= C.lo_band[k] && p <= C.hi_band[k];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) S.a[r] = dot3(f[3 + r], f[6 + r], f[9 + r], C.u[0], C.u[1], C.u[2]);
        const float cx = (S.a[1] * C.d[2]) - (S.a[2] * C.d[1]), cy = (S.a[2] * C.d[0]) - (S.a[0] * C.d[2]),
                    cz = (S.a[0] * C.d[1]) - (S.a[1] * C.d[0]);
        S.sn = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
        S.cs = dot3(S.a[0], S.a[1], S.a[2], C.d[0], C.d[1], C.d[2]);
        const float inv = 1.0f / (S.sn > 0.0f ? S.sn : 1.0f);  // (the quotient stands outside the select, as ik_error's)
        S.n[0] = cx * inv, S.n[1] = cy * inv, S.n[2] = cz * inv;
        const float far = (S.cs * C.cos_m) + (S.sn * C.sin_m);
        const float near = (S.sn * C.cos_m) - (S.cs * C.sin_m);
        S.s = far <= 0.0f ? 1.0f : near;
        const bool axis = C.axis != 0u;
        S.tilted = axis && S.cs < C.cos_m;
        S.anti = axis && S.sn == 0.0f && S.cs < 0.0f;
        S.band = in && (!axis || S.cs >= C.cos_band);
    }
    // the residual pair of a state: |v| (m), the angle beyond max_angle (rad)
    __device__ __forceinline__ void constraint_report(const ConstraintState &S, const ConstraintDev &C, float &res_p, float &res_w)
    {
        res_p = sqrtf(dot3(S.v[0], S.v[1], S.v[2], S.v[0], S.v[1], S.v[2]));
        const float over = atan2f((S.sn * C.cos_m) - (S.cs * C.sin_m), (S.cs * C.cos_m) + (S.sn * C.sin_m));
        res_w = S.tilted ? over : 0.0f;
    }

    // The projection of one lane's configuration `in` (vmv_constraint.h): ik_kernel's loop - one evaluation per pass,
    // selects into the accepted state, no branch but the wave-uniform exit - with the constraint's rows.  The loop is
    // written out here, statement for statement what lm_start, lm_accept and lm_step state.  Calling all three from this
    // lane made project_batch 1 - 3 % and the constrained planner 2 - 6 % slower on the MI355X, calling the schedule and
    // lm_step alone about 1 % (registers as now; DESIGN.md 5o has both measurements), each outside the parent's spread.
    // tests/test_lm_pins_gpu.py holds this copy and the shared statement to the same recorded outputs.  Every lane of
    // the wave calls it; a lane with `live` false rides along and its outputs mean nothing.  q: the result (`in` itself
    // for a non-finite or antiparallel input); status as the kernel writes it.
    __device__ __forceinline__ void constraint_project_lane(const ConstraintParams &P, const ConstraintDev &C, const float (&in)[R::kDim],
                                                            const bool live, float (&q_out)[R::kDim], float &res_p, float &res_w,
                                                            uint32_t &status)
    {
        float cand[R::kDim];
        bool finite = true;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) finite = finite && __builtin_isfinite(in[j]);
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cand[j] = fminf(fmaxf(finite ? in[j] : 0.0f, P.lower[j]), P.upper[j]);

        float q[R::kDim], Jw[6][R::kDim], e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float E = __builtin_inff(), lam = P.damping;
        ConstraintState acc{};
        bool done = !live || !finite, converged = false, given = !finite;
        uint32_t evals = 0;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            q[j] = cand[j];
#pragma unroll
            for (int r = 0; r < 6; ++r) Jw[r][j] = 0.0f;
        }
        for (uint32_t it = 0;; ++it)
        {
            // ---- one evaluation: the candidate's frame, Jacobian, residual and E
            float f[12], df[12][R::kDim], Jc[6][R::kDim], ec[6];
            ConstraintState S;
            R::ee_frame_jac(cand, f, df);
            ee_jacobian(f, df, Jc);
            constraint_residual(f, C, S);
            const float b0 = (S.a[1] * S.n[2]) - (S.a[2] * S.n[1]), b1 = (S.a[2] * S.n[0]) - (S.a[0] * S.n[2]),
                        b2 = (S.a[0] * S.n[1]) - (S.a[1] * S.n[0]);  // a x n
            ec[0] = -S.v[0], ec[1] = -S.v[1], ec[2] = -S.v[2];
            ec[3] = S.tilted ? P.rot_weight * S.s : 0.0f, ec[4] = 0.0f, ec[5] = 0.0f;
            const float Ec = 0.5f * (dot3(ec[0], ec[1], ec[2], ec[0], ec[1], ec[2]) + (ec[3] * ec[3]));
            const bool first = it == 0u;  // the input's evaluation is taken whatever it gives and leaves lambda alone
            const bool stuck = first && S.anti && !done;  // antiparallel input: as given, not converged
            const bool take = !done && (first || Ec < E);
            const float lam_next = take ? fmaxf(lam * (1.0f / kIkLambdaFactor), kIkLambdaFloor) : fminf(lam * kIkLambdaFactor, kIkLambdaCeil);
            lam = (done || first) ? lam : lam_next;
            evals += (done || first) ? 0u : 1u;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
            {
                q[j] = take ? cand[j] : q[j];
                if (ee_joint(j))
                {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                    {
                        const float row = dot3(C.R[k], C.R[3 + k], C.R[6 + k], Jc[0][j], Jc[1][j], Jc[2][j]);
                        Jw[k][j] = take ? (S.v[k] != 0.0f ? row : 0.0f) : Jw[k][j];
                    }
                    const float r3 = P.rot_weight * dot3(S.n[0], S.n[1], S.n[2], Jc[3][j], Jc[4][j], Jc[5][j]);
                    const float r4 = P.rot_weight * dot3(b0, b1, b2, Jc[3][j], Jc[4][j], Jc[5][j]);
                    Jw[3][j] = take ? (S.tilted ? r3 : 0.0f) : Jw[3][j];
                    Jw[4][j] = take ? (S.tilted ? r4 : 0.0f) : Jw[4][j];
                }
            }
#pragma unroll
            for (int r = 0; r < 6; ++r) e[r] = take ? ec[r] : e[r];
            E = take ? Ec : E;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc.v[k] = take ? S.v[k] : acc.v[k];
            acc.sn = take ? S.sn : acc.sn, acc.cs = take ? S.cs : acc.cs, acc.tilted = take ? S.tilted : acc.tilted;
            converged = converged || (take && S.band && !stuck);
            given = given || stuck;
            done = done || (take && S.band) || stuck;
            if (it == P.max_iterations || !wave_any(!done)) break;

            // ---- the step from the accepted state: A = Jm Jm^T + lambda I, A y = e, delta = Jm^T y
            float Jm[6][R::kDim], A[6][6], y[6], delta[R::kDim], big = 0.0f;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
                if (ee_joint(j))
                {
                    float g = Jw[0][j] * e[0];
#pragma unroll
                    for (int r = 1; r < 6; ++r) g += Jw[r][j] * e[r];
                    const bool hold = (q[j] <= P.lower[j] && g < 0.0f) || (q[j] >= P.upper[j] && g > 0.0f);
#pragma unroll
                    for (int r = 0; r < 6; ++r) Jm[r][j] = hold ? 0.0f : Jw[r][j];
                }
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b)
                {
                    float s = a == b ? lam : 0.0f;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j)
                        if (ee_joint(j)) s += Jm[a][j] * Jm[b][j];
                    A[a][b] = s;
                }
            chol6_solve(A, e, y);
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
            {
                delta[j] = 0.0f;
                if (ee_joint(j))
                {
                    float s = Jm[0][j] * y[0];
#pragma unroll
                    for (int r = 1; r < 6; ++r) s += Jm[r][j] * y[r];
                    delta[j] = s;
                    big = fmaxf(big, fabsf(s));
                }
            }
            const float scale = P.max_step / fmaxf(big, P.max_step);
#pragma unroll
            for (int j = 0; j < R::kDim; ++j)
                cand[j] = ee_joint(j) ? fminf(fmaxf(q[j] + delta[j] * scale, P.lower[j]), P.upper[j]) : q[j];
        }
        const float poison = finite ? 0.0f : __builtin_nanf("");
        constraint_report(acc, C, res_p, res_w);
        res_p += poison, res_w += poison;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) q_out[j] = given ? in[j] : q[j];
        status = (converged ? 0x80000000u : 0u) | (finite ? 0u : 0x40000000u) | evals;
    }

    // the band test of one configuration by the primal frame alone; finite: no joint is NaN or infinite
    __device__ __forceinline__ bool constraint_band(const float (&cfg)[R::kDim], const ConstraintDev &C, ConstraintState &S)
    {
        float f[12];
        bool finite = true;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) finite = finite && __builtin_isfinite(cfg[j]);
        R::ee_frame(cfg, f);
        constraint_residual(f, C, S);
        return finite && S.band;
    }

    // The band test of the edge a -> b, asked by a whole wave (vmv_constraint.h): sample i = 1 + lane + 64 r of the n_c, the
    // AND over the wave by a ballot.  The result does not depend on the order, so the wave stops at the first round with
    // a failing sample.  `live` false (wave-uniform): no edge, answers false.
    __device__ __forceinline__ bool constraint_band_edge(const ConstraintParams &P, const ConstraintDev &C, const float (&qa)[R::kDim],
                                                         const float (&qb)[R::kDim], const bool live)
    {
        float dq[R::kDim], sq = 0.0f;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            dq[j] = qb[j] - qa[j];
            sq = j == 0 ? dq[j] * dq[j] : sq + dq[j] * dq[j];
        }
        const float count = fmaxf(1.0f, ceilf(sqrtf(sq) / P.check_step));
        const bool fits = live && count <= (float) kConstraintMaxSamples;  // (a NaN length: one sample, itself NaN, out of band)
        const uint32_t n_c = fits ? (uint32_t) count : 0u;
        const uint32_t lane = threadIdx.x % (uint32_t) kWave;
        bool ok = fits;
        for (uint32_t base = 0; base < n_c && ok; base += (uint32_t) kWave)  // wave-uniform: n_c and ok are
        {
            const uint32_t i = base + lane + 1u;
            const float t = (float) (i <= n_c ? i : n_c) / (float) n_c;  // (a lane past the end repeats the last sample)
            float cfg[R::kDim];
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) cfg[j] = qa[j] + dq[j] * t;
            ConstraintState S;
            const bool in = constraint_band(cfg, C, S);
            ok = __ballot(!in) == 0ull;
        }
        return ok;
    }

    // vmv_constraint_project_batch: one lane per configuration, workgroups of one wave, no LDS, no atomics
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void constraint_project_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                          const float *__restrict__ q_in, const uint32_t n,
                                                                          float *__restrict__ q_out, float *__restrict__ res_out,
                                                                          uint32_t *__restrict__ status_out)
    {
        const uint32_t i = blockIdx.x * kIkBlock + threadIdx.x;
        const bool in_range = i < n;
        const uint32_t row = in_range ? i : 0u;  // (a lane past the end works on row 0 and writes nothing)
        const ConstraintDev C = cons[P.shared != 0u ? 0u : row];
        float in[R::kDim], q[R::kDim], res_p, res_w;
        uint32_t status;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) in[j] = q_in[(size_t) row * R::kDim + j];
        constraint_project_lane(P, C, in, in_range, q, res_p, res_w, status);
        if (!in_range) return;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) q_out[(size_t) i * R::kDim + j] = q[j];
        if (res_out != nullptr) res_out[2 * (size_t) i] = res_p, res_out[2 * (size_t) i + 1] = res_w;
        status_out[i] = status;
    }

    // vmv_constraint_check_batch: one lane per configuration, one ballot word per wave (a plain store by lane 0)
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void constraint_check_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                        const float *__restrict__ q, const uint32_t n,
                                                                        uint64_t *__restrict__ bits, float *__restrict__ res_out)
    {
        const uint32_t i = blockIdx.x * kIkBlock + threadIdx.x;
        const bool in_range = i < n;
        const uint32_t row = in_range ? i : 0u;
        const ConstraintDev C = cons[P.shared != 0u ? 0u : row];
        float cfg[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) cfg[j] = q[(size_t) row * R::kDim + j];
        ConstraintState S;
        const bool in = constraint_band(cfg, C, S);
        const uint64_t word = __ballot(in_range && in);
        if (threadIdx.x == 0u) bits[blockIdx.x] = word;
        if (in_range && res_out != nullptr)
        {
            bool finite = true;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) finite = finite && __builtin_isfinite(cfg[j]);
            const float poison = finite ? 0.0f : __builtin_nanf("");
            float res_p, res_w;
            constraint_report(S, C, res_p, res_w);
            res_out[2 * (size_t) i] = res_p + poison, res_out[2 * (size_t) i + 1] = res_w + poison;
        }
    }

    // vmv_constraint_check_motion_batch: one wave per edge, one byte per edge (a plain store by lane 0)
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void constraint_edge_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                       const float *__restrict__ a, const float *__restrict__ b,
                                                                       const uint32_t n, uint8_t *__restrict__ ok_out)
    {
        const uint32_t e = blockIdx.x;  // the grid has n workgroups
        const ConstraintDev C = cons[P.shared != 0u ? 0u : e];
        float qa[R::kDim], qb[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) qa[j] = a[(size_t) e * R::kDim + j], qb[j] = b[(size_t) e * R::kDim + j];
        const bool ok = constraint_band_edge(P, C, qa, qb, e < n);
        if (threadIdx.x == 0u) ok_out[e] = ok ? 1u : 0u;
    }

    // The constraint's part of a planner round (vmv_rrtc_multi_constrained), one wave per active slot a, after the step
    // kernel on the same stream.  Where the step kernel named a pending node (the far end of an extension or of a march
    // step, just written to q_goal[a] and to that pool element), q_goal[a] is projected - every lane of the wave runs the
    // same projection, so the result is the lane's of constraint_project_kernel bit for bit - and, converged and no
    // farther than `stretch` (max_stretch * range) from q_start[a], replaces both; else both stay and the answer is 0.
    // Then the band test of the edge q_start[a] -> q_goal[a] as constraint_edge_kernel makes it.  c_ok[a]: the answer the
    // step kernel ANDs into the validity bit; refused[problem] counts the questions answered 0 here.  Plain stores by lane 0;
    // problem = active[a] picks the record.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void constraint_round_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                        const uint32_t *__restrict__ active, const float *__restrict__ q_start,
                                                                        float *q_goal, const uint64_t *__restrict__ pending, float *pool,
                                                                        const float stretch, uint8_t *__restrict__ c_ok,
                                                                        uint32_t *__restrict__ refused)
    {
        const uint32_t a = blockIdx.x;  // the grid has one workgroup per active slot
        const ConstraintDev C = cons[P.shared != 0u ? 0u : active[a]];
        const uint64_t pend = pending[a];
        const bool has = pend != ~0ull;
        float qs[R::kDim], qg[R::kDim], q[R::kDim], res_p, res_w;
        uint32_t status;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) qs[j] = q_start[(size_t) a * R::kDim + j], qg[j] = q_goal[(size_t) a * R::kDim + j];
        constraint_project_lane(P, C, qg, has, q, res_p, res_w, status);  // (no pending node: the lanes ride along)
        float sq = 0.0f;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            const float d = q[j] - qs[j];
            sq = j == 0 ? d * d : sq + d * d;
        }
        const bool good = has && (status >> 31) != 0u && sqrtf(sq) <= stretch;
        if (good && threadIdx.x == 0u)
        {
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) q_goal[(size_t) a * R::kDim + j] = q[j], pool[pend * R::kDim + j] = q[j];
        }
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) qg[j] = good ? q[j] : qg[j];
        const bool edge = constraint_band_edge(P, C, qs, qg, !has || good);
        if (threadIdx.x == 0u)
        {
            c_ok[a] = edge ? 1u : 0u;
            if (!edge) refused[active[a]] += 1u;  // (this wave owns its problem's counter; the null question is in band)
        }
    }

    // The constraint's part of a simplifier round (vmv_simplify_multi_constrained, DESIGN.md 5p), one wave per slot of
    // every active path - slot = a * w + s - after the step kernel on the same stream.  pending[slot] says what the step
    // kernel wrote there: 0 a null question (answered 1, nothing is read), 1 an edge to band-check as constraint_edge_kernel
    // does, 2 / 3 the first / second motion of a B-spline candidate, whose midpoint sits in q_goal[slot] / q_start[slot].
    // That midpoint is projected - every lane of the wave runs the same projection, so the result is the lane's of
    // constraint_project_kernel bit for bit, and the two slots of a candidate compute the same bits independently - and,
    // converged, replaces the midpoint in the slot's own question array (code 2 also stores it in proj[path][s / 2], which
    // the next step kernel reads); then the edge is band-checked.  Not converged: nothing is stored, the answer is 0.
    // The branches are taken by the whole wave (the code is the workgroup's).  Plain stores by lane 0; path = active[a]
    // picks the record.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void simplify_band_round_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                           const uint32_t *__restrict__ active, float *q_start, float *q_goal,
                                                                           const uint8_t *__restrict__ pending, float *proj,
                                                                           const uint32_t proj_stride, const uint32_t w,
                                                                           uint8_t *__restrict__ c_ok)
    {
        const uint32_t slot = blockIdx.x;  // the grid has one workgroup per slot
        const uint32_t code = pending[slot];
        if (code == 0u)
        {
            if (threadIdx.x == 0u) c_ok[slot] = 1u;
            return;
        }
        const uint32_t a = slot / w, s = slot - a * w, path = active[a];
        const ConstraintDev C = cons[P.shared != 0u ? 0u : path];
        float qs[R::kDim], qg[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) qs[j] = q_start[(size_t) slot * R::kDim + j], qg[j] = q_goal[(size_t) slot * R::kDim + j];
        bool live = true;
        if (code >= 2u)
        {
            const bool goal = code == 2u;
            float mid[R::kDim], q[R::kDim], res_p, res_w;
            uint32_t status;
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) mid[j] = goal ? qg[j] : qs[j];
            constraint_project_lane(P, C, mid, true, q, res_p, res_w, status);
            live = (status >> 31) != 0u;
            if (live && threadIdx.x == 0u)
            {
                float *own = (goal ? q_goal : q_start) + (size_t) slot * R::kDim;
#pragma unroll
                for (int j = 0; j < R::kDim; ++j) own[j] = q[j];
                if (goal)
                {
                    float *keep = proj + (size_t) path * proj_stride + (size_t) (s >> 1) * R::kDim;
#pragma unroll
                    for (int j = 0; j < R::kDim; ++j) keep[j] = q[j];
                }
            }
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) qs[j] = goal ? qs[j] : q[j], qg[j] = goal ? q[j] : qg[j];
        }
        const bool edge = constraint_band_edge(P, C, qs, qg, live);
        if (threadIdx.x == 0u) c_ok[slot] = edge ? 1u : 0u;
    }

    // The constraint's part of an optimiser iteration (vmv_optimize_multi_constrained, DESIGN.md 5q), one lane per packed
    // waypoint of the active paths, after the step kernel on the same stream.  Row r is waypoint i of active path a =
    // row_path[r] (OptBand, vmv_common.h); path = active[a] picks the record.  The lane projects its waypoint of the new
    // iterate x[cur ^ 1] as constraint_project_kernel's lane does, bit for bit, and writes the projection - or, where it
    // did not converge, the waypoint of iterate x[cur], counted in held[path] - to x[cur ^ 1], to the packed copy q and,
    // with `edges`, to its two places among the edges.  End waypoints, rows past the last one and the rows of a path
    // that ends at this validated iterate (may_end and its step in below min_change: the accept kernel's rule) ride along
    // and write nothing.  initial: the same on the input in x[cur], in place; a lane that does not converge flags its path
    // in unconverged[path] and leaves the waypoint as it is.  Plain vector stores by the owning lane; held by a vector
    // atomicAdd (an integer sum, whatever the order); no LDS.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void opt_band_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons, const OptBand B,
                                                                const uint32_t rows, const uint32_t cur, const uint32_t initial,
                                                                const uint32_t edges, const uint32_t may_end, const float min_change)
    {
        const uint32_t r = blockIdx.x * kIkBlock + threadIdx.x;
        const bool has = r < rows;
        const uint32_t row = has ? r : 0u;  // (a lane past the end works on row 0 and writes nothing)
        const uint32_t a = B.row_path[row], path = B.active[a];
        const uint64_t lo = B.offsets[path], ao = B.act_off[a];
        const uint32_t N = (uint32_t) (B.offsets[path + 1] - lo), i = (uint32_t) (row - ao);
        const bool ends = may_end != 0u && B.change_in[(size_t) path * B.state_stride] < min_change;
        const bool in_range = has && i >= 1u && i + 1u < N && !ends;
        const ConstraintDev C = cons[P.shared != 0u ? 0u : path];
        float *xn = B.x + ((size_t) (initial != 0u ? cur : cur ^ 1u) * B.total + lo + i) * R::kDim;
        const float *xk = B.x + ((size_t) cur * B.total + lo + i) * R::kDim;
        float in[R::kDim], q[R::kDim], res_p, res_w;
        uint32_t status;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j) in[j] = xn[j];
        constraint_project_lane(P, C, in, in_range, q, res_p, res_w, status);
        if (!in_range) return;
        const bool converged = (status >> 31) != 0u;
        if (!converged)
        {
            if (initial != 0u)
                B.unconverged[path] = 1u;
            else
                atomicAdd(&B.held[path], 1u);
        }
        float *qp = B.q + (size_t) row * R::kDim;
        const uint64_t e = B.edge_off[a] + i;  // the edge that starts at this waypoint; the one that ends here is e - 1
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            const float v = converged ? q[j] : xk[j];
            xn[j] = v;
            qp[j] = v;
            if (edges != 0u) B.e_start[e * R::kDim + j] = v, B.e_goal[(e - 1u) * R::kDim + j] = v;
        }
    }

    // The band test of the edge a -> b asked by ONE lane: constraint_band_edge's count, its t = i / n_c and its
    // constraint_band per sample, i = 1 .. n_c in turn, ANDed.  The AND does not depend on the order and the wave form's
    // repeated last sample adds nothing, so the answer is the wave form's bit for bit.  `live` false: no edge, nothing
    // is evaluated, answers false.
    __device__ __forceinline__ bool constraint_band_edge_lane(const ConstraintParams &P, const ConstraintDev &C, const float (&qa)[R::kDim],
                                                              const float (&qb)[R::kDim], const bool live)
    {
        float dq[R::kDim], sq = 0.0f;
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            dq[j] = qb[j] - qa[j];
            sq = j == 0 ? dq[j] * dq[j] : sq + dq[j] * dq[j];
        }
        const float count = fmaxf(1.0f, ceilf(sqrtf(sq) / P.check_step));
        const bool fits = live && count <= (float) kConstraintMaxSamples;
        const uint32_t n_c = fits ? (uint32_t) count : 0u;
        bool ok = fits;
        for (uint32_t i = 1u; i <= n_c && ok; ++i)
        {
            const float t = (float) i / (float) n_c;
            float cfg[R::kDim];
#pragma unroll
            for (int j = 0; j < R::kDim; ++j) cfg[j] = qa[j] + dq[j] * t;
            ConstraintState S;
            ok = constraint_band(cfg, C, S);
        }
        return ok;
    }

    // The band test of a retiming round (vmv_retime_multi_constrained, DESIGN.md 5r), one LANE per packed sample row g:
    // the pair of rows g -> g + 1 of pos, read in place.  A pair of samples dt apart is a few centimetres of joint space,
    // n_c is 1 or 2, and a wave per pair would idle 63 lanes.  Row g belongs to listed path a, the last whose first
    // sample is not behind g (retime_sample_kernel's search); the path's last row has no pair: its lane answers 1 and
    // reads nothing, so no lane reads past row rows - 1.  The record is cons[0] (P.shared) or cons[rec_of[a]].  One byte
    // per row, a plain store by the owning lane; no LDS, no atomics.
    template <int = 0>
    __global__ __launch_bounds__(kIkBlock) void retime_band_kernel(const ConstraintParams P, const ConstraintDev *__restrict__ cons,
                                                                   const uint32_t *__restrict__ rec_of, const uint32_t *__restrict__ sample_lo,
                                                                   const uint32_t n_paths, const float *__restrict__ pos, const uint32_t rows,
                                                                   uint8_t *__restrict__ ok_out)
    {
        const uint32_t g = blockIdx.x * kIkBlock + threadIdx.x;
        if (g >= rows) return;
        uint32_t lo = 0u, hi = n_paths - 1u;
        while (lo < hi)
        {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (sample_lo[mid] <= g) lo = mid;
            else hi = mid - 1u;
        }
        const bool pair = g + 1u < sample_lo[lo + 1u];
        const ConstraintDev C = cons[P.shared != 0u ? 0u : rec_of[lo]];
        float qa[R::kDim], qb[R::kDim];
#pragma unroll
        for (int j = 0; j < R::kDim; ++j)
        {
            qa[j] = pair ? pos[(size_t) g * R::kDim + j] : 0.0f;
            qb[j] = pair ? pos[((size_t) g + 1u) * R::kDim + j] : 0.0f;
        }
        const bool ok = constraint_band_edge_lane(P, C, qa, qb, pair);
        ok_out[g] = (!pair || ok) ? 1u : 0u;
    }

    // ---------------------------------------------------------------------------------------------------------
    // launchers
    // ---------------------------------------------------------------------------------------------------------
#include "vmv_robot_launch.inc"

}  // namespace VMV_ROBOT_NS

#if !defined(__HIP_DEVICE_COMPILE__)
    extern const RobotLaunchers VMV_ROBOT_LAUNCH = VMV_ROBOT_NS::make_launchers();
#endif
}  // namespace vmv
