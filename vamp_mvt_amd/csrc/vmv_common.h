// vmv_common.h — declarations shared by the API translation unit and the per-robot kernel translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "vmv_constraint.h"
#include "vmv_device.h"

namespace vmv
{
    constexpr int kBlock = 256;  // 4 waves per workgroup; each wave owns one LDS slab
    constexpr int kWavesPerBlock = kBlock / kWave;
    constexpr uint32_t kMaxLdsBytes = 160u * 1024u;   // gfx950 LDS per CU / max per workgroup
    constexpr uint32_t kMaxPrimFloats = 12u * 1024u;  // 48 KiB of primitive records

    // what a launcher needs to know about a finalized environment
    struct EnvLaunch
    {
        const EnvDev *d_env;  // device copy
        EnvDev host;          // host copy (sizes)
    };

    // ---- vmv_validate_batch_multi: configurations [lo, hi) of one batch against one environment each ----
    struct MultiSeg  // one segment (device table written by the launcher)
    {
        const EnvDev *env;
        uint32_t lo, hi;        // the segment's configurations [lo, hi) of the whole batch
        uint32_t tests_in_lds;  // the environment's LDS plan, as its single-environment launch makes it
        uint32_t slab;          // LDS float offset of wave 0's slab
    };
    struct MultiTile  // one workgroup's kWavesPerBlock validity words [word, word + 4) of segment `seg`
    {
        uint32_t seg, word;
    };
    constexpr size_t kMultiMaxConfigs = size_t{1} << 31;  // the kernels count configurations and segments in 32 bits

    // Tables of one vmv_validate_batch_multi call: pinned host staging and device scratch per (device, stream), copied with
    // hipMemcpyAsync on the stream.  Calls on one stream run in order, so they share the device buffer; a host buffer whose
    // previous copy has not yet run is not rewritten (another one is taken), so the host never waits.  The lease holds the
    // pool's lock until the call is enqueued.
    class MultiTableLease
    {
        std::unique_lock<std::mutex> lock_;
        void *entry_ = nullptr;  // the (device, stream) entry
        size_t slot_ = 0;        // its host buffer in use

    public:
        void *host = nullptr, *dev = nullptr;
        MultiTableLease();
        int acquire(hipStream_t stream, size_t bytes);
        int upload(hipStream_t stream, size_t bytes);  // host -> dev on `stream`
    };
    void release_multi_tables();

    // The table of a multi-environment launch, [segments | tiles ..] in one lease: the tiles start on a 16-byte boundary
    // behind the segments.  The same offsets hold in the lease's host and device buffer.
    struct MultiTableLayout
    {
        size_t tiles_at, bytes;  // byte offset of the first tile; size of [segments | tiles]
        MultiTableLayout(size_t n_segs, size_t n_tiles)
            : tiles_at((n_segs * sizeof(MultiSeg) + 15u) & ~size_t{15}), bytes(tiles_at + n_tiles * sizeof(MultiTile))
        {
        }
        static MultiSeg *segs(void *base) { return static_cast<MultiSeg *>(base); }
        MultiTile *tiles(void *base) const { return reinterpret_cast<MultiTile *>(static_cast<char *>(base) + tiles_at); }
    };

    // Which kernel variant an environment runs, as the index of every per-robot kernel table (vmv_robot_launch.inc):
    // 0 kEnvZOnly, 1 kEnvPrims, 2 kEnvFull, 3 kEnvClouds.  The primitive-only variants (merged gates, no cloud / heightfield
    // code) serve environments of WELL-FORMED primitives only, kEnvZOnly those without capsules and cuboids; kEnvClouds
    // (no list code, no gate calls in the paired walk) serves point clouds and nothing else; everything else takes the
    // variant that keeps the reference's groups (EnvDev::ill_formed).  (vmv_device.h's "clouds_only" is class 3 here.)
    constexpr int kEnvClasses = 4;
    inline int env_class(const EnvLaunch &e)
    {
        const EnvDev &D = e.host;
        if (D.n_capt + D.n_mvt + D.n_heightfield == 0 && D.ill_formed == 0) return D.n_capsule + D.n_cuboid == 0 ? 0 : 1;
        return D.n_capt != 0 && D.n_floats + D.n_mvt + D.n_heightfield == 0 ? 3 : 2;
    }

    // vmv_ik_batch: the kernel's parameter block - vmv_ik_settings as checked by the API (rot_weight is 0 for a
    // position-only call, so the rotation rows vanish), where the seeds lie, and the robot's bounds [lower, lower + span]
    struct IkParams
    {
        uint32_t n_seeds, max_iterations;
        float pos_tol, rot_tol, rot_weight, damping, max_step;
        uint32_t position_only;
        uint32_t seeds_shared;  // 1: d_seeds is [n_seeds][dim], the same seeds for every target (the Halton seeds)
        float lower[16], upper[16];
    };

    // vmv_cartesian_multi: the tracking kernel's parameter block (vmv_cartesian_settings as checked, rot_weight 0 for a
    // position-only call), one record per problem and one result per problem.  A problem that does not take part
    // (non-finite input, a line that is too long) has m == 0 and a zeroed record: its lane does nothing.
    struct CartParams
    {
        uint32_t max_iterations;
        uint32_t max_k;  // the largest m of the call: the bound of the kernel's outer loop
        float pos_tol, rot_tol, rot_weight, damping, max_step, max_joint_step;
        uint32_t position_only;
        float lower[16], upper[16];
    };
    struct CartLine
    {
        float p0[3], dp[3];  // pose k: p0 + (k / m) dp
        float R0[9];         // row-major; pose k: R0 Rot(axis, (k / m) theta)
        float axis[3], theta;
        uint32_t m;       // segments; 0: the lane does nothing
        uint64_t offset;  // first row of the problem's m + 1 rows in the packed output
    };
    static_assert(sizeof(CartLine) == 88, "19 floats, m, the offset");
    struct CartResult
    {
        uint32_t tracked;  // waypoints 1 .. tracked were accepted and written
        uint32_t status;   // VMV_CART_COMPLETE, VMV_CART_IK_FAILED or VMV_CART_JOINT_JUMP
        uint32_t evaluations, pad;
    };

    // vmv_optimize_multi_constrained (vmv_optimize_multi.hip): where opt_band_kernel finds the waypoint of a packed row.
    // Row r of the active paths' packed waypoints belongs to active path a = row_path[r], path p = active[a]; it is
    // waypoint i = r - act_off[a] of the path's offsets[p + 1] - offsets[p].  The host rebuilds row_path with the active list.
    struct OptBand
    {
        const uint32_t *row_path;   // [rows]
        const uint32_t *active;     // [n_active]
        const uint64_t *act_off;    // [n_active] first row of the path in q
        const uint64_t *edge_off;   // [n_active] first edge of the path in e_start / e_goal
        const uint64_t *offsets;    // [n_paths + 1] in waypoints
        float *x;                   // [2][total][dim] the iterates, double-buffered
        float *q;                   // [rows][dim] the packed copy the clearance call reads
        float *e_start, *e_goal;    // [edges][dim]
        const float *change_in;     // path p's step into the current iterate at change_in[p * state_stride]
        uint32_t state_stride;      // in floats
        uint32_t *held;             // [n_paths] += 1 per projection of an iteration that did not converge
        uint8_t *unconverged;       // [n_paths] = 1 where a projection of the input did not converge (initial)
        size_t total;               // waypoints of the call
    };

    // status codes are the VMV_* values of include/vamp_mvt_amd.h
    struct RobotLaunchers
    {
        // stage bit 1 = environment kernel (writes the words), bit 2 = self-collision kernel, bit 4 = attachment kernel
        // (both AND into them; the attachment kernel only runs for environments with an attachment)
        int (*validate)(const EnvLaunch &, const float *d_q, size_t n, uint64_t *d_bits, hipStream_t, int stages);
        // vmv_validate_batch_multi: configurations [offsets[k], offsets[k + 1]) against *envs[k], n = offsets[n_envs] <
        // kMultiMaxConfigs; every environment finalized on the current device with this robot's part built
        int (*validate_multi)(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                              uint64_t *d_bits, hipStream_t);
        int (*validate_motion)(const EnvLaunch &, const float *d_a, const float *d_b, size_t n, uint64_t *d_bits,
                               hipStream_t);
        // vmv_validate_motion_batch_multi: edges [offsets[k], offsets[k + 1]) against *envs[k], as validate_multi
        int (*validate_motion_multi)(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_a,
                                     const float *d_b, uint64_t *d_bits, hipStream_t);
        int (*fk)(const float *d_q, size_t n, float *d_out, hipStream_t);
        // once per (environment, robot), after the robot's EnvDev is on the device: evaluates the robot's static links
        // against the environment and stores the answer in d_env->static_hit (synchronous)
        int (*prepare)(const EnvLaunch &, EnvDev *d_env);
        // the same for many environments in one launch: d_envs[k] is the device image of *envs[k] (already complete but
        // for static_hit), status[k] = VMV_OK or why environment k could not be launched (it is then left out);
        // synchronous, returns non-OK only for a failure of the launch as a whole
        int (*prepare_multi)(const EnvLaunch *const *envs, EnvDev *const *d_envs, size_t n_envs, int *status);
        int (*eefk)(const float *d_q, size_t n, float *d_out16, hipStream_t);  // 4 x 4 row-major frames
        // contact report (Robot::fkcc_debug) from the fine spheres of launch fk
        int (*contacts)(const EnvLaunch &, const float *d_spheres, size_t n, uint32_t *d_env_words, uint32_t *d_pair_words,
                        hipStream_t);
        int n_self_pairs;
        // vmv_clearance_batch: d_out [n][2] = (environment, self) clearance, d_witness [n][4] or nullptr; env == nullptr:
        // the self clearance alone.  The environment holds no point cloud and no attachment (the API refuses those).
        int (*clearance)(const EnvLaunch *env, const float *d_q, size_t n, float *d_out, uint32_t *d_witness, hipStream_t);
        // vmv_clearance_batch_multi: configurations [offsets[k], offsets[k + 1]) against *envs[k], as validate_multi
        int (*clearance_multi)(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                               float *d_out, uint32_t *d_witness, hipStream_t);
        // vmv_clearance_grad_batch(_multi): the clearance launch as it is, then d_grad [n][2][dim] from the witness it wrote;
        // d_witness is never nullptr (the API lends per-stream scratch where the caller has none)
        int (*clearance_grad)(const EnvLaunch *env, const float *d_q, size_t n, float *d_out, float *d_grad, uint32_t *d_witness,
                              hipStream_t);
        int (*clearance_grad_multi)(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                                    float *d_out, float *d_grad, uint32_t *d_witness, hipStream_t);
        // vmv_eefk_jacobian_batch: d_frames [n][16] as eefk's or nullptr, d_jac [n][6][dim]
        int (*eefk_jacobian)(const float *d_q, size_t n, float *d_frames, float *d_jac, hipStream_t);
        // vmv_ik_batch: n = n_targets * n_seeds lanes (below 2^31), lane i = target i / n_seeds from seed i (or seed
        // i % n_seeds with seeds_shared); d_q [n][dim], d_err [n][2] or nullptr, d_status [n]
        int (*ik)(const IkParams &, const float *d_targets, const float *d_seeds, size_t n, float *d_q, float *d_err,
                  uint32_t *d_status, hipStream_t);
        // vmv_cartesian_multi's tracking: one lane per problem (n below 2^31), d_starts [n][dim], d_points the packed
        // rows (row 0 of a problem is the host's), d_results [n]
        int (*cartesian)(const CartParams &, const CartLine *d_lines, const float *d_starts, size_t n, float *d_points,
                         CartResult *d_results, hipStream_t);
        // vmv_constraint_*_batch (vmv_constraint.h): n below 2^31 lanes / edges; d_cons one record (P.shared) or [n];
        // d_res [n][2] may be nullptr; d_bits ceil(n / 64) words; d_ok one byte per edge
        int (*constraint_project)(const ConstraintParams &, const ConstraintDev *d_cons, const float *d_q, size_t n, float *d_q_out,
                                  float *d_res, uint32_t *d_status, hipStream_t);
        int (*constraint_check)(const ConstraintParams &, const ConstraintDev *d_cons, const float *d_q, size_t n, uint64_t *d_bits,
                                float *d_res, hipStream_t);
        int (*constraint_edges)(const ConstraintParams &, const ConstraintDev *d_cons, const float *d_a, const float *d_b, size_t n,
                                uint8_t *d_ok, hipStream_t);
        // vmv_rrtc_multi_constrained's part of a round, after the step kernel on the same stream: per active slot the
        // pending node (d_pending[a] = its pool element, ~0 = none) projected and written back, then the band test of
        // the edge into d_c_ok[a]; d_cons one record (P.shared) or one per PROBLEM (indexed through d_active)
        int (*constraint_round)(const ConstraintParams &, const ConstraintDev *d_cons, const uint32_t *d_active, const float *d_q_start,
                                float *d_q_goal, const uint64_t *d_pending, float *d_pool, float stretch, uint8_t *d_c_ok,
                                uint32_t *d_refused /* [n_problems], += 1 per question answered 0 */, uint32_t na, hipStream_t);
        // vmv_simplify_multi_constrained's part of a round, after the step kernel on the same stream: one wave per slot
        // a * w + s of the na active paths.  d_pending[slot]: 0 null (answered 1), 1 band-check the edge, 2 / 3 project the
        // B-spline midpoint in d_q_goal / d_q_start[slot] first, write it back there (2: into d_proj[path][s / 2] too, paths
        // proj_stride floats apart) and answer 0 where it does not converge; the answers go to d_c_ok[slot].  d_cons one
        // record (P.shared) or one per PATH (indexed through d_active)
        int (*simplify_band_round)(const ConstraintParams &, const ConstraintDev *d_cons, const uint32_t *d_active, float *d_q_start,
                                   float *d_q_goal, const uint8_t *d_pending, float *d_proj, uint32_t proj_stride, uint8_t *d_c_ok,
                                   uint32_t na, uint32_t w, hipStream_t);
        // vmv_optimize_multi_constrained's part of an iteration, after the step kernel on the same stream: one lane per
        // packed waypoint of the active paths (rows below 2^31).  d_cons one record (P.shared) or one per PATH
        int (*opt_band)(const ConstraintParams &, const ConstraintDev *d_cons, const OptBand &, uint32_t rows, uint32_t cur,
                        uint32_t initial, uint32_t edges, uint32_t may_end, float min_change, hipStream_t);
        // vmv_retime_multi_constrained's band test of a round: one LANE per packed sample row g < rows (below 2^31), the
        // pair g -> g + 1 of d_pos.  Row g belongs to listed path a, the last with sample_lo[a] <= g (sample_lo
        // [n_paths + 1], as retime_sample_kernel reads it); a path's last row has no pair and answers 1 unread.  d_cons one
        // record (P.shared) or record rec_of[a].  d_ok [rows]: constraint_edge_kernel's answer for the pair, bit for bit.
        int (*retime_band)(const ConstraintParams &, const ConstraintDev *d_cons, const uint32_t *d_rec_of, const uint32_t *d_sample_lo,
                           uint32_t n_paths, const float *d_pos, uint32_t rows, uint8_t *d_ok, hipStream_t);
        // vmv_self_screen_flags: bit i of d_words [ceil(n / 64)] = the self-collision screen flags row i; mode 0 the exact
        // screen, 1 the prescreen (robots without either: the exact gates both times); n below 2^31
        int (*self_screen_flags)(const float *d_q, size_t n, int mode, uint64_t *d_words, hipStream_t);
    };

    extern const RobotLaunchers kPandaLaunchers, kUr5Launchers, kFetchLaunchers, kBaxterLaunchers;
    inline const RobotLaunchers &robot_launchers(int robot)  // robot: a VMV_ROBOT_* value the caller has checked
    {
        const RobotLaunchers *const all[] = {&kPandaLaunchers, &kUr5Launchers, &kFetchLaunchers, &kBaxterLaunchers};
        return *all[robot];
    }

    int hip_status(hipError_t e, const char *what);  // records vmv_last_error(), maps to VMV_ERR_*
    int refuse_argument(const char *message);        // records vmv_last_error(), returns VMV_ERR_INVALID_ARGUMENT

    // Element j of Halton sample number k (1-based) of the reference's sequence (random/halton.hh:75-108): the
    // incremental float arithmetic there keeps exact integers n, d = b^digits, so the value is n / d with n the
    // digit-reversed index; then Robot::scale_configuration (q * s_m + s_a, two roundings).  The
    // reference's sequence up to k = 1,000,000 (it re-seeds after that).  Shared by halton_kernel and the lockstep planner.
    __device__ __forceinline__ float halton_element(uint64_t k, int j, float lower, float span)
    {
        static constexpr uint32_t primes[16] = {3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59};
        const uint32_t b = primes[j];
        uint32_t n = 0, d = 1;
        while (k > 0)
        {
            n = n * b + (uint32_t) (k % b);
            d *= b;
            k /= b;
        }
        const float u = (float) n / (float) d;
        return u * span + lower;
    }

    // ---- vmv_env_prepare_multi: grids and reach certificates of many environments (vmv_env_prepare.hip) ----
    constexpr uint32_t kPrepMaxPrims = 128;  // primitives of an environment that has grid_prims (4 candidate words)
    struct PrepPrim  // vmv::GridPrim with its parameters in place
    {
        int type;
        uint32_t word, bit;
        float p[15];
    };
    struct PrepGridJob  // one grid (environment, class) to fill
    {
        uint32_t prim_lo, n_prims;  // its environment's records in the PrepPrim table
        uint32_t dims[3], words;
        float origin[3];
        double hf, half_diag, R;    // vmv::GridGeometry, the class's radius
        unsigned long long cell_lo;  // first word of the grid in the cell buffer
    };
    struct PrepReachLink  // vmv_link_reach of one robot, samples in one table
    {
        int group;
        uint32_t sample_lo, n;
        double need;  // radius + slack + 1 mm
    };
    struct PrepReachJob  // one environment whose certificates are to be evaluated
    {
        uint32_t prim_lo, n_prims;
        EnvDev *image;  // link_skip is stored here ...
        uint32_t out;   // ... and in skip_out[out]
    };
    // all on `stream`, no synchronisation; jobs with dims whose product is 0 are not allowed
    int launch_grid_fill(const PrepPrim *d_prims, const PrepGridJob *d_jobs, const PrepGridJob *jobs, size_t n_jobs,
                         uint32_t *d_cells, hipStream_t stream);
    int launch_reach(const PrepPrim *d_prims, const PrepReachJob *d_jobs, size_t n_jobs, const PrepReachLink *d_links,
                     uint32_t n_links, const float *d_samples, unsigned long long *d_skip_out, hipStream_t stream);

    // ---- (edge, rake) task scheduling of vmv_validate_motion_batch: the robot-independent half (vmv_edge_tasks.hip) ----
    constexpr uint32_t kEdgeScanBlock = 2048;        // edges per workgroup of the scan kernels
    constexpr uint32_t kEdgeSliceEdges = 1u << 20;   // a larger batch is validated slice by slice (32-bit task arithmetic)
    constexpr uint32_t kEdgeMaxPasses = 8;
    struct EdgeScratch
    {
        uint32_t *steps;       // [n] rakes of edge e (planning/validate.hh:41), written by pass 0
        uint32_t *excl;        // [n] exclusive scan of the current pass's task counts
        uint32_t *block_sums;  // [ceil(n / kEdgeScanBlock)]
        uint32_t *total;       // [kEdgeMaxPasses] tasks of each pass
    };
    class EdgeScratchLease
    {
        std::unique_lock<std::mutex> lock_;

    public:
        EdgeScratch s{};
        EdgeScratchLease();
        int acquire(hipStream_t stream, size_t n_edges);  // holds the pool until the lease goes out of scope
    };
    void release_edge_scratch();
    // task counts of the pass that covers rakes [lo, hi) of the edges still valid in d_bits -> s.excl, s.total[slot]
    int launch_edge_pass_scan(const EdgeScratch &s, const uint64_t *d_bits, uint32_t n, uint32_t lo, uint32_t hi, uint32_t slot,
                              hipStream_t stream);

    // ---- vmv_validate_motion_batch_multi: the later pass's tiles, built on the device from the scan ----
    // Segment k's later-pass tasks are [excl[lo_k], excl[hi_k]) (total for the last edge).  Per variant class c, the
    // non-empty segments of the class are entries[at[c] .. at[c] + m[c]) (indices into the MultiSeg table);
    // launch_edge_multi_tiles writes chunk[c] = tasks per tile (a multiple of 32, at least sum / grid[c]) and
    // starts[at[c] + c + j] = tiles of the class's entries before j (m[c] + 1 values), so that the class has at most
    // grid[c] + m[c] tiles and a tile never spans two segments.
    constexpr int kEdgeMultiClasses = kEnvClasses;
    struct EdgeMultiPlan
    {
        uint32_t at[kEdgeMultiClasses], m[kEdgeMultiClasses], grid[kEdgeMultiClasses];
    };
    int launch_edge_multi_tiles(const EdgeScratch &s, const MultiSeg *d_segs, const uint32_t *d_entries, const EdgeMultiPlan &plan,
                                uint32_t n, uint32_t *d_starts, uint32_t *d_chunk, hipStream_t stream);
}  // namespace vmv
