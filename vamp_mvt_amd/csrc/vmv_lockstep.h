// vmv_lockstep.h — the host side the lockstep calls share (vmv_rrtc_multi, vmv_rrtc_multi_goals, vmv_simplify_multi,
// vmv_aorrtc_multi, vmv_fcit_multi and the _constrained forms of the first four; DESIGN §5c "A round"), and the host steps
// every planner and path call has around its kernels: the device-free argument checks, the problem uploads and the packed
// paths of a result (vmv_prm_multi and vmv_roadmaps_* as well), the result object's life cycle (lockstep_call: those, and
// vmv_optimize_multi, vmv_cartesian_multi, vmv_retime_multi with their _constrained forms), the refusal of the
// environments' kinds (check_env_kinds: the last three) and a band's records on the device (upload_records: every
// _constrained call and vmv_retime_band_pairs_host; the band itself is vmv_constraint.h's ConstraintBand).
//
// Every item of a call (a planning problem, a path) is a state machine in device memory.  One round = the call's step
// kernel (one workgroup per unfinished item: consumes the answers to the item's previous questions, advances its state and
// writes its next questions into the round's start / goal arrays) + one vmv_validate_motion_batch_multi call over those
// edges.  The host does nothing per item inside a round and does not synchronise; every check_every rounds it reads the
// finished flags and compacts the active list.  lockstep_rounds() below is that loop, with every synchronisation point
// and every error exit of a call's rounds, LockstepBuffers the arrays it runs on; the kernels and the state stay with
// each caller.
#pragma once

#include "../../include/vamp_mvt_amd.h"

#include "vmv_common.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace vmv
{
    constexpr uint32_t kPlanMaxDim = 16;  // joints of a robot the planner calls accept
    constexpr uint32_t kNone = 0xffffffffu;
    constexpr uint64_t kMaxHaltonIndex = 1000000ull;

    struct DeviceBuffers  // freed on every way out
    {
        std::vector<void *> ptrs;
        void *pinned = nullptr;
        ~DeviceBuffers()
        {
            for (void *p : ptrs) (void) hipFree(p);
            if (pinned) (void) hipHostFree(pinned);
        }
        template <typename T>
        hipError_t alloc(T **out, size_t count)
        {
            void *p = nullptr;
            const hipError_t e = hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16));
            if (e == hipSuccess) ptrs.push_back(p);
            *out = static_cast<T *>(p);
            return e;
        }
    };
#define VMV_LOCKSTEP_HIP(call)                                \
    do                                                        \
    {                                                         \
        const hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_status(e_, #call);   \
    } while (0)

    // `count` constraint records on the device, in memory of `mem`; a set-up copy, synchronous (the host array may go)
    inline int upload_records(DeviceBuffers &mem, const ConstraintDev *records, size_t count, ConstraintDev **d_records)
    {
        VMV_LOCKSTEP_HIP(mem.alloc(d_records, count));
        if (count) VMV_LOCKSTEP_HIP(hipMemcpy(*d_records, records, count * sizeof(ConstraintDev), hipMemcpyHostToDevice));
        return VMV_OK;
    }

    struct LockstepArrays  // what the rounds of one call read and write (LockstepBuffers::arrays())
    {
        uint32_t *active;               // [initial active count] item of each workgroup, uploaded by the caller
        const float *q_start, *q_goal;  // [active][per_item][dim] the round's questions
        uint64_t *bits;                 // their answers, read by the next round's step kernel
        const uint8_t *done;            // [n_items] set by the step kernel
        uint8_t *h_done;                // [n_items] pinned
        size_t n_items;
    };

    namespace  // internal linkage: the library exports nothing of what follows
    {
    // The arrays every lockstep call needs, for n_items items of which at most n_active are active at once, each with
    // per_item questions of dim floats per round.  `done` and the answers start as zeros (in stream order).
    struct LockstepBuffers
    {
        uint32_t *active = nullptr;
        float *q_start = nullptr, *q_goal = nullptr;
        uint64_t *bits = nullptr, *path_offsets = nullptr;  // path_offsets: [n_items], for pack_paths
        uint8_t *done = nullptr, *h_done = nullptr;
        size_t n_items = 0;

        int alloc(DeviceBuffers &mem, size_t n, size_t n_active, size_t per_item, size_t dim, hipStream_t stream)
        {
            const size_t slots = std::max<size_t>(n_active, 1) * per_item, words = (slots + 63) / 64 + 1;
            n_items = n;
            VMV_LOCKSTEP_HIP(mem.alloc(&active, std::max<size_t>(n_active, 1)));
            VMV_LOCKSTEP_HIP(mem.alloc(&q_start, slots * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&q_goal, slots * dim));
            VMV_LOCKSTEP_HIP(mem.alloc(&bits, words));
            VMV_LOCKSTEP_HIP(mem.alloc(&done, n));
            VMV_LOCKSTEP_HIP(mem.alloc(&path_offsets, n));
            VMV_LOCKSTEP_HIP(hipHostMalloc(&mem.pinned, std::max<size_t>(n, 16), hipHostMallocDefault));
            h_done = static_cast<uint8_t *>(mem.pinned);
            VMV_LOCKSTEP_HIP(hipMemsetAsync(bits, 0, words * 8, stream));
            VMV_LOCKSTEP_HIP(hipMemsetAsync(done, 0, std::max<size_t>(n, 16), stream));
            return VMV_OK;
        }
        LockstepArrays arrays() const { return {active, q_start, q_goal, bits, done, h_done, n_items}; }
    };

    // skips [n] on the device; NULL = zeros
    inline int upload_skips(uint64_t *d_skips, const uint64_t *skips, size_t n, hipStream_t stream)
    {
        if (skips)
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(d_skips, skips, n * 8, hipMemcpyHostToDevice, stream));
        else
            VMV_LOCKSTEP_HIP(hipMemsetAsync(d_skips, 0, n * 8, stream));
        return VMV_OK;
    }

    // the inputs of n planning problems on the device: starts, goals [n][dim] and the Halton skips [n]
    inline int upload_problems(DeviceBuffers &mem, size_t n, size_t dim, const float *starts, const float *goals, const uint64_t *skips,
                               hipStream_t stream, const float **d_starts, const float **d_goals, const uint64_t **d_skips)
    {
        float *s = nullptr, *g = nullptr;
        uint64_t *k = nullptr;
        VMV_LOCKSTEP_HIP(mem.alloc(&s, n * dim));
        VMV_LOCKSTEP_HIP(mem.alloc(&g, n * dim));
        VMV_LOCKSTEP_HIP(mem.alloc(&k, n));
        VMV_LOCKSTEP_HIP(hipMemcpyAsync(s, starts, n * dim * 4, hipMemcpyHostToDevice, stream));
        VMV_LOCKSTEP_HIP(hipMemcpyAsync(g, goals, n * dim * 4, hipMemcpyHostToDevice, stream));
        *d_starts = s, *d_goals = g, *d_skips = k;
        return upload_skips(k, skips, n, stream);
    }

    // exclusive prefix sum of the path lengths; total: their sum
    inline std::vector<uint64_t> path_offsets_of(const uint32_t *lengths, size_t n, uint64_t &total)
    {
        std::vector<uint64_t> offsets(n);
        total = 0;
        for (size_t k = 0; k < n; ++k) offsets[k] = total, total += lengths[k];
        return offsets;
    }

    // The paths of a result, packed in item order into `paths`: item k has lengths[k] waypoints of dim floats.
    // launch(d_offsets, d_paths) launches the caller's gather / trace kernel `kernel`, which writes device item s at
    // waypoint d_offsets[s] — the offset of item order[s], or of item s where order is NULL.
    template <typename Launch>
    int pack_paths(DeviceBuffers &mem, uint64_t *d_offsets, const std::vector<uint32_t> &lengths, size_t dim, const uint32_t *order,
                   const char *kernel, Launch &&launch, std::vector<float> &paths)
    {
        const size_t n = lengths.size();
        uint64_t total = 0;
        std::vector<uint64_t> offsets = path_offsets_of(lengths.data(), n, total);
        paths.resize(total * dim);
        if (!total) return VMV_OK;
        if (order)
        {
            const std::vector<uint64_t> by_item(offsets);
            for (size_t s = 0; s < n; ++s) offsets[s] = by_item[order[s]];
        }
        float *d_paths = nullptr;
        VMV_LOCKSTEP_HIP(mem.alloc(&d_paths, total * dim));
        VMV_LOCKSTEP_HIP(hipMemcpy(d_offsets, offsets.data(), n * 8, hipMemcpyHostToDevice));
        launch(d_offsets, d_paths);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        {
            (void) hipDeviceSynchronize();
            return hip_status(e, kernel);
        }
        VMV_LOCKSTEP_HIP(hipMemcpy(paths.data(), d_paths, total * dim * 4, hipMemcpyDeviceToHost));
        return VMV_OK;
    }

    // The device-free checks the planner entry points begin with, in their order: the robot, the NULL pointers, the
    // problem count, the NULL handles.  -> VMV_OK and the robot's dimension, or the first failing check's code.
    inline int check_planner_call(int robot, const void *settings, const void *out, const vmv_env *const *envs, size_t n_problems,
                                  const float *starts, const float *goals, int *dim)
    {
        *dim = vmv_robot_dimension(robot);
        if (robot < 0 || robot >= vmv_num_robots() || *dim <= 0 || *dim > (int) kPlanMaxDim) return VMV_ERR_UNKNOWN_ROBOT;
        if (!settings || !out || (n_problems > 0 && (!envs || !starts || !goals))) return VMV_ERR_INVALID_ARGUMENT;
        if (n_problems >= kMultiMaxConfigs) return VMV_ERR_INVALID_ARGUMENT;
        for (size_t k = 0; k < n_problems; ++k)
            if (!envs[k]) return VMV_ERR_INVALID_ARGUMENT;
        return VMV_OK;
    }
    // The kinds of environment a call refuses, behind its argument checks: the checks vmv_validate_batch_multi - or, with
    // `clearance`, vmv_clearance_batch_multi, which refuses more kinds - makes of its handles, through an empty batch of it
    // (no device, no element read or written).  NULL envs: nothing to check.
    inline int check_env_kinds(int robot, const vmv_env *const *envs, size_t n, bool clearance)
    {
        if (!envs || n == 0) return VMV_OK;
        static float nothing[2] = {0.f, 0.f};
        static uint64_t no_bits[2] = {0, 0};
        const std::vector<size_t> zeros(n + 1, 0);
        return clearance ? vmv_clearance_batch_multi(robot, envs, zeros.data(), n, nothing, nothing, nullptr, nullptr)
                         : vmv_validate_batch_multi(robot, envs, zeros.data(), n, nothing, no_bits, nullptr);
    }
    // whether `draws` Halton elements after every skip stay within the sequence's limit (NULL skips = zeros)
    inline bool halton_skips_ok(const uint64_t *skips, size_t n, uint64_t draws)
    {
        if (!skips) return draws <= kMaxHaltonIndex;
        for (size_t k = 0; k < n; ++k)
            if (skips[k] > kMaxHaltonIndex || skips[k] + draws > kMaxHaltonIndex) return false;
        return true;
    }

    }  // namespace

    // Runs rounds until no item is active.  active / active_envs: the unfinished items and their environments, compacted
    // in place; item k of the list owns questions [k * per_item, (k + 1) * per_item) of a round.  launch_step(na) launches
    // the step kernel for the na active items on `stream`.  max_rounds bounds the rounds whatever the device answers; it
    // is looked at once per block of check_every rounds.  An empty list does nothing.  `call` and `step_kernel` name the
    // two in vmv_last_error().  Every return after a launch leaves the device idle.
    template <typename LaunchStep>
    int lockstep_rounds(int robot, hipStream_t stream, uint32_t check_every, uint64_t max_rounds, size_t per_item,
                        std::vector<uint32_t> &active, std::vector<const vmv_env *> &active_envs, const LockstepArrays &D,
                        const char *call, const char *step_kernel, LaunchStep &&launch_step, uint64_t &rounds)
    {
        std::vector<size_t> seg(active.size() + 1);
        for (size_t k = 0; k < seg.size(); ++k) seg[k] = k * per_item;
        rounds = 0;
        while (!active.empty())
        {
            if (rounds > max_rounds)
            {
                (void) hipDeviceSynchronize();
                return hip_status(hipErrorUnknown, (std::string(call) + ": the round bound was exceeded").c_str());
            }
            const size_t na = active.size();
            for (uint32_t r = 0; r < check_every; ++r, ++rounds)
            {
                launch_step((uint32_t) na);
                if (const hipError_t e = hipGetLastError(); e != hipSuccess)
                {
                    (void) hipDeviceSynchronize();
                    return hip_status(e, step_kernel);
                }
                if (int rc = vmv_validate_motion_batch_multi(robot, active_envs.data(), seg.data(), na, D.q_start, D.q_goal, D.bits,
                                                             stream);
                    rc != VMV_OK)
                {
                    (void) hipDeviceSynchronize();
                    return rc;
                }
            }
            VMV_LOCKSTEP_HIP(hipMemcpyAsync(D.h_done, D.done, D.n_items, hipMemcpyDeviceToHost, stream));
            VMV_LOCKSTEP_HIP(hipStreamSynchronize(stream));
            size_t kept = 0;
            for (size_t k = 0; k < na; ++k)
                if (!D.h_done[active[k]]) active[kept] = active[k], active_envs[kept] = active_envs[k], ++kept;
            if (kept != na)
            {
                active.resize(kept), active_envs.resize(kept);
                if (kept) VMV_LOCKSTEP_HIP(hipMemcpy(D.active, active.data(), kept * 4, hipMemcpyHostToDevice));
            }
        }
        return VMV_OK;
    }

    // What follows an entry point's own argument checks: the result object, vmv_env_prepare_multi (the environments' own
    // checks; builds the robot parts not yet built in one batch; not with envs == NULL, where the call allows that), then
    // run(result) if there is an item at all.  *out is written on success only.
    template <typename Result, typename Run>
    int lockstep_call(int robot, const vmv_env *const *envs, size_t n_items, int dim, Result **out, Run &&run)
    {
        Result *result = new (std::nothrow) Result;
        if (!result) return VMV_ERR_HIP;
        result->dim = dim;
        int rc = VMV_OK;
        if (n_items > 0)
        {
            if (envs) rc = vmv_env_prepare_multi(robot, envs, n_items);
            if (rc == VMV_OK) rc = run(result);
        }
        if (rc != VMV_OK)
        {
            delete result;
            return rc;
        }
        *out = result;
        return VMV_OK;
    }
}  // namespace vmv
