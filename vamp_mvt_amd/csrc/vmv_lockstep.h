// vmv_lockstep.h — the host side the lockstep calls share (vmv_rrtc_multi, vmv_simplify_multi; DESIGN §5c "A round").
//
// Every item of a call (a planning problem, a path) is a state machine in device memory.  One round = the call's step
// kernel (one workgroup per unfinished item: consumes the answers to the item's previous questions, advances its state and
// writes its next questions into the round's start / goal arrays) + one vmv_validate_motion_batch_multi call over those
// edges.  The host does nothing per item inside a round and does not synchronise; every check_every rounds it reads the
// finished flags and compacts the active list.  lockstep_rounds() below is that loop, with every synchronisation point
// and every error exit of a call's rounds; the kernels, the state and the allocation sizes stay with each caller.
#pragma once

#include "../../include/vamp_mvt_amd.h"

#include "vmv_common.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace vmv
{
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

    struct LockstepArrays  // what the rounds of one call read and write; allocated and sized by the caller
    {
        uint32_t *active;               // [initial active count] item of each workgroup, uploaded by the caller
        const float *q_start, *q_goal;  // [active][per_item][dim] the round's questions
        uint64_t *bits;                 // their answers, read by the next round's step kernel
        const uint8_t *done;            // [n_items] set by the step kernel
        uint8_t *h_done;                // [n_items] pinned
        size_t n_items;
    };

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
    // checks; builds the robot parts not yet built in one batch), then run(result) if there is an item at all.  *out is
    // written on success only.
    template <typename Result, typename Run>
    int lockstep_call(int robot, const vmv_env *const *envs, size_t n_items, int dim, Result **out, Run &&run)
    {
        Result *result = new (std::nothrow) Result;
        if (!result) return VMV_ERR_HIP;
        result->dim = dim;
        int rc = VMV_OK;
        if (n_items > 0)
        {
            rc = vmv_env_prepare_multi(robot, envs, n_items);
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
