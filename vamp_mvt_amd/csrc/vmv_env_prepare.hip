// vmv_env_prepare.hip — the robot-specific part of many environments at once (vmv_env_prepare_multi): broad-phase
// grids and reach certificates on the device.  The static links are the third kernel; it needs the robot's generated
// code and lives in vmv_robot_tu.inc (static_links_multi_kernel).
//
// Both kernels evaluate the distance expressions of vmv_grid_build.h (grid_detail, compiled __host__ __device__) in
// double precision, operation for operation as the host builder does: the build has -ffp-contract=off -fno-fast-math,
// double-precision sqrt and division are correctly rounded on gfx950 and double denormals are kept, so every cell word
// and every certificate bit equals what the lazy host path computes (tests/test_env_prepare_gpu.py compares them).
// Every output word has one owning thread: plain vector stores, no atomics.
#include "vmv_grid_build.h"
#include "vmv_common.h"

namespace vmv
{
    namespace
    {
        constexpr uint32_t kPrepBlock = 256;
        constexpr uint32_t kPrepMaxWords = 4;  // candidate words of an environment that has a grid (kMaskWords)

        // the environment's primitive records -> LDS (whole 32-bit words, every lane reads the same record later)
        __device__ __forceinline__ void stage_prims(const PrepPrim *__restrict__ prims, uint32_t lo, uint32_t n, PrepPrim *lds)
        {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(prims + lo);
            uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
            const uint32_t words = n * (uint32_t) (sizeof(PrepPrim) / 4);
            for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
            __syncthreads();
        }

        // One thread per cell of grid job blockIdx.y + job0; the thread owns the cell's candidate words.
        __global__ __launch_bounds__(kPrepBlock) void grid_fill_kernel(const PrepPrim *__restrict__ prims,
                                                                       const PrepGridJob *__restrict__ jobs, const uint32_t job0,
                                                                       uint32_t *__restrict__ cells)
        {
            __shared__ PrepPrim lds[kPrepMaxPrims];
            const PrepGridJob &J = jobs[job0 + blockIdx.y];
            const uint32_t n_cells = J.dims[0] * J.dims[1] * J.dims[2];  // (at most a few 10^4: the host caps the grid)
            if (blockIdx.x * kPrepBlock >= n_cells) return;               // workgroup-uniform
            const uint32_t n_prims = J.n_prims < kPrepMaxPrims ? J.n_prims : kPrepMaxPrims;
            stage_prims(prims, J.prim_lo, n_prims, lds);
            const uint32_t idx = blockIdx.x * kPrepBlock + threadIdx.x;
            if (idx >= n_cells) return;
            const uint32_t iz = idx % J.dims[2], iy = (idx / J.dims[2]) % J.dims[1], ix = idx / (J.dims[2] * J.dims[1]);
            const double hf = J.hf, half_diag = J.half_diag, R = J.R;
            const double c[3] = {grid_detail::cell_centre(J.origin[0], ix, hf), grid_detail::cell_centre(J.origin[1], iy, hf),
                                 grid_detail::cell_centre(J.origin[2], iz, hf)};
            uint32_t w[kPrepMaxWords] = {0u, 0u, 0u, 0u};
            for (uint32_t k = 0; k < n_prims; ++k)
            {
                const PrepPrim &g = lds[k];
                const uint32_t bit = grid_detail::cell_lists(g.type, g.p, c, R, half_diag) ? 1u << g.bit : 0u;
#pragma unroll
                for (uint32_t j = 0; j < kPrepMaxWords; ++j) w[j] |= (g.word == j) ? bit : 0u;
            }
            const uint32_t words = J.words < kPrepMaxWords ? J.words : kPrepMaxWords;
            uint32_t *out = cells + J.cell_lo + (size_t) idx * words;
#pragma unroll
            for (uint32_t j = 0; j < kPrepMaxWords; ++j)
                if (j < words) out[j] = w[j];
        }

        // One workgroup per environment: every sample of every link against every primitive; bit `group` of link_skip
        // is set when no sample of the link comes within `need` (times the primitive's Lipschitz bound) of a primitive.
        __global__ __launch_bounds__(kPrepBlock) void reach_kernel(const PrepPrim *__restrict__ prims,
                                                                   const PrepReachJob *__restrict__ jobs,
                                                                   const PrepReachLink *__restrict__ links, const uint32_t n_links,
                                                                   const float *__restrict__ samples,
                                                                   unsigned long long *__restrict__ skip_out)
        {
            __shared__ PrepPrim lds[kPrepMaxPrims];
            const PrepReachJob &J = jobs[blockIdx.x];
            const uint32_t n_prims = J.n_prims < kPrepMaxPrims ? J.n_prims : kPrepMaxPrims;
            stage_prims(prims, J.prim_lo, n_prims, lds);
            unsigned long long skip = 0ull;
            for (uint32_t l = 0; l < n_links; ++l)  // workgroup-uniform
            {
                const PrepReachLink L = links[l];
                int blocked = 0;
                for (uint32_t i = threadIdx.x; i < L.n; i += kPrepBlock)
                {
                    const float *s = samples + 3 * (size_t) (L.sample_lo + i);
                    const double x[3] = {s[0], s[1], s[2]};
                    for (uint32_t k = 0; k < n_prims; ++k)
                    {
                        const PrepPrim &g = lds[k];
                        double lip = 1.0;
                        const double d = grid_detail::prim_g(g.type, g.p, x, lip);
                        if (!(d > L.need * lip)) blocked = 1;
                    }
                }
                if (!__syncthreads_or(blocked)) skip |= 1ull << L.group;
            }
            if (threadIdx.x == 0)
            {
                J.image->link_skip = skip;
                skip_out[J.out] = skip;
            }
        }
    }  // namespace

    int launch_grid_fill(const PrepPrim *d_prims, const PrepGridJob *d_jobs, const PrepGridJob *jobs, size_t n_jobs,
                         uint32_t *d_cells, hipStream_t stream)
    {
        constexpr size_t kMaxY = 65535;
        for (size_t j0 = 0; j0 < n_jobs; j0 += kMaxY)
        {
            const size_t m = n_jobs - j0 < kMaxY ? n_jobs - j0 : kMaxY;
            uint32_t most = 1;
            for (size_t j = j0; j < j0 + m; ++j)
            {
                const uint32_t n_cells = jobs[j].dims[0] * jobs[j].dims[1] * jobs[j].dims[2];
                most = n_cells > most ? n_cells : most;
            }
            hipLaunchKernelGGL(grid_fill_kernel, dim3((most + kPrepBlock - 1) / kPrepBlock, (uint32_t) m), dim3(kPrepBlock), 0,
                               stream, d_prims, d_jobs, (uint32_t) j0, d_cells);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_status(e, "grid_fill_kernel");
        }
        return 0;
    }

    int launch_reach(const PrepPrim *d_prims, const PrepReachJob *d_jobs, size_t n_jobs, const PrepReachLink *d_links,
                     uint32_t n_links, const float *d_samples, unsigned long long *d_skip_out, hipStream_t stream)
    {
        constexpr size_t kMaxX = size_t{1} << 30;
        for (size_t j0 = 0; j0 < n_jobs; j0 += kMaxX)
        {
            const size_t m = n_jobs - j0 < kMaxX ? n_jobs - j0 : kMaxX;
            hipLaunchKernelGGL(reach_kernel, dim3((uint32_t) m), dim3(kPrepBlock), 0, stream, d_prims, d_jobs + j0, d_links,
                               n_links, d_samples, d_skip_out);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_status(e, "reach_kernel");
        }
        return 0;
    }
}  // namespace vmv
