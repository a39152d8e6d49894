// vmv_robot_launch.inc — the host launchers of ONE robot and make_launchers, which fills its RobotLaunchers object.
// Included by vmv_robot_tu.inc behind the kernels, inside namespace vmv::VMV_ROBOT_NS.
//
// Kernel variants: env_class (vmv_common.h) maps an environment to its class 0..3 and every validate launcher indexes
// its kernel table with it, so the multi launchers run each segment on the variant its environment runs alone.  A new
// variant kernel goes into the table of its launcher and to the end of kVariantKernelOrder; a new launcher goes into
// make_launchers at the end.
    namespace
    {
#define VMV_HIP_TU(call)                                           \
    do                                                             \
    {                                                              \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return hip_status(e_, #call);        \
    } while (0)

        // The compiler lays the instantiated kernels out in the code object in the order in which this file first names
        // them (which of two identical helper instances it keeps follows from that too), and bench.py has shown differences
        // that came from the layout alone (profiles/r29_ab_vs_parent.txt).  This list names the variant kernels first, in
        // the order the code objects have always had, so that the tables below can stand in class order.  Nothing reads it.
        template <class... K>
        constexpr int named(K *...) { return 0; }
        // the self-collision kernel's instances: [VMV_SELF_SCREEN] 0 no screen, 1 (and unset) the prescreen, 2 the exact
        // screen; robots without R::kSelfScreen have the unscreened instance only
        constexpr int self_default() { return R::kSelfScreen ? kSelfPrescreen : kSelfUnscreened; }
        constexpr int self_exact() { return R::kSelfScreen ? kSelfExactScreen : kSelfUnscreened; }
        [[maybe_unused]] constexpr int kVariantKernelOrder = named(
            validate_env_kernel<kEnvClouds>, validate_env_kernel<kEnvFull>, validate_env_kernel<kEnvZOnly>,
            validate_env_kernel<kEnvPrims>, validate_env_kernel<kEnvZOnly, R::kFinePairs>,
            validate_env_kernel<kEnvPrims, R::kFinePairs>, validate_self_kernel<self_default()>, validate_self_kernel<kSelfUnscreened>,
            validate_env_multi_kernel<kEnvZOnly, R::kFinePairs>, validate_env_multi_kernel<kEnvPrims, R::kFinePairs>,
            validate_env_multi_kernel<kEnvZOnly>, validate_env_multi_kernel<kEnvPrims>, validate_env_multi_kernel<kEnvFull>,
            validate_env_multi_kernel<kEnvClouds>, rake_tasks_env_kernel<kEnvClouds>, rake_tasks_env_kernel<kEnvFull>,
            rake_tasks_env_kernel<kEnvZOnly>, rake_tasks_env_kernel<kEnvPrims>, rake_tasks_fused_kernel<kEnvZOnly>,
            rake_tasks_fused_kernel<kEnvPrims>, validate_self_kernel<self_exact()>);

        // LDS of the environment kernels: [primitive block | CAPT split planes | hit flags, radius table | one slab per
        // wave | control words]; of the clearance kernels the same head without planes.  The float offset of wave 0's slab:
        constexpr uint32_t lds_head(const EnvDev &D, uint32_t tests_in_lds)
        {
            return ((D.n_floats + tests_in_lds + 3u) & ~3u) + kEnvRadiiFloats;
        }

        uint32_t lds_bytes(const EnvDev &D, uint32_t tests_in_lds)
        {
            return (lds_head(D, tests_in_lds) + (uint32_t) kWavesPerBlock * slab_floats() + kCtrlWords) * (uint32_t) sizeof(float);
        }

        // The top levels of point cloud 0's split-plane tree go to LDS (every query walks them); the budget keeps
        // four workgroups per CU resident.
        int plan_lds(const EnvLaunch &env, uint32_t &tests_in_lds, uint32_t &shmem)
        {
            const EnvDev &D = env.host;
            const uint32_t budget = 2u * 1024u;  // measured: 2 KiB beats 0, 4, 8, 16 KiB (occupancy outweighs the deeper LDS levels)
            tests_in_lds = 0;  // floats: whole 3-level groups of the blocked plane copy, from the root down
            if (D.n_capt > 0) tests_in_lds = capt_plane_floats(D.capt[0].nlog2, budget / (uint32_t) sizeof(float));
            shmem = lds_bytes(D, tests_in_lds);
            if (shmem > kMaxLdsBytes && tests_in_lds)
            {
                tests_in_lds = 0;
                shmem = lds_bytes(D, 0);
            }
            return shmem > kMaxLdsBytes ? VMV_ERR_CAPACITY : VMV_OK;
        }

        // A kernel takes more than 64 KiB of dynamic LDS only after it has been allowed to.  Reachable: vmv_env_finalize
        // admits kMaxPrimFloats (48 KiB) of primitive records, and radii, flags, slabs and control words add 20.7 KiB
        // (Panda) to 33.1 KiB (Fetch), so environments in the upper part of that budget (above 11,080 floats of records
        // for Panda, 7,916 for Fetch) pass 64 KiB.  The largest plan is 83.1 KiB (Fetch, with 2 KiB of planes): plan_lds'
        // own refusal at kMaxLdsBytes cannot be reached through vmv_env_finalize and stays as the guard it is.
        template <class K>
        hipError_t allow_lds(K *kernel, uint32_t shmem)
        {
            if (shmem <= 64u * 1024u) return hipSuccess;
            return hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) shmem);
        }

        // the pair-dealt instances of the primitive-only configuration kernels (robots with R::kFinePairs;
        // VMV_FINE_PAIRS=0 selects the other instances: measurement and test aid)
        bool fine_pairs()
        {
            if (const char *e = getenv("VMV_FINE_PAIRS")) return strtoul(e, nullptr, 10) != 0ul && R::kFinePairs;
            return R::kFinePairs;
        }

        int grid_for(size_t items, size_t per_block)
        {
            const size_t blocks = (items + per_block - 1) / per_block;
            return (int) (blocks < 256u * 64u ? blocks : 256u * 64u);
        }

        // fn(lo, m) for the slices [lo, lo + m) of n items, m <= slice: the kernels count in 32 bits
        template <class F>
        void for_slices(size_t n, size_t slice, F fn)
        {
            for (size_t lo = 0; lo < n; lo += slice) fn(lo, (uint32_t) std::min(n - lo, slice));
        }

        // one launch without dynamic LDS
        template <class K, class... Args>
        int launch_flat(K *kernel, size_t grid, uint32_t block, hipStream_t stream, Args... args)
        {
            hipLaunchKernelGGL(kernel, dim3((uint32_t) grid), dim3(block), 0, stream, args...);
            VMV_HIP_TU(hipGetLastError());
            return VMV_OK;
        }

        constexpr uint32_t kTasksPerBlock = (uint32_t) (kWavesPerBlock * 8);  // (edge, rake) tasks per workgroup pass
        // the later pass (rakes 1 and up) of `edges` edges: the task count is only known on the device, so the grid is sized
        // for the batch (a workgroup without a task leaves before it stages anything) and strides over the tasks
        int later_grid(size_t edges) { return std::min(grid_for(std::max(edges * 8u, size_t{8192}), kTasksPerBlock), 8192); }

        // the attachment walk's edges per workgroup pass: as large as kChunkEdges while the grid still has >= 2,048
        // workgroups (2.7 rounds of the resident ones), never below one validity word
        uint32_t attach_chunk(size_t edges)
        {
            uint32_t chunk = kChunkEdges;
            while (chunk > 64u && (edges + chunk - 1) / chunk < 2048u) chunk /= 2u;
            return chunk;
        }

#ifdef VMV_SELF_STAMP
        uint64_t *d_stamp = nullptr;
        size_t stamp_cap = 0;
        int stamp_reset(size_t waves, hipStream_t stream)  // the records of one launch, zeroed
        {
            if (waves > stamp_cap)
            {
                if (d_stamp) VMV_HIP_TU(hipFree(d_stamp));
                stamp_cap = waves;
                VMV_HIP_TU(hipMalloc(&d_stamp, stamp_cap * 4 * sizeof(uint64_t)));
                VMV_HIP_TU(hipMemcpyToSymbol(HIP_SYMBOL(self_stamp), &d_stamp, sizeof(d_stamp)));
            }
            VMV_HIP_TU(hipMemsetAsync(d_stamp, 0, waves * 4 * sizeof(uint64_t), stream));
            return VMV_OK;
        }
        // header: n, group, workgroups, 1 (the shared-pass kernel; files of older builds may hold 0, the per-wave
        // kernel); then 4 words per wave.  Overwritten per launch.
        int stamp_dump(uint32_t m, uint32_t group, size_t blocks, hipStream_t stream)
        {
            const char *path = getenv("VMV_SELF_STAMP_OUT");
            if (!path) return VMV_OK;
            std::vector<uint64_t> rec(4 + blocks * kWavesPerBlock * 4);
            rec[0] = m, rec[1] = group, rec[2] = blocks, rec[3] = 1u;
            VMV_HIP_TU(hipMemcpyAsync(rec.data() + 4, d_stamp, blocks * kWavesPerBlock * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                      stream));
            VMV_HIP_TU(hipStreamSynchronize(stream));
            if (FILE *f = fopen(path, "wb"))
            {
                fwrite(rec.data(), sizeof(uint64_t), rec.size(), f);
                fclose(f);
            }
            return VMV_OK;
        }
#else  // (every other build)
        int stamp_reset(size_t, hipStream_t) { return VMV_OK; }
        int stamp_dump(uint32_t, uint32_t, size_t, hipStream_t) { return VMV_OK; }
#endif

        int launch_validate(const EnvLaunch &env, const float *d_q, size_t n, uint64_t *d_bits, hipStream_t stream,
                            int stages)
        {
            constexpr size_t kSlice = size_t{1} << 31;  // the kernels count in 32 bits; slices own whole validity words
            if (stages & 1)
            {
                // [pair-dealt][class]; R::kFinePairs in the second row: the pair-dealt instances exist for these robots only
                static constexpr decltype(&validate_env_kernel<kEnvFull>) kernels[2][kEnvClasses] = {
                    {validate_env_kernel<kEnvZOnly>, validate_env_kernel<kEnvPrims>, validate_env_kernel<kEnvFull>,
                     validate_env_kernel<kEnvClouds>},
                    {validate_env_kernel<kEnvZOnly, R::kFinePairs>, validate_env_kernel<kEnvPrims, R::kFinePairs>,
                     validate_env_kernel<kEnvFull>, validate_env_kernel<kEnvClouds>}};
                const auto kernel = kernels[fine_pairs()][env_class(env)];
                uint32_t tests_in_lds, shmem;
                if (int rc = plan_lds(env, tests_in_lds, shmem); rc != VMV_OK) return rc;
                VMV_HIP_TU(allow_lds(kernel, shmem));
                for_slices(n, kSlice, [&](size_t lo, uint32_t m)
                           {
                               hipLaunchKernelGGL(kernel, dim3(grid_for(m, kBlock)), dim3(kBlock), shmem, stream, env.d_env,
                                                  tests_in_lds, d_q + lo * R::kDim, m, d_bits + lo / kWave);
                           });
                VMV_HIP_TU(hipGetLastError());
            }
            if (stages & 2)
            {
                // words per wave: one round of resident workgroups (the hardware's count: 256 CUs x kSelfBlocks workgroups
                // x 4 waves on the MI355X) covers the batch, at most 8 (VMV_SELF_GROUP overrides: measurement aid)
                const size_t words = (n + kWave - 1) / kWave;
                static const size_t resident = []
                {
                    int per_cu = 0, dev = 0, cus = 256;
                    const void *k = (const void *) validate_self_kernel<self_default()>;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, kBlock, 0) != hipSuccess || per_cu < 1)
                        per_cu = R::kSelfBlocks;
                    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                        cus < 1)
                        cus = 256;
                    return (size_t) cus * (size_t) per_cu * kWavesPerBlock;
                }();
                uint32_t group = (uint32_t) ((words + resident - 1) / resident);
                if (const char *e = getenv("VMV_SELF_GROUP")) group = (uint32_t) strtoul(e, nullptr, 10);
                group = group < 1u ? 1u : (group > 8u ? 8u : group);
                // [VMV_SELF_SCREEN]; every other value, and the variable unset: the default (measurement and test aid)
                static constexpr decltype(&validate_self_kernel<kSelfUnscreened>) self_kernels[3] = {
                    validate_self_kernel<kSelfUnscreened>, validate_self_kernel<self_default()>, validate_self_kernel<self_exact()>};
                auto self_kernel = self_kernels[1];
                if (const char *e = getenv("VMV_SELF_SCREEN"))
                    if (const unsigned long mode = strtoul(e, nullptr, 10); mode == 0ul || mode == 2ul) self_kernel = self_kernels[mode];
                int rc = VMV_OK;  // (of the stamps: measurement builds only)
                for_slices(n, kSlice, [&](size_t lo, uint32_t m)
                           {
                               const size_t waves = (((size_t) m + kWave - 1) / kWave + group - 1) / group;
                               const size_t blocks = grid_for(waves * kWave, kBlock);
                               if (rc == VMV_OK) rc = stamp_reset(blocks * kWavesPerBlock, stream);
                               hipLaunchKernelGGL(self_kernel, dim3(blocks), dim3(kBlock), 0, stream, d_q + lo * R::kDim, m,
                                                  d_bits + lo / kWave, group);
                               if (rc == VMV_OK) rc = stamp_dump(m, group, blocks, stream);
                           });
                if (rc != VMV_OK) return rc;
                VMV_HIP_TU(hipGetLastError());
            }
            if ((stages & 4) && env.host.n_attach > 0)  // planning/validate.hh:43: fkcc_attach iff attachments
            {
                uint32_t tests_in_lds, shmem;
                if (int rc = plan_lds(env, tests_in_lds, shmem); rc != VMV_OK) return rc;
                VMV_HIP_TU(allow_lds(validate_attach_kernel, shmem));
                hipLaunchKernelGGL(validate_attach_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), shmem, stream,
                                   env.d_env, tests_in_lds, d_q, n, d_bits);
                VMV_HIP_TU(hipGetLastError());
            }
            return VMV_OK;
        }

        // vmv_validate_batch_multi.  Every segment runs the variant its environment runs alone (env_class, the choice of
        // launch_validate), one launch per class present, each with its own tile table; then the self-collision
        // kernel once over the whole batch (it does not depend on the environment), then the attachment kernel over the
        // segments whose environment has an attachment.  Table: [segments | tiles of class 0 | .. | class 3 | attachment
        // tiles], one workgroup per tile.
        int launch_validate_multi(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                                  uint64_t *d_bits, hipStream_t stream)
        {
            constexpr int kAttach = kEnvClasses;          // the tables' last column: the attachment kernel
            constexpr size_t kMaxGrid = size_t{1} << 20;  // workgroups per launch (grids of up to 2^24 are legal)
            // [pair-dealt][class | attachment] (robots without the pair-dealt instances: R::kFinePairs is false, the rows
            // are the same kernels)
            static constexpr decltype(&validate_attach_multi_kernel) kernels[2][kEnvClasses + 1] = {
                {validate_env_multi_kernel<kEnvZOnly>, validate_env_multi_kernel<kEnvPrims>, validate_env_multi_kernel<kEnvFull>,
                 validate_env_multi_kernel<kEnvClouds>, validate_attach_multi_kernel},
                {validate_env_multi_kernel<kEnvZOnly, R::kFinePairs>, validate_env_multi_kernel<kEnvPrims, R::kFinePairs>,
                 validate_env_multi_kernel<kEnvFull>, validate_env_multi_kernel<kEnvClouds>, validate_attach_multi_kernel}};
            const size_t n = offsets[n_envs];
            if (n == 0) return VMV_OK;
            std::vector<MultiSeg> segs(n_envs);
            size_t n_tiles[kEnvClasses + 1] = {}, at[kEnvClasses + 1];
            uint32_t shmem[kEnvClasses + 1] = {};
            bool any_shared = false;
            for (size_t k = 0; k < n_envs; ++k)
            {
                const EnvLaunch &e = *envs[k];
                uint32_t tests_in_lds = 0, bytes = 0;
                if (offsets[k] < offsets[k + 1])
                    if (int rc = plan_lds(e, tests_in_lds, bytes); rc != VMV_OK) return rc;
                segs[k] = MultiSeg{e.d_env, (uint32_t) offsets[k], (uint32_t) offsets[k + 1], tests_in_lds,
                                   lds_head(e.host, tests_in_lds)};
                if (offsets[k] == offsets[k + 1]) continue;
                const size_t tiles = ((offsets[k + 1] - 1) / kWave - offsets[k] / kWave) / kWavesPerBlock + 1;
                any_shared |= offsets[k] % kWave != 0;
                for (const int c : {env_class(e), e.host.n_attach > 0 ? kAttach : -1})
                    if (c >= 0)
                    {
                        n_tiles[c] += tiles;
                        shmem[c] = bytes > shmem[c] ? bytes : shmem[c];
                    }
            }
            size_t total = 0;
            for (int c = 0; c <= kEnvClasses; ++c) at[c] = total, total += n_tiles[c];
            const MultiTableLayout table(n_envs, total);
            MultiTableLease lease;
            if (int rc = lease.acquire(stream, table.bytes); rc != VMV_OK) return rc;
            std::memcpy(lease.host, segs.data(), n_envs * sizeof(MultiSeg));
            MultiTile *tiles = table.tiles(lease.host);
            size_t fill[kEnvClasses + 1];
            std::copy(at, at + kEnvClasses + 1, fill);
            for (size_t k = 0; k < n_envs; ++k)
            {
                if (offsets[k] == offsets[k + 1]) continue;
                const int cls = env_class(*envs[k]);
                const bool attach = envs[k]->host.n_attach > 0;
                for (size_t w = offsets[k] / kWave; w <= (offsets[k + 1] - 1) / kWave; w += kWavesPerBlock)
                {
                    tiles[fill[cls]++] = MultiTile{(uint32_t) k, (uint32_t) w};
                    if (attach) tiles[fill[kAttach]++] = MultiTile{(uint32_t) k, (uint32_t) w};
                }
            }
            const MultiSeg *d_segs = table.segs(lease.dev);
            const MultiTile *d_tiles = table.tiles(lease.dev);
            if (any_shared) VMV_HIP_TU(hipMemsetAsync(d_bits, 0, (n + kWave - 1) / kWave * sizeof(uint64_t), stream));
            if (int rc = lease.upload(stream, table.bytes); rc != VMV_OK) return rc;
            const auto *row = kernels[fine_pairs()];
            auto launch = [&](int c) -> int
            {
                if (n_tiles[c] == 0) return VMV_OK;
                VMV_HIP_TU(allow_lds(row[c], shmem[c]));
                for (size_t t0 = 0; t0 < n_tiles[c]; t0 += kMaxGrid)  // one workgroup per tile
                    hipLaunchKernelGGL(row[c], dim3((uint32_t) std::min(n_tiles[c] - t0, kMaxGrid)), dim3(kBlock), shmem[c], stream,
                                       d_segs, d_tiles + at[c] + t0, d_q, (uint32_t) n, d_bits);
                VMV_HIP_TU(hipGetLastError());
                return VMV_OK;
            };
            for (int c = 0; c < kEnvClasses; ++c)
                if (int rc = launch(c); rc != VMV_OK) return rc;
            if (int rc = launch_validate(EnvLaunch{}, d_q, n, d_bits, stream, 2); rc != VMV_OK) return rc;
            return launch(kAttach);
        }

        // vmv_validate_motion_batch as (edge, rake) tasks in two passes: rake 0 of every edge, then all the other rakes of
        // the edges still valid.  Measured on one MI355X against the edge walk (one rake group walks one edge) and against
        // passes of doubling width (profiles/r03_edge_schedules.txt): the two passes won at every batch size and on every
        // workload (UR5 2,048 edges 0.54 -> 0.17 ms, 131,072 edges 1.37 -> 0.90 ms, 1M edges 8.2 -> 6.3 ms; Baxter + CAPT
        // 262,144 edges 26.3 -> 18.9 ms).  fused: both halves in rake_tasks_fused_kernel, one FK and one launch per pass.
        int launch_rake_tasks(const EnvLaunch &env, uint32_t tests_in_lds, uint32_t shmem, const float *d_a, const float *d_b,
                              size_t n_all, uint64_t *d_bits, hipStream_t stream, bool fused)
        {
            // [fused][class]; the fused kernels serve primitives only (the caller has checked: R::kHasFused, class 0 or 1)
            static constexpr decltype(&rake_tasks_env_kernel<kEnvFull>) kernels[2][kEnvClasses] = {
                {rake_tasks_env_kernel<kEnvZOnly>, rake_tasks_env_kernel<kEnvPrims>, rake_tasks_env_kernel<kEnvFull>,
                 rake_tasks_env_kernel<kEnvClouds>},
                {rake_tasks_fused_kernel<kEnvZOnly>, rake_tasks_fused_kernel<kEnvPrims>, nullptr, nullptr}};
            const auto env_kernel = kernels[fused][env_class(env)];
            if (fused)
            {
                shmem = (lds_head(env.host, tests_in_lds) + (uint32_t) kWavesPerBlock * fused_slab_floats()) * (uint32_t) sizeof(float);
                if (shmem > kMaxLdsBytes) return VMV_ERR_CAPACITY;
            }
            VMV_HIP_TU(allow_lds(env_kernel, shmem));
            for (size_t base = 0; base < n_all; base += kEdgeSliceEdges)  // (slices are multiples of 64 edges)
            {
                const uint32_t n = (uint32_t) ((n_all - base < kEdgeSliceEdges) ? n_all - base : kEdgeSliceEdges);
                const float *a = d_a + base * R::kDim, *b = d_b + base * R::kDim;
                uint8_t *bits8 = reinterpret_cast<uint8_t *>(d_bits + base / 64);
                EdgeScratchLease lease;
                if (int rc = lease.acquire(stream, n); rc != VMV_OK) return rc;
                const EdgeScratch &S = lease.s;
                const uint32_t padded = (n + 63u) & ~63u;
                hipLaunchKernelGGL(env_kernel, dim3(grid_for(padded, kTasksPerBlock)), dim3(kBlock), shmem, stream, env.d_env,
                                   tests_in_lds, a, b, n, bits8, S.steps, (const uint32_t *) nullptr, (const uint32_t *) nullptr,
                                   0u, 1u);
                if (!fused)
                    hipLaunchKernelGGL(rake_tasks_self_kernel, dim3(grid_for(n, kTasksPerBlock)), dim3(kBlock), 0, stream, a, b, n,
                                       bits8, (const uint32_t *) nullptr, (const uint32_t *) nullptr, 0u, 1u);
                VMV_HIP_TU(hipGetLastError());
                if (int rc = launch_edge_pass_scan(S, d_bits + base / 64, n, 1u, 0xffffffffu, 0u, stream); rc != VMV_OK) return rc;
                hipLaunchKernelGGL(env_kernel, dim3(later_grid(n)), dim3(kBlock), shmem, stream, env.d_env, tests_in_lds, a, b, n,
                                   bits8, (uint32_t *) nullptr, (const uint32_t *) S.excl, (const uint32_t *) S.total, 1u, 0u);
                if (!fused)
                    hipLaunchKernelGGL(rake_tasks_self_kernel, dim3(later_grid(n)), dim3(kBlock), 0, stream, a, b, n, bits8,
                                       (const uint32_t *) S.excl, (const uint32_t *) S.total, 1u, 0u);
                VMV_HIP_TU(hipGetLastError());
            }
            return VMV_OK;
        }

        int launch_validate_motion(const EnvLaunch &env, const float *d_a, const float *d_b, size_t n, uint64_t *d_bits,
                                   hipStream_t stream)
        {
            uint32_t tests_in_lds, shmem;
            if (int rc = plan_lds(env, tests_in_lds, shmem); rc != VMV_OK) return rc;
            // the fused task kernel where it exists, for batches too small to fill the chip (VMV_EDGE_FUSED_BELOW).
            // VMV_EDGE_TASKS (test aid, read per call: the parity tests switch it) forces one side: 1 = the two task
            // kernels, 3 = the fused one where it exists; any other value is ignored
            const bool can_fuse = R::kHasFused && env_class(env) <= 1 && env.host.n_attach == 0;
            const char *forced = getenv("VMV_EDGE_TASKS");
            const bool force_two = forced && strcmp(forced, "1") == 0, force_fused = forced && strcmp(forced, "3") == 0;
            const bool fused = can_fuse && (force_fused || (!force_two && n < (size_t) VMV_EDGE_FUSED_BELOW));
            if (int rc = launch_rake_tasks(env, tests_in_lds, shmem, d_a, d_b, n, d_bits, stream, fused); rc != VMV_OK) return rc;
            if (env.host.n_attach > 0)  // the attachment part continues the edges still valid (motion_body)
            {
                const uint32_t chunk = attach_chunk(n);
                VMV_HIP_TU(allow_lds(validate_motion_attach_kernel, shmem));
                hipLaunchKernelGGL(validate_motion_attach_kernel, dim3(grid_for(n, chunk)), dim3(kBlock), shmem, stream,
                                   env.d_env, tests_in_lds, d_a, d_b, n, reinterpret_cast<uint32_t *>(d_bits), chunk);
                VMV_HIP_TU(hipGetLastError());
            }
            return VMV_OK;
        }

        // vmv_validate_motion_batch_multi: launch_rake_tasks (two-kernel form) made segmented, slice by slice (segments
        // clipped at the slice's ends).  Per slice: the validity words zeroed; pass 0 of the environment half, one launch
        // per variant class present (each segment runs the class launch_rake_tasks picks for its environment alone), one
        // workgroup per 32-edge validity word of a segment; the self-collision half and the scan once over the slice (they
        // do not depend on the environment); the later pass's tiles from the scan, on the device; the later pass of the
        // environment half per class; the self-collision half's later pass; the attachment walk over the segments whose
        // environment has one.  Table: [segments | pass-0 tiles per class | later-pass entries per class | attachment
        // tiles] written by the host, then [starts | chunk] written by launch_edge_multi_tiles.
        int launch_validate_motion_multi(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_a,
                                         const float *d_b, uint64_t *d_bits, hipStream_t stream)
        {
            constexpr int kClasses = kEnvClasses;
            static_assert(kClasses == kEdgeMultiClasses, "EdgeMultiPlan holds one entry per class");
            // [pass: first, later][class]
            static constexpr decltype(&rake_tasks_env_multi_kernel<kEnvFull, true>) kernels[2][kClasses] = {
                {rake_tasks_env_multi_kernel<kEnvZOnly, true>, rake_tasks_env_multi_kernel<kEnvPrims, true>,
                 rake_tasks_env_multi_kernel<kEnvFull, true>, rake_tasks_env_multi_kernel<kEnvClouds, true>},
                {rake_tasks_env_multi_kernel<kEnvZOnly, false>, rake_tasks_env_multi_kernel<kEnvPrims, false>,
                 rake_tasks_env_multi_kernel<kEnvFull, false>, rake_tasks_env_multi_kernel<kEnvClouds, false>}};
            const size_t n_all = offsets[n_envs];
            if (n_all == 0) return VMV_OK;
            std::vector<uint32_t> tests_in_lds(n_envs), bytes(n_envs);  // every plan before anything is launched
            size_t attach_edges = 0;
            for (size_t k = 0; k < n_envs; ++k)
                if (offsets[k] < offsets[k + 1])
                {
                    if (int rc = plan_lds(*envs[k], tests_in_lds[k], bytes[k]); rc != VMV_OK) return rc;
                    if (envs[k]->host.n_attach > 0) attach_edges += offsets[k + 1] - offsets[k];
                }
            const uint32_t chunk = attach_chunk(attach_edges);  // the attachment walk's, sized as launch_validate_motion sizes it
            size_t k0 = 0;
            for (size_t base = 0; base < n_all; base += kEdgeSliceEdges)  // (slices are multiples of 64 edges)
            {
                const size_t top = std::min(base + (size_t) kEdgeSliceEdges, n_all);
                const uint32_t n = (uint32_t) (top - base);
                while (offsets[k0 + 1] <= base) ++k0;
                std::vector<MultiSeg> segs;
                std::vector<uint8_t> cls, att;
                size_t n_tiles[kClasses] = {}, n_edges[kClasses] = {}, n_att = 0;
                uint32_t shmem[kClasses] = {}, shmem_att = 0;
                EdgeMultiPlan plan{};
                for (size_t k = k0; k < n_envs && offsets[k] < top; ++k)
                {
                    const uint32_t lo = (uint32_t) (std::max(offsets[k], base) - base);
                    const uint32_t hi = (uint32_t) (std::min(offsets[k + 1], top) - base);
                    if (lo >= hi) continue;
                    const EnvLaunch &e = *envs[k];
                    const int c = env_class(e);
                    segs.push_back(MultiSeg{e.d_env, lo, hi, tests_in_lds[k], lds_head(e.host, tests_in_lds[k])});
                    cls.push_back((uint8_t) c);
                    att.push_back(e.host.n_attach > 0);
                    n_tiles[c] += (hi - 1u) / 32u - lo / 32u + 1u;
                    n_edges[c] += hi - lo;
                    plan.m[c] += 1u;
                    shmem[c] = std::max(shmem[c], bytes[k]);
                    if (e.host.n_attach > 0)
                    {
                        n_att += (hi - 1u) / chunk - lo / chunk + 1u;
                        shmem_att = std::max(shmem_att, bytes[k]);
                    }
                }
                size_t at0[kClasses], total0 = 0;
                uint32_t m_all = 0;
                for (int c = 0; c < kClasses; ++c)
                {
                    at0[c] = total0, total0 += n_tiles[c];
                    plan.at[c] = m_all, m_all += plan.m[c];
                    plan.grid[c] = (uint32_t) later_grid(n_edges[c]);  // what launch_rake_tasks would take for the class's edges; the tiles fill it
                }
                const MultiTableLayout table(segs.size(), total0);
                const size_t o_entries = table.bytes;
                const size_t o_att = o_entries + (((size_t) m_all * sizeof(uint32_t) + 7u) & ~size_t{7});
                const size_t host_bytes = o_att + n_att * sizeof(MultiTile);
                const size_t o_starts = (host_bytes + 15u) & ~size_t{15};
                const size_t o_chunk = o_starts + ((((size_t) m_all + kClasses) * sizeof(uint32_t) + 15u) & ~size_t{15});
                MultiTableLease lease;
                if (int rc = lease.acquire(stream, o_chunk + kClasses * sizeof(uint32_t)); rc != VMV_OK) return rc;
                char *h = static_cast<char *>(lease.host);
                std::memcpy(h, segs.data(), segs.size() * sizeof(MultiSeg));
                MultiTile *tiles = table.tiles(h), *att_tiles = reinterpret_cast<MultiTile *>(h + o_att);
                uint32_t *entries = reinterpret_cast<uint32_t *>(h + o_entries);
                size_t fill[kClasses], fill_m[kClasses], fill_att = 0;
                for (int c = 0; c < kClasses; ++c) fill[c] = at0[c], fill_m[c] = plan.at[c];
                for (uint32_t s = 0; s < (uint32_t) segs.size(); ++s)
                {
                    const uint32_t lo = segs[s].lo, hi = segs[s].hi;
                    for (uint32_t w = lo / 32u; w <= (hi - 1u) / 32u; ++w) tiles[fill[cls[s]]++] = MultiTile{s, w};
                    entries[fill_m[cls[s]]++] = s;
                    if (att[s])
                        for (uint32_t c0 = lo / chunk; c0 <= (hi - 1u) / chunk; ++c0) att_tiles[fill_att++] = MultiTile{s, c0 * (chunk / 32u)};
                }
                char *dv = static_cast<char *>(lease.dev);
                const MultiSeg *d_segs = table.segs(dv);
                const MultiTile *d_tiles = table.tiles(dv);
                const MultiTile *d_att = reinterpret_cast<const MultiTile *>(dv + o_att);
                const uint32_t *d_entries = reinterpret_cast<const uint32_t *>(dv + o_entries);
                uint32_t *d_starts = reinterpret_cast<uint32_t *>(dv + o_starts), *d_chunk = reinterpret_cast<uint32_t *>(dv + o_chunk);
                EdgeScratchLease scratch;  // (after the tables: the two pools are always taken in this order)
                if (int rc = scratch.acquire(stream, n); rc != VMV_OK) return rc;
                const EdgeScratch &S = scratch.s;
                const float *a = d_a + base * R::kDim, *b = d_b + base * R::kDim;
                uint64_t *words = d_bits + base / 64;
                uint8_t *bits8 = reinterpret_cast<uint8_t *>(words);
                VMV_HIP_TU(hipMemsetAsync(words, 0, (n + 63u) / 64u * sizeof(uint64_t), stream));
                if (int rc = lease.upload(stream, host_bytes); rc != VMV_OK) return rc;
                for (int c = 0; c < kClasses; ++c)
                    if (n_tiles[c] > 0)
                        for (const auto kernel : {kernels[0][c], kernels[1][c]})
                            VMV_HIP_TU(allow_lds(kernel, shmem[c]));
                for (int c = 0; c < kClasses; ++c)  // pass 0: rake 0 of every edge
                    if (n_tiles[c] > 0)
                        hipLaunchKernelGGL(kernels[0][c], dim3((uint32_t) n_tiles[c]), dim3(kBlock), shmem[c], stream, d_segs,
                                           d_tiles + at0[c], (const uint32_t *) nullptr, 0u, (const uint32_t *) nullptr,
                                           (const uint32_t *) nullptr, a, b, n, bits8, S.steps, (const uint32_t *) nullptr,
                                           (const uint32_t *) nullptr);
                hipLaunchKernelGGL(rake_tasks_self_kernel, dim3(grid_for(n, kTasksPerBlock)), dim3(kBlock), 0, stream, a, b, n, bits8,
                                   (const uint32_t *) nullptr, (const uint32_t *) nullptr, 0u, 1u);
                VMV_HIP_TU(hipGetLastError());
                if (int rc = launch_edge_pass_scan(S, words, n, 1u, 0xffffffffu, 0u, stream); rc != VMV_OK) return rc;
                if (int rc = launch_edge_multi_tiles(S, d_segs, d_entries, plan, n, d_starts, d_chunk, stream); rc != VMV_OK)
                    return rc;
                for (int c = 0; c < kClasses; ++c)  // the later pass: rakes 1 and up of the edges still valid
                    if (plan.m[c] > 0)
                        hipLaunchKernelGGL(kernels[1][c], dim3(plan.grid[c] + plan.m[c]), dim3(kBlock), shmem[c], stream, d_segs,
                                           (const MultiTile *) nullptr, d_entries + plan.at[c], plan.m[c],
                                           (const uint32_t *) (d_starts + plan.at[c] + c), (const uint32_t *) (d_chunk + c), a, b,
                                           n, bits8, (uint32_t *) nullptr, (const uint32_t *) S.excl, (const uint32_t *) S.total);
                hipLaunchKernelGGL(rake_tasks_self_kernel, dim3(later_grid(n)), dim3(kBlock), 0, stream, a, b, n, bits8,
                                   (const uint32_t *) S.excl, (const uint32_t *) S.total, 1u, 0u);
                VMV_HIP_TU(hipGetLastError());
                if (n_att > 0)  // the attachment part continues the edges still valid
                {
                    VMV_HIP_TU(allow_lds(validate_motion_attach_multi_kernel, shmem_att));
                    hipLaunchKernelGGL(validate_motion_attach_multi_kernel, dim3((uint32_t) n_att), dim3(kBlock), shmem_att, stream,
                                       d_segs, d_att, a, b, n, reinterpret_cast<uint32_t *>(words), chunk);
                    VMV_HIP_TU(hipGetLastError());
                }
            }
            return VMV_OK;
        }

        int launch_prepare(const EnvLaunch &env, EnvDev *d_env)
        {
            if (R::kNStaticLinks == 0) return VMV_OK;  // static_hit stays 0
            uint32_t tests_in_lds, shmem;
            if (int rc = plan_lds(env, tests_in_lds, shmem); rc != VMV_OK) return rc;
            VMV_HIP_TU(allow_lds(static_links_kernel, shmem));
            hipLaunchKernelGGL(static_links_kernel, dim3(1), dim3(kBlock), shmem, nullptr, d_env, tests_in_lds);
            VMV_HIP_TU(hipGetLastError());
            VMV_HIP_TU(hipDeviceSynchronize());
            return VMV_OK;
        }

        int launch_prepare_multi(const EnvLaunch *const *envs, EnvDev *const *d_envs, size_t n_envs, int *status)
        {
            for (size_t k = 0; k < n_envs; ++k) status[k] = VMV_OK;
            if (R::kNStaticLinks == 0 || n_envs == 0) return VMV_OK;  // static_hit stays 0
            std::vector<StaticJob> jobs;
            jobs.reserve(n_envs);
            uint32_t shmem_max = 0;
            for (size_t k = 0; k < n_envs; ++k)
            {
                uint32_t tests_in_lds, shmem;
                if ((status[k] = plan_lds(*envs[k], tests_in_lds, shmem)) != VMV_OK) continue;
                jobs.push_back(StaticJob{d_envs[k], tests_in_lds});
                shmem_max = shmem > shmem_max ? shmem : shmem_max;
            }
            if (jobs.empty()) return VMV_OK;
            StaticJob *d_jobs = nullptr;
            VMV_HIP_TU(hipMalloc((void **) &d_jobs, jobs.size() * sizeof(StaticJob)));
            hipError_t e = hipMemcpy(d_jobs, jobs.data(), jobs.size() * sizeof(StaticJob), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = allow_lds(static_links_multi_kernel, shmem_max);
            constexpr size_t kMaxGrid = size_t{1} << 30;
            for (size_t j0 = 0; e == hipSuccess && j0 < jobs.size(); j0 += kMaxGrid)
            {
                const size_t m = jobs.size() - j0 < kMaxGrid ? jobs.size() - j0 : kMaxGrid;
                hipLaunchKernelGGL(static_links_multi_kernel, dim3((uint32_t) m), dim3(kBlock), shmem_max, nullptr, d_jobs + j0);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            (void) hipFree(d_jobs);
            if (e != hipSuccess) return hip_status(e, "static_links_multi_kernel");
            return VMV_OK;
        }

        // d_spheres: [n][kNSpheres][4] from launch_fk; d_env_words: [n][kNSpheres][kReportWords + 1]; d_pair_words:
        // [n][pair_words] zeroed by the caller
        int launch_contacts(const EnvLaunch &env, const float *d_spheres, size_t n, uint32_t *d_env_words,
                            uint32_t *d_pair_words, hipStream_t stream)
        {
            uint32_t report_words = 0;
            for (uint32_t c : {env.host.n_sphere, env.host.n_capsule, env.host.n_zcapsule, env.host.n_cuboid, env.host.n_zcuboid})
                report_words += (c + 31u) / 32u;
            if (report_words > (uint32_t) kReportWords) return VMV_ERR_CAPACITY;  // more than the report's word layout holds
            uint32_t tests_in_lds, shmem;
            if (int rc = plan_lds(env, tests_in_lds, shmem); rc != VMV_OK) return rc;
            VMV_HIP_TU(allow_lds(contacts_env_kernel, shmem));
            const size_t items = n * (size_t) R::kNSpheres;
            hipLaunchKernelGGL(contacts_env_kernel, dim3(grid_for(items, kBlock)), dim3(kBlock), shmem, stream, env.d_env,
                               tests_in_lds, reinterpret_cast<const float4 *>(d_spheres), items, d_env_words);
            VMV_HIP_TU(hipGetLastError());
            if (R::kNSelfPairs == 0) return VMV_OK;
            return launch_flat(contacts_self_kernel, grid_for(n * (size_t) R::kNSelfPairs, kBlock), kBlock, stream,
                               reinterpret_cast<const float4 *>(d_spheres), n, d_pair_words, (uint32_t) ((R::kNSelfPairs + 31) / 32));
        }

        // vmv_self_screen_flags: n below 2^31
        int launch_self_screen_flags(const float *d_q, size_t n, int mode, uint64_t *d_words, hipStream_t stream)
        {
            const auto kernel = mode == 0 ? self_screen_flags_kernel<true> : self_screen_flags_kernel<false>;
            return launch_flat(kernel, (n + kBlock - 1) / kBlock, kBlock, stream, d_q, (uint32_t) n, d_words);
        }

        int launch_eefk(const float *d_q, size_t n, float *d_out, hipStream_t stream)
        {
            return launch_flat(eefk_batch_kernel, (n + kBlock - 1) / kBlock, kBlock, stream, d_q, n, d_out);
        }

        int launch_fk(const float *d_q, size_t n, float *d_out, hipStream_t stream)
        {
            return launch_flat(fk_batch_kernel, (n + kBlock - 1) / kBlock, kBlock, stream, d_q, n, reinterpret_cast<float4 *>(d_out));
        }

        constexpr size_t kClrSlice = (size_t{1} << 20) * kClrTile;  // one workgroup per tile, 2^20 workgroups per launch

        // LDS of the clearance kernels: the staged environment (no point-cloud planes: such environments are refused, so
        // the head is lds_head(D, 0)), then the tile's slab and partial rows.
        // env == nullptr: the self clearance alone (d_out[i][0] = +inf); d_witness may be nullptr
        int launch_clearance(const EnvLaunch *env, const float *d_q, size_t n, float *d_out, uint32_t *d_witness,
                             hipStream_t stream)
        {
            const uint32_t head = env ? lds_head(env->host, 0) : 0u;
            const uint32_t shmem = (head + kClrTailFloats) * (uint32_t) sizeof(float);
            if (shmem > kMaxLdsBytes) return VMV_ERR_CAPACITY;
            VMV_HIP_TU(allow_lds(clearance_kernel<>, shmem));
            for_slices(n, kClrSlice, [&](size_t lo, uint32_t m)
                       {
                           hipLaunchKernelGGL(clearance_kernel<>, dim3((m + kClrTile - 1u) / kClrTile), dim3(kBlock), shmem, stream,
                                              env ? env->d_env : (const EnvDev *) nullptr, head, d_q + lo * R::kDim, m, d_out + 2 * lo,
                                              d_witness ? d_witness + 4 * lo : (uint32_t *) nullptr);
                       });
            VMV_HIP_TU(hipGetLastError());
            return VMV_OK;
        }

        // vmv_clearance_grad_batch: the clearance launch above as it is, then the gradient kernel on the same stream, which
        // reads the witness that launch wrote (d_witness is never nullptr here: the API lends scratch)
        int launch_clearance_grad(const EnvLaunch *env, const float *d_q, size_t n, float *d_out, float *d_grad,
                                  uint32_t *d_witness, hipStream_t stream)
        {
            if (int rc = launch_clearance(env, d_q, n, d_out, d_witness, stream); rc != VMV_OK) return rc;
            for_slices(n, kClrSlice, [&](size_t lo, uint32_t m)  // (the clearance launcher's slices)
                       {
                           hipLaunchKernelGGL(clearance_grad_kernel<>, dim3((m + kGradBlock - 1u) / kGradBlock), dim3(kGradBlock), 0,
                                              stream, env ? env->d_env : (const EnvDev *) nullptr, d_q + lo * R::kDim, m,
                                              d_witness + 4 * lo, d_grad + 2 * lo * R::kDim);
                       });
            VMV_HIP_TU(hipGetLastError());
            return VMV_OK;
        }

        // vmv_clearance_batch_multi: one launch, one workgroup per tile of kClrTile configurations of one segment.
        // Table: [segments | tiles].  d_grad != nullptr (vmv_clearance_grad_batch_multi): the gradient kernel follows, on
        // the same table.
        int launch_clearance_multi(const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                                   float *d_out, float *d_grad, uint32_t *d_witness, hipStream_t stream)
        {
            constexpr size_t kMaxGrid = size_t{1} << 20;  // workgroups per launch
            if (offsets[n_envs] == 0) return VMV_OK;
            std::vector<MultiSeg> segs(n_envs);
            size_t n_tiles = 0;
            uint32_t shmem = 0;
            for (size_t k = 0; k < n_envs; ++k)
            {
                const uint32_t head = lds_head(envs[k]->host, 0);
                segs[k] = MultiSeg{envs[k]->d_env, (uint32_t) offsets[k], (uint32_t) offsets[k + 1], 0u, head};
                if (offsets[k] == offsets[k + 1]) continue;
                n_tiles += (offsets[k + 1] - offsets[k] + kClrTile - 1) / kClrTile;
                shmem = std::max(shmem, (head + kClrTailFloats) * (uint32_t) sizeof(float));
            }
            if (shmem > kMaxLdsBytes) return VMV_ERR_CAPACITY;
            const MultiTableLayout table(n_envs, n_tiles);
            MultiTableLease lease;
            if (int rc = lease.acquire(stream, table.bytes); rc != VMV_OK) return rc;
            std::memcpy(lease.host, segs.data(), n_envs * sizeof(MultiSeg));
            MultiTile *tiles = table.tiles(lease.host);
            size_t fill = 0;
            for (size_t k = 0; k < n_envs; ++k)
                for (size_t first = offsets[k]; first < offsets[k + 1]; first += kClrTile)
                    tiles[fill++] = MultiTile{(uint32_t) k, (uint32_t) first};
            if (int rc = lease.upload(stream, table.bytes); rc != VMV_OK) return rc;
            const MultiSeg *d_segs = table.segs(lease.dev);
            const MultiTile *d_tiles = table.tiles(lease.dev);
            VMV_HIP_TU(allow_lds(clearance_multi_kernel<>, shmem));
            for (size_t t0 = 0; t0 < n_tiles; t0 += kMaxGrid)
                hipLaunchKernelGGL(clearance_multi_kernel<>, dim3((uint32_t) std::min(n_tiles - t0, kMaxGrid)), dim3(kBlock), shmem,
                                   stream, d_segs, d_tiles + t0, d_q, d_out, d_witness);
            constexpr size_t kGradTiles = kMaxGrid * (kGradBlock / kClrTile);  // tiles per launch of the gradient kernel
            for (size_t t0 = 0; d_grad && t0 < n_tiles; t0 += kGradTiles)
            {
                const uint32_t m = (uint32_t) std::min(n_tiles - t0, kGradTiles);
                hipLaunchKernelGGL(clearance_grad_multi_kernel<>, dim3((m + kGradBlock / kClrTile - 1u) / (kGradBlock / kClrTile)),
                                   dim3(kGradBlock), 0, stream, d_segs, d_tiles + t0, m, d_q, d_witness, d_grad);
            }
            VMV_HIP_TU(hipGetLastError());
            return VMV_OK;
        }

        // vmv_eefk_jacobian_batch: d_frames may be nullptr
        int launch_eefk_jacobian(const float *d_q, size_t n, float *d_frames, float *d_jac, hipStream_t stream)
        {
            for_slices(n, (size_t{1} << 20) * kIkBlock, [&](size_t lo, uint32_t m)  // 2^20 workgroups per launch
                       {
                           hipLaunchKernelGGL(eefk_jacobian_kernel<>, dim3((m + kIkBlock - 1u) / kIkBlock), dim3(kIkBlock), 0, stream,
                                              d_q + lo * R::kDim, m, d_frames ? d_frames + 16 * lo : (float *) nullptr,
                                              d_jac + 6 * lo * R::kDim);
                       });
            VMV_HIP_TU(hipGetLastError());
            return VMV_OK;
        }

        // The launchers below: workgroups of one wave (kIkBlock threads), one lane or one wave per item; the counts are
        // below 2^31 (the API checks).
        constexpr size_t lane_grid(size_t n) { return (n + kIkBlock - 1u) / kIkBlock; }  // one lane per item

        // vmv_ik_batch: n = n_targets * n_seeds lanes; d_err may be nullptr
        int launch_ik(const IkParams &P, const float *d_targets, const float *d_seeds, size_t n, float *d_q, float *d_err,
                      uint32_t *d_status, hipStream_t stream)
        {
            return launch_flat(ik_kernel<>, lane_grid(n), kIkBlock, stream, P, d_targets, d_seeds, (uint32_t) n, d_q, d_err, d_status);
        }

        // vmv_cartesian_multi: n lanes
        int launch_cartesian(const CartParams &P, const CartLine *d_lines, const float *d_starts, size_t n, float *d_points,
                             CartResult *d_results, hipStream_t stream)
        {
            return launch_flat(cartesian_track_kernel<>, lane_grid(n), kIkBlock, stream, P, d_lines, d_starts, (uint32_t) n, d_points,
                               d_results);
        }

        // vmv_constraint_*_batch: n lanes / edges; d_res may be nullptr
        int launch_constraint_project(const ConstraintParams &P, const ConstraintDev *d_cons, const float *d_q, size_t n, float *d_q_out,
                                      float *d_res, uint32_t *d_status, hipStream_t stream)
        {
            return launch_flat(constraint_project_kernel<>, lane_grid(n), kIkBlock, stream, P, d_cons, d_q, (uint32_t) n, d_q_out, d_res,
                               d_status);
        }
        int launch_constraint_check(const ConstraintParams &P, const ConstraintDev *d_cons, const float *d_q, size_t n, uint64_t *d_bits,
                                    float *d_res, hipStream_t stream)
        {
            return launch_flat(constraint_check_kernel<>, lane_grid(n), kIkBlock, stream, P, d_cons, d_q, (uint32_t) n, d_bits, d_res);
        }
        int launch_constraint_edges(const ConstraintParams &P, const ConstraintDev *d_cons, const float *d_a, const float *d_b, size_t n,
                                    uint8_t *d_ok, hipStream_t stream)
        {
            return launch_flat(constraint_edge_kernel<>, n, kIkBlock, stream, P, d_cons, d_a, d_b, (uint32_t) n, d_ok);
        }
        // the constraint's part of a planner round: na active slots (vmv_rrtc_multi_constrained)
        int launch_constraint_round(const ConstraintParams &P, const ConstraintDev *d_cons, const uint32_t *d_active, const float *d_q_start,
                                    float *d_q_goal, const uint64_t *d_pending, float *d_pool, float stretch, uint8_t *d_c_ok,
                                    uint32_t *d_refused, uint32_t na, hipStream_t stream)
        {
            return launch_flat(constraint_round_kernel<>, na, kIkBlock, stream, P, d_cons, d_active, d_q_start, d_q_goal, d_pending, d_pool,
                               stretch, d_c_ok, d_refused);
        }
        // the constraint's part of a simplifier round: na active paths of w slots each (vmv_simplify_multi_constrained)
        int launch_simplify_band_round(const ConstraintParams &P, const ConstraintDev *d_cons, const uint32_t *d_active, float *d_q_start,
                                       float *d_q_goal, const uint8_t *d_pending, float *d_proj, uint32_t proj_stride, uint8_t *d_c_ok,
                                       uint32_t na, uint32_t w, hipStream_t stream)
        {
            return launch_flat(simplify_band_round_kernel<>, na * w, kIkBlock, stream, P, d_cons, d_active, d_q_start, d_q_goal, d_pending,
                               d_proj, proj_stride, w, d_c_ok);
        }
        // the constraint's part of an optimiser iteration: `rows` packed waypoints (vmv_optimize_multi_constrained)
        int launch_opt_band(const ConstraintParams &P, const ConstraintDev *d_cons, const OptBand &B, uint32_t rows, uint32_t cur,
                            uint32_t initial, uint32_t edges, uint32_t may_end, float min_change, hipStream_t stream)
        {
            return launch_flat(opt_band_kernel<>, lane_grid(rows), kIkBlock, stream, P, d_cons, B, rows, cur, initial, edges, may_end,
                               min_change);
        }
        // the band test of a retiming round: `rows` packed sample rows of n_paths listed paths (vmv_retime_multi_constrained)
        int launch_retime_band(const ConstraintParams &P, const ConstraintDev *d_cons, const uint32_t *d_rec_of, const uint32_t *d_sample_lo,
                               uint32_t n_paths, const float *d_pos, uint32_t rows, uint8_t *d_ok, hipStream_t stream)
        {
            return launch_flat(retime_band_kernel<>, lane_grid(rows), kIkBlock, stream, P, d_cons, d_rec_of, d_sample_lo, n_paths, d_pos,
                               rows, d_ok);
        }

        // every member by its name: a launcher added to RobotLaunchers is added here, wherever it stands in the struct
        constexpr RobotLaunchers make_launchers()
        {
            RobotLaunchers L{};
            L.validate = launch_validate;
            L.validate_multi = launch_validate_multi;
            L.validate_motion = launch_validate_motion;
            L.validate_motion_multi = launch_validate_motion_multi;
            L.fk = launch_fk;
            L.prepare = launch_prepare;
            L.prepare_multi = launch_prepare_multi;
            L.eefk = launch_eefk;
            L.contacts = launch_contacts;
            L.n_self_pairs = R::kNSelfPairs;
            L.clearance = launch_clearance;
            L.clearance_multi = [](const EnvLaunch *const *envs, const size_t *offsets, size_t n_envs, const float *d_q, float *d_out,
                                   uint32_t *d_witness, hipStream_t stream)
            { return launch_clearance_multi(envs, offsets, n_envs, d_q, d_out, nullptr, d_witness, stream); };
            L.clearance_grad = launch_clearance_grad;
            L.clearance_grad_multi = launch_clearance_multi;
            L.eefk_jacobian = launch_eefk_jacobian;
            L.ik = launch_ik;
            L.cartesian = launch_cartesian;
            L.constraint_project = launch_constraint_project;
            L.constraint_check = launch_constraint_check;
            L.constraint_edges = launch_constraint_edges;
            L.constraint_round = launch_constraint_round;
            L.simplify_band_round = launch_simplify_band_round;
            L.opt_band = launch_opt_band;
            L.retime_band = launch_retime_band;
            L.self_screen_flags = launch_self_screen_flags;
            return L;
        }
    }  // namespace
