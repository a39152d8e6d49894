/*
 * vamp_mvt_amd.h — C ABI of the MI355X-native motion-validation hot path.
 *
 * Drop-in boundary for one path of chingchennn/vamp_mvt: configuration-rake forward kinematics + sphere
 * collision check (+ CAPT point-cloud query).  The reference exposes this path only through its nanobind
 * module `vamp._core` (no C ABI exists there); each entry point below names the reference interface it
 * replaces (file:line under /root/reference/src/impl/vamp/).  INTEGRATION.md shows the binding a maintainer
 * would add on the reference side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, opaque handles, `int` status (0 = VMV_OK); nothing throws/aborts.
 *   - `d_*` pointers are DEVICE pointers (HBM) on the current HIP device; `*_host` variants take host
 *     buffers and do the H2D/D2H copies themselves.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - configurations are fp32, row-major [n][dimension], joint values in radians / metres (not normalised).
 *   - validity results are packed bitmasks, little-endian within 64-bit words: bit (i % 64) of word (i / 64)
 *     is 1 iff configuration/edge i is VALID (collision free).  d_bits must hold ceil(n / 64) words.
 *   - an environment is immutable after vmv_env_finalize() and may then be used from any thread/stream.
 *   - there is no CPU fallback: every compute entry point fails with VMV_ERR_NO_DEVICE without a GPU.
 *   - non-finite input is DEFINED: a configuration with a NaN or +-inf joint is INVALID (bit 0), an edge with such an
 *     endpoint is INVALID; nothing is evaluated for it.  (The reference has no rule: its sign-bit predicates read the
 *     sign of a propagated NaN, vector/interface.hh:257-277 — an artefact of the instruction set.)  vmv_fk_batch /
 *     vmv_eefk_batch return NaN spheres / frames for such a configuration.
 *   - bits of the last word at or beyond n are written as 0; the entry points that AND into existing words
 *     (vmv_validate_batch_self) ignore and clear them.
 */
#ifndef VAMP_MVT_AMD_H
#define VAMP_MVT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    VMV_OK = 0,
    VMV_ERR_INVALID_ARGUMENT = 1,
    VMV_ERR_NO_DEVICE = 2,
    VMV_ERR_HIP = 3,
    VMV_ERR_CAPACITY = 4,      /* environment does not fit the on-chip staging budget */
    VMV_ERR_NOT_FINALIZED = 5,
    VMV_ERR_UNKNOWN_ROBOT = 6,
    VMV_ERR_FINALIZED = 7      /* mutation after finalize */
};

const char *vmv_status_string(int status);
int vmv_abi_version(void);
/* last HIP error text of the calling thread (empty if none) */
const char *vmv_last_error(void);

/* ---- devices ----------------------------------------------------------------------------------------- */
int vmv_device_count(int *count);
int vmv_set_device(int device);
int vmv_get_device(int *device);

/* ---- robots (replaces the per-robot submodule constants, bindings/robot_helper.hh:326-360) ------------ */
int vmv_num_robots(void);
const char *vmv_robot_name(int robot);
int vmv_robot_id(const char *name);           /* -1 if unknown ("panda", "ur5", "fetch", "baxter") */
int vmv_robot_dimension(int robot);           /* Robot::dimension */
int vmv_robot_n_spheres(int robot);           /* Robot::n_spheres */
int vmv_robot_resolution(int robot);          /* Robot::resolution */
int vmv_robot_min_max_radii(int robot, float *min_radius, float *max_radius);
/* lower[d], span[d], descale[d]: Robot::s_a, s_m, d_m (robots/panda.hh:50-75) */
int vmv_robot_bounds(int robot, float *lower, float *span, float *descale);
const char *vmv_robot_joint_name(int robot, int joint);
const char *vmv_robot_end_effector(int robot);

/* ---- point-cloud filters (replaces vamp.filter_pointcloud, bindings/environment.cc:183-239) ------------ */
/* filter_type 0 = "scdf" (collision/filter.hh:175-275; uses min_dist, max_range, cull), 1 = "centervox"
 * (collision/filter_centervox.hh:288-313; uses voxel_size, max_range).  points / out: host pointers, [n][3] fp32; the
 * kept points come back in the reference's order.  out may be NULL (count only); VMV_ERR_CAPACITY if out is too small
 * or where the reference throws "Voxel pool exhausted".  nanoseconds: wall time including transfers (what the
 * reference's binding reports), device_nanoseconds: HIP-event time of the device work alone; both may be NULL. */
int vmv_filter_pointcloud(const float *points_xyz, size_t n, float min_dist, float max_range, float voxel_size,
                          const float *origin3, const float *workspace_min3, const float *workspace_max3, int cull,
                          int filter_type, float *out_xyz, size_t capacity, size_t *n_out, uint64_t *nanoseconds,
                          uint64_t *device_nanoseconds);

/* ---- environment (replaces vamp.Environment, bindings/environment.cc:111-163) -------------------------- */
typedef struct vmv_env vmv_env;

int vmv_env_create(vmv_env **out);
int vmv_env_destroy(vmv_env *env);
/* Environment.add_sphere(Sphere(center, r)) — environment.cc:113-119, collision/shapes.hh:226-239 */
int vmv_env_add_sphere(vmv_env *env, float x, float y, float z, float r);
/* Environment.add_cuboid — environment.cc:120-133.  15 floats: centre xyz | axis_1 xyz | axis_2 xyz |
 * axis_3 xyz | half extents 1..3 (collision/shapes.hh:32-49).  Filed as z-aligned iff axis_3_z == 1. */
int vmv_env_add_cuboid(vmv_env *env, const float *params15);
/* Environment.add_capsule — environment.cc:134-147.  8 floats: x1 y1 z1 | xv yv zv | r | rdv
 * (collision/shapes.hh:128-143).  Filed as z-aligned iff xv == 0 and yv == 0.
 * min_distance is collision/shapes.hh:165-189, with one rule where that is not a number: if the origin lies on the
 * capsule's axis the reference divides 0 by 0; the true distance, 0, is stored instead, and so is any min_distance that
 * is still not finite (a zero-length capsule with rdv = inf).  Such an entry sorts first and never triggers the sorted
 * early break (for any sphere with max_extent > 0).  This reproduces the reference wherever its own sorted order is
 * defined (the capsule inserted first); where it is not, the environment answers the OR of the reference's predicates
 * over every capsule. */
int vmv_env_add_capsule(vmv_env *env, const float *params8);
/* make_heightfield(center, scaling, dimensions, data) + Environment.add_heightfield — collision/factory.hh:363-423,
 * bindings/environment.cc:100,149-151, collision/shapes.hh:250-312.  data: host pointer, row-major [yd][xd] fp32;
 * scale3 as given to make_heightfield (the shape stores the reciprocals).  At most 4 per environment.
 * Cell index (collision/sphere_heightfield.hh:20-26): clamped to [0, xd] x [0, yd], one past the image on both axes.
 * xs == xd in any row but the last reads the first cell of the next row, as in the reference; xs == xd in the last
 * row and ys == yd are past the reference's buffer (undefined there) and read the last pixel here. */
int vmv_env_add_heightfield(vmv_env *env, const float *center3, const float *scale3, size_t xd, size_t yd,
                            const float *data);
int vmv_env_heightfield_count(const vmv_env *env, size_t *count);
/* Environment.attach(Attachment) / detach — bindings/environment.cc:178-181; Attachment(tf) + add_sphere(s)
 * (:241-259), collision/attachments.hh.  tf: 4 x 4 row-major, the attachment's frame relative to the end-effector
 * frame; spheres: [n][4] = x y z r in that frame, n <= 256.  With an attachment (and n > 0) every validate call is
 * Robot::fkcc_attach (planning/validate.hh:43,58): plain fkcc, then the posed spheres against the environment and
 * against the links of the reference's "Attachment vs. <link>" blocks. */
int vmv_env_attach(vmv_env *env, const float *tf_rowmajor_4x4, const float *spheres_xyzr, size_t n);
int vmv_env_detach(vmv_env *env);
/* Environment.add_capt_pointcloud(points, r_min, r_max, r_point) -> build ns — environment.cc:152-163,
 * collision/capt.hh:296-369.  points: host pointer, [n][3] fp32. */
int vmv_env_add_capt_pointcloud(vmv_env *env, const float *points_xyz, size_t n, float r_min, float r_max,
                                float r_point, uint64_t *build_nanoseconds);
/* The same point cloud structure built on the GPU: identical arrays, level-synchronous build
 * (csrc/vmv_capt_gpu.hip).  build_nanoseconds: wall time including the upload of the points and the download of the
 * arrays; device_nanoseconds: HIP-event time of the build on the device alone.  Either may be NULL. */
int vmv_env_add_capt_pointcloud_gpu(vmv_env *env, const float *points_xyz, size_t n, float r_min, float r_max,
                                    float r_point, uint64_t *build_nanoseconds, uint64_t *device_nanoseconds);
/* Environment.add_mvt_pointcloud(points, r_min, r_max, workspace_aabb_min, workspace_aabb_max, r_point) -> build ns
 * — environment.cc:164-177, collision/mvt.hh:147-170 (the fork's Multi-level Voxel Table).  Where the reference
 * throws inside its noexcept constructor (a pool it sized up front runs out: mvt.hh:66-70, 634-648), this returns
 * VMV_ERR_CAPACITY and `*reason` (may be NULL) = 1 voxel capacity, 2 point pool (> 10 % of the voxels occupied),
 * 3 z-table pool (> 50 % of the (x, y) columns occupied), 4 degenerate grid, 5 grid too large for the dense table. */
int vmv_env_add_mvt_pointcloud(vmv_env *env, const float *points_xyz, size_t n, float r_min, float r_max,
                               const float *workspace_min3, const float *workspace_max3, float r_point,
                               uint64_t *build_nanoseconds, int *reason);
/* Sorts every primitive list by min_distance (collision/environment.hh:46-72) and uploads the environment to
 * the current device.  The reference re-sorts on every add and converts per call (robot_helper.hh:266). */
int vmv_env_finalize(vmv_env *env);
/* counts[6]: spheres, capsules, z_capsules, cuboids, z_cuboids, capt point clouds; vmv_env_mvt_count: MVT clouds */
int vmv_env_counts(const vmv_env *env, size_t *counts6);
int vmv_env_mvt_count(const vmv_env *env, size_t *count);
/* MVT cloud `index`: grid_width, per-voxel capacity, occupied voxels, inverse scale factor, global box (6 floats) */
int vmv_env_mvt_info(const vmv_env *env, size_t index, uint32_t *grid_width, uint32_t *capacity, uint32_t *n_voxels,
                     float *inverse_scale_factor, float *global_box6);
/* sorted host copies for inspection: spheres [n][5] (x y z r min_distance), cuboids [n][16], capsules [n][9] */
int vmv_env_get_spheres(const vmv_env *env, float *out, size_t capacity, size_t *n);
int vmv_env_get_cuboids(const vmv_env *env, int z_aligned, float *out, size_t capacity, size_t *n);
int vmv_env_get_capsules(const vmv_env *env, int z_aligned, float *out, size_t capacity, size_t *n);
/* CAPT arrays of point cloud `index` (collision/capt.hh:588-623) — sizes first, then copies (NULL = skip) */
int vmv_env_capt_sizes(const vmv_env *env, size_t index, uint32_t *nlog2, uint32_t *n_aff_vectors);
int vmv_env_capt_arrays(const vmv_env *env, size_t index, float *tests, uint32_t *aff_starts, float *aabbs,
                        float *aff_x, float *aff_y, float *aff_z, float *aabb_top6);

/* ---- batched hot path ---------------------------------------------------------------------------------- */
/* <robot>.fk(q) -> list[Sphere] — robot_helper.hh:234-247, Robot::sphere_fk (robots/panda.hh:116-462).
 * d_out: [n][n_spheres][4] = x y z r. */
int vmv_fk_batch(int robot, const float *d_q, size_t n, float *d_out, void *stream);
/* <robot>.eefk(q) -> 4 x 4 — robot_helper.hh:279-282, Robot::eefk.  d_out: [n][16] row-major frames. */
int vmv_eefk_batch(int robot, const float *d_q, size_t n, float *d_out, void *stream);
/* <robot>.validate(q, env) — robot_helper.hh:255-267 -> validate_motion<Robot, 8, 1>(q, q, env)
 * (planning/validate.hh:70-77) -> Robot::fkcc (robots/panda.hh:5226-10262).  One bit per configuration. */
int vmv_validate_batch(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, void *stream);
/* The two halves vmv_validate_batch launches back to back, exposed for per-kernel measurement and for callers that
 * pipeline them: `_env` WRITES the validity words (environment half of fkcc), `_self` ANDs the self-collision half
 * into words already written.  vmv_validate_batch == _env then _self on the same stream. */
int vmv_validate_batch_env(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, void *stream);
int vmv_validate_batch_self(int robot, const float *d_q, size_t n, uint64_t *d_bits, void *stream);
/* Probes of the self-collision kernel's first round ("Gate screen"), for tests and measurement.
 * vmv_self_screen_flags: bit i of d_words (ceil(n / 64) words, every one written, bits at and beyond n zero) = the screen
 * flags configuration i, whatever its validity: mode 0 the exact screen (the gates' own arithmetic), mode 1 the default
 * screen on the hardware's sine and cosine, which flags a superset.  Robots without a screen answer with the exact gates
 * for both modes.  n < 2^31, else VMV_ERR_INVALID_ARGUMENT.
 * vmv_bare_trig_error: over every fp32 value whose bit pattern lies in [lo_bits, hi_bits] (positive, finite) and its
 * negative, out2[0] = max |hardware sine - the reference's sine|, out2[1] = the same for the cosines, as the kernels
 * compute the four.  out2 is a HOST array; the call waits for its kernels. */
int vmv_self_screen_flags(int robot, const float *d_q, size_t n, int mode, uint64_t *d_words, void *stream);
int vmv_bare_trig_error(uint32_t lo_bits, uint32_t hi_bits, float *out2, void *stream);
/* Many environments in one call: configurations [offsets[k], offsets[k+1]) against envs[k]; offsets: host array of
 * n_envs + 1, offsets[0] == 0, non-decreasing, offsets[n_envs] == n.  Bit i of d_bits = configuration i is collision
 * free (flat layout: the same words as concatenating one vmv_validate_batch per environment, and the same bits).  Empty
 * ranges and repeated handles are allowed.  Every environment must be finalized on the current device.
 * Limits: n < 2^31 and n_envs < 2^31 (the kernels count in 32 bits), else VMV_ERR_INVALID_ARGUMENT.
 * Every argument is checked before anything is launched: a call that fails a check launches nothing and writes nothing.
 * The checks that need no device (robot, NULL pointers and handles, offsets, limits, unfinalized environments) come
 * first.  The device entry point does not synchronise with the host: its tables go through pinned host staging and
 * device scratch kept per (device, stream) (freed by vmv_release_staging) and are copied on `stream`.  The launches:
 * one environment kernel per variant class present (each segment runs the variant its environment runs alone), the
 * self-collision kernel once over all n, the attachment kernel over the segments with an attachment. */
int vmv_validate_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                             const float *d_q, uint64_t *d_bits, void *stream);
int vmv_validate_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                  const float *q, uint64_t *bits);
/* validate_motion<Robot, 8, Robot::resolution>(start, goal, env) — planning/validate.hh:24-77, the call every
 * planner makes per edge (rrtc.hh:136-140, prm.hh:59, fcit.hh:238 ...).  One bit per edge.
 * A sequence of kernels on `stream` (rake 0 of every edge, a scan, the remaining rakes of the surviving edges), with 8
 * bytes of internal device scratch per edge kept per (device, stream); batches beyond 2^20 edges run slice by slice.
 * Rake counts are 32-bit: the rakes of one slice must number below 2^32 (edges averaging 4,096 rakes = 512 rad at
 * resolution 64 — far beyond any joint range; the reference's walk of such an edge would not end either). */
int vmv_validate_motion_batch(int robot, const vmv_env *env, const float *d_start, const float *d_goal, size_t n,
                              uint64_t *d_bits, void *stream);
/* Many environments in one call, for edges: edge i = d_start[i] -> d_goal[i], edges [offsets[k], offsets[k+1]) against
 * envs[k].  The contract of vmv_validate_batch_multi, word for word (offsets, limits, checks before the first launch
 * and device-free checks first, environments of another device refused, no host synchronisation, tables and scratch per
 * (device, stream) freed by vmv_release_staging), with the bits of one vmv_validate_motion_batch per environment,
 * concatenated.  The launches per 2^20-edge slice (segments clipped at its ends): the validity words zeroed, rake 0 of
 * the environment half once per variant class present, the self-collision half and the scan once over the slice, the
 * later pass's tiles built on the device from the scan, the remaining rakes of the environment half once per class,
 * those of the self-collision half once, the attachment walk over the segments with an attachment. */
int vmv_validate_motion_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                    const float *d_start, const float *d_goal, uint64_t *d_bits, void *stream);
int vmv_validate_motion_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                         const float *start, const float *goal, uint64_t *bits);

/* Builds the part of each environment that depends on the robot (broad-phase grids, reach certificates, static links)
 * for all of them together, on the device.  After VMV_OK every later call with (envs[k], robot) finds it built; without
 * this call the part is built on the first use of (environment, robot), one environment at a time on the host (the
 * multi-environment validate calls build their not-yet-built environments this way, in one batch).  Both ways give the
 * same part, bit for bit.  Checks before any work, device-free ones first: unknown robot; envs NULL with n_envs > 0 or
 * a NULL handle (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment (VMV_ERR_NOT_FINALIZED); an environment
 * finalized on another device than the current one (VMV_ERR_INVALID_ARGUMENT) — a call that fails a check prepares
 * nothing.  n_envs == 0 is VMV_OK.  Repeated handles are allowed, parts already built are skipped.  Synchronous, like
 * vmv_env_finalize, and thread safe against itself and against first uses on other threads (whoever comes second
 * waits).  A failure is recorded per (environment, robot) and returned by every later use; the call returns the first
 * non-OK status in envs order after preparing the others.  VMV_NO_GRID, VMV_NO_LINK_SKIP, VMV_GRID_CELLS and
 * VMV_GRID_MIN_CELL mean what they mean on first use.  Device memory: one allocation per call, shared by the
 * environments it prepared and freed by vmv_env_destroy of the last of them. */
int vmv_env_prepare_multi(int robot, const vmv_env *const *envs, size_t n_envs);
/* Inspection of the robot part (builds it as a first use would if it is not built yet).  Grid of one class:
 * dims 0,0,0 = this environment runs without a grid; cells = uint32 [dims0][dims1][dims2][words]. */
int vmv_env_grid_info(const vmv_env *env, int robot, int grid_class, uint32_t *dims3, float *origin3, float *inv_cell,
                      uint32_t *words);
int vmv_env_grid_cells(const vmv_env *env, int robot, int grid_class, uint32_t *out, size_t capacity, size_t *n);
int vmv_env_robot_flags(const vmv_env *env, int robot, uint64_t *link_skip, uint32_t *static_hit);

/* <robot>.debug(q, env) — robot_helper.hh:249-253 -> Robot::fkcc_debug: per fine sphere the environment objects it
 * collides with (sphere_environment_get_collisions, collision/validity.hh:161-256: the five sorted primitive lists with
 * their early break, then the heightfields; no point clouds), and the fine sphere pairs of the self-collision groups
 * that overlap (all pairs, no bounding gates).  Host buffers.  env_words: [n][n_spheres][9]; words 0..7 hold 32
 * sorted-list positions each, the lists back to back (vmv_env_report_layout gives each list's first word), word 8 the
 * heightfields.  pair_words: [n][ceil(n_pairs / 32)], bit p = pair p of vmv_robot_self_pairs.  Environments whose
 * lists need more than 8 words: VMV_ERR_CAPACITY. */
int vmv_contacts_batch_host(int robot, const vmv_env *env, const float *q, size_t n, uint32_t *env_words,
                            uint32_t *pair_words);
/* first word of each sorted list in the report: spheres, capsules, z_capsules, cuboids, z_cuboids */
int vmv_env_report_layout(const vmv_env *env, uint32_t *first_word5);
/* the fine pairs the report covers: n_pairs, and (a, b) sphere indices into pairs2 (may be NULL) */
int vmv_robot_self_pairs(int robot, size_t *n_pairs, uint16_t *pairs2);

/* Clearances: how far each configuration is from contact (no counterpart in the reference, whose answers are booleans).
 * Per configuration two fp32 values, d_clearance [n][2]:
 *   [0] env  = min over the robot's fine spheres s (those of vmv_fk_batch) and over every contact c of the environment
 *              of the signed distance between the two surfaces, negative = penetration:
 *                sphere                |c_s - c_p| - (r_s + r_p)
 *                capsule, z-capsule    distance to the segment, minus both radii
 *                cuboid, z-cuboid      distance to the box (0 inside), minus r_s; the z-aligned kind with its first two
 *                                      axes in x, y and +z as the third, as the reference's test reads it
 *                heightfield           the reference's vertical value z - r_s - height, the cell chosen by the fp32
 *                                      arithmetic of its sphere_heightfield test
 *              +inf for an environment without contacts (and for env == NULL);
 *   [1] self = min over the fine self pairs (a, b) of vmv_robot_self_pairs of |c_a - c_b| - (r_a + r_b).
 * The minimum is FLAT: the bounding-sphere gates, reach certificates, candidate words and the sorted early break of the
 * validation kernels prune a boolean and play no part in it.
 * d_witness [n][4] uint32 (may be NULL): env_sphere; env_kind (0 sphere, 1 capsule, 2 z-capsule, 3 cuboid, 4 z-cuboid,
 * 5 heightfield); env_index = the position in that kind's list as vmv_env_get_spheres / _cuboids / _capsules return it
 * after finalize, for heightfields the insertion index; self_pair = index into vmv_robot_self_pairs.  A field with
 * nothing to point at is UINT32_MAX.  Among equal fp32 values the first wins, ordered by sphere index, then kind, then
 * list index; for self pairs the lowest pair index.  So a configuration's values and witness do not depend on the batch
 * size, on its position in the batch, or on which of these calls computed it.
 * Arithmetic: fp32 + - * / sqrt, one rounding per operation (no contraction), on the sphere centres of Robot::sphere_fk,
 * which stay on chip.  A configuration with a non-finite joint gives NaN in both values and UINT32_MAX in all four
 * witness fields.
 * Out of scope: an environment holding a point cloud (CAPT or MVT) - a distance to a cloud needs a nearest-neighbour
 * structure, which neither index is - or an attachment is refused with VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names
 * the kind.  Checks before anything is launched, those that need no device first: unknown robot; NULL d_q / d_clearance
 * (VMV_ERR_INVALID_ARGUMENT); a refused kind; an unfinalized environment (VMV_ERR_NOT_FINALIZED); then the device.
 * env == NULL: the self clearance alone.  The sign agrees with vmv_validate_batch except within rounding of contact, and
 * where the reference's bounding-sphere gate reads another heightfield cell than the fine spheres do. */
int vmv_clearance_batch(int robot, const vmv_env *env, const float *d_q, size_t n, float *d_clearance, uint32_t *d_witness,
                        void *stream);
int vmv_clearance_batch_host(int robot, const vmv_env *env, const float *q, size_t n, float *clearance, uint32_t *witness);
/* Many environments in one call: configurations [offsets[k], offsets[k+1]) against envs[k].  Offsets, limits, the order
 * of the checks (NULL handles named by index, a refused kind named by index, unfinalized environments, environments of
 * another device; n >= 2^31 refused before any array is read), the absence of host synchronisation and the tables per
 * (device, stream) are those of vmv_validate_batch_multi.  Every envs[k] is a handle (no NULL).  The values and the
 * witness are bit for bit those of one vmv_clearance_batch per environment, concatenated.  One launch. */
int vmv_clearance_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs, const float *d_q,
                              float *d_clearance, uint32_t *d_witness, void *stream);
int vmv_clearance_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs, const float *q,
                                   float *clearance, uint32_t *witness);

/* Clearance gradients: the two values and the witness of vmv_clearance_batch, BIT FOR BIT (the call launches that call's
 * kernel unchanged, then a second kernel on the same stream that reads q and the witness), plus d_grad [n][2][dim] fp32:
 * d_grad[i][0] = d env / d q, d_grad[i][1] = d self / d q, both with the WITNESS HELD FIXED - the derivative of the
 * minimum wherever the minimiser is unique, one of its one-sided derivatives elsewhere.
 *   env, witness sphere s against the witness primitive: g_j = n . dc_s/dq_j, n = (c_s - p) / |c_s - p|, p the closest
 *     point of the primitive to c_s by the closest-point arithmetic that produced the value: a sphere's centre; the
 *     clamped point on a capsule's / z-capsule's segment; the clamped point in a cuboid's / z-cuboid's box - a centre
 *     inside the box has the flat value -r_s and the gradient 0; heightfield: the value is z - r - height(cell), the
 *     cell held fixed, so n = (0, 0, 1).  |c_s - p| = 0: gradient 0.
 *   self, witness pair (a, b): g_j = n . (dc_a/dq_j - dc_b/dq_j), n = (c_a - c_b) / |c_a - c_b|; coincident centres: 0.
 *   No witness (the value is +inf; env == NULL for the env half): zeros.  A non-finite joint: NaN in all 2 * dim entries,
 *     beside the NaN values.
 * dc/dq is the forward-mode tangent of the robot's kinematic op tape as written (tools/gen_hip.py: tangent_tape):
 * d(q_j)/dq_j = 1, d sin(q_j) = cos(q_j), d cos(q_j) = -sin(q_j) with the kernels' own sine and cosine, product and sum
 * rules elsewhere (a prismatic joint is no special case), in fp32 without contraction.  A configuration's gradient does
 * not depend on its batch, on its position in it, or on which of these calls computed it; the multi-environment call is
 * bit for bit one call per environment.
 * d_witness may be NULL (the call then uses scratch per (device, stream), released by vmv_release_staging).  Checks,
 * their order and what is refused (point clouds, attachments) are those of vmv_clearance_batch / _multi; a NULL d_grad
 * is VMV_ERR_INVALID_ARGUMENT like a NULL d_q or d_clearance.  A refused call writes nothing; n == 0 needs no device. */
int vmv_clearance_grad_batch(int robot, const vmv_env *env, const float *d_q, size_t n, float *d_clearance /* [n][2] */,
                             float *d_grad /* [n][2][dim] */, uint32_t *d_witness /* [n][4], may be NULL */, void *stream);
int vmv_clearance_grad_batch_host(int robot, const vmv_env *env, const float *q, size_t n, float *clearance, float *grad,
                                  uint32_t *witness);
/* One clearance launch plus one gradient launch, however many environments. */
int vmv_clearance_grad_batch_multi(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                   const float *d_q, float *d_clearance, float *d_grad, uint32_t *d_witness, void *stream);
int vmv_clearance_grad_batch_multi_host(int robot, const vmv_env *const *envs, const size_t *offsets, size_t n_envs,
                                        const float *q, float *clearance, float *grad, uint32_t *witness);

/* ---- end-effector Jacobian and inverse kinematics (no counterpart in the reference) ------------------ */
/* The end-effector frame and its geometric Jacobian in the world frame: d_frames [n][16] (may be NULL) are bit for bit
 * those of vmv_eefk_batch; d_jac [n][6][dim] fp32: rows 0-2 are dt/dq_j, rows 3-5 the angular velocity omega_j: with
 * A = (dR/dq_j) R^T, omega = 1/2 (A21 - A12, A02 - A20, A10 - A01), every 3-term product of A as ((a0 b0 + a1 b1) + a2 b2).
 * dt/dq and dR/dq are the forward-mode tangents of the end-effector op tape as written (tools/gen_hip.py: ee_tangent_tape;
 * the rules of vmv_clearance_grad_batch), fp32 without contraction; a joint that does not move the end effector has a
 * zero column.  A configuration with a non-finite joint: the frame vmv_eefk_batch gives it and 6 * dim NaNs.  Checks:
 * unknown robot; NULL d_q / d_jac (VMV_ERR_INVALID_ARGUMENT, "null pointer"); n == 0 is VMV_OK without a device. */
int vmv_eefk_jacobian_batch(int robot, const float *d_q, size_t n, float *d_frames /* [n][16], may be NULL */,
                            float *d_jac /* [n][6][dim] */, void *stream);
int vmv_eefk_jacobian_batch_host(int robot, const float *q, size_t n, float *frames, float *jac);

/* Numerical inverse kinematics for many targets at once: n_seeds independent damped least-squares (Levenberg-Marquardt)
 * iterations per target, one lane per (target, seed).  Targets are frames as vmv_eefk_batch writes them.
 *   Seeds: d_seeds [n_targets][n_seeds][dim] (a warm start along a trajectory, say), clipped to the joint bounds; or NULL:
 *     seed s of every target is Halton sample halton_skip + s + 1 (vmv_halton_configs' sequence, generated on the stream
 *     into scratch per (device, stream) that vmv_release_staging frees), valid while halton_skip + n_seeds <= 1,000,000.
 *   Error of a state q with frame (R, t) against the target (R*, t*): e_p = t* - t; e_w = 1/2 sum_k R_k x R*_k over the
 *     three columns, whose norm is sin(theta) of the rotation between the frames; where tr(R*^T R) <= 1 (theta >= 90
 *     degrees) e_w enters the weighted error at unit length.  e = [e_p ; rot_weight e_w], E = 1/2 |e|^2.
 *   Converged: |e_p| <= pos_tol and, unless position_only, tr(R*^T R) > 1 and |e_w| <= rot_tol (e_w as it is).
 *   Iteration: evaluate the seed; then per iteration, with J the Jacobian above, its rotation rows times rot_weight and the
 *     column of every joint that sits at a bound while the descent direction (J^T e)_j points out of the range set to
 *     zero: A = J J^T + lambda I, A y = e (6 x 6 Cholesky), delta = J^T y scaled so that max_j |delta_j| <= max_step,
 *     q' = q + delta clipped to [lower, lower + span] of vmv_robot_bounds; evaluate q'; E' < E: accept and lambda =
 *     max(lambda / 4, 1e-5), else keep q and lambda = min(4 lambda, 1e6).  The converged test runs on the accepted state
 *     after every evaluation; a converged lane stops changing; a wave stops when its lanes are done or at max_iterations.
 *   Outputs per (target, seed): d_q the accepted state of smallest E - never worse than the (clipped) seed, always inside
 *     the bounds; d_err (may be NULL) = |e_p|, |e_w| of that state; d_status: bit 31 converged, bit 30 invalid input (a
 *     non-finite entry of the target or the seed: d_q is the seed as given, d_err NaN), the low bits the evaluations made
 *     after the seed's.
 * A lane's result depends on its own target, seed and settings alone, bit for bit - not on the batch, its position in it,
 * the entry point, or whether its Halton seed was generated or passed in.  fp32 without contraction.
 * Checks before any launch, those that need no device first: unknown robot; NULL d_targets / settings / d_q / d_status
 * ("null pointer"); the limits of the settings in the struct's order; the Halton limit (d_seeds == NULL); n_targets *
 * n_seeds >= 2^31 (all VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the check).  A refused call writes nothing;
 * n_targets == 0 is VMV_OK without a device. */
typedef struct
{
    uint32_t n_seeds;        /* seeds per target, 1 .. 1,024 */
    uint32_t max_iterations; /* 1 .. 2^30 - 1 */
    float pos_tol, rot_tol;  /* metres, radians; finite, > 0 */
    float rot_weight;        /* metres per radian: weight of the three rotation rows; finite, > 0 */
    float damping;           /* initial lambda; finite, > 0 */
    float max_step;          /* limit on the largest joint change of one step; finite, > 0 */
    int position_only;       /* 0 / 1: the rotation rows are zero and rot_tol is not tested */
} vmv_ik_settings;
int vmv_ik_batch(int robot, const float *d_targets /* [n_targets][16] */, size_t n_targets,
                 const float *d_seeds /* [n_targets][n_seeds][dim], or NULL */, uint64_t halton_skip,
                 const vmv_ik_settings *settings, float *d_q /* [n_targets][n_seeds][dim] */,
                 float *d_err /* [n_targets][n_seeds][2]: position, rotation; may be NULL */,
                 uint32_t *d_status /* [n_targets][n_seeds] */, void *stream);
int vmv_ik_batch_host(int robot, const float *targets, size_t n_targets, const float *seeds, uint64_t halton_skip,
                      const vmv_ik_settings *settings, float *q, float *err, uint32_t *status);

/* ---- end-effector constraints (no counterpart in the reference) -------------------------------------- */
/* A tolerance band on the end-effector frame (R, t) of a configuration: a position box in a frame C and a cone for one
 * tool axis, each optional.  csrc/vmv_constraint.h states the set-up, the residual, the band test, the projection and
 * the edge test in full; in short:
 *   position  p = C_R^T (t - C_t) with pos_lo <= p <= pos_hi per axis;
 *   axis      the angle between R tool_axis and C_R ref_axis is at most max_angle (axes normalised by the set-up);
 *   band test the nominal band widened by pos_tol and rot_tol: everyone - the projection's converged test, the check of a
 *             configuration, every sample of an edge - asks this one test, in fp32 on the frame vmv_eefk_batch computes;
 *   residual  v_k = p_k - clamp(p_k, lo_k, hi_k) and the sine of the angle beyond max_angle, about a x d.
 * The constraint records are HOST memory in every entry point (the set-up runs on the host in float64); n_constraints is
 * 1 (shared by all lanes) or n (one per lane). */
typedef struct
{
    float frame[16];            /* rigid frame C in the world, row-major 4 x 4 (R^T R = I within 1e-4) */
    float pos_lo[3], pos_hi[3]; /* bounds on p = C_R^T (t - C_t); -inf / +inf = free; lo == hi allowed (a plane, a line) */
    float tool_axis[3];         /* in the end-effector frame */
    float ref_axis[3];          /* in C */
    float max_angle;            /* bound on the angle between R tool_axis and C_R ref_axis; 0 = orientation free; <= pi/2 */
} vmv_ee_constraint;
typedef struct
{
    uint32_t max_iterations;               /* 0 = 16: evaluations after the first; below 2^30 */
    float pos_tol, rot_tol;                /* 0 = 1e-4 m, 1e-3 rad: the band everyone tests is the nominal one widened by these */
    float rot_weight, damping, max_step;   /* 0 = vmv_ik_settings' defaults (0.25, 1e-2, 0.5) */
    float check_step;                      /* 0 = 0.05: joint-space distance between two band samples of an edge */
} vmv_constraint_settings;
/* The layout of vmv_constraint_settings is final at these seven fields (28 bytes) for vmv_abi_version() 1: it is passed by
 * pointer without a size, so it never grows.  A later call that needs more settings (a planner's, say) takes a struct of
 * its own that holds this one as its first member `base`, as vmv_rrtc_goals_settings holds vmv_rrtc_settings. */
/* Projection into the band: vmv_ik_batch's damped least-squares iteration (its Jacobian, Cholesky solve, bound-hold rule,
 * step cap, clip to the joint bounds and damping schedule) on the residual above, one lane per configuration.  d_q_out
 * [n][dim] is the accepted state of smallest residual energy, inside the joint bounds but for the two kinds of rows below that come
 * back as given, which are not clipped; only joints that move the end effector change.  d_residuals [n][2] (may be NULL): |v| in metres and the angle beyond max_angle in radians of that
 * state.  d_status [n]: bit 31 converged (the band test passes), bit 30 a non-finite joint (the row comes back as given
 * with NaN residuals), the low bits the evaluations after the first.  A configuration inside the joint bounds and in
 * the band comes back bit for bit with 0 evaluations; one whose axes are antiparallel once clipped to the joint bounds
 * comes back as given (unclipped, so outside the bounds if it was), not converged, with 0 evaluations.  A lane's result depends on its own configuration, constraint and settings alone, bit for bit.  d_q_out
 * must not overlap d_q.
 * Checks before any launch, in this order: unknown robot; NULL d_q / constraints / settings / d_q_out / d_status ("null
 * pointer"); n_constraints not 1 and not n; the settings in the struct's order (finite, not negative); n >= 2^31; then
 * every constraint in order: non-finite frame, NaN bounds, pos_lo > pos_hi, non-finite axes, NaN max_angle, a frame that
 * is not rigid within 1e-4, max_angle outside [0, pi/2], a zero axis with max_angle > 0 (all VMV_ERR_INVALID_ARGUMENT,
 * vmv_last_error() names the check and the constraint's index).  A refused call writes nothing; n == 0 is VMV_OK without
 * a device. */
int vmv_constraint_project_batch(int robot, const float *d_q /* [n][dim] */, size_t n, const vmv_ee_constraint *constraints,
                                 size_t n_constraints, const vmv_constraint_settings *settings, float *d_q_out /* [n][dim] */,
                                 float *d_residuals /* [n][2], may be NULL */, uint32_t *d_status /* [n] */, void *stream);
int vmv_constraint_project_batch_host(int robot, const float *q, size_t n, const vmv_ee_constraint *constraints,
                                      size_t n_constraints, const vmv_constraint_settings *settings, float *q_out,
                                      float *residuals, uint32_t *status);
/* The band test of n configurations: bit i of d_bits (ceil(n / 64) words, the unused bits 0) is 1 iff configuration i is
 * in the band; d_residuals [n][2] (may be NULL) as above, NaN for a non-finite row.  The checks of the projection, with
 * d_bits in place of the outputs. */
int vmv_constraint_check_batch(int robot, const float *d_q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                               const vmv_constraint_settings *settings, uint64_t *d_bits, float *d_residuals, void *stream);
int vmv_constraint_check_batch_host(int robot, const float *q, size_t n, const vmv_ee_constraint *constraints, size_t n_constraints,
                                    const vmv_constraint_settings *settings, uint64_t *bits, float *residuals);
/* The band test of n edges a -> b: n_c = max(1, ceil(|b - a| / check_step)) samples a + (b - a) * (i / n_c), i = 1 .. n_c,
 * d_ok[e] = 1 iff all of them are in the band, else 0; an edge of more than 1,024 samples or of non-finite length answers
 * 0.  One wave per edge.  The checks of the projection, with d_a, d_b and d_ok as the arrays. */
int vmv_constraint_check_motion_batch(int robot, const float *d_a, const float *d_b, size_t n, const vmv_ee_constraint *constraints,
                                      size_t n_constraints, const vmv_constraint_settings *settings, uint8_t *d_ok, void *stream);
int vmv_constraint_check_motion_batch_host(int robot, const float *a, const float *b, size_t n, const vmv_ee_constraint *constraints,
                                           size_t n_constraints, const vmv_constraint_settings *settings, uint8_t *ok);

/* sphere_environment_in_collision(environment, x, y, z, r) — collision/validity.hh:47-158, the predicate every fkcc
 * check is made of (and CAPT::collides / MVT::collides behind it, collision/capt.hh:374-415), for a batch of free
 * spheres: spheres [n][4] = x y z r, hits[i] = 1 iff sphere i collides with the environment.  Each sphere is its own
 * replicated rake (lanes independent). */
int vmv_spheres_in_collision_batch(const vmv_env *env, const float *d_spheres, size_t n, uint8_t *d_hits, void *stream);
int vmv_spheres_in_collision_batch_host(const vmv_env *env, const float *spheres, size_t n, uint8_t *hits);

/* <robot>.filter_self_from_pointcloud(pc, point_radius, configuration, environment) — bindings/robot_helper.hh:284-322:
 * keeps the points whose sphere (x, y, z, point_radius) neither overlaps a collision sphere of the robot at `q`
 * (sphere_sphere_sql2 < 0) nor collides with the environment; order preserved.  Host buffers; out may be NULL (count only);
 * VMV_ERR_CAPACITY if out is too small. */
int vmv_filter_self_from_pointcloud(int robot, const vmv_env *env, const float *q, const float *points_xyz, size_t n,
                                    float point_radius, float *out_xyz, size_t capacity, size_t *n_out);

/* host-buffer variants (copies included; the PCIe-inclusive path) */
int vmv_fk_batch_host(int robot, const float *q, size_t n, float *out);
int vmv_eefk_batch_host(int robot, const float *q, size_t n, float *out);
int vmv_validate_batch_host(int robot, const vmv_env *env, const float *q, size_t n, uint64_t *bits);
int vmv_validate_motion_batch_host(int robot, const vmv_env *env, const float *start, const float *goal, size_t n,
                                   uint64_t *bits);
/* Every call that takes host buffers (the *_host variants, vmv_contacts_batch_host and vmv_filter_self_from_pointcloud
 * included) stages through a per-thread device arena that is reused between calls: a thread keeps up to 64 MiB of device
 * memory after such a call (requests above 64 MiB are not kept beyond their call) until it calls this function.
 * vmv_validate_motion_batch keeps 8 bytes of device scratch per edge per (device, stream) for its task
 * lists, the multi-environment calls their tables, vmv_ik_batch 64 KiB of Halton seeds.  Frees the calling thread's
 * arena and every stream's scratch and tables (waits for the batches in flight); optional — none of this memory is touched at thread or process exit. */
int vmv_release_staging(void);

/* ---- multi-GPU: one process per GPU, every unit independent given the read-only environment ------- */
/* Contiguous shard [*lo, *hi) of an n-unit batch (configurations or edges) for `rank` of `world`: every boundary except
 * the last is a multiple of 64, so a shard owns whole validity words and - an edge being a whole sequence of 8-lane
 * rakes - no rake straddles two GPUs.  Each rank finalizes its own copy of the environment on its device, calls
 * vmv_validate_batch / vmv_validate_motion_batch on its shard (d_q + lo * dimension, hi - lo units) and the ranks
 * all-gather the packed words (ncclAllGather of vmv_shard_words(n, world) uint64 per rank; ranks whose shard is
 * shorter pad with zero words).  That all-gather is the path's only exchange step.  Python: vamp_mvt_amd.sharding. */
int vmv_shard_range(size_t n, int rank, int world, size_t *lo, size_t *hi);
/* uint64 words each rank contributes to the all-gather: ceil(ceil(n / 64) / world) */
size_t vmv_shard_words(size_t n, int world);

/* ---- sampler --------------------------------------------------------------------------------------------- */
/* <robot>.halton() / RNG.next() — random/halton.hh:75-108 with the default prime bases, generated on the device:
 * fills d_q[n][dimension] with samples skip+1 .. skip+n of the reference's sequence (bit-exact: the sequence's
 * n/d are exact small integers, so element j of sample i is float(radical_inverse_numerator) / float(b_j^k),
 * scaled by Robot::scale_configuration).  Valid while skip + n <= 1,000,000 (the reference re-seeds after that). */
int vmv_halton_configs(int robot, uint64_t skip, float *d_q, size_t n, void *stream);

/* ---- lockstep planner: many independent RRT-Connect problems in one call ------------------------------- */
/* RRT-Connect (planning/rrtc.hh:33-245 without dynamic domain, one goal, start_tree_first = false; vmv_rrtc_multi_goals
 * below has the three) for n_problems problems at once, problem p from
 * starts[p] to goals[p] ([n_problems][dimension] host arrays) in envs[p], its samples the Halton samples
 * halton_skips[p] + 1, + 2, ... (halton_skips NULL = all 0).  The problems advance in lockstep rounds: per round a step
 * kernel (nearest neighbour, extension, connect march, tree bookkeeping, termination; one workgroup per unfinished
 * problem) writes ONE edge question per unfinished problem, and one vmv_validate_motion_batch_multi launch sequence
 * answers all of them.  Every check_every rounds (0 = the default, 16) the host reads which problems are finished and
 * drops them from the next rounds.  A problem's result depends on its own inputs alone, bit for bit (DESIGN §5c gives the
 * arithmetic: fp32, one rounding per operation, the first nearest node on ties).  Each problem owns a pool of max_samples
 * nodes on the device (max_samples * (dimension + 1) * 4 bytes) and never holds more.
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / starts / goals / settings / out
 * or a NULL handle, range not finite or <= 0, max_samples < 2, halton skip + max_iterations > 1,000,000 (the sequence's
 * validity limit, as vmv_halton_configs), n_problems >= 2^31 (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment
 * (VMV_ERR_NOT_FINALIZED); an environment of another device (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out
 * untouched.  n_problems == 0 is VMV_OK with an empty result.  A start or goal with a non-finite joint: that problem ends
 * unsolved (every edge from or to it is invalid).  Environments not yet prepared for the robot are prepared in one batch.
 * Synchronous, host buffers, on the default stream; repeated handles are allowed. */
typedef struct
{
    float range;                 /* rrtc_settings.hh: range */
    int balance;                 /* 0 / 1 */
    float tree_ratio;
    uint32_t max_iterations, max_samples;
    uint32_t check_every;        /* rounds between two looks of the host at the finished flags; 0 = default */
} vmv_rrtc_settings;
typedef struct vmv_plans vmv_plans;
enum
{
    VMV_PLAN_SOLVED = 0,
    VMV_PLAN_MAX_ITERATIONS = 1, /* the loop ended because iterations reached max_iterations (checked first) */
    VMV_PLAN_MAX_SAMPLES = 2     /* ... because the two trees together hold max_samples nodes */
};
int vmv_rrtc_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                   const uint64_t *halton_skips, const vmv_rrtc_settings *settings, vmv_plans **out);
/* Per problem (arrays of n_problems, any may be NULL): status (VMV_PLAN_*), iterations, sizes2 = |A|, |B| as the
 * planner's last iteration named the trees (PlanningResult::size), path_lengths in waypoints (0 = unsolved).  Totals (may
 * be NULL): rounds = validation launches made, questions = edge questions the problems asked (the null questions of
 * finished problems not counted). */
int vmv_plans_summary(const vmv_plans *plans, uint8_t *status, uint32_t *iterations, uint32_t *sizes2,
                      uint32_t *path_lengths, uint64_t *rounds, uint64_t *questions);
/* every path's waypoints ([path_length][dimension] each, the stored node bits, start first), packed in problem order;
 * VMV_ERR_CAPACITY if capacity_floats is too small (nothing is written) */
int vmv_plans_paths(const vmv_plans *plans, float *out, size_t capacity_floats);
int vmv_plans_destroy(vmv_plans *plans);
/* vmv_rrtc_multi with the three things of planning/rrtc.hh:33-245 it leaves out ("Goal sets, dynamic domain,
 * start_tree_first"); with all three off and one goal per problem the result is vmv_rrtc_multi's, byte for byte.
 *   Goal sets: goals is [goal_offsets[n_problems]][dimension] and problem p owns goals [goal_offsets[p],
 *     goal_offsets[p + 1]) (goal_offsets NULL = one goal per problem, goals [n_problems][dimension]).  The questions
 *     start -> goal g are asked in order of g, one per round; the first valid one ends the problem with (start, goal g).
 *     Otherwise every goal is a root of the goal tree (goal g at index g).  A non-finite goal is never the nearest node.
 *   Dynamic domain (rrtc.hh:121-126, 148-155, 226-237): every node has a radius, unset (FLT_MAX) at first.  An iteration
 *     whose sample lies farther from its nearest node than that node's radius ends there: it has spent its iteration and
 *     its draw and asks nothing, so the step kernel draws again within the same round.  A valid extension multiplies a set
 *     radius of the nearest node by (1 + alpha); an invalid one sets an unset radius to `radius` and makes a set one
 *     max(r * (1 - alpha), min_radius).  The connect march neither reads nor writes a radius.  Costs max_samples * 4 more
 *     bytes per problem.
 *   start_tree_first: the first iteration starts with A = goal tree, so that with equal sizes the balance rule hands the
 *     first extension to the start tree (the reference's default; 0 is vmv_rrtc_multi's behaviour).
 * Checks: those of vmv_rrtc_multi in its order, then goal_offsets not starting at 0 or decreasing, an empty goal set,
 * 1 + a set's goals > max_samples, 2^31 goals or more in all; with dynamic_domain set, radius or min_radius not finite or
 * <= 0, alpha not finite, < 0 or >= 1 (all VMV_ERR_INVALID_ARGUMENT; with dynamic_domain 0 the three values are not read).
 * A call that fails leaves *out untouched.  n_problems == 0 is VMV_OK with an empty result.  vmv_plans_summary,
 * vmv_plans_paths and vmv_plans_destroy work on the result as on vmv_rrtc_multi's. */
typedef struct
{
    vmv_rrtc_settings base;
    int dynamic_domain;          /* 0 / 1 */
    float radius, alpha, min_radius; /* rrtc_settings.hh: 4, 0.0001, 1 */
    int start_tree_first;        /* 0 / 1 */
} vmv_rrtc_goals_settings;
int vmv_rrtc_multi_goals(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                         const size_t *goal_offsets, const uint64_t *halton_skips, const vmv_rrtc_goals_settings *settings,
                         vmv_plans **out);
/* Per problem of a vmv_rrtc_multi_goals result (n_problems, may be NULL): the index, within its own set, of the goal its
 * path ends in; UINT32_MAX = unsolved.  VMV_ERR_INVALID_ARGUMENT on the plans of another call. */
/* RRT-Connect under an end-effector constraint: vmv_rrtc_multi_goals - its arguments, its checks in its
 * order, its state machine (extension, connect march, dynamic domain, goal sets, start_tree_first, the limits, the trace)
 * and its result - with every tree node projected into the band of the problem's constraint and every edge band-checked.
 *   Before the rounds ONE band test (vmv_constraint_check_batch's) runs over all starts and goals.  A problem whose start
 *     is out of band or that has no in-band goal ends VMV_PLAN_INVALID_ENDPOINT with no path and no question; the
 *     out-of-band goals of a set are never roots and never asked (goal indices still count within the caller's set).
 *   A round: the step kernel writes each problem's question; then one launch per round projects the question's far end
 *     where it is a new node (the extension's `new`, a march step's point; vmv_constraint_project_batch's lane, bit for
 *     bit) and writes it back to the question and to the tree.  A projection that does not converge, or lands farther
 *     than max_stretch * range from the question's near end, leaves both as they were and answers 0.  Then the edge's band
 *     test (vmv_constraint_check_motion_batch's, bit for bit).  The answer the state machine consumes is validity AND
 *     that.  A direct question start -> goal is band-checked only.
 *   The path: its waypoints are in the band and its edges pass the edge test at check_step; the last point of a connect
 *     march lies within one fp32 rounding of the node it reaches, and that closing step is not asked, as in
 *     vmv_rrtc_multi.  With a constraint that restricts nothing the result is vmv_rrtc_multi_goals's byte for byte while
 *     every node lies inside the joint bounds (the projection clips to them).
 * Further checks, after vmv_rrtc_multi_goals's and before any device call: NULL constraints / constraint_settings ("null
 * pointer"); n_constraints not 1 and not n_problems; the settings as the batch calls check them; max_stretch (finite, not
 * negative); every constraint (VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the check).  A problem's result is its
 * own, whatever the batch, its order and check_every.  Readouts: vmv_plans_summary / _paths / _goal_indices / _destroy. */
typedef struct
{
    vmv_constraint_settings base;
    float max_stretch; /* 0 = 2: a projected far end farther than max_stretch * range from its near end is answered invalid */
} vmv_constraint_plan_settings;
int vmv_rrtc_multi_constrained(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                               const size_t *goal_offsets, const uint64_t *halton_skips, const vmv_rrtc_goals_settings *settings,
                               const vmv_ee_constraint *constraints /* host, [n_constraints] */, size_t n_constraints,
                               const vmv_constraint_plan_settings *constraint_settings, vmv_plans **out);
/* refused [n_problems]: per problem the questions the constraint answered 0 (a failed or overstretched projection, an edge
 * out of band), whatever validity said.  VMV_ERR_INVALID_ARGUMENT on plans made by neither vmv_rrtc_multi_constrained nor
 * vmv_aorrtc_multi_constrained (which adds its searches' and its simplifications' counts, see there). */
int vmv_plans_band_refused(const vmv_plans *plans, uint32_t *refused);
int vmv_plans_goal_indices(const vmv_plans *plans, uint32_t *goal_index);

/* ---- batched PRM: many independent roadmap problems in one call ------------------------------------------ */
/* A probabilistic roadmap per problem, for n_problems problems at once: problem p runs from starts[p] to goals[p] in
 * envs[p]; its roadmap is built over n_samples samples, the Halton samples halton_skips[p] + 1, ... (NULL = all 0) or,
 * where `samples` is not NULL, the caller's ([n_problems][n_samples][dimension] host floats; halton_skips is then not
 * read).  The launches are a fixed sequence whatever the problems are: the vertices and ONE vmv_validate_batch_multi
 * call; the k nearest valid vertices of every valid vertex; the candidate edges and ONE vmv_validate_motion_batch_multi
 * call; the shortest path; the paths gathered.  The host synchronises once in between (the per-problem edge counts).
 * Per problem, bit-defined (fp32, one rounding per written operation):
 *   V = n_samples + 2 vertices: 0 = start, 1 = goal, 2 + i = sample i; valid[v] = validate(vertex v) (a non-finite
 *   joint: invalid).  !valid[0] or !valid[1]: VMV_PLAN_INVALID_ENDPOINT, no path, no edge is asked.
 *   d2(v, u) = sum over the joints in order of (v[j] - u[j])^2, w = sqrtf(d2), R2 = radius * radius (+inf: no cut).
 *   nbr(v), for every valid v: the k valid vertices u != v with 0 < d2(v, u) <= R2 that come first in the order (d2, then
 *   vertex id), fewer if fewer exist; vertices 0 and 1 are never each other's neighbour.
 *   Candidate edges, in this order: (0, 1); then for v ascending, for slot s ascending, u = nbr(v)[s]: the edge {v, u} if
 *   v < u or v is not in nbr(u) (every undirected pair once).  The question of {a, b}, a < b, is validate_motion(a -> b).
 *   Edge (0, 1) valid: VMV_PLAN_SOLVED, path = [start, goal], cost = w(0, 1), iterations 0.  Else g[0] = 0, g[v] = min over
 *   the valid edges {u, v} of fl(g[u] + w(u, v)) (the least fixpoint; w = +inf relaxes nothing); g[1] = +inf:
 *   VMV_PLAN_NO_PATH; else VMV_PLAN_SOLVED, cost = g[1], the path walked back from 1 with parent(v) = the lowest id u with
 *   a valid edge {u, v}, fl(g[u] + w(u, v)) == g[v] and g[u] < g[v] (a walk that finds no parent ends as
 *   VMV_PLAN_NO_PATH); iterations = n_samples (also for VMV_PLAN_NO_PATH).
 * A problem's result depends on its own inputs alone, bit for bit.  Agreement with the reference's incremental PRM
 * (planning/prm.hh) is not claimed.  The result is a vmv_plans: vmv_plans_summary reports sizes2 = [valid vertices,
 * valid edges], rounds = validation calls made, questions = candidate edges asked; vmv_plans_paths and
 * vmv_plans_destroy work as for vmv_rrtc_multi.
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / starts / goals / settings / out
 * or a NULL handle, n_samples not a multiple of 64 or outside 64 .. 8,128, k outside 1 .. 16, radius NaN or <= 0, halton
 * skip + n_samples > 1,000,000 where samples is NULL, n_problems * (n_samples + 2) * k >= 2^31
 * (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment (VMV_ERR_NOT_FINALIZED); an environment of another device
 * (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out untouched.  n_problems == 0 is VMV_OK with an empty result.
 * Environments not yet prepared for the robot are prepared in one batch.  Synchronous, host buffers, on the default
 * stream; repeated handles are allowed.  The vertices are validated as 2 * n_problems segments of one
 * vmv_validate_batch_multi call: each problem's samples own whole validity words (hence the multiple of 64), its two
 * endpoints share a word with other problems' and rest on that call's flat layout (shared words are zeroed first and
 * each segment's bits combined in atomically). */
typedef struct
{
    uint32_t n_samples, k;
    float radius;                /* neighbours lie within this distance; +inf = no cut */
    int keep_roadmaps;           /* 0 / 1: keep host copies of every problem's vertex flags and candidate edges */
} vmv_prm_settings;
enum
{
    VMV_PLAN_NO_PATH = 3,         /* start and goal are valid and the roadmap does not connect them */
    VMV_PLAN_INVALID_ENDPOINT = 4 /* the start or the goal is invalid */
};
int vmv_prm_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                  const uint64_t *halton_skips, const float *samples, const vmv_prm_settings *settings, vmv_plans **out);
/* Per problem of a vmv_prm_multi result (arrays of n_problems, any may be NULL): valid vertices, candidate edges, valid
 * edges, cost (+inf = unsolved).  VMV_ERR_INVALID_ARGUMENT on the plans of vmv_rrtc_multi; the next two also unless
 * keep_roadmaps was set, or for p out of range. */
int vmv_plans_roadmap_summary(const vmv_plans *plans, uint32_t *valid_vertices, uint32_t *candidate_edges,
                              uint32_t *valid_edges, float *costs);
/* valid[v] of problem p's n_samples + 2 vertices */
int vmv_plans_roadmap_vertices(const vmv_plans *plans, size_t p, uint8_t *valid);
/* problem p's candidate edges in candidate order: *n = their number (n may be NULL); pairs2 [n][2] vertex ids a < b and
 * valid [n] (either may be NULL; with both NULL the call only counts); VMV_ERR_CAPACITY if capacity (in edges) is too
 * small (nothing is written but *n) */
int vmv_plans_roadmap_edges(const vmv_plans *plans, size_t p, uint32_t *pairs2, uint8_t *valid, size_t capacity, size_t *n);

/* ---- device-resident roadmaps: built once per scene, asked many times ------------------------------------ */
/* vmv_roadmaps_build builds n_roadmaps roadmaps in one call, roadmap r in envs[r], over n_samples samples each: the Halton
 * samples halton_skips[r] + 1, ... (NULL = all 0) or, where `samples` is not NULL, the caller's
 * ([n_roadmaps][n_samples][dimension] host floats).  It is vmv_prm_multi without endpoints: all samples through ONE
 * vmv_validate_batch_multi call, the k nearest valid samples of every valid sample, all candidate edges through ONE
 * vmv_validate_motion_batch_multi call, one host synchronisation in between (the edge counts).  The samples, their validity
 * words, the candidate pairs, their weights and their answers stay on the device inside the handle.
 * Roadmap r, bit-defined (the arithmetic of vmv_prm_multi): vertices are the samples i = 0 .. n_samples - 1,
 *   valid[i] = finite and validate; nbr(v) for a valid v = the k valid u != v with 0 < d2(v, u) <= radius^2 first in the
 *   order (d2, id); candidate edges for v ascending, slot ascending, u = nbr(v)[slot]: {v, u} if v < u or v is not in nbr(u);
 *   each is asked lower id -> higher id.  Samples 0 and 1 are ordinary vertices.
 * A roadmap does not depend on which other roadmaps share the call.
 * The handle records the robot, the device and the environment handles.  AN ENVIRONMENT MUST OUTLIVE ITS ROADMAPS, and a
 * roadmap answers for the environment as it was finalized at build time (an environment is immutable after
 * vmv_env_finalize, so a handle cannot go stale while its environments live).  The handle is used on the device it was
 * built on (another current device: VMV_ERR_INVALID_ARGUMENT).
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / settings / out or a NULL handle,
 * n_samples not a multiple of 64 or outside 64 .. 8,128, k outside 1 .. 16, radius NaN or <= 0, halton skip + n_samples >
 * 1,000,000 where samples is NULL, n_roadmaps * n_samples * k >= 2^31 (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment
 * (VMV_ERR_NOT_FINALIZED); an environment of another device (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out
 * untouched.  n_roadmaps == 0 is VMV_OK with an empty handle.  Synchronous, host buffers, on the default stream; repeated
 * environment handles are allowed. */
typedef struct vmv_roadmaps vmv_roadmaps;
typedef struct
{
    uint32_t n_samples, k;
    float radius;                /* neighbours lie within this distance; +inf = no cut */
} vmv_roadmap_settings;
typedef struct
{
    uint32_t k_connect;          /* connections tried per endpoint, 1 .. 32 */
    float radius;                /* they lie within this distance; +inf = no cut */
} vmv_roadmap_query_settings;
int vmv_roadmaps_build(int robot, const vmv_env *const *envs, size_t n_roadmaps, const uint64_t *halton_skips,
                       const float *samples, const vmv_roadmap_settings *settings, vmv_roadmaps **out);
/* n_queries queries in one call, query q from starts[q] to goals[q] ([n_queries][dimension] host floats) against roadmap
 * roadmap_of_query[q] (NULL = all 0).  A fixed launch sequence with no host synchronisation before the results: all
 * endpoints through ONE vmv_validate_batch_multi call (the host groups the queries by roadmap with a stable counting sort,
 * one segment per roadmap that has queries, and un-permutes the results); a connect kernel; 1 + 2 * k_connect edge
 * questions per query through ONE vmv_validate_motion_batch_multi call; a shortest-path kernel (one workgroup per query,
 * over the roadmap's shared edge list plus the query's own connection edges); the paths gathered.
 * Per query, bit-defined: graph ids 0 = start, 1 = goal, 2 + i = sample i.  An endpoint that is not finite or
 *   not valid: VMV_PLAN_INVALID_ENDPOINT, nothing is asked.  conn(e), e = start, goal: the k_connect valid samples u with
 *   0 < d2(e, u) <= radius^2 first in the order (d2, id).  Questions, in this order: start -> goal; start -> u over
 *   conn(start); goal -> u over conn(goal).  The direct edge valid: VMV_PLAN_SOLVED, path = [start, goal], cost =
 *   sqrtf(d2(start, goal)), iterations 0.  Else iterations = n_samples; over the roadmap's valid edges plus the valid
 *   connection edges g[0] = 0, g = the least fixpoint of g[v] = min fl(g[u] + w), parent(v) = the lowest id u with an edge
 *   {u, v}, fl(g[u] + w) == g[v] and g[u] < g[v]; g[1] finite and the walk from 1 reaching 0: VMV_PLAN_SOLVED, cost =
 *   g[1]; else VMV_PLAN_NO_PATH.
 * A query's result depends on its endpoints, its roadmap and the settings alone.  The result is a vmv_plans:
 * vmv_plans_summary reports sizes2 = [valid connection edges of the start, of the goal], rounds = validation calls that
 * carried a question (2; 1 if no query has both endpoints valid: the edge call then carries null questions only),
 * questions = the sum of the queries' questions; vmv_plans_paths and vmv_plans_destroy work as for vmv_rrtc_multi,
 * vmv_plans_query_summary gives the costs, vmv_plans_roadmap_* refuse it.  Each query owns a block of 1 + 2 * k_connect
 * question slots; unused slots, and every slot of a query with an invalid endpoint, carry a null question (an endpoint to
 * itself) that is neither counted nor read.
 * Device-free checks first: NULL roadmaps / starts / goals / settings / out, k_connect outside 1 .. 32, radius NaN or <= 0,
 * n_queries * (1 + 2 * k_connect) >= 2^31, a roadmap_of_query entry >= the handle's roadmap count
 * (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out untouched.  n_queries == 0 is VMV_OK with an empty result. */
int vmv_roadmaps_query(const vmv_roadmaps *roadmaps, size_t n_queries, const uint32_t *roadmap_of_query, const float *starts,
                       const float *goals, const vmv_roadmap_query_settings *settings, vmv_plans **out);
/* Per query of a vmv_roadmaps_query result (arrays of n_queries, either may be NULL): cost (+inf = unsolved) and
 * edges_checked = 1 + |conn(start)| + |conn(goal)| (0 for VMV_PLAN_INVALID_ENDPOINT).  VMV_ERR_INVALID_ARGUMENT on plans
 * of another origin. */
int vmv_plans_query_summary(const vmv_plans *plans, float *costs, uint32_t *edges_checked);
/* Per roadmap (arrays of the handle's roadmap count, any may be NULL): valid samples, candidate edges, valid edges. */
int vmv_roadmaps_summary(const vmv_roadmaps *roadmaps, uint32_t *valid_vertices, uint32_t *candidate_edges,
                         uint32_t *valid_edges);
/* roadmap r's samples ([n_samples][dimension]) and valid[i] of each (either may be NULL), copied from the device */
int vmv_roadmaps_vertices(const vmv_roadmaps *roadmaps, size_t r, float *samples, uint8_t *valid);
/* roadmap r's candidate edges in candidate order, as vmv_plans_roadmap_edges gives a problem's: pairs2 [n][2] sample ids
 * a < b, valid [n]; VMV_ERR_CAPACITY if capacity (in edges) is too small (nothing is written but *n) */
int vmv_roadmaps_edges(const vmv_roadmaps *roadmaps, size_t r, uint32_t *pairs2, uint8_t *valid, size_t capacity, size_t *n);
int vmv_roadmaps_destroy(vmv_roadmaps *roadmaps);

/* ---- lockstep simplifier: many independent paths in one call -------------------------------------------- */
/* simplify() (planning/simplify.hh:192-260) with the SHORTCUT and BSPLINE routines for n_paths paths at once: path p is
 * points[offsets[p] .. offsets[p + 1]) ([offsets[n_paths]][dimension] host floats, offsets in waypoints, offsets[0] = 0)
 * in envs[p].  The paths advance in lockstep rounds like the problems of vmv_rrtc_multi: per round a step kernel (one
 * wave per unfinished path: consumes the answers of the previous round, erases or replaces waypoints, advances the
 * routine) writes questions_per_round edge questions per unfinished path, and one vmv_validate_motion_batch_multi launch
 * sequence answers all of them.  Shortcut asks the next candidates j of its waypoint i from the far end and takes the
 * largest valid one; a B-spline step asks both motions of the next candidates that passed the min_change test.  Both
 * end with the path the reference's one-question-at-a-time loops end with, so a path's result depends on its own
 * inputs and the settings other than questions_per_round and check_every alone, bit for bit (DESIGN §5d gives the
 * arithmetic: fp32, one rounding per operation).  Paths of fewer than 3 waypoints come back as they are without a
 * question.  Each path owns max_waypoints waypoints (twice, 2 * max_waypoints * dimension * 4 bytes on the device): a
 * B-spline subdivision that would need more is not made, the path stays as it stood (still a valid path between its
 * ends) and ends with VMV_SIMPLIFY_CAPACITY.
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / points / offsets / settings /
 * out or a NULL handle, offsets not starting at 0 or decreasing, an operation other than SHORTCUT / BSPLINE (REDUCE and
 * PERTURB draw random numbers: not part of this call), n_operations > 8, interpolate != 0, questions_per_round not one
 * of 0 2 4 8 16 32 64, max_waypoints below the longest path, n_paths * questions_per_round >= 2^31
 * (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment (VMV_ERR_NOT_FINALIZED); an environment of another device
 * (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out untouched.  n_paths == 0 is VMV_OK with an empty result.
 * A question that touches a non-finite waypoint is invalid, and no non-finite distance exceeds min_change.
 * Environments not yet prepared for the robot are prepared in one batch.  Synchronous, host buffers, on the default
 * stream; repeated handles are allowed. */
enum
{
    VMV_SIMPLIFY_BSPLINE = 0, /* the values of planning/simplify_settings.hh: SimplifyRoutine */
    VMV_SIMPLIFY_REDUCE = 1,  /* refused */
    VMV_SIMPLIFY_SHORTCUT = 2,
    VMV_SIMPLIFY_PERTURB = 3  /* refused */
};
enum
{
    VMV_SIMPLIFY_OK = 0,
    VMV_SIMPLIFY_CAPACITY = 1 /* a subdivision would have exceeded max_waypoints */
};
typedef struct
{
    uint32_t max_iterations;
    uint32_t interpolate;             /* must be 0 */
    uint32_t n_operations;            /* <= 8; repeated operations and either order are allowed */
    uint32_t operations[8];           /* VMV_SIMPLIFY_SHORTCUT / VMV_SIMPLIFY_BSPLINE, run in this order per iteration */
    uint32_t bspline_max_steps;
    float bspline_min_change;
    float bspline_midpoint_interpolation;
    uint32_t max_waypoints;           /* waypoints a path may grow to; 0 = default (2,048) */
    uint32_t questions_per_round;     /* edge questions per path per round: 2 4 8 16 32 64; 0 = default */
    uint32_t check_every;             /* rounds between two looks of the host at the finished flags; 0 = default */
} vmv_simplify_settings;
typedef struct vmv_paths vmv_paths;
int vmv_simplify_multi(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                       const vmv_simplify_settings *settings, vmv_paths **out);
/* Per path (arrays of n_paths, any may be NULL): status (VMV_SIMPLIFY_*), iterations as the reference counts them,
 * lengths in waypoints, questions asked.  Totals (may be NULL): rounds = validation launches made, total_questions =
 * edge questions the paths asked (the null questions of unused slots and finished paths not counted). */
int vmv_paths_summary(const vmv_paths *paths, uint8_t *status, uint32_t *iterations, uint32_t *lengths,
                      uint32_t *questions, uint64_t *rounds, uint64_t *total_questions);
/* every path's waypoints ([length][dimension] each), packed in path order; VMV_ERR_CAPACITY if capacity_floats is too
 * small (nothing is written) */
int vmv_paths_points(const vmv_paths *paths, float *out, size_t capacity_floats);
int vmv_paths_destroy(vmv_paths *paths);

/* ---- lockstep simplifier under end-effector constraints ------------------------------------- */
/* vmv_simplify_multi inside the band of an end-effector constraint: the arguments are vmv_simplify_multi's, then one
 * constraint for every path or one per path (n_constraints = 1 or n_paths) and the vmv_constraint_settings of the
 * vmv_constraint_*_batch calls.  The contract per path is vmv_simplify_multi's (simplify.hh's control flow, fp32, one
 * rounding per operation) with three changes:
 *  1. Every question (a, b) is validate_motion(a, b) AND band_edge(a, b).  band_edge is vmv_constraint_check_motion_batch's
 *     answer for that edge under the path's constraint and constraint_settings: the same samples, the same check_step,
 *     the same 1,024-sample cap.
 *  2. A B-spline candidate is projected before it is asked.  mid is computed as in vmv_simplify_multi, the min_change test
 *     on the unprojected mid included; then mid is replaced by mid_p, vmv_constraint_project_batch's result for it bit for
 *     bit (a mid already in the band and inside the joint bounds comes back unchanged with 0 evaluations).  Where the
 *     projection does not converge both motions of the candidate are answered 0 and the waypoint stays.  Where it does,
 *     the motions asked are (path[index - 1], mid_p) and (mid_p, path[index + 1]), and the waypoint is replaced by mid_p
 *     iff both answers are 1 AND distance(path[index], mid_p) > bspline_min_change, distance being the fp32 function of
 *     the first test.  There is no bound on how far the projection moves mid: the two motions asked bound the move.
 *  3. The input is looked at before the rounds: one band test over the first waypoint of every path and one edge band
 *     test over every input edge.  A path of 3 waypoints or more that fails either ends VMV_SIMPLIFY_OUT_OF_BAND: it comes
 *     back with its input bytes, 0 iterations and 0 questions and does not disturb the other paths.  (A non-finite
 *     waypoint is out of band.)  Paths of fewer than 3 waypoints come back as they are without any test.
 * As in vmv_simplify_multi a subdivision does not ask the halves of an edge.  So every point of a returned OK or
 * CAPACITY path lies on an asked in-band edge or on a half of one: within check_step / 2 of joint-space length of a
 * passing sample, not necessarily on one.
 * vmv_paths_band_refused: per path, of the questions the SERIAL loop asks - the shortcut candidates of a waypoint from
 * the far end down to and including the first accepted one, the first motion of every B-spline candidate and the second
 * only where the first was answered 1, the direct question - those the constraint answered 0 (a failed projection, an
 * out-of-band edge), whatever validity said.  It does not depend on questions_per_round; `questions` in
 * vmv_paths_summary keeps its windowed meaning.
 * A path's waypoints, status, iterations and band_refused depend on its own input, environment, constraint and the
 * settings other than questions_per_round and check_every alone, bit for bit.  With a constraint that restricts nothing
 * (all bounds infinite, max_angle 0) and finite input the result is vmv_simplify_multi's byte for byte, rounds and
 * questions included.
 * Checks: vmv_simplify_multi's in its order, then NULL constraints / constraint_settings, n_constraints other than 1 or
 * n_paths, the settings' and the constraints' own checks in vmv_constraint_project_batch's order
 * (VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the field); then the environments' checks.  A call that fails
 * leaves *out untouched.  Per round one more launch than vmv_simplify_multi: one wave per question slot. */
enum
{
    VMV_SIMPLIFY_OUT_OF_BAND = 2 /* vmv_simplify_multi_constrained: the input's first waypoint or an input edge is out of band */
};
int vmv_simplify_multi_constrained(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                                   const vmv_simplify_settings *settings, const vmv_ee_constraint *constraints,
                                   size_t n_constraints, const vmv_constraint_settings *constraint_settings, vmv_paths **out);
/* refused [n_paths] (may be NULL); VMV_ERR_INVALID_ARGUMENT for paths not made by vmv_simplify_multi_constrained */
int vmv_paths_band_refused(const vmv_paths *paths, uint32_t *refused);

/* ---- clearance-aware path optimisation: many independent paths in one call ------------------ */
/* A covariant gradient iteration (CHOMP's update; its velocity-projection / curvature terms are LEFT OUT) on the
 * waypoints of n_paths paths at once, the arguments those of vmv_simplify_multi: path p is points[offsets[p] ..
 * offsets[p + 1]) in envs[p].  A path of N waypoints keeps its ends x_0, x_{N-1} (their bits are untouched) and N; its
 * n = N - 2 inner waypoints move.  No counterpart in the reference.
 *
 * Cost of an iterate X, fp32:   U = sum over i = 0 .. N-2, ascending from 0.0f, of t_i,
 *     t_i = w_smooth * (0.5f * s_i) + o_i,   s_i = sum over joints j, ascending from 0.0f, of (x_{i+1,j} - x_{i,j})^2,
 *     o_0 = 0,   o_i = w_env * c(env_i; env_margin) + w_self * c(self_i; self_margin) for i >= 1,
 * (env_i, self_i) the two values of vmv_clearance_grad_batch_multi at x_i, c CHOMP's hinge:
 *     c(v; e) = (0 - v) + 0.5f * e for v < 0;  ((v - e) * (v - e)) / (2.0f * e) for 0 <= v <= e;  0 above (+inf, NaN: 0).
 * Gradient at an inner waypoint, per joint, with g^env_i, g^self_i the two gradient rows of that call (the witness held
 * fixed) and c'(v; e) = -1 for v < 0, (v - e) / e for 0 <= v <= e, 0 above:
 *     G_ij = ((w_smooth * (((2.0f * x_ij) - x_{i-1,j}) - x_{i+1,j})) + (w_env * c'(env_i)) * g^env_ij) + (w_self * c'(self_i)) * g^self_ij.
 * Step: per joint column solve A z = G, A the n x n tridiagonal (-1, 2, -1), by the Thomas recurrence on reciprocals
 * r_0 = 0.5f, r_i = 1.0f / (2.0f - r_{i-1}) (computed on the host; IEEE division):
 *     d_0 = G_0, d_i = G_i + r_{i-1} * d_{i-1};   z_{n-1} = d_{n-1} * r_{n-1}, z_i = (d_i + z_{i+1}) * r_i;
 * D = (0 - step) * z;  m = the largest |D_ij| over the whole path (NaN ignored);  scale = max_step / max(m, max_step);
 * x_ij <- clip(x_ij + D_ij * scale) to [lower, lower + span] of vmv_robot_bounds.  The step's size is m * scale.
 * Every operation above is one fp32 operation with one rounding (no contraction), so a path's result depends on its own
 * waypoints, its environment and the settings other than validate_every's effect described below - not on the batch, on
 * the path's place in it, or on the other paths.  tests/optimize_serial.py states the same in numpy float32.
 *
 * Lockstep: all paths share the iteration counter k.  Per iteration ONE vmv_clearance_grad_batch_multi call (d_witness
 * NULL) for the waypoints of all unfinished paths and one step kernel.  Iterates k = 0, v, 2v, ... and k = max_iterations
 * (v = validate_every) are VALIDATED: their N - 1 consecutive edges go through ONE vmv_validate_motion_batch_multi call for
 * all unfinished paths, and an accept kernel keeps a path's BEST: the validated iterate with every edge valid and the
 * smallest U, the first such iterate among equal costs.  A path ends at the first validated iterate k > 0 whose step
 * into it was smaller than min_change, or at k = max_iterations.  The host looks at the finished flags only at
 * validated iterates and compacts the list of unfinished paths there; between two looks nothing synchronises.
 * validate_every therefore chooses WHICH iterates can be returned and where a path can end; the iterates themselves do
 * not depend on it.
 *
 * Result per path: the best iterate's waypoints; status VMV_OPT_OK (a valid iterate is returned), VMV_OPT_NO_VALID (no
 * validated iterate was valid: the input comes back bit for bit) or VMV_OPT_NONFINITE (a non-finite waypoint: the input
 * comes back and no question is asked); iterations run; best_iteration (0 without a best); U of iterate 0 and of the
 * best; the smallest env and self over all N waypoints (-0 below +0, NaN ignored, +inf without a finite value) of
 * iterate 0 and of the best (without a best: iterate 0's figures twice).  Paths of fewer than 3 waypoints come back as
 * they are with 0 iterations, costs 0 and NaN clearances (no clearance question); a finite path of 2 waypoints has its one
 * edge validated: VMV_OPT_OK or VMV_OPT_NO_VALID.  Consequence: a path whose input is valid edge by edge comes back
 * valid edge by edge with cost <= cost_first.  The clearances are those of the WAYPOINTS, validity is
 * vmv_validate_motion_batch's on the consecutive edges, the gradient is the current witness's.
 *
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / points / offsets / settings /
 * out, n_paths >= 2^31, max_waypoints above 1,024, offsets not starting at 0 or decreasing, a path longer than
 * max_waypoints, a NULL handle, step / max_step / env_margin / self_margin not finite or not positive, a weight negative
 * or not finite, min_change NaN, validate_every == 0, offsets[n_paths] >= 2^31 (all VMV_ERR_INVALID_ARGUMENT); an
 * environment holding a point cloud or an attachment, refused as vmv_clearance_batch_multi refuses it
 * (VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the kind and the index; before the finalized check); an unfinalized
 * environment (VMV_ERR_NOT_FINALIZED); an environment of another device (VMV_ERR_INVALID_ARGUMENT).  A call that fails
 * leaves *out untouched.  n_paths == 0 is VMV_OK with an empty result.  Environments not yet prepared for the robot are
 * prepared in one batch.  Synchronous, host buffers, on the default stream; repeated handles are allowed.
 * Device memory per call: 4 copies of the waypoints, their clearances [2] and gradients [2][dim], the edges twice. */
enum
{
    VMV_OPT_OK = 0,
    VMV_OPT_NO_VALID = 1,
    VMV_OPT_NONFINITE = 2
};
typedef struct
{
    uint32_t max_iterations; /* 0 = default (64) */
    uint32_t validate_every; /* iterations between two validated iterates; must not be 0 (the study's default: 8) */
    float step;              /* > 0 (1/40) */
    float max_step;          /* > 0: cap on the largest joint change of one iteration over the whole path (0.1) */
    float min_change;        /* a path ends once a step is smaller than this (1e-4); <= 0: only max_iterations ends it */
    float smooth_weight, env_weight, self_weight; /* >= 0 (1, 1, 1) */
    float env_margin, self_margin;                /* > 0, metres (0.05, 0.01) */
    uint32_t max_waypoints;  /* cap on a path's waypoints, at most 1,024; 0 = default (1,024) */
} vmv_optimize_settings;
typedef struct vmv_optimized vmv_optimized;
int vmv_optimize_multi(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                       const vmv_optimize_settings *settings, vmv_optimized **out);
/* Per path (arrays of n_paths, any may be NULL): status (VMV_OPT_*), iterations, best_iteration, cost_first, cost,
 * clearance_first [n][2] and clearance [n][2] (env, self).  Totals (may be NULL): the clearance-gradient calls and the
 * validation calls the whole call made. */
int vmv_optimized_summary(const vmv_optimized *result, uint8_t *status, uint32_t *iterations, uint32_t *best_iteration,
                          float *cost_first, float *cost, float *clearance_first, float *clearance,
                          uint64_t *clearance_calls, uint64_t *validation_calls);
/* every path's waypoints, packed in path order with the input's offsets; VMV_ERR_CAPACITY if capacity_floats is too
 * small (nothing is written) */
int vmv_optimized_points(const vmv_optimized *result, float *out, size_t capacity_floats);
int vmv_optimized_destroy(vmv_optimized *result);

/* ---- clearance-aware path optimisation under end-effector constraints ----------------------- */
/* vmv_optimize_multi inside the band of an end-effector constraint: the arguments are vmv_optimize_multi's, then one
 * constraint for every path or one per path (n_constraints = 1 or n_paths) and the vmv_constraint_settings of the
 * vmv_constraint_*_batch calls.  The contract per path is vmv_optimize_multi's - the same U, gradient, Thomas solve, cap,
 * clip, lockstep counter and validate_every rule, fp32 with one rounding per operation - with four changes:
 *  1. The input is looked at first.  A path with a non-finite waypoint ends VMV_OPT_NONFINITE as before.  Of a finite path
 *     of N >= 2 both end waypoints are band-tested: vmv_constraint_check_batch's answer under the path's constraint and
 *     constraint_settings.  For N >= 3 every inner waypoint is projected: vmv_constraint_project_batch's lane bit for bit
 *     (a row already in the band and inside the joint bounds comes back unchanged with 0 evaluations).  Iterate 0 is the
 *     input with its inner waypoints replaced by their projections.  An end out of band, or an inner waypoint whose
 *     projection does not converge, ends the path VMV_OPT_OUT_OF_BAND: it comes back with its input bytes, 0 iterations,
 *     costs 0 and NaN clearances, asks no question and does not disturb the other paths, which run as in a call of their
 *     own.  Paths of fewer than 2 waypoints come back as they are without any test.
 *  2. Every new iterate is projected.  The step gives x'_i = clip(x_i + D_i * scale) as in vmv_optimize_multi; then every
 *     inner waypoint becomes project(x'_i) where that projection converged, and keeps its value of iterate k where it did
 *     not (that value is in the band by induction; the waypoint is HELD).  U, the clearances and the gradient of iterate
 *     k + 1 are those of the projected waypoints.  The step's size for the min_change rule stays m * scale, computed before
 *     the projection.  There is no bound on how far a projection moves a waypoint: max_step bounds the step, and the
 *     validated edges bound what is returned.
 *  3. A validated iterate's question for edge (a, b) is validate_motion(a, b) AND band_edge(a, b), band_edge being
 *     vmv_constraint_check_motion_batch's answer: the same samples, check_step and 1,024-sample cap.  A path's best is the
 *     validated iterate whose edges all answer 1 with the smallest U, the first among equals.  A finite path of 2 waypoints
 *     with both ends in band has its one edge asked this way: VMV_OPT_OK or VMV_OPT_NO_VALID.
 *  4. Results as in vmv_optimized_summary, and vmv_optimized_held: per path the number of (iteration, inner waypoint)
 *     projections that did not converge over the iterations the path ran - the steps out of iterates 0 .. iterations - 1 -
 *     so it does not depend on the batch.  VMV_OPT_NO_VALID returns the input's bytes, not iterate 0.
 * Consequences: every waypoint of every iterate is in the band; every edge of a VMV_OPT_OK result has been asked afresh,
 * so vmv_validate_motion_batch and vmv_constraint_check_motion_batch answer 1 for each of them; an input whose waypoints
 * are all in the band and whose edges are all valid and in band comes back the same way with cost <= cost_first.  With a
 * constraint that restricts nothing (all bounds infinite, max_angle 0) and finite input inside the joint bounds the result
 * is vmv_optimize_multi's byte for byte, clearance_calls and validation_calls included, and held is 0.
 * Checks: vmv_optimize_multi's argument checks in its order, then NULL constraints / constraint_settings, n_constraints
 * other than 1 or n_paths, the settings' and the constraints' own checks in vmv_constraint_project_batch's order
 * (VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the field); then the environments' checks as in vmv_optimize_multi (a
 * point cloud or an attachment, unfinalized, another device).  None needs a device.  A call that fails leaves *out untouched.  Per iteration one more launch than vmv_optimize_multi
 * (one lane per waypoint of the unfinished paths), per validated iterate one more (one wave per edge), and two launches
 * and one synchronisation for the look at the input.  With one constraint per path the edge band test reads one 136-byte
 * record per edge; the per-iteration kernel reads one per path. */
enum
{
    VMV_OPT_OUT_OF_BAND = 3 /* vmv_optimize_multi_constrained: an end out of band or an inner waypoint that cannot be projected */
};
int vmv_optimize_multi_constrained(int robot, const vmv_env *const *envs, size_t n_paths, const float *points, const size_t *offsets,
                                   const vmv_optimize_settings *settings, const vmv_ee_constraint *constraints,
                                   size_t n_constraints, const vmv_constraint_settings *constraint_settings, vmv_optimized **out);
/* held [n_paths] (may be NULL); VMV_ERR_INVALID_ARGUMENT for results not made by vmv_optimize_multi_constrained */
int vmv_optimized_held(const vmv_optimized *result, uint32_t *held);

/* ---- straight-line end-effector motions for many independent problems (no counterpart in the reference) -- */
/* Problem p: a start configuration q0 (starts [n][dim]) and a target frame T1 (targets [n][16], vmv_eefk_batch's layout),
 * in environment envs[p]; envs == NULL is the kinematics-only call (nothing is validated).  The end effector is led from
 * q0's frame to T1 along a straight line in position and a rotation about one fixed axis, pose by pose, every pose
 * tracked by vmv_ik_batch's iteration from the previous waypoint.  All problems are tracked by ONE kernel launch, one
 * lane per problem.
 *   Start frame: T0 = the frame vmv_eefk_batch gives q0, bit for bit.
 *   Line (host, float64 from the fp32 frames): dp = p1 - p0; (a, theta), theta in [0, pi], the axis and angle of R0^T R1:
 *     theta = atan2(|v|, (tr - 1) / 2), v = 1/2 (R21 - R12, R02 - R20, R10 - R01); a = v / |v| while (tr - 1) / 2 >= -1/2,
 *     beyond that from the symmetric part: the largest column of 1/2 (R + R^T) - cos(theta) I, normalised, signed like v;
 *     |v| < 1e-12: a = (0, 0, 1).  With position_only theta = 0.  Segments m = max(1, ceil(|dp| / pos_step),
 *     ceil(theta / rot_step)).  m + 1 > max_waypoints: status VMV_CART_TOO_LONG, nothing is tracked or asked.
 *   Pose k = 1 .. m (device, fp32, one rounding per operation): s = float(k) / float(m); p0 + s * dp;
 *     R0 * Rot(a, s * theta), Rot by Rodrigues' formula with c = vcos(s theta), n = vsin(s theta) (the kernels' own sine
 *     and cosine), u = (1 - c) * a: Rot_rr = c + u_r * a_r, Rot_rc = u_r * a_c -/+ n * a_t; every 3-term product as
 *     ((x0 y0 + x1 y1) + x2 y2).
 *   Tracking: waypoint k is what vmv_ik_batch's iteration (its error, weights, damping schedule, bound-hold rule, max_step
 *     and clip to [lower, lower + span]; include above) gives from waypoint k - 1 towards pose k within max_iterations
 *     evaluations after the first.  It is accepted if it converged (pos_tol, rot_tol; with position_only pos_tol alone)
 *     and max_j |q_k - q_{k-1}| <= max_joint_step; otherwise the path stops at waypoint k - 1 with VMV_CART_IK_FAILED or
 *     VMV_CART_JOINT_JUMP.  evaluations counts every evaluation after a waypoint's first, over all waypoints.
 *   Validation (envs != NULL), after tracking: the starts of all tracked problems in ONE vmv_validate_batch_multi call,
 *     every tracked edge (q_{k-1}, q_k) of every problem in ONE vmv_validate_motion_batch_multi call, each problem in its
 *     own environment.  A start that is not valid: VMV_CART_INVALID_START, achieved 0.  Otherwise the path is cut in
 *     front of its first invalid edge (VMV_CART_COLLISION).
 *   A non-finite entry of a start or a target, or a finite start so large that vmv_eefk_batch gives it no finite frame:
 *     VMV_CART_NON_FINITE, one waypoint (the start as passed), nothing tracked or asked.
 * Result per problem: status; segments = m (0 for VMV_CART_NON_FINITE); achieved = the segments kept; evaluations; the
 * achieved + 1 waypoints, the first being q0's bits.  Totals: the validation calls made (0 .. 2) and the questions asked
 * (starts + edges).  A problem's result depends on its own start, target, environment and the settings alone, bit for
 * bit - not on the batch or its place in it.
 * Checks before anything is launched, device-free ones first: unknown robot; NULL starts / targets / settings /
 * out; the settings in the struct's order (a non-finite value, max_iterations >= 2^30, max_waypoints above
 * 1,024, position_only other than 0 / 1); n >= 2^31; then, with envs, vmv_validate_batch_multi's checks of the handles
 * (NULL, finalized) with its messages (all VMV_ERR_INVALID_ARGUMENT but VMV_ERR_NOT_FINALIZED); n == 0 is VMV_OK with an
 * empty result and no device; a device at all; the environments' device and the robot's parts (built in one batch).  A call
 * that fails leaves *out untouched.  Synchronous, host buffers, default stream; repeated handles are allowed. */
enum
{
    VMV_CART_COMPLETE = 0,
    VMV_CART_IK_FAILED = 1,
    VMV_CART_JOINT_JUMP = 2,
    VMV_CART_COLLISION = 3,
    VMV_CART_INVALID_START = 4,
    VMV_CART_TOO_LONG = 5,
    VMV_CART_NON_FINITE = 6
};
typedef struct
{
    float pos_step, rot_step; /* metres, radians per segment; <= 0: default (0.01, 0.05) */
    uint32_t max_iterations;  /* evaluations per waypoint after the first; 0: default (16); below 2^30 */
    float pos_tol, rot_tol;   /* <= 0: default (1e-4, 1e-3) */
    float rot_weight;         /* <= 0: default (0.25) */
    float damping;            /* <= 0: default (1e-2) */
    float max_step;           /* <= 0: default (0.5) */
    float max_joint_step;     /* largest joint change between two waypoints; <= 0: default (0.3) */
    uint32_t max_waypoints;   /* cap on m + 1, at most 1,024; 0: default (1,024) */
    int position_only;        /* 0 / 1 */
} vmv_cartesian_settings;
typedef struct vmv_cartesian vmv_cartesian;
int vmv_cartesian_multi(int robot, const vmv_env *const *envs /* [n] or NULL */, size_t n, const float *starts /* [n][dim] */,
                        const float *targets /* [n][16] */, const vmv_cartesian_settings *settings, vmv_cartesian **out);
/* Per problem (arrays of n, any may be NULL): status (VMV_CART_*), segments, achieved, evaluations.  Totals (may be NULL). */
int vmv_cartesian_summary(const vmv_cartesian *result, uint8_t *status, uint32_t *segments, uint32_t *achieved,
                          uint32_t *evaluations, uint64_t *validation_calls, uint64_t *questions);
/* every problem's achieved + 1 waypoints, packed in problem order; VMV_ERR_CAPACITY if capacity_floats is too small
 * (nothing is written) */
int vmv_cartesian_points(const vmv_cartesian *result, float *out, size_t capacity_floats);
int vmv_cartesian_destroy(vmv_cartesian *result);

/* ---- time-optimal trajectories along many independent paths (no counterpart in the reference) ----------- */
/* Path p: waypoints points[offsets[p] .. offsets[p+1]) ([dim] each), in environment envs[p]; envs == NULL: nothing is
 * validated.  vel_limits, acc_limits: [dim], finite and > 0 (no robot model here carries any).  Per path the call gives a
 * C1 path of straight pieces with parabolic blends at the corners, the time-optimal rest-to-rest velocity profile along it
 * under |qdot_j| <= vel_limits[j] (at the grid points) and |qddot_j| <= acc_limits[j] (everywhere), and that trajectory
 * sampled every dt.  No jerk limits, no torque limits, no non-zero end velocities.
 *   Set-up (host, float64 from the fp32 waypoints): a waypoint equal to its predecessor is dropped; edge lengths L_e are L2
 *     norms summed over the joints in order, u_e the unit directions; blend half-length d_i = min(blend, L_{i-1} / 2,
 *     L_i / 2) at every inner waypoint, 0 with stop_at_waypoints.  Pieces in order: the line of edge e from w_e + d_e u_e,
 *     span L_e - d_e - d_{e+1}, left out when it is not above 1e-9; the blend at waypoint i (d_i > 0) from w_i - d_i u_in,
 *     span 2 d_i, q(s) = base + u_in s + 1/2 q'' s^2 with q'' = (u_out - u_in) / (2 d_i).  A corner with d_i = 0 is a stop
 *     point, as are the first and the last grid point.  Every piece is cut into n = max(2, ceil(span / grid_step)) equal
 *     intervals; N = their sum; N > max_grid: VMV_RETIME_TOO_LONG.  The piece records (base, u_in, u_out, d, span, n,
 *     first grid index, stop flag) go to the device rounded to fp32.
 *   Profile (device, fp32, one rounding per written operation; x = sdot^2, u = sddot constant per interval): per piece
 *     Delta = span / float(n), q''_j = (u_out_j - u_in_j) / (d + d) (0 on a line); interval k of a piece has s0 =
 *     float(k) Delta, s1 = float(k + 1) Delta, tangents a0 = u_in + q'' s0, a1 = u_in + q'' s1.  Per joint two constraints
 *     |c u + e x| <= A_j with (c, e) = (a0_j, q''_j) and (a1_j + (2 Delta) q''_j, q''_j): with |c| > 1e-6 the band
 *     |u - s x| <= g, s = (-e) / c, g = A_j / |c|; else, with e != 0, the cap x <= A_j / |e|.  Velocity caps
 *     (V_j / |a_j|)^2 over both tangents that meet at a grid point and have |a_j| > 1e-6; 0 at a stop point.  The reach
 *     lines are u >= -x / (2 Delta) and u <= (K_{i+1} - x) / (2 Delta).  Backward from K_N = 0: K_i = max(0, min(caps,
 *     velocity caps, (g_p + g_q) / (s_p - s_q) over all bands with s_p - s_q > 0, and the reach lines against every band
 *     with both sides of the quotient multiplied by 2 Delta, so that an interval of 1e-9 costs no digit:
 *     (g_q (2 Delta)) / (-1 - s_q (2 Delta)) where that denominator is > 0, (K_{i+1} + g_p (2 Delta)) / (1 + s_p (2 Delta))
 *     where that is > 0)).  A minimum of non-NaN values does not depend on its order.  Forward from x_0 = 0: u_i =
 *     max(min(min_q (g_q + s_q x), (K_{i+1} - x) / (2 Delta)), max(max_p (s_p x - g_p), (-x) / (2 Delta))), x_{i+1} =
 *     min(max(x + (2 Delta) u_i, 0), K_{i+1}), T_{i+1} = T_i + (2 Delta) / (sqrt(x_i) + sqrt(x_{i+1})).  u_i stays the
 *     value chosen (it is NOT recomputed from x_{i+1} - x_i: on a line of 1e-8 between two blends one ulp of x over
 *     2 Delta is several times the acceleration limit).  A non-finite time: VMV_RETIME_STALLED.
 *   Samples: samples = ceil(T / dt) + 1 in float64; above max_samples: VMV_RETIME_TOO_LONG.  Sample k (device, fp32):
 *     t = min(float(k) dt, T); i = the last interval with T_i <= t; tau = t - T_i; sigma = min(max(sqrt(x_i) tau +
 *     (u_i / 2) (tau tau), 0), Delta); s = s0 + sigma; x(s) = max(x_i + (u_i + u_i) sigma, 0); position (base + u_in s) +
 *     (q'' / 2) (s s); velocity q'(s) sqrt(x(s)) with q'(s) = u_in + q'' s; acceleration q'(s) u_i + q'' x(s).  Row 0 and
 *     the last row carry the first and the last waypoint's own bits, with zero velocity.
 *   Validation (envs != NULL): all consecutive sample pairs of all sampled paths in ONE
 *     vmv_validate_motion_batch_multi call, each path in its own environment; a path with an invalid pair is
 *     VMV_RETIME_COLLISION with first_invalid = the first invalid pair's index.  The samples are returned whole.
 *   A NaN or infinite waypoint: VMV_RETIME_NON_FINITE.  A path without waypoints: no samples; a path of one distinct
 *     waypoint (or one whose lines are all at most 1e-9 long): one sample, duration 0, VMV_RETIME_COMPLETE.  Paths that
 *     are TOO_LONG, NON_FINITE or STALLED have no samples.
 * A path's result depends on its own waypoints, environment, the limits and the settings alone, bit for bit - not on the
 * batch or its place in it.
 * Checks before anything is launched, device-free ones first, vmv_last_error() names the argument: unknown robot; NULL
 * settings / out / vel_limits / acc_limits / offsets; blend, grid_step or dt NaN or infinite; grid_step or dt in (0, 1e-6);
 * max_grid above 4,096; stop_at_waypoints other than 0 / 1; a limit that is not finite and > 0; n >= 2^31; offsets[0] != 0
 * or decreasing offsets; 2^31 waypoints or more; NULL points with waypoints (all VMV_ERR_INVALID_ARGUMENT); then, with
 * envs, vmv_validate_batch_multi's checks of the handles (NULL, finalized) with its messages; n == 0 is VMV_OK with an
 * empty result and no device; a device at all; the environments' device and the robot's parts (built in one batch).  A call
 * that fails leaves *out untouched.  Synchronous, host buffers, default stream; repeated handles are allowed. */
enum
{
    VMV_RETIME_COMPLETE = 0,
    VMV_RETIME_COLLISION = 1,
    VMV_RETIME_TOO_LONG = 2,
    VMV_RETIME_NON_FINITE = 3,
    VMV_RETIME_STALLED = 4,
    VMV_RETIME_OUT_OF_BAND = 5 /* vmv_retime_multi_constrained only: the first failing sample pair is valid and leaves the band */
};
#define VMV_RETIME_NONE 0xffffffffu /* first_invalid of a path without an invalid sample pair */
typedef struct
{
    float blend;           /* largest blend half-length, in joint-space distance; <= 0: default (0.1) */
    float grid_step;       /* largest interval of the profile's grid; <= 0: default (0.02); else at least 1e-6 */
    float dt;              /* sampling period in seconds; <= 0: default (0.01); else at least 1e-6 */
    uint32_t max_grid;     /* cap on a path's intervals, at most 4,096; 0: default (4,096) */
    uint32_t max_samples;  /* cap on a path's samples; 0: default (65,536) */
    int stop_at_waypoints; /* 0 / 1: no blends, the trajectory rests at every waypoint and stays on the polyline */
} vmv_retime_settings;
typedef struct vmv_trajectories vmv_trajectories;
int vmv_retime_multi(int robot, const vmv_env *const *envs /* [n] or NULL */, size_t n, const float *points,
                     const size_t *offsets /* [n + 1] */, const float *vel_limits /* [dim] */, const float *acc_limits /* [dim] */,
                     const vmv_retime_settings *settings, vmv_trajectories **out);
/* Per path (arrays of n, any may be NULL): status (VMV_RETIME_*), intervals, samples, duration, first_invalid.  Totals (may
 * be NULL): the validation calls made (0 or 1) and the sample pairs asked. */
int vmv_retime_summary(const vmv_trajectories *result, uint8_t *status, uint32_t *intervals, uint32_t *samples, float *duration,
                       uint32_t *first_invalid, uint64_t *validation_calls, uint64_t *questions);
/* every path's samples, packed in path order: times [S], positions, velocities, accelerations [S][dim]; VMV_ERR_CAPACITY
 * if capacity_samples is below S (nothing is written) */
int vmv_retime_samples(const vmv_trajectories *result, float *times, float *positions, float *velocities, float *accelerations,
                       size_t capacity_samples);
int vmv_retime_destroy(vmv_trajectories *result);

/* ---- retiming that repairs its own blends: valid and inside the band -------------------------------- */
/* vmv_retime_multi with a level h_i in 0 .. H + 1 (H = blend_halvings) at every corner (inner distinct waypoint), all 0 at
 * the start, all H + 1 with base.stop_at_waypoints.  The blend half-length, float64: d_i = min(blend, L_{i-1} / 2, L_i / 2)
 * 2^-h_i for h_i <= H (an exact scaling: every level halves, also where the edge length clamps) and 0 at H + 1, which is
 * the stop vmv_retime_multi makes of a corner with d_i = 0.  Set-up, profile and samples are otherwise vmv_retime_multi's.
 * constraints: NULL / n_constraints 0 (no band), one for all paths, or one per path; constraint_settings as in
 * vmv_constraint_check_motion_batch (needed with constraints).  Rounds, all unfinished paths together:
 *   1. set-up with the path's levels (host), retime_profile_kernel, retime_sample_kernel; TOO_LONG, STALLED and NON_FINITE
 *      by vmv_retime_multi's rules - in a later round too, since smaller blends change the interval count - end the path
 *      with that status and no samples.  Rows 0 and last become the end waypoints at rest, as in vmv_retime_multi.
 *   2. every consecutive pair of the samples as returned gets two answers: valid = validate_motion's in the path's
 *      environment (1 without envs), band = vmv_constraint_check_motion_batch's under the path's constraint (the same
 *      samples, check_step and sample cap, bit for bit; 1 without constraints).  The pair fails where valid AND band is 0.
 *   3. with piece(k) the piece sample k was evaluated on (the last interval with T_i <= t, then the last piece with first
 *      <= i), a failing pair k blames every blend piece in [piece(k), piece(k + 1)]; a blend piece is one corner's.
 *   4. no failing pair: VMV_RETIME_COMPLETE.  Some failing pair that blames no blend (it lies on lines and stops, no level
 *      moves it), or round max_rounds: the path ends with first_invalid = its first failing pair and VMV_RETIME_COLLISION
 *      where that pair's valid is 0, else VMV_RETIME_OUT_OF_BAND; the samples come back whole.  Otherwise every blamed
 *      corner's level goes up by one and the path takes another round.
 * Everything reported is the last round's; `questions` counts the pairs put to step 2 and validation_calls the
 * vmv_validate_motion_batch_multi calls, over all rounds.  A path's result depends on its own waypoints, environment,
 * constraint, the limits and the settings alone, bit for bit.  Hence: every COMPLETE result passes validate_motion and the
 * band test on every returned pair; where vmv_retime_multi is COMPLETE (and no constraint restricts) the result is its
 * bytes, rounds 1, levels 0; where round 1's failing pairs include one that blames no blend the result is round 1's, which
 * without constraints is vmv_retime_multi's COLLISION, first_invalid and bytes; a path whose corners are all at H + 1 has
 * the samples of vmv_retime_multi with stop_at_waypoints.
 * Corners are repaired, edges are not: a failing pair on a line ends the path.  A blend at a lower level is not proven
 * faster than a stop.  blend_halvings 3 and max_rounds 8 are choices, not measurements.
 * On the device per round: the samples stay there and vmv_validate_motion_batch_multi and retime_band_kernel (one lane per
 * pair) read them in place, one segment per path; retime_blame_kernel (one wave per path) makes the round record - first
 * failing pair, what failed there, the ended flag, the blamed pieces - which, with the grid times, is all that comes to the
 * host; a path's samples are downloaded once, in the round it ends.
 * Checks: vmv_retime_multi's, in its order, on `base`; blend_halvings above 8; n_constraints neither 0, 1 nor n; with
 * constraints, NULL constraints / constraint_settings, then vmv_constraint_project_batch's checks of the settings and of
 * every constraint (all VMV_ERR_INVALID_ARGUMENT, vmv_last_error() names the argument); the rest as vmv_retime_multi.  A
 * call that fails leaves *out untouched.  The result is a vmv_trajectories: vmv_retime_summary, vmv_retime_samples and
 * vmv_retime_destroy read it unchanged. */
typedef struct
{
    vmv_retime_settings base;
    uint32_t blend_halvings; /* H: levels that halve a corner's blend before the stop; 0: default (3); at most 8 */
    uint32_t max_rounds;     /* rounds before an unfinished path ends; 0: default (8) */
} vmv_retime_constrained_settings;
int vmv_retime_multi_constrained(int robot, const vmv_env *const *envs /* [n] or NULL */, size_t n, const float *points,
                                 const size_t *offsets /* [n + 1] */, const float *vel_limits /* [dim] */,
                                 const float *acc_limits /* [dim] */, const vmv_ee_constraint *constraints /* NULL, 1 or n */,
                                 size_t n_constraints, const vmv_retime_constrained_settings *settings,
                                 const vmv_constraint_settings *constraint_settings, vmv_trajectories **out);
/* Any may be NULL.  levels: one byte per input waypoint (offsets[n] of them), the corner's level of the last round, 0 for
 * the ends and for dropped duplicates; per path: rounds taken, repaired = corners with level > 0, stops = corners at
 * H + 1.  A result of vmv_retime_multi is refused (VMV_ERR_INVALID_ARGUMENT). */
int vmv_retime_levels(const vmv_trajectories *result, uint8_t *levels, uint32_t *rounds, uint32_t *repaired, uint32_t *stops);

/* ---- lockstep AORRTC: cost-bounded RRT-Connect searches for many independent problems --------------------- */
/* AORRTC (planning/aorrtc.hh, one goal, PHS sampling, no dynamic domain) for n_problems problems at once; the arguments
 * are those of vmv_rrtc_multi.  Per problem:
 *   1. a first solution by vmv_rrtc_multi's contract with max_iterations and max_samples of these settings (rrtc's own two
 *      maxima are overwritten, aorrtc.hh:384-386), on the Halton samples halton_skips[p] + 1, ...; unsolved: the problem
 *      ends with that status and no path;
 *   2. with simplify_intermediate, the path simplified by vmv_simplify_multi's contract under `simplify` (a path of more
 *      than simplify.max_waypoints waypoints stays as it is);
 *   3. first_cost = cost = Path::cost (the fp32 sum of the segment lengths in order); without `optimize`, or with a path
 *      of 2 waypoints, the problem ends here;
 *   4. while iterations < max_iterations, cost - distance(start, goal) > 1e-8f and (max_searches == 0 or searches <
 *      max_searches): one cost-bounded search below `cost` with a budget of min(max_iterations - iterations,
 *      max_internal_iterations) iterations on fresh trees; ++searches, iterations += the search's; a solution is
 *      simplified as in 2. and, if its cost < cost, becomes the path (++improvements);
 *   5. VMV_PLAN_SOLVED with the best path; iterations of all stages; sizes2 = the trees of the last search run.
 * A search (DESIGN 5f gives every operation; fp32, one rounding per written operation, + - * / sqrtf and integer
 * operations only): samples drawn directly from the prolate hyperspheroid of the bound with foci start and goal - a
 * counter-based 32-bit hash seeded with (uint32) halton_skips[p] for the uniforms, a polynomial ln, Marsaglia's polar
 * method, a Householder reflection - and rejected outside the joint bounds; the nearest node by the asymmetric
 * cost-space key of aorrtc.hh:61-85 as an associative argmin (the first of the least key among the admissible nodes);
 * with cost_bound_resample up to max_cost_bound_resamples attempts to re-parent the new node under a resampled cost
 * bound (aorrtc.hh:197-237); the connect march of vmv_rrtc_multi towards the other tree's nearest node where that can
 * beat the bound.  A problem's result depends on its own inputs and the settings other than check_every alone, bit for
 * bit.  Search g of every still-optimising problem is one lockstep call (one 256-thread workgroup per unfinished problem
 * and one edge question per problem per round, as vmv_rrtc_multi); the first solutions and the simplifications of a
 * generation are one vmv_rrtc_multi / vmv_simplify_multi call each over the problems concerned; the host compares costs.
 * Each problem owns a pool of max_samples nodes on the device (max_samples * (dimension + 2) * 4 bytes).
 * Checks before anything is launched, device-free ones first: those of vmv_rrtc_multi (n_problems >= 2^25 is refused
 * here), max_internal_iterations == 0, max_cost_bound_resamples > 64, the simplifier's settings as vmv_simplify_multi
 * checks them (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment (VMV_ERR_NOT_FINALIZED); an environment of another
 * device (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out untouched.  n_problems == 0 is VMV_OK with an empty
 * result.  A start or goal with a non-finite joint: that problem ends unsolved.  Synchronous, host buffers, on the
 * default stream; repeated handles are allowed.  The result is a vmv_plans: vmv_plans_summary (rounds and questions
 * count every stage), vmv_plans_paths, vmv_plans_destroy, and vmv_plans_costs below. */
typedef struct
{
    vmv_rrtc_settings rrtc;          /* range, balance, tree_ratio, check_every; its two maxima are overwritten */
    vmv_simplify_settings simplify;
    int optimize;                    /* 0: first solution (+ simplification) only */
    int cost_bound_resample;         /* 0 / 1 */
    int simplify_intermediate;       /* 0 / 1 */
    uint32_t max_iterations;         /* of all stages together */
    uint32_t max_internal_iterations; /* of one cost-bounded search; > 0 */
    uint32_t max_samples;            /* nodes of a problem's two trees together, in every stage */
    uint32_t max_cost_bound_resamples; /* <= 64 */
    uint32_t max_searches;           /* cost-bounded searches per problem; 0 = no limit but max_iterations */
} vmv_aorrtc_settings;
int vmv_aorrtc_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                     const uint64_t *halton_skips, const vmv_aorrtc_settings *settings, vmv_plans **out);
/* Per problem of a vmv_aorrtc_multi or vmv_aorrtc_multi_constrained result (arrays of n_problems, any may be NULL): the cost after the first stage, the
 * cost of the returned path (+inf = unsolved), the cost-bounded searches run, those that gave a cheaper path.
 * VMV_ERR_INVALID_ARGUMENT on the plans of another call. */
int vmv_plans_costs(const vmv_plans *plans, float *first_costs, float *costs, uint32_t *searches, uint32_t *improvements);

/* ---- lockstep AORRTC under end-effector constraints ----------------------------------------- */
/* vmv_aorrtc_multi inside the band of an end-effector constraint: its arguments, then one constraint for every problem or
 * one per problem (n_constraints = 1 or n_problems) and vmv_rrtc_multi_constrained's plan settings.  The contract per
 * problem is vmv_aorrtc_multi's meta loop with these substitutions and nothing else:
 *   1. The first solution is vmv_rrtc_multi_constrained's with one goal, dynamic domain and start_tree_first off and the
 *      two maxima of these settings.  A start or goal out of band: VMV_PLAN_INVALID_ENDPOINT, no question, no path,
 *      first_cost = cost = +inf, searches = 0.
 *   2. Every simplification is vmv_simplify_multi_constrained's under the same constraint and constraint_settings->base.
 *      A path longer than simplify.max_waypoints stays as it is; so does one that comes back VMV_SIMPLIFY_OUT_OF_BAND,
 *      whose cost is then that of the unsimplified path.
 *   3. A search is vmv_aorrtc_multi's with three kinds of question.  An extension near -> new and a march step from -> w
 *      end in a NEW node, which gets vmv_rrtc_multi_constrained's treatment: it is projected
 *      (vmv_constraint_project_batch's lane, bit for bit), accepted only if the projection converged and lies within
 *      max_stretch * range of the question's near end, written back to the tree and to the question, and then the edge's
 *      band test (vmv_constraint_check_motion_batch's) is ANDed into validity; refused, the node stays as written and the
 *      answer is 0.  A re-parent question A[mi] -> new has no new node - `new` is projected already - and is band-checked
 *      only: the stretch rule does not apply to it (its near end is a nearest node in cost space).  The null questions are
 *      band-checked only (start -> start).  The closing step of a march is not asked, as in vmv_rrtc_multi.
 *      Whatever is derived from a new node - new_cost, g2, a march node's cost = cost[prev] + dist(w, prev) - is computed
 *      after the answer, from the projected point.  The PHS sample itself is never projected.
 * The result is a vmv_plans as vmv_aorrtc_multi's; vmv_plans_costs reads it, and vmv_plans_band_refused gives per problem
 * the first stage's count + the searches' questions the constraint answered 0 + every simplification's
 * vmv_paths_band_refused.  rounds and questions count every stage.  A problem's result is its own, bit for bit, whatever
 * the batch, its order and check_every.  With a constraint that restricts nothing the result is vmv_aorrtc_multi's byte for
 * byte, rounds and questions included, while every node lies inside the joint bounds.
 * NOT promised: as in vmv_simplify_multi_constrained the halves of a subdivided edge are not asked again, so a returned
 * path lies on asked in-band edges or on halves of them, and a fresh sampling of its edges
 * (vmv_constraint_check_motion_batch over the returned waypoints) may still answer 0 for some.  Only the end-effector
 * frame can be constrained.
 * Checks, all before any device call: vmv_aorrtc_multi's in its order, then vmv_rrtc_multi's remaining ones and the
 * constraint's own as vmv_rrtc_multi_constrained makes them ("null pointer", n_constraints, the settings, max_stretch, every
 * constraint; vmv_last_error() names the check); then the environments' checks.  A call that fails leaves *out untouched.
 * Per round of a search one more launch than vmv_aorrtc_multi: one wave per question. */
int vmv_aorrtc_multi_constrained(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                                 const uint64_t *halton_skips, const vmv_aorrtc_settings *settings,
                                 const vmv_ee_constraint *constraints /* host, [n_constraints] */, size_t n_constraints,
                                 const vmv_constraint_plan_settings *constraint_settings, vmv_plans **out);

/* ---- lazy complete-graph search: many independent problems in one call ----------------------------------- */
/* A* over the complete graph of a problem's valid samples with every unchecked edge taken as free, for n_problems problems
 * at once; the arguments are those of vmv_prm_multi (starts, goals, envs, halton_skips or the caller's `samples`).  The
 * vertices of all problems go through ONE vmv_validate_batch_multi call (vmv_prm_multi's layout); then the problems
 * advance in lockstep rounds like those of vmv_rrtc_multi: per round a step kernel (one 256-thread workgroup per unfinished
 * problem; g, h, parents and the open / closed flags of the valid vertices in LDS, the pair state in global memory)
 * writes questions_per_round edge questions per unfinished problem, and one vmv_validate_motion_batch_multi launch
 * sequence answers all of them.
 * Per problem, bit-defined (fp32, one rounding per written operation):
 *   V = n_samples + 2 vertices: 0 = start, 1 = goal, 2 + i = sample i; valid[v] = validate(vertex v) (a non-finite
 *   joint: invalid).  !valid[0] or !valid[1]: VMV_PLAN_INVALID_ENDPOINT, no path, no edge is asked.
 *   d2(u, v) = sum over the joints in order of (u[j] - v[j])^2, w(u, v) = sqrtf(d2(u, v)), h(v) = w(v, 1).
 *   State: a set B of blocked unordered pairs, empty at first, and iterations = 0.
 *   Search (at most V pops): iterations == max_iterations: VMV_PLAN_MAX_ITERATIONS, no path; else ++iterations, g[0] = 0,
 *   every other g = +inf, open = {0}, nothing closed.  Pop the open, not closed vertex u least by (fl(g[u] + h[u]), then
 *   vertex id); none: VMV_PLAN_NO_PATH; u == 1: the path is the parent chain.  Else close u, and for every valid, not
 *   closed v != u with {u, v} not in B: c = fl(g[u] + w(u, v)); c < g[v]: g[v] = c, parent[v] = u, v is open.  A closed
 *   vertex is never reopened.  g[1] is the left-to-right fp32 sum along the path.
 *   Check: the path's edges from the start; the question of {a, b}, a < b, is validate_motion(a -> b).  An edge known
 *   valid is skipped; one answered valid is remembered and the walk goes on; the first one answered invalid enters B and
 *   the search runs again; every edge valid: VMV_PLAN_SOLVED, the path the vertices' stored bits, cost = g[1].
 *   The first proposed path is always [0, 1].
 * A problem's result (status, iterations, path, cost, valid vertices, |B|, edges known valid) depends on its own inputs
 * and max_iterations alone, bit for bit: not on the batch, questions_per_round or check_every.  Slot 0 of a round is the
 * next question the rules above reach, so every round makes progress; the other slots are predictions — the proposed
 * path's later unknown edges, then the first unknown edge of the paths found with the round's questions taken as invalid;
 * none with a problem's first question, the straight edge — whose answers only fill a cache that the walk consults before it asks (a cached invalid answer enters B when the walk
 * reaches that edge).  Unused slots and finished problems ask the null question start -> start.  A problem runs at most
 * 64 searches per round, predictions included; beyond that it asks null questions and carries on in the next round.
 * Agreement with the reference's FCIT* (planning/fcit.hh, an edge-queue search) is not claimed.
 * Device memory per problem: 2 * V * ceil(V / 32) * 4 bytes of pair state (two answer-cache bits and one blocked bit per
 * ordered pair), V * (dimension + 1) * 4 bytes of vertices and path, questions_per_round * (2 * dimension + 2) * 4 bytes
 * of questions; the pair state is 1.07 MB at n_samples = 2,048 and 18.6 KB at 256.
 * The result is a vmv_plans: vmv_plans_summary reports iterations = searches run, sizes2 = [valid vertices, blocked
 * edges], rounds = validation calls made (the vertices' included), questions = edge questions asked (null questions not
 * counted); vmv_plans_paths and vmv_plans_destroy work as for vmv_rrtc_multi.
 * Checks before anything is launched, device-free ones first: unknown robot; NULL envs / starts / goals / settings / out
 * or a NULL handle, n_samples not a multiple of 64 or outside 64 .. 2,048, questions_per_round outside 1 .. 32,
 * max_iterations == 0, halton skip + n_samples > 1,000,000 where samples is NULL, n_problems * V * ceil(V / 32) >= 2^31
 * (the words of one pair-state matrix) or n_problems * questions_per_round >= 2^31 (the questions of a round)
 * (VMV_ERR_INVALID_ARGUMENT); an unfinalized environment (VMV_ERR_NOT_FINALIZED); an environment of another device
 * (VMV_ERR_INVALID_ARGUMENT).  A call that fails leaves *out untouched.  n_problems == 0 is VMV_OK with an empty result.
 * Environments not yet prepared for the robot are prepared in one batch.  Synchronous, host buffers, on the default
 * stream; repeated handles are allowed. */
typedef struct
{
    uint32_t n_samples;
    uint32_t max_iterations;      /* searches per problem; >= 1 */
    uint32_t questions_per_round; /* edge questions per problem per round: 1 .. 32 */
    uint32_t check_every;         /* rounds between two looks of the host at the finished flags; 0 = default */
} vmv_fcit_settings;
int vmv_fcit_multi(int robot, const vmv_env *const *envs, size_t n_problems, const float *starts, const float *goals,
                   const uint64_t *halton_skips, const float *samples, const vmv_fcit_settings *settings, vmv_plans **out);
/* Per problem of a vmv_fcit_multi result (arrays of n_problems, either may be NULL): cost (+inf = unsolved) and the edges
 * the walk found valid.  VMV_ERR_INVALID_ARGUMENT on the plans of another call. */
int vmv_plans_fcit_summary(const vmv_plans *plans, float *costs, uint32_t *known_valid_edges);

/* ---- measurement support (bench.py) ---------------------------------------------------------------------- */
/* Runs vmv_validate_batch `iters` times on `stream` between two HIP events recorded on that same stream and
 * returns the average kernel time in milliseconds. */
int vmv_time_validate_batch(int robot, const vmv_env *env, const float *d_q, size_t n, uint64_t *d_bits, int iters,
                            void *stream, float *avg_ms);
/* fills d_q[n][dimension] with uniform configurations inside the joint bounds (splitmix64 counter RNG) */
int vmv_fill_uniform_configs(int robot, float *d_q, size_t n, uint64_t seed, void *stream);
/* name of the dominant kernel symbol for a robot (to match rocprofv3 --kernel-trace rows) */
const char *vmv_kernel_name(int robot, const char *entry_point);
/* test support: n successive PHS samples of vmv_aorrtc_multi's sampler for the foci start and goal and the bound
 * max_cost, drawn in a kernel from the uniform stream (seed, counter): out_q [n][dimension], out_in_bounds [n] (1 = inside
 * the joint bounds), *out_counter = the counter after the last draw.  Host buffers, synchronous. */
int vmv_phs_samples(int robot, const float *start, const float *goal, float max_cost, uint32_t seed, uint32_t counter, size_t n,
                    float *out_q, uint8_t *out_in_bounds, uint32_t *out_counter);

#ifdef __cplusplus
}
#endif
#endif
