/* include/ssx_test_hooks.h -- hooks of the TESTS and TOOLS of this repository into libssx.so.  NOT part of the product ABI
 * (include/ssx.h): they may change or disappear at any time, and a product build leaves them out altogether
 * (-DSSX_NO_TEST_HOOKS, which `SSX_PRODUCT_BUILD=1 python -m ssvio_amd.build` passes).  The default build carries them because the
 * driver's GPU tests load the very library that ships (tests/test_ba_gpu.py, tests/test_window_host.py, tools/kernel_resources.py,
 * tools/asan_prepare.py). */
#ifndef SSX_TEST_HOOKS_H
#define SSX_TEST_HOOKS_H
#include "ssx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test hook, needs no GPU: `steps` random pushes / pops / removals of observations and landmarks on a window without a device (fix
 * rule 1), its contents, order and fixed flags checked against a plain model after every step, and two twin windows that receive the same edits through ssx_ba_window_update_batch (two windows per call: the
 * threaded path) against the window itself; 0 = all steps agree, else the first step that does not */
SSX_API int32_t ssx_ba_window_selftest(uint32_t seed, int32_t steps);
/* test hook: how often the window's observation storage has been rewritten without its dead entries (tests that need dead entries
 * before and after a rewrite ask it which state they built); -1 = no window */
SSX_API int32_t ssx_ba_window_debug_rewrites(const ssx_ba_window* win);

/* tools hook, needs no GPU: dynamic LDS bytes a BA kernel is launched with (-1: depends on the problem); the compiler's
 * resource report and rocprofv3's dispatch rows only know static __shared__ arrays (tools/kernel_resources.py) */
SSX_API int64_t ssx_debug_kernel_dynamic_lds(const char* kernel);
/* tests hook: 1 = the linearise / Schur kernels write, and the reductions read, every entry of the per-chunk partial sums (round 3's
 * dense slabs); 0 (default) = only the blocks of the reduced system and the poses a chunk contributes to; < 0 = the environment's
 * choice (SSX_BA_DENSE_SLABS).  Same bits either way (tests/test_ba_gpu.py::test_sparse_slabs_equal_dense_slabs); applies to problems
 * uploaded after the call. */
SSX_API void ssx_debug_set_dense_slabs(int32_t mode);

/* tests hook: who completes an LM trial of a small window on one GPU.  1 (default) = the last chunk of k_backsub_residual to publish
 * its three sums adds them and takes the LM step (agent-scope stores + a ticket, no fence); 0 = a launch of k_reduce_trial does (rounds
 * 1-4).  Same bits either way: tests/test_ba_gpu.py::test_trial_finish_litmus. */
SSX_API void ssx_debug_set_trial_finish(int32_t mode);

/* tools hook, needs no GPU: seconds of host marshalling (edge sort by landmark, chunks, index lists) for one problem */
SSX_API double ssx_ba_debug_prepare_seconds(const ssx_ba_problem* prob, int32_t reps);

/* tools / tests hook, needs no GPU: how ssx_ba_solve / ssx_ba_solve_batch would send this problem's observation arrays
 * across PCIe (lossless narrowing): bit 0 = keyframe indices as bytes, bit 1 = landmark indices as 16-bit words, bit 2 =
 * pixel coordinates as floats (every edge_uv value is a float's value, as the reference's cv::KeyPoint::pt measurements
 * are); 0 = as handed over (large windows, SSX_BA_HOST_PREP set); -1 = invalid problem */
SSX_API int32_t ssx_ba_debug_upload_format(const ssx_ba_problem* prob);

/* test hook, needs no GPU: FNV-1a digest of the host marshalling of a LARGE window (per-landmark offsets, every observation's rank
 * inside its landmark, per-keyframe counts, chunk cuts) with the observation pass on `threads` host threads (>= 65 536 observations
 * take it on the worker pool; SSX_BA_PREP_THREADS, default min(8, cores)).  The digest must not depend on `threads`.  0 = invalid. */
SSX_API uint64_t ssx_ba_debug_prepare_digest(const ssx_ba_problem* prob, int32_t threads);

/* tests / tools hook, needs no GPU: the plan of the ORB front-end (pyramid geometry, cell grid, capacities, tilings, cv::resize
 * tables, arena layout) for `images` images of rows x cols, built exactly as the entry points build it but without a device.
 *   status / error   what the entry point would return and ssx_last_error() would show; the rest is filled for SSX_OK only
 *   digest           FNV-1a of [0] every scalar of the device view, [1] every buffer's offset and the arena's bytes, [2] the cell and the two
 *                    resize tables byte for byte (tools/orb_plan_ab.py compares them between two builds of the library)
 *   buf_off / _bytes the arena's buffers in memory order
 * unchecked != 0 skips the argument checks that come first (but for the number of levels, which sizes arrays), so that the refusals
 * behind them can be reached and their order tested. */
typedef struct ssx_orb_plan_info {
  int32_t status, n_buffers;
  uint64_t digest[3];
  uint64_t arena_bytes, buf_off[32], buf_bytes[32];
  int32_t nlevels, out_cap;
  int32_t lvl_rows[8], lvl_cols[8], feat[8], lvl_cell0[9], gauss_tile0[9];
  char error[256];
} ssx_orb_plan_info;
SSX_API ssx_status ssx_orb_debug_plan(int32_t rows, int32_t cols, int32_t images, const ssx_orb_params* prm, int32_t has_mask,
                                      int32_t detect_only, int32_t unchecked, ssx_orb_plan_info* out);

/* ---- kernel taps (moved here from ssx.h in 0.1.20): intermediate results of the kernels, for the parity tests and tools ---- */

/* One linearisation of the problem at its current state (no update): the blocks the kernels build,
 * for kernel-level parity tests and profiling.  Any output may be NULL.
 *   Hpp P x 36 (row-major 6x6), bp P x 6, Hll L x 9, bl L x 3, Hpl E x 18 (6x3 row-major, per edge),
 *   err E x 2, chi2 = robust chi2.  Rows of fixed vertices are zero. */
SSX_API ssx_status ssx_ba_linearize(ssx_ctx* ctx, const ssx_ba_problem* prob, double huber_delta, int32_t jac_mode,
                            double* Hpp, double* bp, double* Hll, double* bl, double* Hpl, double* err,
                            double* chi2);

/* Parity / profiling hooks: copies of intermediate buffers of the LAST ssx_orb_extract / ssx_orb_detect /
 * ssx_stereo_* call on this ctx, image `image` of that call (0 = left / only image, 1 = right ...).
 *   level image (u8, rows x cols returned), blurred level image, and the grid-FAST candidates of a level
 *   (keypoints relative to the 16-px border, reference order = cell-row-major then row-major in the cell). */
SSX_API ssx_status ssx_orb_stage_level(ssx_ctx* ctx, int32_t image, int32_t level, int32_t blurred,
                                       uint8_t* out, int32_t out_cap, int32_t* rows, int32_t* cols);
SSX_API ssx_status ssx_orb_stage_candidates(ssx_ctx* ctx, int32_t image, int32_t level, int32_t cap,
                                            ssx_keypoint* out, int32_t* n);

/* tests hook: k_octree (csrc/octree.hip) on the CALLER'S candidates, no image involved (tests/test_octree_gpu.py,
 * tests/octree_cases.py).  The key (rows, cols, images, prm, detect_only; no mask) is planned as the entry points plan it -- the
 * same build_plan, the same arena, so the same one of the kernel's four builds and the same scratch stride -- and the n candidates,
 * parallel int32 arrays (image, level, x, y, response) with x, y relative to the 16-px border as in cell_cand, are written into
 * the cell lists as k_fast_cells would have left them: each into the one cell whose ROI, less its 3-px frame, holds it, in
 * input order inside a cell.  status and every cell_count are zeroed first; then launch_octree runs as the pipeline calls it and
 * the stream is synchronised.  Outputs (any may be NULL), L = the plan's levels (1 for detect_only):
 *   lvl_ncand, sel_count   images x L (-1 where the kernel wrote nothing)
 *   sel                    images x L x 4096 packed x | y << 12 | response << 24; the first sel_count entries, in list order
 *   status                 per image (bit 0 candidates, bit 1 nodes, bit 2 outputs over capacity)
 * SSX_ERR_INVALID_ARG with text, and nothing launched, for: an image or level out of range, a coordinate outside 0..4095, a
 * response outside 1..255, a candidate in no cell, more than 256 candidates in a cell.  The key's own refusals are the plan's.
 * Afterwards ssx_orb_stage_candidates returns the candidates in reference order, as after a run on an image. */
SSX_API ssx_status ssx_orb_debug_octree(ssx_ctx* ctx, int32_t rows, int32_t cols, int32_t images, const ssx_orb_params* prm,
                                        int32_t detect_only, int32_t n, const int32_t* image, const int32_t* level, const int32_t* x,
                                        const int32_t* y, const int32_t* response, int32_t* lvl_ncand, int32_t* sel_count,
                                        uint32_t* sel, int32_t* status);

/* Test access to the pyramids (which = 0 previous, 1 next) and the Scharr images (int16 dx, dy interleaved) of
 * the last ssx_lk_track call. */
SSX_API ssx_status ssx_lk_stage_level(ssx_ctx* ctx, int32_t which, int32_t level, uint8_t* out, int32_t out_cap,
                                      int32_t* rows, int32_t* cols);
SSX_API ssx_status ssx_lk_stage_deriv(ssx_ctx* ctx, int32_t level, int16_t* out, int32_t out_cap, int32_t* rows,
                                      int32_t* cols);

/* tests / tools hooks: one LK call as the host side plans it (csrc/lk.hip: build_geom, build_call) -- what ssx_lk_track /
 * ssx_lk_track_next / ssx_lk_track_batch would do, without doing it.
 *   status / error   what the entry point would return and ssx_last_error() would show; the rest is filled for SSX_OK only
 *   levels .. deriv_words   the geometry of the key (rows, cols, win, max_level): per level rows, cols, pitch, byte offset inside a
 *                    pyramid, word offset inside the derivative images
 *   fused_ok         k_lk_pyramid can build this geometry's pyramids; use_fused: this call uses it; scharr_now: this call runs k_lk_scharr
 *   intake           how the level-0 images reach the device: SSX_LK_STAGED host images through the pinned io block, SSX_LK_ARENA one DMA
 *                    copy of a pinned arena (arena_bytes), SSX_LK_EACH one DMA copy per host image, SSX_LK_IN_PLACE read where they lie
 *   span_off / _bytes  the io block in memory order: job table, staged images, previous points, next points, status, error, device
 *                    images; [0, in_bytes) is sent, [next points, host_end) comes back, io_bytes is the whole block
 *   launch           the launches in order: kernel (SSX_LK_K_*), grid, which / level (-1: the kernel takes none)
 *   slot_flags       per job (the first SSX_LK_MAX_INFO_JOBS), the slot's state after a successful call: bit 0 have_next, bit 1
 *                    have_next_deriv, bit 2 flip; job_roles: which of the slot's two buffers the job's table names as bit 0 pyr[0],
 *                    bit 1 pyr[1], bit 2 deriv, bit 3 deriv1 */
enum { SSX_LK_STAGED = 0, SSX_LK_ARENA = 1, SSX_LK_EACH = 2, SSX_LK_IN_PLACE = 3 };
enum { SSX_LK_K_PYRAMID = 0, SSX_LK_K_PAD_LEVEL0 = 1, SSX_LK_K_PYR_DOWN = 2, SSX_LK_K_SCHARR = 3, SSX_LK_K_TRACK = 4 };
enum { SSX_LK_SPANS = 7, SSX_LK_MAX_LAUNCHES = 32, SSX_LK_MAX_INFO_JOBS = 256 };
typedef struct ssx_lk_call_info {
  int32_t status;
  char error[256];
  int32_t levels, win, pad, rows[8], cols[8], pitch[8];
  uint64_t off[8], doff[8], pyr_bytes, deriv_words;
  int32_t fused_ok, use_fused, scharr_now, intake;
  uint64_t span_off[7], span_bytes[7], in_bytes, host_end, io_bytes, arena_bytes;
  int32_t n_launches, n_jobs;
  struct { int32_t kernel, grid[3], which, level; } launch[32];
  uint8_t slot_flags[256], job_roles[256];
} ssx_lk_call_info;
/* a job as ssx_lk_debug_plan needs it: next_off = its `next` pointer minus jobs[0].next, in bytes */
typedef struct ssx_lk_job_facts {
  int32_t slot, fresh, n, prev_stride, next_stride, reserved;
  int64_t next_off;
} ssx_lk_job_facts;
/* needs no GPU.  planned_key: rows, cols, win, max_level of the context's last successful call (NULL: those of this call);
 * slot_flags: per job its slot's state before the call, bits as above; call_facts: what the entry points would learn from the
 * runtime about the image pointers (each looked at only where they would ask) -- bit 0 jobs[0].next is host memory, bit 1 the
 * `next` images do NOT lie in one allocation (so 0 and 1 mean what they meant when the argument was next0_is_host alone: pointers
 * that pass the arena's arithmetic are one arena).  Returns out->status. */
enum { SSX_LK_FACT_NEXT0_IS_HOST = 1, SSX_LK_FACT_SEVERAL_ALLOCATIONS = 2 };
SSX_API ssx_status ssx_lk_debug_plan(int32_t rows, int32_t cols, int32_t win, int32_t max_level, const int32_t* planned_key, int32_t n_jobs,
                                     const ssx_lk_job_facts* jobs, const uint8_t* slot_flags, int32_t images_on_device, int32_t call_facts,
                                     ssx_lk_call_info* out);
/* which intake (SSX_LK_*) ssx_lk_track_batch would take for these jobs' REAL image pointers on this device; arena_arithmetic
 * (optional): 1 when the `next` pointers pass the arena's arithmetic (ascending, equal strides, at least an image apart, within
 * 2 x jobs images) -- then SSX_LK_ARENA or not is the runtime's answer about the allocation.  Only the `next` pointers and strides
 * of the jobs are looked at.  Makes the runtime's pointer queries of the entry point and nothing else: no copy, no launch, and the
 * context (its geometry, slots, last call) stays as it is. */
SSX_API ssx_status ssx_lk_debug_intake(ssx_ctx* ctx, int32_t n_jobs, const ssx_lk_job* jobs, int32_t rows, int32_t cols, const ssx_lk_params* prm,
                                       int32_t images_on_device, int32_t* intake, int32_t* arena_arithmetic);
/* the same struct for the last successful LK call of ctx (status SSX_OK, no error text) */
SSX_API ssx_status ssx_lk_debug_last_call(ssx_ctx* ctx, ssx_lk_call_info* out);

/* tests hook of the pose-only Levenberg kernels (csrc/pose_only.hip): ssx_pose_only_opt_batch -- jobs of any size in one call, so
 * k_pose_only<2> (M <= 512), k_pose_only<6> (M <= 1536) and k_pose_only_generic are all reached -- behind `warmup` optimize(iters)
 * passes over all edges (0: ssx_pose_only_opt; 1: ssx_loop_pose_opt), run by TRACED instantiations of the same three kernel bodies.
 * They fill what g2o exposes in postIteration, which is also what oracle/ref_driver.cpp's ref_pose_only_trace and the oracle's
 * orc_pose_only_trace record, so that every Levenberg decision of a run can be held against the compiled reference and not only
 * its end (tests/test_pose_only_edges_gpu.py, tests/golden/ref_po_trace.npz):
 *   per LM iteration   it_chi2 = the robust chi2 of the edges' current errors (the TRIAL state when the last trial was rejected: pop()
 *                      restores vertices only), it_lambda = lambda after the iteration, it_trials = its trials (levenbergIteration())
 *   per optimize()     round_rec, 4 ints: active edges at its start, iterations run, 1 = its last iteration returned Terminate (ten
 *                      trials, rho == 0 or a non-finite lambda), outliers after the classification (-1 behind a warm-up pass)
 * Layout: job after job, R_j = warmup + jobs[j].rounds optimize() calls each: R_j * iters_j slots in the three it_* arrays (slot
 * r * iters_j + it; slots of iterations that did not run are 0), R_j * 4 ints in round_rec.  A job with M = 0 records zeros.
 * The job's outputs (pose_io, inlier_out, n_inliers) are written as ssx_pose_only_opt_batch writes them and, for warmup = 0, equal
 * its bytes: the shipped instantiations take no record argument and compile to the code they had before the hook existed. */
SSX_API ssx_status ssx_pose_only_debug_trace(ssx_ctx* ctx, int32_t n, const ssx_pose_only_job* jobs, int32_t warmup, double* it_chi2,
                                             double* it_lambda, int32_t* it_trials, int32_t* round_rec);

/* tests / tools hook, needs no GPU: the host side of the pose-only and loop-pose calls as plain plans (csrc/pose_only.hpp: PoProblem;
 * csrc/pose_only.hip: po_plan_batch; csrc/pnp.hip: plan_pnp).  Either output may be NULL.
 * out: what ssx_pose_only_opt_batch (traced != 0: ssx_pose_only_debug_trace) would do with n <= SSX_PO_MAX_INFO_JOBS jobs of M[j] edges.
 *   job[j]     cls 0 = k_pose_only<2>, 1 = k_pose_only<6>, 2 = k_pose_only_generic, 3 = empty (no block: -1); the block it lies in; offset
 *              and bytes of its buffers there in memory order: xyz, uv, pose in, err, level, result (record + M flags)
 *   block[b]   block 0 is the pinned block of the register classes when there is such a job (read and written in place: nothing sent,
 *              nothing returned; desc_* its descriptor table, trace_* the record table of a traced batch), then one block per generic job
 *              in job order (device arena + pinned mirror: [0, sent) goes up, [ret_off, ret_off + ret_bytes) comes back)
 *   launch[i]  in order: class, workgroups, block, index of its first descriptor in the block's table (-1: handed over by value)
 * pnp_out: the one block of ssx_pnp_ransac / ssx_loop_pose_opt / ssx_loop_compute_pose (tap: ssx_pnp_debug_counts) for pnp_M pairs and
 * pnp_H hypotheses; spans in memory order: best + ticket, xyz, uv, pose in, err, level, result, RANSAC header, RANSAC mask, tap counts,
 * the refinement's descriptor (used in the pinned mirror only); sent / ret_* as above; refine_cls as job[].cls */
enum { SSX_PO_SPANS = 6, SSX_PO_MAX_INFO_JOBS = 16, SSX_PNP_SPANS = 11 };
typedef struct ssx_po_plan_info {
  int32_t n_jobs, n_blocks, n_launches, reserved;
  struct { int32_t cls, block; uint64_t span_off[6], span_bytes[6]; } job[16];
  struct { uint64_t bytes, sent, ret_off, ret_bytes, desc_off, desc_bytes, trace_off, trace_bytes; } block[16];
  struct { int32_t cls, grid, block, first_desc; } launch[16];
} ssx_po_plan_info;
typedef struct ssx_pnp_plan_info {
  uint64_t span_off[11], span_bytes[11], bytes, sent, ret_off, ret_bytes;
  int32_t refine_cls, reserved;
} ssx_pnp_plan_info;
SSX_API ssx_status ssx_po_debug_plan(int32_t n, const int32_t* M, int32_t traced, ssx_po_plan_info* out, int32_t pnp_M, int32_t pnp_H,
                                     int32_t pnp_tap, ssx_pnp_plan_info* pnp_out);

/* tests hooks of the P3P-RANSAC (csrc/pnp.hip, model: tools/pnp_model.py): the sample triples of (seed, M >= 3, H) as the kernel's
 * device function draws them (triples_out H x 3), and the best inlier count of each of the max_iters hypotheses of an
 * ssx_pnp_ransac call with the same arguments (counts_out max_iters) */
SSX_API ssx_status ssx_pnp_debug_samples(ssx_ctx* ctx, uint32_t seed, int32_t M, int32_t H, int32_t* triples_out);
SSX_API ssx_status ssx_pnp_debug_counts(ssx_ctx* ctx, const double* K4, int32_t M, const double* xyz, const double* uv,
                                        int32_t max_iters, double reproj_px, uint32_t seed, int32_t* counts_out);
/* the minimal solver alone: n triples (xyz n x 3 x 3, uv n x 3 x 2), one thread each, p3p_solve and rot_to_quat as k_pnp_ransac calls
 * them -> per triple and slot (solution 2 p + r is root r of plane p) valid_out n x 4, R_out n x 4 x 9 (row-major), t_out n x 4 x 3 and
 * pose_out n x 4 x 7 (qx qy qz qw tx ty tz); a slot that is not valid is all zeros.  n = 0 does nothing.  Reference:
 * tests/golden/p3p_hp.npz */
SSX_API ssx_status ssx_pnp_debug_p3p(ssx_ctx* ctx, const double* K4, int32_t n, const double* xyz, const double* uv, int32_t* valid_out,
                                     double* R_out, double* t_out, double* pose_out);

/* tests / tools hooks of the per-keyframe step (csrc/loop.hip).  What the database's last ssx_kfdb_process_keyframe issued, each counted
 * where it is issued: kernel launches, stream synchronisations (a new ORB plan's two included), bytes sent up and bytes that came down
 * (the pairs are written by the kernel into mapped pinned memory: 8 bytes of header and 8 per pair).  Likewise for the database's last
 * ssx_kfdb_relocalize_query or ssx_kfdb_guided_search, whichever call came last.  Any output may be NULL. */
SSX_API ssx_status ssx_kfdb_debug_last_step(const ssx_kf_database* db, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up,
                                            int64_t* bytes_down);
/* the same for the context's last ssx_kfdb_process_keyframe_batch (all zero after a call that failed before its first synchronisation);
 * the match table of the found jobs, read by the device from pinned memory, counts as bytes sent up */
SSX_API ssx_status ssx_kfdb_debug_last_batch(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down);
/* k_voc_words + k_kf_bow alone: the BowVector of n descriptors as the step assembles it on the device (ids ascending, values);
 * *n_entries = its size, SSX_ERR_CAPACITY when cap is smaller */
SSX_API ssx_status ssx_kfdb_debug_bow(ssx_vocabulary* voc, const uint8_t* desc, int32_t n, int32_t cap, int32_t* ids_out, double* vals_out,
                                      int32_t* n_entries);

/* tests / tools hook of ssx_undistort (csrc/undistort.hip): what the context's last call issued, counted from the lists of copies
 * it issued (filled once the call has synchronised) -- kernel launches, stream synchronisations, bytes sent up (the job table and, for host images,
 * the sources) and bytes that came down (the results of host images).  All zero after a call that was refused.  Any output may be NULL. */
SSX_API ssx_status ssx_undistort_debug_last_call(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down);
/* the same for a plan (ssx_undistort_plan_*): what its last ssx_undistort_plan_add or ssx_undistort_plan_apply issued.  copies_up /
 * copies_down count the copies that carry images (a staged call's one copy up carries the job table too; otherwise the table goes up
 * beside them, in bytes_up and not in copies_up).  All zero after a call that was refused, and after an add that found its map. */
SSX_API ssx_status ssx_undistort_plan_debug_last_call(const ssx_undistort_plan* plan, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up,
                                                      int64_t* bytes_down, int32_t* copies_up, int32_t* copies_down);
/* The call that ssx_undistort (entry 0), ssx_undistort_lens (1) or ssx_undistort_plan_apply (2) would issue, as csrc/undistort.hip
 * plans it (UdCall), or its refusal.  Needs no GPU and no context: the same checks and the same builder run on jobs stated as facts.
 *   jobs[k]     src_off / dst_off = the job's pointers minus jobs[0].src, in bytes (flags: the pointer is null instead); the strides;
 *               tag = its lens model (entries 0, 1) or its map index (entry 2).  jobs = NULL is a null table.
 *   n_maps      the maps the plan holds (entry 2)
 *   src_facts / dst_facts   what the entry point would learn from the runtime about that side's images (looked at only where it would
 *               ask: entry 2 with images_on_device): one_allocation, and kind[k] of image k -- 1 pinned host, 0 device, -1 neither; with
 *               one_allocation only kind[0] counts.  NULL, or kind = NULL: every image is device memory.
 * out->status and out->error are what the entry point would return and ssx_last_error would show; the rest is filled for SSX_OK with
 * n > 0: the launch, the intakes (SSX_UD_*), the spans of the device block in memory order (table, sources, results), per job what its
 * table entry carries (an offset into the block or SSX_UD_WHERE_IT_LIES, and the strides), the copies in the order they are issued
 * (host: the caller's address in a space where jobs[0].src - jobs[0].src_off is SSX_UD_BASE, or 0: the pinned staging buffer at
 * `off`; a down copy is height rows of width bytes), and the counters the call would report.  Returns out->status. */
enum { SSX_UD_ENTRY_UNDISTORT = 0, SSX_UD_ENTRY_LENS = 1, SSX_UD_ENTRY_PLAN_APPLY = 2 };
enum { SSX_UD_STAGED = 0, SSX_UD_IN_PLACE = 1, SSX_UD_RANGE = 2, SSX_UD_EACH = 3 };
enum { SSX_UD_SRC_IS_NULL = 1, SSX_UD_DST_IS_NULL = 2 };
#define SSX_UD_WHERE_IT_LIES (~(uint64_t)0)
#define SSX_UD_BASE ((uint64_t)1 << 40)
typedef struct ssx_undistort_job_facts { int64_t src_off, dst_off; int32_t src_stride, dst_stride, tag, flags; } ssx_undistort_job_facts;
typedef struct ssx_undistort_side_facts { int32_t one_allocation, reserved; const int8_t* kind; } ssx_undistort_side_facts;
typedef struct ssx_undistort_call_info {
  int32_t status;
  char error[256];
  int32_t grid[3], block[3], src_intake, dst_intake;
  uint64_t span_off[3], span_bytes[3], up_bytes, arena_bytes, stage_bytes;
  int32_t n_jobs, n_up, n_down, launches, syncs, copies_up, copies_down, reserved;
  int64_t bytes_up, bytes_down;
  struct { uint64_t src_off, dst_off; int64_t src_stride, dst_stride; } job[1024];
  struct { uint64_t off, host, bytes, images; } up[1025];
  struct { uint64_t host, host_pitch, off, dev_pitch, width, height; } down[1024];
} ssx_undistort_call_info;
SSX_API ssx_status ssx_undistort_debug_plan(int32_t entry, int32_t rows, int32_t cols, int32_t images_on_device, int32_t n, const ssx_undistort_job_facts* jobs,
                                            int32_t n_maps, const ssx_undistort_side_facts* src_facts, const ssx_undistort_side_facts* dst_facts,
                                            ssx_undistort_call_info* out);
/* the stored map `map_index` as tools/undistort_model.py's pack_map returns it: out = three planes of rows x cols u16 (xs, ys, ab),
 * each contiguous */
SSX_API ssx_status ssx_undistort_plan_debug_map(ssx_undistort_plan* plan, int32_t map_index, uint16_t* out);
/* the device's atan_c and sqrt of the KB4 lens (csrc/undistort.hip: ud_atan) over n host doubles (0 .. 2^24), so that their bits are
 * compared with tools/rectify_model.py's directly; either output may be NULL */
SSX_API ssx_status ssx_lens_debug_atan(ssx_ctx* ctx, int32_t n, const double* r, double* atan_out, double* sqrt_out);

/* tests / tools hooks of ssx_stereo_dense (csrc/dense.hip).  What the context's last call issued, counted where it is issued, as
 * ssx_undistort_debug_last_call counts (a fill of workspace counts as a launch), and the number of groups it worked through.  All
 * zero after a call that was refused.  Any output may be NULL. */
SSX_API ssx_status ssx_dense_debug_last_call(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down,
                                             int32_t* groups);
/* tests hook: the workspace cap the dense calls of ctx group their jobs by, in bytes; 0 = SSX_DENSE_WORKSPACE_CAP (the default).
 * A call takes as many jobs a group as stay under the cap, at least one, where one job counts as
 *   pix * (16 + 2 * disparities + 4) + 768 bytes   in ssx_stereo_dense and ssx_stereo_dense_post (census, S and right key per pixel),
 *   pix * 8 + rows * 4 + 768 bytes                 in ssx_dense_postprocess (label and size per pixel, a count per row),
 * pix = rows * cols.  The tests work out the cap for a group size from these (tests/test_dense_groups_gpu.py) and assert the groups
 * that ssx_dense_debug_last_call reports.  The cap stays until it is set again: a test that sets it restores 0. */
SSX_API ssx_status ssx_dense_debug_set_workspace_cap(ssx_ctx* ctx, uint64_t bytes);
/* the stages of ONE pair of host images through the kernels of ssx_stereo_dense, named as tools/dense_model.py names them: the census
 * words of both images (rows x cols u64 each), the path volume L of `direction` (0 .. paths - 1; rows x cols x disparities u8, d
 * fastest), the summed volume S (u16, the same shape) and the right disparity dR (rows x cols u8).  Any output may be NULL. */
SSX_API ssx_status ssx_dense_debug_stages(ssx_ctx* ctx, const uint8_t* left, int32_t left_stride, const uint8_t* right, int32_t right_stride,
                                          int32_t rows, int32_t cols, const ssx_dense_params* prm, int32_t direction, uint64_t* census_left,
                                          uint64_t* census_right, uint8_t* path_volume, uint16_t* sum_volume, uint8_t* right_disparity);
/* the connected components of ONE host map (rows x cols int16 at a pitch of disp_stride elements) through the labelling kernels of
 * ssx_dense_postprocess, as tools/dense_post_model.py's components() names them: per pixel the size of its component and its root
 * (the smallest raster index y * cols + x), 0 and -1 where the pixel is not valid.  Either output may be NULL.
 * ssx_dense_debug_last_call (above) counts ssx_dense_postprocess and ssx_stereo_dense_post as it counts ssx_stereo_dense. */
SSX_API ssx_status ssx_dense_debug_components(ssx_ctx* ctx, const int16_t* disp, int32_t disp_stride, int32_t rows, int32_t cols, int32_t speckle_range,
                                              int32_t* size, int32_t* root);

#ifdef __cplusplus
}
#endif
#endif /* SSX_TEST_HOOKS_H */
