/* include/ssx.h -- C ABI of libssx.so, the MI355X (gfx950) compute core that drops in behind
 * ssvio's ORBextractor / FrontEnd / Backend class surfaces.
 *
 * The reference (weihaoysgs/ssvio, /root/reference) has no plugin/FFI layer: its seams are the
 * non-virtual C++ methods listed per entry point below.  A maintainer
 * replaces the BODY of each cited method with a marshalling call into this ABI (INTEGRATION.md shows
 * the stubs; include/ssx_shim.hpp ships ready-made C++ wrappers with the reference's method names).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  All array arguments are HOST pointers
 *     unless the parameter name ends in _dev (device pointers, for callers that keep data in HBM).
 *   - every function returns an ssx_status (0 = OK, <0 = error) and never aborts or throws;
 *     ssx_last_error(ctx) returns a human-readable message for the last failure on that ctx.
 *   - the caller owns every buffer; outputs are caller-allocated with a capacity + *count.
 *   - one ssx_ctx = one GPU + one HIP stream.  A ctx is single-threaded; different ctxs may be used
 *     concurrently from different threads (the reference's front-end thread and backend thread each
 *     hold their own; multi-GPU = one ctx per device, one process per GPU under torch.distributed).
 *   - pose layout = Sophus::SE3d::data(): qx qy qz qw tx ty tz (T_cw, world -> camera).
 *   - there is NO CPU fallback: if no gfx950 device is present ssx_ctx_create fails with
 *     SSX_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef SSX_H
#define SSX_H
#include <stddef.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSX_VERSION 120 /* 0.1.20: + ssx_lk_track_batch, ssx_pose_only_opt_batch, ssx_host_alloc / _free; the kernel taps (ssx_*_stage_*,
                           * ssx_ba_linearize) moved to ssx_test_hooks.h, ssx_ba_batch_set_persistent (a no-op since round 4) removed.  0.1.10: ssx_config grew by cu_first / cu_count, ssx_ba_result by ms_comm, ssx_ba_window_update by the
                           * removal fields -- see ssx_abi_check */
#if defined(__GNUC__)
#define SSX_API __attribute__((visibility("default")))
#else
#define SSX_API
#endif

typedef enum {
  SSX_OK = 0,
  SSX_ERR_INVALID_ARG = -1,
  SSX_ERR_NO_DEVICE = -2,
  SSX_ERR_HIP = -3,        /* a HIP runtime call failed; see ssx_last_error */
  SSX_ERR_CAPACITY = -4,   /* an output capacity was too small; *count holds the needed size */
  SSX_ERR_UNSUPPORTED = -5,
  SSX_ERR_COMM = -6        /* the all-reduce callback reported a failure */
} ssx_status;

typedef struct ssx_ctx ssx_ctx;

/* Construction parameters the reference reads from its YAML through Setting::Get
 * (src/ssvio/system.cpp:59-70,117-128; config/kitti_00.yaml). */
typedef struct {
  int device;          /* HIP device ordinal */
  void* stream;        /* hipStream_t to run on, or NULL to create a private non-blocking stream */
  int max_width, max_height; /* largest image the ctx will see (scratch sizing); 0 = grow on demand */
  /* Partition the chip between contexts that run side by side (the front-end's ctx and the backend's): when cu_count > 0
   * every stream the ctx CREATES (stream == NULL above, its auxiliary and group streams) is restricted to cu_count
   * compute units starting at cu_first (hipExtStreamCreateWithCUMask; bit i of the mask lands on XCD i mod 8, so any
   * contiguous range is spread evenly over the eight XCDs).  0 / 0 = the whole chip.  Ignored for a caller's stream.
   * NOTE: hipExtStreamCreateWithCUMask takes no flags -- the streams of a masked ctx have default flags and normal priority:
   * they are not hipStreamNonBlocking (they synchronise implicitly with the legacy NULL stream, e.g. torch's default stream) and
   * the auxiliary stream loses the lowest priority an unmasked ctx gives it. */
  int cu_first, cu_count;
} ssx_config;

SSX_API int ssx_version(void);
/* The structs of this header carry no size field: a caller built against another version of it would hand the library a
 * shorter ssx_config (cu_count read from garbage) or receive ms_comm past the end of its ssx_ba_result.  Call this once after
 * loading the library with SSX_VERSION and the sizeof of the structs AS THE CALLER WAS COMPILED:
 *   ssx_abi_check(SSX_VERSION, sizeof(ssx_config), sizeof(ssx_ba_problem), sizeof(ssx_ba_options), sizeof(ssx_ba_result),
 *                 sizeof(ssx_ba_window_update))
 * SSX_OK when they are the library's, SSX_ERR_UNSUPPORTED otherwise (include/ssx_shim.hpp and ssvio_amd/_lib.py do it when they
 * load the library).  Every struct must be zero-initialised before its fields are set: later versions append fields whose
 * zero value means "as before". */
SSX_API ssx_status ssx_abi_check(int header_version, size_t sizeof_config, size_t sizeof_ba_problem, size_t sizeof_ba_options,
                                 size_t sizeof_ba_result, size_t sizeof_window_update);
SSX_API int ssx_device_count(void);
SSX_API ssx_status ssx_ctx_create(const ssx_config* cfg, ssx_ctx** out);
SSX_API void ssx_ctx_destroy(ssx_ctx* ctx);
SSX_API const char* ssx_last_error(const ssx_ctx* ctx);
SSX_API ssx_status ssx_ctx_synchronize(ssx_ctx* ctx);
/* hipStream_t the ctx enqueues on (for callers that bracket calls with their own events). */
SSX_API void* ssx_ctx_stream(ssx_ctx* ctx);
/* Page-locked (pinned, GPU-readable) host memory for callers without a HIP toolchain of their own: images kept in such a buffer can
 * be handed to the batched entry points with images_on_device = 1 (the kernels read them over PCIe, nothing is staged).  NULL when
 * the allocation fails.  (hipHostMalloc / hipHostFree.) */
SSX_API void* ssx_host_alloc(size_t bytes);
SSX_API void ssx_host_free(void* p);

/* Per-kernel GPU time, measured with HIP events recorded on the ctx stream around every kernel launch
 * between ssx_profile_begin and ssx_profile_end (the counterpart of g2o's G2OBatchStatistics; bench.py uses it
 * for the roofline of the dominant kernel).  Event pairs add a little launch overhead: time throughput with
 * profiling off. */
typedef struct {
  char name[48];
  int32_t calls;
  double total_ms;
} ssx_kernel_time;
SSX_API ssx_status ssx_profile_begin(ssx_ctx* ctx);
SSX_API ssx_status ssx_profile_end(ssx_ctx* ctx, ssx_kernel_time* out, int32_t cap, int32_t* n);

/* ------------------------------------------------------------------------------------------------
 * Local bundle adjustment -- replaces the body of Backend::OptimizeActiveMap
 * (src/ssvio/backend.cpp:78-245): g2o BlockSolver_6_3 + LinearSolverCSparse + Levenberg-Marquardt
 * with EdgeProjection / VertexPose / VertexXYZ (include/ssvio/g2otypes.hpp:28-65,112-162), Huber kernel,
 * landmarks marginalised (Schur complement, thirdparty/g2o/g2o/core/block_solver.hpp:315-447).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t P;                 /* poses (active keyframes, backend.cpp:88-103) */
  const double* poses;       /* P x 7 */
  const uint8_t* pose_fixed; /* P, nullable (reference: none fixed) */
  int32_t L;                 /* landmarks (backend.cpp:113-132) */
  const double* points;      /* L x 3 */
  const uint8_t* point_fixed;/* L, nullable (backend.cpp:125-130) */
  int32_t E;                 /* observations / EdgeProjection edges (backend.cpp:135-168) */
  const int32_t* edge_pose;  /* E, index into poses */
  const int32_t* edge_point; /* E, index into points */
  const double* edge_uv;     /* E x 2 measured pixel (cv::Point2f widened to double, backend.cpp:80,160) */
  const uint8_t* edge_cam;   /* E, 0 = left extrinsic, 1 = right (backend.cpp:148-155); nullable = all 0 */
  double K[4];               /* fx fy cx cy (Camera::getK) */
  double cam_ext[14];        /* 2 x 7: left / right camera extrinsic (Camera::getPose, system.cpp:63,71) */
} ssx_ba_problem;

typedef enum { SSX_JAC_ANALYTIC = 0, SSX_JAC_NUMERIC_G2O = 1 } ssx_jac_mode;
typedef enum { SSX_LARGE_SOLVER_AUTO = 0, SSX_LARGE_SOLVER_TILES = 1, SSX_LARGE_SOLVER_BAND = 2 } ssx_large_solver;

/* Sum-all-reduce hook for landmark-sharded multi-GPU BA.  `buf_dev` is a DEVICE pointer to `count`
 * doubles on the ctx's device; the callee must enqueue an in-place sum over all ranks ordered after
 * work already enqueued on `stream` and make later work on `stream` wait for it (torch.distributed
 * all_reduce on a tensor aliasing buf_dev does exactly that when the ctx runs on torch's current
 * stream).  Return 0 on success. */
typedef int (*ssx_allreduce_fn)(void* user, double* buf_dev, size_t count, void* stream);

/* RCCL inside the library (the reference is a single process, there is no counterpart): one
 * process per GPU, one communicator per process.  Rank 0 calls ssx_comm_unique_id and hands the 128 bytes to the other
 * ranks by whatever channel the host has (MPI, a file, torch.distributed); every rank then calls ssx_comm_init
 * (collective: ncclCommInitRank on the ctx's device).  ssx_comm_wrap adopts an ncclComm_t the host already owns.
 * With ssx_ba_options.comm set, ssx_ba_solve sums its exchange buffers with ncclAllReduce(f64, sum) enqueued on the
 * ctx stream -- no callback, no host round trip.  librccl.so.1 is bound at run time (the copy already loaded in the
 * process, else /opt/rocm/lib); SSX_ERR_COMM when it cannot be found. */
typedef struct ssx_comm ssx_comm;
typedef struct { char bytes[128]; } ssx_comm_id;      /* an ncclUniqueId */
SSX_API ssx_status ssx_comm_unique_id(ssx_ctx* ctx, ssx_comm_id* out);
SSX_API ssx_status ssx_comm_init(ssx_ctx* ctx, const ssx_comm_id* id, int32_t rank, int32_t world_size, ssx_comm** out);
SSX_API ssx_status ssx_comm_wrap(ssx_ctx* ctx, void* nccl_comm, int32_t rank, int32_t world_size, ssx_comm** out);
SSX_API void ssx_comm_destroy(ssx_comm* comm);
SSX_API ssx_status ssx_comm_info(const ssx_comm* comm, int32_t* rank, int32_t* world_size);
/* in-place f64 sum of `count` doubles at the DEVICE pointer buf_dev, ordered on the ctx stream */
SSX_API ssx_status ssx_comm_allreduce_sum(ssx_ctx* ctx, ssx_comm* comm, double* buf_dev, size_t count);

typedef struct {
  int32_t outer_rounds;   /* backend.cpp:175  while (iteration < 5)            default 5     */
  int32_t iters;          /* backend.cpp:178  optimizer.optimize(10)           default 10    */
  double chi2_th;         /* backend.cpp:109                                    default 5.891 */
  double huber_delta;     /* backend.cpp:163  rk->setDelta(chi2_th)             default 5.891 */
  double inlier_ratio;    /* backend.cpp:195                                    default 0.7   */
  int32_t jac_mode;       /* ssx_jac_mode; the reference uses g2o's numeric Jacobians
                             (linearizeOplus is commented out, g2otypes.hpp:133-153)           */
  /* multi-GPU: this rank holds a landmark shard (all edges of its landmarks, every pose replicated);
   * allreduce sums the reduced pose system and the chi2/scale scalars across ranks.  NULL = 1 GPU. */
  ssx_allreduce_fn allreduce;
  void* allreduce_user;
  int32_t rank, world_size; /* of this shard; world_size <= 1 = single GPU */
  /* the native path: an ssx_comm (RCCL).  When set it takes precedence over `allreduce`, and rank / world_size are
   * the communicator's.  The callback above stays for hosts with their own collective layer and for tests. */
  ssx_comm* comm;
  int32_t collect_stats;    /* 1 = time every phase with HIP events (fills ssx_ba_result.ms_*; a few us per launch) */
  /* windows with more than 16 free keyframes, the reduced pose system: SSX_LARGE_SOLVER_AUTO picks the band solver
   * (sliding-window block Cholesky + nested dissection along the trajectory) when every keyframe shares landmarks only
   * with keyframes within 5 positions along the (possibly closed) trajectory (block bandwidth w <= 5) and the window
   * has at least 2 w + 2 free keyframes, else the 64x64-tile sparse Cholesky; _TILES / _BAND force one (BAND fails
   * with SSX_ERR_UNSUPPORTED on a wider co-visibility or a shorter window). */
  int32_t large_solver;
} ssx_ba_options;

#define SSX_BA_MAX_STATS 128
typedef struct {
  double* poses_out;        /* P x 7, nullable */
  double* points_out;       /* L x 3, nullable */
  double* edge_chi2;        /* E, nullable: edge->chi2() as backend.cpp:185,209 reads it */
  uint8_t* edge_outlier;    /* E, nullable: chi2 > chi2_th (backend.cpp:209-227) */
  int32_t rounds;           /* outer rounds executed */
  int32_t n_iters;          /* LM iterations executed over all rounds (<= SSX_BA_MAX_STATS recorded) */
  double iter_chi2[SSX_BA_MAX_STATS];   /* robust chi2 after each LM iteration */
  double iter_lambda[SSX_BA_MAX_STATS]; /* lambda after each LM iteration */
  int32_t iter_trials[SSX_BA_MAX_STATS];/* LM trials of each iteration */
  int32_t n_inliers, n_outliers;        /* of the last round (backend.cpp:181-194) */
  /* GPU time of this call, milliseconds (HIP events on the ctx stream): upload .. last download */
  float ms_total, ms_setup;
  /* with ssx_ba_options.collect_stats: GPU time per phase summed over the call, the fields of g2o's
   * G2OBatchStatistics (thirdparty/g2o/g2o/core/batch_stats.h:38-68) they correspond to in brackets */
  float ms_linearize;       /* residuals + Jacobians + quadratic form   [timeResiduals + timeLinearize + timeQuadraticForm] */
  float ms_schur;           /* landmark elimination                     [timeSchurComplement]                               */
  float ms_linear_solution; /* reduced-system factorisation + solves    [timeLinearSolution]                                */
  float ms_update;          /* back-substitution, state update, trial residuals  [timeUpdate + the next computeActiveErrors] */
  float ms_reduce;          /* cross-chunk reductions                   [no g2o counterpart: single-threaded]               */
  float ms_comm;            /* the all-reduces of a landmark-sharded solve (enqueue to completion on the ctx stream)         */
} ssx_ba_result;

SSX_API void ssx_ba_default_options(ssx_ba_options* opt);
SSX_API ssx_status ssx_ba_solve(ssx_ctx* ctx, const ssx_ba_problem* prob, const ssx_ba_options* opt,
                        ssx_ba_result* res);

/* n windows in one call: what a batch of stereo pairs / a set of concurrent streams hands to its backends together.
 * Per window the arithmetic and the result are those of ssx_ba_solve (bit-identical); the kernels run once for all
 * windows (one grid dimension is the window), each window's device-driven LM loop advances on its own, one upload and
 * one download carry all of them, and the host marshalling runs on several threads.  Windows with more than 16 free
 * keyframes, a collective in `opt`, or n == 1 are solved one after the other.  `opt` applies to every window. */
SSX_API ssx_status ssx_ba_solve_batch(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt,
                                      ssx_ba_result* results);

/* A RESIDENT batch: marshalled and uploaded once, the windows stay in HBM; every ssx_ba_batch_solve optimises all of them
 * again from the uploaded state.  results may be NULL (nothing is downloaded; *lm_iterations_total, optional, still
 * counts the LM iterations run); with_edge_errors = 1 keeps what ssx_ba_result.edge_chi2 / edge_outlier need.
 * A batch belongs to its ctx and must be destroyed before it. */
typedef struct ssx_ba_batch ssx_ba_batch;
SSX_API ssx_status ssx_ba_batch_create(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt,
                                       int32_t with_edge_errors, ssx_ba_batch** out);
SSX_API ssx_status ssx_ba_batch_solve(ssx_ba_batch* batch, ssx_ba_result* results, int32_t* lm_iterations_total);
SSX_API int32_t ssx_ba_batch_size(const ssx_ba_batch* batch);
/* groups of windows ssx_ba_batch_solve runs side by side, each on its own stream (every batched kernel is launched once
   per group; 1 for fewer than 8 windows; SSX_BA_GROUPS in the environment overrides the default of 2) */
SSX_API int32_t ssx_ba_batch_groups(const ssx_ba_batch* batch);
/* 1 .. 4 groups for the following solves; 0 = back to the default (per-kernel profiles want 1: one launch per kernel and
   LM slot, nothing else on the chip beside it) */
SSX_API void ssx_ba_batch_set_groups(ssx_ba_batch* batch, int32_t groups);
SSX_API void ssx_ba_batch_destroy(ssx_ba_batch* batch);
/* Process-wide: the device phases of batched solves (ssx_ba_solve_batch, ssx_ba_batch_solve, ssx_ba_window_solve_batch) of DIFFERENT
 * contexts run one after the other on the device, in the order they were enqueued: the kernels of an LM round wait, on the device
 * (hipStreamWaitEvent), for the end of the round enqueued before it, whichever context that was.  Nothing is serialised on the host
 * but the enqueueing.  For servers that drive groups of windows from several host threads, one context each (the backend threads of
 * concurrent streams, backend.cpp:57-76): without turns the device phases of the groups interleave on the chip, end together, and
 * the groups' host phases (pending uploads, counting tables, unpacking) then coincide with the device idle; with turns one group's
 * host phase lies beside the other's kernels.  Off by default; no effect on results. */
SSX_API void ssx_ba_device_turns(int32_t enable);
/* Groups of windows (1 .. 4, each on a stream of its own; 0 = the default, 2 from 8 windows on) the ONE-SHOT batched solves of this ctx
 * -- ssx_ba_solve_batch, ssx_ba_window_solve_batch -- are run in, as ssx_ba_batch_set_groups does for a resident batch.  A server that
 * already drives several contexts side by side wants 1: the GPU has four hardware queues, and three backend contexts of one stream
 * each beside the front-end's measured 18 k stereo frames/s where three contexts of two streams each measured 14 k
 * (profiles/r05/live_backend_orchestration.md).  No effect on results. */
SSX_API ssx_status ssx_ba_set_batch_groups(ssx_ctx* ctx, int32_t groups);

/* ------------------------------------------------------------------------------------------------
 * A sliding local-BA window that STAYS in HBM.  Backend::OptimizeActiveMap (src/ssvio/backend.cpp:88-169) rebuilds its
 * graph from the active map at every keyframe, and that map changes by ONE keyframe between two optimisations
 * (Map::InsertKeyFrame, RemoveOldActiveKeyframe, RemoveOldActiveMapPoints: src/ssvio/map.cpp:27-56, 89-160).  The window
 * mirrors that: push a keyframe (its pose, the landmarks it introduces, its observations: the only data that crosses PCIe),
 * pop a keyframe (its observations go, and every landmark nobody observes any more), solve what is resident.  The device
 * sorts the observations by landmark itself; per solve the host counts observations per landmark (one pass over the
 * window) and uploads ~3.6 bytes per observation + 13 per landmark of tables.  Keyframes and landmarks are named by the
 * caller's 64-bit ids (KeyFrame::key_frame_id_, MapPoint::id_).  <= 16 free keyframes (the reference keeps 12:
 * config/kitti_00.yaml:30).  A window belongs to its ctx and must be destroyed before it.
 * ORDER: a solve gives its vertices the order of the caller's ids -- keyframes ascending by id, landmarks ascending by id, as
 * g2o orders its vertices and as a caller that re-marshals its map per keyframe does -- so its bits depend on what the window
 * holds, never on the storage slots it reused.  ssx_ba_window_export lists the window in that order, and the result of
 * ssx_ba_window_solve is, bit for bit, that of ssx_ba_solve on the exported problem.
 * BETWEEN TWO OPTIMISATIONS the reference changes its map by more than one keyframe in / one out (backend.cpp:205-244,
 * map.cpp:142-194): outlier observations are unlinked (ssx_ba_window_remove_flagged / _remove_observations), condemned map
 * points are deleted (ssx_ba_window_remove_landmarks), and a map point is FIXED while the keyframe of its first remaining
 * observation is outside the window (backend.cpp:125-130: ssx_ba_window_set_fix_rule).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_ba_window ssx_ba_window;
SSX_API ssx_status ssx_ba_window_create(ssx_ctx* ctx, const ssx_ba_options* opt, const double* K4, const double* cam_ext14,
                                        ssx_ba_window** out);
SSX_API void ssx_ba_window_destroy(ssx_ba_window* win);
/* new_ids / new_xyz / new_fixed: the n_new landmarks this keyframe brings into the window (ids not yet in it);
 * obs_lm / obs_uv (n_obs x 2) / obs_cam (nullable = all left): its observations, of those or of landmarks already in
 * the window (backend.cpp:135-168).  Nothing is changed when the call fails. */
SSX_API ssx_status ssx_ba_window_push_keyframe(ssx_ba_window* win, int64_t kf_id, const double* pose7, int32_t pose_fixed,
                                               int32_t n_new, const int64_t* new_ids, const double* new_xyz,
                                               const uint8_t* new_fixed, int32_t n_obs, const int64_t* obs_lm,
                                               const double* obs_uv, const uint8_t* obs_cam);
/* The same for a caller that keeps, with every map point, the SLOT the window gave it (new_slots_out[i] = slot of the i-th
 * new landmark, valid until the landmark leaves the window): obs_slot[j] >= 0 = that slot, -1 - i = the i-th new landmark
 * of this call.  No id is looked up: a 2000-observation keyframe costs ~10 us of host time instead of ~70. */
SSX_API ssx_status ssx_ba_window_push_keyframe_slots(ssx_ba_window* win, int64_t kf_id, const double* pose7, int32_t pose_fixed,
                                                     int32_t n_new, const int64_t* new_ids, const double* new_xyz,
                                                     const uint8_t* new_fixed, int32_t* new_slots_out, int32_t n_obs,
                                                     const int32_t* obs_slot, const double* obs_uv, const uint8_t* obs_cam);
SSX_API ssx_status ssx_ba_window_pop_keyframe(ssx_ba_window* win, int64_t kf_id);
/* backend.cpp:205-227 (`if (ef.first->chi2() > chi2_th)`: mappoint->RemoveActiveObservation + RemoveObservation): unlink
 * observations; a landmark left without any leaves the window (Map::RemoveOldActiveMapPoints, and map.cpp:175-194 when the
 * reference deletes it altogether).
 *   _remove_flagged       flags[i] != 0 removes the i-th observation in the order of ssx_ba_window_export: the
 *                         ssx_ba_result.edge_outlier of the solve that just ran can be handed back as it is; n_obs must be the
 *                         window's observation count
 *   _remove_observations  the observations keyframe kf_id holds of the landmarks lm_ids[i] (camera cams[i] != 0 = right;
 *                         cams NULL = either); pairs the window does not hold are skipped, an unknown kf_id is an error
 * *n_removed (nullable) receives the number of observations removed. */
SSX_API ssx_status ssx_ba_window_remove_flagged(ssx_ba_window* win, int32_t n_obs, const uint8_t* flags, int32_t* n_removed);
SSX_API ssx_status ssx_ba_window_remove_observations(ssx_ba_window* win, int64_t kf_id, int32_t n, const int64_t* lm_ids,
                                                     const uint8_t* cams, int32_t* n_removed);
/* Map::RemoveAllOutlierMapPoints (map.cpp:175-194; the map points FrontEnd::EstimateCurrentPose, frontend.cpp:283-288, or the
 * backend condemned): the landmarks leave with all their observations.  Ids the window does not hold are skipped;
 * *n_removed (nullable) = landmarks removed. */
SSX_API ssx_status ssx_ba_window_remove_landmarks(ssx_ba_window* win, int32_t n, const int64_t* lm_ids, int32_t* n_removed);
/* rule 0 (default): a landmark is fixed when the caller says so (new_fixed, ssx_ba_window_set_landmark).
 * rule 1: backend.cpp:125-130 as well -- `mp->GetObservations().front()`'s keyframe is not active: a landmark is fixed while the
 * earliest-pushed keyframe among its remaining observations (MapPoint::observations_ keeps those of keyframes that left the
 * window, and loses those removed as outliers) is no longer in the window; ssx_ba_window_pop_keyframe and the removals keep
 * that up to date.  A landmark that comes BACK into a window it had left is pushed with new_fixed = what the caller's map says. */
SSX_API ssx_status ssx_ba_window_set_fix_rule(ssx_ba_window* win, int32_t rule);
/* One keyframe replaced in each of n windows of ONE ctx, in one call, the windows spread over the ctx's host threads (the
 * windows of concurrent streams all change at every keyframe; the edits are independent host work, ~25-70 us per window).
 * Per window, in this order: n_remove_flags > 0 -> ssx_ba_window_remove_flagged (what the LAST optimisation decided: its flags
 * refer to the window as that solve saw it); n_remove_lm > 0 -> ssx_ba_window_remove_landmarks; pop != 0 ->
 * ssx_ba_window_pop_keyframe(pop_kf_id); push != 0 -> ssx_ba_window_push_keyframe (obs_lm) or
 * _push_keyframe_slots (obs_lm NULL, obs_slot) with the remaining fields.  status_out (nullable) receives every window's own
 * status; the call returns the first one that is not SSX_OK (a failing window is left as its own failing call leaves it, the
 * others are updated).  The windows must be distinct. */
typedef struct ssx_ba_window_update {
  int32_t pop, push;
  int64_t pop_kf_id, kf_id;
  const double* pose7;
  int32_t pose_fixed, n_new;
  const int64_t* new_ids;
  const double* new_xyz;
  const uint8_t* new_fixed;
  int32_t* new_slots_out;       /* slots form only */
  int32_t n_obs, reserved;
  const int64_t* obs_lm;        /* observations by landmark id, or NULL and ... */
  const int32_t* obs_slot;      /* ... by slot (see ssx_ba_window_push_keyframe_slots) */
  const double* obs_uv;
  const uint8_t* obs_cam;
  int32_t n_remove_flags, n_remove_lm;
  const uint8_t* remove_flags;  /* n_remove_flags = the window's observation count before this update */
  const int64_t* remove_lm_ids;
} ssx_ba_window_update;
SSX_API ssx_status ssx_ba_window_update_batch(int32_t n, ssx_ba_window* const* wins, const ssx_ba_window_update* updates,
                                              ssx_status* status_out);
/* overwrite the estimate / the fixed flag of a keyframe or landmark of the window (fixed < 0: unchanged; xyz NULL: unchanged) */
SSX_API ssx_status ssx_ba_window_set_pose(ssx_ba_window* win, int64_t kf_id, const double* pose7, int32_t fixed);
SSX_API ssx_status ssx_ba_window_set_landmark(ssx_ba_window* win, int64_t lm_id, const double* xyz, int32_t fixed);
SSX_API ssx_status ssx_ba_window_size(const ssx_ba_window* win, int32_t* n_keyframes, int32_t* n_landmarks,
                                      int32_t* n_observations);
/* the window as an ordinary ssx_ba_problem (current estimate): arrays of ssx_ba_window_size() entries, any may be NULL.
 * Keyframes ascending by id, landmarks ascending by id, observations in the order they were pushed; point_fixed = the flags
 * the next solve uses (fix rule included). */
SSX_API ssx_status ssx_ba_window_export(const ssx_ba_window* win, int64_t* kf_ids, double* poses, uint8_t* pose_fixed,
                                        int64_t* lm_ids, double* points, uint8_t* point_fixed, int32_t* edge_pose,
                                        int32_t* edge_point, double* edge_uv, uint8_t* edge_cam);
/* res->poses_out / points_out / edge_chi2 / edge_outlier (nullable) in the order of ssx_ba_window_export; the window's
 * state becomes the result (the next solve starts from it) */
SSX_API ssx_status ssx_ba_window_solve(ssx_ba_window* win, ssx_ba_result* res);
/* n windows of ONE ctx in one call (one launch sequence for all of them, like ssx_ba_solve_batch): the windows of the
 * concurrent streams of BASELINE configs[4], or of a batch of stereo pairs.  Per window the bits of ssx_ba_window_solve.
 * The options of the first window apply. */
SSX_API ssx_status ssx_ba_window_solve_batch(int32_t n, ssx_ba_window* const* wins, ssx_ba_result* results);
/* A loop correction applied to the window where it lies: LoopClosing::CorrectActivateKeyframeAndMappoint (loopclosing.cpp:378-453)
 * on what the window holds -- every keyframe of a window is active, so this is stage 1 of ssx_loop_correct on the resident state,
 * followed by the fusion of :427-453, which for a window is a removal (below).  One small upload, one download, one synchronisation.
 *   Poses:  T'_cur = corrected_pose7; every other keyframe a gets T'_a = (T_a * T_cur^-1) * corrected_pose7, grouped as :394-397
 *           group it.  pose_fixed is unchanged.
 *   Points: every landmark somebody observes gets p' = T'_a^-1 * (T_a * p); its anchor a is the keyframe of its first active
 *           observation (:408) -- among its remaining observations the keyframe that was PUSHED earliest (not the lowest id;
 *           observations removed as outliers do not count).  Fixed landmarks move as well (the reference moves every active map
 *           point); the fixed flags are unchanged.  A landmark nobody observes is left alone.
 *   Fusion: :439-448 appends the current map point's observations to the loop map point with AddObservation only and calls
 *           Map::RemoveMapPoint(current_mp) (map.cpp:162-173); the loop map point is not inserted into the active map.  So the
 *           landmarks fused_lm_ids (the ids of the current keyframe's map points that had a loop map point to merge into) leave
 *           with all their observations, exactly as ssx_ba_window_remove_landmarks removes them after the correction; ids the
 *           window does not hold are skipped.  The loop map point enters later through an ordinary push with new_fixed = 1.
 * The arithmetic is that of ssx_loop_correct (the same kernels): on the exported window with every keyframe and point active and
 * these anchors, that call returns the same bits.  Afterwards both state buffers and the host mirror hold the corrected state: the
 * next solve starts from it and ssx_ba_window_export returns it.  Edits still pending (a push not yet solved) are sent first.
 * res (nullable), arrays nullable, in the order of ssx_ba_window_export of the window as the call found it:
 *   poses_out n_keyframes x 7, points_out n_landmarks x 3 (the fused ones still among them), anchor_kf_out n_landmarks = the id of
 *   the keyframe each landmark was re-anchored to (-1: nobody observes it).
 * SSX_ERR_INVALID_ARG: win or corrected_pose7 null, n_fused < 0 or n_fused > 0 with null ids, an empty window, cur_kf_id not in
 * the window, a corrected pose that is not finite or whose quaternion is zero.  All are refused before anything is launched; on
 * any failure the window, its mirror and res are unchanged. */
typedef struct ssx_ba_window_loop_result {
  int32_t n_keyframes, n_landmarks;   /* the window when the call began (= ssx_ba_window_size) */
  int32_t n_points_moved;             /* landmarks re-anchored (:417-419) */
  int32_t n_fused_removed;            /* landmarks that left (:447) */
  double* poses_out;
  double* points_out;
  int64_t* anchor_kf_out;
} ssx_ba_window_loop_result;
SSX_API ssx_status ssx_ba_window_loop_correct(ssx_ba_window* win, int64_t cur_kf_id, const double* corrected_pose7, int32_t n_fused,
                                              const int64_t* fused_lm_ids, ssx_ba_window_loop_result* res);

/* (test and tools hooks -- ssx_ba_window_selftest, ssx_debug_*, ssx_ba_debug_*, the kernel taps ssx_ba_linearize / ssx_orb_stage_* /
 * ssx_lk_stage_* -- are NOT part of this ABI: include/ssx_test_hooks.h,
 * compiled out of the library by -DSSX_NO_TEST_HOOKS / SSX_PRODUCT_BUILD=1 python -m ssvio_amd.build) */

/* ------------------------------------------------------------------------------------------------
 * Pose-only robust optimisation -- replaces the g2o part of FrontEnd::EstimateCurrentPose
 * (src/ssvio/frontend.cpp:184-270): one VertexPose, EdgeProjectionPoseOnly per tracked map point
 * (include/ssvio/g2otypes.hpp:67-110), Huber delta 1.0 (g2o default), `rounds` x optimize(`iters`) with
 * chi2 > chi2_th => outlier after every round and the robust kernels dropped before the last round.
 * The whole procedure (all rounds, iterations, LM trials) is ONE kernel launch.
 *   pose_io: initial estimate in, result out;  xyz: M x 3 map points;  uv: M x 2 measured pixels (cv::Point2f
 *   widened to double);  inlier_out[i] = 1 if the feature ends as inlier;  *n_inliers = features.size() - outliers.
 *   Reference defaults: rounds 4, iters 10, chi2_th 5.991, huber_delta 1.0.
 *   Every input value must be finite and no map point may coincide with the camera centre (0 / 0): behaviour on NaN or infinity is undefined.
 * ------------------------------------------------------------------------------------------------ */
SSX_API ssx_status ssx_pose_only_opt(ssx_ctx* ctx, double* pose_io, const double* K4, int32_t M, const double* xyz,
                                     const double* uv, int32_t rounds, int32_t iters, double chi2_th,
                                     double huber_delta, uint8_t* inlier_out, int32_t* n_inliers);

/* n problems in ONE call -- one frame of each of n streams (BASELINE configs[4]; FrontEnd::EstimateCurrentPose is one such problem
 * per frame, frontend.cpp:184-300): one workgroup per problem, one launch, one synchronisation.  Per problem the arguments of
 * ssx_pose_only_opt and, bit for bit, its results. */
typedef struct ssx_pose_only_job {
  double* pose_io; const double* K4; int32_t M; const double* xyz; const double* uv;
  int32_t rounds, iters; double chi2_th, huber_delta;
  uint8_t* inlier_out;        /* nullable */
  int32_t* n_inliers;         /* nullable */
} ssx_pose_only_job;
SSX_API ssx_status ssx_pose_only_opt_batch(ssx_ctx* ctx, int32_t n, const ssx_pose_only_job* jobs);

/* ------------------------------------------------------------------------------------------------
 * ORB extraction -- replaces the bodies of ssvio::ORBextractor::Detect / DetectAndCompute
 * (include/ssvio/orbextractor.hpp:50-59, src/ssvio/orbextractor.cpp:755-842, 687-753) and everything
 * they call: cv::FAST per grid cell, DistributeOctTree, ComputePyramid (cv::resize), IC_Angle
 * (cv::fastAtan2), cv::GaussianBlur 7x7 sigma 2, computeOrbDescriptor (steered BRIEF-256).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {          /* binary layout of cv::KeyPoint (28 bytes) */
  float x, y;             /* pt */
  float size, angle, response;
  int32_t octave, class_id;
} ssx_keypoint;

typedef struct {          /* ORBextractor ctor arguments (orbextractor.hpp:44-45, system.cpp:117-128) */
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t ini_th_fast, min_th_fast;
} ssx_orb_params;

SSX_API void ssx_orb_default_params(ssx_orb_params* p); /* 2000, 1.2, 8, 20, 7 (config/kitti_00.yaml:41-49) */

/* Output capacity `cap` of the two calls below: a pyramid level returns at most max(N_level + 3, 4 * nIni) keypoints
 * (the quadtree stops within 3 nodes of its budget, but its first subdivision already makes up to 4 * nIni <= 256
 * nodes however small the budget is); nfeatures + 260 * nlevels is always enough.  SSX_ERR_CAPACITY otherwise.
 *
 * ORBextractor::Detect: single-level grid FAST + octree.  mask may be NULL (all 255).  Empty image:
 * returns SSX_OK with *n = 0 (the reference silently returns, orbextractor.cpp:758-759).
 * Output: keypoints {pt, size 7, angle -1, response = FAST score, octave 0, class_id -1}. */
SSX_API ssx_status ssx_orb_detect(ssx_ctx* ctx, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                  const uint8_t* mask, int32_t mask_stride, const ssx_orb_params* prm,
                                  int32_t cap, ssx_keypoint* kps_out, int32_t* n);
/* The same with the mask of FrontEnd::DetectFeatures (src/ssvio/frontend.cpp:302-312: 255 everywhere, a FILLED cv::rectangle of
 * pt -+ (10, 10) set to 0 per tracked feature) handed over as its rectangles: boxes_xyxy = n_boxes x (x0, y0, x1, y1), corners
 * INCLUSIVE (cv::rectangle's convention), clipped to the image by the library.  16 bytes per tracked feature cross PCIe instead
 * of rows x cols bytes; the mask is rasterised on the device.  Same keypoints as ssx_orb_detect on the rasterised mask. */
SSX_API ssx_status ssx_orb_detect_boxes(ssx_ctx* ctx, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                        const int32_t* boxes_xyxy, int32_t n_boxes, const ssx_orb_params* prm,
                                        int32_t cap, ssx_keypoint* kps_out, int32_t* n);

/* ssx_orb_detect_boxes for n images in ONE call -- one keyframe of each of n streams (BASELINE configs[4]).  All images rows x cols with
 * one stride and one parameter set; images_on_device != 0: the image pointers are GPU-readable (device or pinned host memory) and are
 * read where they lie.  Per image the bits of ssx_orb_detect_boxes; SSX_ERR_CAPACITY if any image's keypoints do not fit its cap
 * (the others are still returned, *n_out of every job is set). */
typedef struct ssx_orb_detect_job {
  const uint8_t* img; int32_t stride;
  const int32_t* boxes_xyxy; int32_t n_boxes;
  int32_t cap; ssx_keypoint* kps_out; int32_t* n_out;
} ssx_orb_detect_job;
SSX_API ssx_status ssx_orb_detect_boxes_batch(ssx_ctx* ctx, int32_t n, const ssx_orb_detect_job* jobs, int32_t rows, int32_t cols,
                                              const ssx_orb_params* prm, int32_t images_on_device);

/* ORBextractor::DetectAndCompute: 8-level pyramid ORB.  desc_out: cap x 32 bytes (CV_8U N x 32). */
SSX_API ssx_status ssx_orb_extract(ssx_ctx* ctx, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                   const uint8_t* mask, int32_t mask_stride, const ssx_orb_params* prm,
                                   int32_t cap, ssx_keypoint* kps_out, uint8_t* desc_out, int32_t* n);

/* ORBextractor::ScreenAndComputeKPsParams + CalcDescriptors (orbextractor.hpp:54-55,69-71; the loop-closing use,
 * src/ssvio/loopclosing.cpp:622-629): keypoints are GIVEN (level-0 position + octave); those at least 19 px inside
 * their pyramid level that pass the FAST segment test at minThFAST are kept (input order), get angle / size, and
 * are described on the blurred level.  kps_out / desc_out need capacity n_in. */
SSX_API ssx_status ssx_orb_describe_at(ssx_ctx* ctx, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                       const ssx_orb_params* prm, const ssx_keypoint* kps_in, int32_t n_in,
                                       ssx_keypoint* kps_out, uint8_t* desc_out, int32_t* n);

/* ------------------------------------------------------------------------------------------------
 * Stereo association + triangulation.
 * The north_star asks for row-band Hamming matching; the reference itself associates by LK optical flow
 * (FrontEnd::FindFeaturesInRight, src/ssvio/frontend.cpp:346-428) and only matches descriptors in loop
 * closing with OpenCV BruteForce-Hamming (src/ssvio/loopclosing.cpp:105-145) -- whose semantics (minimum
 * distance, lowest train index wins ties) this matcher keeps inside the row band.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  float band_px;            /* |vL - vR| <= band_px * scale_factor^octave_L */
  float min_disp, max_disp; /* uL - uR in [min_disp, max_disp] */
  int32_t max_dist;         /* accept iff best Hamming distance <= max_dist */
  int32_t max_octave_diff;  /* |octave_L - octave_R| <= this */
  float scale_factor;
} ssx_match_params;

SSX_API void ssx_match_default_params(ssx_match_params* p); /* 2, 0, 120, 80, 1, 1.2 */

/* match_idx[i] = index of the right keypoint or -1; dist[i] = best distance found (257 = no candidate). */
SSX_API ssx_status ssx_stereo_match(ssx_ctx* ctx, const ssx_keypoint* kL, const uint8_t* dL, int32_t nL,
                                    const ssx_keypoint* kR, const uint8_t* dR, int32_t nR,
                                    const ssx_match_params* prm, int32_t* match_idx, int32_t* dist);

/* Brute-force Hamming match() of loopclosing.cpp:108 (query -> train), next-row N2. */
SSX_API ssx_status ssx_bf_match(ssx_ctx* ctx, const uint8_t* dq, int32_t nq, const uint8_t* dt, int32_t nt,
                                int32_t* idx, int32_t* dist);

typedef struct {           /* the rig System::GenerateSteroCamera builds (src/ssvio/system.cpp:54-113) */
  double fx, fy, cx, cy;
  double baseline;         /* Camera.Base.Line / fx */
} ssx_stereo_rig;

/* ssvio::triangulation (include/ssvio/algorithm.hpp:23-45) for left = [I|0], right = [I|(-baseline,0,0)] with
 * Camera::pixel2camera (src/ssvio/camera.cpp:25-30); ok = sigma3/sigma2 < 1e-2 && z > 0 (frontend.cpp:466,528).
 * A pair without positive disparity (uL <= uR: a point at or behind infinity, where the sign of z is rounding noise)
 * is reported ok = 0 with a zeroed camera-frame point.
 * T_wc (nullable, 7 doubles) maps the camera-frame point to the world (frontend.cpp:503,531). */
SSX_API ssx_status ssx_triangulate(ssx_ctx* ctx, int32_t n, const double* uvL, const double* uvR,
                                   const ssx_stereo_rig* rig, const double* T_wc, double* xyz_out,
                                   uint8_t* ok_out);
/* n calls of ssx_triangulate in one launch (one keyframe of each of n streams).  Per job the arguments and, bit for bit, the results
 * of ssx_triangulate. */
typedef struct ssx_triangulate_job {
  int32_t n; const double* uvL; const double* uvR; const ssx_stereo_rig* rig; const double* T_wc;   /* T_wc nullable */
  double* xyz_out; uint8_t* ok_out;
} ssx_triangulate_job;
SSX_API ssx_status ssx_triangulate_batch(ssx_ctx* ctx, int32_t n_jobs, const ssx_triangulate_job* jobs);

/* One stereo frame, fully on the device: extract left+right (one batched launch sequence), row-band match,
 * triangulate the matches.  Replaces DetectFeatures + FindFeaturesInRight + BuidInitMap/TriangulateNewPoints
 * of the front-end (frontend.cpp:302-544) for the north_star pipeline.  All outputs are optional. */
typedef struct {
  int32_t cap;                    /* capacity of every per-keypoint array below */
  ssx_keypoint *kpsL, *kpsR;
  uint8_t *descL, *descR;         /* cap x 32 */
  int32_t nL, nR;                 /* out */
  int32_t* match_idx;             /* nL */
  int32_t* match_dist;            /* nL */
  double* xyz;                    /* nL x 3 (valid where ok) */
  uint8_t* ok;                    /* nL */
  int32_t n_matched, n_triangulated;  /* out */
} ssx_stereo_frame_out;

SSX_API ssx_status ssx_stereo_frame(ssx_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int32_t stride,
                                    int32_t rows, int32_t cols, const ssx_orb_params* orb,
                                    const ssx_match_params* mp, const ssx_stereo_rig* rig, const double* T_wc,
                                    ssx_stereo_frame_out* out);

/* Batched, device-resident variant for throughput: `pairs` stereo pairs already in HBM
 * (imgs_dev = [pairs][2][rows][stride] u8, DEVICE pointer).  Results stay on the device inside the ctx;
 * counts_out (host, pairs x 4 int32: nL, nR, n_matched, n_triangulated) is the only download.
 * Use ssx_stereo_batch_fetch to copy one pair's results out afterwards. */
SSX_API ssx_status ssx_stereo_batch_dev(ssx_ctx* ctx, int32_t pairs, const uint8_t* imgs_dev, int32_t stride,
                                        int32_t rows, int32_t cols, const ssx_orb_params* orb,
                                        const ssx_match_params* mp, const ssx_stereo_rig* rig,
                                        int32_t* counts_out);
SSX_API ssx_status ssx_stereo_batch_fetch(ssx_ctx* ctx, int32_t pair, ssx_stereo_frame_out* out);
/* Batches that arrive from the HOST, as the reference's loop hands System::RunStep a fresh pair at every step
 * (test/test_system.cpp:36-47).  imgs_host = [pairs][2][rows][stride] u8 in host memory (pinned: the upload is then
 * asynchronous).  The images go up on a copy stream of the ctx's own into one of two device buffers; a batch's pipeline waits
 * for its own upload only.
 *   ssx_stereo_batch_upload  start the upload of a batch and return (at most two uploaded batches may be waiting); imgs_host
 *                            must stay untouched until the batch has been run and a later call of these functions returned
 *   ssx_stereo_batch_run     enqueue the whole front-end on the OLDEST uploaded batch; nothing is synchronised
 *   ssx_stereo_batch_host    upload + run in one call
 *   ssx_stereo_batch_counts  the counts of the OLDEST batch that was run and not collected yet (at most two may be waiting): waits
 *                            for that batch only; counts_out = pairs x 4 int32: nL, nR, n_matched, n_triangulated.
 *                            A run that failed after it consumed its batch still owns its place in this FIFO: the counts call
 *                            that collects it returns the run's status, and the batches around it keep their own counts.
 *                            ssx_stereo_batch_fetch copies one pair's keypoints / matches / points of the batch run LAST -- after
 *                            run(k + 1); counts() -> batch k, a fetch reads batch k + 1: fetch a batch before the next one is run.
 * A server keeps one upload ahead and collects one batch behind -- upload(k + 1); run(k); ...; counts() -> batch k - 1 -- so that
 * batch k + 1 crosses PCIe and batch k's front-end runs while the host waits for nothing but its own backend (bench.py's
 * headline region); counts() right after run(k) returns batch k's counts once it is done. */
SSX_API ssx_status ssx_stereo_batch_upload(ssx_ctx* ctx, int32_t pairs, const uint8_t* imgs_host, int32_t stride, int32_t rows,
                                           int32_t cols);
SSX_API ssx_status ssx_stereo_batch_run(ssx_ctx* ctx, const ssx_orb_params* orb, const ssx_match_params* mp,
                                        const ssx_stereo_rig* rig);
SSX_API ssx_status ssx_stereo_batch_host(ssx_ctx* ctx, int32_t pairs, const uint8_t* imgs_host, int32_t stride, int32_t rows,
                                         int32_t cols, const ssx_orb_params* orb, const ssx_match_params* mp,
                                         const ssx_stereo_rig* rig);
SSX_API ssx_status ssx_stereo_batch_counts(ssx_ctx* ctx, int32_t* counts_out);
/* Timing hook: enqueue the batch again on the already-resident inputs WITHOUT any host synchronisation or
 * download (bench.py brackets a run of these with HIP events). */
SSX_API ssx_status ssx_stereo_batch_enqueue(ssx_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * N1: pyramidal Lucas-Kanade tracking.
 * Replaces the two cv::calcOpticalFlowPyrLK calls of the reference front-end:
 *   FrontEnd::TrackLastFrame        /root/reference/src/ssvio/frontend.cpp:130-182 (call at :156-166)
 *   FrontEnd::FindFeaturesInRight   /root/reference/src/ssvio/frontend.cpp:346-428 (call at :374-384)
 * both with cv::Size(11,11), maxLevel 3, TermCriteria(COUNT+EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW.
 * Semantics of OpenCV 3.x calcOpticalFlowPyrLK: buildOpticalFlowPyramid (pyrDown, REFLECT_101 border, the pyramid
 * stops before a level not larger than the window), Scharr derivatives, 14-bit bilinear weights, status = 0 when
 * the window leaves the image or the smaller eigenvalue of the normal matrix falls below the threshold, err =
 * mean absolute patch difference / 32 at level 0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_lk_params {
  int32_t win;                /* winSize (square, odd, 3..15): 11 */
  int32_t max_level;          /* maxLevel: 3 */
  int32_t max_iters;          /* TermCriteria COUNT: 30 */
  double eps;                 /* TermCriteria EPS: 0.01 (compared squared against |delta|^2) */
  float min_eig_threshold;    /* minEigThreshold: 1e-4 */
  int32_t use_initial_flow;   /* OPTFLOW_USE_INITIAL_FLOW: next_pts holds the initial guesses */
} ssx_lk_params;
SSX_API void ssx_lk_default_params(ssx_lk_params* p);
/* prev / next: host images rows x cols (8-bit, strides in bytes); prev_pts: n x 2 floats (x, y); next_pts: n x 2
 * floats, in (initial guess when use_initial_flow) and out; status: n bytes; err: n floats or NULL;
 * top_level (optional): the top pyramid level actually used. */
SSX_API ssx_status ssx_lk_track(ssx_ctx* ctx, const uint8_t* prev, int32_t prev_stride, const uint8_t* next,
                                int32_t next_stride, int32_t rows, int32_t cols, int32_t n, const float* prev_pts,
                                float* next_pts, uint8_t* status, float* err, const ssx_lk_params* prm,
                                int32_t* top_level);
/* Frame-to-frame chaining (FrontEnd::TrackLastFrame calls LK on (last, current) every frame, frontend.cpp:156-166):
 * the previous image is the `next` image of the last ssx_lk_track / ssx_lk_track_next call on this context, whose
 * pyramid is still on the device -- only the new image is uploaded and reduced. Same results as ssx_lk_track on the
 * two images; SSX_ERR_INVALID_ARG when there is no such call or the size / window / max_level changed. A context
 * holds one chain: keep the left-right stereo LK calls of a keyframe on a second context.
 * A context holds chains for ONE key (rows, cols, win, max_level) at a time.  A successful call with another key re-plans the
 * context for that key and DROPS EVERY CHAIN it held, on all slots: the next chained call with the earlier key is refused
 * (SSX_ERR_INVALID_ARG, nothing is run, next_pts stays as passed) until a call with both images has started a new chain.
 * Streams of different image sizes therefore need a context per size. */
SSX_API ssx_status ssx_lk_track_next(ssx_ctx* ctx, const uint8_t* next, int32_t next_stride, int32_t rows,
                                     int32_t cols, int32_t n, const float* prev_pts, float* next_pts,
                                     uint8_t* status, float* err, const ssx_lk_params* prm, int32_t* top_level);
/* n_jobs tracking problems in ONE call -- one frame of each of n_jobs streams (BASELINE configs[4]): every kernel of the tracker runs
 * once for all jobs.  A job names the SLOT of the context that holds its pyramids (0 .. 4095; ssx_lk_track / _next use slot 0; a
 * slot at most once per call); prev == NULL chains it to the slot's last job like ssx_lk_track_next.  All jobs share rows x cols
 * and prm -- the context's one key (see ssx_lk_track_next: a call with another size drops the chains of ALL slots, so the jobs of
 * streams with different image sizes go to different contexts, not to one context in turn).
 * images_on_device != 0: the image pointers are readable by the GPU -- device memory, or pinned host memory
 * (hipHostMalloc / hipHostRegister) -- and nothing is staged; 0: ordinary host memory.  The images are then read where they lie,
 * which asks of the caller: (1) every image, rows x stride bytes from its pointer up to the end of its last row, lies inside ONE
 * allocation the HIP runtime knows (hipMalloc, hipHostMalloc / ssx_host_alloc, hipHostRegister), readable from this context's
 * device; (2) it stays allocated and unchanged until the call returns.  The images of different jobs may be separate allocations
 * anywhere.  When the `next` images ascend at a constant distance AND the runtime confirms that the first and the last lie in one
 * allocation that covers the whole range (a pinned arena with a slice per stream), that range crosses PCIe in one copy, bytes
 * between the images included; images allocated one by one are copied or read one by one, however close they lie.
 * Per job the bits of ssx_lk_track / ssx_lk_track_next. */
typedef struct ssx_lk_job {
  int32_t slot;
  const uint8_t* prev; int32_t prev_stride;      /* NULL: the slot's last `next` image */
  const uint8_t* next; int32_t next_stride;
  int32_t n; const float* prev_pts; float* next_pts; uint8_t* status; float* err;   /* err nullable */
} ssx_lk_job;
SSX_API ssx_status ssx_lk_track_batch(ssx_ctx* ctx, int32_t n_jobs, const ssx_lk_job* jobs, int32_t rows, int32_t cols,
                                      const ssx_lk_params* prm, int32_t images_on_device);
/* ------------------------------------------------------------------------------------------------
 * Image undistortion: Camera::UndistortImage (src/ssvio/camera.cpp:43-55, a cv::undistort with the camera matrix and
 * k1 k2 p1 p2), which FrontEnd::GrabSteroImage applies to both images when Camera.NeedUndistortion is set (frontend.cpp:39-45).
 * The contract is tools/undistort_model.py: the map in f64, operation by operation, quantised to 1/32 pixel; integer
 * bilinear weights (the 10-bit products of the 5-bit fractions); taps outside the image read 0, each on its own; a non-finite or
 * far-away source position yields 0.  K = (fx, fy, cx, cy); dist = (k1, k2, p1, p2, k3); iR = the inverse of newK * R, row-major
 * (the caller's: a rectifying rotation costs nothing).  ssx_undistort_default fills iR for the reference's case, R = I and
 * newK = K: [1/fx, 0, -cx/fx, 0, 1/fy, -cy/fy, 0, 0, 1]; it is host code and needs no device (a null argument: nothing is written).
 *
 * ssx_undistort: n jobs (0 .. SSX_UNDISTORT_MAX_JOBS; a stereo pair is n = 2) of one size rows x cols, 8-bit, strides in bytes, each
 * with its own parameters, in ONE launch; one upload, one download and one synchronisation whatever n is.
 * images_on_device != 0: src and dst are read and written where they lie -- device memory or pinned host memory, under the rules
 * ssx_lk_track_batch states -- so a buffer of ssx_host_alloc filled by this call can go straight into
 * ssx_lk_track_batch(..., images_on_device = 1); 0: ordinary host memory.  Bytes of dst beyond cols in a pitched row are untouched.
 * SSX_ERR_INVALID_ARG with a message, before anything is touched: n < 0 or above the limit, a null pointer, a stride smaller than
 * cols, rows or cols < 1, a dst that overlaps any src of the call (there is no in-place form: the reference clones the source).
 * SSX_ERR_UNSUPPORTED: rows or cols above 32768.
 * ------------------------------------------------------------------------------------------------ */
#define SSX_UNDISTORT_MAX_JOBS 1024
typedef struct { double K[4]; double dist[5]; /* k1 k2 p1 p2 k3 */ double iR[9]; } ssx_undistort_params;
typedef struct { const uint8_t* src; int32_t src_stride; uint8_t* dst; int32_t dst_stride; ssx_undistort_params prm; } ssx_undistort_job;
SSX_API void ssx_undistort_default(const double K4[4], const double dist5[5], ssx_undistort_params* out);
SSX_API ssx_status ssx_undistort(ssx_ctx* ctx, int32_t n, const ssx_undistort_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device);
/* The batched form over many streams: a PLAN holds, for one image size, the stored maps of the cameras it was shown, and applies them
 * to n images in one launch without f64.  The streams of a cohort usually share one rig: one stored map per camera serves them all.
 * The stored form of a map is tools/undistort_model.py's pack_map -- per pixel three u16: X0 + 2 and Y0 + 2 (the integer position,
 * clamped to [-2, cols] and [-2, rows]: the clamp keeps every tap's inside / outside test) and a | b << 5 (the two 5-bit fractions);
 * in memory three planes at a pitch of cols rounded up to 4: 2.8 MB at 1241 x 376, so SSX_UNDISTORT_PLAN_MAX_MAPS of them 179 MB of HBM.
 * The result of ssx_undistort_plan_apply is, byte for byte, ssx_undistort's.
 *
 * ssx_undistort_plan_create: rows, cols >= 1 (SSX_ERR_INVALID_ARG) and at most 65533 a side (SSX_ERR_UNSUPPORTED: position + 2 is a
 * u16).  The plan lives on ctx (its stream, its error text) and is destroyed before it.
 * ssx_undistort_plan_add: the index of the parameter set's map.  A set whose bytes equal those of an earlier one gets that one's index
 * and nothing is launched; a new set launches k_undistort_map once (and synchronises).  Beyond SSX_UNDISTORT_PLAN_MAX_MAPS:
 * SSX_ERR_CAPACITY with a message, the plan unchanged.
 * ssx_undistort_plan_apply: n jobs (0 .. SSX_UNDISTORT_MAX_JOBS), each naming a map of the plan, in ONE launch and with ONE
 * synchronisation whatever n is and whatever maps the jobs name.  images_on_device = 0: ordinary host memory, staged like
 * ssx_undistort (one copy up, one copy down).  images_on_device != 0: every pointer is device memory or pinned host memory.  Device
 * images are read and written where they lie.  Host images are never read or written by the kernel tap by tap across PCIe: they are
 * copied to the device and the results copied back by the DMA engines -- the sources in ONE copy when they stand in job order
 * ascending, at distances of at least one image, in ONE allocation (an ssx_host_alloc arena, a slice per stream; the rule of
 * ssx_lk_track_batch, the runtime asked whether the range really is one allocation), else one copy per image; the results in ONE copy
 * when the destinations stand so, at one constant distance and at a stride of cols (the copy then writes the images' bytes and
 * nothing between them), else one copy per image, which writes the pixels and leaves the pitch bytes alone.
 * SSX_ERR_INVALID_ARG with a message, before anything is touched: every refusal of ssx_undistort, a map index the plan does not hold,
 * and with images_on_device != 0 a pointer that is neither device nor pinned memory. */
#define SSX_UNDISTORT_PLAN_MAX_MAPS 64
typedef struct ssx_undistort_plan ssx_undistort_plan;
typedef struct { const uint8_t* src; int32_t src_stride; uint8_t* dst; int32_t dst_stride; int32_t map; } ssx_undistort_plan_job;
SSX_API ssx_status ssx_undistort_plan_create(ssx_ctx* ctx, int32_t rows, int32_t cols, ssx_undistort_plan** plan);
SSX_API ssx_status ssx_undistort_plan_add(ssx_undistort_plan* plan, const ssx_undistort_params* prm, int32_t* map_index);
SSX_API ssx_status ssx_undistort_plan_apply(ssx_undistort_plan* plan, int32_t n, const ssx_undistort_plan_job* jobs, int32_t images_on_device);
SSX_API ssx_status ssx_undistort_plan_size(const ssx_undistort_plan* plan, int32_t* rows, int32_t* cols, int32_t* n_maps);
SSX_API void ssx_undistort_plan_destroy(ssx_undistort_plan* plan);
/* Dense stereo: a disparity for every pixel of a rectified pair, by census + semi-global matching.  The contract is
 * tools/dense_model.py, integers only, and the device is held to it bit for bit: a 9 x 7 census with a replicated
 * border, Hamming cost (63 where x - d < 0), `paths` (4 or 8) path directions with penalties 1 <= p1 <= p2 <= 192, the first minimum
 * of the summed volume, a uniqueness margin in percent (0 .. 99), a left-right check of lr_tolerance whole disparities (-1: off,
 * at most `disparities`) against the right disparity of the same volume, and an integer sub-pixel step.  disparities is 64 or 128, the
 * minimum disparity is 0.  Output: int16 in 1/16 pixel, -16 where a pixel is invalid.
 * ssx_stereo_dense: n pairs (0 .. SSX_DENSE_MAX_JOBS) of one size rows x cols (40 .. 4000 a side), 8-bit, image strides in bytes and
 * disp_stride in elements, each at least cols.  images_on_device == 0: host memory, staged -- ONE copy up (the job table and the
 * images), ONE copy down (the maps), ONE synchronisation.  images_on_device != 0: every pointer is device memory or pinned host
 * memory (ssx_host_alloc) and is read and written where it lies; only the job table goes up.  The census words, the summed volume and
 * the right keys are workspace of the context: (20 + 2 disparities) bytes per pixel and pair.  A call works through its pairs in
 * groups whose workspace stays under SSX_DENSE_WORKSPACE_CAP, six launches (two of them fills) per group whatever the image size or
 * content -- four with lr_tolerance = -1; one pair always runs, whatever it takes (4000 x 4000 at 128: 4.4 GB).
 * SSX_ERR_INVALID_ARG with a message in ssx_last_error, before anything is touched or launched: a parameter out of range, a
 * non-zero `reserved`, a null prm / jobs / image / disp, a stride below cols, n or a side out of range. */
typedef struct { int32_t disparities, p1, p2, uniqueness, lr_tolerance, paths, reserved[2]; } ssx_dense_params;
typedef struct { const uint8_t* left; int32_t left_stride; const uint8_t* right; int32_t right_stride;
                 int16_t* disp; int32_t disp_stride; /* in elements */ } ssx_dense_job;
#define SSX_DENSE_MAX_JOBS 1024
#define SSX_DENSE_WORKSPACE_CAP (1ull << 30) /* bytes: 8 pairs of 1241 x 376 at 128 disparities */
SSX_API void ssx_dense_default_params(ssx_dense_params* p); /* 128, 7, 86, 10, 1, 8 */
SSX_API ssx_status ssx_stereo_dense(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, int32_t rows, int32_t cols,
                                    const ssx_dense_params* prm, int32_t images_on_device);
/* What follows a disparity map: the speckle filter and the samples a keyframe keeps.  The contract is tools/dense_post_model.py
 * (DESIGN.md 6p), integers only, bit for bit.  A pixel is valid iff its value is > 0.  Two 4-neighbours are joined iff both are valid
 * and differ by at most speckle_range (1/16 pixel; row ends and the maps of two jobs are no neighbours); every valid pixel whose
 * connected component has at most speckle_size pixels becomes -16 (the rule of cv::filterSpeckles with newVal = -16); speckle_size = 0:
 * no filter.  cloud_stride > 0: every cloud_stride-th pixel of every cloud_stride-th row of the FILTERED map whose value is at least
 * cloud_min_disp16 (ssx_dense_min_disp16: the depth bar z = bf * 16 / disp16 <= max_depth as one integer) is written as an
 * ssx_dense_sample, in raster order.
 * clouds: a host array of n, null if and only if cloud_stride == 0.  samples: host memory, or with on_device device / pinned memory,
 * 8-byte aligned; capacity at least ceil(rows / stride) * ceil(cols / stride), so nothing can overflow; count is written after the
 * call's one synchronisation.
 * ssx_dense_postprocess: the stage on the caller's maps -- jobs[k].disp is read and written in place, left is needed only with
 * cloud_stride > 0, right is ignored.  ssx_stereo_dense_post: the launches of ssx_stereo_dense followed by the stage's on the same
 * stream; jobs[k].disp may be null when clouds is given (then no map comes down).  With speckle_size = 0 and cloud_stride = 0 it
 * writes the bytes of ssx_stereo_dense.  Per call ONE copy up, ONE copy down (its size a function of the shapes and the settings: the
 * counts travel with the samples) and ONE synchronisation; per group at most six launches more (four for the filter, two for the
 * samples), whatever the image size or content.  Labels and sizes (8 bytes a pixel) take the place of the census words in the chained
 * call; the stand-alone call carves them from the same workspace under SSX_DENSE_WORKSPACE_CAP.
 * SSX_ERR_INVALID_ARG with a message before anything is touched: the refusals of ssx_stereo_dense, a field of post out of range, a
 * non-zero `reserved`, clouds given or missing against cloud_stride, null samples, a capacity too small.  SSX_ERR_HIP with a message
 * if a labelling loop ever passed its bound (derived from the pixel count; not reachable by a map). */
typedef struct { int32_t speckle_size;      /* 0 = no filter; 0 .. rows * cols */
                 int32_t speckle_range;     /* 1/16 pixel, 0 .. 32767 */
                 int32_t cloud_stride;      /* 0 = no samples; else 1 .. 4000 */
                 int32_t cloud_min_disp16;  /* 1 .. 32768 */
                 int32_t reserved[4]; } ssx_dense_post;                       /* 32 bytes, reserved must be 0 */
typedef struct { uint16_t u, v; int16_t disp16; uint8_t intensity, reserved; } ssx_dense_sample;   /* 8 bytes */
typedef struct { ssx_dense_sample* samples; int32_t capacity; int32_t count; /* out */ } ssx_dense_cloud;  /* 16 bytes */
SSX_API void ssx_dense_default_post(ssx_dense_post* p); /* 0, 16, 0, 1: everything off; null is no fault */
SSX_API int32_t ssx_dense_min_disp16(double bf, double max_depth); /* host code: the smallest d in 1 .. 32767 with bf * 16 / d <= max_depth (f64), else 32768 */
SSX_API ssx_status ssx_dense_postprocess(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, ssx_dense_cloud* clouds, int32_t rows, int32_t cols,
                                         const ssx_dense_post* post, int32_t on_device);
SSX_API ssx_status ssx_stereo_dense_post(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, ssx_dense_cloud* clouds, int32_t rows, int32_t cols,
                                         const ssx_dense_params* prm, const ssx_dense_post* post, int32_t images_on_device);
/* Raw stereo rigs: lens models and rectification.  The contract is tools/rectify_model.py.
 * A lens is SSX_LENS_RADTAN -- coeffs = k1 k2 p1 p2 k3, the map of ssx_undistort, whose entry points are this case -- or SSX_LENS_KB4,
 * Kannala-Brandt "equidistant" with coeffs = k1 k2 k3 k4 (coeffs[4] is ignored): theta_d = theta (1 + k1 theta^2 + ... + k4 theta^8),
 * theta = atan(r) by the contract's own atan_c in f64 operations (no library atan); a pixel whose ray has W <= 0 (behind the camera,
 * or NaN) is 0.  `reserved` is 0.
 * ssx_undistort_lens / ssx_undistort_plan_add_lens: ssx_undistort / ssx_undistort_plan_add with a lens model per job / per map --
 * their refusals, limits, images_on_device rules and counters; jobs of mixed models are ONE launch.  In addition a model that is
 * neither of the two is SSX_ERR_INVALID_ARG before anything is touched.  Two parameter sets are one map when their bytes are equal;
 * a RADTAN set finds the map its ssx_undistort_params form was added as, and the other way round.
 * ssx_stereo_rectify: host arithmetic (+ - * / sqrt only, no ctx, no device), rectify() of the contract bit for bit.  rig: the two
 * cameras (left, right; iR ignored), X_right = R X_left + t (R row-major), and f, cx, cy of the common camera (0: the mean of the
 * four focal lengths / of the two principal points).  out: the rectifying rotations, newK = (f, f, cx, cy), the baseline, and the two
 * cameras with iR filled in, ready for the two calls above; the rectified right camera sits at (-baseline, 0, 0).
 * SSX_ERR_INVALID_ARG, the reason in why (nullable, why_cap bytes, always terminated), out untouched: a null rig or out, an unknown
 * model, a non-finite input, a zero baseline, max|R R^T - I| > 1e-6, a right camera that is not to the right (vertical and reversed
 * rigs), optical axes along the baseline. */
enum { SSX_LENS_RADTAN = 0, SSX_LENS_KB4 = 1 };
typedef struct { int32_t model, reserved; double K[4]; double coeffs[5]; double iR[9]; } ssx_lens_params;
typedef struct { const uint8_t* src; int32_t src_stride; uint8_t* dst; int32_t dst_stride; ssx_lens_params prm; } ssx_lens_job;
SSX_API ssx_status ssx_undistort_lens(ssx_ctx* ctx, int32_t n, const ssx_lens_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device);
SSX_API ssx_status ssx_undistort_plan_add_lens(ssx_undistort_plan* plan, const ssx_lens_params* prm, int32_t* map_index);
typedef struct { ssx_lens_params cam[2]; double R[9], t[3]; double f, cx, cy; } ssx_stereo_raw_rig;
typedef struct { double R_l[9], R_r[9], newK[4], baseline; ssx_lens_params cam[2]; } ssx_stereo_rectified;
SSX_API ssx_status ssx_stereo_rectify(const ssx_stereo_raw_rig* rig, ssx_stereo_rectified* out, char* why, int32_t why_cap);
/* ------------------------------------------------------------------------------------------------
 * N3: pose-graph optimisation.
 * Replaces the optimisation of LoopClosing::PoseGraphOptimization
 * (/root/reference/src/ssvio/loopclosing.cpp:458-539): one VertexPose per keyframe (pose_fixed = the initial, the
 * active and the loop keyframes, :484-489), one EdgePoseGraph per temporal (:502-514) or loop (:515-528) constraint
 * with error log(M^-1 T_i T_j^-1) (include/ssvio/g2otypes.hpp:164-176), identity information, no robust kernel,
 * g2o numeric Jacobians, Levenberg-Marquardt, optimizer.optimize(iterations = 20).
 * poses are T_cw as (qx qy qz qw tx ty tz), in/out (fixed keyframes are returned unchanged).
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_pose_graph_problem {
  int32_t n_poses;
  int32_t n_edges;
  double* poses;                /* n_poses x 7, in/out */
  const uint8_t* pose_fixed;    /* n_poses */
  const int32_t* edge_i;        /* n_edges: vertex 0 of the edge (the keyframe itself) */
  const int32_t* edge_j;        /* n_edges: vertex 1 (its predecessor / its loop keyframe) */
  const double* edge_meas;      /* n_edges x 7: the measured relative pose T_i * T_j^-1 */
  double* edge_err_out;         /* optional, n_edges x 6: the edges' errors of the last evaluation */
  int32_t stats_cap;            /* optional per-iteration statistics (chi2 after the iteration, lambda, trials) */
  double* stats_chi2;
  double* stats_lambda;
  int32_t* stats_trials;
} ssx_pose_graph_problem;
typedef struct ssx_pose_graph_result {
  int32_t n_iters;              /* LM iterations executed (0: nothing to optimise) */
  int32_t stats_n;
  double chi2_initial;
  double chi2_final;
} ssx_pose_graph_result;
SSX_API ssx_status ssx_pose_graph_opt(ssx_ctx* ctx, const ssx_pose_graph_problem* prob, int32_t iterations,
                                      ssx_pose_graph_result* res);

/* ------------------------------------------------------------------------------------------------
 * Bag of words for loop detection -- replaces ORBVocabulary::transform / ::score, i.e.
 * DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ssvio/orbvocabulary.hpp:10) as LoopClosing uses it:
 *   dbow2_vocabulary_->transform(desc, keyframe->bow2_vec_)      src/ssvio/loopclosing.cpp:633
 *   dbow2_vocabulary_->score(current->bow2_vec_, db->bow2_vec_)  src/ssvio/loopclosing.cpp:84
 * The vocabulary is a k-ary tree of 32-byte descriptors kept in HBM; a descriptor descends to the child with the
 * smallest Hamming distance (the first one on ties) until it reaches a leaf = its word
 * (thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1217-1260).  L1_NORM scoring only (what ORBvoc.txt declares).
 * A vocabulary belongs to the context it was created on and must be destroyed before it.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_vocabulary ssx_vocabulary;
/* Flat tree: node 0 = root; node i >= 1: parent[i] (< i), is_leaf[i], desc[32 i .. 32 i + 31], weight[i]; entry 0 of
 * each array is ignored.  Word ids number the leaves in node order.  weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY
 * (DBoW2::WeightingType); scoring must be 0 (L1_NORM). */
SSX_API ssx_status ssx_voc_create(ssx_ctx* ctx, int32_t k, int32_t L, int32_t scoring, int32_t weighting, int32_t n_nodes,
                                  const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                                  const double* weight, ssx_vocabulary** out);
/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1337-1420): the ORBvoc.txt format */
SSX_API ssx_status ssx_voc_load_text(ssx_ctx* ctx, const char* path, ssx_vocabulary** out);
SSX_API void ssx_voc_destroy(ssx_vocabulary* voc);
SSX_API ssx_status ssx_voc_info(const ssx_vocabulary* voc, int32_t* k, int32_t* L, int32_t* n_nodes, int32_t* n_words,
                                int32_t* weighting);
/* transform(): desc = n x 32 bytes.  words_out / weights_out (n each, nullable): word id and node weight of every
 * feature (-1 / 0 when the vocabulary is empty).  ids_out / vals_out (capacity cap): the BowVector -- word ids in
 * ascending order with their L1-normalised values; *n_entries = its size (SSX_ERR_CAPACITY when cap is too small,
 * except cap == 0 with ids_out == NULL: only the size and the per-feature outputs are wanted). */
SSX_API ssx_status ssx_voc_transform(ssx_vocabulary* voc, const uint8_t* desc, int32_t n, int32_t* words_out,
                                     double* weights_out, int32_t cap, int32_t* ids_out, double* vals_out,
                                     int32_t* n_entries);
/* L1Scoring::score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of two BowVectors; host arithmetic, in [0, 1] */
SSX_API double ssx_bow_score_l1(int32_t n1, const int32_t* id1, const double* v1, int32_t n2, const int32_t* id2,
                                const double* v2);

/* ------------------------------------------------------------------------------------------------
 * The keyframe database of loop closing, resident on the device -- replaces key_frame_database_ with the two functions
 * that read it:
 *   AddToKeyframeDatabase   src/ssvio/loopclosing.cpp:646-649
 *   DetectLoop              src/ssvio/loopclosing.cpp:72-103
 *   MatchFeatures           src/ssvio/loopclosing.cpp:105-145
 * Every keyframe's BowVector and pyramid descriptors stay in HBM; a query uploads only the current keyframe's.
 * A database belongs to the context it was created on and must be destroyed before it.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_kf_database ssx_kf_database;
/* keyframes_hint sizes the first allocation (about 48 KB per keyframe); the database grows as needed */
SSX_API ssx_status ssx_kfdb_create(ssx_ctx* ctx, int32_t keyframes_hint, ssx_kf_database** out);
SSX_API void ssx_kfdb_destroy(ssx_kf_database* db);
SSX_API ssx_status ssx_kfdb_size(const ssx_kf_database* db, int32_t* n_keyframes, int64_t* n_bow_entries,
                                 int64_t* n_descriptors);
/* AddToKeyframeDatabase: the BowVector (ids ascending, values) and optionally the keyframe's pyramid descriptors
 * (n_desc x 32) with the class_id of each (the feature index ProcessNewKeyframe writes, loopclosing.cpp:610-616).
 * desc == NULL: the keyframe is stored without descriptors and cannot be matched against.  kf_id must be greater than
 * every id already stored (the std::map's order); otherwise, or when the word ids do not ascend, SSX_ERR_INVALID_ARG. */
SSX_API ssx_status ssx_kfdb_add(ssx_kf_database* db, int64_t kf_id, int32_t n_bow, const int32_t* ids, const double* vals,
                                int32_t n_desc, const uint8_t* desc, const int32_t* class_id);
/* DetectLoop for a current keyframe (query_kf_id, BowVector with ascending ids).  The stored keyframes with
 * query_kf_id - kf_id >= min_id_gap (the reference: 20) are eligible: a prefix in id order, *n_scored of them.
 * scores_out (nullable, capacity scores_cap >= *n_scored, else SSX_ERR_CAPACITY): scores_out[i] is, bit for bit,
 * ssx_bow_score_l1(query, i-th stored keyframe); 0 where either BowVector is empty (the reference skips those).
 * The winner is the reference's: scores narrowed to float, the maximum starts at 0, a strictly greater score replaces
 * it (so the lowest id wins among equal floats).  *found = 0 when no score is above 0 or the best float score is below
 * threshold (Loop.Threshold.Heigher); best_kf_id / best_score (nullable) are written only when *found = 1. */
SSX_API ssx_status ssx_kfdb_detect_loop(ssx_kf_database* db, int64_t query_kf_id, int32_t n_bow, const int32_t* ids,
                                        const double* vals, int32_t min_id_gap, float threshold, int32_t* found,
                                        int64_t* best_kf_id, float* best_score, int32_t scores_cap, double* scores_out,
                                        int32_t* n_scored);
/* MatchFeatures against a stored keyframe: cv::BFMatcher(NORM_HAMMING)::match(loop, current) as ssx_bf_match does it
 * (query = the stored descriptors, train = cur_desc, n_cur <= 65535 else SSX_ERR_UNSUPPORTED), *min_distance = the
 * smallest distance of all matches, a match is kept when dist <= max(2 * min_distance, 30), and a kept match gives the
 * pair (cur_class_id[train], class_id[query]).  pairs_out (cap x 2) receives the reference's std::set: unique pairs in
 * ascending (current, loop) order; *n_pairs = their number (SSX_ERR_CAPACITY when cap is smaller, with the first cap
 * pairs written).  No descriptors on either side: zero pairs, *min_distance = -1.  SSX_ERR_INVALID_ARG for a
 * loop_kf_id that is not stored or was stored without descriptors.  The "fewer than 10 pairs" verdict
 * (loopclosing.cpp:139) is the caller's. */
SSX_API ssx_status ssx_kfdb_match_features(ssx_kf_database* db, int64_t loop_kf_id, int32_t n_cur, const uint8_t* cur_desc,
                                           const int32_t* cur_class_id, int32_t cap, int32_t* pairs_out, int32_t* n_pairs,
                                           int32_t* min_distance);

/* The per-keyframe step of LoopClosingThread (src/ssvio/loopclosing.cpp:39-70) as ONE call: ProcessNewKeyframe (:596-634:
 * the left features replicated over the pyramid levels :607-619, ScreenAndComputeKPsParams + CalcDescriptors :622-629,
 * dbow2_vocabulary_->transform :633), DetectLoop (:72-103) when more than min_db_size keyframes are stored (:48), and
 * MatchFeatures (:105-145) against the winner.  Only the image and the features go up; only this result and the pairs
 * come down (one synchronisation, two when a loop was found).  The keyframe's pyramid keypoints, descriptors, class ids
 * and BowVector stay on the device as the PENDING keyframe of the database, for ssx_kfdb_add_pending. */
typedef struct ssx_kfdb_step_result {
  int32_t n_pyramid;     /* pyramid keypoints that survive ScreenAndComputeKPsParams = descriptors of the keyframe */
  int32_t n_bow;         /* entries of its BowVector */
  int32_t detect_ran;    /* stored keyframes > min_db_size (loopclosing.cpp:48) */
  int32_t n_scored;      /* eligible stored keyframes, as ssx_kfdb_detect_loop; 0 when detection did not run */
  int32_t found;         /* DetectLoop's verdict */
  float   score;         /* the winner's float score (found only) */
  int64_t loop_kf_id;    /* (found only) */
  int32_t n_pairs;       /* set_valid_feature_matches_.size(); 0 when !found */
  int32_t min_distance;  /* as ssx_kfdb_match_features; -1 when !found or no match exists */
} ssx_kfdb_step_result;
/* features[i] = features_left_[i]->kp_position_; pyramid keypoint i * pyramid_levels + level is a copy of it with
 * octave = level, response = -1, class_id = i.  Every result is, bit for bit, what ssx_orb_describe_at on that list,
 * ssx_voc_transform of its descriptors, ssx_kfdb_detect_loop(kf_id, that BowVector, min_id_gap, threshold) and
 * ssx_kfdb_match_features(the winner, those descriptors and class ids) return.  pairs_out (pairs_cap x 2) as there:
 * SSX_ERR_CAPACITY when pairs_cap is smaller than res->n_pairs, with the first pairs_cap pairs written and the keyframe
 * still pending.  The "fewer than 10 pairs" verdict (:139) is the caller's.  SSX_ERR_UNSUPPORTED when n_features *
 * pyramid_levels > 65535; SSX_ERR_INVALID_ARG when voc and db belong to different contexts or the winner was stored
 * without descriptors.  An empty vocabulary, no features or no surviving keypoint: an empty BowVector, nothing found, and
 * the keyframe can still be committed.  A call that fails otherwise leaves the stored keyframes as they were and nothing
 * pending. */
SSX_API ssx_status ssx_kfdb_process_keyframe(ssx_kf_database* db, ssx_vocabulary* voc, int64_t kf_id, const uint8_t* img,
                                             int32_t stride, int32_t rows, int32_t cols, const ssx_orb_params* prm,
                                             int32_t n_features, const ssx_keypoint* features, int32_t pyramid_levels,
                                             int32_t min_db_size, int32_t min_id_gap, float threshold, int32_t pairs_cap,
                                             int32_t* pairs_out, ssx_kfdb_step_result* res);
/* The same step for n databases of ONE context in one call (one keyframe of each of n streams): one launch chain and one
 * synchronisation for all jobs, and one more launch pair and a second synchronisation when at least one job found a loop;
 * neither number depends on n.  Every job has a database of its own; all of them and the vocabulary belong to one
 * context, the images share rows, cols and stride.  commit_pending != 0: ssx_kfdb_add_pending(db) first, inside the same
 * chain (growing that database's arena or table adds that growth's own synchronisation).  Per job, *res, pairs_out and the
 * keyframe left pending in job.db are bit for bit what ssx_kfdb_add_pending (when asked for) + ssx_kfdb_process_keyframe
 * leave, whatever n is and wherever the job stands in the table; afterwards the single-database entry points work on every
 * database as before.  images_on_device != 0: the images are read where they lie (device or pinned host memory).
 * Rejected before anything is touched, pending keyframes included: n < 0, a missing db / res / status_out / image, two jobs
 * with one database, a database of another context, differing strides, commit_pending with nothing pending or an id that
 * does not ascend (SSX_ERR_INVALID_ARG), n_features * pyramid_levels > 65535 (SSX_ERR_UNSUPPORTED).  n == 0: SSX_OK.
 * What depends on the data goes to the job's *status_out -- SSX_ERR_CAPACITY when pairs_cap is too small (the keyframe
 * still pending), SSX_ERR_INVALID_ARG when the winner was stored without descriptors (nothing pending) -- while the other
 * jobs complete; the call returns the first status that is not SSX_OK, so a return value that no job's status carries is a
 * failure of the whole call.  A HIP error (SSX_ERR_HIP) leaves the stored keyframes of every database as they were and, unless
 * it struck while an arena or table was grown before the call began on the databases, nothing pending. */
typedef struct ssx_kfdb_step_job {
  ssx_kf_database* db;
  int64_t kf_id;
  const uint8_t* img; int32_t stride;
  int32_t n_features; const ssx_keypoint* features;
  int32_t commit_pending;
  int32_t pairs_cap; int32_t* pairs_out;
  ssx_kfdb_step_result* res;
  int32_t* status_out;            /* this job's ssx_status */
} ssx_kfdb_step_job;
SSX_API ssx_status ssx_kfdb_process_keyframe_batch(ssx_vocabulary* voc, int32_t n, const ssx_kfdb_step_job* jobs, int32_t rows,
                                                   int32_t cols, const ssx_orb_params* prm, int32_t pyramid_levels,
                                                   int32_t min_db_size, int32_t min_id_gap, float threshold,
                                                   int32_t images_on_device);
/* AddToKeyframeDatabase (:646-649) for the keyframe of the last successful ssx_kfdb_process_keyframe: stored exactly as
 * ssx_kfdb_add(kf_id, its BowVector, its descriptors, its class ids) would store it, device to device.  The same
 * id-must-ascend rule; SSX_ERR_INVALID_ARG when nothing is pending (a keyframe is committed once).  ssx_kfdb_add and
 * the growth of the database between the two calls leave the pending keyframe intact. */
SSX_API ssx_status ssx_kfdb_add_pending(ssx_kf_database* db);
/* Download the pending keyframe (ORBDescriptors_, pyramid_key_points_, bow2_vec_ of :622-633).  Every output is nullable;
 * kps_out / desc_out / class_id_out hold kps_cap entries, ids_out / vals_out bow_cap (SSX_ERR_CAPACITY when smaller than
 * the counts, which are written first).  SSX_ERR_INVALID_ARG when nothing is pending. */
SSX_API ssx_status ssx_kfdb_pending(ssx_kf_database* db, int64_t* kf_id, int32_t kps_cap, ssx_keypoint* kps_out,
                                    uint8_t* desc_out, int32_t* class_id_out, int32_t* n_pyramid, int32_t bow_cap,
                                    int32_t* ids_out, double* vals_out, int32_t* n_bow);

/* The candidate query of relocalisation (the reference has a TODO there, src/ssvio/frontend.cpp:62-66): which stored
 * keyframes a frame that lost tracking resembles, and its feature matches against each of them, in ONE call with ONE
 * synchronisation (two more the first time an image shape is planned); neither the launches nor the synchronisations
 * depend on max_candidates or on the number of stored keyframes.  The frame is described and its BowVector assembled as
 * ssx_kfdb_process_keyframe does it; EVERY stored keyframe is scored (no id gap, no minimum size).  With f[row] the
 * score narrowed to float and f_best the largest, the candidates are the rows with f > 0, f >= threshold and
 * f >= ratio * f_best (a float product), ordered by f descending and then by row ascending (the lower id first), cut to
 * max_candidates (tools/reloc_model.py): cand[0] is the winner of ssx_kfdb_detect_loop(INT64_MAX, that BowVector,
 * min_id_gap 0, threshold).  Per candidate, n_pairs, min_distance and its slice pairs_out[c * pairs_cap * 2 ...] are bit
 * for bit what ssx_kfdb_match_features(cand.kf_id, the frame's descriptors and class ids) returns; a candidate stored
 * without descriptors has no_descriptors = 1, no pairs and min_distance -1 and is no error.  SSX_ERR_CAPACITY when some
 * candidate has more than pairs_cap pairs: every count is true and the first pairs_cap pairs of each are written.
 * The database is only read: the stored keyframes and the pending keyframe are as before the call.
 * SSX_ERR_INVALID_ARG, before anything is touched: a null required pointer, max_candidates outside
 * [1, SSX_RELOC_MAX_CANDIDATES], ratio not finite or outside [0, 1], threshold negative or NaN, a vocabulary of another
 * context; SSX_ERR_UNSUPPORTED: n_features * pyramid_levels > 65535.  An empty database, no features, no surviving
 * keypoint or an empty vocabulary: n_candidates = 0 and SSX_OK. */
#define SSX_RELOC_MAX_CANDIDATES 8
typedef struct ssx_reloc_candidate {
  int64_t kf_id;
  float   score;            /* f */
  int32_t row;              /* its index among the stored keyframes, in id order */
  int32_t no_descriptors;
  int32_t n_pairs;
  int32_t min_distance;
} ssx_reloc_candidate;
typedef struct ssx_reloc_query_result {
  int32_t n_pyramid, n_bow; /* as ssx_kfdb_step_result */
  int32_t n_scored;         /* stored keyframes */
  int32_t n_candidates;
  ssx_reloc_candidate cand[SSX_RELOC_MAX_CANDIDATES];   /* behind n_candidates: kf_id -1, row -1, min_distance -1 */
} ssx_reloc_query_result;
SSX_API ssx_status ssx_kfdb_relocalize_query(ssx_kf_database* db, ssx_vocabulary* voc, const uint8_t* img, int32_t stride,
                                             int32_t rows, int32_t cols, const ssx_orb_params* prm, int32_t n_features,
                                             const ssx_keypoint* features, int32_t pyramid_levels, int32_t max_candidates,
                                             float threshold, float ratio, int32_t pairs_cap,
                                             int32_t* pairs_out /* max_candidates x pairs_cap x 2 */,
                                             ssx_reloc_query_result* res);
/* The same query for one frame of each of n databases of ONE context in one call (the streams of a cohort that lost
 * tracking together): one launch chain and ONE synchronisation for all jobs; neither number depends on n, on
 * max_candidates or on the number of stored keyframes (growing a database's arena or table for a commit adds that
 * growth's own synchronisation, planning a new image shape its own).  Every job has a database of its own; all of them
 * and the vocabulary belong to one context, the images share rows, cols and stride.  commit_pending != 0:
 * ssx_kfdb_add_pending(db) first, inside the same chain -- the keyframe is scored and matched like any stored one
 * (n_scored counts it, it can be cand[0]) and nothing is pending afterwards; a job without it only reads its database,
 * the pending keyframe included.  Per job, *res and pairs_out (max_candidates x pairs_cap x 2) are bit for bit what
 * ssx_kfdb_add_pending (when asked for) + ssx_kfdb_relocalize_query return, whatever n is and wherever the job stands in
 * the table, and the stored contents of every database equal what those calls leave.  images_on_device as
 * ssx_kfdb_process_keyframe_batch.  Rejected before anything is touched, pending keyframes included: n < 0, a missing
 * db / res / status_out / image, two jobs with one database, a database of another context, differing strides,
 * commit_pending with nothing pending or an id that does not ascend, and the argument checks of the single query
 * (SSX_ERR_INVALID_ARG); n_features * pyramid_levels > 65535 or n * max_candidates > 65535 (SSX_ERR_UNSUPPORTED).
 * n == 0: SSX_OK.  What depends on the data goes to the job's *status_out -- SSX_ERR_CAPACITY when some candidate has
 * more than pairs_cap pairs, every count true and the first pairs_cap pairs of each written -- while the other jobs
 * complete; the call returns the first status that is not SSX_OK, by the rule of ssx_kfdb_process_keyframe_batch.  A HIP
 * error (SSX_ERR_HIP) leaves the stored keyframes and the pending keyframe of every database as they were.  An empty
 * database, a job without features, no surviving keypoint or an empty vocabulary: n_candidates = 0 for that job. */
typedef struct ssx_reloc_query_job {
  ssx_kf_database* db;
  const uint8_t* img; int32_t stride;
  int32_t n_features; const ssx_keypoint* features;
  int32_t commit_pending;                 /* != 0: ssx_kfdb_add_pending(db) first, inside the same chain */
  int32_t pairs_cap; int32_t* pairs_out;  /* max_candidates x pairs_cap x 2 */
  ssx_reloc_query_result* res;
  int32_t* status_out;                    /* this job's ssx_status */
} ssx_reloc_query_job;
SSX_API ssx_status ssx_kfdb_relocalize_query_batch(ssx_vocabulary* voc, int32_t n, const ssx_reloc_query_job* jobs, int32_t rows,
                                                   int32_t cols, const ssx_orb_params* prm, int32_t pyramid_levels,
                                                   int32_t max_candidates, float threshold, float ratio,
                                                   int32_t images_on_device);

/* The guided search of relocalisation, the second step behind an accepted candidate (tools/guided_model.py states the
 * rule operation by operation): P map points are projected into the frame with the pose just found, K4 = (fx, fy, cx,
 * cy) and T_cw12 = [R|t] row-major, in f64 with every operation rounded on its own; a point behind the camera or with a
 * non-finite camera position is SSX_GUIDED_BEHIND, one that does not fall in [0, cols) x [0, rows) SSX_GUIDED_OUTSIDE.
 * A point's descriptors are ALL stored descriptors of keyframe point_kf[p] whose class id is point_cls[p]
 * (SSX_GUIDED_NO_DESCRIPTOR, and no error, for an id that is not stored, a keyframe stored without descriptors or none
 * of that class).  Feature i of the F frame features is a candidate iff taken[i] == 0 (taken null: none is taken),
 * |x_i - u| <= radius and |y_i - v| <= radius (edges inclusive) and it has a frame descriptor (SSX_GUIDED_NO_FEATURE
 * when there is none); its distance is the least Hamming distance over the point's and its own descriptors.  The best
 * candidate has the lowest distance d1, then the lowest index; d2 is the lowest distance of any OTHER candidate.  The
 * point is accepted iff d1 <= max_distance (else SSX_GUIDED_DISTANCE) and there is no second or 100 d1 < ratio_pct d2
 * in integers (else SSX_GUIDED_RATIO).  A feature goes to one point: of the accepted points that claim it the lowest
 * d1 wins, then the lowest point; the others are SSX_GUIDED_CLAIMED.  Per point: feat_out (-1 unless MATCHED), d1_out,
 * d2_out (-1 where there is none), status_out, uv_out (nullable; zeros for BEHIND); *n_matched counts the MATCHED.
 * The result is a pure function of the arguments and the stored keyframes: two calls give the same bytes.
 * ssx_kfdb_project_match is the stage on a caller's arrays (as ssx_kfdb_match_features is for MatchFeatures): n_cur
 * frame descriptors with the feature each belongs to, cur_cls[j] in [0, F).
 * SSX_ERR_INVALID_ARG, before anything is touched (the outputs included): a null required pointer; P, F or n_cur < 0;
 * a cur_cls outside [0, F); rows or cols < 1; radius negative or not finite; max_distance outside [0, 256]; ratio_pct
 * outside [0, 100]; a non-finite K4 or T_cw12.  SSX_ERR_UNSUPPORTED: P > 65535.  P == 0, F == 0 or n_cur == 0:
 * SSX_OK, every point that projects into the image is SSX_GUIDED_NO_FEATURE (or SSX_GUIDED_NO_DESCRIPTOR), *n_matched
 * = 0.  The database is only read. */
typedef enum ssx_guided_status {
  SSX_GUIDED_MATCHED = 0,
  SSX_GUIDED_BEHIND,
  SSX_GUIDED_OUTSIDE,
  SSX_GUIDED_NO_DESCRIPTOR,
  SSX_GUIDED_NO_FEATURE,
  SSX_GUIDED_DISTANCE,
  SSX_GUIDED_RATIO,
  SSX_GUIDED_CLAIMED
} ssx_guided_status;
SSX_API ssx_status ssx_kfdb_project_match(ssx_kf_database* db, const double* K4, const double* T_cw12, int32_t rows,
                                          int32_t cols, int32_t F, const float* feat_xy /* F x 2 */,
                                          const uint8_t* taken /* nullable */, int32_t n_cur, const uint8_t* cur_desc,
                                          const int32_t* cur_cls, int32_t P, const int64_t* point_kf,
                                          const int32_t* point_cls, const double* xyz, double radius,
                                          int32_t max_distance, int32_t ratio_pct, int32_t* feat_out, int32_t* d1_out,
                                          int32_t* d2_out, int32_t* status_out, double* uv_out /* nullable, P x 2 */,
                                          int32_t* n_matched);
/* The call the system uses: the frame is described exactly as ssx_kfdb_relocalize_query describes it (on purpose a
 * second time: a describe on a rare path is cheaper than a "last query" slot every other call on the database would
 * have to invalidate), and the search reads the described arrays where they lie.  F = n_features, a feature's position
 * is features[i].x, .y; taken (nullable) has n_features entries.  The outputs are, bit for bit, what
 * ssx_kfdb_project_match returns on the frame's descriptors and class ids.  One upload behind the describe's, one result
 * copy and ONE synchronisation (two more the first time an image shape is planned); neither the launches nor the
 * synchronisations depend on P, n_features or the number of stored keyframes.  The stored keyframes and the pending
 * keyframe are as before the call.  Refused as ssx_kfdb_project_match, and as the query refuses its frame arguments;
 * SSX_ERR_UNSUPPORTED also for n_features * pyramid_levels > 65535. */
SSX_API ssx_status ssx_kfdb_guided_search(ssx_kf_database* db, const uint8_t* img, int32_t stride, int32_t rows,
                                          int32_t cols, const ssx_orb_params* prm, int32_t n_features,
                                          const ssx_keypoint* features, int32_t pyramid_levels,
                                          const uint8_t* taken /* nullable */, const double* K4, const double* T_cw12,
                                          int32_t P, const int64_t* point_kf, const int32_t* point_cls,
                                          const double* xyz, double radius, int32_t max_distance, int32_t ratio_pct,
                                          int32_t* feat_out, int32_t* d1_out, int32_t* d2_out, int32_t* status_out,
                                          double* uv_out /* nullable, P x 2 */, int32_t* n_matched);

/* ------------------------------------------------------------------------------------------------
 * The pose correction of loop closing -- replaces LoopClosing::ComputeCorrectPose (src/ssvio/loopclosing.cpp:147-243)
 * with its cv::solvePnPRansac call (:205-206) and LoopClosing::OptimizeCurrentPose (:245-351).
 *
 * cv::solvePnPRansac is not restated to the bit: its sampler and its confidence-driven early exit belong to OpenCV's
 * sequential loop.  The contract of ssx_pnp_ransac is its own, stated in tools/pnp_model.py, which the kernel follows
 * operation by operation:
 *   - max_iters hypotheses (the reference passes 100), ALL scored in one launch (no early exit, hence no confidence);
 *   - hypothesis h draws three distinct points as a pure function of (seed, h, M); its P3P yields up to four poses;
 *   - a point is an inlier of a pose when its depth is positive and its reprojection error is at most reproj_px PIXELS
 *     (the reference passes 5.991, its chi-square constant, as this pixel threshold);
 *   - the winner has the most inliers, then the lowest hypothesis, then the lowest solution.
 * The reference uses only the pose of the RANSAC, never its inliers; OptimizeCurrentPose then runs g2o over ALL pairs:
 * one optimize(10) with every edge active, then the procedure of ssx_pose_only_opt (4 rounds x optimize(10), chi2 > chi2_th
 * => outlier after every round, the robust kernels dropped before the last).  ssx_loop_pose_opt is that, with the arithmetic
 * of ssx_pose_only_opt.
 * ------------------------------------------------------------------------------------------------ */
#define SSX_PNP_MAX_ITERS 4096
/* xyz M x 3, uv M x 2 (cv::Point2f widened to double), pose_out = qx qy qz qw tx ty tz (normalised, qw >= 0) of the winner,
 * inlier_out (nullable) M bytes, *best_hypothesis (nullable) = 4 h + s of the winner: hypothesis h, its solution s.
 * *found = 0 when no hypothesis reaches 4 inliers (a hypothesis explains its own 3 points) or M < 3 -- the exception the
 * reference catches (:203-210); pose_out is then the identity and *n_inliers = 0.
 * SSX_ERR_INVALID_ARG: M < 0, a null required pointer, max_iters outside [1, SSX_PNP_MAX_ITERS], reproj_px negative or NaN,
 * a non-finite K4. */
SSX_API ssx_status ssx_pnp_ransac(ssx_ctx* ctx, const double* K4, int32_t M, const double* xyz, const double* uv,
                                  int32_t max_iters, double reproj_px, uint32_t seed, double* pose_out, uint8_t* inlier_out,
                                  int32_t* n_inliers, int32_t* best_hypothesis, int32_t* found);
/* OptimizeCurrentPose: pose_io = corrected_current_pose_ in and out, inlier_out[i] (nullable) = 1 when pair i survives,
 * *n_inliers (nullable) = their number.  Reference: chi2_th 5.991, huber_delta 1.0. */
SSX_API ssx_status ssx_loop_pose_opt(ssx_ctx* ctx, double* pose_io, const double* K4, int32_t M, const double* xyz,
                                     const double* uv, double chi2_th, double huber_delta, uint8_t* inlier_out,
                                     int32_t* n_inliers);
/* n poses in ONE call (relocalisation: one per candidate keyframe): per job, bit for bit, ssx_pnp_ransac(K4, M, xyz, uv,
 * max_iters, reproj_px, seed) and, where that found a pose, ssx_loop_pose_opt(chi2_th, huber_delta) started from it --
 * pose_out, inlier_out and n_inliers are then the refinement's -- whatever n is and wherever the job stands in the table.
 * A job with M < 3 or nothing found: found = 0, the identity, n_inliers = 0, inlier_out zeroed.  One upload, one download,
 * one synchronisation; one launch of the RANSAC and at most one of the refinement per kernel class, independent of n.
 * n in [0, SSX_PNP_BATCH_MAX] (0: SSX_OK); otherwise SSX_ERR_INVALID_ARG as ssx_pnp_ransac, before anything is written. */
#define SSX_PNP_BATCH_MAX 64
typedef struct ssx_pnp_pose_job {
  int32_t M; const double* xyz; const double* uv; uint32_t seed;             /* in */
  double pose_out[7]; uint8_t* inlier_out /* nullable, M */;                 /* out */
  int32_t found, n_ransac_inliers, best_hypothesis, n_inliers;
} ssx_pnp_pose_job;
SSX_API ssx_status ssx_pnp_pose_batch(ssx_ctx* ctx, const double* K4, int32_t n, ssx_pnp_pose_job* jobs, int32_t max_iters,
                                      double reproj_px, double chi2_th, double huber_delta);

typedef enum ssx_loop_verdict {
  SSX_LOOP_OK = 0,               /* ComputeCorrectPose returns true */
  SSX_LOOP_FEW_MAP_POINTS = 1,   /* fewer than 10 pairs with a live map point (:193) */
  SSX_LOOP_NO_POSE = 2,          /* the RANSAC found nothing (:203-210) */
  SSX_LOOP_FEW_INLIERS = 3       /* fewer than 10 pairs survive the optimisation (:219) */
} ssx_loop_verdict;
typedef struct ssx_loop_pose_result {
  int32_t verdict;               /* ssx_loop_verdict */
  int32_t n_with_point;          /* pairs whose map point is alive */
  int32_t n_ransac_inliers;      /* inliers of the RANSAC's winner; best_hypothesis = its 4 h + s (-1: none) */
  int32_t best_hypothesis;
  int32_t n_inliers;             /* cnt_inliner: pairs that survive OptimizeCurrentPose */
  int32_t need_correct;          /* need_correct_loop_pose_ = error > 1 && error < 15 */
  double error;                  /* |log(T_cur * corrected_pose^-1)| */
  double corrected_pose[7];      /* corrected_current_pose_: written for SSX_LOOP_OK and SSX_LOOP_FEW_INLIERS (the
                                  * optimisation ran), the identity for the other two verdicts */
  double relative_to_loop[7];    /* relative_pose_to_loop_KF_ = corrected_pose * T_loop^-1 */
} ssx_loop_pose_result;
/* The whole of ComputeCorrectPose for the n_pairs pairs of ssx_kfdb_match_features: two launches (the RANSAC, the
 * optimisation, which takes the RANSAC's pose where it lies in device memory) and one synchronisation.
 *   loop_xyz n_pairs x 3   the map point of the loop keyframe's feature of each pair (ignored where has_point[i] == 0)
 *   has_point n_pairs      0 = the feature's map_point_ has expired: the pair is erased (:170-173)
 *   cur_uv n_pairs x 2     the current keyframe's pixel of each pair
 *   T_cur, T_loop          the poses of the current and of the loop keyframe
 *   kept n_pairs           set_valid_feature_matches_ afterwards: 1 = the pair is still in it
 * RANSAC threshold 5.991 px, chi2_th 5.991 and Huber delta 1.0 are the reference's.  error, need_correct and
 * relative_to_loop are written for SSX_LOOP_OK only (the reference returns before it computes them otherwise).
 * SSX_ERR_INVALID_ARG as for ssx_pnp_ransac. */
SSX_API ssx_status ssx_loop_compute_pose(ssx_ctx* ctx, int32_t n_pairs, const double* loop_xyz, const uint8_t* has_point,
                                         const double* cur_uv, const double* T_cur, const double* T_loop, const double* K4,
                                         int32_t max_iters, uint32_t seed, uint8_t* kept, ssx_loop_pose_result* out);

/* ------------------------------------------------------------------------------------------------
 * The geometry of LoopClosing::LoopCorrect (reference: src/ssvio/loopclosing.cpp:353-594) as one call: what the thread does
 * with need_correct, corrected_pose and relative_to_loop of ssx_loop_compute_pose.  One upload, three short kernel passes around
 * the optimiser of ssx_pose_graph_opt, one download.  Keyframes and map points are flat arrays; the caller gathers indices for
 * the reference's pointers.  The pointer-level map fusion of :427-453 moves no number and stays with the caller.
 *
 * Stage 1, CorrectActivateKeyframeAndMappoint (:378-425):
 *   an active keyframe a != cur_kf gets T'_a = (T_a * T_cur^-1) * corrected_pose, grouped as :394-397 group it; T'_cur =
 *   corrected_pose (:384-385); keyframes that are not active keep their bits (:387 visits the active ones only).
 *   An active point whose anchor is an active keyframe a gets p' = T'_a^-1 * (T_a * p) (:417-419).  An active point whose anchor
 *   is -1 or not active is left alone (:413-415).
 * Stage 2, PoseGraphOptimization (:458-533): exactly ssx_pose_graph_opt(iterations) on the poses stage 1 left, with
 *   pose_fixed[i] = kf_active[i] | (i == loop_kf) | (i == initial_kf) (:482-486).  When nothing can be optimised -- no free
 *   keyframe, no edge, iterations <= 0 -- stages 1 and 3 still run, pg.n_iters = 0, and edge_err_out and the statistics are
 *   not written.
 * Stage 3 (:537-591): every point with point_active == 0 and anchor a >= 0 gets p' = T_opt_a^-1 * (T_stage1_a * p) (:562-565);
 *   T_stage1_a is the pose after stage 1 (getPose() at :562), T_opt_a the vertex estimate (:564).  The two-step product is applied
 *   where the vertex was fixed as well, so such points move by rounding, as the reference's do.  A point with anchor -1 is left
 *   alone (:556-561).
 * Poses returned: every keyframe gets the optimiser's estimate (:588) except keep_kf, the front-end's reference keyframe, which
 *   gets its stage-1 pose (:572-587) while its points were re-anchored with the estimate.
 * Every product, inverse and action is Sophus' (SE3 operator*, inverse(), operator* on a point: the quaternion re-normalised after
 * a product and an inverse); T'^-1 is computed once per keyframe, not once per point -- the same function, the same bits.
 *
 * SSX_ERR_INVALID_ARG: a null array that is needed (points, point_anchor, point_active may be null when n_points == 0, the edge
 *   arrays when n_edges == 0), n_keyframes < 1, cur_kf or loop_kf outside [0, n_keyframes), initial_kf or keep_kf outside
 *   [-1, n_keyframes), an edge index or a point_anchor out of range, and kf_active[cur_kf] == 0: the reference sets poses for
 *   active keyframes only (:422-425), and a current keyframe outside the window is not a case ssvio produces.
 * SSX_ERR_UNSUPPORTED: more than 2048 free keyframes, as for ssx_pose_graph_opt.
 * On any failure poses, points and the optional outputs are untouched: they are written after the final synchronisation only.
 * Inputs must be finite.
 * ------------------------------------------------------------------------------------------------ */
typedef struct ssx_loop_correct_problem {
  int32_t n_keyframes, n_edges, n_points;
  int32_t cur_kf, loop_kf;        /* indices into poses: current_keyframe_, loop_keyframe_ */
  int32_t initial_kf;             /* keyframe id 0 (:483), -1 = none */
  int32_t keep_kf;                /* the front-end's reference keyframe (:568-572), -1 = none */
  double* poses;                  /* n_keyframes x 7 (qx qy qz qw tx ty tz, T_cw), in/out */
  const uint8_t* kf_active;       /* n_keyframes: in Map::GetActiveKeyFrames() */
  const double* corrected_pose;   /* 7: corrected_current_pose_ */
  const int32_t* edge_i; const int32_t* edge_j; const double* edge_meas;   /* as ssx_pose_graph_problem (:492-529) */
  double* points;                 /* n_points x 3, in/out */
  const int32_t* point_anchor;    /* n_points: keyframe index the point is re-anchored to, -1 = leave the point alone.
                                     Active point: GetActiveObservations().front() (:408); other: GetObservations().front() (:554) */
  const uint8_t* point_active;    /* n_points: in Map::GetActiveMapPoints() (:402, :543-547) */
  double* stage1_poses_out;       /* optional n_keyframes x 7: the poses after CorrectActivateKeyframeAndMappoint (:422-425) */
  double* edge_err_out; int32_t stats_cap; double* stats_chi2; double* stats_lambda; int32_t* stats_trials;  /* as the pose graph's */
} ssx_loop_correct_problem;
typedef struct ssx_loop_correct_result {
  ssx_pose_graph_result pg;       /* stage 2 */
  int32_t n_active_kf;            /* keyframes moved by stage 1 */
  int32_t n_active_points_moved;  /* stage 1 (:417-419) */
  int32_t n_other_points_moved;   /* stage 3 (:562-565) */
  int32_t n_points_skipped;       /* left alone by both stages (:413-415, :556-561): n_points minus the two above */
} ssx_loop_correct_result;
SSX_API ssx_status ssx_loop_correct(ssx_ctx* ctx, const ssx_loop_correct_problem* prob, int32_t iterations,
                                    ssx_loop_correct_result* res);

#ifdef __cplusplus
}
#endif
#endif /* SSX_H */
