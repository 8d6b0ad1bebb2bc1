// ssvio_amd/csrc/loop_correct.inc -- the geometry of LoopClosing::LoopCorrect as one call, included behind pg.inc at the end of ba.hip.
//
// Replaces what the reference's src/ssvio/loopclosing.cpp:353-594 computes (DESIGN.md section 6g):
//   stage 1  CorrectActivateKeyframeAndMappoint (:378-425): the active keyframes move rigidly with the corrected current keyframe,
//            every active map point is re-anchored to its first active observer
//   stage 2  PoseGraphOptimization (:458-533): the optimiser of pg.inc on the stage-1 poses (pg_plan .. pg_lm_loop, shared)
//   stage 3  :537-591: every non-active map point is re-anchored to its first observer (old pose = after stage 1, new pose = the
//            vertex estimate), the front-end's reference keyframe keeps its pose
//   k_lc_correct_keyframes   one thread per keyframe: the stage-1 pose and its inverse
//   k_lc_invert_keyframes    one thread per keyframe: the inverse of the optimised pose; the reference keyframe's pose restored
//   k_reanchor_points        one thread per point: p' = inv(T_new) * (T_old * p), both stages
// All SE3 arithmetic is se3.hpp's (se3_mul, se3_inverse, se3_act: Sophus' re-normalising forms).  No atomics, no LDS: the point kernel
// moves 52 bytes per point and gathers two poses that stay in L2.
namespace {

// old_pose [P][7] -> s1_pose, inv_pose [P][7].  The input is only read (every thread needs T_cur), so no thread races the one that
// replaces the current keyframe's pose; the caller copies s1_pose over the optimiser's state afterwards.
__global__ __launch_bounds__(256) void k_lc_correct_keyframes(int P, int cur_kf, const double* __restrict__ old_pose, const uint8_t* __restrict__ kf_active,
                                                              const double* __restrict__ corrected, double* __restrict__ s1_pose, double* __restrict__ inv_pose)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  double T[7], Tn[7], Ti[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = old_pose[7 * (size_t)i + k];
  if (!kf_active[i]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) Tn[k] = T[k];                 // untouched (:387: only the active keyframes are visited)
  } else if (i == cur_kf) {
#pragma unroll
    for (int k = 0; k < 7; ++k) Tn[k] = corrected[k];         // :384-385
  } else {
    double Tc[7], C[7], Tci[7], rel[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { Tc[k] = old_pose[7 * (size_t)cur_kf + k]; C[k] = corrected[k]; }
    ssx::se3_inverse(Tc, Tci);
    ssx::se3_mul(T, Tci, rel);                                // T_kn_k = T_a * T_cur^-1       (:394)
    ssx::se3_mul(rel, C, Tn);                                 // T_kn_true = T_kn_k * corrected (:397)
  }
  ssx::se3_inverse(Tn, Ti);                                   // correct_pose.inverse() (:419), once per keyframe
#pragma unroll
  for (int k = 0; k < 7; ++k) { s1_pose[7 * (size_t)i + k] = Tn[k]; inv_pose[7 * (size_t)i + k] = Ti[k]; }
}

// inv_pose = inverse of the vertex estimates (:564-565); afterwards keep_kf (>= 0) gets its stage-1 pose back (:572-587) -- its points
// are still re-anchored with the estimate's inverse written here
__global__ __launch_bounds__(256) void k_lc_invert_keyframes(int P, int keep_kf, double* __restrict__ pose, const double* __restrict__ s1_pose,
                                                             double* __restrict__ inv_pose)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  double T[7], Ti[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = pose[7 * (size_t)i + k];
  ssx::se3_inverse(T, Ti);
#pragma unroll
  for (int k = 0; k < 7; ++k) inv_pose[7 * (size_t)i + k] = Ti[k];
  if (i == keep_kf) {
#pragma unroll
    for (int k = 0; k < 7; ++k) pose[7 * (size_t)i + k] = s1_pose[7 * (size_t)i + k];
  }
}

// p' = inv_new[a] * (old[a] * p) for the points with point_active == want_active, anchor a >= 0 and (kf_mask == nullptr or kf_mask[a]);
// every other point keeps its bits
__global__ __launch_bounds__(256) void k_reanchor_points(int N, const double* __restrict__ old_pose, const double* __restrict__ inv_new_pose,
                                                         const uint8_t* __restrict__ kf_mask, const int* __restrict__ anchor,
                                                         const uint8_t* __restrict__ point_active, int want_active, double* __restrict__ pts)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if ((point_active[i] != 0) != (want_active != 0)) return;
  const int a = anchor[i];
  if (a < 0) return;
  if (kf_mask && !kf_mask[a]) return;
  double To[7], Tn[7], p[3], pc[3], q[3];
#pragma unroll
  for (int k = 0; k < 7; ++k) { To[k] = old_pose[7 * (size_t)a + k]; Tn[k] = inv_new_pose[7 * (size_t)a + k]; }
  p[0] = pts[3 * (size_t)i]; p[1] = pts[3 * (size_t)i + 1]; p[2] = pts[3 * (size_t)i + 2];
  ssx::se3_act(To, p, pc);                                    // pos_cam = T_cw * P_w (:417, :562)
  ssx::se3_act(Tn, pc, q);                                    // T'^-1 * pos_cam      (:419, :565)
  pts[3 * (size_t)i] = q[0]; pts[3 * (size_t)i + 1] = q[1]; pts[3 * (size_t)i + 2] = q[2];
}

}  // namespace

extern "C" {

ssx_status ssx_loop_correct(ssx_ctx* ctx, const ssx_loop_correct_problem* prob, int32_t iterations, ssx_loop_correct_result* res)
{
  if (!ctx || !prob || !res || prob->n_keyframes < 1 || prob->n_edges < 0 || prob->n_points < 0 || !prob->poses || !prob->kf_active ||
      !prob->corrected_pose || (prob->n_edges > 0 && (!prob->edge_i || !prob->edge_j || !prob->edge_meas)) ||
      (prob->n_points > 0 && (!prob->points || !prob->point_anchor || !prob->point_active)))
    return SSX_ERR_INVALID_ARG;
  const int P = prob->n_keyframes, E = prob->n_edges, N = prob->n_points;
  auto kf_ok = [&](int k, int lo) { return k >= lo && k < P; };
  if (!kf_ok(prob->cur_kf, 0) || !kf_ok(prob->loop_kf, 0) || !kf_ok(prob->initial_kf, -1) || !kf_ok(prob->keep_kf, -1)) {
    ctx->set_error("ssx_loop_correct: cur_kf %d, loop_kf %d, initial_kf %d or keep_kf %d outside [0, %d) (the last two: or -1)", prob->cur_kf,
                   prob->loop_kf, prob->initial_kf, prob->keep_kf, P);
    return SSX_ERR_INVALID_ARG;
  }
  if (!prob->kf_active[prob->cur_kf]) {
    ctx->set_error("ssx_loop_correct: the current keyframe %d is not active", prob->cur_kf);
    return SSX_ERR_INVALID_ARG;
  }
  for (int k = 0; k < E; ++k)
    if (prob->edge_i[k] < 0 || prob->edge_i[k] >= P || prob->edge_j[k] < 0 || prob->edge_j[k] >= P) {
      ctx->set_error("ssx_loop_correct: edge %d references a keyframe outside [0, %d)", k, P);
      return SSX_ERR_INVALID_ARG;
    }
  int n_active_kf = 0, n_act_moved = 0, n_oth_moved = 0;
  for (int i = 0; i < P; ++i) n_active_kf += prob->kf_active[i] != 0;
  for (int i = 0; i < N; ++i) {
    const int a = prob->point_anchor[i];
    if (a < -1 || a >= P) {
      ctx->set_error("ssx_loop_correct: point %d is anchored to keyframe %d outside [-1, %d)", i, a, P);
      return SSX_ERR_INVALID_ARG;
    }
    if (a < 0) continue;
    if (prob->point_active[i]) n_act_moved += prob->kf_active[a] != 0;
    else n_oth_moved++;
  }
  // stage 2's fixed set: the active, the loop and the initial keyframes (:482-486)
  std::vector<uint8_t> fixed(P);
  int nP = 0;
  for (int i = 0; i < P; ++i) {
    fixed[i] = prob->kf_active[i] != 0 || i == prob->loop_kf || i == prob->initial_kf;
    nP += !fixed[i];
  }
  if (nP > 2048) { ctx->set_error("ssx_loop_correct: %d free keyframes exceed the supported 2048", nP); return SSX_ERR_UNSUPPORTED; }
  const bool optimise = nP > 0 && E > 0 && iterations > 0;     // otherwise stages 1 and 3 alone (g2o: optimize() returns at once)
  BaWorkspace* ws = ba_workspace(ctx);
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // ---- one staging blob: the pose graph's inputs (when it runs), then this call's ----
  PgPlan pl;
  if (optimise) pg_plan(pl, P, E, fixed.data(), prob->edge_i, prob->edge_j);
  else pl.o_pose0 = pl.in.take(sizeof(double) * 7 * P);
  const size_t o_kfa = pl.in.take((size_t)P), o_corr = pl.in.take(sizeof(double) * 7);
  const size_t o_pts = pl.in.take(sizeof(double) * 3 * (size_t)N), o_anc = pl.in.take(sizeof(int) * (size_t)N), o_pact = pl.in.take((size_t)N);
  if (optimise) pg_layout(pl);
  else { pl.in_bytes = pl.in.off; pl.all = pl.in; }
  const size_t o_s1 = pl.all.take(sizeof(double) * 7 * P), o_inv = pl.all.take(sizeof(double) * 7 * P);
  // downloads: poses | points | stage-1 poses | edge errors
  const bool want_err = optimise && prob->edge_err_out;
  Layout dl;
  const size_t h_pose = dl.take(sizeof(double) * 7 * P), h_pts = dl.take(sizeof(double) * 3 * (size_t)N);
  const size_t h_s1 = dl.take(prob->stage1_poses_out ? sizeof(double) * 7 * P : 0), h_err = dl.take(want_err ? sizeof(double) * 6 * (size_t)E : 0);
  SSX_HIP_TRY(ctx, ws->arena.reserve(pl.all.off));
  SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(pl.in_bytes, dl.off)));
  SSX_HIP_TRY(ctx, ws->scal.reserve(sizeof(double) * SC_N));
  char* hs = ws->stage.as<char>();
  if (optimise) pg_stage(pl, hs, prob->poses, prob->edge_i, prob->edge_j, prob->edge_meas);
  else memcpy(hs + pl.o_pose0, prob->poses, sizeof(double) * 7 * P);
  memcpy(hs + o_kfa, prob->kf_active, (size_t)P);
  memcpy(hs + o_corr, prob->corrected_pose, sizeof(double) * 7);
  if (N > 0) {
    memcpy(hs + o_pts, prob->points, sizeof(double) * 3 * (size_t)N);
    memcpy(hs + o_anc, prob->point_anchor, sizeof(int) * (size_t)N);
    memcpy(hs + o_pact, prob->point_active, (size_t)N);
  }
  char* base = ws->arena.as<char>();
  hipStream_t s = ctx->stream;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, pl.in_bytes, hipMemcpyHostToDevice, s));
  PgRun run;
  if (optimise) pg_wire(pl, base, run);
  double* pose0 = (double*)(base + pl.o_pose0);
  double* s1 = (double*)(base + o_s1); double* inv = (double*)(base + o_inv);
  const uint8_t* kfa = (const uint8_t*)(base + o_kfa);
  double* pts = (double*)(base + o_pts);
  const int* anc = (const int*)(base + o_anc);
  const uint8_t* pact = (const uint8_t*)(base + o_pact);
  const int kgrid = (P + 255) / 256, pgrid = (N + 255) / 256;
  // ---- stage 1 (pose0 still holds the poses before the correction) ----
  SSX_PROF(ctx, KID_LC_KEYFRAMES, hipLaunchKernelGGL(k_lc_correct_keyframes, dim3(kgrid), dim3(256), 0, s, P, (int)prob->cur_kf, (const double*)pose0, kfa,
                                                     (const double*)(base + o_corr), s1, inv));
  if (N > 0) SSX_PROF(ctx, KID_LC_REANCHOR, hipLaunchKernelGGL(k_reanchor_points, dim3(pgrid), dim3(256), 0, s, N, (const double*)pose0, (const double*)inv, kfa, anc, pact, 1, pts));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(pose0, s1, sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, s));          // the optimiser's state
  // ---- stage 2 ----
  ssx_pose_graph_result pg{};
  std::vector<double> st_chi2, st_lambda;
  std::vector<int32_t> st_trials;
  double* pose_fin = pose0;
  if (optimise) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(run.d.pose[1], run.d.pose[0], sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, s));   // fixed keyframes
    const int cap = std::max(0, (int)prob->stats_cap);
    st_chi2.assign(cap, 0.0); st_lambda.assign(cap, 0.0); st_trials.assign(cap, 0);
    PgStats so;                                               // into vectors: the caller's arrays are written after the last synchronisation
    so.cap = cap; so.chi2 = st_chi2.data(); so.lambda = st_lambda.data(); so.trials = st_trials.data();
    int cur = 0;
    const ssx_status st = pg_lm_loop(ctx, ws, pl, run, iterations, so, &pg, &cur);
    if (st != SSX_OK) return st;
    pose_fin = run.d.pose[cur];
  }
  // ---- stage 3 ----
  SSX_PROF(ctx, KID_LC_KEYFRAMES, hipLaunchKernelGGL(k_lc_invert_keyframes, dim3(kgrid), dim3(256), 0, s, P, (int)prob->keep_kf, pose_fin, (const double*)s1, inv));
  if (N > 0) SSX_PROF(ctx, KID_LC_REANCHOR, hipLaunchKernelGGL(k_reanchor_points, dim3(pgrid), dim3(256), 0, s, N, (const double*)s1, (const double*)inv,
                                                               (const uint8_t*)nullptr, anc, pact, 0, pts));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_pose, pose_fin, sizeof(double) * 7 * P, hipMemcpyDeviceToHost, s));
  if (N > 0) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_pts, pts, sizeof(double) * 3 * (size_t)N, hipMemcpyDeviceToHost, s));
  if (prob->stage1_poses_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_s1, s1, sizeof(double) * 7 * P, hipMemcpyDeviceToHost, s));
  if (want_err) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_err, run.g.err, sizeof(double) * 6 * (size_t)E, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  memcpy(prob->poses, hs + h_pose, sizeof(double) * 7 * P);
  if (N > 0) memcpy(prob->points, hs + h_pts, sizeof(double) * 3 * (size_t)N);
  if (prob->stage1_poses_out) memcpy(prob->stage1_poses_out, hs + h_s1, sizeof(double) * 7 * P);
  if (want_err) memcpy(prob->edge_err_out, hs + h_err, sizeof(double) * 6 * (size_t)E);
  for (int k = 0; k < pg.stats_n; ++k) {
    if (prob->stats_chi2) prob->stats_chi2[k] = st_chi2[k];
    if (prob->stats_lambda) prob->stats_lambda[k] = st_lambda[k];
    if (prob->stats_trials) prob->stats_trials[k] = st_trials[k];
  }
  res->pg = pg;
  res->n_active_kf = n_active_kf; res->n_active_points_moved = n_act_moved; res->n_other_points_moved = n_oth_moved;
  res->n_points_skipped = N - n_act_moved - n_oth_moved;
  return SSX_OK;
}

}  // extern "C"
