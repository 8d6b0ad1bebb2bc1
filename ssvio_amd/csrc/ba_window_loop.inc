// ssvio_amd/csrc/ba_window_loop.inc -- ssx_ba_window_loop_correct: a loop correction applied to a resident window where it lies
// (included behind loop_correct.inc at the end of ba.hip; DESIGN.md section 6h).
//
// LoopClosing::CorrectActivateKeyframeAndMappoint (reference: src/ssvio/loopclosing.cpp:378-453) on what an ssx_ba_window holds.  Every
// keyframe of a window is active, so the window needs stage 1 of ssx_loop_correct only, and :427-453 -- the pointer-level fusion --
// is a removal for it: Map::RemoveMapPoint erases the current map point from activate_map_points_ (map.cpp:162-173), and the loop map
// point is not inserted there (it comes back with an ordinary push when a later keyframe observes it, map.cpp:41-49).
//   k_win_anchor_rank        one thread per stored observation: atomic minimum, per landmark slot, of the push-order rank of the
//                            observing keyframe (:408 GetActiveObservations().front(): the keyframe that was pushed earliest)
//   k_win_anchor_slot        one thread per landmark slot: minimum rank -> keyframe slot, -1 where nobody observes the slot
//   k_lc_correct_keyframes   loop_correct.inc, on the window's current pose buffer, into scratch (every thread reads T_cur)
//   k_reanchor_points        loop_correct.inc, in place on the window's current point buffer
// then device-to-device copies bring the poses into both pose buffers and the points into the other point buffer, and ONE download
// refreshes the host mirror.  A minimum does not depend on the order the atomics arrive in, so the anchors -- and with them every bit
// of the result -- are those of ssx_loop_correct on the exported window.
namespace {

// (lm_min starts as 0x7f7f7f7f -- what hipMemsetAsync(0x7f) leaves -- which is above every rank)
__global__ __launch_bounds__(256) void k_win_anchor_rank(int E, int P, int L, const int* __restrict__ e_pose, const int* __restrict__ e_point,
                                                         const int* __restrict__ kf_rank, int* __restrict__ lm_min)
{
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int l = e_point[e];                            // -1: a dead entry
  const int k = e_pose[e];
  if ((unsigned)l >= (unsigned)L || (unsigned)k >= (unsigned)P) return;
  const int r = kf_rank[k];                            // -1: a dead keyframe slot (its observations are dead entries already)
  if (r >= 0) atomicMin(&lm_min[l], r);
}

__global__ __launch_bounds__(256) void k_win_anchor_slot(int L, int n_live, const int* __restrict__ rank_slot, int* __restrict__ lm_anchor)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  const int r = lm_anchor[i];
  lm_anchor[i] = (unsigned)r < (unsigned)n_live ? rank_slot[r] : -1;
}

}  // namespace

extern "C" {

ssx_status ssx_ba_window_loop_correct(ssx_ba_window* w, int64_t cur_kf_id, const double* corrected_pose7, int32_t n_fused, const int64_t* fused_lm_ids,
                                      ssx_ba_window_loop_result* res)
{
  if (!w || !corrected_pose7 || n_fused < 0 || (n_fused > 0 && !fused_lm_ids)) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = w->ctx;
  // ---- everything that can be refused is refused here, before the first launch ----
  if (win_n_kf(w) == 0) { ctx->set_error("ssx_ba_window_loop_correct: the window is empty"); return SSX_ERR_INVALID_ARG; }
  const auto it = w->kf_slot.find(cur_kf_id);
  if (it == w->kf_slot.end()) { ctx->set_error("ssx_ba_window_loop_correct: keyframe %lld is not in the window", (long long)cur_kf_id); return SSX_ERR_INVALID_ARG; }
  const int cur_slot = it->second;
  {
    bool finite = true;
    for (int k = 0; k < 7; ++k) finite = finite && std::isfinite(corrected_pose7[k]);
    const double* q = corrected_pose7;
    if (!finite || !(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) {
      ctx->set_error("ssx_ba_window_loop_correct: the corrected pose is not finite or its quaternion is zero");
      return SSX_ERR_INVALID_ARG;
    }
  }
  // pending edits first: the device copies then hold exactly what the mirror holds
  ssx_status st = win_sync(w);
  if (st != SSX_OK) return st;
  const int P = (int)w->kf.size(), L = (int)w->lm_id.size(), E = (int)w->e_pose.size();
  // push order of the live keyframe slots: rank per slot (-1 dead), slot per rank, and the mask of the pose kernel
  std::vector<int> by_seq;
  for (int s = 0; s < P; ++s) if (w->kf[s].alive) by_seq.push_back(s);
  std::sort(by_seq.begin(), by_seq.end(), [&](int a, int b) { return w->kf[a].seq < w->kf[b].seq; });
  const int n_live = (int)by_seq.size();
  BaWorkspace* ws = ba_workspace(ctx);
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout in;                                            // uploaded: corrected pose | rank per slot | slot per rank | live mask
  const size_t o_corr = in.take(sizeof(double) * 7), o_rank = in.take(sizeof(int) * (size_t)P), o_rslot = in.take(sizeof(int) * (size_t)P), o_mask = in.take((size_t)P);
  const size_t in_bytes = in.off;
  Layout all = in;                                      // scratch behind it
  const size_t o_s1 = all.take(sizeof(double) * 7 * (size_t)P), o_inv = all.take(sizeof(double) * 7 * (size_t)P);
  const size_t o_anc = all.take(sizeof(int) * (size_t)L), o_ones = all.take((size_t)L);
  const bool want_anchor = res && res->anchor_kf_out;
  Layout dl;                                            // downloaded: poses | points | anchors (on request)
  const size_t h_pose = dl.take(sizeof(double) * 7 * (size_t)P), h_pts = dl.take(sizeof(double) * 3 * (size_t)L);
  const size_t h_anc = dl.take(want_anchor ? sizeof(int) * (size_t)L : 0);
  SSX_HIP_TRY(ctx, ws->arena.reserve(all.off));
  SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(in_bytes, dl.off)));
  char* hs = ws->stage.as<char>();
  memcpy(hs + o_corr, corrected_pose7, sizeof(double) * 7);
  {
    int* rank = reinterpret_cast<int*>(hs + o_rank); int* rslot = reinterpret_cast<int*>(hs + o_rslot); uint8_t* mask = reinterpret_cast<uint8_t*>(hs + o_mask);
    for (int s = 0; s < P; ++s) { rank[s] = -1; rslot[s] = -1; mask[s] = 0; }
    for (int r = 0; r < n_live; ++r) { rank[by_seq[r]] = r; rslot[r] = by_seq[r]; mask[by_seq[r]] = 1; }
  }
  char* base = ws->arena.as<char>();
  hipStream_t s = ctx->stream;
  const int cur = w->ext.cur;
  double* pose_cur = w->d_pose[cur].as<double>();
  double* pt_cur = w->d_point[cur].as<double>();
  double* s1 = (double*)(base + o_s1); double* inv = (double*)(base + o_inv);
  int* anc = (int*)(base + o_anc);
  uint8_t* ones = (uint8_t*)(base + o_ones);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, s));
  if (L > 0) {
    SSX_HIP_TRY(ctx, hipMemsetAsync(anc, 0x7f, sizeof(int) * (size_t)L, s));
    SSX_HIP_TRY(ctx, hipMemsetAsync(ones, 1, (size_t)L, s));
    if (E > 0)
      SSX_PROF(ctx, KID_WIN_ANCHOR, hipLaunchKernelGGL(k_win_anchor_rank, dim3((E + 255) / 256), dim3(256), 0, s, E, P, L, (const int*)w->d_epose.as<int>(),
                                                       (const int*)w->d_epoint.as<int>(), (const int*)(base + o_rank), anc));
    SSX_PROF(ctx, KID_WIN_ANCHOR, hipLaunchKernelGGL(k_win_anchor_slot, dim3((L + 255) / 256), dim3(256), 0, s, L, n_live, (const int*)(base + o_rslot), anc));
  }
  SSX_PROF(ctx, KID_LC_KEYFRAMES, hipLaunchKernelGGL(k_lc_correct_keyframes, dim3((P + 255) / 256), dim3(256), 0, s, P, cur_slot, (const double*)pose_cur,
                                                     (const uint8_t*)(base + o_mask), (const double*)(base + o_corr), s1, inv));
  if (L > 0)                                            // (old pose = the buffer the pose kernel only read)
    SSX_PROF(ctx, KID_LC_REANCHOR, hipLaunchKernelGGL(k_reanchor_points, dim3((L + 255) / 256), dim3(256), 0, s, L, (const double*)pose_cur, (const double*)inv,
                                                      (const uint8_t*)nullptr, (const int*)anc, (const uint8_t*)ones, 1, pt_cur));
  SSX_HIP_TRY(ctx, hipGetLastError());
  for (int b = 0; b < 2; ++b) SSX_HIP_TRY(ctx, hipMemcpyAsync(w->d_pose[b].p, s1, sizeof(double) * 7 * (size_t)P, hipMemcpyDeviceToDevice, s));
  if (L > 0) SSX_HIP_TRY(ctx, hipMemcpyAsync(w->d_point[1 - cur].p, pt_cur, sizeof(double) * 3 * (size_t)L, hipMemcpyDeviceToDevice, s));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_pose, s1, sizeof(double) * 7 * (size_t)P, hipMemcpyDeviceToHost, s));
  if (L > 0) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_pts, pt_cur, sizeof(double) * 3 * (size_t)L, hipMemcpyDeviceToHost, s));
  if (want_anchor && L > 0) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + h_anc, anc, sizeof(int) * (size_t)L, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  // ---- the mirror and the caller's arrays, after the one synchronisation ----
  const double* hp = reinterpret_cast<const double*>(hs + h_pose); const double* hq = reinterpret_cast<const double*>(hs + h_pts);
  for (int k = 0; k < P; ++k) if (w->kf[k].alive) memcpy(&w->poses[7 * (size_t)k], hp + 7 * (size_t)k, sizeof(double) * 7);
  int n_moved = 0;
  for (int l = 0; l < L; ++l) {
    if (!w->lm_alive[l]) continue;
    memcpy(&w->points[3 * (size_t)l], hq + 3 * (size_t)l, sizeof(double) * 3);
    n_moved += w->lm_obs[l] > 0;                        // observed = anchored (every observer of a window is a live keyframe)
  }
  if (res) {
    std::vector<int> okf, olm;
    win_order_lists(w, okf, olm);
    res->n_keyframes = (int32_t)okf.size(); res->n_landmarks = (int32_t)olm.size();
    res->n_points_moved = n_moved;
    if (res->poses_out) { size_t k = 0; for (int sl : okf) { memcpy(res->poses_out + 7 * k, &w->poses[7 * (size_t)sl], sizeof(double) * 7); ++k; } }
    if (res->points_out) { size_t k = 0; for (int l : olm) { memcpy(res->points_out + 3 * k, &w->points[3 * (size_t)l], sizeof(double) * 3); ++k; } }
    if (want_anchor) {
      const int* ha = reinterpret_cast<const int*>(hs + h_anc);
      size_t k = 0;
      for (int l : olm) { const int a = ha[l]; res->anchor_kf_out[k++] = (a >= 0 && a < P) ? w->kf[a].id : -1; }
    }
  }
  // ---- :439-448 for the window: the fused map points leave with all their observations ----
  int32_t n_removed = 0;
  st = ssx_ba_window_remove_landmarks(w, n_fused, fused_lm_ids, &n_removed);
  if (res) res->n_fused_removed = n_removed;
  return st;
}

#ifndef SSX_NO_TEST_HOOKS
int32_t ssx_ba_window_debug_rewrites(const ssx_ba_window* w) { return w ? w->n_rewrites : -1; }
#endif

}  // extern "C"
