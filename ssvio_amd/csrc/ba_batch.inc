// ssvio_amd/csrc/ba_batch.inc -- batches of small windows: ssx_ba_solve_batch, the resident ssx_ba_batch, what ssx_ba_window solves with
// (included by ba.hip after the single solve, whose outer loop, slot rule and result unpacking it shares).
// Many small windows together (one window per stereo pair of a batch, per stream of BASELINE configs[4], ...): every
// kernel of the small-window path runs ONCE for all windows (blockIdx.y = window), the device-driven LM loop of each
// window advances independently, one upload and one download carry all windows.  Same arithmetic as n calls of
// ssx_ba_solve -- identical bits per window.

struct ssx_ba_batch {
  ssx_ctx* ctx = nullptr;
  int device = 0;                                    // the ctx's device (ssx_ba_batch_destroy must not read it through ctx)
  int n = 0;
  ssx_ba_options opt;
  DevBuf arena_own; HostBuf stage_own, scal_own;     // a resident batch owns its memory; the one-call path borrows the ctx workspace
  DevBuf* arena = nullptr; HostBuf* stage = nullptr; HostBuf* scal = nullptr;
  std::vector<BaDev> devs;
  std::vector<std::vector<int>> perm;                // sorted edge -> caller's edge, per window
  std::vector<int> P, L, E, E_raw;
  std::vector<WinExt*> exts;                         // windows of ssx_ba_window objects (one-shot batches only), else empty
  const ssx_ba_problem* probs = nullptr;             // (valid during a one-shot call: the dead entries of a window's storage)
  std::vector<size_t> out_off;
  size_t out_total = 0, a_out = 0, a_gather = 0, a_head = 0, in_total = 0, o_dv = 0, o_ctrl = 0, o_ooff = 0;
  int max_ch = 1, max_rl = 1, max_rs = 1, total_ch = 0, min_ch = 0;
  bool any_solve64 = false, any_solve80 = false, any_solve = false, with_err = false, fresh = false;
  int threads = 1;
  int groups = 0;                                    // ssx_ba_batch_set_groups; 0: batch_groups(n)
};

namespace {

// Groups of windows a batch is run in, each on its own stream (batch_run).  Two: measured 2.61 / 2.45 / 2.39 / 3.01 ms for
// 64 windows in 1 / 2 / 3 / 4 groups in a process with nothing else on the GPU, but 2.61 / 2.45 / 3.24 ms next to a
// front-end on its own two streams (more streams than hardware queues: the groups then wait for each other).
int batch_groups(int n)
{
  static const int groups_env = getenv("SSX_BA_GROUPS") ? atoi(getenv("SSX_BA_GROUPS")) : 2;
  return n >= 8 ? std::min(std::max(groups_env, 1), 4) : 1;
}

// marshal + upload n small windows; SSX_ERR_UNSUPPORTED when one of them is a large window (> 16 free keyframes)
ssx_status batch_build(ssx_ctx* ctx, int n, const ssx_ba_problem* probs, const ssx_ba_options& opt, bool with_err, bool own, ssx_ba_batch* B,
                       WinExt* const* exts = nullptr)
{
  BaWorkspace* ws = ba_workspace(ctx);
  // (the marshalling scratch of the windows is kept with the ctx between calls; after a batch larger than PREPS_KEEP
  // windows it is trimmed back, see the end of this function)
  if ((int)ws->preps.size() < n) ws->preps.resize(n);
  std::vector<HostPrep>& preps = ws->preps;
  const int hw = (int)std::thread::hardware_concurrency();
  const int T = std::max(1, std::min({n, host_threads_cap(), hw > 1 ? hw / 2 : 1}));
  B->ctx = ctx; B->device = ctx->device; B->n = n; B->opt = opt; B->threads = T; B->with_err = with_err;
  if (!own) B->groups = ctx->ba_batch_groups;                       // (a resident batch has its own setting: ssx_ba_batch_set_groups)
  static const int timing_mode = getenv("SSX_BATCH_TIMING") ? std::max(atoi(getenv("SSX_BATCH_TIMING")), 1) : 0;   // phase times on stderr
  const bool timing = timing_mode == 1;                              // 1: with synchronisations (tools/batch_time.py), 2: host clocks only
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); };
  const auto t_begin = now();
  // ---- 1. host marshalling of every window (edge sort, chunks, index lists), T threads
  std::vector<ssx_status> sts(n, SSX_OK);
  ws->pool.run(n, T, [&](int w) { sts[w] = prepare(ctx, &probs[w], preps[w], true, exts ? exts[w] : nullptr); });
  for (int w = 0; w < n; ++w) if (sts[w] != SSX_OK) return sts[w];
  for (int w = 0; w < n; ++w) if (preps[w].big || (exts && !preps[w].dev_prep)) return SSX_ERR_UNSUPPORTED;
  const double t_prepare = ms_since(t_begin);
  B->probs = probs;
  if (exts) B->exts.assign(exts, exts + n); else B->exts.clear();
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  B->arena = own ? &B->arena_own : &ws->arena;
  B->stage = own ? &B->stage_own : &ws->stage;
  B->scal = own ? &B->scal_own : &ws->scal;
  // ---- 2. sizes, one arena: [blobs of all windows | BaDev[n] | ctrl int[3n] | out offsets | scratch of all windows | packed outputs | gather]
  std::vector<ArenaPlan> plans(n);                                   // (each window is planned once; the pool threads fill and wire from the plan)
  B->devs.assign(n, BaDev{});
  BandPlan no_band;
  size_t in_total = 0, rest_total = 0, out_total = 0;
  std::vector<size_t> in_off(n), rest_off(n);
  B->out_off.assign(n, 0); B->P.resize(n); B->L.resize(n); B->E.resize(n); B->E_raw.resize(n); B->perm.resize(n);
  for (int w = 0; w < n; ++w) {
    plans[w] = plan_arena(&probs[w], preps[w], no_band, 1, own, exts ? exts[w] : nullptr, false);
    in_off[w] = in_total; in_total += plans[w].in_bytes;
    rest_off[w] = rest_total; rest_total += plans[w].total - plans[w].in_bytes;
    B->out_off[w] = out_total;
    B->P[w] = preps[w].P; B->L[w] = preps[w].L; B->E[w] = preps[w].E; B->E_raw[w] = preps[w].E_raw;
    out_total += 7 * (size_t)preps[w].P + 3 * (size_t)preps[w].L + (with_err ? std::max(2 * (size_t)preps[w].E, (size_t)preps[w].E_raw) : 0);
  }
  Layout tail;
  B->o_dv = tail.take(sizeof(BaDev) * n); B->o_ctrl = tail.take(sizeof(int) * 3 * n); B->o_ooff = tail.take(sizeof(size_t) * n);
  const size_t head_bytes = in_total + tail.off;                     // everything that is uploaded
  Layout arena;
  B->a_head = arena.take(head_bytes);
  const size_t a_rest = arena.take(rest_total);
  B->a_out = arena.take(sizeof(double) * (out_total + 1));
  B->a_gather = arena.take(sizeof(double) * (size_t)n * (3 * SSX_BA_MAX_STATS));
  B->in_total = in_total; B->out_total = out_total;
  // (resident windows: their storage grows with every keyframe until it is rewritten at twice the live size, and a grown arena
  // is a hipFree -- a device-wide synchronisation, 5-20 ms in the middle of a step -- so a reallocation asks for 2.5x the need)
  const double grow = exts ? 2.5 : 1.25;
  SSX_HIP_TRY(ctx, B->arena->reserve(arena.off, grow));
  SSX_HIP_TRY(ctx, B->stage->reserve(std::max(head_bytes, sizeof(double) * (out_total + 1)), grow));
  SSX_HIP_TRY(ctx, B->scal->reserve(sizeof(double) * (size_t)n * (SC_N + 3 * SSX_BA_MAX_STATS) + sizeof(int) * 3 * n + 64));
  char* dev_base = B->arena->as<char>();
  char* hst = B->stage->as<char>();
  // ---- 3. fill the pinned mirror (T threads) and upload it, in Q pieces: the copy engine moves one piece while the threads fill
  // the next (128 C3 windows: 0.7 ms of filling, 1.65 ms on PCIe for 86 MB)
  static const int pieces_env = getenv("SSX_BA_UPLOAD_PIECES") ? std::min(std::max(atoi(getenv("SSX_BA_UPLOAD_PIECES")), 1), 16) : 4;
  const int Q = n >= 32 && !exts ? pieces_env : 1;                   // (resident windows send a few KB each: one piece)
  for (int q = 0; q < Q; ++q) {
  const int q0 = (int)((long long)n * q / Q), q1 = (int)((long long)n * (q + 1) / Q);
  ws->pool.run(q1 - q0, T, [&](int wi) {
    const int w = q0 + wi;
    BigDev bd; BandDev bnd;
    fill_blob(plans[w], &probs[w], preps[w], no_band, hst + in_off[w]);
    wire_arena(plans[w], dev_base + B->a_head + in_off[w], dev_base + a_rest + rest_off[w], &probs[w], opt.huber_delta, opt.chi2_th, 1, 0,
               exts ? exts[w] : nullptr, nullptr, nullptr, nullptr, B->devs[w], bd, bnd);
    B->devs[w].store_w = opt.jac_mode == SSX_JAC_NUMERIC_G2O ? 1 : 0;
    B->devs[w].no_err = with_err ? 0 : 1;
    if (with_err) B->perm[w] = preps[w].perm;
  });
  if (q + 1 < Q) {
    const size_t b0 = in_off[q0], b1 = in_off[q1];
    if (b1 > b0) SSX_HIP_TRY(ctx, hipMemcpyAsync(dev_base + B->a_head + b0, hst + b0, b1 - b0, hipMemcpyHostToDevice, ctx->stream));
  }
  }
  const size_t up0 = Q > 1 ? in_off[(int)((long long)n * (Q - 1) / Q)] : 0;   // the last piece goes with the tail
  memcpy(hst + in_total + B->o_dv, B->devs.data(), sizeof(BaDev) * n);
  memset(hst + in_total + B->o_ctrl, 0, sizeof(int) * 3 * n);
  memcpy(hst + in_total + B->o_ooff, B->out_off.data(), sizeof(size_t) * n);
  for (int w = 0; w < n; ++w) {
    const BaDev& d = B->devs[w];
    B->max_ch = std::max(B->max_ch, d.nCh);
    B->min_ch = w == 0 ? d.nCh : std::min(B->min_ch, d.nCh);
    B->total_ch += d.nCh;
    B->max_rl = std::max(B->max_rl, (d.nP * 27 + 63) / 64);
    B->max_rs = std::max(B->max_rs, (d.nBlk * 36 + d.nP * 6 + 63) / 64);
    if (6 * d.nP <= NB) B->any_solve64 = true; else if (6 * d.nP <= 80) B->any_solve80 = true; else B->any_solve = true;
  }
  const double t_fill = ms_since(t_begin);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev_base + B->a_head + up0, hst + up0, head_bytes - up0, hipMemcpyHostToDevice, ctx->stream));
  double t_up = 0.0;
  if (timing) { (void)hipStreamSynchronize(ctx->stream); t_up = ms_since(t_begin); }
  {
    // pair lists + work items of every window, on the device (windows marshalled with SSX_BA_HOST_LISTS brought theirs along)
    const BaDev* dvb = reinterpret_cast<const BaDev*>(dev_base + B->a_head + in_total + B->o_dv);
    if (!exts) hipLaunchKernelGGL(k_dup_state_b, dim3(16, n), dim3(CH), 0, ctx->stream, dvb);   // (windows keep both buffers themselves)
    int max_e = 1;
    bool any_prep = false;
    for (int w = 0; w < n; ++w) { max_e = std::max(max_e, B->devs[w].E_raw); any_prep = any_prep || B->devs[w].dev_prep; }
    if (any_prep) hipLaunchKernelGGL(k_prep_scatter_b, dim3((max_e + CH - 1) / CH, n), dim3(CH), 0, ctx->stream, dvb);
    hipLaunchKernelGGL(k_prep_chunk_b, dim3(B->max_ch, n), dim3(CH), 0, ctx->stream, dvb);
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  if (timing_mode == 2)
    fprintf(stderr, "[batch_build n=%d, no syncs] prepare %.3f | sizes + fill %.3f | enqueue of upload + marshalling kernels %.3f ms\n", n, t_prepare,
            t_fill - t_prepare, ms_since(t_begin) - t_fill);
  if (timing) {
    (void)hipStreamSynchronize(ctx->stream);
    fprintf(stderr, "[batch_build n=%d] prepare %.3f | sizes + fill (+ upload of 3 pieces of 4) %.3f | %.1f MB on the device %.3f later | device marshalling %.3f ms\n", n, t_prepare,
            t_fill - t_prepare, head_bytes / 1e6, t_up - t_fill, ms_since(t_begin) - t_up);
  }
  B->fresh = true;                                                   // the state buffers hold the uploaded state
  raise_lds_limits();
  // the marshalling scratch stays allocated between calls up to 64 MB (device-marshalled windows keep ~6 bytes per observation:
  // 64 C3 windows = 8 MB; host-marshalled ones ~100 bytes: the cache is trimmed back to 16 windows after such a batch)
  size_t prep_bytes = 0;
  for (const HostPrep& hp : ws->preps)
    prep_bytes += hp.slot8.capacity() + sizeof(int) * (hp.cnt_tmp.capacity() + hp.start_tmp.capacity() + hp.lm_compact.capacity() + hp.e_rec.capacity() +
                                                       hp.perm.capacity() + hp.e_pose.capacity() + hp.e_lmc.capacity() + hp.bseg.capacity()) +
                  sizeof(double) * hp.e_uv.capacity() + hp.pair_a.capacity() + hp.pair_b.capacity();
  constexpr size_t PREPS_KEEP = 16;
  if (ws->preps.size() > PREPS_KEEP && prep_bytes > (size_t(64) << 20)) { ws->preps.resize(PREPS_KEEP); ws->preps.shrink_to_fit(); }
  return SSX_OK;
}

// optimise every window of a built batch; results may be null (nothing is downloaded then, counters only in `summary`)
ssx_status batch_run(ssx_ba_batch* B, ssx_ba_result* results, int32_t* lm_iterations_total)
{
  ssx_ctx* ctx = B->ctx;
  const int n = B->n;
  const ssx_ba_options& opt = B->opt;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  char* dev_base = B->arena->as<char>();
  const BaDev* dv = reinterpret_cast<const BaDev*>(dev_base + B->a_head + B->in_total + B->o_dv);
  const size_t* d_ooff = reinterpret_cast<const size_t*>(dev_base + B->a_head + B->in_total + B->o_ooff);
  hipStream_t s = ctx->stream;
  const int wg_x = B->max_ch;                                        // workgroups per window of the linearise / Schur kernels
  if (!B->fresh) hipLaunchKernelGGL(k_reset_state_b, dim3(16, n), dim3(CH), 0, s, dv);
  B->fresh = false;
  // per-window host state of the outer loop; a window without a single chunk never runs
  std::vector<OuterState> wsn(n);
  for (int w = 0; w < n; ++w)
    wsn[w].begin(B->exts.empty() ? 0 : B->exts[w]->cur, !(B->devs[w].nCh > 0) || opt.iters <= 0, opt.outer_rounds, IDLE_ROUNDS_SKIPPED);
  // nobody asked for landmarks or per-edge errors: only the poses cross PCIe (560 B instead of 97 KB per C3 window), and they are
  // requested speculatively at the end of every outer round (below)
  bool spec_poses = results != nullptr && !B->with_err;
  int spec_maxP = 0;
  if (results) for (int w = 0; w < n; ++w) { spec_poses = spec_poses && !results[w].points_out; spec_maxP = std::max(spec_maxP, B->P[w]); }
  spec_poses = spec_poses && (size_t)n * 7 * spec_maxP <= B->out_total;
  bool spec_done = false;                                            // a speculative poses download was really enqueued (no LM round may run at all)
  double* hscal = B->scal->as<double>();                             // n x SC_N, then n x 3 x MAX_STATS, then the ctrl words
  int* h_ctrl = reinterpret_cast<int*>(hscal + (size_t)n * (SC_N + 3 * SSX_BA_MAX_STATS));
  int G = std::min(B->groups > 0 ? std::min(B->groups, 4) : batch_groups(n), std::max(n, 1));   // never an empty group (gridDim.y == 0)
  for (int g = 0; g + 1 < G; ++g) {
    if (!ctx->grp[g] && ctx->make_stream(&ctx->grp[g], false) != hipSuccess) { (void)hipGetLastError(); G = g + 1; break; }
    if (!ctx->grp_ev[g] && hipEventCreateWithFlags(&ctx->grp_ev[g], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); G = g + 1; break; }
  }
  const bool split = G > 1;
  const bool turns_on = g_turns.enabled() && ctx->ba != nullptr;
  if (turns_on && !ctx->ba->ev_turn && hipEventCreateWithFlags(&ctx->ba->ev_turn, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ctx->ba->ev_turn = nullptr; }
  auto all_done = [&] { for (int w = 0; w < n; ++w) if (!wsn[w].done) return false; return true; };
  while (!all_done()) {
    for (int w = 0; w < n; ++w) { h_ctrl[w] = wsn[w].cur; h_ctrl[n + w] = wsn[w].n_iters; h_ctrl[2 * n + w] = wsn[w].done ? 1 : 0; }
    // (no copies: the control words are READ by the kernel from the pinned block, the state words and results are WRITTEN by the
    // gather / pack kernels into pinned host memory -- a hipMemcpyAsync of this runtime runs as a blit KERNEL on the compute units
    // whenever the SDMA engines are taken, tools/microbench/copy_engine.hip, and costs the host ~10 us each)
    hipLaunchKernelGGL(k_lm_begin_batch, dim3(n), dim3(64), 0, s, dv, (const int*)h_ctrl, n, opt.iters);
    bool first_slot = true;
    for (int pass = 0;; ++pass) {
      const int slots = slots_to_enqueue(opt.iters, pass == 0, hscal, wsn.data(), n);
      if (slots == 0) break;
      // ssx_ba_device_turns: this round's kernels run after the round enqueued before it, whichever context enqueued that
      struct TurnScope {
        bool on; BaWorkspace* w; int dev; hipStream_t st;
        TurnScope(bool o, BaWorkspace* w_, int d, hipStream_t s_) : on(o), w(w_), dev(d), st(s_) { if (on) g_turns.begin(w, dev, st); }
        void close() { if (on) { g_turns.end(w, dev, w->ev_turn, st); on = false; } }
        ~TurnScope() { close(); }
      } turn(turns_on, ctx->ba, ctx->device, s);
      // The batch in G groups of windows on G streams: the narrow kernels of one half (one workgroup per window: the reduced
      // solve, the reductions -- a third of an iteration's time on a quarter of the chip) run beside the wide kernels
      // of the other.  The windows are independent; the halves meet again before the state words are gathered.
      if (split) {
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
        for (int g = 0; g + 1 < G; ++g) SSX_HIP_TRY(ctx, hipStreamWaitEvent(ctx->grp[g], ctx->ev_fork, 0));
      }
      for (int sidx = 0; sidx < slots; ++sidx) {
        const bool fused = !first_slot;                                // see ssx_ba_solve: lambda is known after the first slot
        for (int g = 0; g < G; ++g) {
          hipStream_t hs = g ? ctx->grp[g - 1] : s;
          const int w0 = (int)((long long)n * g / G), hn = (int)((long long)n * (g + 1) / G) - w0;
          const BaDev* hv = dv + w0;
          const dim3 gCh(B->max_ch, hn), gWg(wg_x, hn), gRl(B->max_rl, hn), gRs(B->max_rs, hn), gOne(1, hn);
          const bool fin_b = B->min_ch > 0 && g_trial_finish.load() != 0;   // the last chunk of k_backsub_residual finishes the trial
          if (fused) SSX_PROF_ON(ctx, hs, KID_BA_LIN_SCHUR, LAUNCH_JAC(opt.jac_mode, k_lin_schur_b, gWg, dim3(CH), FUSED_LDS_BYTES, hs, hv));
          else SSX_PROF_ON(ctx, hs, KID_BA_LINEARIZE, LAUNCH_JAC(opt.jac_mode, k_linearize_b, gWg, dim3(CH), LIN_LDS_BYTES, hs, hv, -1));
          static const bool no_both_env = getenv("SSX_BA_SPLIT_REDUCE") != nullptr;   // (tools: the two launches, for A/B timing)
          const bool both = fused && !first_slot && !no_both_env;    // (the first slot needs lambda between the two reductions)
          if (both) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_both_b, dim3(B->max_rl + B->max_rs, hn), dim3(CH), 0, hs, hv, B->max_rl));
          else SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin_b, gRl, dim3(CH), 0, hs, hv));
          if (first_slot) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init_b, gOne, dim3(64), 0, hs, hv, 1));
          if (!fused) SSX_PROF_ON(ctx, hs, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_b, gWg, dim3(CH), SCHUR_LDS_BYTES, hs, hv));
          if (!both) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_schur_b, gRs, dim3(CH), 0, hs, hv));
          if (B->any_solve64) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve64_b, gOne, dim3(CH), 0, hs, hv));
          if (B->any_solve80) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve80_b, gOne, dim3(CH), 0, hs, hv));
          if (B->any_solve) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve_b, gOne, dim3(CH), 0, hs, hv));
          SSX_PROF_ON(ctx, hs, KID_BA_BACKSUB, hipLaunchKernelGGL(k_backsub_residual_b, gCh, dim3(CH), 0, hs, hv, fin_b ? 1 : 0));
          if (!fin_b) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_reduce_trial_b, gOne, dim3(CH), 0, hs, hv, 1));   // (a window without chunks: nobody would finish its trial)
        }
        first_slot = false;
      }
      for (int g = 0; g + 1 < G; ++g) {
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->grp_ev[g], ctx->grp[g]));
        SSX_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->grp_ev[g], 0));
      }
      SSX_HIP_TRY(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal, 0);
      if (spec_poses) {
        // poses-only results ride behind the control words of this round, before the host has looked at them: if the round turns
        // out to be the last one (the usual case) the solve ends on ONE synchronisation instead of two; otherwise the next round
        // overwrites them.  The packing kernel takes the state buffer index from the window's own control block.
        hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal + (size_t)n * SC_N, 1);
        hipLaunchKernelGGL(k_pack_poses_b, dim3(n), dim3(CH), 0, s, dv, (const int*)nullptr, n, spec_maxP, B->stage->as<double>());
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
        spec_done = true;
      }
      turn.close();
      SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
    }
    for (int w = 0; w < n; ++w)
      if (!wsn[w].done) wsn[w].after_optimize(hscal + (size_t)w * SC_N, (double)B->devs[w].E, opt);
  }
  if (lm_iterations_total) { int t = 0; for (int w = 0; w < n; ++w) t += wsn[w].n_iters; *lm_iterations_total = t; }
  if (!B->exts.empty()) for (int w = 0; w < n; ++w) B->exts[w]->cur = wsn[w].cur;   // ... and the one that holds the result
  if (!results) {                                                    // nothing to download: the caller only wants the work done
    SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
    return SSX_OK;
  }
  // ---- statistics + results: one packing kernel, one download
  const bool want_err = B->with_err;
  // (iters <= 0, outer_rounds <= 0 or windows without a single chunk: no round ran, nothing was staged -- the ordinary
  // gather / pack / download returns the input state)
  const bool poses_only = spec_poses && spec_done;
  const int maxP = spec_maxP;
  double* h_out = B->stage->as<double>();
  if (!poses_only) {
  for (int w = 0; w < n; ++w) { h_ctrl[w] = wsn[w].cur; h_ctrl[n + w] = wsn[w].trial_err ? 1 : 0; h_ctrl[2 * n + w] = 1; }
  hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal + (size_t)n * SC_N, 1);
  if (want_err)                                                       // windows that never ran a trial: errors of the input state
    for (int w = 0; w < n; ++w)
      if (!wsn[w].trial_err && B->devs[w].nCh > 0)
        hipLaunchKernelGGL(k_linearize<SSX_JAC_ANALYTIC>, dim3(B->devs[w].nCh), dim3(CH), LIN_LDS_BYTES, s, B->devs[w], wsn[w].cur);
  if (want_err) {
    // (per-edge chi2 goes back in the CALLER's order: a scatter of 8-byte words, which belongs in HBM -- over PCIe every one of them
    // would be a transaction of its own; a streaming kernel then moves the packed block)
    double* d_out = reinterpret_cast<double*>(dev_base + B->a_out);
    hipLaunchKernelGGL(k_pack_out_b, dim3(64, n), dim3(CH), 0, s, dv, (const int*)h_ctrl, n, d_ooff, d_out, 1);
    hipLaunchKernelGGL(k_stream_out, dim3((unsigned)std::min<size_t>(1024, (B->out_total + 2 * CH - 1) / (2 * CH))), dim3(CH), 0, s, (const double*)d_out, h_out, B->out_total);
  } else {
    hipLaunchKernelGGL(k_pack_out_b, dim3(64, n), dim3(CH), 0, s, dv, (const int*)h_ctrl, n, d_ooff, h_out, 0);
  }
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  }   // (!poses_only)
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  static const bool timing = getenv("SSX_BATCH_TIMING") != nullptr;
  const auto t_unpack = std::chrono::steady_clock::now();
  // (poses only: 560 bytes per window -- waking the worker threads costs more than copying them here)
  ctx->ba->pool.run(n, poses_only ? 1 : B->threads, [&](int w) {
    ssx_ba_result& r = results[w];
    const int P = B->P[w], L = B->L[w];
    wsn[w].report(r);
    r.ms_linearize = r.ms_schur = r.ms_linear_solution = r.ms_update = r.ms_reduce = r.ms_comm = 0.f;
    const double* o = poses_only ? h_out + (size_t)w * 7 * maxP : h_out + B->out_off[w];
    if (r.poses_out) memcpy(r.poses_out, o, sizeof(double) * 7 * P);
    if (r.points_out && L) memcpy(r.points_out, o + 7 * (size_t)P, sizeof(double) * 3 * L);
    if (want_err)                                                    // (a device-marshalled window: chi2 already in the caller's order)
      unpack_edge_errors(r, o + 7 * (size_t)P + 3 * (size_t)L, B->E[w], B->E_raw[w], B->devs[w].dev_prep ? nullptr : B->perm[w].data(),
                         (!B->exts.empty() && B->probs) ? B->probs[w].edge_point : nullptr, opt.chi2_th);
    copy_lm_history(r, hscal + (size_t)n * SC_N + (size_t)w * 3 * SSX_BA_MAX_STATS, 0, r.n_iters);
    r.ms_total = ms;
    r.ms_setup = 0.f;
  });
  if (timing)
    fprintf(stderr, "[batch_run n=%d] solve + download of %.1f MB %.3f (GPU clock) | unpack %.3f ms\n", n, sizeof(double) * B->out_total / 1e6, ms,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_unpack).count());
  return SSX_OK;
}

}  // namespace

extern "C" {

ssx_status ssx_ba_solve_batch(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt_in, ssx_ba_result* results)
{
  if (!ctx || n < 0 || (n > 0 && (!probs || !results))) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  auto sequential = [&]() -> ssx_status {
    for (int w = 0; w < n; ++w) {
      SSX_TRY(ssx_ba_solve(ctx, &probs[w], &opt, &results[w]));
    }
    return SSX_OK;
  };
  if (opt.comm || opt.allreduce || n == 1) return sequential();
  bool with_err = false;
  for (int w = 0; w < n; ++w) if (results[w].edge_chi2 || results[w].edge_outlier) with_err = true;
  ssx_ba_batch B;
  ssx_status st = batch_build(ctx, n, probs, opt, with_err, false, &B);
  if (st == SSX_ERR_UNSUPPORTED) return sequential();                 // a large window in the batch
  if (st != SSX_OK) return st;
  return batch_run(&B, results, nullptr);
}

// A RESIDENT batch: the windows are marshalled and uploaded once and stay in HBM; every ssx_ba_batch_solve optimises
// them again from the uploaded state (bench.py times this with nothing crossing PCIe but the LM control words).
ssx_status ssx_ba_batch_create(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt_in, int32_t with_edge_errors,
                               ssx_ba_batch** out)
{
  if (!ctx || n <= 0 || !probs || !out) return SSX_ERR_INVALID_ARG;
  *out = nullptr;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  if (opt.comm || opt.allreduce) { ctx->set_error("ssx_ba_batch_create: batches do not take a collective"); return SSX_ERR_UNSUPPORTED; }
  ssx_ba_batch* B = new ssx_ba_batch();
  const ssx_status st = batch_build(ctx, n, probs, opt, with_edge_errors != 0, true, B);
  if (st != SSX_OK) {
    if (st == SSX_ERR_UNSUPPORTED) ctx->set_error("ssx_ba_batch_create: a window has more than %d free keyframes (use ssx_ba_solve)", SSX_BA_SMALL_P);
    ssx_ba_batch_destroy(B);
    return st;
  }
  *out = B;
  return SSX_OK;
}

ssx_status ssx_ba_batch_solve(ssx_ba_batch* batch, ssx_ba_result* results, int32_t* lm_iterations_total)
{
  if (!batch) return SSX_ERR_INVALID_ARG;
  return batch_run(batch, results, lm_iterations_total);
}

void ssx_ba_device_turns(int32_t enable) { g_turns.enable(enable != 0); }

ssx_status ssx_ba_set_batch_groups(ssx_ctx* ctx, int32_t groups)
{
  if (!ctx || groups < 0 || groups > 4) return SSX_ERR_INVALID_ARG;
  ctx->ba_batch_groups = groups;
  return SSX_OK;
}

int32_t ssx_ba_batch_size(const ssx_ba_batch* batch) { return batch ? batch->n : 0; }

int32_t ssx_ba_batch_groups(const ssx_ba_batch* batch) { return !batch ? 0 : (batch->groups > 0 ? std::min(batch->groups, 4) : batch_groups(batch->n)); }

void ssx_ba_batch_set_groups(ssx_ba_batch* batch, int32_t groups) { if (batch) batch->groups = groups > 0 ? groups : 0; }

void ssx_ba_batch_destroy(ssx_ba_batch* batch)
{
  if (!batch) return;
  (void)hipSetDevice(batch->device);
  batch->arena_own.release(); batch->stage_own.release(); batch->scal_own.release();
  delete batch;
}

}  // extern "C"
