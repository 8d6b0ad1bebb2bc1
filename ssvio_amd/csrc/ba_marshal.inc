// ssvio_amd/csrc/ba_marshal.inc -- host marshalling of a bundle adjustment window (included by ba.hip after BaWorkspace): the counting
// pass over the observations (prepare), the plan of the band solver, the arena and its upload, a large window's device-built records and pairs.

// chunks of whole landmarks, <= CH_E edges and <= CH_L landmarks each (h.lm_ptr, h.nLm given)
void make_chunks(HostPrep& h)
{
  h.ch_lm.clear();
  h.ch_lm.push_back(0);
  int acc_e = 0, acc_l = 0;
  for (int lc = 0; lc < h.nLm; ++lc) {
    const int k = h.lm_ptr[lc + 1] - h.lm_ptr[lc];
    if (acc_e + k > CH_E || acc_l + 1 > CH_L) {
      h.ch_lm.push_back(lc);
      acc_e = 0; acc_l = 0;
    }
    acc_e += k; acc_l += 1;
  }
  if (h.nLm > 0) h.ch_lm.push_back(h.nLm);
  h.nCh = (int)h.ch_lm.size() - 1;
  if (h.nCh < 0) h.nCh = 0;
}

// A window whose raw observation arrays and state live in device buffers of their own (ssx_ba_window): upload() then sends
// only the counting tables, and the solve starts from / leaves its result in the window's state buffers.
struct WinExt {
  const int* r_edge_pose = nullptr; const int* r_edge_point = nullptr; const double* r_edge_uv = nullptr; const uint8_t* r_edge_cam = nullptr;
  double* pose[2] = {nullptr, nullptr}; double* point[2] = {nullptr, nullptr};
  int cur = 0;                       // in: the buffer that holds the current estimate; out: the one that holds the result
  // the order the solve gives its vertices: the window's live keyframe / landmark SLOTS sorted by the caller's ids (what g2o does
  // with its vertex ids, sparse_optimizer.cpp:305-330) -- free-pose indices, the order of a landmark's edges, the landmark order of
  // the chunks all follow it, so the bits of a solve do not depend on which slots the window happened to reuse
  const int* pose_order = nullptr; int n_pose_order = 0;
  const int* lm_order = nullptr; int n_lm_order = 0;
};

static int g_prep_threads_override = 0;   // test hook (ssx_ba_debug_prepare_digest): threads of the large-window observation pass

// allow_dev_prep: small windows leave everything beyond counting to the device (see HostPrep::dev_prep); SSX_BA_HOST_PREP=1
// keeps the host marshalling below as the reference of the tests (same bits: test_device_marshalling_equals_host_marshalling)
ssx_status prepare(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, bool allow_dev_prep = true, const WinExt* ext = nullptr)
{
  const bool dead_ok = ext != nullptr;
  const int P = pr->P, L = pr->L, E = pr->E;
  if (P <= 0 || L < 0 || E < 0 || !pr->poses || (L && !pr->points) ||
      (E && (!pr->edge_pose || !pr->edge_point || !pr->edge_uv))) {
    ctx->set_error("ssx_ba: invalid problem (P=%d L=%d E=%d or null arrays)", P, L, E);
    return SSX_ERR_INVALID_ARG;
  }
  h.P = P; h.L = L; h.E = E; h.E_raw = E;
  h.pose_free.assign(P, -1);
  h.nP = 0;
  h.pose_rank.clear();
  if (ext && ext->pose_order) {
    h.pose_rank.assign(P, P);                             // (dead slots: behind every live keyframe; nothing refers to them)
    for (int i = 0; i < ext->n_pose_order; ++i) {
      const int sl = ext->pose_order[i];
      h.pose_rank[sl] = i;
      if (!(pr->pose_fixed && pr->pose_fixed[sl])) h.pose_free[sl] = h.nP++;
    }
  } else
  for (int i = 0; i < P; ++i)
    if (!(pr->pose_fixed && pr->pose_fixed[i])) h.pose_free[i] = h.nP++;
  static const bool host_prep_env = getenv("SSX_BA_HOST_PREP") != nullptr;
  static const bool host_lists_env = getenv("SSX_BA_HOST_LISTS") != nullptr;
  h.big = h.nP > SSX_BA_SMALL_P;
  h.dev_prep = allow_dev_prep && !host_prep_env && !host_lists_env;
  // counting sort of the edges by landmark
  std::vector<int>& cnt = h.cnt_tmp;
  cnt.assign(L + 1, 0);
  std::vector<int>& first_pf = h.first_pf_tmp;            // per landmark: the first free pose (in free-pose order) that observes it
  first_pf.assign((size_t)L + 1, h.nP + 1);
  if (h.dev_prep) h.slot8.resize((size_t)std::max(E, 1));
  int n_dead = 0;
  const bool big_dev = h.big && h.dev_prep;               // large window, device-marshalled: the host also counts edges per free pose
  if (big_dev) h.pe_ptr.assign((size_t)h.nP + 1, 0);
  // The one pass over the observations.  A large window (480 000 observations at BASELINE configs[3]: 1.05 ms on one core, a sixth of
  // a 10-iteration solve) takes it on the worker pool: every thread counts its range into tables of its own (slot8 = the rank
  // inside the range), the per-landmark offsets of the ranges are summed landmark-parallel, a second pass adds them -- the same
  // ranks as the serial loop, whatever the number of threads.
  static const int prep_threads = [] { const char* e = getenv("SSX_BA_PREP_THREADS"); const int v = e ? atoi(e) : 0;
                                       return v > 0 ? std::min(v, 32) : std::min(32, std::max(std::min(8, std::max(1, (int)std::thread::hardware_concurrency())), (int)std::thread::hardware_concurrency() / 2)); }();   // (measured at configs[3] on a 256-core host: 1.70 / 1.27 / 0.74 ms of prepare() on 8 / 16 / 32 threads, profiles/r06/c4_prepare_threads.txt)
  const int T = (big_dev && !dead_ok && E >= (1 << 16) && ctx->ba) ? (g_prep_threads_override > 0 ? g_prep_threads_override : prep_threads) : 1;
  if (T > 1) {
    h.thr_cnt.resize((size_t)T * L); h.thr_pe.resize((size_t)T * (h.nP + 1));
    std::vector<int> bad(T, -1);
    auto lo = [&](int t, int n) { return (int)((long long)n * t / T); };
    ctx->ba->pool.run(T, T, [&](int t) {
      int* c = h.thr_cnt.data() + (size_t)t * L; int* pe = h.thr_pe.data() + (size_t)t * (h.nP + 1);
      std::fill(c, c + L, 0); std::fill(pe, pe + h.nP + 1, 0);
      for (int e = lo(t, E), e1 = lo(t + 1, E); e < e1; ++e) {
        const int l = pr->edge_point[e], p = pr->edge_pose[e];
        if (l < 0 || l >= L || p < 0 || p >= P) { bad[t] = e; return; }
        h.slot8[e] = (uint8_t)c[l];
        c[l]++;
        const int pf = h.pose_free[p];
        if (pf >= 0) pe[pf + 1]++;
      }
    });
    for (int t = 0; t < T; ++t)
      if (bad[t] >= 0) {
        ctx->set_error("ssx_ba: edge %d references pose %d / point %d out of range", bad[t], pr->edge_pose[bad[t]], pr->edge_point[bad[t]]);
        return SSX_ERR_INVALID_ARG;
      }
    ctx->ba->pool.run(T, T, [&](int t) {
      for (int l = lo(t, L), l1 = lo(t + 1, L); l < l1; ++l) {
        int run = 0;
        for (int tt = 0; tt < T; ++tt) { int& c = h.thr_cnt[(size_t)tt * L + l]; const int k = c; c = run; run += k; }
        cnt[l + 1] = run;
      }
    });
    ctx->ba->pool.run(T - 1, T - 1, [&](int t1) {
      const int t = t1 + 1;
      const int* c = h.thr_cnt.data() + (size_t)t * L;
      for (int e = lo(t, E), e1 = lo(t + 1, E); e < e1; ++e) h.slot8[e] = (uint8_t)(h.slot8[e] + c[pr->edge_point[e]]);
    });
    for (int t = 0; t < T; ++t)
      for (int p = 0; p < h.nP; ++p) h.pe_ptr[p + 1] += h.thr_pe[(size_t)t * (h.nP + 1) + p + 1];
  } else
  for (int e = 0; e < E; ++e) {
    const int l = pr->edge_point[e], p = pr->edge_pose[e];
    if (dead_ok && l < 0) { ++n_dead; continue; }           // a window's storage: observation of a removed keyframe
    if (l < 0 || l >= L || p < 0 || p >= P) {
      ctx->set_error("ssx_ba: edge %d references pose %d / point %d out of range", e, p, l);
      return SSX_ERR_INVALID_ARG;
    }
    if (h.dev_prep) h.slot8[e] = (uint8_t)cnt[l + 1];      // (a count beyond CH_E is reported below: the wrapped value is never used)
    cnt[l + 1]++;
    { const int pfk = h.pose_free[p] >= 0 ? h.pose_free[p] : h.nP; if (pfk < first_pf[l]) first_pf[l] = pfk; }
    if (big_dev) { const int pf = h.pose_free[p]; if (pf >= 0) h.pe_ptr[pf + 1]++; }
  }
  if (n_dead && !h.dev_prep) { ctx->set_error("ssx_ba: dead observations need the device-side marshalling"); return SSX_ERR_UNSUPPORTED; }
  h.E = E - n_dead;
  // Lossless narrowing of the raw arrays on their way across PCIe (26 -> 13 bytes per observation): pose indices as bytes,
  // landmark indices as 16-bit words, and the pixel coordinates as floats when every one of them IS a float's value -- the
  // reference's measurements are cv::KeyPoint::pt (Point2f) widened to double (frontend.cpp:232-236, backend.cpp:126-160).
  h.raw_fmt = 0;
  if (h.dev_prep && !h.big && !dead_ok) {
    if (P <= 256) h.raw_fmt |= 1;
    if (L <= 65536) h.raw_fmt |= 2;
    bool exact = true;
    const double* uvp = pr->edge_uv;
    for (size_t i = 0; i < 2 * (size_t)E; ++i) exact &= (double)(float)uvp[i] == uvp[i];
    if (exact) h.raw_fmt |= 4;
  }
  h.lm_id.clear(); h.lm_ptr.clear(); h.lm_fixed.clear();
  std::vector<int>& lm_compact = h.lm_compact;
  std::vector<int>& start = h.start_tmp;
  lm_compact.assign(L, -1); start.assign(L + 1, 0);
  // The compact order of the landmarks: the caller's order (a window: ascending ids), then -- stable -- by the FIRST free pose that
  // observes a landmark.  Map points are created keyframe by keyframe, so real windows arrive almost sorted already; what the
  // sort buys is locality for every input: the landmarks of a chunk then share their poses, a chunk contributes to 15-25 of the
  // 55 blocks of a 10-keyframe reduced system instead of all of them, and writes / the reductions read only those (BaDev::touch).
  const bool lm_ordered = ext && ext->lm_order;
  const int n_visit = lm_ordered ? ext->n_lm_order : L;
  std::vector<int>& visit = h.visit_tmp;
  visit.clear();
  for (int i = 0; i < n_visit; ++i) {
    const int l = lm_ordered ? ext->lm_order[i] : i;
    if (cnt[l + 1] == 0) continue;
    if (cnt[l + 1] > CH_E) {
      ctx->set_error("ssx_ba: landmark %d has %d observations (> %d per landmark unsupported)", l, cnt[l + 1], CH_E);
      return SSX_ERR_UNSUPPORTED;
    }
    visit.push_back(l);
  }
  if (!h.big) {
    std::vector<int>& out = h.visit2_tmp;
    int bucket[SSX_BA_SMALL_P + 3] = {0};
    for (int l : visit) bucket[first_pf[l] + 1]++;
    for (int b = 0; b < SSX_BA_SMALL_P + 2; ++b) bucket[b + 1] += bucket[b];
    out.resize(visit.size());
    for (int l : visit) out[bucket[first_pf[l]]++] = l;
    visit.swap(out);
  }
  int run = 0;
  for (int l : visit) {
    lm_compact[l] = (int)h.lm_id.size();
    h.lm_id.push_back(l);
    h.lm_ptr.push_back(run);
    run += cnt[l + 1];
    h.lm_fixed.push_back(pr->point_fixed ? (pr->point_fixed[l] ? 1 : 0) : 0);
  }
  if (run != E - n_dead) { ctx->set_error("ssx_ba_window: an observation refers to a landmark that is not in the window's order list"); return SSX_ERR_INVALID_ARG; }
  h.lm_ptr.push_back(h.E);
  h.nLm = (int)h.lm_id.size();
  if (h.dev_prep) {
    // ---- the light path: chunks + chunk descriptors + the block table; the device does the rest ----
    make_chunks(h);
    h.ch_desc.resize(4 * (size_t)std::max(h.nCh, 1));
    for (int c = 0; c < h.nCh; ++c) {
      const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
      int* cd = &h.ch_desc[4 * (size_t)c];
      cd[0] = e0; cd[1] = e1 - e0; cd[2] = lm0; cd[3] = lm1 - lm0;
    }
    h.blk_pa.clear(); h.blk_pb.clear();
    h.band_w = -1;
    h.perm.clear(); h.pptr.clear(); h.pair_ptr.clear(); h.pair_a.clear(); h.pair_b.clear(); h.bseg.clear(); h.bseg_ptr.clear();
    h.pe_edge.clear(); h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
    if (h.big) {
      if (h.nP > 2048) { ctx->set_error("ssx_ba: %d free poses exceed the supported 2048", h.nP); return SSX_ERR_UNSUPPORTED; }
      for (int p = 0; p < h.nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];   // counts -> offsets; the edge list itself is the device's (big_records)
      h.nBlk = 0;
      h.dev_lists = false;
      return SSX_OK;
    }
    h.pe_ptr.clear();
    for (int a = 0; a < h.nP; ++a)
      for (int b = a; b < h.nP; ++b) { h.blk_pa.push_back((int8_t)a); h.blk_pb.push_back((int8_t)b); }
    h.nBlk = (int)h.blk_pa.size();
    h.dev_lists = true;
    return SSX_OK;
  }
  h.perm.assign(E, 0);
  {
    std::vector<int> fill((size_t)L, 0);
    for (int l = 0; l < L; ++l) if (lm_compact[l] >= 0) fill[l] = h.lm_ptr[lm_compact[l]];
    for (int e = 0; e < E; ++e) h.perm[fill[pr->edge_point[e]]++] = e;
  }
  // inside a landmark: stable sort by pose so that duplicates of a (landmark,pose) pair are adjacent
  for (int lc = 0; lc < h.nLm; ++lc) {
    const int a = h.lm_ptr[lc], b = h.lm_ptr[lc + 1];
    bool sorted = true;
    for (int s = a + 1; s < b && sorted; ++s) sorted = pr->edge_pose[h.perm[s - 1]] <= pr->edge_pose[h.perm[s]];
    if (!sorted)
      std::stable_sort(h.perm.begin() + a, h.perm.begin() + b, [&](int x, int y) { return pr->edge_pose[x] < pr->edge_pose[y]; });
  }
  h.e_pose.resize(E); h.e_lmc.resize(E); h.e_cam.resize(E); h.e_dup.assign(E, 0); h.e_uv.resize(2 * (size_t)E);
  for (int s = 0; s < E; ++s) {
    const int e = h.perm[s];
    h.e_pose[s] = pr->edge_pose[e];
    h.e_lmc[s] = lm_compact[pr->edge_point[e]];
    h.e_cam[s] = pr->edge_cam ? (pr->edge_cam[e] ? 1 : 0) : 0;
    h.e_uv[s] = pr->edge_uv[2 * (size_t)e];
    h.e_uv[(size_t)E + s] = pr->edge_uv[2 * (size_t)e + 1];
    if (s > 0 && h.e_lmc[s] == h.e_lmc[s - 1] && h.e_pose[s] == h.e_pose[s - 1]) h.e_dup[s] = 1;
  }
  make_chunks(h);
  h.ch_desc.resize(4 * (size_t)std::max(h.nCh, 1)); h.e_rec.resize(4 * (size_t)std::max(E, 1)); h.l_rec.resize(4 * (size_t)std::max(h.nLm, 1));
  h.lm_chunk.resize((size_t)std::max(h.nLm, 1));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
    int* cd = &h.ch_desc[4 * (size_t)c];
    cd[0] = e0; cd[1] = e1 - e0; cd[2] = lm0; cd[3] = lm1 - lm0;
    for (int lc = lm0; lc < lm1; ++lc) {
      h.lm_chunk[lc] = c;
      int* lr = &h.l_rec[4 * (size_t)lc];
      lr[0] = h.lm_ptr[lc] - e0; lr[1] = h.lm_ptr[lc + 1] - h.lm_ptr[lc]; lr[2] = h.lm_id[lc]; lr[3] = h.lm_fixed[lc];
      for (int s2 = h.lm_ptr[lc]; s2 < h.lm_ptr[lc + 1]; ++s2) {
        int* er = &h.e_rec[4 * (size_t)s2];
        er[0] = h.e_pose[s2]; er[1] = h.pose_free[h.e_pose[s2]]; er[2] = h.lm_id[lc];
        const int next_dup = (s2 + 1 < h.lm_ptr[lc + 1] && h.e_dup[s2 + 1]) ? 1 : 0;   // duplicates are of the same landmark
        er[3] = (int)h.e_cam[s2] | ((int)h.e_dup[s2] << 1) | ((int)h.lm_fixed[lc] << 2) | (next_dup << 3) |
                ((h.pose_free[h.e_pose[s2]] < 0 ? 1 : 0) << 5) | ((lc - lm0) << 8);
      }
    }
  }
  h.blk_pa.clear(); h.blk_pb.clear();
  if (h.nP <= SSX_BA_SMALL_P)
    for (int a = 0; a < h.nP; ++a)
      for (int b = a; b < h.nP; ++b) { h.blk_pa.push_back((int8_t)a); h.blk_pb.push_back((int8_t)b); }
  h.nBlk = (int)h.blk_pa.size();
  if (h.big) {
    const int nP = h.nP;
    if (nP > 2048) { ctx->set_error("ssx_ba: %d free poses exceed the supported 2048", nP); return SSX_ERR_UNSUPPORTED; }
    // pose-major edge list (free poses)
    h.pe_ptr.assign(nP + 1, 0);
    for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_ptr[pf + 1]++; }
    for (int p = 0; p < nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];
    h.pe_edge.assign(std::max(h.pe_ptr[nP], 1), 0);
    {
      std::vector<int> fill(h.pe_ptr.begin(), h.pe_ptr.end() - 1);
      for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_edge[fill[pf]++] = s; }
    }
    // the non-zero blocks of the reduced system and their (edge, edge) pair lists are built on the device (build_pairs)
    h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
    h.nBlk = 0;
    h.band_w = -1;
    h.bseg.clear(); h.bseg_ptr.clear();
    h.dev_lists = false;
    return SSX_OK;
  }
  // per-chunk index lists: edges grouped by free pose; leader pairs grouped by reduced-system block
  h.dev_lists = !host_lists_env;                // (SSX_BA_HOST_LISTS: the host builder stays as the reference of the tests)
  const int nP = h.nP, nBlk = h.nBlk;
  h.pptr.assign((size_t)h.nCh * (nP + 1) + 1, 0);
  h.pair_ptr.assign((size_t)h.nCh * (nBlk + 1) + 1, 0);
  h.pair_a.clear(); h.pair_b.clear();
  h.bseg.clear(); h.bseg_ptr.assign(2 * (size_t)h.nCh + 2, 0);
  h.touch.assign(TOUCH_WORDS * (size_t)(h.nCh + 1), 0u);
  std::vector<int> blk_of((size_t)std::max(nP, 1) * std::max(nP, 1), -1);
  for (int b = 0; b < nBlk; ++b) blk_of[(size_t)h.blk_pa[b] * nP + h.blk_pb[b]] = b;
  std::vector<int> pc(nP + 1), bc(nBlk + 1);
  std::vector<uint32_t>& tmp_pairs = h.tmp_pairs;
  std::vector<std::pair<int, int>>& order = h.tmp_order;   // (-part length, block)
  h.bseg.reserve(4 * ((size_t)h.nCh * (nBlk + 8)));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1];
    const int e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
    // --- by pose ---
    std::fill(pc.begin(), pc.end(), 0);
    for (int s = e0; s < e1; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) pc[pf + 1]++; }
    for (int p = 0; p < nP; ++p) pc[p + 1] += pc[p];
    uint16_t* pp = &h.pptr[(size_t)c * (nP + 1)];
    for (int p = 0; p <= nP; ++p) pp[p] = (uint16_t)pc[p];
    int tail = pc[nP];
    for (int s = e0; s < e1; ++s) {
      const int pf = h.pose_free[h.e_pose[s]];
      const int pos = pf >= 0 ? pc[pf]++ : tail++;
      h.e_rec[4 * (size_t)s + 3] = (h.e_rec[4 * (size_t)s + 3] & 0xFFFF) | (pos << 16);   // the inverse map, for the kernels that store pose-major
    }
    if (h.dev_lists) continue;                    // k_build_lists (same lists, on the device)
    // --- pairs by block: one pass over the landmarks of the chunk lists (block, edge a, edge b), a counting sort by
    // block keeps the landmark order inside a block ---
    std::fill(bc.begin(), bc.end(), 0);
    tmp_pairs.clear();
    for (int lc = lm0; lc < lm1; ++lc) {
      if (h.lm_fixed[lc]) continue;
      int nl = 0;
      uint8_t led[CH_E]; int16_t lpf[CH_E];
      for (int s = h.lm_ptr[lc]; s < h.lm_ptr[lc + 1]; ++s) {
        const int pf = h.pose_free[h.e_pose[s]];
        if (pf >= 0 && !h.e_dup[s]) { led[nl] = (uint8_t)(s - e0); lpf[nl] = (int16_t)pf; ++nl; }
      }
      for (int i = 0; i < nl; ++i) {
        const int* row = &blk_of[(size_t)lpf[i] * nP];
        for (int j = i; j < nl; ++j) {
          const int b = row[lpf[j]];                        // pa <= pb: edges of a landmark are sorted by pose
          bc[b + 1]++;
          tmp_pairs.push_back((uint32_t)b << 16 | (uint32_t)led[i] << 8 | led[j]);
        }
      }
    }
    {
      const int base = (int)h.pair_a.size();
      bc[0] = base;
      for (int b = 0; b < nBlk; ++b) bc[b + 1] += bc[b];
      int* bp = &h.pair_ptr[(size_t)c * (nBlk + 1)];
      for (int b = 0; b <= nBlk; ++b) bp[b] = bc[b];
      h.pair_a.resize(bc[nBlk]); h.pair_b.resize(bc[nBlk]);
      for (const uint32_t k : tmp_pairs) {
        const int q = bc[k >> 16]++;
        h.pair_a[q] = (uint8_t)(k >> 8); h.pair_b[q] = (uint8_t)k;
      }
    }
    // --- work items of the block phase.  A lane walks ONE pair list and a wave takes as long as its longest list, so
    // the lists (0 .. 40 pairs in a local window) are cut into parts of about the same length, the parts sorted by
    // length, and the parts of one block kept inside one wave (their partial sums meet through wave shuffles).
    {
      const int* bp = &h.pair_ptr[(size_t)c * (nBlk + 1)];
      const int base = bp[0];
      int maxlen = 0;
      for (int b = 0; b < nBlk; ++b) maxlen = std::max(maxlen, bp[b + 1] - bp[b]);
      const int seg = std::max(BSEG_MIN, (maxlen + BSEG_PARTS - 1) / BSEG_PARTS);
      const bool dense = dense_slabs_mode() != 0;
      // (BaDev::touch, as k_build_lists writes it: blocks with pairs, poses with edges)
      unsigned int* tm = &h.touch[(size_t)c * TOUCH_WORDS];
      for (int b = 0; b < nBlk + nP; ++b) {
        const bool on = b < nBlk ? (bp[b + 1] > bp[b]) : (pp[b - nBlk + 1] > pp[b - nBlk]);
        if (on || dense) tm[b >> 5] |= 1u << (b & 31);
      }
      order.clear();
      for (int b = 0; b < nBlk; ++b) {
        const int n = bp[b + 1] - bp[b], k = (n == 0 && !dense) ? 0 : std::max(1, (n + seg - 1) / seg);
        order.push_back({k ? -((n + k - 1) / k) : 0, b});
      }
      std::stable_sort(order.begin(), order.end());
      h.bseg_ptr[2 * c] = (int)(h.bseg.size() / 4);
      int pos = 0;                                // in items (16 per wave, four lanes each; a block's parts inside one row of 16 lanes)
      for (const auto& ob : order) {
        const int b = ob.second, n = bp[b + 1] - bp[b], k = (n == 0 && !dense) ? 0 : std::max(1, (n + seg - 1) / seg), len = k ? (n + k - 1) / k : 0;
        while ((pos & 3) + k > 4) { h.bseg.push_back(-1); h.bseg.push_back(0); h.bseg.push_back(0); h.bseg.push_back(1 << 4); ++pos; }
        for (int i = 0; i < k; ++i) {
          const int q0 = bp[b] - base + std::min(n, i * len), q1 = bp[b] - base + std::min(n, (i + 1) * len);
          h.bseg.push_back(b); h.bseg.push_back(q0); h.bseg.push_back(q1); h.bseg.push_back(i | (k << 4));
          ++pos;
        }
      }
      h.bseg_ptr[2 * c + 1] = (int)(h.bseg.size() / 4) - h.bseg_ptr[2 * c];
    }
  }
  return SSX_OK;
}

// carve the arena and upload the problem
// Segment plan of the band solver (ba_band.inc): w > 0 switches it on.  K interiors of >= w poses separated by w poses.
struct BandPlan {
  int w = 0, K = 1;
  std::vector<int> seg_p0, seg_m;
  BcrPlan bcr;                       // bcr.on: block cyclic reduction (ba_bcr.inc) solves the band instead of the segments
};

void plan_band(int nP, int w, BandPlan& bp)
{
  bp.w = w; bp.K = 1; bp.seg_p0.assign(1, 0); bp.seg_m.assign(1, nP - w);
  if (w <= 0) return;
  if (nP >= 48) {
    // dependent chain ~ nP / K interior pivots + 1.5 K w separator pivots (the top window is wider)
    int K = (int)std::lround(std::sqrt((double)nP / (1.5 * w)));
    K = std::max(2, std::min(K, 64));
    while (K > 1 && (nP - K * w) / K < w) --K;                      // every interior must hold >= w poses
    while ((nP - K * w + K - 1) / K > 480) ++K;                     // LDS of the back-substitution
    bp.K = K;
  }
  if (bp.K == 1) return;
  const int K = bp.K, inner = nP - K * w, base = inner / K, rem = inner % K;
  bp.seg_p0.resize(K); bp.seg_m.resize(K);
  int p = 0;
  for (int k = 0; k < K; ++k) {
    bp.seg_p0[k] = p;
    bp.seg_m[k] = base + (k < rem ? 1 : 0);
    p += bp.seg_m[k] + w;
  }
}

struct UploadPlace {          // where a window of a batch lives (nullptr = a single window in the ctx arena)
  bool dry = false;            // sizing pass: only in_bytes / rest_bytes are computed
  size_t in_bytes = 0, rest_bytes = 0;
  char* in_dev = nullptr;      // uploaded blob on the device
  char* rest_dev = nullptr;    // scratch on the device
  char* in_host = nullptr;     // pinned mirror of the blob
  bool keep_init = false;      // a RESIDENT batch keeps a pristine copy of the uploaded state (it is solved again from it)
};

ssx_status upload(ssx_ctx* ctx, const ssx_ba_problem* pr, const HostPrep& h, double huber_delta, double chi2_th,
                  int world, int rank, BaDev& d, BigDev& bd, const BandPlan& bp, BandDev& bnd, UploadPlace* place = nullptr,
                  const WinExt* ext = nullptr, const BaDev* recs = nullptr, const int* pe_ptr_dev = nullptr, const int* pe_edge_dev = nullptr)
{
  const bool rz = recs != nullptr;               // large window whose records / columns / raw arrays already live on the device (big_records)
  BaWorkspace* ws = ba_workspace(ctx);
  const bool dup_state = place != nullptr;       // batched windows: the second state buffer is part of the uploaded blob
  const int P = h.P, L = h.L, E = h.E, nP = h.nP, nLm = h.nLm, nCh = h.nCh, nBlk = h.nBlk;
  const int n = 6 * nP;
  const bool big = h.big;
  const bool dev_lists = h.dev_lists && !big;
  const int bseg_cap = dev_lists ? 2 * nBlk * BSEG_PARTS + 16 : 0;
  const size_t nPairs = dev_lists ? 0 : h.pair_a.size();
  const int lin_stride = big ? 2 : nP * 27 + 2;
  const int n_pad = big ? ((n + NB - 1) / NB) * NB : 0;
  const size_t nBlkS = h.sblk_pa.size();
  Layout in;   // input blob (mirrored in pinned staging)
  const size_t o_pose_free = in.take(rz ? 0 : sizeof(int) * P);
  // (the landmark / chunk tables and the structure-of-arrays edge columns are read by the large-window kernels only: the
  // small-window kernels take everything from the packed records -- a quarter of a C3 window's blob not staged, not sent)
  const bool dev_prep = h.dev_prep && !big;
  const bool lm_tables = big || dev_prep;
  const size_t o_lm_fixed = in.take(lm_tables && !rz ? nLm : 0);
  const size_t o_lm_id = in.take(lm_tables && !rz ? sizeof(int) * nLm : 0);
  const size_t o_lm_ptr = in.take(lm_tables && !rz ? sizeof(int) * (nLm + 1) : 0);
  const size_t o_ch_lm = in.take(big && !rz ? sizeof(int) * (nCh + 1) : 0);
  const size_t o_e_pose = in.take(big && !rz ? sizeof(int) * E : 0);
  const size_t o_e_lmc = in.take(big && !rz ? sizeof(int) * E : 0);
  const size_t o_e_cam = in.take(big && !rz ? E : 0);
  // (device-marshalled windows upload the caller's arrays; the sorted columns / records are scratch, written by k_prep_chunk)
  size_t o_e_dup = (dev_prep || rz) ? 0 : in.take(E);
  size_t o_e_uv = (dev_prep || rz) ? 0 : in.take(sizeof(double) * 2 * E);
  const size_t o_ch_desc = in.take(rz ? 0 : sizeof(int) * 4 * (size_t)(nCh + 1));
  size_t o_e_rec = (dev_prep || rz) ? 0 : in.take(sizeof(int) * 4 * (size_t)(E + 1));
  size_t o_l_rec = (dev_prep || rz) ? 0 : in.take(sizeof(int) * 4 * (size_t)(nLm + 1));
  const size_t o_blk_pa = in.take(nBlk + 1);
  const size_t o_blk_pb = in.take(nBlk + 1);
  size_t o_pptr = (dev_prep || rz) ? 0 : in.take(sizeof(uint16_t) * (h.pptr.size() + 1));
  // (an ssx_ba_window keeps the raw observation arrays and the state in device buffers of its own: `ext`)
  const int E_raw = h.E_raw;
  const bool raw_in = dev_prep && !ext;
  const bool have_cam = dev_prep && (ext ? ext->r_edge_cam != nullptr : pr->edge_cam != nullptr);
  const size_t o_lm_compact = in.take(dev_prep ? sizeof(int) * (size_t)(L + 1) : 0);
  const bool have_rank = dev_prep && !h.pose_rank.empty();
  const size_t o_pose_rank = in.take(have_rank ? sizeof(int) * (size_t)P : 0);
  const int raw_fmt = raw_in && !rz ? h.raw_fmt : 0;
  const size_t o_r_pose = in.take(raw_in ? ((raw_fmt & 1) ? 1 : sizeof(int)) * (size_t)(E + 1) : 0);
  const size_t o_r_point = in.take(raw_in ? ((raw_fmt & 2) ? sizeof(uint16_t) : sizeof(int)) * (size_t)(E + 1) : 0);
  const size_t o_r_uv = in.take(raw_in ? ((raw_fmt & 4) ? sizeof(float) : sizeof(double)) * 2 * (size_t)(E + 1) : 0);
  const size_t o_r_cam = in.take(have_cam && raw_in ? (size_t)E + 1 : 0);
  const size_t o_slot8 = in.take(dev_prep ? (size_t)E_raw + 1 : 0);
  // (host-built lists travel with the blob; device-built ones are scratch behind it, a fixed capacity per chunk)
  size_t o_pair_a = dev_lists ? 0 : in.take(nPairs + 1);
  size_t o_pair_b = dev_lists ? 0 : in.take(nPairs + 1);
  size_t o_pair_ptr = dev_lists ? 0 : in.take(sizeof(int) * (h.pair_ptr.size() + 1));
  size_t o_bseg = dev_lists ? 0 : in.take(sizeof(int) * (h.bseg.size() + 4));
  size_t o_bseg_ptr = dev_lists ? 0 : in.take(sizeof(int) * (h.bseg_ptr.size() + 1));
  const size_t touch_bytes = big ? 0 : sizeof(unsigned int) * TOUCH_WORDS * (size_t)(nCh + 1);
  size_t o_touch = (dev_lists || big) ? 0 : in.take(touch_bytes);
  const size_t o_pe_ptr = in.take(rz ? 0 : sizeof(int) * (h.pe_ptr.size() + 1));
  const size_t o_pe_edge = in.take(rz ? 0 : sizeof(int) * (h.pe_edge.size() + 1));
  const size_t o_sblk_pa = in.take(sizeof(int) * (nBlkS + 1));
  const size_t o_sblk_pb = in.take(sizeof(int) * (nBlkS + 1));
  const size_t o_spair_ptr = in.take(sizeof(int) * (h.spair_ptr.size() + 1));
  const bool band = big && bp.w > 0;
  const size_t o_seg_p0 = in.take(sizeof(int) * (bp.seg_p0.size() + 1));
  const size_t o_seg_m = in.take(sizeof(int) * (bp.seg_m.size() + 1));
  const bool bcr = band && bp.bcr.on;                                 // block cyclic reduction of the band (ba_bcr.inc)
  const size_t o_bcr_p0 = in.take(bcr ? sizeof(int) * (bp.bcr.p0.size() + 1) : 0);
  const size_t o_bcr_elim = in.take(bcr ? sizeof(int) * (bp.bcr.elim.size() + 4) : 0);
  if (ext && !dev_prep) { ctx->set_error("ssx_ba: a window needs the device-side marshalling (<= %d free keyframes, no SSX_BA_HOST_PREP)", SSX_BA_SMALL_P); return SSX_ERR_UNSUPPORTED; }
  const size_t o_pose0 = in.take(ext ? 0 : sizeof(double) * 7 * P);
  const size_t o_point0 = in.take(ext ? 0 : sizeof(double) * 3 * (L + 1));
  // (the state crosses PCIe ONCE: the second buffer and, for a resident batch, the pristine copy are made on the device,
  // k_dup_state_b -- the blob of a C3 window carried three copies of its 96 KB of landmarks)
  const size_t in_bytes = in.off;
  Layout all = in;
  const size_t o_pose1 = ext ? 0 : all.take(sizeof(double) * 7 * P);
  const size_t o_point1 = ext ? 0 : all.take(sizeof(double) * 3 * (L + 1));
  const bool keep_init = dup_state && !ext && place->keep_init;
  const size_t o_pose_init = keep_init ? all.take(sizeof(double) * 7 * P) : 0;
  const size_t o_point_init = keep_init ? all.take(sizeof(double) * 3 * (L + 1)) : 0;
  size_t o_perm = 0, o_c2 = 0;
  if (dev_prep) {
    o_e_dup = all.take((size_t)E + 1);
    o_e_uv = all.take(sizeof(double) * 2 * (size_t)(E + 1));
    o_e_rec = all.take(sizeof(int) * 4 * (size_t)(E + 1));
    o_l_rec = all.take(sizeof(int) * 4 * (size_t)(nLm + 1));
    o_pptr = all.take(sizeof(uint16_t) * ((size_t)(nCh + 1) * (nP + 1) + 1));
    o_perm = all.take(sizeof(int) * (size_t)(E + 1));
    o_c2 = all.take(sizeof(double) * (size_t)(E_raw + 1));
  }
  if (dev_lists) {
    o_pair_a = all.take((size_t)(nCh + 1) * MAX_PAIRS);
    o_pair_b = all.take((size_t)(nCh + 1) * MAX_PAIRS);
    o_pair_ptr = all.take(sizeof(int) * ((size_t)(nCh + 1) * (nBlk + 1) + 1));
    o_bseg = all.take(sizeof(int) * 4 * ((size_t)(nCh + 1) * bseg_cap + 1));
    o_bseg_ptr = all.take(sizeof(int) * (2 * (size_t)nCh + 2));
    o_touch = all.take(touch_bytes);
  }
  const size_t o_W = all.take(sizeof(double) * 18 * (size_t)E);
  const size_t o_err_lin = all.take(sizeof(double) * 2 * (size_t)E);
  const size_t o_err_trial = all.take(sizeof(double) * 2 * (size_t)E);
  const size_t o_Hll = all.take(sizeof(double) * 6 * (size_t)nLm);
  const size_t o_bl = all.take(sizeof(double) * 3 * (size_t)nLm);
  const size_t o_lin_slab = all.take(sizeof(double) * (size_t)(nCh + 1) * lin_stride);
  const size_t o_Hpp = all.take(sizeof(double) * (nP + 1) * UPPER6);
  const size_t o_bp = all.take(sizeof(double) * (nP + 1) * 6);
  const size_t iter_count = (size_t)nP * 27 + 1 + world;
  // (band solver: iter_comm sits right behind [band | rhs] so that ONE all-reduce per trial carries the reduced system AND the
  // linearisation's pose blocks / chi2 -- see big_trial)
  const bool band_pre = big && bp.w > 0;
  size_t o_iter = band_pre ? 0 : all.take(sizeof(double) * (iter_count + 1));
  const size_t o_schur = all.take(big ? 256 : sizeof(double) * (size_t)(nCh + 1) * (nBlk * 36 + nP * 6));
  const size_t o_trial_comm = all.take(big ? 256 : sizeof(double) * ((size_t)n * n + n + 1));
  const size_t o_BDa = all.take(big ? sizeof(double) * 18 * (size_t)(E + 1) : 256);
  const size_t o_Wma = all.take(big ? sizeof(double) * 18 * (size_t)(E + 1) : 256);
  const size_t o_Cv = all.take(big ? sizeof(double) * 6 * (size_t)(E + 1) : 256);
  const size_t o_S = all.take((big && !band) ? sizeof(double) * (size_t)(n_pad + NB) * n_pad : 256);
  // band solver: band + rhs, segment updates, factors of both levels, the separator system
  const int bw = bp.w, bK = bp.K, bnPr = bK * bw, bwr = 2 * bw - 1;
  const int NW0 = 6 * (2 * bw + 1) + 1, LS0 = 36 + NW0 * 6;
  const int w1 = bK == 1 ? bw : bwr, NW1 = 6 * (w1 + 1 + bw) + 1, LS1 = 36 + NW1 * 6;
  const int NU = 12 * bw + 1;
  const size_t sb_count = band ? (size_t)nP * (bw + 1) * 36 + (size_t)n : 0;
  const size_t sr_count = (band && bK > 1) ? (size_t)bnPr * (bwr + 1) * 36 + 6 * (size_t)bnPr : 0;
  const size_t o_Sb = all.take(sizeof(double) * (sb_count + 1 + (band ? iter_count + 1 : 0)));
  if (band) o_iter = o_Sb + sizeof(double) * sb_count;
  const size_t o_U = all.take(band ? sizeof(double) * (size_t)bK * NU * NU : 256);
  const size_t o_Ls0 = all.take((band && bK > 1) ? sizeof(double) * (size_t)nP * LS0 : 256);
  const size_t o_Sr = all.take(sizeof(double) * (sr_count + 1));
  const size_t o_Ls1 = all.take(band ? sizeof(double) * (size_t)(bK > 1 ? bnPr : nP) * LS1 : 256);
  const size_t o_bcr_mem = all.take(bcr ? sizeof(double) * (bcr_mem_doubles(bp.bcr.N, bp.bcr.m) + 8) : 256);
  const size_t o_xr = all.take(sizeof(double) * (6 * (size_t)bnPr + 8));
  const size_t o_x = all.take(sizeof(double) * (n_pad + 8));
  const size_t o_Ld = all.take(sizeof(double) * NB * NB);
  const size_t o_invd = all.take(sizeof(double) * (n_pad + 8));
  const size_t o_Ninv = all.take(sizeof(double) * 4 * 256);
  const size_t o_scale_part = all.take(sizeof(double) * 64);
  const size_t o_xp = all.take(sizeof(double) * (n + 1));
  const size_t o_trial = all.take(sizeof(double) * 3 * (nCh + 1));
  const size_t o_scal_comm = all.take(sizeof(double) * 4);
  const size_t o_scal = all.take(sizeof(double) * SC_N);
  const size_t o_lmstat = all.take(sizeof(double) * 3 * SSX_BA_MAX_STATS);
  const size_t o_ticket = all.take(sizeof(unsigned int) * 4);

  if (place && place->dry) {                     // sizing pass of a batch
    place->in_bytes = in_bytes;
    place->rest_bytes = all.off - in_bytes;
    return SSX_OK;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!place) {
    SSX_HIP_TRY(ctx, ws->arena.reserve(all.off));
    SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(in_bytes, sizeof(double) * (7 * (size_t)P + 3 * (size_t)L + 2 * (size_t)E + (size_t)h.E_raw))));
    SSX_HIP_TRY(ctx, ws->scal.reserve(sizeof(double) * (SC_N + 3 * SSX_BA_MAX_STATS)));
  }
  char* hs = place ? place->in_host : ws->stage.as<char>();
  if (!rz) memcpy(hs + o_pose_free, h.pose_free.data(), sizeof(int) * P);
  if (lm_tables && nLm && !rz) {
    memcpy(hs + o_lm_fixed, h.lm_fixed.data(), nLm);
    memcpy(hs + o_lm_id, h.lm_id.data(), sizeof(int) * nLm);
  }
  if (lm_tables && !rz) memcpy(hs + o_lm_ptr, h.lm_ptr.data(), sizeof(int) * (nLm + 1));
  if (nCh && !rz) memcpy(hs + o_ch_desc, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
  if (dev_prep) {
    if (L) memcpy(hs + o_lm_compact, h.lm_compact.data(), sizeof(int) * (size_t)L);
    if (have_rank) memcpy(hs + o_pose_rank, h.pose_rank.data(), sizeof(int) * (size_t)P);
    if (E && raw_in) {
      if (raw_fmt & 1) { uint8_t* o = (uint8_t*)(hs + o_r_pose); for (int e = 0; e < E; ++e) o[e] = (uint8_t)pr->edge_pose[e]; }
      else memcpy(hs + o_r_pose, pr->edge_pose, sizeof(int) * (size_t)E);
      if (raw_fmt & 2) { uint16_t* o = (uint16_t*)(hs + o_r_point); for (int e = 0; e < E; ++e) o[e] = (uint16_t)pr->edge_point[e]; }
      else memcpy(hs + o_r_point, pr->edge_point, sizeof(int) * (size_t)E);
      if (raw_fmt & 4) { float* o = (float*)(hs + o_r_uv); for (size_t i = 0; i < 2 * (size_t)E; ++i) o[i] = (float)pr->edge_uv[i]; }
      else memcpy(hs + o_r_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
      if (have_cam) memcpy(hs + o_r_cam, pr->edge_cam, (size_t)E);
    }
    if (E_raw) memcpy(hs + o_slot8, h.slot8.data(), (size_t)E_raw);
  } else if (!rz) {
  if (E) memcpy(hs + o_e_rec, h.e_rec.data(), sizeof(int) * 4 * (size_t)E);
  if (nLm) memcpy(hs + o_l_rec, h.l_rec.data(), sizeof(int) * 4 * (size_t)nLm);
  }
  if (big && !rz) memcpy(hs + o_ch_lm, h.ch_lm.data(), sizeof(int) * h.ch_lm.size());
  if (E && !rz) {
    if (big) {
      memcpy(hs + o_e_pose, h.e_pose.data(), sizeof(int) * E);
      memcpy(hs + o_e_lmc, h.e_lmc.data(), sizeof(int) * E);
      memcpy(hs + o_e_cam, h.e_cam.data(), E);
    }
    if (!dev_prep) {
      memcpy(hs + o_e_dup, h.e_dup.data(), E);
      memcpy(hs + o_e_uv, h.e_uv.data(), sizeof(double) * 2 * E);
    }
  }
  if (nBlk) {
    memcpy(hs + o_blk_pa, h.blk_pa.data(), nBlk);
    memcpy(hs + o_blk_pb, h.blk_pb.data(), nBlk);
  }
  if (!dev_prep && !h.pptr.empty()) memcpy(hs + o_pptr, h.pptr.data(), sizeof(uint16_t) * h.pptr.size());
  if (nPairs) {
    memcpy(hs + o_pair_a, h.pair_a.data(), nPairs);
    memcpy(hs + o_pair_b, h.pair_b.data(), nPairs);
  }
  if (!dev_lists) {
    if (!h.pair_ptr.empty()) memcpy(hs + o_pair_ptr, h.pair_ptr.data(), sizeof(int) * h.pair_ptr.size());
    if (!h.bseg.empty()) memcpy(hs + o_bseg, h.bseg.data(), sizeof(int) * h.bseg.size());
    if (!h.bseg_ptr.empty()) memcpy(hs + o_bseg_ptr, h.bseg_ptr.data(), sizeof(int) * h.bseg_ptr.size());
    if (!big && !h.touch.empty()) memcpy(hs + o_touch, h.touch.data(), sizeof(unsigned int) * h.touch.size());
  }
  if (big && !rz) {
    memcpy(hs + o_pe_ptr, h.pe_ptr.data(), sizeof(int) * h.pe_ptr.size());
    memcpy(hs + o_pe_edge, h.pe_edge.data(), sizeof(int) * h.pe_edge.size());
  }
  if (big) {
    memcpy(hs + o_sblk_pa, h.sblk_pa.data(), sizeof(int) * nBlkS);
    memcpy(hs + o_sblk_pb, h.sblk_pb.data(), sizeof(int) * nBlkS);
    memcpy(hs + o_spair_ptr, h.spair_ptr.data(), sizeof(int) * h.spair_ptr.size());
  }
  if (band) {
    memcpy(hs + o_seg_p0, bp.seg_p0.data(), sizeof(int) * bp.seg_p0.size());
    memcpy(hs + o_seg_m, bp.seg_m.data(), sizeof(int) * bp.seg_m.size());
    if (bcr) {
      memcpy(hs + o_bcr_p0, bp.bcr.p0.data(), sizeof(int) * bp.bcr.p0.size());
      memcpy(hs + o_bcr_elim, bp.bcr.elim.data(), sizeof(int) * bp.bcr.elim.size());
    }
  }
  if (!ext) {
    memcpy(hs + o_pose0, pr->poses, sizeof(double) * 7 * P);
    if (L) memcpy(hs + o_point0, pr->points, sizeof(double) * 3 * L);
  }
  // device addresses: the uploaded blob and the scratch behind it (one arena; a batch keeps all blobs together so that
  // ONE copy uploads every window)
  char* base_in = place ? place->in_dev : ws->arena.as<char>();
  char* base_rest = place ? place->rest_dev : base_in + in_bytes;
  auto at = [&](size_t o) -> char* { return o < in_bytes ? base_in + o : base_rest + (o - in_bytes); };
  if (!place) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(base_in, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    // the second state buffer starts as a copy (landmarks without edges are never rewritten)
    if (!ext) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(at(o_pose1), at(o_pose0), sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, ctx->stream));
    if (L)
      SSX_HIP_TRY(ctx, hipMemcpyAsync(at(o_point1), at(o_point0), sizeof(double) * 3 * L, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }

  d.P = P; d.L = L; d.E = E; d.nP = nP; d.nLm = nLm; d.nCh = nCh; d.nBlk = nBlk; d.world = world; d.rank = rank;
  d.big = big ? 1 : 0; d.lin_stride = lin_stride;
  d.dense_slabs = dense_slabs_mode();
  d.touch = (unsigned int*)(at(o_touch));
  d.store_w = 1;                                 // the caller clears it for small windows with analytic Jacobians
  d.pose_free = (const int*)(at(o_pose_free));
  d.lm_fixed = (const uint8_t*)(at(o_lm_fixed));
  d.lm_id = (const int*)(at(o_lm_id));
  d.lm_ptr = (const int*)(at(o_lm_ptr));
  d.ch_lm = (const int*)(at(o_ch_lm));
  d.e_pose = (const int*)(at(o_e_pose));
  d.e_lmc = (const int*)(at(o_e_lmc));
  d.e_cam = (const uint8_t*)(at(o_e_cam));
  d.e_dup = (const uint8_t*)(at(o_e_dup));
  d.e_uv = (const double*)(at(o_e_uv));
  d.ch_desc = (const int4*)(at(o_ch_desc)); d.e_rec = (const int4*)(at(o_e_rec)); d.l_rec = (const int4*)(at(o_l_rec));
  d.blk_pa = (const int8_t*)(at(o_blk_pa));
  d.blk_pb = (const int8_t*)(at(o_blk_pb));
  d.pptr = (const uint16_t*)(at(o_pptr));
  d.pair_a = (uint8_t*)(at(o_pair_a));
  d.pair_b = (uint8_t*)(at(o_pair_b));
  d.pair_ptr = (int*)(at(o_pair_ptr));
  d.bseg = (int4*)(at(o_bseg)); d.bseg_ptr = (int*)(at(o_bseg_ptr));
  d.bseg_cap = bseg_cap;
  d.dev_prep = dev_prep ? 1 : 0;
  d.E_raw = E_raw;
  d.raw_fmt = raw_fmt;
  d.no_err = 0;                                  // (the solve entry points set it when no per-edge errors were asked for)
  if (ext) {
    d.r_edge_pose = ext->r_edge_pose; d.r_edge_point = ext->r_edge_point; d.r_edge_uv = ext->r_edge_uv; d.r_edge_cam = ext->r_edge_cam;
  } else {
  d.r_edge_pose = (const int*)(dev_prep ? at(o_r_pose) : nullptr); d.r_edge_point = (const int*)(dev_prep ? at(o_r_point) : nullptr);
  d.r_edge_uv = (const double*)(dev_prep ? at(o_r_uv) : nullptr); d.r_edge_cam = (const uint8_t*)(have_cam ? at(o_r_cam) : nullptr);
  }
  d.r_slot8 = (const uint8_t*)(dev_prep ? at(o_slot8) : nullptr); d.lm_compact = (const int*)(dev_prep ? at(o_lm_compact) : nullptr);
  d.perm = (int*)(dev_prep ? at(o_perm) : nullptr); d.c2_out = (double*)(dev_prep ? at(o_c2) : nullptr);
  d.pose_rank = (const int*)(have_rank ? at(o_pose_rank) : nullptr);
  d.K = Cam{pr->K[0], pr->K[1], pr->K[2], pr->K[3]};
  for (int i = 0; i < 14; ++i) d.ext[i] = pr->cam_ext[i];
  d.huber_delta = huber_delta; d.chi2_th = chi2_th;
  d.pose_init = keep_init ? (const double*)(at(o_pose_init)) : nullptr;
  d.point_init = keep_init ? (const double*)(at(o_point_init)) : nullptr;
  if (ext) {
    d.pose[0] = ext->pose[0]; d.pose[1] = ext->pose[1]; d.point[0] = ext->point[0]; d.point[1] = ext->point[1];
  } else {
  d.pose[0] = (double*)(at(o_pose0)); d.pose[1] = (double*)(at(o_pose1));
  d.point[0] = (double*)(at(o_point0)); d.point[1] = (double*)(at(o_point1));
  }
  d.W = (double*)(at(o_W));
  d.err_lin = (double*)(at(o_err_lin));
  d.err_trial = (double*)(at(o_err_trial));
  d.Hll = (double*)(at(o_Hll)); d.bl = (double*)(at(o_bl));
  d.lin_slab = (double*)(at(o_lin_slab));
  d.Hpp = (double*)(at(o_Hpp)); d.bp = (double*)(at(o_bp));
  d.iter_comm = (double*)(at(o_iter));
  d.schur_slab = (double*)(at(o_schur));
  d.trial_comm = (double*)(at(o_trial_comm));
  d.xp = (double*)(at(o_xp));
  d.trial_slab = (double*)(at(o_trial));
  d.scal_comm = (double*)(at(o_scal_comm));
  d.scal = (double*)(at(o_scal));
  d.lm_stat = (double*)(at(o_lmstat));
  d.ticket = (unsigned int*)(at(o_ticket));
  if (rz) {                                      // the records, columns and raw arrays of big_records
    d.dev_prep = 1; d.E_raw = recs->E_raw;
    d.pose_free = recs->pose_free; d.lm_fixed = recs->lm_fixed; d.lm_id = recs->lm_id; d.lm_ptr = recs->lm_ptr; d.ch_lm = recs->ch_lm;
    d.e_pose = recs->e_pose; d.e_lmc = recs->e_lmc; d.e_cam = recs->e_cam; d.e_dup = recs->e_dup; d.e_uv = recs->e_uv;
    d.ch_desc = recs->ch_desc; d.e_rec = recs->e_rec; d.l_rec = recs->l_rec; d.perm = recs->perm; d.c2_out = recs->c2_out; d.lm_chunk = recs->lm_chunk;
    d.r_edge_pose = recs->r_edge_pose; d.r_edge_point = recs->r_edge_point; d.r_edge_uv = recs->r_edge_uv; d.r_edge_cam = recs->r_edge_cam;
    d.r_slot8 = recs->r_slot8; d.lm_compact = recs->lm_compact; d.pose_rank = nullptr;
  }
  bd = BigDev{};
  bnd = BandDev{};
  if (big) {
    bd.n = n; bd.n_pad = n_pad; bd.ld = n_pad; bd.T = n_pad / NB; bd.nBlkS = (int)nBlkS;
    bd.pe_ptr = rz ? pe_ptr_dev : (const int*)(at(o_pe_ptr)); bd.pe_edge = rz ? pe_edge_dev : (const int*)(at(o_pe_edge));
    bd.sblk_pa = (const int*)(at(o_sblk_pa)); bd.sblk_pb = (const int*)(at(o_sblk_pb));
    bd.spair_ptr = (const int*)(at(o_spair_ptr)); bd.spair_ab = nullptr;   // the pair lists live in the workspace of build_pairs
    bd.BDa = (double*)(at(o_BDa)); bd.Wma = (double*)(at(o_Wma)); bd.Cv = (double*)(at(o_Cv));
    bnd = BandDev{};
    if (band) {
      bnd.on = 1; bnd.w = bw; bnd.K = bK; bnd.nP = nP; bnd.nPr = bnPr; bnd.wr = bwr;
      bnd.Sb = (double*)(at(o_Sb)); bnd.bsv = bnd.Sb + (size_t)nP * (bw + 1) * 36;
      bnd.seg_p0 = (const int*)(at(o_seg_p0)); bnd.seg_m = (const int*)(at(o_seg_m));
      bnd.U = (double*)(at(o_U)); bnd.Ls0 = (double*)(at(o_Ls0)); bnd.Sr = (double*)(at(o_Sr));
      bnd.Ls1 = (double*)(at(o_Ls1)); bnd.xr = (double*)(at(o_xr)); bnd.LS0 = LS0; bnd.LS1 = LS1;
      bnd.bcr = BcrDev{};
      if (bcr) {
        BcrDev& q = bnd.bcr;
        q.on = 1; q.N = bp.bcr.N; q.m = bp.bcr.m;
        q.p0 = (const int*)(at(o_bcr_p0)); q.elim = (const int4*)(at(o_bcr_elim));
        const size_t mmN = (size_t)q.N * q.m * q.m, mN = (size_t)q.N * q.m;
        double* base = (double*)(at(o_bcr_mem));
        q.D = base; q.E = q.D + mmN; q.DL = q.E + 2 * mmN;   /* E: two buffers, bcr_e_buf */ q.DR = q.DL + mmN; q.Lf = q.DR + mmN; q.Ul = q.Lf + mmN; q.Ur = q.Ul + mmN;
        q.R = q.Ur + mmN; q.RL = q.R + mN; q.RR = q.RL + mN; q.Y = q.RR + mN; q.X = q.Y + mN;
      }
    }
    bd.S = (double*)(at(o_S)); bd.x = (double*)(at(o_x)); bd.Ld = (double*)(at(o_Ld)); bd.invd = (double*)(at(o_invd)); bd.Ninv = (double*)(at(o_Ninv)); bd.scale_part = (double*)(at(o_scale_part));
  }
  if (!place && nCh > 0 && (dev_lists || dev_prep)) {   // (a batch marshals all its windows with one launch pair: batch_build)
    if (dev_prep) {
      hipLaunchKernelGGL(k_prep_scatter, dim3((E_raw + CH - 1) / CH), dim3(CH), 0, ctx->stream, d);
      hipLaunchKernelGGL(k_prep_chunk, dim3(nCh), dim3(CH), 0, ctx->stream, d);
    } else {
      hipLaunchKernelGGL(k_build_lists, dim3(nCh), dim3(CH), 0, ctx->stream, d);
    }
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  return SSX_OK;
}

// Large windows: the non-zero blocks of the reduced system and their pair lists, on the device (kernels in ba_big.inc).
// Fills h.sblk_pa / h.sblk_pb / h.spair_ptr (sorted by (pa, pb); every diagonal block present, possibly with an empty
// list) and h.band_w; the lists themselves stay in the workspace: *ab_dev.
// Large windows, device-side marshalling (HostPrep::dev_prep): the caller's arrays and the host's counting tables go up once
// (25 bytes per observation instead of ~62 of marshalled records and columns, and none of the ~3 ms of host work a
// 480 000-observation window cost), k_prep_scatter / k_prep_chunk build the (landmark, pose) order, the packed records and the
// structure-of-arrays columns, and a stable radix sort by free pose gives the pose-major edge list.  Everything lives in
// ws->recs for the duration of the solve; `r` receives the pointers (the pair builder and upload() take them from there).
// The observation columns as the caller holds them (pose index, landmark index, uv, camera) into pinned staging on the worker
// pool and on their way to the device; nothing here depends on prepare()'s counting, which then runs beside the copy.
ssx_status raw_upload_early(ssx_ctx* ctx, const ssx_ba_problem* pr)
{
  BaWorkspace* ws = ba_workspace(ctx);
  ws->raw_early.valid = false;
  const int E = pr->E;
  if (E <= 0 || !pr->edge_pose || !pr->edge_point || !pr->edge_uv) return SSX_OK;      // (prepare() reports it)
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool have_cam = pr->edge_cam != nullptr;
  Layout in;
  BaWorkspace::RawEarly re;
  re.o_pose = in.take(sizeof(int) * (size_t)(E + 1)); re.o_point = in.take(sizeof(int) * (size_t)(E + 1));
  re.o_uv = in.take(sizeof(double) * 2 * (size_t)(E + 1)); re.o_cam = in.take(have_cam ? (size_t)E + 1 : 0);
  SSX_HIP_TRY(ctx, ws->raw_d.reserve(in.off));
  SSX_HIP_TRY(ctx, ws->raw_h.reserve(in.off));
  char* hs = ws->raw_h.as<char>();
  struct Cp { size_t off; const void* src; size_t n; };
  std::vector<Cp> cps;
  auto add = [&](size_t off, const void* src, size_t n) {
    for (size_t a = 0; a < n; a += (size_t)1 << 20) cps.push_back({off + a, (const char*)src + a, std::min(n - a, (size_t)1 << 20)});
  };
  add(re.o_pose, pr->edge_pose, sizeof(int) * (size_t)E); add(re.o_point, pr->edge_point, sizeof(int) * (size_t)E);
  add(re.o_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
  if (have_cam) add(re.o_cam, pr->edge_cam, (size_t)E);
  ws->pool.run((int)cps.size(), std::min<int>(16, (int)cps.size()), [&](int q) { memcpy(hs + cps[q].off, cps[q].src, cps[q].n); });
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ws->raw_d.p, hs, in.off, hipMemcpyHostToDevice, ctx->stream));
  re.valid = true; re.key = pr->edge_pose; re.E = E;
  ws->raw_early = re;
  return SSX_OK;
}

ssx_status big_records(ssx_ctx* ctx, const ssx_ba_problem* pr, const HostPrep& h, BaDev& r, const int** pe_ptr_dev, const int** pe_edge_dev)
{
  BaWorkspace* ws = ba_workspace(ctx);
  hipStream_t s = ctx->stream;
  const int P = h.P, L = h.L, E = h.E, nP = h.nP, nLm = h.nLm, nCh = h.nCh;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int key_bits = 1;
  while ((1u << key_bits) < (unsigned)(nP + 1)) ++key_bits;
  size_t sort_tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)std::max(E, 1), 0, key_bits, s);
  const bool have_cam = pr->edge_cam != nullptr;
  // (the observation columns may be on the device already: raw_upload_early)
  const BaWorkspace::RawEarly early = ws->raw_early;
  const bool sent = early.valid && early.key == pr->edge_pose && early.E == E && E == h.E_raw;
  ws->raw_early.valid = false;
  Layout in;
  const size_t o_pose_free = in.take(sizeof(int) * P), o_lm_compact = in.take(sizeof(int) * (size_t)(L + 1));
  const size_t o_lm_ptr = in.take(sizeof(int) * (size_t)(nLm + 1)), o_lm_id = in.take(sizeof(int) * (size_t)(nLm + 1)), o_lm_fixed = in.take((size_t)nLm + 1);
  const size_t o_ch_lm = in.take(sizeof(int) * (size_t)(nCh + 1)), o_ch_desc = in.take(sizeof(int) * 4 * (size_t)(nCh + 1)), o_pe_ptr = in.take(sizeof(int) * (size_t)(nP + 1));
  const size_t o_r_pose = in.take(sent ? 0 : sizeof(int) * (size_t)(E + 1)), o_r_point = in.take(sent ? 0 : sizeof(int) * (size_t)(E + 1));
  const size_t o_r_uv = in.take(sent ? 0 : sizeof(double) * 2 * (size_t)(E + 1));
  const size_t o_r_cam = in.take(have_cam && !sent ? (size_t)E + 1 : 0), o_slot8 = in.take((size_t)E + 1);
  const size_t in_bytes = in.off;
  Layout all = in;
  const size_t o_perm = all.take(sizeof(int) * (size_t)(E + 1)), o_e_rec = all.take(sizeof(int) * 4 * (size_t)(E + 1)), o_l_rec = all.take(sizeof(int) * 4 * (size_t)(nLm + 1));
  const size_t o_e_dup = all.take((size_t)E + 1), o_e_uv = all.take(sizeof(double) * 2 * (size_t)(E + 1));
  const size_t o_e_pose = all.take(sizeof(int) * (size_t)(E + 1)), o_e_lmc = all.take(sizeof(int) * (size_t)(E + 1)), o_e_cam = all.take((size_t)E + 1);
  const size_t o_lm_chunk = all.take(sizeof(int) * (size_t)(nLm + 1)), o_pe_edge = all.take(sizeof(int) * (size_t)(E + 1)), o_c2 = all.take(sizeof(double) * (size_t)(E + 1));
  const size_t o_k0 = all.take(sizeof(int) * (size_t)(E + 1)), o_k1 = all.take(sizeof(int) * (size_t)(E + 1)), o_v0 = all.take(sizeof(int) * (size_t)(E + 1));
  const size_t o_tmp = all.take(sort_tmp + 256);
  SSX_HIP_TRY(ctx, ws->recs.reserve(all.off));
  SSX_HIP_TRY(ctx, ws->recs_h.reserve(in_bytes));
  char* hs = ws->recs_h.as<char>();
  char* dv = ws->recs.as<char>();
  memcpy(hs + o_pose_free, h.pose_free.data(), sizeof(int) * P);
  if (L) memcpy(hs + o_lm_compact, h.lm_compact.data(), sizeof(int) * (size_t)L);
  memcpy(hs + o_lm_ptr, h.lm_ptr.data(), sizeof(int) * (size_t)(nLm + 1));
  if (nLm) { memcpy(hs + o_lm_id, h.lm_id.data(), sizeof(int) * (size_t)nLm); memcpy(hs + o_lm_fixed, h.lm_fixed.data(), (size_t)nLm); }
  memcpy(hs + o_ch_lm, h.ch_lm.data(), sizeof(int) * h.ch_lm.size());
  if (nCh) memcpy(hs + o_ch_desc, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
  memcpy(hs + o_pe_ptr, h.pe_ptr.data(), sizeof(int) * (size_t)(nP + 1));
  // the big columns on the worker pool (12 MB at 480 000 observations)
  struct Cp { size_t off; const void* src; size_t n; };
  std::vector<Cp> cps;
  auto add = [&](size_t off, const void* src, size_t n) {
    for (size_t a = 0; a < n; a += (size_t)1 << 20) cps.push_back({off + a, (const char*)src + a, std::min(n - a, (size_t)1 << 20)});
  };
  if (E) {
    if (!sent) {
      add(o_r_pose, pr->edge_pose, sizeof(int) * (size_t)E); add(o_r_point, pr->edge_point, sizeof(int) * (size_t)E);
      add(o_r_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
      if (have_cam) add(o_r_cam, pr->edge_cam, (size_t)E);
    }
    add(o_slot8, h.slot8.data(), (size_t)E);
  }
  ws->pool.run((int)cps.size(), std::min<int>(16, (int)cps.size()), [&](int q) { memcpy(hs + cps[q].off, cps[q].src, cps[q].n); });
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dv, hs, in_bytes, hipMemcpyHostToDevice, s));
  r = BaDev{};
  r.P = P; r.L = L; r.E = E; r.E_raw = h.E_raw; r.nP = nP; r.nLm = nLm; r.nCh = nCh; r.nBlk = 0; r.big = 1; r.dev_prep = 1; r.bseg_cap = 0;
  r.pose_rank = nullptr;
  r.pose_free = (const int*)(dv + o_pose_free); r.lm_compact = (const int*)(dv + o_lm_compact); r.lm_ptr = (const int*)(dv + o_lm_ptr);
  r.lm_id = (const int*)(dv + o_lm_id); r.lm_fixed = (const uint8_t*)(dv + o_lm_fixed); r.ch_lm = (const int*)(dv + o_ch_lm);
  r.ch_desc = (const int4*)(dv + o_ch_desc);
  if (sent) {
    char* rd = ws->raw_d.as<char>();
    r.r_edge_pose = (const int*)(rd + early.o_pose); r.r_edge_point = (const int*)(rd + early.o_point); r.r_edge_uv = (const double*)(rd + early.o_uv);
    r.r_edge_cam = (const uint8_t*)(have_cam ? rd + early.o_cam : nullptr);
  } else {
    r.r_edge_pose = (const int*)(dv + o_r_pose); r.r_edge_point = (const int*)(dv + o_r_point); r.r_edge_uv = (const double*)(dv + o_r_uv);
    r.r_edge_cam = (const uint8_t*)(have_cam ? dv + o_r_cam : nullptr);
  }
  r.r_slot8 = (const uint8_t*)(dv + o_slot8);
  r.perm = (int*)(dv + o_perm); r.e_rec = (const int4*)(dv + o_e_rec); r.l_rec = (const int4*)(dv + o_l_rec); r.e_dup = (const uint8_t*)(dv + o_e_dup);
  r.e_uv = (const double*)(dv + o_e_uv); r.e_pose = (const int*)(dv + o_e_pose); r.e_lmc = (const int*)(dv + o_e_lmc); r.e_cam = (const uint8_t*)(dv + o_e_cam);
  r.lm_chunk = (int*)(dv + o_lm_chunk); r.c2_out = (double*)(dv + o_c2);
  r.pptr = (const uint16_t*)nullptr;
  *pe_ptr_dev = (const int*)(dv + o_pe_ptr);
  *pe_edge_dev = (const int*)(dv + o_pe_edge);
  if (E > 0 && nCh > 0) {
    hipLaunchKernelGGL(k_prep_scatter, dim3((h.E_raw + CH - 1) / CH), dim3(CH), 0, s, r);
    hipLaunchKernelGGL(k_prep_chunk, dim3(nCh), dim3(CH), 0, s, r);
    hipLaunchKernelGGL(k_pe_keys, dim3((E + CH - 1) / CH), dim3(CH), 0, s, r, (unsigned int*)(dv + o_k0), (unsigned int*)(dv + o_v0));
    if (rocprim::radix_sort_pairs(dv + o_tmp, sort_tmp, (unsigned int*)(dv + o_k0), (unsigned int*)(dv + o_k1), (unsigned int*)(dv + o_v0),
                                  (unsigned int*)(dv + o_pe_edge), (size_t)E, 0, key_bits, s) != hipSuccess) {
      ctx->set_error("ssx_ba: rocprim::radix_sort_pairs failed (pose-major edge list)"); return SSX_ERR_HIP;
    }
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  return SSX_OK;
}

// recs (nullable): the records already on the device (big_records)
ssx_status build_pairs(ssx_ctx* ctx, HostPrep& h, const unsigned long long** ab_dev, const BaDev* recs = nullptr)
{
  BaWorkspace* ws = ba_workspace(ctx);
  hipStream_t s = ctx->stream;
  const int nLm = h.nLm, nP = h.nP, E = h.E, nCh = h.nCh;
  *ab_dev = nullptr;
  h.sblk_pa.clear(); h.sblk_pb.clear();
  auto add_diagonals_only = [&] {
    for (int p = 0; p < nP; ++p) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); }
    h.spair_ptr.assign((size_t)nP + 1, 0);
    h.band_w = 0;
  };
  if (nLm == 0 || E == 0) { add_diagonals_only(); return SSX_OK; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // ---- stage A: records in, count + scan
  size_t scan_tmp = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, (int*)nullptr, (int*)nullptr, 0, (size_t)nLm + 1, rocprim::plus<int>(), s);
  Layout la;
  const size_t a_erec = la.take(sizeof(int) * 4 * (size_t)E), a_lrec = la.take(sizeof(int) * 4 * (size_t)nLm), a_cd = la.take(sizeof(int) * 4 * (size_t)nCh);
  const size_t a_lmc = la.take(sizeof(int) * (size_t)nLm);
  const size_t a_in_bytes = la.off;
  const size_t a_cnt = la.take(sizeof(int) * ((size_t)nLm + 1)), a_off = la.take(sizeof(int) * ((size_t)nLm + 1)), a_scal = la.take(64), a_tmp = la.take(scan_tmp + 256);
  SSX_HIP_TRY(ctx, ws->pairs_a.reserve(la.off));
  SSX_HIP_TRY(ctx, ws->pairs_h.reserve(std::max(a_in_bytes, sizeof(int) * 2 * ((size_t)nP * (nP + 1) / 2 + 8))));
  char* da = ws->pairs_a.as<char>();
  char* hh = ws->pairs_h.as<char>();
  if (!recs) {
    memcpy(hh + a_erec, h.e_rec.data(), sizeof(int) * 4 * (size_t)E);
    memcpy(hh + a_lrec, h.l_rec.data(), sizeof(int) * 4 * (size_t)nLm);
    memcpy(hh + a_cd, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
    memcpy(hh + a_lmc, h.lm_chunk.data(), sizeof(int) * (size_t)nLm);
    SSX_HIP_TRY(ctx, hipMemcpyAsync(da, hh, a_in_bytes, hipMemcpyHostToDevice, s));
  }
  SSX_HIP_TRY(ctx, hipMemsetAsync(da + a_cnt, 0, sizeof(int) * ((size_t)nLm + 1), s));
  SSX_HIP_TRY(ctx, hipMemsetAsync(da + a_scal, 0, 64, s));
  const int4* d_erec = recs ? (const int4*)recs->e_rec.p : (const int4*)(da + a_erec);
  const int4* d_lrec = recs ? (const int4*)recs->l_rec.p : (const int4*)(da + a_lrec);
  const int4* d_cd = recs ? (const int4*)recs->ch_desc.p : (const int4*)(da + a_cd);
  const int* d_lmc = recs ? (const int*)recs->lm_chunk.p : (const int*)(da + a_lmc);
  int* d_cnt = (int*)(da + a_cnt); int* d_off = (int*)(da + a_off); int* d_scal = (int*)(da + a_scal);
  hipLaunchKernelGGL(k_pairs_count, dim3((nLm + CH - 1) / CH), dim3(CH), 0, s, d_erec, d_lrec, d_cd, d_lmc, nLm, nP, d_cnt, d_scal);
  if (rocprim::exclusive_scan(da + a_tmp, scan_tmp, d_cnt, d_off, 0, (size_t)nLm + 1, rocprim::plus<int>(), s) != hipSuccess) {
    ctx->set_error("ssx_ba: rocprim::exclusive_scan failed"); return SSX_ERR_HIP;
  }
  int h_np_w[2] = {0, 0};
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&h_np_w[0], d_off + nLm, sizeof(int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&h_np_w[1], d_scal, sizeof(int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  const size_t NP = (size_t)h_np_w[0];
  if (NP == 0) { add_diagonals_only(); return SSX_OK; }
  // ---- stage B: emit, sort by block key, run-length encode
  int key_bits = 1;
  while ((1ull << key_bits) < (unsigned long long)nP * nP) ++key_bits;
  size_t sort_tmp = 0, rle_tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr, NP, 0,
                                  key_bits, s);
  (void)rocprim::run_length_encode(nullptr, rle_tmp, (unsigned int*)nullptr, (unsigned int)NP, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, s);
  const size_t max_blk = std::min((size_t)nP * (nP + 1) / 2, NP);
  Layout lb;
  const size_t b_k0 = lb.take(sizeof(unsigned int) * NP), b_k1 = lb.take(sizeof(unsigned int) * NP), b_v0 = lb.take(sizeof(unsigned long long) * NP);
  const size_t b_uq = lb.take(sizeof(unsigned int) * (max_blk + 1)), b_ct = lb.take(sizeof(unsigned int) * (max_blk + 1)), b_nr = lb.take(64);
  const size_t b_tmp = lb.take(std::max(sort_tmp, rle_tmp) + 256);
  SSX_HIP_TRY(ctx, ws->pairs_b.reserve(lb.off));
  SSX_HIP_TRY(ctx, ws->pairs_c.reserve(sizeof(unsigned long long) * NP + 64));
  char* db = ws->pairs_b.as<char>();
  unsigned int* d_k0 = (unsigned int*)(db + b_k0); unsigned int* d_k1 = (unsigned int*)(db + b_k1);
  unsigned long long* d_v0 = (unsigned long long*)(db + b_v0);
  unsigned long long* d_v1 = ws->pairs_c.as<unsigned long long>();   // the sorted values = the final lists
  unsigned int* d_uq = (unsigned int*)(db + b_uq); unsigned int* d_ct = (unsigned int*)(db + b_ct); unsigned int* d_nr = (unsigned int*)(db + b_nr);
  hipLaunchKernelGGL(k_pairs_emit, dim3((nLm + CH - 1) / CH), dim3(CH), 0, s, d_erec, d_lrec, d_cd, d_lmc, nLm, nP, (const int*)d_off, d_k0, d_v0);
  if (rocprim::radix_sort_pairs(db + b_tmp, sort_tmp, d_k0, d_k1, d_v0, d_v1, NP, 0, key_bits, s) != hipSuccess ||
      rocprim::run_length_encode(db + b_tmp, rle_tmp, d_k1, (unsigned int)NP, d_uq, d_ct, d_nr, s) != hipSuccess) {
    ctx->set_error("ssx_ba: rocprim radix_sort_pairs / run_length_encode failed"); return SSX_ERR_HIP;
  }
  unsigned int n_runs = 0;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&n_runs, d_nr, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  unsigned int* h_uq = reinterpret_cast<unsigned int*>(hh);
  unsigned int* h_ct = h_uq + n_runs;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(h_uq, d_uq, sizeof(unsigned int) * n_runs, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(h_ct, d_ct, sizeof(unsigned int) * n_runs, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  // ---- the block list: the runs (sorted by key) merged with the diagonal blocks that have no pair (a pose whose
  // landmarks are all fixed still owns its Hpp block)
  h.spair_ptr.clear(); h.spair_ptr.push_back(0);
  unsigned int r = 0;
  int run_sum = 0;
  for (int p = 0; p < nP; ++p) {
    const unsigned int diag = (unsigned int)p * nP + p;
    bool have_diag = false;
    while (r < n_runs && h_uq[r] / (unsigned int)nP == (unsigned int)p) {      // the blocks of block-row p, ascending pb
      if (h_uq[r] > diag && !have_diag) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); h.spair_ptr.push_back(run_sum); have_diag = true; }
      if (h_uq[r] == diag) have_diag = true;
      h.sblk_pa.push_back(p); h.sblk_pb.push_back((int)(h_uq[r] % (unsigned int)nP));
      run_sum += (int)h_ct[r];
      h.spair_ptr.push_back(run_sum);
      ++r;
    }
    if (!have_diag) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); h.spair_ptr.push_back(run_sum); }
  }
  h.band_w = h_np_w[1];
  *ab_dev = d_v1;
  return SSX_OK;
}
