// ssvio_amd/csrc/ba_marshal.inc -- host marshalling of a bundle adjustment window (included by ba.hip after BaWorkspace): prepare() as a
// sequence of passes (the tests' host reference builders apart), the plan of the band solver, the arena as plan / fill / wire and its
// upload, a large window's device-built records and pairs.

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

// ---- prepare(): the passes of the production path, in the order prepare() runs them ----

// validation, and the index of the free poses (a window: in the order of its keyframe ids, WinExt::pose_order)
ssx_status prep_free_poses(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, const WinExt* ext)
{
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
  return SSX_OK;
}

// The one pass over the observations, serial: edges per landmark (cnt_tmp), the rank of an edge inside its landmark (slot8), the
// first free pose of every landmark (first_pf_tmp), edges per free pose of a device-marshalled large window (pe_ptr).
ssx_status prep_count_serial(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, bool dead_ok, bool big_dev, int& n_dead)
{
  const int P = h.P, L = h.L;
  std::vector<int>& cnt = h.cnt_tmp;
  std::vector<int>& first_pf = h.first_pf_tmp;
  for (int e = 0; e < h.E_raw; ++e) {
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
  return SSX_OK;
}

// The same tables on T threads of the worker pool, for a large window (480 000 observations at BASELINE configs[3]: 1.05 ms on one
// core, a sixth of a 10-iteration solve): every thread counts its range into tables of its own (slot8 = the rank inside the range), the
// per-landmark offsets of the ranges are summed landmark-parallel, a second pass adds them -- the same ranks as the serial loop,
// whatever the number of threads.
ssx_status prep_count_pool(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, int T)
{
  const int P = h.P, L = h.L, E = h.E_raw;
  std::vector<int>& cnt = h.cnt_tmp;
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
  return SSX_OK;
}

// Lossless narrowing of the raw arrays on their way across PCIe (26 -> 13 bytes per observation): pose indices as bytes,
// landmark indices as 16-bit words, and the pixel coordinates as floats when every one of them IS a float's value -- the
// reference's measurements are cv::KeyPoint::pt (Point2f) widened to double (frontend.cpp:232-236, backend.cpp:126-160).
void prep_raw_format(const ssx_ba_problem* pr, HostPrep& h, bool dead_ok)
{
  h.raw_fmt = 0;
  if (!(h.dev_prep && !h.big && !dead_ok)) return;
  if (h.P <= 256) h.raw_fmt |= 1;
  if (h.L <= 65536) h.raw_fmt |= 2;
  bool exact = true;
  const double* uvp = pr->edge_uv;
  for (size_t i = 0; i < 2 * (size_t)h.E_raw; ++i) exact &= (double)(float)uvp[i] == uvp[i];
  if (exact) h.raw_fmt |= 4;
}

// The compact order of the landmarks: the caller's order (a window: ascending ids), then -- stable -- by the FIRST free pose that
// observes a landmark.  Map points are created keyframe by keyframe, so real windows arrive almost sorted already; what the
// sort buys is locality for every input: the landmarks of a chunk then share their poses, a chunk contributes to 15-25 of the
// 55 blocks of a 10-keyframe reduced system instead of all of them, and writes / the reductions read only those (BaDev::touch).
ssx_status prep_landmark_order(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, const WinExt* ext)
{
  const int L = h.L;
  const std::vector<int>& cnt = h.cnt_tmp;
  const std::vector<int>& first_pf = h.first_pf_tmp;
  h.lm_id.clear(); h.lm_ptr.clear(); h.lm_fixed.clear();
  h.lm_compact.assign(L, -1); h.start_tmp.assign(L + 1, 0);
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
    h.lm_compact[l] = (int)h.lm_id.size();
    h.lm_id.push_back(l);
    h.lm_ptr.push_back(run);
    run += cnt[l + 1];
    h.lm_fixed.push_back(pr->point_fixed ? (pr->point_fixed[l] ? 1 : 0) : 0);
  }
  if (run != h.E) { ctx->set_error("ssx_ba_window: an observation refers to a landmark that is not in the window's order list"); return SSX_ERR_INVALID_ARG; }
  h.lm_ptr.push_back(h.E);
  h.nLm = (int)h.lm_id.size();
  return SSX_OK;
}

// the chunk cut and the chunk descriptors (first edge, edges, first landmark, landmarks)
void prep_chunks(HostPrep& h)
{
  make_chunks(h);
  h.ch_desc.resize(4 * (size_t)std::max(h.nCh, 1));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
    int* cd = &h.ch_desc[4 * (size_t)c];
    cd[0] = e0; cd[1] = e1 - e0; cd[2] = lm0; cd[3] = lm1 - lm0;
  }
}

// a device-marshalled window hands on nothing of what the device builds: the host reference's arrays of an earlier call are dropped
void prep_drop_reference(HostPrep& h)
{
  h.blk_pa.clear(); h.blk_pb.clear();
  h.band_w = -1;
  h.perm.clear(); h.pptr.clear(); h.pair_ptr.clear(); h.pair_a.clear(); h.pair_b.clear(); h.bseg.clear(); h.bseg_ptr.clear();
  h.pe_edge.clear(); h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
}

// small window: every block (a <= b) of the reduced system, row by row
void prep_small_blocks(HostPrep& h)
{
  h.blk_pa.clear(); h.blk_pb.clear();
  for (int a = 0; a < h.nP; ++a)
    for (int b = a; b < h.nP; ++b) { h.blk_pa.push_back((int8_t)a); h.blk_pb.push_back((int8_t)b); }
  h.nBlk = (int)h.blk_pa.size();
}

void ref_pose_major(HostPrep& h);   // (the host reference's, below)
// large window: the pose-major offsets (the edge list itself is the device's, big_records; the host reference builds its own); the
// non-zero blocks of the reduced system and their (edge, edge) pair lists are built on the device (build_pairs)
ssx_status prep_big_tail(ssx_ctx* ctx, HostPrep& h)
{
  if (h.nP > 2048) { ctx->set_error("ssx_ba: %d free poses exceed the supported 2048", h.nP); return SSX_ERR_UNSUPPORTED; }
  if (h.dev_prep) for (int p = 0; p < h.nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];   // counts -> offsets
  else ref_pose_major(h);
  h.blk_pa.clear(); h.blk_pb.clear();
  h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
  h.nBlk = 0;
  h.band_w = -1;
  h.bseg.clear(); h.bseg_ptr.clear();
  h.dev_lists = false;
  return SSX_OK;
}

// ---- the host reference of the tests (SSX_BA_HOST_PREP / SSX_BA_HOST_LISTS, ssx_ba_linearize): what the device builds from the light
// tables, built here; same bits (test_device_marshalling_equals_host_marshalling, test_device_built_lists_equal_host_built_lists).
// The production path runs none of the ref_* functions. ----

// reference: edges sorted by (landmark, pose), the sorted columns, duplicates of a (landmark, pose) pair marked
void ref_sort_columns(const ssx_ba_problem* pr, HostPrep& h)
{
  const int L = h.L, E = h.E;
  h.perm.assign(E, 0);
  {
    std::vector<int> fill((size_t)L, 0);
    for (int l = 0; l < L; ++l) if (h.lm_compact[l] >= 0) fill[l] = h.lm_ptr[h.lm_compact[l]];
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
    h.e_lmc[s] = h.lm_compact[pr->edge_point[e]];
    h.e_cam[s] = pr->edge_cam ? (pr->edge_cam[e] ? 1 : 0) : 0;
    h.e_uv[s] = pr->edge_uv[2 * (size_t)e];
    h.e_uv[(size_t)E + s] = pr->edge_uv[2 * (size_t)e + 1];
    if (s > 0 && h.e_lmc[s] == h.e_lmc[s - 1] && h.e_pose[s] == h.e_pose[s - 1]) h.e_dup[s] = 1;
  }
}

// reference: the packed landmark and edge records of every chunk (what k_prep_chunk writes)
void ref_records(HostPrep& h)
{
  h.e_rec.resize(4 * (size_t)std::max(h.E, 1)); h.l_rec.resize(4 * (size_t)std::max(h.nLm, 1));
  h.lm_chunk.resize((size_t)std::max(h.nLm, 1));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0];
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
}

// reference, large window: the pose-major edge list (free poses)
void ref_pose_major(HostPrep& h)
{
  const int nP = h.nP, E = h.E;
  h.pe_ptr.assign(nP + 1, 0);
  for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_ptr[pf + 1]++; }
  for (int p = 0; p < nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];
  h.pe_edge.assign(std::max(h.pe_ptr[nP], 1), 0);
  std::vector<int> fill(h.pe_ptr.begin(), h.pe_ptr.end() - 1);
  for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_edge[fill[pf]++] = s; }
}

// reference, small window: the per-chunk index lists -- edges grouped by free pose; with build_lists (SSX_BA_HOST_LISTS) also the
// leader pairs grouped by reduced-system block, the work items of the block phase and the touch masks (what k_build_lists writes)
void ref_chunk_lists(HostPrep& h, bool build_lists)
{
  h.dev_lists = !build_lists;
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
}

// The host marshalling of one window.  allow_dev_prep: everything beyond counting is left to the device (see HostPrep::dev_prep);
// without it, or with SSX_BA_HOST_PREP / SSX_BA_HOST_LISTS in the environment, the host reference above builds the same arrays.
ssx_status prepare(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, bool allow_dev_prep = true, const WinExt* ext = nullptr)
{
  const bool dead_ok = ext != nullptr;
  SSX_TRY(prep_free_poses(ctx, pr, h, ext));
  const int L = h.L, E = h.E_raw;
  static const bool host_prep_env = getenv("SSX_BA_HOST_PREP") != nullptr;
  static const bool host_lists_env = getenv("SSX_BA_HOST_LISTS") != nullptr;
  h.big = h.nP > SSX_BA_SMALL_P;
  h.dev_prep = allow_dev_prep && !host_prep_env && !host_lists_env;
  const bool big_dev = h.big && h.dev_prep;               // large window, device-marshalled: the host also counts edges per free pose
  h.cnt_tmp.assign(L + 1, 0);
  h.first_pf_tmp.assign((size_t)L + 1, h.nP + 1);
  if (h.dev_prep) h.slot8.resize((size_t)std::max(E, 1));
  if (big_dev) h.pe_ptr.assign((size_t)h.nP + 1, 0);
  static const int prep_threads = [] { const char* e = getenv("SSX_BA_PREP_THREADS"); const int v = e ? atoi(e) : 0;
                                       return v > 0 ? std::min(v, 32) : std::min(32, std::max(std::min(8, std::max(1, (int)std::thread::hardware_concurrency())), (int)std::thread::hardware_concurrency() / 2)); }();   // (measured at configs[3] on a 256-core host: 1.70 / 1.27 / 0.74 ms of prepare() on 8 / 16 / 32 threads, profiles/r06/c4_prepare_threads.txt)
  const int T = (big_dev && !dead_ok && E >= (1 << 16) && ctx->ba) ? (g_prep_threads_override > 0 ? g_prep_threads_override : prep_threads) : 1;
  int n_dead = 0;
  SSX_TRY(T > 1 ? prep_count_pool(ctx, pr, h, T) : prep_count_serial(ctx, pr, h, dead_ok, big_dev, n_dead));
  if (n_dead && !h.dev_prep) { ctx->set_error("ssx_ba: dead observations need the device-side marshalling"); return SSX_ERR_UNSUPPORTED; }
  h.E = E - n_dead;
  prep_raw_format(pr, h, dead_ok);
  SSX_TRY(prep_landmark_order(ctx, pr, h, ext));
  if (h.dev_prep) prep_drop_reference(h); else ref_sort_columns(pr, h);
  prep_chunks(h);
  if (!h.dev_prep) ref_records(h);
  if (h.big) return prep_big_tail(ctx, h);
  prep_small_blocks(h);
  if (h.dev_prep) { h.pe_ptr.clear(); h.dev_lists = true; }
  else ref_chunk_lists(h, host_lists_env);
  return SSX_OK;
}

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

// ---- the arena of one window: plan (arithmetic), fill (the host blob), wire (device pointers) ----

struct Span { size_t off = 0, n = 0; };   // a buffer of the arena: its offset, and the bytes fill_blob() copies there (0: nothing travels)

// Where every buffer of a window lives: [uploaded blob | scratch], each buffer rounded to 256 bytes.  The ORDER OF THE SPANS IS THE
// MEMORY LAYOUT (a buffer that is uploaded when the host built it and scratch when the device builds it is declared at its place
// in the blob).  A buffer that does not exist has n == 0 and an offset nobody reads through.
struct ArenaPlan {
  int P, L, E, E_raw, nP, nLm, nCh, nBlk, nBlkS, n, n_pad, lin_stride, bseg_cap, raw_fmt;
  int bw, bK, bnPr, bwr, LS0, LS1, bcrN, bcrm;   // band solver (BandPlan)
  // every condition of the layout, named once
  bool big;          // large window (> SSX_BA_SMALL_P free poses)
  bool on_dev;       // large window whose records, columns and raw arrays already live on the device (big_records)
  bool dev_prep;     // small window marshalled by k_prep_scatter / k_prep_chunk: records and columns are scratch
  bool dev_lists;    // small window whose pair lists and work items k_build_lists / k_prep_chunk builds: they are scratch
  bool host_recs;    // host records and sorted columns travel in the blob
  bool ext;          // an ssx_ba_window: raw arrays and state live in buffers of its own (WinExt)
  bool raw_in;       // the caller's raw arrays travel in the blob
  bool cam_in;       // ... with a camera column
  bool have_rank;    // a window's keyframe order travels (BaDev::pose_rank)
  bool keep_init;    // a resident batch keeps a pristine copy of the uploaded state
  bool band, bcr;    // large window on the band solver / its block cyclic reduction
  size_t in_bytes, total;
  Span pose_free, lm_fixed, lm_id, lm_ptr, ch_lm, e_pose, e_lmc, e_cam, e_dup, e_uv, ch_desc, e_rec, l_rec, blk_pa, blk_pb, pptr, lm_compact, pose_rank,
       r_pose, r_point, r_uv, r_cam, slot8, pair_a, pair_b, pair_ptr, bseg, bseg_ptr, touch, pe_ptr, pe_edge, sblk_pa, sblk_pb, spair_ptr, seg_p0, seg_m,
       bcr_p0, bcr_elim, pose0, point0,                                                                                       // <- in_bytes
       pose1, point1, pose_init, point_init, perm, c2, W, err_lin, err_trial, Hll, bl, lin_slab, Hpp, bp, iter, schur, trial_comm, BDa, Wma, Cv, S, Sb,
       U, Ls0, Sr, Ls1, bcr_mem, xr, x, Ld, invd, Ninv, scale_part, xp, trial, scal_comm, scal, lmstat, ticket;
  const Span* spans_begin() const { return &pose_free; }
  const Span* spans_end() const { return &ticket + 1; }
};
static_assert(offsetof(ArenaPlan, ticket) - offsetof(ArenaPlan, pose_free) == 78 * sizeof(Span), "ArenaPlan: the spans are one run of 79 Span members");

// The layout of a window.  batch: one of a batch's windows (the second state buffer is then made by k_dup_state_b; keep_init: and a
// pristine copy for a resident batch); on_dev: see ArenaPlan.  Arithmetic only.
ArenaPlan plan_arena(const ssx_ba_problem* pr, const HostPrep& h, const BandPlan& bp, int world, bool keep_init, const WinExt* ext, bool on_dev)
{
  ArenaPlan p{};
  const int P = p.P = h.P, L = p.L = h.L, E = p.E = h.E, nP = p.nP = h.nP, nLm = p.nLm = h.nLm, nCh = p.nCh = h.nCh, nBlk = p.nBlk = h.nBlk;
  const int E_raw = p.E_raw = h.E_raw, n = p.n = 6 * nP;
  const bool big = p.big = h.big, rz = p.on_dev = on_dev;
  const bool dev_prep = p.dev_prep = h.dev_prep && !big, dev_lists = p.dev_lists = h.dev_lists && !big;
  const bool host_recs = p.host_recs = !dev_prep && !rz, host_lists = !dev_lists;
  const bool big_up = big && !rz;                // a large window's tables and columns travel in the blob
  const bool lm_up = (big || dev_prep) && !rz;   // the landmark tables travel (the small-window kernels take everything from the packed
                                                 // records -- a quarter of a C3 window's blob not staged, not sent -- unless the device packs them)
  p.ext = ext != nullptr;
  const bool raw_in = p.raw_in = dev_prep && !ext;
  p.cam_in = raw_in && pr->edge_cam != nullptr;
  p.have_rank = dev_prep && !h.pose_rank.empty();
  p.keep_init = keep_init && !ext;
  const bool band = p.band = big && bp.w > 0, bcr = p.bcr = band && bp.bcr.on;
  p.bseg_cap = dev_lists ? 2 * nBlk * BSEG_PARTS + 16 : 0;
  p.lin_stride = big ? 2 : nP * 27 + 2;
  const int n_pad = p.n_pad = big ? ((n + NB - 1) / NB) * NB : 0;
  const size_t nBlkS = h.sblk_pa.size();
  p.nBlkS = (int)nBlkS;
  const int raw_fmt = p.raw_fmt = raw_in ? h.raw_fmt : 0;
  const size_t I = sizeof(int), D = sizeof(double);
  Layout lay;
  // a buffer of the blob: n bytes that fill_blob() copies (when `filled`) + pad bytes of slack, or nothing
  auto blob = [&](bool on, size_t nbytes, size_t pad = 0, bool filled = true) { return Span{lay.take(on ? nbytes + pad : 0), on && filled ? nbytes : 0}; };
  auto scratch = [&](size_t nbytes) { return Span{lay.take(nbytes), 0}; };
  p.pose_free = blob(!rz, I * P);
  p.lm_fixed = blob(lm_up, nLm); p.lm_id = blob(lm_up, I * nLm); p.lm_ptr = blob(lm_up, I * (nLm + 1));
  p.ch_lm = blob(big_up, I * (nCh + 1));
  p.e_pose = blob(big_up, I * E); p.e_lmc = blob(big_up, I * E); p.e_cam = blob(big_up, E);
  // (device-marshalled windows upload the caller's arrays; the sorted columns / records are scratch, written by k_prep_chunk)
  if (host_recs) { p.e_dup = blob(true, E); p.e_uv = blob(true, D * 2 * E); }
  p.ch_desc = blob(!rz, I * 4 * (size_t)nCh, I * 4);
  if (host_recs) { p.e_rec = blob(true, I * 4 * (size_t)E, I * 4); p.l_rec = blob(true, I * 4 * (size_t)nLm, I * 4); }
  p.blk_pa = blob(true, nBlk, 1); p.blk_pb = blob(true, nBlk, 1);
  if (host_recs) p.pptr = blob(true, sizeof(uint16_t) * h.pptr.size(), sizeof(uint16_t));
  p.lm_compact = blob(dev_prep, I * (size_t)L, I);
  p.pose_rank = blob(p.have_rank, I * (size_t)P);
  { const size_t wp = (raw_fmt & 1) ? 1 : I, wl = (raw_fmt & 2) ? sizeof(uint16_t) : I, wuv = 2 * ((raw_fmt & 4) ? sizeof(float) : D);
    p.r_pose = blob(raw_in, wp * E, wp); p.r_point = blob(raw_in, wl * E, wl); p.r_uv = blob(raw_in, wuv * E, wuv); }
  p.r_cam = blob(p.cam_in, E, 1);
  p.slot8 = blob(dev_prep, E_raw, 1);
  // (host-built lists travel with the blob; device-built ones are scratch behind it, a fixed capacity per chunk)
  const size_t touch_bytes = big ? 0 : sizeof(unsigned int) * TOUCH_WORDS * (size_t)(nCh + 1);
  if (host_lists) {
    p.pair_a = blob(true, h.pair_a.size(), 1); p.pair_b = blob(true, h.pair_a.size(), 1);
    p.pair_ptr = blob(true, I * h.pair_ptr.size(), I); p.bseg = blob(true, I * h.bseg.size(), I * 4); p.bseg_ptr = blob(true, I * h.bseg_ptr.size(), I);
    if (!big) p.touch = blob(true, touch_bytes);
  }
  p.pe_ptr = blob(!rz, I * h.pe_ptr.size(), I, big); p.pe_edge = blob(!rz, I * h.pe_edge.size(), I, big);
  p.sblk_pa = blob(true, I * nBlkS, I, big); p.sblk_pb = blob(true, I * nBlkS, I, big); p.spair_ptr = blob(true, I * h.spair_ptr.size(), I, big);
  p.seg_p0 = blob(true, I * bp.seg_p0.size(), I, band); p.seg_m = blob(true, I * bp.seg_m.size(), I, band);
  p.bcr_p0 = blob(bcr, I * bp.bcr.p0.size(), I); p.bcr_elim = blob(bcr, I * bp.bcr.elim.size(), I * 4);
  p.pose0 = blob(!ext, D * 7 * P); p.point0 = blob(!ext, D * 3 * L, D * 3);
  // (the state crosses PCIe ONCE: the second buffer and, for a resident batch, the pristine copy are made on the device,
  // k_dup_state_b -- the blob of a C3 window carried three copies of its 96 KB of landmarks)
  p.in_bytes = lay.off;
  if (!ext) { p.pose1 = scratch(D * 7 * P); p.point1 = scratch(D * 3 * (L + 1)); }
  if (p.keep_init) { p.pose_init = scratch(D * 7 * P); p.point_init = scratch(D * 3 * (L + 1)); }
  if (dev_prep) {
    p.e_dup = scratch((size_t)E + 1); p.e_uv = scratch(D * 2 * (size_t)(E + 1));
    p.e_rec = scratch(I * 4 * (size_t)(E + 1)); p.l_rec = scratch(I * 4 * (size_t)(nLm + 1));
    p.pptr = scratch(sizeof(uint16_t) * ((size_t)(nCh + 1) * (nP + 1) + 1));
    p.perm = scratch(I * (size_t)(E + 1)); p.c2 = scratch(D * (size_t)(E_raw + 1));
  }
  if (dev_lists) {
    p.pair_a = scratch((size_t)(nCh + 1) * MAX_PAIRS); p.pair_b = scratch((size_t)(nCh + 1) * MAX_PAIRS);
    p.pair_ptr = scratch(I * ((size_t)(nCh + 1) * (nBlk + 1) + 1));
    p.bseg = scratch(I * 4 * ((size_t)(nCh + 1) * p.bseg_cap + 1)); p.bseg_ptr = scratch(I * (2 * (size_t)nCh + 2));
    p.touch = scratch(touch_bytes);
  }
  p.W = scratch(D * 18 * (size_t)E); p.err_lin = scratch(D * 2 * (size_t)E); p.err_trial = scratch(D * 2 * (size_t)E);
  p.Hll = scratch(D * 6 * (size_t)nLm); p.bl = scratch(D * 3 * (size_t)nLm);
  p.lin_slab = scratch(D * (size_t)(nCh + 1) * p.lin_stride);
  p.Hpp = scratch(D * (nP + 1) * UPPER6); p.bp = scratch(D * (nP + 1) * 6);
  // (band solver: iter_comm sits right behind [band | rhs] so that ONE all-reduce per trial carries the reduced system AND the
  // linearisation's pose blocks / chi2 -- see big_trial)
  const size_t iter_count = (size_t)nP * 27 + 1 + world;
  if (!band) p.iter = scratch(D * (iter_count + 1));
  p.schur = scratch(big ? 256 : D * (size_t)(nCh + 1) * (nBlk * 36 + nP * 6));
  p.trial_comm = scratch(big ? 256 : D * ((size_t)n * n + n + 1));
  p.BDa = scratch(big ? D * 18 * (size_t)(E + 1) : 256); p.Wma = scratch(big ? D * 18 * (size_t)(E + 1) : 256); p.Cv = scratch(big ? D * 6 * (size_t)(E + 1) : 256);
  p.S = scratch((big && !band) ? D * (size_t)(n_pad + NB) * n_pad : 256);
  // band solver: band + rhs, segment updates, factors of both levels, the separator system
  const int bw = p.bw = bp.w, bK = p.bK = bp.K, bnPr = p.bnPr = bK * bw, bwr = p.bwr = 2 * bw - 1;
  const int NW0 = 6 * (2 * bw + 1) + 1, w1 = bK == 1 ? bw : bwr, NW1 = 6 * (w1 + 1 + bw) + 1, NU = 12 * bw + 1;
  p.LS0 = 36 + NW0 * 6; p.LS1 = 36 + NW1 * 6;
  p.bcrN = bp.bcr.N; p.bcrm = bp.bcr.m;
  const size_t sb_count = band ? band_rhs_doubles(nP, bw) : 0;
  const size_t sr_count = (band && bK > 1) ? (size_t)bnPr * (bwr + 1) * 36 + 6 * (size_t)bnPr : 0;
  p.Sb = scratch(D * (sb_count + 1 + (band ? iter_count + 1 : 0)));
  if (band) p.iter = Span{p.Sb.off + D * sb_count, 0};
  p.U = scratch(band ? D * (size_t)bK * NU * NU : 256);
  p.Ls0 = scratch((band && bK > 1) ? D * (size_t)nP * p.LS0 : 256);
  p.Sr = scratch(D * (sr_count + 1));
  p.Ls1 = scratch(band ? D * (size_t)(bK > 1 ? bnPr : nP) * p.LS1 : 256);
  p.bcr_mem = scratch(bcr ? D * (bcr_mem_doubles(p.bcrN, p.bcrm) + 8) : 256);
  p.xr = scratch(D * (6 * (size_t)bnPr + 8)); p.x = scratch(D * (n_pad + 8)); p.Ld = scratch(D * NB * NB); p.invd = scratch(D * (n_pad + 8));
  p.Ninv = scratch(D * 4 * 256); p.scale_part = scratch(D * 64); p.xp = scratch(D * (n + 1)); p.trial = scratch(D * 3 * (nCh + 1));
  p.scal_comm = scratch(D * 4); p.scal = scratch(D * SC_N); p.lmstat = scratch(D * 3 * SSX_BA_MAX_STATS); p.ticket = scratch(sizeof(unsigned int) * 4);
  p.total = lay.off;
  return p;
}

// the input blob of a window into hs (pinned staging, p.in_bytes of it); a span of zero planned bytes is skipped
void fill_blob(const ArenaPlan& p, const ssx_ba_problem* pr, const HostPrep& h, const BandPlan& bp, char* hs)
{
  auto put = [&](const Span& s, const void* src) { if (s.n) memcpy(hs + s.off, src, s.n); };
  put(p.pose_free, h.pose_free.data());
  put(p.lm_fixed, h.lm_fixed.data()); put(p.lm_id, h.lm_id.data()); put(p.lm_ptr, h.lm_ptr.data());
  put(p.ch_lm, h.ch_lm.data());
  put(p.e_pose, h.e_pose.data()); put(p.e_lmc, h.e_lmc.data()); put(p.e_cam, h.e_cam.data());
  put(p.e_dup, h.e_dup.data()); put(p.e_uv, h.e_uv.data());
  put(p.ch_desc, h.ch_desc.data()); put(p.e_rec, h.e_rec.data()); put(p.l_rec, h.l_rec.data());
  put(p.blk_pa, h.blk_pa.data()); put(p.blk_pb, h.blk_pb.data());
  put(p.pptr, h.pptr.data());
  put(p.lm_compact, h.lm_compact.data()); put(p.pose_rank, h.pose_rank.data());
  if (p.r_pose.n && (p.raw_fmt & 1)) { uint8_t* o = (uint8_t*)(hs + p.r_pose.off); for (int e = 0; e < p.E; ++e) o[e] = (uint8_t)pr->edge_pose[e]; }
  else put(p.r_pose, pr->edge_pose);
  if (p.r_point.n && (p.raw_fmt & 2)) { uint16_t* o = (uint16_t*)(hs + p.r_point.off); for (int e = 0; e < p.E; ++e) o[e] = (uint16_t)pr->edge_point[e]; }
  else put(p.r_point, pr->edge_point);
  if (p.r_uv.n && (p.raw_fmt & 4)) { float* o = (float*)(hs + p.r_uv.off); for (size_t i = 0; i < 2 * (size_t)p.E; ++i) o[i] = (float)pr->edge_uv[i]; }
  else put(p.r_uv, pr->edge_uv);
  put(p.r_cam, pr->edge_cam);
  put(p.slot8, h.slot8.data());
  put(p.pair_a, h.pair_a.data()); put(p.pair_b, h.pair_b.data()); put(p.pair_ptr, h.pair_ptr.data());
  put(p.bseg, h.bseg.data()); put(p.bseg_ptr, h.bseg_ptr.data()); put(p.touch, h.touch.data());
  put(p.pe_ptr, h.pe_ptr.data()); put(p.pe_edge, h.pe_edge.data());
  put(p.sblk_pa, h.sblk_pa.data()); put(p.sblk_pb, h.sblk_pb.data()); put(p.spair_ptr, h.spair_ptr.data());
  put(p.seg_p0, bp.seg_p0.data()); put(p.seg_m, bp.seg_m.data());
  put(p.bcr_p0, bp.bcr.p0.data()); put(p.bcr_elim, bp.bcr.elim.data());
  put(p.pose0, pr->poses); put(p.point0, pr->points);
}

// The solve's view of a planned arena: base_in is the uploaded blob on the device, base_rest the scratch behind it (one arena; a
// batch keeps all blobs together so that ONE copy uploads every window).  recs (nullable): the records, columns and raw arrays of
// big_records, with its pose-major list pe_ptr_dev / pe_edge_dev.
void wire_arena(const ArenaPlan& p, char* base_in, char* base_rest, const ssx_ba_problem* pr, double huber_delta, double chi2_th, int world, int rank,
                const WinExt* ext, const BaDev* recs, const int* pe_ptr_dev, const int* pe_edge_dev, BaDev& d, BigDev& bd, BandDev& bnd)
{
  auto at = [&](const Span& s) -> char* { return s.off < p.in_bytes ? base_in + s.off : base_rest + (s.off - p.in_bytes); };
  auto at_if = [&](bool on, const Span& s) -> char* { return on ? at(s) : nullptr; };
  d.P = p.P; d.L = p.L; d.E = p.E; d.nP = p.nP; d.nLm = p.nLm; d.nCh = p.nCh; d.nBlk = p.nBlk; d.world = world; d.rank = rank;
  d.big = p.big ? 1 : 0; d.lin_stride = p.lin_stride;
  d.dense_slabs = dense_slabs_mode();
  d.touch = (unsigned int*)at(p.touch);
  d.store_w = 1;                                 // the caller clears it for small windows with analytic Jacobians
  d.pose_free = (const int*)at(p.pose_free); d.ch_lm = (const int*)at(p.ch_lm);
  d.lm_fixed = (const uint8_t*)at(p.lm_fixed); d.lm_id = (const int*)at(p.lm_id); d.lm_ptr = (const int*)at(p.lm_ptr);
  d.e_pose = (const int*)at(p.e_pose); d.e_lmc = (const int*)at(p.e_lmc); d.e_cam = (const uint8_t*)at(p.e_cam);
  d.e_dup = (const uint8_t*)at(p.e_dup); d.e_uv = (const double*)at(p.e_uv);
  d.ch_desc = (const int4*)at(p.ch_desc); d.e_rec = (const int4*)at(p.e_rec); d.l_rec = (const int4*)at(p.l_rec);
  d.blk_pa = (const int8_t*)at(p.blk_pa); d.blk_pb = (const int8_t*)at(p.blk_pb); d.pptr = (const uint16_t*)at(p.pptr);
  d.pair_a = (uint8_t*)at(p.pair_a); d.pair_b = (uint8_t*)at(p.pair_b); d.pair_ptr = (int*)at(p.pair_ptr);
  d.bseg = (int4*)at(p.bseg); d.bseg_ptr = (int*)at(p.bseg_ptr);
  d.bseg_cap = p.bseg_cap; d.dev_prep = p.dev_prep ? 1 : 0; d.E_raw = p.E_raw; d.raw_fmt = p.raw_fmt;
  d.no_err = 0;                                  // (the solve entry points set it when no per-edge errors were asked for)
  if (p.ext) {
    d.r_edge_pose = ext->r_edge_pose; d.r_edge_point = ext->r_edge_point; d.r_edge_uv = ext->r_edge_uv; d.r_edge_cam = ext->r_edge_cam;
    d.pose[0] = ext->pose[0]; d.pose[1] = ext->pose[1]; d.point[0] = ext->point[0]; d.point[1] = ext->point[1];
  } else {
    d.r_edge_pose = (const int*)at_if(p.dev_prep, p.r_pose); d.r_edge_point = (const int*)at_if(p.dev_prep, p.r_point);
    d.r_edge_uv = (const double*)at_if(p.dev_prep, p.r_uv); d.r_edge_cam = (const uint8_t*)at_if(p.cam_in, p.r_cam);
    d.pose[0] = (double*)at(p.pose0); d.pose[1] = (double*)at(p.pose1); d.point[0] = (double*)at(p.point0); d.point[1] = (double*)at(p.point1);
  }
  d.r_slot8 = (const uint8_t*)at_if(p.dev_prep, p.slot8); d.lm_compact = (const int*)at_if(p.dev_prep, p.lm_compact);
  d.perm = (int*)at_if(p.dev_prep, p.perm); d.c2_out = (double*)at_if(p.dev_prep, p.c2);
  d.pose_rank = (const int*)at_if(p.have_rank, p.pose_rank);
  d.K = Cam{pr->K[0], pr->K[1], pr->K[2], pr->K[3]};
  for (int i = 0; i < 14; ++i) d.ext[i] = pr->cam_ext[i];
  d.huber_delta = huber_delta; d.chi2_th = chi2_th;
  d.pose_init = (const double*)at_if(p.keep_init, p.pose_init); d.point_init = (const double*)at_if(p.keep_init, p.point_init);
  d.W = (double*)at(p.W); d.err_lin = (double*)at(p.err_lin); d.err_trial = (double*)at(p.err_trial);
  d.Hll = (double*)at(p.Hll); d.bl = (double*)at(p.bl); d.lin_slab = (double*)at(p.lin_slab);
  d.Hpp = (double*)at(p.Hpp); d.bp = (double*)at(p.bp); d.iter_comm = (double*)at(p.iter);
  d.schur_slab = (double*)at(p.schur); d.trial_comm = (double*)at(p.trial_comm); d.xp = (double*)at(p.xp); d.trial_slab = (double*)at(p.trial);
  d.scal_comm = (double*)at(p.scal_comm); d.scal = (double*)at(p.scal); d.lm_stat = (double*)at(p.lmstat); d.ticket = (unsigned int*)at(p.ticket);
  if (p.on_dev) {
    d.dev_prep = 1; d.E_raw = recs->E_raw;
    d.pose_free = recs->pose_free; d.lm_fixed = recs->lm_fixed; d.lm_id = recs->lm_id; d.lm_ptr = recs->lm_ptr; d.ch_lm = recs->ch_lm;
    d.e_pose = recs->e_pose; d.e_lmc = recs->e_lmc; d.e_cam = recs->e_cam; d.e_dup = recs->e_dup; d.e_uv = recs->e_uv;
    d.ch_desc = recs->ch_desc; d.e_rec = recs->e_rec; d.l_rec = recs->l_rec; d.perm = recs->perm; d.c2_out = recs->c2_out; d.lm_chunk = recs->lm_chunk;
    d.r_edge_pose = recs->r_edge_pose; d.r_edge_point = recs->r_edge_point; d.r_edge_uv = recs->r_edge_uv; d.r_edge_cam = recs->r_edge_cam;
    d.r_slot8 = recs->r_slot8; d.lm_compact = recs->lm_compact; d.pose_rank = nullptr;
  }
  bd = BigDev{}; bnd = BandDev{};
  if (!p.big) return;
  bd.n = p.n; bd.n_pad = p.n_pad; bd.ld = p.n_pad; bd.T = p.n_pad / NB; bd.nBlkS = p.nBlkS;
  bd.pe_ptr = p.on_dev ? pe_ptr_dev : (const int*)at(p.pe_ptr); bd.pe_edge = p.on_dev ? pe_edge_dev : (const int*)at(p.pe_edge);
  bd.sblk_pa = (const int*)at(p.sblk_pa); bd.sblk_pb = (const int*)at(p.sblk_pb);
  bd.spair_ptr = (const int*)at(p.spair_ptr); bd.spair_ab = nullptr;   // the pair lists live in the workspace of build_pairs
  bd.BDa = (double*)at(p.BDa); bd.Wma = (double*)at(p.Wma); bd.Cv = (double*)at(p.Cv);
  bd.S = (double*)at(p.S); bd.x = (double*)at(p.x); bd.Ld = (double*)at(p.Ld); bd.invd = (double*)at(p.invd); bd.Ninv = (double*)at(p.Ninv); bd.scale_part = (double*)at(p.scale_part);
  if (!p.band) return;
  bnd.on = 1; bnd.w = p.bw; bnd.K = p.bK; bnd.nP = p.nP; bnd.nPr = p.bnPr; bnd.wr = p.bwr;
  bnd.Sb = (double*)at(p.Sb); bnd.bsv = bnd.Sb + band_doubles(p.nP, p.bw);
  bnd.seg_p0 = (const int*)at(p.seg_p0); bnd.seg_m = (const int*)at(p.seg_m);
  bnd.U = (double*)at(p.U); bnd.Ls0 = (double*)at(p.Ls0); bnd.Sr = (double*)at(p.Sr);
  bnd.Ls1 = (double*)at(p.Ls1); bnd.xr = (double*)at(p.xr); bnd.LS0 = p.LS0; bnd.LS1 = p.LS1;
  if (p.bcr) {
    bnd.bcr.p0 = (const int*)at(p.bcr_p0); bnd.bcr.elim = (const int4*)at(p.bcr_elim);
    bcr_carve(bnd.bcr, (double*)at(p.bcr_mem), p.bcrN, p.bcrm);
  }
}

// A single window in the ctx arena: plan, reserve, fill, upload, the second state buffer, wire, the device's share of the marshalling.
ssx_status upload(ssx_ctx* ctx, const ssx_ba_problem* pr, const HostPrep& h, double huber_delta, double chi2_th, int world, int rank, BaDev& d, BigDev& bd,
                  const BandPlan& bp, BandDev& bnd, const WinExt* ext = nullptr, const BaDev* recs = nullptr, const int* pe_ptr_dev = nullptr, const int* pe_edge_dev = nullptr)
{
  BaWorkspace* ws = ba_workspace(ctx);
  const ArenaPlan p = plan_arena(pr, h, bp, world, false, ext, recs != nullptr);
  if (p.ext && !p.dev_prep) { ctx->set_error("ssx_ba: a window needs the device-side marshalling (<= %d free keyframes, no SSX_BA_HOST_PREP)", SSX_BA_SMALL_P); return SSX_ERR_UNSUPPORTED; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, ws->arena.reserve(p.total));
  SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(p.in_bytes, sizeof(double) * (7 * (size_t)p.P + 3 * (size_t)p.L + 2 * (size_t)p.E + (size_t)p.E_raw))));
  SSX_HIP_TRY(ctx, ws->scal.reserve(sizeof(double) * (SC_N + 3 * SSX_BA_MAX_STATS)));
  char* hs = ws->stage.as<char>();
  char* base = ws->arena.as<char>();
  fill_blob(p, pr, h, bp, hs);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, p.in_bytes, hipMemcpyHostToDevice, ctx->stream));
  wire_arena(p, base, base + p.in_bytes, pr, huber_delta, chi2_th, world, rank, ext, recs, pe_ptr_dev, pe_edge_dev, d, bd, bnd);
  // the second state buffer starts as a copy (landmarks without edges are never rewritten)
  if (p.pose0.n) SSX_HIP_TRY(ctx, hipMemcpyAsync(d.pose[1], d.pose[0], p.pose0.n, hipMemcpyDeviceToDevice, ctx->stream));
  if (p.point0.n) SSX_HIP_TRY(ctx, hipMemcpyAsync(d.point[1], d.point[0], p.point0.n, hipMemcpyDeviceToDevice, ctx->stream));
  if (p.nCh > 0 && (p.dev_lists || p.dev_prep)) {   // (a batch marshals all its windows with one launch pair: batch_build)
    if (p.dev_prep) {
      hipLaunchKernelGGL(k_prep_scatter, dim3((p.E_raw + CH - 1) / CH), dim3(CH), 0, ctx->stream, d);
      hipLaunchKernelGGL(k_prep_chunk, dim3(p.nCh), dim3(CH), 0, ctx->stream, d);
    } else {
      hipLaunchKernelGGL(k_build_lists, dim3(p.nCh), dim3(CH), 0, ctx->stream, d);
    }
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  return SSX_OK;
}

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

// Large windows, device-side marshalling (HostPrep::dev_prep): the caller's arrays and the host's counting tables go up once
// (25 bytes per observation instead of ~62 of marshalled records and columns, and none of the ~3 ms of host work a
// 480 000-observation window cost), k_prep_scatter / k_prep_chunk build the (landmark, pose) order, the packed records and the
// structure-of-arrays columns, and a stable radix sort by free pose gives the pose-major edge list.  Everything lives in
// ws->recs for the duration of the solve; `r` receives the pointers (the pair builder and upload() take them from there).
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

// Large windows: the non-zero blocks of the reduced system and their pair lists, on the device (kernels in ba_big.inc).
// Fills h.sblk_pa / h.sblk_pb / h.spair_ptr (sorted by (pa, pb); every diagonal block present, possibly with an empty
// list) and h.band_w; the lists themselves stay in the workspace: *ab_dev.
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
