// ssvio_amd/csrc/ba_window.inc -- ssx_ba_window: a sliding local-BA window that STAYS in HBM (included by ba.hip).
//
// Backend::OptimizeActiveMap (/root/reference/src/ssvio/backend.cpp:88-169) rebuilds its g2o graph from the active map at
// every keyframe, and Map::InsertKeyFrame / RemoveOldActiveKeyframe / RemoveOldActiveMapPoints
// (/root/reference/src/ssvio/map.cpp:27-56, 89-160) change that map by ONE keyframe between two optimisations.  The window
// object mirrors exactly that: a keyframe is pushed with its pose, the landmarks it introduces and its observations (only
// these cross PCIe), a keyframe is popped together with its observations and the landmarks nobody sees any more, and a
// solve works on what is resident: the observation arrays as they were pushed (the device sorts them, k_prep_*), the
// poses and landmarks in the window's two state buffers, which also receive the result.  Per solve the host counts the
// observations per landmark (one pass) and uploads ~3.6 bytes per observation + 13 per landmark of tables.
//
// Storage: keyframes and landmarks live in SLOTS (an index that never changes while the object is alive; freed slots are
// reused); the observations of a keyframe are one block of the observation storage; a popped keyframe's block stays as
// dead entries (landmark index -1) until more than half of the storage is dead, then the storage is rewritten.
// ORDER.  A solve gives its vertices the order of the caller's IDS (keyframes ascending by id, landmarks ascending by id) -- what
// g2o does with its vertex ids, and what a caller that re-marshals its map per keyframe (Backend::OptimizeActiveMap,
// backend.cpp:88-132 through g2o's id-sorted vertex containers) gets: free-pose indices, the edge order inside a landmark and the
// landmark order of the chunks follow it, so the bits of a solve are a function of the window's CONTENTS, never of which slots it
// reused.  ssx_ba_window_export lists the window in that order (observations in storage order), and a fresh ssx_ba_solve of the
// exported problem returns the bits the window returns.
//
// BETWEEN TWO OPTIMISATIONS the reference's map changes by more than one keyframe in / one out (backend.cpp:205-244):
//   outlier observations are unlinked   mappoint->RemoveActiveObservation / RemoveObservation     ssx_ba_window_remove_flagged /
//                                                                                                  ssx_ba_window_remove_observations
//   condemned map points are deleted    Map::RemoveAllOutlierMapPoints (map.cpp:175-194)          ssx_ba_window_remove_landmarks
//   a map point is FIXED while the keyframe of its first remaining observation is outside the window (backend.cpp:125-130):
//                                       ssx_ba_window_set_fix_rule(win, 1) keeps that flag itself -- per landmark the push
//                                       sequence number of the earliest POPPED keyframe that still observed it at its pop; the
//                                       landmark is fixed while that number is below the sequence numbers of all its live observers.

// caller's 64-bit id -> slot: open addressing, linear probing (a push resolves ~2400 ids, a pop erases ~400: std::unordered_map
// spent 100 of the 146 us of a pop + push here)
struct WinIdMap {
  std::vector<int64_t> keys;
  std::vector<int> vals;                               // >= 0 slot, -1 empty, -2 deleted
  size_t n_full = 0, n_used = 0;
  static size_t hash(int64_t k) { return (size_t)(((uint64_t)k * 0x9E3779B97F4A7C15ull) >> 20); }
  void rehash(size_t cap)
  {
    std::vector<int64_t> ok; std::vector<int> ov;
    ok.swap(keys); ov.swap(vals);
    keys.assign(cap, 0); vals.assign(cap, -1);
    n_full = n_used = 0;
    for (size_t i = 0; i < ov.size(); ++i) if (ov[i] >= 0) insert(ok[i], ov[i]);
  }
  int find(int64_t k) const
  {
    if (keys.empty()) return -1;
    const size_t m = keys.size() - 1;
    for (size_t i = hash(k) & m;; i = (i + 1) & m) {
      if (vals[i] == -1) return -1;
      if (vals[i] >= 0 && keys[i] == k) return vals[i];
    }
  }
  void insert(int64_t k, int v)                        // k must not be present
  {
    if ((n_used + 1) * 10 > keys.size() * 6) rehash(std::max<size_t>(1024, keys.size() * (n_full * 4 > keys.size() ? 2 : 1)));
    const size_t m = keys.size() - 1;
    size_t i = hash(k) & m;
    while (vals[i] >= 0) i = (i + 1) & m;
    if (vals[i] == -1) ++n_used;
    keys[i] = k; vals[i] = v; ++n_full;
  }
  void erase(int64_t k)
  {
    if (keys.empty()) return;
    const size_t m = keys.size() - 1;
    for (size_t i = hash(k) & m;; i = (i + 1) & m) {
      if (vals[i] == -1) return;
      if (vals[i] >= 0 && keys[i] == k) { vals[i] = -2; --n_full; return; }
    }
  }
};

struct ssx_ba_window {
  ssx_ctx* ctx = nullptr;
  int device = 0;
  ssx_ba_options opt;
  double K[4], cam_ext[14];
  struct Kf { int64_t id = 0; bool alive = false; int e_begin = 0, e_end = 0; int64_t seq = 0; };
  std::vector<Kf> kf;                                  // keyframe slot -> keyframe (seq: push sequence number, grows with every push)
  int64_t next_seq = 1;
  std::vector<int64_t> lm_id;                          // landmark slot -> caller's id
  std::vector<uint8_t> lm_alive;
  std::vector<int> lm_obs;                             // live observations per landmark slot
  std::vector<int> lm_free;                            // freed landmark slots (reused lowest first)
  std::unordered_map<int64_t, int> kf_slot;
  WinIdMap lm_slot;
  std::vector<int> obs_slot_tmp;                       // push: the landmark slots of the new observations (-1 - i = the i-th new landmark)
  // the order of the ids: (id, slot) ascending by id; a landmark that left keeps its entry with slot -1 until the list is cleaned
  std::vector<std::pair<int64_t, int>> lm_order;
  std::vector<int> lm_pos;                             // landmark slot -> its entry in lm_order
  size_t lm_tomb = 0;
  bool lm_unsorted = false;                            // an id below the last one was appended: sorted again before the next use
  std::vector<int> ord_kf, ord_lm;                     // live slots in id order (win_order, before every solve)
  // backend.cpp:125-130 (ssx_ba_window_set_fix_rule): see the file comment
  int fix_rule = 0;
  bool fixed_dirty = false;
  std::vector<uint8_t> lm_user_fixed;                  // the caller's flag (new_fixed, ssx_ba_window_set_landmark)
  std::vector<int64_t> lm_first_popped;                // per landmark slot; INT64_MAX = no popped observer
  std::vector<int64_t> min_live_tmp;
  // host mirror = the window as an ssx_ba_problem over slots (dead pose slots are fixed and unobserved, dead landmark
  // slots unobserved, dead observations carry landmark -1)
  std::vector<double> poses, points, e_uv;
  std::vector<uint8_t> pose_fixed, point_fixed, e_cam;
  std::vector<int> e_pose, e_point;
  int n_dead = 0;
  int n_rewrites = 0;                                  // how often the observation storage was rewritten (win_compact)
  // device
  DevBuf d_epose, d_epoint, d_euv, d_ecam, d_pose[2], d_point[2];
  size_t cap_e = 0, cap_p = 0, cap_l = 0;              // capacities in entries
  size_t e_on_device = 0;                              // observation entries already uploaded
  std::vector<std::pair<int, int>> dead_ranges;        // storage ranges killed since the last upload
  std::vector<int> dirty_kf, dirty_lm;                 // slots whose state must be (re)sent to BOTH state buffers
  WinExt ext;
  // scratch of the result mapping
  std::vector<double> r_pose, r_point, r_c2;
  std::vector<uint8_t> r_out;
};

namespace {

ssx_status win_grow(ssx_ctx* ctx, DevBuf& b, size_t new_bytes, size_t used_bytes)
{
  if (new_bytes <= b.cap) return SSX_OK;
  void* np = nullptr;
  const size_t want = new_bytes + new_bytes / 2 + 256;
  SSX_HIP_TRY(ctx, hipMalloc(&np, want));
  if (b.p && used_bytes) SSX_HIP_TRY(ctx, hipMemcpyAsync(np, b.p, used_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (b.p) { SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(b.p); }
  b.p = np; b.cap = want;
  return SSX_OK;
}

int win_n_kf(const ssx_ba_window* w) { int n = 0; for (const auto& k : w->kf) n += k.alive ? 1 : 0; return n; }
int win_n_lm(const ssx_ba_window* w) { int n = 0; for (uint8_t a : w->lm_alive) n += a ? 1 : 0; return n; }

// rewrite the observation storage without its dead entries (host mirror; the device copy is re-sent by win_sync)
void win_compact(ssx_ba_window* w)
{
  std::vector<int> ep, el; std::vector<double> uv; std::vector<uint8_t> cam;
  ep.reserve(w->e_pose.size() - w->n_dead); el.reserve(ep.capacity()); uv.reserve(2 * ep.capacity()); cam.reserve(ep.capacity());
  // blocks in storage order
  std::vector<int> order;
  for (int s = 0; s < (int)w->kf.size(); ++s) if (w->kf[s].alive) order.push_back(s);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return w->kf[a].e_begin < w->kf[b].e_begin; });
  for (int s : order) {
    ssx_ba_window::Kf& k = w->kf[s];
    const int nb = (int)ep.size();
    for (int e = k.e_begin; e < k.e_end; ++e) {
      if (w->e_point[e] < 0) continue;                  // an observation removed on its own (ssx_ba_window_remove_*)
      ep.push_back(w->e_pose[e]); el.push_back(w->e_point[e]); uv.push_back(w->e_uv[2 * (size_t)e]); uv.push_back(w->e_uv[2 * (size_t)e + 1]);
      cam.push_back(w->e_cam[e]);
    }
    k.e_begin = nb; k.e_end = (int)ep.size();
  }
  w->e_pose.swap(ep); w->e_point.swap(el); w->e_uv.swap(uv); w->e_cam.swap(cam);
  w->n_dead = 0;
  ++w->n_rewrites;
  w->e_on_device = 0;                                 // everything is re-sent
  w->dead_ranges.clear();
}

// a landmark leaves the window (nobody observes it any more, or the caller removed it)
void win_lm_free(ssx_ba_window* w, int ls)
{
  w->lm_alive[ls] = 0;
  w->lm_slot.erase(w->lm_id[ls]);
  w->lm_free.push_back(ls);
  w->lm_order[w->lm_pos[ls]].second = -1;
  ++w->lm_tomb;
}

// one observation dies where it lies (the caller records the storage range for the device copy)
inline void win_kill_obs(ssx_ba_window* w, int e)
{
  const int ls = w->e_point[e];
  w->e_point[e] = -1;
  ++w->n_dead;
  if (--w->lm_obs[ls] == 0) win_lm_free(w, ls);         // Map::RemoveOldActiveMapPoints: nobody sees it any more
}

// killed storage indices (ascending) -> dead ranges for the next sync, adjacent ones merged
void win_dead_indices(ssx_ba_window* w, const std::vector<int>& idx)
{
  for (size_t i = 0; i < idx.size();) {
    size_t j = i + 1;
    while (j < idx.size() && idx[j] == idx[j - 1] + 1) ++j;
    w->dead_ranges.emplace_back(idx[i], idx[j - 1] + 1);
    i = j;
  }
}

// trailing dead entries are simply dropped; a storage that is more than half dead is rewritten
void win_trim(ssx_ba_window* w)
{
  bool cut = false;
  while (!w->e_point.empty() && w->e_point.back() < 0) {
    w->e_pose.pop_back(); w->e_point.pop_back(); w->e_uv.pop_back(); w->e_uv.pop_back(); w->e_cam.pop_back(); --w->n_dead;
    cut = true;
  }
  if (cut) {
    const int n = (int)w->e_pose.size();
    for (auto& k : w->kf) if (k.alive) { k.e_end = std::min(k.e_end, n); k.e_begin = std::min(k.e_begin, k.e_end); }
    if (w->e_on_device > w->e_pose.size()) w->e_on_device = w->e_pose.size();
  }
  if ((size_t)w->n_dead * 2 > w->e_pose.size() && w->n_dead > 1024) win_compact(w);
}

// live slots in the order of the caller's ids (const: export may need it on a window nobody may change)
void win_order_lists(const ssx_ba_window* w, std::vector<int>& okf, std::vector<int>& olm)
{
  okf.clear();
  for (int s = 0; s < (int)w->kf.size(); ++s) if (w->kf[s].alive) okf.push_back(s);
  std::sort(okf.begin(), okf.end(), [&](int a, int b) { return w->kf[a].id < w->kf[b].id; });
  olm.clear();
  olm.reserve(w->lm_order.size());
  if (!w->lm_unsorted) {
    for (const auto& it : w->lm_order) if (it.second >= 0) olm.push_back(it.second);
  } else {
    std::vector<std::pair<int64_t, int>> tmp;
    for (const auto& it : w->lm_order) if (it.second >= 0) tmp.push_back(it);
    std::sort(tmp.begin(), tmp.end());
    for (const auto& it : tmp) olm.push_back(it.second);
  }
}

// before a solve: the order list is cleaned (entries of landmarks that left, ids that arrived out of order), the order of the
// live slots is handed to prepare() through the window's WinExt
void win_order(ssx_ba_window* w)
{
  if (w->lm_unsorted || w->lm_tomb * 2 > w->lm_order.size() + 64) {
    size_t k = 0;
    for (size_t i = 0; i < w->lm_order.size(); ++i) if (w->lm_order[i].second >= 0) w->lm_order[k++] = w->lm_order[i];
    w->lm_order.resize(k);
    if (w->lm_unsorted) std::sort(w->lm_order.begin(), w->lm_order.end());
    for (size_t i = 0; i < k; ++i) w->lm_pos[w->lm_order[i].second] = (int)i;
    w->lm_tomb = 0; w->lm_unsorted = false;
  }
  win_order_lists(w, w->ord_kf, w->ord_lm);
  w->ext.pose_order = w->ord_kf.data(); w->ext.n_pose_order = (int)w->ord_kf.size();
  w->ext.lm_order = w->ord_lm.data(); w->ext.n_lm_order = (int)w->ord_lm.size();
}

// backend.cpp:125-130 on the window: fixed = the caller's flag, or an observer that was popped precedes every live observer
void win_refresh_fixed(ssx_ba_window* w)
{
  if (!w->fix_rule || !w->fixed_dirty) return;
  const size_t nL = w->lm_id.size();
  std::vector<int64_t>& mn = w->min_live_tmp;
  mn.assign(nL, std::numeric_limits<int64_t>::max());
  for (const auto& k : w->kf) {
    if (!k.alive) continue;
    for (int e = k.e_begin; e < k.e_end; ++e) { const int ls = w->e_point[e]; if (ls >= 0 && k.seq < mn[ls]) mn[ls] = k.seq; }
  }
  for (size_t l = 0; l < nL; ++l)
    if (w->lm_alive[l]) w->point_fixed[l] = (w->lm_user_fixed[l] || w->lm_first_popped[l] < mn[l]) ? 1 : 0;
  w->fixed_dirty = false;
}

// Bring the device copies of n windows up to date -- appended observations, killed ranges, new / overwritten poses and
// landmarks -- with ONE host-to-device copy and ONE kernel: everything pending is gathered into a pinned block behind a
// table of segments (destination, source offset, bytes; or "fill with -1"), copied to a device staging block, and
// k_win_scatter distributes it (64 windows x ~10 small hipMemcpyAsync calls cost 3 ms of host time per step).
struct WinSeg { unsigned long long dst, dst2; unsigned int src_off, nbytes; int kind, rows; };
// kind 0: nbytes from data + src_off to dst (and to dst2 when it is not null: the two state buffers of a window)
// kind 1: (int) -1 over nbytes at dst (the landmark indices of a popped keyframe's observations)
// kind 2: `rows` rows of three doubles to rows idx[i] of dst and dst2; data + src_off = idx (rows ints, padded to 8 bytes), then the
//         values -- the landmarks a push brought in: their slots come from the free list and are scattered

__global__ __launch_bounds__(CH) void k_win_scatter(const WinSeg* __restrict__ segs, const char* __restrict__ data)
{
  const WinSeg sg = segs[blockIdx.x];
  char* dst = reinterpret_cast<char*>(sg.dst);
  char* dst2 = reinterpret_cast<char*>(sg.dst2);
  const char* src = data + sg.src_off;
  if (sg.kind == 1) {
    for (unsigned i = threadIdx.x; i < sg.nbytes / 4; i += CH) reinterpret_cast<int*>(dst)[i] = -1;
    return;
  }
  if (sg.kind == 2) {
    const int* idx = reinterpret_cast<const int*>(src);
    const double* val = reinterpret_cast<const double*>(src + (((size_t)sg.rows * sizeof(int) + 7) & ~size_t(7)));
    for (int i = threadIdx.x; i < 3 * sg.rows; i += CH) {
      const int r = i / 3, c = i - 3 * r;
      const double v = val[i];
      const size_t o = 3 * (size_t)idx[r] + c;
      reinterpret_cast<double*>(dst)[o] = v;
      reinterpret_cast<double*>(dst2)[o] = v;
    }
    return;
  }
  if (((sg.dst | sg.dst2 | sg.src_off | sg.nbytes) & 3) == 0) {
    for (unsigned i = threadIdx.x; i < sg.nbytes / 4; i += CH) {
      const unsigned v = reinterpret_cast<const unsigned*>(src)[i];
      reinterpret_cast<unsigned*>(dst)[i] = v;
      if (dst2) reinterpret_cast<unsigned*>(dst2)[i] = v;
    }
  } else {
    for (unsigned i = threadIdx.x; i < sg.nbytes; i += CH) { dst[i] = src[i]; if (dst2) dst2[i] = src[i]; }
  }
}

ssx_status win_sync_many(int n, ssx_ba_window* const* wins)
{
  ssx_ctx* ctx = wins[0]->ctx;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  BaWorkspace* ws = ba_workspace(ctx);
  static const bool timing = getenv("SSX_WIN_TIMING") != nullptr;
  const auto tq0 = std::chrono::steady_clock::now();
  auto tq_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq0).count(); };
  // 1. capacities (contents preserved; rare)
  for (int i = 0; i < n; ++i) {
    ssx_ba_window* w = wins[i];
    const size_t nE = w->e_pose.size(), nP = w->kf.size(), nL = w->lm_id.size();
    if (nE > w->cap_e) {
      const size_t c = std::max<size_t>(nE * 2, 4096), used = w->e_on_device;
      ssx_status st;
      if ((st = win_grow(ctx, w->d_epose, sizeof(int) * c, sizeof(int) * used)) != SSX_OK) return st;
      if ((st = win_grow(ctx, w->d_epoint, sizeof(int) * c, sizeof(int) * used)) != SSX_OK) return st;
      if ((st = win_grow(ctx, w->d_euv, sizeof(double) * 2 * c, sizeof(double) * 2 * used)) != SSX_OK) return st;
      if ((st = win_grow(ctx, w->d_ecam, c, used)) != SSX_OK) return st;
      w->cap_e = c;
    }
    if (nP > w->cap_p) {
      const size_t c = std::max<size_t>(nP * 2, 32);
      for (int b = 0; b < 2; ++b) { ssx_status st = win_grow(ctx, w->d_pose[b], sizeof(double) * 7 * c, sizeof(double) * 7 * w->cap_p); if (st != SSX_OK) return st; }
      w->cap_p = c;
    }
    if (nL > w->cap_l) {
      const size_t c = std::max<size_t>(nL * 2, 4096);
      for (int b = 0; b < 2; ++b) { ssx_status st = win_grow(ctx, w->d_point[b], sizeof(double) * 3 * c, sizeof(double) * 3 * w->cap_l); if (st != SSX_OK) return st; }
      w->cap_l = c;
    }
  }
  // 2. the segments and their data
  std::vector<WinSeg> segs;
  size_t data_bytes = 0;
  auto add = [&](void* dst, void* dst2, size_t nbytes) -> size_t {           // returns the offset of the segment's data
    const size_t off = data_bytes;
    segs.push_back(WinSeg{(unsigned long long)(uintptr_t)dst, (unsigned long long)(uintptr_t)dst2, (unsigned)off, (unsigned)nbytes, 0, 0});
    data_bytes += (nbytes + 15) & ~size_t(15);
    return off;
  };
  struct Fill { size_t off; const void* src; size_t n; ssx_ba_window* gather; };   // gather: the window whose dirty landmarks are packed at `off`
  std::vector<Fill> fills;
  for (int i = 0; i < n; ++i) {
    ssx_ba_window* w = wins[i];
    const size_t nE = w->e_pose.size(), a = w->e_on_device, ne = nE - a;
    if (ne) {
      fills.push_back({add(w->d_epose.as<int>() + a, nullptr, sizeof(int) * ne), &w->e_pose[a], sizeof(int) * ne, nullptr});
      fills.push_back({add(w->d_epoint.as<int>() + a, nullptr, sizeof(int) * ne), &w->e_point[a], sizeof(int) * ne, nullptr});
      fills.push_back({add(w->d_euv.as<double>() + 2 * a, nullptr, sizeof(double) * 2 * ne), &w->e_uv[2 * a], sizeof(double) * 2 * ne, nullptr});
      fills.push_back({add(w->d_ecam.as<uint8_t>() + a, nullptr, ne), &w->e_cam[a], ne, nullptr});
    }
    for (const auto& r : w->dead_ranges)
      if (r.second > r.first && (size_t)r.first < a)
        segs.push_back(WinSeg{(unsigned long long)(uintptr_t)(w->d_epoint.as<int>() + r.first), 0ull, 0u,
                              (unsigned)(sizeof(int) * (std::min<size_t>(r.second, a) - r.first)), 1, 0});
    std::sort(w->dirty_kf.begin(), w->dirty_kf.end());
    w->dirty_kf.erase(std::unique(w->dirty_kf.begin(), w->dirty_kf.end()), w->dirty_kf.end());
    for (int k : w->dirty_kf)
      fills.push_back({add(w->d_pose[0].as<double>() + 7 * (size_t)k, w->d_pose[1].as<double>() + 7 * (size_t)k, sizeof(double) * 7), &w->poses[7 * (size_t)k],
                       sizeof(double) * 7, nullptr});
    std::sort(w->dirty_lm.begin(), w->dirty_lm.end());
    w->dirty_lm.erase(std::unique(w->dirty_lm.begin(), w->dirty_lm.end()), w->dirty_lm.end());
    if (!w->dirty_lm.empty()) {                                    // ONE segment: [slots | xyz], scattered by the kernel into both buffers
      const size_t m = w->dirty_lm.size();
      const size_t nb = ((m * sizeof(int) + 7) & ~size_t(7)) + sizeof(double) * 3 * m;
      const size_t off = add(w->d_point[0].as<double>(), w->d_point[1].as<double>(), nb);
      segs.back().kind = 2; segs.back().rows = (int)m;
      fills.push_back({off, nullptr, 0, w});
    }
    w->ext.r_edge_pose = w->d_epose.as<int>(); w->ext.r_edge_point = w->d_epoint.as<int>();
    w->ext.r_edge_uv = w->d_euv.as<double>(); w->ext.r_edge_cam = w->d_ecam.as<uint8_t>();
    for (int b = 0; b < 2; ++b) { w->ext.pose[b] = w->d_pose[b].as<double>(); w->ext.point[b] = w->d_point[b].as<double>(); }
  }
  // (the windows' pending lists are cleared only once the copy and the scatter kernel are enqueued: a failure in between leaves
  // them pending, and the next sync sends them again)
  auto commit = [&]() {
    for (int i = 0; i < n; ++i) {
      ssx_ba_window* w = wins[i];
      w->dead_ranges.clear(); w->dirty_kf.clear(); w->dirty_lm.clear();
      w->e_on_device = w->e_pose.size();
    }
  };
  if (segs.empty()) { commit(); return SSX_OK; }
  if (data_bytes > 0xFFFFFFF0ull) { ctx->set_error("ssx_ba_window: more than 4 GB of pending uploads"); return SSX_ERR_UNSUPPORTED; }
  // 3. one pinned block [segment table | data] -> one copy -> one kernel
  const size_t tab_bytes = (sizeof(WinSeg) * segs.size() + 255) & ~size_t(255);
  SSX_HIP_TRY(ctx, ws->win_stage_h.reserve(tab_bytes + data_bytes + 256, 2.0));
  SSX_HIP_TRY(ctx, ws->win_stage_d.reserve(tab_bytes + data_bytes + 256, 2.0));
  char* hs = ws->win_stage_h.as<char>();
  const double tq_seg = tq_ms();
  memcpy(hs, segs.data(), sizeof(WinSeg) * segs.size());
  // (segments that carry data were added in the order of `fills`)
  ws->pool.run((int)fills.size(), std::min<int>(16, std::max<int>(1, (int)fills.size() / 8)), [&](int q) {
    const Fill& f = fills[q];
    if (!f.gather) { memcpy(hs + tab_bytes + f.off, f.src, f.n); return; }
    ssx_ba_window* w = f.gather;
    const size_t m = w->dirty_lm.size();
    int* idx = reinterpret_cast<int*>(hs + tab_bytes + f.off);
    double* val = reinterpret_cast<double*>(hs + tab_bytes + f.off + ((m * sizeof(int) + 7) & ~size_t(7)));
    for (size_t j = 0; j < m; ++j) {
      const int l = w->dirty_lm[j];
      idx[j] = l;
      val[3 * j] = w->points[3 * (size_t)l]; val[3 * j + 1] = w->points[3 * (size_t)l + 1]; val[3 * j + 2] = w->points[3 * (size_t)l + 2];
    }
  });
  const double tq_fill = tq_ms();
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ws->win_stage_d.p, hs, tab_bytes + data_bytes, hipMemcpyHostToDevice, s));
  const double tq_copy = tq_ms();
  hipLaunchKernelGGL(k_win_scatter, dim3((unsigned)segs.size()), dim3(CH), 0, s, reinterpret_cast<const WinSeg*>(ws->win_stage_d.p),
                     ws->win_stage_d.as<char>() + tab_bytes);
  SSX_HIP_TRY(ctx, hipGetLastError());
  commit();
  if (timing)
    fprintf(stderr, "[win_sync_many n=%d] segments %.3f | gather of %zu pieces, %.2f MB %.3f | hipMemcpyAsync %.3f | launch + commit %.3f ms\n", n, tq_seg, fills.size(),
            (tab_bytes + data_bytes) / 1e6, tq_fill - tq_seg, tq_copy - tq_fill, tq_ms() - tq_copy);
  return SSX_OK;
}

ssx_status win_sync(ssx_ba_window* w) { return win_sync_many(1, &w); }

// the window as an ssx_ba_problem over SLOTS (what prepare() / upload() see); the order of the ids travels in w->ext
void win_view(ssx_ba_window* w, ssx_ba_problem* pr)
{
  win_refresh_fixed(w);
  win_order(w);
  memset(pr, 0, sizeof(*pr));
  pr->P = (int)w->kf.size(); pr->poses = w->poses.data(); pr->pose_fixed = w->pose_fixed.data();
  pr->L = (int)w->lm_id.size(); pr->points = w->points.data(); pr->point_fixed = w->point_fixed.data();
  pr->E = (int)w->e_pose.size(); pr->edge_pose = w->e_pose.data(); pr->edge_point = w->e_point.data(); pr->edge_uv = w->e_uv.data();
  pr->edge_cam = w->e_cam.data();
  memcpy(pr->K, w->K, sizeof(pr->K)); memcpy(pr->cam_ext, w->cam_ext, sizeof(pr->cam_ext));
}

// results over slots / storage -> the caller's arrays in export order (win_view built it: ord_kf / ord_lm); the host mirror
// takes the new state
void win_unpack(ssx_ba_window* w, const ssx_ba_result& slot_res, ssx_ba_result* res)
{
  w->poses.swap(w->r_pose);                          // (dead slots keep whatever they held: never read)
  w->points.swap(w->r_point);
  const std::vector<double>& rp = w->poses; const std::vector<double>& rq = w->points;
  double* po = res->poses_out; double* pt = res->points_out; double* c2 = res->edge_chi2; uint8_t* ol = res->edge_outlier;
  *res = slot_res;
  res->poses_out = po; res->points_out = pt; res->edge_chi2 = c2; res->edge_outlier = ol;
  if (po) { size_t k = 0; for (int s : w->ord_kf) { memcpy(po + 7 * k, &rp[7 * (size_t)s], sizeof(double) * 7); ++k; } }
  if (pt) { size_t k = 0; for (int l : w->ord_lm) { memcpy(pt + 3 * k, &rq[3 * (size_t)l], sizeof(double) * 3); ++k; } }
  if (c2 || ol) {
    size_t k = 0;
    for (size_t e = 0; e < w->e_point.size(); ++e) {
      if (w->e_point[e] < 0) continue;
      if (c2) c2[k] = w->r_c2[e];
      if (ol) ol[k] = w->r_out[e];
      ++k;
    }
  }
}

}  // namespace

extern "C" {

ssx_status ssx_ba_window_create(ssx_ctx* ctx, const ssx_ba_options* opt_in, const double* K4, const double* cam_ext14, ssx_ba_window** out)
{
  if (!ctx || !K4 || !cam_ext14 || !out) return SSX_ERR_INVALID_ARG;
  *out = nullptr;
  ssx_ba_window* w = new ssx_ba_window();
  w->ctx = ctx; w->device = ctx->device;
  if (opt_in) w->opt = *opt_in; else ssx_ba_default_options(&w->opt);
  if (w->opt.comm || w->opt.allreduce) { delete w; ctx->set_error("ssx_ba_window_create: a window does not take a collective"); return SSX_ERR_UNSUPPORTED; }
  memcpy(w->K, K4, sizeof(w->K)); memcpy(w->cam_ext, cam_ext14, sizeof(w->cam_ext));
  *out = w;
  return SSX_OK;
}

void ssx_ba_window_destroy(ssx_ba_window* w)
{
  if (!w) return;
  (void)hipSetDevice(w->device);
  w->d_epose.release(); w->d_epoint.release(); w->d_euv.release(); w->d_ecam.release();
  for (int b = 0; b < 2; ++b) { w->d_pose[b].release(); w->d_point[b].release(); }
  delete w;
}

ssx_status ssx_ba_window_set_fix_rule(ssx_ba_window* w, int32_t rule)
{
  if (!w || rule < 0 || rule > 1) return SSX_ERR_INVALID_ARG;
  w->fix_rule = rule;
  if (rule) w->fixed_dirty = true;
  else for (size_t l = 0; l < w->lm_id.size(); ++l) w->point_fixed[l] = w->lm_user_fixed[l];
  return SSX_OK;
}

}  // extern "C"

// obs_lm (ids) or obs_slot (landmark slots as ssx_ba_window_push_keyframe_slots takes them): exactly one is given
static ssx_status win_push(ssx_ba_window* w, int64_t kf_id, const double* pose7, int32_t pose_fixed, int32_t n_new, const int64_t* new_ids,
                           const double* new_xyz, const uint8_t* new_fixed, int32_t* new_slots_out, int32_t n_obs, const int64_t* obs_lm,
                           const int32_t* obs_slot, const double* obs_uv, const uint8_t* obs_cam)
{
  if (!w || !pose7 || n_new < 0 || n_obs < 0 || (n_new && (!new_ids || !new_xyz)) || (n_obs && ((!obs_lm && !obs_slot) || !obs_uv))) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = w->ctx;
  if (w->kf_slot.count(kf_id)) { ctx->set_error("ssx_ba_window_push_keyframe: keyframe %lld is already in the window", (long long)kf_id); return SSX_ERR_INVALID_ARG; }
  // validate before anything is changed; every observation's landmark is resolved ONCE (slot, or -1 - i for the i-th new one)
  for (int i = 0; i < n_new; ++i)
    if (w->lm_slot.find(new_ids[i]) >= 0) { ctx->set_error("ssx_ba_window_push_keyframe: landmark %lld is already in the window", (long long)new_ids[i]); return SSX_ERR_INVALID_ARG; }
  {
    WinIdMap fresh;
    fresh.rehash(std::max<size_t>(1024, (size_t)1 << (32 - __builtin_clz((unsigned)(2 * n_new + 1)))));
    for (int i = 0; i < n_new; ++i) {
      if (fresh.find(new_ids[i]) >= 0) { ctx->set_error("ssx_ba_window_push_keyframe: landmark %lld listed twice", (long long)new_ids[i]); return SSX_ERR_INVALID_ARG; }
      fresh.insert(new_ids[i], i);
    }
    w->obs_slot_tmp.resize((size_t)n_obs);
    if (obs_slot) {                                    // the caller kept the slots: no id is looked up
      for (int i = 0; i < n_obs; ++i) {
        const int r = obs_slot[i];
        if (r >= 0 ? (r >= (int)w->lm_alive.size() || !w->lm_alive[r]) : (-1 - r >= n_new)) {
          ctx->set_error("ssx_ba_window_push_keyframe_slots: observation %d refers to landmark slot %d, which holds no landmark", i, r);
          return SSX_ERR_INVALID_ARG;
        }
        w->obs_slot_tmp[i] = r;
      }
    } else
    for (int i = 0; i < n_obs; ++i) {
      int ls = w->lm_slot.find(obs_lm[i]);
      if (ls < 0) {
        const int f = fresh.find(obs_lm[i]);
        if (f < 0) {
          ctx->set_error("ssx_ba_window_push_keyframe: observation %d refers to landmark %lld, which is not in the window", i, (long long)obs_lm[i]);
          return SSX_ERR_INVALID_ARG;
        }
        ls = -1 - f;
      }
      w->obs_slot_tmp[i] = ls;
    }
  }
  // keyframe slot: the lowest free one
  int ks = -1;
  for (int s = 0; s < (int)w->kf.size(); ++s) if (!w->kf[s].alive) { ks = s; break; }
  if (ks < 0) { ks = (int)w->kf.size(); w->kf.emplace_back(); w->poses.resize(7 * w->kf.size(), 0.0); w->pose_fixed.resize(w->kf.size(), 1); }
  ssx_ba_window::Kf& k = w->kf[ks];
  k.id = kf_id; k.alive = true; k.seq = w->next_seq++;
  memcpy(&w->poses[7 * (size_t)ks], pose7, sizeof(double) * 7);
  w->pose_fixed[ks] = pose_fixed ? 1 : 0;
  w->kf_slot[kf_id] = ks;
  w->dirty_kf.push_back(ks);
  // landmarks: lowest freed slots first
  std::sort(w->lm_free.begin(), w->lm_free.end(), std::greater<int>());
  std::vector<int> new_slot((size_t)n_new);
  for (int i = 0; i < n_new; ++i) {
    int ls;
    if (!w->lm_free.empty()) { ls = w->lm_free.back(); w->lm_free.pop_back(); }
    else {
      ls = (int)w->lm_id.size();
      w->lm_id.push_back(0); w->lm_alive.push_back(0); w->lm_obs.push_back(0); w->point_fixed.push_back(0); w->points.resize(3 * w->lm_id.size(), 0.0);
      w->lm_user_fixed.push_back(0); w->lm_first_popped.push_back(0); w->lm_pos.push_back(0);
    }
    w->lm_id[ls] = new_ids[i]; w->lm_alive[ls] = 1; w->lm_obs[ls] = 0;
    w->lm_user_fixed[ls] = (new_fixed && new_fixed[i]) ? 1 : 0;
    w->point_fixed[ls] = w->lm_user_fixed[ls];
    w->lm_first_popped[ls] = std::numeric_limits<int64_t>::max();
    memcpy(&w->points[3 * (size_t)ls], new_xyz + 3 * (size_t)i, sizeof(double) * 3);
    w->lm_slot.insert(new_ids[i], ls);
    if (!w->lm_order.empty() && new_ids[i] < w->lm_order.back().first) w->lm_unsorted = true;   // (map-point ids grow with time: rare)
    w->lm_pos[ls] = (int)w->lm_order.size();
    w->lm_order.emplace_back(new_ids[i], ls);
    w->dirty_lm.push_back(ls);
    new_slot[i] = ls;
    if (new_slots_out) new_slots_out[i] = ls;
  }
  // observations: one block at the end of the storage
  k.e_begin = (int)w->e_pose.size();
  const size_t e0 = w->e_pose.size();
  w->e_pose.resize(e0 + n_obs, ks); w->e_point.resize(e0 + n_obs); w->e_uv.resize(2 * (e0 + n_obs)); w->e_cam.resize(e0 + n_obs);
  for (size_t e = e0; e < e0 + (size_t)n_obs; ++e) w->e_pose[e] = ks;
  if (n_obs) memcpy(&w->e_uv[2 * e0], obs_uv, sizeof(double) * 2 * (size_t)n_obs);
  for (int i = 0; i < n_obs; ++i) {
    const int r = w->obs_slot_tmp[i];
    const int ls = r >= 0 ? r : new_slot[-1 - r];
    w->e_point[e0 + i] = ls;
    w->e_cam[e0 + i] = (obs_cam && obs_cam[i]) ? 1 : 0;
    w->lm_obs[ls]++;
  }
  k.e_end = (int)w->e_pose.size();
  return SSX_OK;
}

extern "C" {

ssx_status ssx_ba_window_push_keyframe(ssx_ba_window* w, int64_t kf_id, const double* pose7, int32_t pose_fixed, int32_t n_new,
                                       const int64_t* new_ids, const double* new_xyz, const uint8_t* new_fixed, int32_t n_obs,
                                       const int64_t* obs_lm, const double* obs_uv, const uint8_t* obs_cam)
{
  if (n_obs > 0 && !obs_lm) return SSX_ERR_INVALID_ARG;
  return win_push(w, kf_id, pose7, pose_fixed, n_new, new_ids, new_xyz, new_fixed, nullptr, n_obs, obs_lm, nullptr, obs_uv, obs_cam);
}

ssx_status ssx_ba_window_push_keyframe_slots(ssx_ba_window* w, int64_t kf_id, const double* pose7, int32_t pose_fixed, int32_t n_new,
                                             const int64_t* new_ids, const double* new_xyz, const uint8_t* new_fixed, int32_t* new_slots_out,
                                             int32_t n_obs, const int32_t* obs_slot, const double* obs_uv, const uint8_t* obs_cam)
{
  if (n_obs > 0 && !obs_slot) return SSX_ERR_INVALID_ARG;
  return win_push(w, kf_id, pose7, pose_fixed, n_new, new_ids, new_xyz, new_fixed, new_slots_out, n_obs, nullptr, obs_slot, obs_uv, obs_cam);
}

// Map::RemoveOldActiveKeyframe + RemoveOldActiveMapPoints (map.cpp:89-160): the keyframe goes with its observations; a landmark
// nobody observes any more goes too; a landmark it was the FIRST observer of is fixed from now on (fix rule 1)
ssx_status ssx_ba_window_pop_keyframe(ssx_ba_window* w, int64_t kf_id)
{
  if (!w) return SSX_ERR_INVALID_ARG;
  auto it = w->kf_slot.find(kf_id);
  if (it == w->kf_slot.end()) { w->ctx->set_error("ssx_ba_window_pop_keyframe: keyframe %lld is not in the window", (long long)kf_id); return SSX_ERR_INVALID_ARG; }
  const int ks = it->second;
  ssx_ba_window::Kf& k = w->kf[ks];
  int first_live = -1, end_live = -1;
  for (int e = k.e_begin; e < k.e_end; ++e) {
    const int ls = w->e_point[e];
    if (ls < 0) continue;
    if (k.seq < w->lm_first_popped[ls]) w->lm_first_popped[ls] = k.seq;
    win_kill_obs(w, e);
    if (first_live < 0) first_live = e;
    end_live = e + 1;
  }
  if (first_live >= 0) w->dead_ranges.emplace_back(first_live, end_live);   // (entries in between that were dead already are -1 on the device too)
  k.alive = false; k.e_begin = k.e_end = 0;
  w->pose_fixed[ks] = 1;
  w->kf_slot.erase(it);
  w->fixed_dirty = true;
  win_trim(w);
  return SSX_OK;
}

// backend.cpp:205-227: the observations of keyframe kf_id of the landmarks lm_ids[i] (camera cams[i]; cams NULL = either camera)
// are unlinked.  A pair the window does not hold is skipped (the reference's RemoveActiveObservation is silent there too);
// *n_removed (nullable) counts what was removed.
ssx_status ssx_ba_window_remove_observations(ssx_ba_window* w, int64_t kf_id, int32_t n, const int64_t* lm_ids, const uint8_t* cams,
                                             int32_t* n_removed)
{
  if (!w || n < 0 || (n > 0 && !lm_ids)) return SSX_ERR_INVALID_ARG;
  if (n_removed) *n_removed = 0;
  auto it = w->kf_slot.find(kf_id);
  if (it == w->kf_slot.end()) { w->ctx->set_error("ssx_ba_window_remove_observations: keyframe %lld is not in the window", (long long)kf_id); return SSX_ERR_INVALID_ARG; }
  const ssx_ba_window::Kf& k = w->kf[it->second];
  // mark[slot]: bit 0 = remove the left observation, bit 1 = the right one
  std::vector<uint8_t> mark(w->lm_id.size(), 0);
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const int ls = w->lm_slot.find(lm_ids[i]);
    if (ls < 0) continue;
    mark[ls] |= cams ? (cams[i] ? 2 : 1) : 3;
    any = true;
  }
  if (!any) return SSX_OK;
  std::vector<int> killed;
  for (int e = k.e_begin; e < k.e_end; ++e) {
    const int ls = w->e_point[e];
    if (ls < 0 || !(mark[ls] & (w->e_cam[e] ? 2 : 1))) continue;
    win_kill_obs(w, e);
    killed.push_back(e);
  }
  win_dead_indices(w, killed);
  if (n_removed) *n_removed = (int32_t)killed.size();
  if (!killed.empty()) { w->fixed_dirty = true; win_trim(w); }
  return SSX_OK;
}

// The same, addressed like the result of a solve: flags[i] != 0 removes the i-th observation in the order of
// ssx_ba_window_export -- ssx_ba_result.edge_outlier of the solve that just ran can be passed as it is
// (backend.cpp:207-227 `if (ef.first->chi2() > chi2_th)`).  n_obs must be the window's observation count.
ssx_status ssx_ba_window_remove_flagged(ssx_ba_window* w, int32_t n_obs, const uint8_t* flags, int32_t* n_removed)
{
  if (!w || n_obs < 0 || (n_obs > 0 && !flags)) return SSX_ERR_INVALID_ARG;
  if (n_removed) *n_removed = 0;
  if ((size_t)n_obs != w->e_pose.size() - (size_t)w->n_dead) {
    w->ctx->set_error("ssx_ba_window_remove_flagged: %d flags for a window of %d observations", n_obs, (int)(w->e_pose.size() - (size_t)w->n_dead));
    return SSX_ERR_INVALID_ARG;
  }
  std::vector<int> killed;
  size_t k = 0;
  for (size_t e = 0; e < w->e_point.size(); ++e) {
    if (w->e_point[e] < 0) continue;
    if (flags[k++]) killed.push_back((int)e);
  }
  for (int e : killed) win_kill_obs(w, e);
  win_dead_indices(w, killed);
  if (n_removed) *n_removed = (int32_t)killed.size();
  if (!killed.empty()) { w->fixed_dirty = true; win_trim(w); }
  return SSX_OK;
}

// Map::RemoveAllOutlierMapPoints (map.cpp:175-194; the points EstimateCurrentPose or the backend condemned): the landmarks go
// with all their observations.  Ids the window does not hold are skipped.
ssx_status ssx_ba_window_remove_landmarks(ssx_ba_window* w, int32_t n, const int64_t* lm_ids, int32_t* n_removed)
{
  if (!w || n < 0 || (n > 0 && !lm_ids)) return SSX_ERR_INVALID_ARG;
  if (n_removed) *n_removed = 0;
  std::vector<uint8_t> mark(w->lm_id.size(), 0);
  int found = 0;
  for (int i = 0; i < n; ++i) {
    const int ls = w->lm_slot.find(lm_ids[i]);
    if (ls >= 0 && !mark[ls]) { mark[ls] = 1; ++found; }
  }
  if (!found) return SSX_OK;
  std::vector<int> killed;
  for (size_t e = 0; e < w->e_point.size(); ++e) {
    const int ls = w->e_point[e];
    if (ls >= 0 && mark[ls]) killed.push_back((int)e);
  }
  for (int e : killed) win_kill_obs(w, e);               // (the landmark's last observation frees its slot)
  for (size_t ls = 0; ls < mark.size(); ++ls) if (mark[ls] && w->lm_alive[ls]) win_lm_free(w, (int)ls);   // pushed without observations
  win_dead_indices(w, killed);
  if (n_removed) *n_removed = found;
  win_trim(w);
  return SSX_OK;
}

ssx_status ssx_ba_window_update_batch(int32_t n, ssx_ba_window* const* wins, const ssx_ba_window_update* ups, ssx_status* status_out)
{
  if (n < 0 || (n > 0 && (!wins || !ups))) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  for (int i = 0; i < n; ++i) if (!wins[i] || wins[i]->ctx != wins[0]->ctx) return SSX_ERR_INVALID_ARG;
  {
    std::vector<const ssx_ba_window*> sorted(wins, wins + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return SSX_ERR_INVALID_ARG;   // two edits of one window would race
  }
  auto one = [&](int i) -> ssx_status {
    const ssx_ba_window_update& u = ups[i];
    // what the last optimisation decided first (its flags are in the order of the window BEFORE this call's other edits)
    if (u.n_remove_flags > 0) { const ssx_status st = ssx_ba_window_remove_flagged(wins[i], u.n_remove_flags, u.remove_flags, nullptr); if (st != SSX_OK) return st; }
    if (u.n_remove_lm > 0) { const ssx_status st = ssx_ba_window_remove_landmarks(wins[i], u.n_remove_lm, u.remove_lm_ids, nullptr); if (st != SSX_OK) return st; }
    if (u.pop) { const ssx_status st = ssx_ba_window_pop_keyframe(wins[i], u.pop_kf_id); if (st != SSX_OK) return st; }
    if (!u.push) return SSX_OK;
    return win_push(wins[i], u.kf_id, u.pose7, u.pose_fixed, u.n_new, u.new_ids, u.new_xyz, u.new_fixed, u.obs_lm ? nullptr : u.new_slots_out, u.n_obs,
                    u.obs_lm, u.obs_lm ? nullptr : u.obs_slot, u.obs_uv, u.obs_cam);
  };
  std::vector<ssx_status> sts(n, SSX_OK);
  ssx_ctx* ctx = wins[0]->ctx;
  if (ctx && n > 1) {
    const int hw = (int)std::thread::hardware_concurrency();
    ba_workspace(ctx)->pool.run(n, std::max(1, std::min({n, host_threads_cap(), hw > 1 ? hw / 2 : 1})), [&](int i) { sts[i] = one(i); });
  } else {
    for (int i = 0; i < n; ++i) sts[i] = one(i);
  }
  ssx_status first = SSX_OK;
  for (int i = 0; i < n; ++i) {
    if (status_out) status_out[i] = sts[i];
    if (first == SSX_OK && sts[i] != SSX_OK) first = sts[i];
  }
  return first;
}

ssx_status ssx_ba_window_set_pose(ssx_ba_window* w, int64_t kf_id, const double* pose7, int32_t fixed)
{
  if (!w || !pose7) return SSX_ERR_INVALID_ARG;
  auto it = w->kf_slot.find(kf_id);
  if (it == w->kf_slot.end()) { w->ctx->set_error("ssx_ba_window_set_pose: keyframe %lld is not in the window", (long long)kf_id); return SSX_ERR_INVALID_ARG; }
  memcpy(&w->poses[7 * (size_t)it->second], pose7, sizeof(double) * 7);
  if (fixed >= 0) w->pose_fixed[it->second] = fixed ? 1 : 0;
  w->dirty_kf.push_back(it->second);
  return SSX_OK;
}

ssx_status ssx_ba_window_set_landmark(ssx_ba_window* w, int64_t lm_id, const double* xyz, int32_t fixed)
{
  if (!w) return SSX_ERR_INVALID_ARG;
  const int ls = w->lm_slot.find(lm_id);
  if (ls < 0) { w->ctx->set_error("ssx_ba_window_set_landmark: landmark %lld is not in the window", (long long)lm_id); return SSX_ERR_INVALID_ARG; }
  if (xyz) { memcpy(&w->points[3 * (size_t)ls], xyz, sizeof(double) * 3); w->dirty_lm.push_back(ls); }
  if (fixed >= 0) {
    w->lm_user_fixed[ls] = fixed ? 1 : 0;
    if (w->fix_rule) w->fixed_dirty = true; else w->point_fixed[ls] = w->lm_user_fixed[ls];
  }
  return SSX_OK;
}

ssx_status ssx_ba_window_size(const ssx_ba_window* w, int32_t* n_keyframes, int32_t* n_landmarks, int32_t* n_observations)
{
  if (!w) return SSX_ERR_INVALID_ARG;
  if (n_keyframes) *n_keyframes = win_n_kf(w);
  if (n_landmarks) *n_landmarks = win_n_lm(w);
  if (n_observations) *n_observations = (int32_t)(w->e_pose.size() - (size_t)w->n_dead);
  return SSX_OK;
}

// The window as an ordinary problem (current estimate): the caller's arrays must hold ssx_ba_window_size() entries.
// Keyframes and landmarks ascending by id (the order a solve uses), observations in storage order.
ssx_status ssx_ba_window_export(const ssx_ba_window* w, int64_t* kf_ids, double* poses, uint8_t* pose_fixed, int64_t* lm_ids, double* points,
                                uint8_t* point_fixed, int32_t* edge_pose, int32_t* edge_point, double* edge_uv, uint8_t* edge_cam)
{
  if (!w) return SSX_ERR_INVALID_ARG;
  std::vector<int> okf, olm;
  win_order_lists(w, okf, olm);
  std::vector<uint8_t> fx;                              // the flags the next solve would use (fix rule 1), without touching the window
  if (point_fixed) {
    fx = w->point_fixed;
    if (w->fix_rule && w->fixed_dirty) {
      std::vector<int64_t> mn(w->lm_id.size(), std::numeric_limits<int64_t>::max());
      for (const auto& k : w->kf) {
        if (!k.alive) continue;
        for (int e = k.e_begin; e < k.e_end; ++e) { const int ls = w->e_point[e]; if (ls >= 0 && k.seq < mn[ls]) mn[ls] = k.seq; }
      }
      for (size_t l = 0; l < fx.size(); ++l) if (w->lm_alive[l]) fx[l] = (w->lm_user_fixed[l] || w->lm_first_popped[l] < mn[l]) ? 1 : 0;
    }
  }
  std::vector<int> kf_rank(w->kf.size(), -1), lm_rank(w->lm_id.size(), -1);
  int k = 0;
  for (int s : okf) {
    kf_rank[s] = k;
    if (kf_ids) kf_ids[k] = w->kf[s].id;
    if (poses) memcpy(poses + 7 * (size_t)k, &w->poses[7 * (size_t)s], sizeof(double) * 7);
    if (pose_fixed) pose_fixed[k] = w->pose_fixed[s];
    ++k;
  }
  k = 0;
  for (int l : olm) {
    lm_rank[l] = k;
    if (lm_ids) lm_ids[k] = w->lm_id[l];
    if (points) memcpy(points + 3 * (size_t)k, &w->points[3 * (size_t)l], sizeof(double) * 3);
    if (point_fixed) point_fixed[k] = fx[l];
    ++k;
  }
  k = 0;
  for (size_t e = 0; e < w->e_point.size(); ++e) {
    if (w->e_point[e] < 0) continue;
    if (edge_pose) edge_pose[k] = kf_rank[w->e_pose[e]];
    if (edge_point) edge_point[k] = lm_rank[w->e_point[e]];
    if (edge_uv) { edge_uv[2 * (size_t)k] = w->e_uv[2 * e]; edge_uv[2 * (size_t)k + 1] = w->e_uv[2 * e + 1]; }
    if (edge_cam) edge_cam[k] = w->e_cam[e];
    ++k;
  }
  return SSX_OK;
}

// Optimise the window where it lies.  res->poses_out (n_keyframes x 7), points_out (n_landmarks x 3), edge_chi2 /
// edge_outlier (n_observations) are in the order of ssx_ba_window_export; the window's state becomes the result.
ssx_status ssx_ba_window_solve(ssx_ba_window* w, ssx_ba_result* res)
{
  if (!w || !res) return SSX_ERR_INVALID_ARG;
  ssx_status st = win_sync(w);
  if (st != SSX_OK) return st;
  ssx_ba_problem pr;
  win_view(w, &pr);
  w->r_pose.assign(7 * w->kf.size() + 1, 0.0); w->r_point.assign(3 * w->lm_id.size() + 1, 0.0);
  w->r_c2.assign(w->e_pose.size() + 1, 0.0); w->r_out.assign(w->e_pose.size() + 1, 0);
  ssx_ba_result sr;
  memset(&sr, 0, sizeof(sr));
  sr.poses_out = w->r_pose.data(); sr.points_out = w->r_point.data();
  const bool want_err = res->edge_chi2 || res->edge_outlier;
  sr.edge_chi2 = want_err ? w->r_c2.data() : nullptr; sr.edge_outlier = want_err ? w->r_out.data() : nullptr;
  st = ba_solve_impl(w->ctx, &pr, &w->opt, &sr, &w->ext);
  if (st != SSX_OK) return st;
  w->r_pose.resize(w->poses.size()); w->r_point.resize(w->points.size());
  win_unpack(w, sr, res);
  return SSX_OK;
}

// n windows of one ctx in one call: the batched kernels (one grid dimension = the window), one upload of the counting
// tables, one download.  Per window the bits of ssx_ba_window_solve.
ssx_status ssx_ba_window_solve_batch(int32_t n, ssx_ba_window* const* wins, ssx_ba_result* results)
{
  if (n < 0 || (n > 0 && (!wins || !results))) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  for (int i = 0; i < n; ++i) if (!wins[i] || wins[i]->ctx != wins[0]->ctx) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = wins[0]->ctx;
  if (n == 1) return ssx_ba_window_solve(wins[0], &results[0]);
  std::vector<ssx_ba_problem> prs(n);
  std::vector<ssx_ba_result> srs(n);
  std::vector<WinExt*> exts(n);
  bool with_err = false;
  static const bool timing = getenv("SSX_WIN_TIMING") != nullptr;      // phase times of the call on stderr (tools/window_time.py)
  const auto tp0 = std::chrono::steady_clock::now();
  {
    const ssx_status st0 = win_sync_many(n, wins);
    if (st0 != SSX_OK) return st0;
  }
  const auto tp1 = std::chrono::steady_clock::now();
  ba_workspace(ctx)->pool.run(n, std::min(n, host_threads_cap()), [&](int i) {    // (the fix-rule pass and the id order are per-window host work)
    ssx_ba_window* w = wins[i];
    win_view(w, &prs[i]);
    w->r_pose.resize(7 * w->kf.size() + 1); w->r_point.resize(3 * w->lm_id.size() + 1);
    const bool we = results[i].edge_chi2 || results[i].edge_outlier;
    if (we) { w->r_c2.assign(w->e_pose.size() + 1, 0.0); w->r_out.assign(w->e_pose.size() + 1, 0); }
    memset(&srs[i], 0, sizeof(ssx_ba_result));
    srs[i].poses_out = w->r_pose.data(); srs[i].points_out = w->r_point.data();
    srs[i].edge_chi2 = we ? w->r_c2.data() : nullptr; srs[i].edge_outlier = we ? w->r_out.data() : nullptr;
    exts[i] = &w->ext;
  });
  for (int i = 0; i < n; ++i) with_err = with_err || results[i].edge_chi2 || results[i].edge_outlier;
  ssx_ba_batch B;
  ssx_status st = batch_build(ctx, n, prs.data(), wins[0]->opt, with_err, false, &B, exts.data());
  if (st == SSX_ERR_UNSUPPORTED) {                   // a window with more than 16 free keyframes: one after the other reports it properly
    for (int i = 0; i < n; ++i) { st = ssx_ba_window_solve(wins[i], &results[i]); if (st != SSX_OK) return st; }
    return SSX_OK;
  }
  if (st != SSX_OK) return st;
  const auto tp2 = std::chrono::steady_clock::now();
  st = batch_run(&B, srs.data(), nullptr);
  if (st != SSX_OK) return st;
  const auto tp3 = std::chrono::steady_clock::now();
  ctx->ba->pool.run(n, std::min(n, host_threads_cap()), [&](int i) {
    ssx_ba_window* w = wins[i];
    w->r_pose.resize(w->poses.size()); w->r_point.resize(w->points.size());
    win_unpack(w, srs[i], &results[i]);
  });
  if (timing) {
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const double t_abs = std::chrono::duration<double, std::milli>(tp0.time_since_epoch()).count();
    fprintf(stderr, "[ssx_ba_window_solve_batch n=%d ctx=%p t0=%.3f] sync %.3f ms, views + marshal + upload %.3f ms, solve + download %.3f ms, unpack %.3f ms\n", n,
            (void*)ctx, fmod(t_abs, 100000.0), ms(tp0, tp1), ms(tp1, tp2), ms(tp2, tp3), ms(tp3, std::chrono::steady_clock::now()));
  }
  return SSX_OK;
}


#ifndef SSX_NO_TEST_HOOKS
// Test hook, needs no GPU: a random sequence of pushes (by id and by slot), pops (any keyframe, not only the oldest), removals of
// single observations (by keyframe + landmark, and by flags in export order), removals of landmarks and estimate overwrites on a
// window without a device, checked after every step against a plain model of what the window must hold -- keyframes ascending
// by id, landmarks ascending by id, the observations in push order, the fixed flags of backend.cpp:125-130 (the model keeps
// every landmark's observer list like MapPoint::observations_ does), index ranges, sizes.  Exercises the id map (insert /
// erase / rehash with tombstones), slot reuse, the id-order list (ids arriving out of order, entries of landmarks that left),
// dead observation blocks, trailing trims and the storage rewrite.  Returns 0, or the number of the step at which the window
// and the model disagree.
int32_t ssx_ba_window_selftest(uint32_t seed, int32_t steps)
{
  ssx_ctx dummy;
  ssx_ba_window* w = new ssx_ba_window();
  w->ctx = &dummy;
  ssx_ba_default_options(&w->opt);
  ssx_ba_window_set_fix_rule(w, 1);
  // two twins receive every edit through ssx_ba_window_update_batch (two windows per call: the threaded path) and must end up
  // exactly like w
  ssx_ba_window* tw[2] = {new ssx_ba_window(), new ssx_ba_window()};
  for (ssx_ba_window* t : tw) { t->ctx = &dummy; ssx_ba_default_options(&t->opt); ssx_ba_window_set_fix_rule(t, 1); }
  auto twins_agree = [&]() {
    for (ssx_ba_window* t : tw)
      if (t->e_pose != w->e_pose || t->e_point != w->e_point || t->e_uv != w->e_uv || t->e_cam != w->e_cam || t->lm_id != w->lm_id ||
          t->lm_alive != w->lm_alive || t->poses != w->poses || t->points != w->points || t->n_dead != w->n_dead ||
          t->lm_first_popped != w->lm_first_popped || t->lm_user_fixed != w->lm_user_fixed)
        return false;
    return true;
  };
  uint64_t rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed << 17) ^ seed;
  auto rnd = [&](uint32_t n) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)((rng >> 11) % (n ? n : 1)); };
  struct Obs { int64_t kf, lm; double u, v; uint8_t cam; };
  struct MLm { bool user_fixed = false; int slot = -1; std::vector<std::pair<int64_t, uint8_t>> observers; };   // MapPoint::observations_: (keyframe, camera) in insertion order
  std::vector<int64_t> m_kf;                                   // model: keyframes in the window
  std::vector<Obs> m_obs;                                      // model: live observations, push order
  std::map<int64_t, MLm> m_lm;                                 // model: landmarks in the window
  int64_t next_kf = 1000, next_lm = 1;
  int32_t bad = 0;
  int n_removed_obs = 0, n_removed_lm = 0, n_fixed_seen = 0;
  // landmarks without a live observation leave the model (the window drops them in the same calls)
  auto model_sweep = [&]() {
    std::unordered_map<int64_t, int> live;
    for (const Obs& o : m_obs) live[o.lm]++;
    for (auto it = m_lm.begin(); it != m_lm.end();) it = live.count(it->first) ? std::next(it) : m_lm.erase(it);
  };
  auto model_remove_obs = [&](int64_t kf, int64_t lm, int cam_mask) {   // cam_mask: bit 0 left, bit 1 right
    int n = 0;
    std::vector<Obs> keep;
    for (const Obs& o : m_obs) {
      if (o.kf == kf && o.lm == lm && (cam_mask & (o.cam ? 2 : 1))) { ++n; continue; }
      keep.push_back(o);
    }
    m_obs.swap(keep);
    auto it = m_lm.find(lm);
    if (it != m_lm.end() && n) {
      auto& ob = it->second.observers;
      ob.erase(std::remove_if(ob.begin(), ob.end(), [&](const std::pair<int64_t, uint8_t>& p) { return p.first == kf && (cam_mask & (p.second ? 2 : 1)); }), ob.end());
    }
    return n;
  };
  for (int32_t step = 1; step <= steps && !bad; ++step) {
    const uint32_t dice = rnd(12);
    const bool do_pop = !m_kf.empty() && (m_kf.size() >= 12 || dice < 3);
    if (!do_pop && dice == 3 && !m_obs.empty()) {
      // ---- outlier observations of one keyframe, by (keyframe, landmark[, camera])
      const Obs pick = m_obs[rnd((uint32_t)m_obs.size())];
      std::vector<int64_t> ids; std::vector<uint8_t> cams;
      for (const Obs& o : m_obs) if (o.kf == pick.kf && (o.lm == pick.lm || rnd(6) == 0)) { ids.push_back(o.lm); cams.push_back(o.cam); }
      ids.push_back(-77);  cams.push_back(0);                             // an id the window does not know: skipped
      const bool with_cam = rnd(2) != 0;
      int32_t got = 0;
      if (ssx_ba_window_remove_observations(w, pick.kf, (int)ids.size(), ids.data(), with_cam ? cams.data() : nullptr, &got) != SSX_OK) { bad = step; break; }
      for (ssx_ba_window* t : tw) if (ssx_ba_window_remove_observations(t, pick.kf, (int)ids.size(), ids.data(), with_cam ? cams.data() : nullptr, nullptr) != SSX_OK) bad = step;
      int want = 0;
      for (size_t i = 0; i + 1 < ids.size(); ++i) want += model_remove_obs(pick.kf, ids[i], with_cam ? (cams[i] ? 2 : 1) : 3);
      model_sweep();
      if (bad || got != want || !twins_agree()) { bad = step; break; }
      n_removed_obs += got;
      if (ssx_ba_window_remove_observations(w, -5, 0, nullptr, nullptr, nullptr) == SSX_OK) { bad = step; break; }   // unknown keyframe: refused
    } else if (!do_pop && dice == 4 && !m_obs.empty()) {
      // ---- outlier observations by flags in export order (ssx_ba_result.edge_outlier handed back), through the batched edit
      std::vector<uint8_t> flags(m_obs.size(), 0);
      for (auto& f : flags) f = rnd(10) == 0;
      int32_t got = 0;
      if (ssx_ba_window_remove_flagged(w, (int)flags.size(), flags.data(), &got) != SSX_OK) { bad = step; break; }
      ssx_ba_window_update up[2] = {};
      up[0].n_remove_flags = up[1].n_remove_flags = (int)flags.size(); up[0].remove_flags = up[1].remove_flags = flags.data();
      if (ssx_ba_window_update_batch(2, tw, up, nullptr) != SSX_OK) { bad = step; break; }
      std::vector<Obs> snapshot = m_obs;
      int want = 0;
      // (one flag per observation: duplicates of a (keyframe, landmark, camera) triple are removed one by one)
      std::vector<Obs> keep;
      for (size_t i = 0; i < snapshot.size(); ++i) {
        if (!flags[i]) { keep.push_back(snapshot[i]); continue; }
        ++want;
        auto it = m_lm.find(snapshot[i].lm);
        auto& ob = it->second.observers;
        for (size_t q = 0; q < ob.size(); ++q) if (ob[q].first == snapshot[i].kf && ob[q].second == snapshot[i].cam) { ob.erase(ob.begin() + q); break; }
      }
      m_obs.swap(keep);
      model_sweep();
      if (got != want || !twins_agree()) { bad = step; break; }
      n_removed_obs += got;
      if (ssx_ba_window_remove_flagged(w, (int)m_obs.size() + 1, flags.data(), nullptr) == SSX_OK) { bad = step; break; }   // wrong count: refused
    } else if (!do_pop && dice == 5 && !m_lm.empty()) {
      // ---- condemned landmarks
      std::vector<int64_t> ids;
      for (const auto& kv : m_lm) if (rnd(40) == 0) ids.push_back(kv.first);
      ids.push_back(-123456);
      int32_t got = 0;
      if (ssx_ba_window_remove_landmarks(w, (int)ids.size(), ids.data(), &got) != SSX_OK) { bad = step; break; }
      ssx_ba_window_update up[2] = {};
      up[0].n_remove_lm = up[1].n_remove_lm = (int)ids.size(); up[0].remove_lm_ids = up[1].remove_lm_ids = ids.data();
      if (ssx_ba_window_update_batch(2, tw, up, nullptr) != SSX_OK) { bad = step; break; }
      std::unordered_map<int64_t, int> gone;
      for (size_t i = 0; i + 1 < ids.size(); ++i) gone[ids[i]] = 1;
      std::vector<Obs> keep;
      for (const Obs& o : m_obs) if (!gone.count(o.lm)) keep.push_back(o);
      m_obs.swap(keep);
      for (const auto& g : gone) m_lm.erase(g.first);
      if (got != (int)ids.size() - 1 || !twins_agree()) { bad = step; break; }
      n_removed_lm += got;
    } else if (do_pop) {
      const size_t which = rnd(4) ? 0 : rnd((uint32_t)m_kf.size());          // mostly the oldest
      const int64_t id = m_kf[which];
      if (ssx_ba_window_pop_keyframe(w, id) != SSX_OK) { bad = step; break; }
      {
        ssx_ba_window_update up[2] = {};
        up[0].pop = up[1].pop = 1; up[0].pop_kf_id = up[1].pop_kf_id = id;
        if (ssx_ba_window_update_batch(2, tw, up, nullptr) != SSX_OK || !twins_agree()) { bad = step; break; }
      }
      m_kf.erase(m_kf.begin() + which);
      std::vector<Obs> keep;
      for (const Obs& o : m_obs) if (o.kf != id) keep.push_back(o);
      m_obs.swap(keep);
      model_sweep();                                            // (the observer lists keep the popped keyframe's entries)
    } else {
      // a keyframe that sees some landmarks already in the window and brings some new ones
      std::vector<int64_t> known;
      for (const auto& kv : m_lm) known.push_back(kv.first);
      const int n_new = (int)rnd(step % 7 == 0 ? 900 : 40), n_old = known.empty() ? 0 : (int)rnd((uint32_t)std::min<size_t>(known.size(), 300) + 1);
      std::vector<int64_t> new_ids, obs_lm; std::vector<double> new_xyz, uv; std::vector<uint8_t> new_fixed, cam; std::vector<int32_t> obs_slot;
      // ids: scrambled inside one push (out of order), growing from push to push; now and then an id BELOW everything (a landmark
      // that comes back into the window: the order list must be sorted again)
      for (int i = 0; i < n_new; ++i) {
        int64_t id = next_lm++ * 7919 % 1000003 + 1000003 * (int64_t)(step);
        if (rnd(50) == 0) id = -(int64_t)(next_lm * 3 + step);
        new_ids.push_back(id); new_xyz.insert(new_xyz.end(), {1.0 * i, 2.0, 3.0 + step}); new_fixed.push_back(rnd(5) == 0);
      }
      const int64_t kf_id = next_kf++;
      for (int i = 0; i < n_new; ++i) { obs_lm.push_back(new_ids[i]); obs_slot.push_back(-1 - i); uv.push_back(10.0 + i); uv.push_back(0.5 * step); cam.push_back(0); }
      for (int i = 0; i < n_old; ++i) {
        const int64_t lm = known[rnd((uint32_t)known.size())];
        obs_lm.push_back(lm); obs_slot.push_back(m_lm[lm].slot); uv.push_back(700.0 + i); uv.push_back(-1.0 * step); cam.push_back(i & 1);
      }
      if (rnd(9) == 0 && n_new) { obs_lm.push_back(new_ids[0]); obs_slot.push_back(-1); uv.push_back(3.25); uv.push_back(4.5); cam.push_back(1); }   // the right-camera twin
      const double pose[7] = {0, 0, 0, 1, 0.1 * step, 0, 0};
      std::vector<int32_t> slots((size_t)n_new + 1);
      ssx_status st;
      if (step & 1) st = ssx_ba_window_push_keyframe(w, kf_id, pose, 0, n_new, new_ids.data(), new_xyz.data(), new_fixed.data(), (int)obs_lm.size(), obs_lm.data(), uv.data(), cam.data());
      else st = ssx_ba_window_push_keyframe_slots(w, kf_id, pose, 0, n_new, new_ids.data(), new_xyz.data(), new_fixed.data(), slots.data(), (int)obs_slot.size(), obs_slot.data(), uv.data(), cam.data());
      if (st != SSX_OK) { bad = step; break; }
      {
        std::vector<int32_t> tslots[2] = {std::vector<int32_t>((size_t)n_new + 1), std::vector<int32_t>((size_t)n_new + 1)};
        ssx_ba_window_update up[2] = {};
        for (int q = 0; q < 2; ++q) {
          up[q].push = 1; up[q].kf_id = kf_id; up[q].pose7 = pose; up[q].n_new = n_new; up[q].new_ids = new_ids.data(); up[q].new_xyz = new_xyz.data();
          up[q].new_fixed = new_fixed.data(); up[q].n_obs = (int)obs_lm.size(); up[q].obs_uv = uv.data(); up[q].obs_cam = cam.data();
          if (step & 1) up[q].obs_lm = obs_lm.data(); else { up[q].obs_slot = obs_slot.data(); up[q].new_slots_out = tslots[q].data(); }
        }
        ssx_status sts[2] = {SSX_OK, SSX_OK};
        if (ssx_ba_window_update_batch(2, tw, up, sts) != SSX_OK || sts[0] != SSX_OK || sts[1] != SSX_OK || !twins_agree()) { bad = step; break; }
        if ((step & 1) == 0) for (int i = 0; i < n_new; ++i) if (tslots[0][i] != slots[i] || tslots[1][i] != slots[i]) { bad = step; break; }
        if (bad) break;
        // the same window twice in one call is refused and changes nothing
        ssx_ba_window* same[2] = {tw[0], tw[0]};
        up[0].kf_id = up[1].kf_id = kf_id + 1000000;
        if (ssx_ba_window_update_batch(2, same, up, nullptr) == SSX_OK || !twins_agree()) { bad = step; break; }
      }
      // a push that must fail changes nothing
      if (ssx_ba_window_push_keyframe(w, kf_id, pose, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SSX_OK) { bad = step; break; }
      m_kf.push_back(kf_id);
      for (int i = 0; i < n_new; ++i) {
        MLm& m = m_lm[new_ids[i]];
        m.user_fixed = new_fixed[i] != 0;
        m.slot = (step & 1) ? w->lm_slot.find(new_ids[i]) : slots[i];
      }
      for (size_t i = 0; i < obs_lm.size(); ++i) {
        m_obs.push_back(Obs{kf_id, obs_lm[i], uv[2 * i], uv[2 * i + 1], cam[i]});
        m_lm[obs_lm[i]].observers.emplace_back(kf_id, cam[i]);
      }
      if ((step & 1) == 0) for (int i = 0; i < n_new; ++i) if (w->lm_slot.find(new_ids[i]) != slots[i]) { bad = step; break; }
      model_sweep();                                            // (a new landmark nobody observes is legal to push; the model keeps only observed ones ...
    }
    if (bad) break;
    // ---- compare: sizes, then the export, entry by entry
    int nk = 0, nl = 0, no = 0;
    ssx_ba_window_size(w, &nk, &nl, &no);
    // ... and the window keeps it until something removes it: count those through the window's own table)
    std::vector<int64_t> unobserved;
    for (size_t l = 0; l < w->lm_id.size(); ++l) if (w->lm_alive[l] && w->lm_obs[l] == 0) unobserved.push_back(w->lm_id[l]);
    if (nk != (int)m_kf.size() || no != (int)m_obs.size() || nl != (int)m_lm.size() + (int)unobserved.size()) { bad = step; break; }
    std::vector<int64_t> kf_ids((size_t)nk + 1), lm_ids((size_t)nl + 1);
    std::vector<int32_t> ep((size_t)no + 1), el((size_t)no + 1);
    std::vector<double> euv(2 * (size_t)no + 2); std::vector<uint8_t> ecam((size_t)no + 1), pfx((size_t)nl + 1);
    ssx_ba_window_export(w, kf_ids.data(), nullptr, nullptr, lm_ids.data(), nullptr, pfx.data(), ep.data(), el.data(), euv.data(), ecam.data());
    std::vector<int64_t> b = m_kf;
    std::sort(b.begin(), b.end());
    if (std::vector<int64_t>(kf_ids.begin(), kf_ids.begin() + nk) != b) { bad = step; break; }          // ascending by id
    std::vector<int64_t> want_lm;
    for (const auto& kv : m_lm) want_lm.push_back(kv.first);
    want_lm.insert(want_lm.end(), unobserved.begin(), unobserved.end());
    std::sort(want_lm.begin(), want_lm.end());
    if (std::vector<int64_t>(lm_ids.begin(), lm_ids.begin() + nl) != want_lm) { bad = step; break; }     // ascending by id
    for (int e = 0; e < no && !bad; ++e) {                                                                  // push order
      if (ep[e] < 0 || ep[e] >= nk || el[e] < 0 || el[e] >= nl) { bad = step; break; }
      const Obs& o = m_obs[e];
      if (kf_ids[ep[e]] != o.kf || lm_ids[el[e]] != o.lm || euv[2 * (size_t)e] != o.u || euv[2 * (size_t)e + 1] != o.v || ecam[e] != o.cam) bad = step;
    }
    if (bad) break;
    // the fixed flags: the caller's, or the keyframe of the first remaining observation is no longer in the window
    for (int l = 0; l < nl && !bad; ++l) {
      auto it = m_lm.find(lm_ids[l]);
      if (it == m_lm.end()) continue;                                                                        // unobserved
      const MLm& m = it->second;
      const bool front_in = !m.observers.empty() && std::find(m_kf.begin(), m_kf.end(), m.observers.front().first) != m_kf.end();
      const bool want = m.user_fixed || !front_in;
      if ((pfx[l] != 0) != want) bad = step;
      if (want && !m.user_fixed) ++n_fixed_seen;
    }
    if (bad) break;
    // the window's own pass agrees with the export's, and the order lists a solve would use are consistent
    {
      ssx_ba_problem pr;
      win_view(w, &pr);
      for (int l = 0; l < nl && !bad; ++l) { const int ls = w->lm_slot.find(lm_ids[l]); if (ls < 0 || w->ord_lm[l] != ls || pr.point_fixed[ls] != pfx[l]) bad = step; }
      for (int k = 0; k < nk && !bad; ++k) if (w->kf[w->ord_kf[k]].id != kf_ids[k]) bad = step;
    }
    // the id map agrees with the slots
    for (size_t l = 0; l < w->lm_id.size() && !bad; ++l) if (w->lm_alive[l] && (w->lm_slot.find(w->lm_id[l]) != (int)l || w->lm_order[w->lm_pos[l]].second != (int)l)) bad = step;
  }
  // the run must have covered the storage rewrite, both kinds of removal and landmarks fixed by the rule
  if (!bad && steps >= 300 && (w->n_rewrites == 0 || w->lm_slot.keys.size() < 1024 || n_removed_obs == 0 || n_removed_lm == 0 || n_fixed_seen == 0)) bad = -1;
  delete w;
  for (ssx_ba_window* t : tw) delete t;
  if (dummy.ba && dummy.ba_free) { dummy.ba_free(dummy.ba); dummy.ba = nullptr; }   // (the update batches created the ctx's worker pool)
  return bad;
}
#endif  // SSX_NO_TEST_HOOKS

}  // extern "C"
