// ssvio_amd/csrc/ctx.hpp -- ssx_ctx: one GPU, one HIP stream, grow-only scratch arenas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ssx.h"

// Wrap a kernel launch: when profiling is on, bracket it with two HIP events on the ctx stream.
#define SSX_PROF(ctx, kid, stmt)                                              \
  do {                                                                        \
    if ((ctx)->prof.on) {                                                     \
      SsxProf::Rec _r{(kid), (ctx)->prof.get(), (ctx)->prof.get()};           \
      (void)hipEventRecord(_r.a, (ctx)->stream);                              \
      stmt;                                                                   \
      (void)hipEventRecord(_r.b, (ctx)->stream);                              \
      (ctx)->prof.recs.push_back(_r);                                         \
    } else {                                                                  \
      stmt;                                                                   \
    }                                                                         \
  } while (0)

#define SSX_PROF_ON(ctx, strm, kid, stmt)                                     \
  do {                                                                        \
    if ((ctx)->prof.on) {                                                     \
      SsxProf::Rec _r{(kid), (ctx)->prof.get(), (ctx)->prof.get()};           \
      (void)hipEventRecord(_r.a, (strm));                                     \
      stmt;                                                                   \
      (void)hipEventRecord(_r.b, (strm));                                     \
      (ctx)->prof.recs.push_back(_r);                                         \
    } else {                                                                  \
      stmt;                                                                   \
    }                                                                         \
  } while (0)

#define SSX_HIP_TRY(ctx, expr)                                                                  \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (ctx)->set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));    \
      return SSX_ERR_HIP;                                                                       \
    }                                                                                           \
  } while (0)

// A device buffer that only ever grows (288 GB of HBM: keep scratch resident between calls instead of
// paying hipMalloc/hipFree on the hot path).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  // (grow = what a reallocation asks for, in units of the request: a hipFree synchronises the whole device)
  hipError_t reserve(size_t bytes, double grow = 1.25)
  {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = (size_t)((double)bytes * grow) + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Pinned host staging buffer (async H2D/D2H without the runtime's bounce copy).
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes, double grow = 1.25)
  {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    size_t want = (size_t)((double)bytes * grow) + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// bump allocator for carving one arena into 256-byte aligned sub-buffers
struct Layout {
  size_t off = 0;
  size_t take(size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; }
};
// a buffer's pointer, whatever its type, from the base of its block and its offset
template <class T> void wire(T*& ptr, char* base, size_t off) { ptr = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off); }
// The buffers of one block, each stated ONCE: `each(f)` calls f(pointer, bytes) for every buffer in memory order.  Wires the pointers
// from `base` (null: offsets only, to size the block before it is reserved) and returns the bytes the block takes.
template <class Each> size_t carve(char* base, Each&& each) { Layout lay; each([&](auto*& ptr, size_t bytes) { wire(ptr, base, lay.take(bytes)); }); return lay.off; }

// ---- per-kernel timing with HIP events on the ctx stream (ssx_profile_begin / ssx_profile_end) ----
enum SsxKernelId {
  KID_BA_LINEARIZE = 0, KID_BA_REDUCE_LIN, KID_BA_SCHUR, KID_BA_REDUCE_SCHUR, KID_BA_SOLVE, KID_BA_BACKSUB,
  KID_BA_REDUCE_TRIAL, KID_ORB_RESIZE, KID_ORB_FAST, KID_ORB_OCTREE, KID_ORB_ORIENT, KID_ORB_GAUSS, KID_ORB_BRIEF,
  KID_ORB_MISC, KID_ST_BUCKET, KID_ST_MATCH, KID_ST_TRIANGULATE, KID_ST_MISC, KID_POSE_ONLY, KID_BA_COMM, KID_BA_LIN_SCHUR,
  KID_LOOP_SCORE, KID_LOOP_MATCH, KID_LOOP_PAIRS, KID_PNP_RANSAC, KID_LOOP_COMPACT, KID_LOOP_WORDS, KID_LOOP_BOW, KID_LOOP_COMMIT,
  KID_LC_KEYFRAMES, KID_LC_REANCHOR, KID_WIN_ANCHOR, KID_LOOP_TOPK, KID_LOOP_GUIDED, KID_UNDISTORT, KID_UNDISTORT_MAP,
  KID_UNDISTORT_REMAP, KID_DENSE_CENSUS, KID_DENSE_PATHS, KID_DENSE_RIGHT, KID_DENSE_SELECT,
  KID_DENSE_LABEL_TILE, KID_DENSE_LABEL_MERGE, KID_DENSE_LABEL_COUNT, KID_DENSE_SPECKLE, KID_DENSE_SAMPLE_ROWS, KID_DENSE_SAMPLE_WRITE, KID_COUNT
};
static const char* const kSsxKernelNames[KID_COUNT] = {
  "k_linearize", "k_reduce_lin", "k_schur", "k_reduce_schur", "k_solve", "k_backsub_residual", "k_reduce_trial",
  "k_resize", "k_fast_cells", "k_octree", "k_orient", "k_gauss7", "k_orient_brief", "orb_misc", "k_row_bucket", "k_match",
  "k_triangulate_matches", "stereo_misc", "k_pose_only", "ba_allreduce", "k_lin_schur",
  "k_kfdb_score", "kfdb_bf_match", "k_kfdb_pairs", "k_pnp_ransac", "k_kf_compact", "kf_voc_words", "k_kf_bow", "k_kfdb_commit",
  "k_lc_keyframes", "k_reanchor_points", "k_win_anchor", "k_kfdb_topk", "kfdb_guided", "k_undistort", "k_undistort_map",
  "k_undistort_remap", "k_dense_census", "k_dense_paths", "k_dense_right", "k_dense_select",
  "k_dense_label_tile", "k_dense_label_merge", "k_dense_label_count", "k_dense_speckle", "k_dense_sample_rows", "k_dense_sample_write"};

struct SsxProf {
  bool on = false;
  struct Rec { int id; hipEvent_t a, b; };
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<Rec> recs;
  hipEvent_t get()
  {
    if (used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
    return pool[used++];
  }
};

// what one call of the keyframe database's chain (loop.hip) issued: of a step or a query in its database, of a batch in the context
struct KfChainStats { int32_t launches = 0, syncs = 0; int64_t bytes_up = 0, bytes_down = 0; };

struct BaWorkspace;   // ba.hip
struct OrbWorkspace;  // orb.hip

struct ssx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 256;
  uint32_t cu_mask[16] = {0};                // ssx_config.cu_first / cu_count as a bit mask; cu_mask_words == 0: no mask
  int cu_mask_words = 0;
  // every stream the ctx creates: CU-masked when the ctx is, lowest priority on request
  hipError_t make_stream(hipStream_t* out, bool low_priority)
  {
    if (cu_mask_words > 0) return hipExtStreamCreateWithCUMask(out, (uint32_t)cu_mask_words, cu_mask);
    if (low_priority) {
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (hipStreamCreateWithPriority(out, hipStreamNonBlocking, least) == hipSuccess) return hipSuccess;
      (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  }
  char err[512] = {0};
  BaWorkspace* ba = nullptr;
  OrbWorkspace* orb = nullptr;
  void (*ba_free)(BaWorkspace*) = nullptr;    // set by the module that allocates the workspace
  void (*orb_free)(OrbWorkspace*) = nullptr;
  void* lk = nullptr;                        // lk.hip workspace
  void (*lk_free)(void*) = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t aux = nullptr;                 // second stream: independent stages overlap (blur || detect)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_pyr = nullptr, ev_fast0 = nullptr;
  hipStream_t grp[3] = {nullptr, nullptr, nullptr};   // batched BA: the groups of windows beside the main stream (created on first use)
  hipEvent_t grp_ev[3] = {nullptr, nullptr, nullptr};
  int ba_batch_groups = 0;                   // ssx_ba_set_batch_groups: groups of windows of this ctx's one-shot batched solves (0: the default)
  SsxProf prof;
  DevBuf po_arena;                           // pose-only optimisation scratch
  HostBuf po_stage;
  DevBuf pnp_arena;                          // loop closing's pose correction (pnp.hip)
  HostBuf pnp_stage;
  KfChainStats kf_batch;                     // the last ssx_kfdb_process_keyframe_batch (ssx_kfdb_debug_last_batch)
  DevBuf ud_arena;                           // image undistortion (undistort.hip): the job table and, for host images, the staged images
  HostBuf ud_stage;
  struct UdStats : KfChainStats { int32_t copies_up = 0, copies_down = 0; } undistort;   // the last ssx_undistort* (ssx_undistort_debug_last_call reports the four)
  DevBuf dn_arena, dn_work;                  // dense stereo (dense.hip): the job table and staged images / maps; census, volume and right keys of a group
  HostBuf dn_stage;
  KfChainStats dense;                        // the last ssx_stereo_dense / ssx_stereo_dense_post / ssx_dense_postprocess (ssx_dense_debug_last_call)
  int32_t dense_groups = 0;
#ifndef SSX_NO_TEST_HOOKS
  uint64_t dense_cap = 0;                    // ssx_dense_debug_set_workspace_cap: the cap the dense calls group by; 0 = SSX_DENSE_WORKSPACE_CAP
#endif

  std::mutex err_mu;                         // worker threads of a batched call may report failures concurrently

  void set_error(const char* fmt, ...)
  {
    std::lock_guard<std::mutex> lk(err_mu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof(err), fmt, ap);
    va_end(ap);
  }
};

