// ssvio_amd/host/stream_batcher.cpp -- see stream_batcher.hpp: the request kinds (what a stream files, what a call's jobs must share,
// the library call) and the three adapters that file them; who is served when is batch_dispatch.hpp
#include "stream_batcher.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <tuple>

#include "../../include/ssx_shim.hpp"
#include "batch_dispatch.hpp"

namespace ssx::host {

namespace {
enum Kind : int { LK, PO, DET, LKS, TRI, BA, LOOP, CALL, UND, RELOC, POSES, N_KINDS };   // indices into the table of Impl::Kinds
// what the jobs of one call share -- the keys of Groups
struct ImageSize {
  int rows = 0, cols = 0;
  bool operator==(const ImageSize& o) const { return rows == o.rows && cols == o.cols; }
  bool operator<(const ImageSize& o) const { return std::tie(rows, cols) < std::tie(o.rows, o.cols); }
};
using OrbParamBytes = std::array<unsigned char, sizeof(ssx_orb_params)>;   // (extractor settings are equal when their bytes are)
OrbParamBytes Bytes(const ssx_orb_params& p)
{
  OrbParamBytes b;
  std::memcpy(b.data(), &p, sizeof p);
  return b;
}
// the per-slot requests
struct LkReq { ssx_lk_job job{}; ImageSize size; };   // temporal and stereo LK
struct DetReq { ssx_orb_detect_job job{}; ssx_orb_params prm{}; ImageSize size; };
struct BaReq { ssx_ba_window* win = nullptr; ssx_ba_result* res = nullptr; };
// a frame's pair through the lenses' maps: two jobs (left, right) of one request, raw images and results in the stream's pinned buffers
struct UndReq { const uint8_t* src[2] = {nullptr, nullptr}; uint8_t* dst[2] = {nullptr, nullptr}; ssx_lens_params prm[2] = {}; ImageSize size; };   // (an undistortion request: its RADTAN lenses)
// one keyframe step of loop closing as a stream files it (ssx_kfdb_process_keyframe_batch): the job and what a call's jobs must share
struct LoopReq { ssx_kfdb_step_job job{}; ssx_orb_params prm{}; ImageSize size; int levels = 0, min_db = 0, min_gap = 0; float threshold = 0.f; int32_t status = 0; };
// the candidate query of a stream that lost tracking (ssx_kfdb_relocalize_query_batch), in the same form
struct RelocReq { ssx_reloc_query_job job{}; ssx_orb_params prm{}; ImageSize size; int levels = 0, candidates = 0; float threshold = 0.f, ratio = 0.f; int32_t status = 0; };
// the pose jobs of that stream's candidates (ssx_pnp_pose_batch): the jobs of a call share the intrinsics
struct PosesReq { const double* K4 = nullptr; std::vector<ssx_pnp_pose_job>* jobs = nullptr; };
using K4Bytes = std::array<unsigned char, 4 * sizeof(double)>;
}

struct StreamBatcher::Impl {
  // Request slots (batch_dispatch.hpp): k < S is stream k's own thread; S + k is the worker thread of stream k's backend when the
  // backend is asynchronous (Backend.Async: 1 -- it files window solves while the stream's thread goes on tracking).
  // The two dispatchers.  Per frame, pose-only first: the cohort then reaches its next LK request where a straggler from a keyframe
  // already waits (see the header).  The keyframe path of the streams (FrontEnd::DetectFeatures -> FindFeaturesInRight ->
  // TriangulateNewPoints -> Backend: masked detection, stereo LK, triangulation, window optimisation) is batched like the per-frame
  // calls, on contexts of its own beside them.  The EARLIEST stage that has requests is served first, so that streams which reached
  // their keyframe a little later catch up and all of them meet in one window solve (a batched solve costs what a single one costs).
  // The loop step follows the window solve inside the backend: served after it, the streams that solved a little later merge into one
  // loop call; the rare single calls of a correction come last.
  // Relocalisation (a lost stream's candidate query, then the poses of its candidates) stands at the very beginning of a frame and is
  // served first, the query before the poses: streams that lose tracking at the same frame meet in one query and then in one pose call.
  // Both run on the loop context and so belong to this dispatcher, never beside a loop step or a correction's call.  The front-end's
  // thread files them from its own slot while it holds the stream's map mutex; its backend's slot may be blocked on that mutex, but a
  // backend slot that is not filing rests IDLE, which the rest condition does not wait for, so the rule stands as it is
  // (tests/host/test_reloc_dispatch_units.cpp).
  // Undistortion (Camera.NeedUndistortion) is the first call of a frame and is served LAST of the per-frame kinds, by the reasoning of
  // the header's "pose-only before LK": the later stage first, so that the cohort arrives where a straggler waits.
  Impl(int device_, int streams) : device(device_), S(streams), po_ctx(device_), ba_ctx(device_), det_ctx(device_), tri_ctx(device_), lk_req(streams),
                                   po_req(streams), det_req(streams), tri_req(streams), ba_req(2 * (size_t)streams), loop_req(2 * (size_t)streams),
                                   call_req(2 * (size_t)streams, nullptr), und_req(streams), reloc_req(2 * (size_t)streams), poses_req(2 * (size_t)streams),
                                   core(streams, Kinds(), {{PO, LK, UND}, false, false}, {{RELOC, POSES, DET, LKS, TRI, BA, LOOP, CALL}, true, true})
  {
  }
  ~Impl()
  {
    // (the streams have finished: the dispatchers, which stop with `core`, are idle)
    if (voc) ssx_voc_destroy(voc);                  // (the streams' databases went with their Systems)
    ssx_host_free(pin_arena);
    ssx_host_free(raw_arena);
  }

  // The cohort's loop context and its ONE vocabulary, loaded when the first stream asks for them (128 streams with a vocabulary each
  // would hold 128 copies of ORBvoc in HBM); every stream's keyframe database lives on that context.
  ssx_kf_database* MakeLoopDatabase(const std::string& voc_path)
  {
    std::lock_guard<std::mutex> lk(loop_mu);
    if (!loop_ctx) {
      auto ctx = std::make_unique<ssx::Context>(device);
      ssx_vocabulary* v = nullptr;
      if (ssx_voc_load_text(ctx->get(), voc_path.c_str(), &v) != SSX_OK)
        throw std::runtime_error("DBOW2.VOC.Path: cannot read the vocabulary \"" + voc_path + "\": " + ssx_last_error(ctx->get()));
      loop_ctx = std::move(ctx); voc = v; loop_voc_path = voc_path;
    } else if (voc_path != loop_voc_path) {
      throw std::runtime_error("DBOW2.VOC.Path: the streams of a batched cohort share one vocabulary, \"" + loop_voc_path + "\" is loaded and \"" + voc_path +
                               "\" was asked for");
    }
    ssx_kf_database* db = nullptr;
    loop_ctx->check(ssx_kfdb_create(loop_ctx->get(), 256, &db));
    return db;
  }

  // The LK contexts of ONE image size: `lk` for the frame-to-frame chains, `lks` for the left-right calls of a keyframe, slot k of
  // either for stream k.  An LK context holds chains for one (rows, cols, window, max_level) at a time and a call of another size
  // drops them all (include/ssx.h, ssx_lk_track_next), so the streams of a cohort that differ in image size (KITTI 00 at 1241 x 376
  // beside KITTI 04 at 1226 x 370) cannot take turns on one context: every size has a pair of its own, made when its first request
  // is served.  A cohort of n sizes costs n LK calls per frame instead of one; the streams of one size still travel together.
  struct SizeCtx {
    explicit SizeCtx(int device) : lk(device), lks(device) {}
    ssx::Context lk, lks;
  };
  SizeCtx& ForSize(ImageSize size)
  {
    std::lock_guard<std::mutex> lk(size_mu);        // (both dispatchers come here)
    std::unique_ptr<SizeCtx>& p = size_ctx[size];
    if (!p) p = std::make_unique<SizeCtx>(device);
    return *p;
  }

  // The undistortion plan of ONE image size on a context of its own (the grouping key of the request, as for LK): the stored maps of the
  // cameras its streams showed it -- a cohort of one rig has two -- made when the size's first request is served.
  struct UndSize {
    UndSize(int device, ImageSize size) : ctx(device) { ctx.check(ssx_undistort_plan_create(ctx.get(), size.rows, size.cols, &plan)); }
    ~UndSize() { ssx_undistort_plan_destroy(plan); }
    ssx::Context ctx;
    ssx_undistort_plan* plan = nullptr;
  };
  UndSize& ForUndSize(ImageSize size)
  {
    std::lock_guard<std::mutex> lk(size_mu);
    std::unique_ptr<UndSize>& p = und_size[size];
    if (!p) p = std::make_unique<UndSize>(device, size);
    return *p;
  }

  // The streams' pinned image buffers are slices of ONE arena: buffer `which` of stream k at (which * S + k) * slice, the slice sized
  // by the stream that pins first.  Buffers 0 and 1 are the images the calls read (BatchedCompute::Pinned).  Buffers 2 and 3 take a
  // frame's raw pair when the images go through undistortion first, whose results are then written into 0 and 1; they are slices
  // of a second arena of the same shape, made when the first stream undistorts (a cohort that does not pins nothing more).  The `next` images of a cohort's LK jobs then lie at a constant distance in one allocation and
  // cross PCIe in one DMA copy (ssx_lk_track_batch).  In a cohort of several image sizes a stream with SMALLER images than the
  // first one uses its slice all the same (the images of its size are then further apart than the one-copy rule allows and are read
  // one by one); a stream with LARGER images gets nullptr and keeps two pinned buffers of its own (BatchedCompute::Pinned), which
  // the library takes one by one wherever the allocator put them.
  uint8_t* PinSlice(int k, int which, size_t bytes)
  {
    std::lock_guard<std::mutex> lk(pin_mu);
    const size_t need = (bytes + 255) & ~size_t(255);
    if (!pin_arena) {
      pin_slice = need;
      pin_arena = static_cast<uint8_t*>(ssx_host_alloc(pin_slice * 2 * (size_t)S));
      if (!pin_arena) throw std::runtime_error("StreamBatcher: no pinned memory for the streams' images");
    }
    if (need > pin_slice) return nullptr;
    if (which < 2) return pin_arena + ((size_t)which * S + k) * pin_slice;
    if (!raw_arena) raw_arena = static_cast<uint8_t*>(ssx_host_alloc(pin_slice * 2 * (size_t)S));
    if (!raw_arena) throw std::runtime_error("StreamBatcher: no pinned memory for the streams' raw images");
    return raw_arena + ((size_t)(which - 2) * S + k) * pin_slice;
  }

  // A kind's callable: the requests of a dispatch in groups of equal key(slot), one library call per group -- call(slots, errs), errs[j]
  // for slots[j] -- and job by job where a call is rejected (Isolated)
  template <class Key, class Call>
  static auto Grouped(Key key, Call call)
  {
    return [key, call](const std::vector<int>& who, std::vector<std::string>& errs, long& calls, long& jobs) {
      std::vector<decltype(key(0))> keys;
      for (int k : who) keys.push_back(key(k));
      for (const auto& g : Groups(keys))
        Isolated(g, errs, calls, jobs, [&](const std::vector<size_t>& sub) {
          std::vector<int> slots;
          for (size_t i : sub) slots.push_back(who[i]);
          std::vector<std::string> e(sub.size());
          call(slots, e);
          for (size_t j = 0; j < sub.size(); ++j) if (!e[j].empty()) errs[sub[j]] = e[j];
        });
    };
  }
  static int NoKey(int) { return 0; }

  std::vector<BatchDispatch::Kind> Kinds()
  {
    using Slots = const std::vector<int>&;
    using Errs = std::vector<std::string>&;
    // (jobs of one call share the image size: the streams of another size go in a call of their own, on that size's context -- their
    // chains live there)
    auto lk_size = [this](int k) { return lk_req[k].size; };
    auto lk_call = [this](bool stereo) {
      return [this, stereo](Slots slots, Errs) {
        const ImageSize size = lk_req[slots[0]].size;
        SizeCtx& sc = ForSize(size);
        ssx::Context& ctx = stereo ? sc.lks : sc.lk;
        std::vector<ssx_lk_job> jobs;
        for (int k : slots) jobs.push_back(lk_req[k].job);
        ssx_lk_params p;
        ssx_lk_default_params(&p);
        p.win = 11; p.max_level = 3; p.max_iters = 30; p.eps = 0.01; p.use_initial_flow = 1;
        ctx.check(ssx_lk_track_batch(ctx.get(), (int32_t)jobs.size(), jobs.data(), size.rows, size.cols, &p, 1));
      };
    };
    std::vector<BatchDispatch::Kind> t(N_KINDS);
    t[LK] = {"temporal LK", Grouped(lk_size, lk_call(false))};
    t[LKS] = {"stereo LK", Grouped(lk_size, lk_call(true))};
    t[PO] = {"pose-only", Grouped(NoKey, [this](Slots slots, Errs) {
      std::vector<ssx_pose_only_job> jobs;
      for (int k : slots) jobs.push_back(po_req[k]);
      po_ctx.check(ssx_pose_only_opt_batch(po_ctx.get(), (int32_t)jobs.size(), jobs.data()));
    })};
    // detection: the jobs of a call share image size, stride and extractor settings
    t[DET] = {"detection", Grouped([this](int k) { return std::make_tuple(det_req[k].size, det_req[k].job.stride, Bytes(det_req[k].prm)); }, [this](Slots slots, Errs) {
      std::vector<ssx_orb_detect_job> jobs;
      for (int k : slots) jobs.push_back(det_req[k].job);
      const DetReq& r0 = det_req[slots[0]];
      const ssx_status rc = ssx_orb_detect_boxes_batch(det_ctx.get(), (int32_t)jobs.size(), jobs.data(), r0.size.rows, r0.size.cols, &r0.prm, 1);
      // (SSX_ERR_CAPACITY is per image -- the other images of the call are complete: every stream looks at its own count)
      if (rc != SSX_ERR_CAPACITY) det_ctx.check(rc);
    })};
    t[TRI] = {"triangulation", Grouped(NoKey, [this](Slots slots, Errs) {
      std::vector<ssx_triangulate_job> jobs;
      for (int k : slots) jobs.push_back(tri_req[k]);
      tri_ctx.check(ssx_triangulate_batch(tri_ctx.get(), (int32_t)jobs.size(), jobs.data()));
    })};
    t[BA] = {"window solve", Grouped(NoKey, [this](Slots slots, Errs) {
      std::vector<ssx_ba_window*> wins;
      std::vector<ssx_ba_result> res;
      for (int k : slots) { wins.push_back(ba_req[k].win); res.push_back(*ba_req[k].res); }
      ba_ctx.check(ssx_ba_window_solve_batch((int32_t)wins.size(), wins.data(), res.data()));
      for (size_t j = 0; j < slots.size(); ++j) *ba_req[slots[j]].res = res[j];
    })};
    auto loop_key = [this](int k) {
      const LoopReq& r = loop_req[k];
      return std::make_tuple(r.size, r.job.stride, Bytes(r.prm), r.levels, r.min_db, r.min_gap, r.threshold);
    };
    t[LOOP] = {"loop step", Grouped(loop_key, [this](Slots slots, Errs errs) {
      std::vector<ssx_kfdb_step_job> jobs;
      for (int k : slots) { LoopReq& r = loop_req[k]; r.status = SSX_OK; r.job.status_out = &r.status; jobs.push_back(r.job); }
      const LoopReq& r0 = loop_req[slots[0]];
      const ssx_status rc = ssx_kfdb_process_keyframe_batch(voc, (int32_t)jobs.size(), jobs.data(), r0.size.rows, r0.size.cols, &r0.prm, r0.levels, r0.min_db,
                                                            r0.min_gap, r0.threshold, 1);
      if (rc == SSX_OK) return;
      // The call returns the first job status that is not SSX_OK: a return value that one of the jobs carries is that job's own
      // outcome, the other jobs are complete (SSX_ERR_CAPACITY: the stream asks again with the room the count names).  Any other
      // value is a failure of the whole call.
      bool per_job = false;
      for (int k : slots) per_job = per_job || loop_req[k].status == (int32_t)rc;
      const std::string why = ssx_last_error(loop_ctx->get());
      if (per_job) {
        for (size_t j = 0; j < slots.size(); ++j) {
          const int32_t js = loop_req[slots[j]].status;
          if (js != SSX_OK && js != SSX_ERR_CAPACITY) errs[j] = "ssx_kfdb_process_keyframe_batch: job status " + std::to_string(js) + ": " + why;
        }
        return;
      }
      // a HIP error: the library had begun (commits may be lost, nothing is pending any more), so no job of the call has a result and
      // none is tried again; every stream of the call gets the error, and its AddPending stays unserved
      if (rc == SSX_ERR_HIP) {
        for (std::string& e : errs) e = "ssx_kfdb_process_keyframe_batch: " + why;
        return;
      }
      loop_ctx->check(rc);                          // rejected before anything was touched: Isolated tries the jobs one by one
    })};
    // the candidate query of the lost streams: the jobs of a call share image size, stride, extractor settings, levels, candidates,
    // threshold and ratio; statuses and errors as the loop step's
    auto reloc_key = [this](int k) {
      const RelocReq& r = reloc_req[k];
      return std::make_tuple(r.size, r.job.stride, Bytes(r.prm), r.levels, r.candidates, r.threshold, r.ratio);
    };
    t[RELOC] = {"relocalisation query", Grouped(reloc_key, [this](Slots slots, Errs errs) {
      static const std::string who = "ssx_kfdb_relocalize_query_batch: ";
      std::vector<ssx_reloc_query_job> jobs;
      for (int k : slots) { RelocReq& r = reloc_req[k]; r.status = SSX_OK; r.job.status_out = &r.status; jobs.push_back(r.job); }
      const RelocReq& r0 = reloc_req[slots[0]];
      const ssx_status rc = ssx_kfdb_relocalize_query_batch(voc, (int32_t)jobs.size(), jobs.data(), r0.size.rows, r0.size.cols, &r0.prm, r0.levels, r0.candidates,
                                                            r0.threshold, r0.ratio, 1);
      if (rc == SSX_OK) return;
      bool per_job = false;                         // (the rule of the loop step: a return value that a job carries is that job's own outcome)
      for (int k : slots) per_job = per_job || reloc_req[k].status == (int32_t)rc;
      const std::string why = ssx_last_error(loop_ctx->get());
      if (per_job) {
        for (size_t j = 0; j < slots.size(); ++j) {
          const int32_t js = reloc_req[slots[j]].status;
          if (js != SSX_OK && js != SSX_ERR_CAPACITY) errs[j] = who + "job status " + std::to_string(js) + ": " + why;
        }
        return;
      }
      if (rc == SSX_ERR_HIP) {                      // the library had begun: no job of the call has a result and none is tried again
        for (std::string& e : errs) e = who + why;
        return;
      }
      loop_ctx->check(rc);                          // rejected before anything was touched: Isolated tries the jobs one by one
    })};
    // the poses of the lost streams' candidates: packed into calls by PackPoseCalls, the out fields copied back to each requester's jobs;
    // a call that is refused goes once more part by part, so that only the request at fault gets the error
    t[POSES] = {"relocalisation poses", [this](Slots slots, Errs errs, long& calls, long& jobs) {
      std::vector<int> counts;
      std::vector<K4Bytes> keys;
      for (int k : slots) {
        counts.push_back((int)poses_req[k].jobs->size());
        K4Bytes b;
        std::memcpy(b.data(), poses_req[k].K4, b.size());
        keys.push_back(b);
      }
      for (const PoseCall& pc : PackPoseCalls(counts, keys, SSX_PNP_BATCH_MAX)) {
        std::vector<size_t> parts(pc.size());
        for (size_t i = 0; i < parts.size(); ++i) parts[i] = i;
        std::vector<std::string> part_errs(pc.size());
        long unused_calls = 0, unused_jobs = 0;
        Isolated(parts, part_errs, unused_calls, unused_jobs, [&](const std::vector<size_t>& sub) {
          std::vector<ssx_pnp_pose_job> packed;
          for (size_t i : sub) {
            const std::vector<ssx_pnp_pose_job>& src = *poses_req[slots[pc[i].request]].jobs;
            packed.insert(packed.end(), src.begin() + pc[i].first, src.begin() + pc[i].first + pc[i].count);
          }
          loop_ctx->check(ssx_pnp_pose_batch(loop_ctx->get(), poses_req[slots[pc[sub[0]].request]].K4, (int32_t)packed.size(), packed.data(), 100, 5.991, 5.991, 1.0));
          size_t at = 0;
          for (size_t i : sub) {
            std::vector<ssx_pnp_pose_job>& dst = *poses_req[slots[pc[i].request]].jobs;
            for (int j = 0; j < pc[i].count; ++j, ++at) {
              ssx_pnp_pose_job& d = dst[(size_t)(pc[i].first + j)];
              const ssx_pnp_pose_job& q = packed[at];
              std::memcpy(d.pose_out, q.pose_out, sizeof d.pose_out);
              d.found = q.found; d.n_ransac_inliers = q.n_ransac_inliers; d.best_hypothesis = q.best_hypothesis; d.n_inliers = q.n_inliers;
            }
          }
          ++calls; jobs += (long)packed.size();
        });
        for (size_t i = 0; i < pc.size(); ++i) if (!part_errs[i].empty()) errs[pc[i].request] = part_errs[i];
      }
    }};
    // undistortion: the jobs of a call share the image size; its plan holds one map per camera (ssx_undistort_plan_add finds a set it was
    // shown by its bytes).  All left images, then all right ones: the raw pairs and the results then stand in the arena in ascending
    // order -- one copy up and, when the whole cohort is in the call, one copy down (ssx_undistort_plan_apply).
    t[UND] = {"undistortion", Grouped([this](int k) { return und_req[k].size; }, [this](Slots slots, Errs) {
      UndSize& us = ForUndSize(und_req[slots[0]].size);
      std::vector<ssx_undistort_plan_job> jobs;
      for (int side = 0; side < 2; ++side)
        for (int k : slots) {
          const UndReq& r = und_req[k];
          int32_t map = -1;
          us.ctx.check(ssx_undistort_plan_add_lens(us.plan, &r.prm[side], &map));
          jobs.push_back({r.src[side], r.size.cols, r.dst[side], r.size.cols, map});
        }
      us.ctx.check(ssx_undistort_plan_apply(us.plan, (int32_t)jobs.size(), jobs.data(), 1));
    })};
    // ComputeCorrectPose, LoopCorrect and the window's loop correction: one at a time, here, so that none runs on the loop context or
    // the window context beside a batched call of this dispatcher
    t[CALL] = {"single call", [this](Slots slots, Errs errs, long& calls, long& jobs) {
      for (size_t i = 0; i < slots.size(); ++i) {
        try { (*call_req[slots[i]])(); } catch (const std::exception& e) { errs[i] = e.what(); }
      }
      calls += (long)slots.size(); jobs += (long)slots.size();
    }};
    return t;
  }

  std::mutex pin_mu;
  uint8_t* pin_arena = nullptr, *raw_arena = nullptr;
  size_t pin_slice = 0;
  int device, S;
  ssx::Context po_ctx, ba_ctx, det_ctx, tri_ctx;
  std::mutex size_mu;
  std::map<ImageSize, std::unique_ptr<SizeCtx>> size_ctx;   // that size's LK contexts
  std::map<ImageSize, std::unique_ptr<UndSize>> und_size;   // that size's undistortion plan
  std::vector<LkReq> lk_req;
  std::vector<ssx_pose_only_job> po_req;
  std::vector<DetReq> det_req;
  std::vector<ssx_triangulate_job> tri_req;
  std::vector<BaReq> ba_req;
  std::mutex loop_mu;                               // the making of the loop context, the vocabulary and the databases
  std::unique_ptr<ssx::Context> loop_ctx;
  ssx_vocabulary* voc = nullptr;
  std::string loop_voc_path;
  std::vector<LoopReq> loop_req;
  std::vector<std::function<void()>*> call_req;
  std::vector<UndReq> und_req;
  std::vector<RelocReq> reloc_req;
  std::vector<PosesReq> poses_req;
  BatchDispatch core;                               // (last: its threads start when the rest is made and stop before it goes)
};

namespace {

class BatchedBaWindow final : public BaWindow {
 public:
  BatchedBaWindow(StreamBatcher::Impl& im, int k, const double* K4, const double* cam_ext14, const ssx_ba_options& opt) : im_(im), k_(k)
  {
    im_.ba_ctx.check(ssx_ba_window_create(im_.ba_ctx.get(), &opt, K4, cam_ext14, &win_));
    im_.ba_ctx.check(ssx_ba_window_set_fix_rule(win_, 1));
  }
  ~BatchedBaWindow() override { ssx_ba_window_destroy(win_); }
  void Push(int64_t kf_id, const double* pose7, int n_new, const int64_t* new_ids, const double* new_xyz, const uint8_t* new_fixed, int n_obs,
            const int64_t* obs_lm, const double* obs_uv, const uint8_t* obs_cam) override
  {
    check(ssx_ba_window_push_keyframe(win_, kf_id, pose7, 0, n_new, new_ids, new_xyz, new_fixed, n_obs, obs_lm, obs_uv, obs_cam));
  }
  void Pop(int64_t kf_id) override { check(ssx_ba_window_pop_keyframe(win_, kf_id)); }
  void RemoveLandmarks(int n, const int64_t* lm_ids) override { check(ssx_ba_window_remove_landmarks(win_, n, lm_ids, nullptr)); }
  void RemoveFlagged(int n_obs, const uint8_t* flags) override { check(ssx_ba_window_remove_flagged(win_, n_obs, flags, nullptr)); }
  void Size(int& nk, int& nl, int& no) override
  {
    int32_t a = 0, b = 0, c = 0;
    check(ssx_ba_window_size(win_, &a, &b, &c));
    nk = a; nl = b; no = c;
  }
  void Export(int64_t* kf_ids, int64_t* lm_ids, uint8_t* point_fixed, int32_t* edge_pose, int32_t* edge_point, double* edge_uv) override
  {
    check(ssx_ba_window_export(win_, kf_ids, nullptr, nullptr, lm_ids, nullptr, point_fixed, edge_pose, edge_point, edge_uv, nullptr));
  }
  void Solve(ssx_ba_result& res) override
  {
    // the stream's own thread files the request in the stream's slot; the worker thread of an asynchronous backend has a slot of its
    // own (the stream's thread goes on filing per-frame requests meanwhile)
    const int slot = im_.core.Slot(k_);
    im_.ba_req[slot] = {win_, &res};
    im_.core.SubmitAndWait(slot, BA);
  }
  void LoopCorrect(int64_t cur_kf_id, const double* corrected_pose7, int n_fused, const int64_t* fused_ids, ssx_ba_window_loop_result* res) override
  {
    // (the windows of a cohort share ba_ctx: the keyframe dispatcher makes the call, never beside one of its batched solves)
    std::function<void()> call = [&] { im_.ba_ctx.check(ssx_ba_window_loop_correct(win_, cur_kf_id, corrected_pose7, n_fused, n_fused > 0 ? fused_ids : nullptr, res)); };
    const int slot = im_.core.Slot(k_);
    im_.call_req[slot] = &call;
    im_.core.SubmitAndWait(slot, CALL);
  }

 private:
  // (these calls only edit the window's host mirror; the shared context's error text may belong to another stream's call, so the
  // message names the status instead)
  void check(ssx_status st) const { if (st != SSX_OK) throw std::runtime_error("ssx_ba_window: edit failed with status " + std::to_string((int)st)); }
  StreamBatcher::Impl& im_;
  int k_;
  ssx_ba_window* win_ = nullptr;
};

// The loop-closing calls of one stream of a cohort: its keyframe database on the cohort's loop context.  The keyframe step is filed
// like a window solve and served as one job of ssx_kfdb_process_keyframe_batch; the rare calls of a correction go to the keyframe
// dispatcher one at a time.
class BatchedLoopCompute final : public LoopCompute {
 public:
  BatchedLoopCompute(StreamBatcher::Impl& im, int k, const std::string& voc_path) : im_(im), k_(k), db_(im.MakeLoopDatabase(voc_path)) {}
  ~BatchedLoopCompute() override
  {
    ssx_kfdb_destroy(db_);
    ssx_host_free(pin_);
  }
  void ProcessKeyframe(int64_t kf_id, const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, int min_db_size,
                       int min_id_gap, float threshold, ssx_kfdb_step_result& res, std::vector<int32_t>& pairs) override
  {
    const int slot = im_.core.Slot(k_);
    Pin(img);
    pairs.resize(2 * std::max<size_t>(1024, features.size() * (size_t)std::max(pyramid_levels, 1)));
    LoopReq& r = im_.loop_req[slot];
    for (int attempt = 0;; ++attempt) {
      r = LoopReq{};
      r.job.db = db_; r.job.kf_id = kf_id; r.job.img = pin_; r.job.stride = img.cols; r.job.n_features = (int32_t)features.size(); r.job.features = features.data();
      r.job.commit_pending = commit_next_ ? 1 : 0; r.job.pairs_cap = (int32_t)(pairs.size() / 2); r.job.pairs_out = pairs.data(); r.job.res = &res;
      r.prm = prm; r.size = {img.rows, img.cols}; r.levels = pyramid_levels; r.min_db = min_db_size; r.min_gap = min_id_gap; r.threshold = threshold;
      im_.core.SubmitAndWait(slot, LOOP);
      commit_next_ = false;                         // (the call ran: the keyframe of AddPending is stored)
      if (r.status != SSX_ERR_CAPACITY || attempt > 0) break;
      pairs.resize(2 * (size_t)res.n_pairs);        // a larger loop keyframe: the count is known now, the step once more
    }
    if (r.status != SSX_OK) throw std::runtime_error("ssx_kfdb_process_keyframe_batch: job status " + std::to_string(r.status));
    pairs.resize(2 * (size_t)res.n_pairs);
  }
  // nothing is launched: the stream's next step carries commit_pending, and the keyframe is read no earlier than that
  void AddPending() override { commit_next_ = true; }
  void ComputePose(int n_pairs, const double* loop_xyz, const uint8_t* has_point, const double* cur_uv, const double* T_cur, const double* T_loop,
                   const double* K4, uint8_t* kept, ssx_loop_pose_result& out) override
  {
    Single([&] { im_.loop_ctx->check(ssx_loop_compute_pose(im_.loop_ctx->get(), n_pairs, loop_xyz, has_point, cur_uv, T_cur, T_loop, K4, 100, 0, kept, &out)); });
  }
  void LoopCorrect(const ssx_loop_correct_problem& prob, ssx_loop_correct_result& res) override
  {
    Single([&] { im_.loop_ctx->check(ssx_loop_correct(im_.loop_ctx->get(), &prob, 20, &res)); });
  }
  // The candidate query of a lost front-end as one job of ssx_kfdb_relocalize_query_batch.  The keyframe of AddPending is not in the
  // database yet (nothing was launched for it): the job carries commit_pending, as the stream's next keyframe step would have
  void RelocalizeQuery(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, int max_candidates,
                       float threshold, float ratio, ssx_reloc_query_result& res, std::vector<std::vector<int32_t>>& pairs) override
  {
    const int slot = im_.core.Slot(k_);
    Pin(img);
    const size_t K = (size_t)std::max(max_candidates, 1);
    size_t cap = std::max<size_t>(1024, features.size() * (size_t)std::max(pyramid_levels, 1));
    std::vector<int32_t> flat;
    RelocReq& r = im_.reloc_req[slot];
    for (int attempt = 0;; ++attempt) {
      flat.assign(2 * K * cap, 0);
      r = RelocReq{};
      r.job.db = db_; r.job.img = pin_; r.job.stride = img.cols; r.job.n_features = (int32_t)features.size(); r.job.features = features.data();
      r.job.commit_pending = commit_next_ ? 1 : 0; r.job.pairs_cap = (int32_t)cap; r.job.pairs_out = flat.data(); r.job.res = &res;
      r.prm = prm; r.size = {img.rows, img.cols}; r.levels = pyramid_levels; r.candidates = max_candidates; r.threshold = threshold; r.ratio = ratio;
      im_.core.SubmitAndWait(slot, RELOC);
      commit_next_ = false;                         // (the call ran: the keyframe of AddPending is stored)
      if (r.status != SSX_ERR_CAPACITY || attempt > 0) break;
      for (int c = 0; c < res.n_candidates; ++c) cap = std::max(cap, (size_t)res.cand[c].n_pairs);   // a larger stored keyframe: the counts are known now
    }
    if (r.status != SSX_OK) throw std::runtime_error("ssx_kfdb_relocalize_query_batch: job status " + std::to_string(r.status));
    pairs.assign((size_t)res.n_candidates, {});
    for (int c = 0; c < res.n_candidates; ++c) pairs[c].assign(flat.begin() + 2 * c * cap, flat.begin() + 2 * (c * cap + (size_t)res.cand[c].n_pairs));
  }
  void PosesBatch(const double* K4, std::vector<ssx_pnp_pose_job>& jobs) override
  {
    const int slot = im_.core.Slot(k_);
    im_.poses_req[slot] = PosesReq{K4, &jobs};
    im_.core.SubmitAndWait(slot, POSES);
  }

 private:
  // the image in a pinned buffer of the stream's own, read there by the GPU
  void Pin(const Image& img)
  {
    const size_t bytes = (size_t)img.rows * img.cols;
    if (bytes > pin_bytes_) {
      ssx_host_free(pin_);
      pin_ = static_cast<uint8_t*>(ssx_host_alloc(bytes));
      if (!pin_) throw std::runtime_error("StreamBatcher: no pinned memory for the loop step's image");
      pin_bytes_ = bytes;
    }
    std::memcpy(pin_, img.ptr(), bytes);
  }
  void Single(std::function<void()> call)
  {
    const int slot = im_.core.Slot(k_);
    im_.call_req[slot] = &call;
    im_.core.SubmitAndWait(slot, CALL);
  }
  StreamBatcher::Impl& im_;
  int k_;
  ssx_kf_database* db_ = nullptr;
  uint8_t* pin_ = nullptr;
  size_t pin_bytes_ = 0;
  bool commit_next_ = false;
};

class BatchedCompute final : public Compute {
 public:
  BatchedCompute(StreamBatcher::Impl& im, int k) : im_(im), k_(k), frame_(im.device) { im_.core.Bind(k_); }
  ~BatchedCompute() override
  {
    if (own_pins_) { ssx_host_free(pin_[0]); ssx_host_free(pin_[1]); }
    if (own_raw_) { ssx_host_free(raw_[0]); ssx_host_free(raw_[1]); }
  }

  bool CanUndistort() const override { return true; }
  // Camera::UndistortImage on the frame's pair as ONE request of two jobs (UND).  This thread copies the raw pair into the stream's
  // pinned buffers 2 and 3; the call writes the results into buffers 0 and 1, which then hold the frame's images under the ids the
  // front-end gave them -- the frame's LK calls find them there and copy nothing -- and this thread fills the host images from them.
  void UndistortPair(const Image& left, const Image& right, const ssx_undistort_params prm[2], Image& left_out, Image& right_out) override
  {
    ssx_lens_params lens[2] = {};                  // (the RADTAN lens a parameter set is: the bytes ssx_undistort_plan_add gives it)
    for (int s = 0; s < 2; ++s) {
      lens[s].model = SSX_LENS_RADTAN;
      std::memcpy(lens[s].K, prm[s].K, sizeof lens[s].K); std::memcpy(lens[s].coeffs, prm[s].dist, sizeof lens[s].coeffs); std::memcpy(lens[s].iR, prm[s].iR, sizeof lens[s].iR);
    }
    RectifyPair(left, right, lens, left_out, right_out);
  }

  bool CanRectify() const override { return true; }
  // Camera.Rectify: the same request kind -- a map is a map, whatever lens and rotation it was made from
  void RectifyPair(const Image& left, const Image& right, const ssx_lens_params prm[2], Image& left_out, Image& right_out) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    if (left.rows != right.rows || left.cols != right.cols) throw std::invalid_argument("UndistortPair: left / right image sizes differ");
    const size_t bytes = (size_t)left.rows * left.cols;
    Reserve(bytes);
    if (bytes > raw_bytes_) {
      if (own_raw_) { ssx_host_free(raw_[0]); ssx_host_free(raw_[1]); }
      raw_[0] = own_pins_ ? nullptr : im_.PinSlice(k_, 2, bytes); raw_[1] = own_pins_ ? nullptr : im_.PinSlice(k_, 3, bytes);
      own_raw_ = !raw_[0] || !raw_[1];
      if (own_raw_) { raw_[0] = static_cast<uint8_t*>(ssx_host_alloc(bytes)); raw_[1] = static_cast<uint8_t*>(ssx_host_alloc(bytes)); }
      if (!raw_[0] || !raw_[1]) throw std::runtime_error("StreamBatcher: no pinned memory for the stream's raw images");
      raw_bytes_ = bytes;
    }
    std::memcpy(raw_[0], left.ptr(), bytes); std::memcpy(raw_[1], right.ptr(), bytes);
    left_out.rows = right_out.rows = left.rows; left_out.cols = right_out.cols = left.cols;
    left_out.data.resize(bytes); right_out.data.resize(bytes);
    UndReq& r = im_.und_req[k_];
    r = UndReq{};
    r.src[0] = raw_[0]; r.src[1] = raw_[1]; r.dst[0] = pin_[0]; r.dst[1] = pin_[1]; r.prm[0] = prm[0]; r.prm[1] = prm[1]; r.size = {left.rows, left.cols};
    pin_id_[0] = pin_id_[1] = 0;                   // (the call overwrites both; a failed call leaves nothing there)
    im_.core.SubmitAndWait(k_, UND);
    pin_id_[0] = left_out.id; pin_id_[1] = right_out.id;
    std::memcpy(left_out.data.data(), pin_[0], bytes); std::memcpy(right_out.data.data(), pin_[1], bytes);
  }

  void Detect(const Image& img, const uint8_t* mask, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    BatchDispatch::LongOp op(im_.core, k_);
    kps.assign((size_t)prm.nfeatures + 260 + 64, ssx_keypoint{});
    int32_t n = 0;
    ssx_status st = ssx_orb_detect(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, mask, img.cols, &prm, (int32_t)kps.size(), kps.data(), &n);
    if (st == SSX_ERR_CAPACITY && n > (int32_t)kps.size()) {
      kps.assign((size_t)n, ssx_keypoint{});
      st = ssx_orb_detect(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, mask, img.cols, &prm, (int32_t)kps.size(), kps.data(), &n);
    }
    frame_.check(st);
    kps.resize(n);
  }
  void DetectBoxes(const Image& img, const std::vector<int32_t>& boxes, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    kps.assign((size_t)prm.nfeatures + 260 + 64, ssx_keypoint{});
    int32_t n = 0;
    const uint8_t* pinned = Pinned(img, 0);        // (the current left image: usually there already, from the frame's temporal LK)
    DetReq& r = im_.det_req[k_];
    r = DetReq{};
    ssx_orb_detect_job& q = r.job;
    q.img = pinned; q.stride = img.cols; q.boxes_xyxy = boxes.data(); q.n_boxes = (int32_t)(boxes.size() / 4);
    q.cap = (int32_t)kps.size(); q.kps_out = kps.data(); q.n_out = &n;
    r.prm = prm; r.size = {img.rows, img.cols};
    im_.core.SubmitAndWait(k_, DET);
    if (n > (int32_t)kps.size()) {
      // (a grid returned more than the bound of ssx.h: once more with the size it asked for, on the stream's own context)
      BatchDispatch::LongOp op(im_.core, k_);
      kps.assign((size_t)n, ssx_keypoint{});
      frame_.check(ssx_orb_detect_boxes(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, boxes.data(), (int32_t)(boxes.size() / 4), &prm, (int32_t)kps.size(),
                                        kps.data(), &n));
    }
    kps.resize(n);
  }

  void TrackLK(const Image& prev, const Image& next, const std::vector<float>& prev_pts, std::vector<float>& next_pts, std::vector<uint8_t>& status,
               bool temporal) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    const int n = (int)(prev_pts.size() / 2);
    status.assign(n, 0);
    LkReq& r = im_.lk_req[k_];
    r = LkReq{};
    ssx_lk_job& q = r.job;
    q.slot = k_;
    q.n = n; q.prev_pts = prev_pts.data(); q.next_pts = next_pts.data(); q.status = status.data(); q.err = nullptr;
    r.size = {next.rows, next.cols};
    if (!temporal) {
      // FindFeaturesInRight (frontend.cpp:346-428): left -> right of one frame, both pyramids built afresh, on this stream's slot of
      // its image size's stereo LK context
      if (prev.rows != next.rows || prev.cols != next.cols) throw std::invalid_argument("TrackLK: image sizes differ");
      q.prev = Pinned(prev, 0); q.prev_stride = prev.cols;
      q.next = Pinned(next, 1, q.prev); q.next_stride = next.cols;
      im_.core.SubmitAndWait(k_, LKS);
      return;
    }
    // the frame-to-frame chain: this stream's slot of its image size's LK context keeps the pyramid of its last `next` image.  The new
    // image goes into the stream's pinned buffer (this thread copies it: S streams copy side by side) and is read from there by the
    // GPU -- no staging inside the batched call.
    const bool chained = prev.id != 0 && prev.id == chain_next_id_ && prev.rows == chain_rows_ && prev.cols == chain_cols_ && next.rows == prev.rows &&
                         next.cols == prev.cols;
    if (!chained) { q.prev = Pinned(prev, 1); q.prev_stride = prev.cols; }
    q.next = Pinned(next, 0, q.prev); q.next_stride = next.cols;
    chain_next_id_ = 0;                            // (a failed call leaves no chain)
    im_.core.SubmitAndWait(k_, LK);
    chain_next_id_ = next.id; chain_rows_ = next.rows; chain_cols_ = next.cols;
  }

  int PoseOnly(double* pose_io, const double* K4, int M, const double* xyz, const double* uv, uint8_t* inlier) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    int32_t n_in = 0;
    ssx_pose_only_job& q = im_.po_req[k_];
    q = ssx_pose_only_job{};
    q.pose_io = pose_io; q.K4 = K4; q.M = M; q.xyz = xyz; q.uv = uv; q.rounds = 4; q.iters = 10; q.chi2_th = 5.991; q.huber_delta = 1.0;
    q.inlier_out = inlier; q.n_inliers = &n_in;
    im_.core.SubmitAndWait(k_, PO);
    return n_in;
  }

  void Triangulate(int n, const double* uvL, const double* uvR, const ssx_stereo_rig& rig, const double* T_wc, double* xyz, uint8_t* ok) override
  {
    im_.core.Bind(k_);                             // (the front-end calls come from the stream's thread)
    ssx_triangulate_job& q = im_.tri_req[k_];
    q = ssx_triangulate_job{};
    q.n = n; q.uvL = uvL; q.uvR = uvR; q.rig = &rig; q.T_wc = T_wc; q.xyz_out = xyz; q.ok_out = ok;
    im_.core.SubmitAndWait(k_, TRI);
  }

  void BundleAdjust(const ssx_ba_problem& prob, const ssx_ba_options& opt, ssx_ba_result& res) override
  {
    // (Backend.Window: 0 -- the re-marshalled map, one window per call)
    if (im_.core.Slot(k_) != k_) {
      // the worker thread of an asynchronous backend: a context of its own, and the stream's slot is not touched (its thread is tracking)
      if (!async_ba_) async_ba_ = std::make_unique<ssx::Context>(im_.device);
      async_ba_->check(ssx_ba_solve(async_ba_->get(), &prob, &opt, &res));
      return;
    }
    BatchDispatch::LongOp op(im_.core, k_);
    frame_.check(ssx_ba_solve(frame_.get(), &prob, &opt, &res));
  }

  std::unique_ptr<BaWindow> MakeBaWindow(const double* K4, const double* cam_ext14, const ssx_ba_options& opt) override
  {
    return std::make_unique<BatchedBaWindow>(im_, k_, K4, cam_ext14, opt);
  }

  std::unique_ptr<LoopCompute> MakeLoopCompute(const std::string& voc_path) override { return std::make_unique<BatchedLoopCompute>(im_, k_, voc_path); }

 private:
  // the image in the stream's pinned buffer `which` (copied by this thread unless it is there already)
  // (keep: a buffer this call must not overwrite -- the other image of a two-image request)
  const uint8_t* Pinned(const Image& img, int which, const uint8_t* keep = nullptr)
  {
    const size_t bytes = (size_t)img.rows * img.cols;
    Reserve(bytes);
    if (img.id != 0 && pin_id_[which] == img.id) return pin_[which];
    if (img.id != 0 && pin_id_[which ^ 1] == img.id) return pin_[which ^ 1];
    if (keep && pin_[which] == keep) which ^= 1;
    std::memcpy(pin_[which], img.ptr(), bytes);
    pin_id_[which] = img.id;
    return pin_[which];
  }
  // the stream's two pinned image buffers hold `bytes` each: slices of the cohort's arena, or buffers of its own
  void Reserve(size_t bytes)
  {
    if (bytes > pin_bytes_) {
      if (own_pins_) { ssx_host_free(pin_[0]); ssx_host_free(pin_[1]); }
      pin_[0] = im_.PinSlice(k_, 0, bytes); pin_[1] = im_.PinSlice(k_, 1, bytes);
      own_pins_ = !pin_[0] || !pin_[1];
      if (own_pins_) { pin_[0] = static_cast<uint8_t*>(ssx_host_alloc(bytes)); pin_[1] = static_cast<uint8_t*>(ssx_host_alloc(bytes)); }
      if (!pin_[0] || !pin_[1]) throw std::runtime_error("StreamBatcher: no pinned memory for the stream's images");
      pin_bytes_ = bytes; pin_id_[0] = pin_id_[1] = 0;
    }
  }

  StreamBatcher::Impl& im_;
  int k_;
  std::unique_ptr<ssx::Context> async_ba_;
  ssx::Context frame_;
  uint8_t* pin_[2] = {nullptr, nullptr};
  uint64_t pin_id_[2] = {0, 0};
  size_t pin_bytes_ = 0;
  bool own_pins_ = false;
  uint8_t* raw_[2] = {nullptr, nullptr};            // a frame's raw pair on its way through undistortion (arena buffers 2 and 3, or its own)
  size_t raw_bytes_ = 0;
  bool own_raw_ = false;
  uint64_t chain_next_id_ = 0;
  int chain_rows_ = 0, chain_cols_ = 0;
};

}  // namespace

// `cohorts` independent batchers, stream k in cohort k mod cohorts: while one cohort's batch is on the GPU the other cohort's streams do
// their host work (bookkeeping, the copy of the next frame into pinned memory, the wake-ups) -- two cohorts ping-pong
StreamBatcher::StreamBatcher(int device, int streams, int cohorts)
{
  streams = std::max(streams, 1);
  const int C = std::max(1, std::min(cohorts, streams));
  for (int c = 0; c < C; ++c) impls_.push_back(std::make_unique<Impl>(device, (streams - c + C - 1) / C));
  n_streams_ = streams;
}
StreamBatcher::~StreamBatcher() = default;

std::unique_ptr<Compute> StreamBatcher::MakeCompute(int k)
{
  if (k < 0 || k >= n_streams_) throw std::invalid_argument("StreamBatcher::MakeCompute: stream index out of range");
  const int C = (int)impls_.size();
  return std::make_unique<BatchedCompute>(*impls_[k % C], k / C);
}

void StreamBatcher::Finish(int k)
{
  const int C = (int)impls_.size();
  if (k >= 0 && k < n_streams_) impls_[k % C]->core.Finish(k / C);
}

size_t StreamBatcher::PinnedSliceBytes(int k)
{
  if (k < 0 || k >= n_streams_) return 0;
  Impl& im = *impls_[k % (int)impls_.size()];
  std::lock_guard<std::mutex> lk(im.pin_mu);
  return im.pin_slice;
}

void StreamBatcher::ResetStats()
{
  for (auto& im : impls_) im->core.ResetCounters();
}

StreamBatcher::Stats StreamBatcher::stats()
{
  Stats t;
  long single_jobs = 0;
  for (auto& im : impls_) {
    auto add = [&](Kind kind, long& calls, long& jobs, double& seconds) {
      const BatchDispatch::Counters c = im->core.counters(kind);
      calls += c.calls; jobs += c.jobs; seconds += c.seconds;
    };
    add(LK, t.lk_calls, t.lk_jobs, t.lk_s);
    add(PO, t.po_calls, t.po_jobs, t.po_s);
    for (Kind kf : {DET, LKS, TRI}) add(kf, t.kf_calls, t.kf_jobs, t.kf_s);
    add(BA, t.ba_calls, t.ba_jobs, t.ba_s);
    add(LOOP, t.loop_calls, t.loop_jobs, t.loop_s);
    add(CALL, t.single_calls, single_jobs, t.single_s);
    long und_requests = 0;
    add(UND, t.und_calls, und_requests, t.und_s);
    add(RELOC, t.reloc_calls, t.reloc_jobs, t.reloc_s);
    add(POSES, t.pose_calls, t.pose_jobs, t.pose_s);
    t.und_jobs += 2 * und_requests;                 // (a request is a frame's pair)
    t.wait_s += im->core.wait_s();
  }
  return t;
}

}  // namespace ssx::host
