// ssvio_amd/host/ssx_compute.cpp -- Compute on libssx.so (see compute.hpp)
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "../../include/ssx_shim.hpp"
#include "compute.hpp"

namespace ssx::host {
namespace {

class SsxBaWindow final : public BaWindow {
 public:
  SsxBaWindow(ssx::Context& ctx, const double* K4, const double* cam_ext14, const ssx_ba_options& opt) : ctx_(ctx)
  {
    ctx_.check(ssx_ba_window_create(ctx_.get(), &opt, K4, cam_ext14, &win_));
    ctx_.check(ssx_ba_window_set_fix_rule(win_, 1));
  }
  ~SsxBaWindow() override { ssx_ba_window_destroy(win_); }
  void Push(int64_t kf_id, const double* pose7, int n_new, const int64_t* new_ids, const double* new_xyz, const uint8_t* new_fixed, int n_obs,
            const int64_t* obs_lm, const double* obs_uv, const uint8_t* obs_cam) override
  {
    ctx_.check(ssx_ba_window_push_keyframe(win_, kf_id, pose7, 0, n_new, new_ids, new_xyz, new_fixed, n_obs, obs_lm, obs_uv, obs_cam));
  }
  void Pop(int64_t kf_id) override { ctx_.check(ssx_ba_window_pop_keyframe(win_, kf_id)); }
  void RemoveLandmarks(int n, const int64_t* lm_ids) override { ctx_.check(ssx_ba_window_remove_landmarks(win_, n, lm_ids, nullptr)); }
  void RemoveFlagged(int n_obs, const uint8_t* flags) override { ctx_.check(ssx_ba_window_remove_flagged(win_, n_obs, flags, nullptr)); }
  void Size(int& nk, int& nl, int& no) override
  {
    int32_t a = 0, b = 0, c = 0;
    ctx_.check(ssx_ba_window_size(win_, &a, &b, &c));
    nk = a; nl = b; no = c;
  }
  void Export(int64_t* kf_ids, int64_t* lm_ids, uint8_t* point_fixed, int32_t* edge_pose, int32_t* edge_point, double* edge_uv) override
  {
    ctx_.check(ssx_ba_window_export(win_, kf_ids, nullptr, nullptr, lm_ids, nullptr, point_fixed, edge_pose, edge_point, edge_uv, nullptr));
  }
  void Solve(ssx_ba_result& res) override { ctx_.check(ssx_ba_window_solve(win_, &res)); }
  void LoopCorrect(int64_t cur_kf_id, const double* corrected_pose7, int n_fused, const int64_t* fused_ids, ssx_ba_window_loop_result* res) override
  {
    ctx_.check(ssx_ba_window_loop_correct(win_, cur_kf_id, corrected_pose7, n_fused, n_fused > 0 ? fused_ids : nullptr, res));
  }

 private:
  ssx::Context& ctx_;
  ssx_ba_window* win_ = nullptr;
};

// The loop-closing calls of one stream: a context of its own (the loop thread's), the vocabulary, the resident keyframe database.
class SsxLoopCompute final : public LoopCompute {
 public:
  SsxLoopCompute(int device, const std::string& voc_path) : ctx_(device)
  {
    if (ssx_voc_load_text(ctx_.get(), voc_path.c_str(), &voc_) != SSX_OK)
      throw std::runtime_error("DBOW2.VOC.Path: cannot read the vocabulary \"" + voc_path + "\": " + ssx_last_error(ctx_.get()));
    const ssx_status st = ssx_kfdb_create(ctx_.get(), 256, &db_);
    if (st != SSX_OK) {
      ssx_voc_destroy(voc_);
      ctx_.check(st);
    }
  }
  ~SsxLoopCompute() override
  {
    ssx_kfdb_destroy(db_);
    ssx_voc_destroy(voc_);
  }
  void ProcessKeyframe(int64_t kf_id, const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, int min_db_size,
                       int min_id_gap, float threshold, ssx_kfdb_step_result& res, std::vector<int32_t>& pairs) override
  {
    pairs.resize(2 * std::max<size_t>(1024, features.size() * (size_t)std::max(pyramid_levels, 1)));
    auto call = [&] {
      return ssx_kfdb_process_keyframe(db_, voc_, kf_id, img.ptr(), img.cols, img.rows, img.cols, &prm, (int32_t)features.size(), features.data(), pyramid_levels,
                                       min_db_size, min_id_gap, threshold, (int32_t)(pairs.size() / 2), pairs.data(), &res);
    };
    ssx_status st = call();
    if (st == SSX_ERR_CAPACITY) {                                        // a larger loop keyframe: the count is known now
      pairs.resize(2 * (size_t)res.n_pairs);
      st = call();
    }
    ctx_.check(st);
    pairs.resize(2 * (size_t)res.n_pairs);
  }
  void AddPending() override { ctx_.check(ssx_kfdb_add_pending(db_)); }
  void ComputePose(int n_pairs, const double* loop_xyz, const uint8_t* has_point, const double* cur_uv, const double* T_cur, const double* T_loop,
                   const double* K4, uint8_t* kept, ssx_loop_pose_result& out) override
  {
    ctx_.check(ssx_loop_compute_pose(ctx_.get(), n_pairs, loop_xyz, has_point, cur_uv, T_cur, T_loop, K4, 100, 0, kept, &out));   // :205-206: 100 iterations
  }
  void LoopCorrect(const ssx_loop_correct_problem& prob, ssx_loop_correct_result& res) override
  {
    ctx_.check(ssx_loop_correct(ctx_.get(), &prob, 20, &res));           // :533 optimize(20)
  }
  void RelocalizeQuery(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, int max_candidates,
                       float threshold, float ratio, ssx_reloc_query_result& res, std::vector<std::vector<int32_t>>& pairs) override
  {
    const size_t K = (size_t)std::max(max_candidates, 1);
    size_t cap = std::max<size_t>(1024, features.size() * (size_t)std::max(pyramid_levels, 1));
    std::vector<int32_t> flat(2 * K * cap);
    auto call = [&] {
      return ssx_kfdb_relocalize_query(db_, voc_, img.ptr(), img.cols, img.rows, img.cols, &prm, (int32_t)features.size(), features.data(), pyramid_levels,
                                       max_candidates, threshold, ratio, (int32_t)cap, flat.data(), &res);
    };
    ssx_status st = call();
    if (st == SSX_ERR_CAPACITY) {                                        // a larger stored keyframe: the counts are known now
      for (int c = 0; c < res.n_candidates; ++c) cap = std::max(cap, (size_t)res.cand[c].n_pairs);
      flat.assign(2 * K * cap, 0);
      st = call();
    }
    ctx_.check(st);
    pairs.assign((size_t)res.n_candidates, {});
    for (int c = 0; c < res.n_candidates; ++c) pairs[c].assign(flat.begin() + 2 * c * cap, flat.begin() + 2 * (c * cap + (size_t)res.cand[c].n_pairs));
  }
  void PosesBatch(const double* K4, std::vector<ssx_pnp_pose_job>& jobs) override
  {
    ctx_.check(ssx_pnp_pose_batch(ctx_.get(), K4, (int32_t)jobs.size(), jobs.data(), 100, 5.991, 5.991, 1.0));   // :205-206, :301, g2o's Huber
  }
  void GuidedSearch(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, const std::vector<uint8_t>& taken,
                    const double* K4, const double* T_cw12, const std::vector<int64_t>& point_kf, const std::vector<int32_t>& point_cls, const std::vector<double>& xyz,
                    const GuidedParams& gp, GuidedMatches& out) override
  {
    const size_t P = point_kf.size();
    if (point_cls.size() != P || xyz.size() != 3 * P || (!taken.empty() && taken.size() != features.size()))
      throw std::invalid_argument("GuidedSearch: one keyframe, one class id and one position per point, one flag per feature");
    out.feat.assign(P, -1); out.d1.assign(P, -1); out.d2.assign(P, -1); out.status.assign(P, 0);
    int32_t n = 0;
    ctx_.check(ssx_kfdb_guided_search(db_, img.ptr(), img.cols, img.rows, img.cols, &prm, (int32_t)features.size(), features.data(), pyramid_levels,
                                      taken.empty() ? nullptr : taken.data(), K4, T_cw12, (int32_t)P, point_kf.data(), point_cls.data(), xyz.data(), gp.radius,
                                      gp.max_distance, gp.ratio_pct, out.feat.data(), out.d1.data(), out.d2.data(), out.status.data(), nullptr, &n));
    out.n_matched = n;
  }
  void RefinePose(const double* K4, int M, const double* xyz, const double* uv, double* pose_io, uint8_t* inlier_out, int* n_inliers, int* found) override
  {
    int32_t n = 0;
    ctx_.check(ssx_loop_pose_opt(ctx_.get(), pose_io, K4, M, xyz, uv, 5.991, 1.0, inlier_out, &n));   // :301, g2o's Huber
    bool finite = true;
    for (int k = 0; k < 7; ++k) finite = finite && std::isfinite(pose_io[k]);
    *n_inliers = n; *found = finite ? 1 : 0;
  }

 private:
  ssx::Context ctx_;
  ssx_vocabulary* voc_ = nullptr;
  ssx_kf_database* db_ = nullptr;
};

class SsxCompute final : public Compute {
 public:
  explicit SsxCompute(int device) : device_(device), frame_(device), chain_(device), backend_(device) {}

  void Detect(const Image& img, const uint8_t* mask, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps) override
  {
    // Detect is single-level: <= max(N + 3, 4 * nIni <= 256) keypoints by the bound of ssx.h; should a grid ever return
    // more, the call reports the size it needs (SSX_ERR_CAPACITY, n > capacity) and is repeated once with that size
    kps.assign((size_t)prm.nfeatures + 260 + 64, ssx_keypoint{});
    int32_t n = 0;
    ssx_status st = ssx_orb_detect(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, mask, img.cols, &prm, (int32_t)kps.size(),
                                   kps.data(), &n);
    if (st == SSX_ERR_CAPACITY && n > (int32_t)kps.size()) {
      kps.assign((size_t)n, ssx_keypoint{});
      st = ssx_orb_detect(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, mask, img.cols, &prm, (int32_t)kps.size(), kps.data(), &n);
    }
    frame_.check(st);
    kps.resize(n);
  }

  void DetectBoxes(const Image& img, const std::vector<int32_t>& boxes, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps) override
  {
    kps.assign((size_t)prm.nfeatures + 260 + 64, ssx_keypoint{});
    int32_t n = 0;
    const int32_t nb = (int32_t)(boxes.size() / 4);
    ssx_status st = ssx_orb_detect_boxes(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, boxes.data(), nb, &prm, (int32_t)kps.size(), kps.data(), &n);
    if (st == SSX_ERR_CAPACITY && n > (int32_t)kps.size()) {
      kps.assign((size_t)n, ssx_keypoint{});
      st = ssx_orb_detect_boxes(frame_.get(), img.ptr(), img.cols, img.rows, img.cols, boxes.data(), nb, &prm, (int32_t)kps.size(), kps.data(), &n);
    }
    frame_.check(st);
    kps.resize(n);
  }

  bool CanUndistort() const override { return true; }

  // the frame's two images in one ssx_undistort call of two jobs on the per-frame context
  void UndistortPair(const Image& left, const Image& right, const ssx_undistort_params prm[2], Image& left_out, Image& right_out) override
  {
    if (left.rows != right.rows || left.cols != right.cols) throw std::invalid_argument("UndistortPair: left / right image sizes differ");
    left_out.rows = right_out.rows = left.rows; left_out.cols = right_out.cols = left.cols;
    left_out.data.resize(left.data.size()); right_out.data.resize(right.data.size());
    const ssx_undistort_job jobs[2] = {{left.ptr(), left.cols, left_out.data.data(), left.cols, prm[0]},
                                       {right.ptr(), right.cols, right_out.data.data(), right.cols, prm[1]}};
    frame_.check(ssx_undistort(frame_.get(), 2, jobs, left.rows, left.cols, 0));
  }

  bool CanRectify() const override { return true; }

  // the frame's raw pair in one ssx_undistort_lens call of two jobs, whatever the two lens models are
  void RectifyPair(const Image& left, const Image& right, const ssx_lens_params prm[2], Image& left_out, Image& right_out) override
  {
    if (left.rows != right.rows || left.cols != right.cols) throw std::invalid_argument("RectifyPair: left / right image sizes differ");
    left_out.rows = right_out.rows = left.rows; left_out.cols = right_out.cols = left.cols;
    left_out.data.resize(left.data.size()); right_out.data.resize(right.data.size());
    const ssx_lens_job jobs[2] = {{left.ptr(), left.cols, left_out.data.data(), left.cols, prm[0]},
                                  {right.ptr(), right.cols, right_out.data.data(), right.cols, prm[1]}};
    frame_.check(ssx_undistort_lens(frame_.get(), 2, jobs, left.rows, left.cols, 0));
  }

  bool CanDense() const override { return true; }

  // a keyframe's pair in one ssx_stereo_dense call on the per-frame context
  void DenseDisparity(const Image& left, const Image& right, const ssx_dense_params& prm, std::vector<int16_t>& disp) override
  {
    if (left.rows != right.rows || left.cols != right.cols) throw std::invalid_argument("DenseDisparity: left / right image sizes differ");
    disp.resize((size_t)left.rows * left.cols);
    const ssx_dense_job job = {left.ptr(), left.cols, right.ptr(), right.cols, disp.data(), left.cols};
    frame_.check(ssx_stereo_dense(frame_.get(), 1, &job, left.rows, left.cols, &prm, 0));
  }

  bool CanDensePost() const override { return true; }

  // a keyframe's pair, the filter and the samples in one ssx_stereo_dense_post call on the per-frame context
  void DenseKeyframe(const Image& left, const Image& right, const ssx_dense_params& prm, const ssx_dense_post& post, bool want_map, std::vector<int16_t>& disp,
                     std::vector<ssx_dense_sample>& samples) override
  {
    if (left.rows != right.rows || left.cols != right.cols) throw std::invalid_argument("DenseKeyframe: left / right image sizes differ");
    const bool sampling = post.cloud_stride > 0;
    if (!want_map && !sampling) throw std::invalid_argument("DenseKeyframe: neither the map nor samples are asked for");
    disp.resize(want_map ? (size_t)left.rows * left.cols : 0);
    const int s = sampling ? post.cloud_stride : 1;
    samples.resize(sampling ? (size_t)((left.rows + s - 1) / s) * (size_t)((left.cols + s - 1) / s) : 0);
    const ssx_dense_job job = {left.ptr(), left.cols, right.ptr(), right.cols, want_map ? disp.data() : nullptr, left.cols};
    ssx_dense_cloud cloud = {samples.data(), (int32_t)samples.size(), 0};
    frame_.check(ssx_stereo_dense_post(frame_.get(), 1, &job, sampling ? &cloud : nullptr, left.rows, left.cols, &prm, &post, 0));
    samples.resize(sampling ? (size_t)cloud.count : 0);
  }

  void TrackLK(const Image& prev, const Image& next, const std::vector<float>& prev_pts, std::vector<float>& next_pts,
               std::vector<uint8_t>& status, bool temporal) override
  {
    const int n = (int)(prev_pts.size() / 2);
    status.assign(n, 0);
    ssx_lk_params p;
    ssx_lk_default_params(&p);
    p.win = 11; p.max_level = 3; p.max_iters = 30; p.eps = 0.01; p.use_initial_flow = 1;
    if (!temporal) {
      frame_.check(ssx_lk_track(frame_.get(), prev.ptr(), prev.cols, next.ptr(), next.cols, prev.rows, prev.cols, n, prev_pts.data(),
                                next_pts.data(), status.data(), nullptr, &p, nullptr));
      return;
    }
    // consecutive frames: the pyramid of `prev` is still on the device when it was the `next` image of the last call
    if (prev.id != 0 && prev.id == chain_next_id_ && prev.rows == chain_rows_ && prev.cols == chain_cols_) {
      chain_.check(ssx_lk_track_next(chain_.get(), next.ptr(), next.cols, next.rows, next.cols, n, prev_pts.data(), next_pts.data(),
                                     status.data(), nullptr, &p, nullptr));
    } else {
      chain_.check(ssx_lk_track(chain_.get(), prev.ptr(), prev.cols, next.ptr(), next.cols, prev.rows, prev.cols, n, prev_pts.data(),
                                next_pts.data(), status.data(), nullptr, &p, nullptr));
    }
    chain_next_id_ = next.id; chain_rows_ = next.rows; chain_cols_ = next.cols;
  }

  int PoseOnly(double* pose_io, const double* K4, int M, const double* xyz, const double* uv, uint8_t* inlier) override
  {
    int32_t n_in = 0;
    frame_.check(ssx_pose_only_opt(frame_.get(), pose_io, K4, M, xyz, uv, 4, 10, 5.991, 1.0, inlier, &n_in));
    return n_in;
  }

  void Triangulate(int n, const double* uvL, const double* uvR, const ssx_stereo_rig& rig, const double* T_wc, double* xyz,
                   uint8_t* ok) override
  {
    frame_.check(ssx_triangulate(frame_.get(), n, uvL, uvR, &rig, T_wc, xyz, ok));
  }

  void BundleAdjust(const ssx_ba_problem& prob, const ssx_ba_options& opt, ssx_ba_result& res) override
  {
    backend_.check(ssx_ba_solve(backend_.get(), &prob, &opt, &res));
  }

  std::unique_ptr<BaWindow> MakeBaWindow(const double* K4, const double* cam_ext14, const ssx_ba_options& opt) override
  {
    return std::make_unique<SsxBaWindow>(backend_, K4, cam_ext14, opt);    // (the window must be destroyed before this Compute)
  }

  std::unique_ptr<LoopCompute> MakeLoopCompute(const std::string& voc_path) override { return std::make_unique<SsxLoopCompute>(device_, voc_path); }

 private:
  int device_;
  ssx::Context frame_, chain_, backend_;
  uint64_t chain_next_id_ = 0;
  int chain_rows_ = 0, chain_cols_ = 0;
};

}  // namespace

std::unique_ptr<Compute> MakeSsxCompute(int device) { return std::make_unique<SsxCompute>(device); }

}  // namespace ssx::host
