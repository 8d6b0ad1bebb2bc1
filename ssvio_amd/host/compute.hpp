// ssvio_amd/host/compute.hpp -- the compute calls the reference's front-end, backend and loop closing make, as one interface
// the host layer is written against:
//   UndistortPair   Camera::UndistortImage, twice     (frontend.cpp:39-45 GrabSteroImage, camera.cpp:43-55)
//   Detect          ORBextractor::Detect              (frontend.cpp:302-344 DetectFeatures)
//   TrackLK         cv::calcOpticalFlowPyrLK          (frontend.cpp:156-166 TrackLastFrame, :374-384 FindFeaturesInRight)
//   PoseOnly        the g2o part of EstimateCurrentPose (frontend.cpp:196-270)
//   Triangulate     ssvio::triangulation + z > 0      (frontend.cpp:448-544)
//   BundleAdjust    the g2o part of OptimizeActiveMap (backend.cpp:78-205)
//   DenseDisparity  a disparity for every pixel of a keyframe's pair (no counterpart in the reference; Dense.Open)
//   LoopCompute     the per-keyframe step, ComputeCorrectPose and LoopCorrect's geometry (loopclosing.cpp:39-70, 147-243, 353-594)
// SsxCompute is the product implementation: the C ABI of libssx.so on an MI355X, nothing else (no CPU fallback; the
// constructor throws without a gfx950 device).  The interface exists so tests can run the same host logic against
// the CPU oracle and compare whole trajectories.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ssx.h"
#include "dataset.hpp"

namespace ssx::host {

// The active window of the backend RESIDENT on the device (ssx_ba_window, include/ssx.h): the backend mirrors every change of
// its map -- a keyframe in, a keyframe out, outlier observations unlinked, condemned map points deleted
// (map.cpp:18-58, 89-194; backend.cpp:205-244) -- instead of re-marshalling the whole window at every keyframe.  Keyframes and
// map points are named by their ids; the window solves in id order, so its result is, bit for bit, the one BundleAdjust returns
// for the re-marshalled map (Backend::Marshal).
class BaWindow {
 public:
  virtual ~BaWindow() = default;
  virtual void Push(int64_t kf_id, const double* pose7, int n_new, const int64_t* new_ids, const double* new_xyz, const uint8_t* new_fixed,
                    int n_obs, const int64_t* obs_lm, const double* obs_uv, const uint8_t* obs_cam) = 0;
  virtual void Pop(int64_t kf_id) = 0;
  virtual void RemoveLandmarks(int n, const int64_t* lm_ids) = 0;
  virtual void RemoveFlagged(int n_obs, const uint8_t* flags) = 0;             // flags in the order of Export / of the last Solve
  virtual void Size(int& n_keyframes, int& n_landmarks, int& n_observations) = 0;
  // ids ascending; edge_pose / edge_point index into them; point_fixed = the flags the next solve uses (any may be null)
  virtual void Export(int64_t* kf_ids, int64_t* lm_ids, uint8_t* point_fixed, int32_t* edge_pose, int32_t* edge_point, double* edge_uv) = 0;
  virtual void Solve(ssx_ba_result& res) = 0;                                   // res.* in the order of Export
  // LoopClosing::CorrectActivateKeyframeAndMappoint on the window where it lies (ssx_ba_window_loop_correct): every keyframe moves
  // with the corrected current one, every observed landmark is re-anchored, the fused landmarks leave with their observations.
  // res may be null.  An implementation without it cannot take part in loop closing.
  virtual void LoopCorrect(int64_t cur_kf_id, const double* corrected_pose7, int n_fused, const int64_t* fused_ids, ssx_ba_window_loop_result* res)
  {
    (void)cur_kf_id; (void)corrected_pose7; (void)n_fused; (void)fused_ids; (void)res;
    throw std::logic_error("BaWindow::LoopCorrect: this window cannot apply a loop correction");
  }
};

// The library calls of the loop-closing thread (loopclosing.cpp:39-70, 147-243, 353-594), one method per call.  An object owns the
// vocabulary and the keyframe database of ONE stream.
class LoopCompute {
 public:
  virtual ~LoopCompute() = default;
  // ssx_kfdb_process_keyframe: ProcessNewKeyframe + DetectLoop + MatchFeatures.  pairs = res.n_pairs x (current feature, loop feature),
  // ascending; the keyframe stays pending on the device until AddPending or the next ProcessKeyframe.
  virtual void ProcessKeyframe(int64_t kf_id, const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels,
                               int min_db_size, int min_id_gap, float threshold, ssx_kfdb_step_result& res, std::vector<int32_t>& pairs) = 0;
  virtual void AddPending() = 0;                                                // ssx_kfdb_add_pending (AddToKeyframeDatabase)
  // ssx_loop_compute_pose with the reference's 100 hypotheses: kept[i] = pair i is still in set_valid_feature_matches_
  virtual void ComputePose(int n_pairs, const double* loop_xyz, const uint8_t* has_point, const double* cur_uv, const double* T_cur, const double* T_loop,
                           const double* K4, uint8_t* kept, ssx_loop_pose_result& out) = 0;
  // ssx_loop_correct with optimize(20): prob.poses / prob.points are corrected in place
  virtual void LoopCorrect(const ssx_loop_correct_problem& prob, ssx_loop_correct_result& res) = 0;
  // Relocalisation (LoopClosing::Relocalize).  ssx_kfdb_relocalize_query: the stored keyframes a frame resembles, best first, and its
  // feature matches against each; pairs[c] = res.cand[c].n_pairs x (frame feature, keyframe feature), ascending.  The database and
  // its pending keyframe are only read.
  virtual void RelocalizeQuery(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, int max_candidates,
                               float threshold, float ratio, ssx_reloc_query_result& res, std::vector<std::vector<int32_t>>& pairs)
  {
    (void)img; (void)features; (void)prm; (void)pyramid_levels; (void)max_candidates; (void)threshold; (void)ratio; (void)res; (void)pairs;
    throw std::logic_error("LoopCompute::RelocalizeQuery: this implementation cannot relocalise");
  }
  // ssx_pnp_pose_batch with the reference's 100 hypotheses, 5.991 px, chi2 5.991 and Huber 1.0: one pose per job
  virtual void PosesBatch(const double* K4, std::vector<ssx_pnp_pose_job>& jobs)
  {
    (void)K4; (void)jobs;
    throw std::logic_error("LoopCompute::PosesBatch: this implementation cannot relocalise");
  }
  // The second step of relocalisation (Relocalization.Guided.Open: 1; the rule: tools/guided_model.py).  ssx_kfdb_guided_search: P map
  // points, each with the stored keyframe and the feature index there that hold its descriptors, projected into the frame with T_cw12 =
  // [R|t] row-major and matched in a window against the features that are not taken.  Per point the frame's feature (-1 unless matched),
  // the two distances and the ssx_guided_status.  The database and its pending keyframe are only read.
  struct GuidedParams { double radius = 10.0; int max_distance = 50, ratio_pct = 90; };
  struct GuidedMatches { std::vector<int32_t> feat, d1, d2, status; int n_matched = 0; };
  virtual void GuidedSearch(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int pyramid_levels, const std::vector<uint8_t>& taken,
                            const double* K4, const double* T_cw12, const std::vector<int64_t>& point_kf, const std::vector<int32_t>& point_cls,
                            const std::vector<double>& xyz, const GuidedParams& gp, GuidedMatches& out)
  {
    (void)img; (void)features; (void)prm; (void)pyramid_levels; (void)taken; (void)K4; (void)T_cw12; (void)point_kf; (void)point_cls; (void)xyz; (void)gp; (void)out;
    throw std::logic_error("LoopCompute::GuidedSearch: this implementation has no guided search");
  }
  // ssx_loop_pose_opt with chi2 5.991 and Huber 1.0 from pose_io over M pairs; *found = 0 when the refinement has no finite pose
  virtual void RefinePose(const double* K4, int M, const double* xyz, const double* uv, double* pose_io, uint8_t* inlier_out, int* n_inliers, int* found)
  {
    (void)K4; (void)M; (void)xyz; (void)uv; (void)pose_io; (void)inlier_out; (void)n_inliers; (void)found;
    throw std::logic_error("LoopCompute::RefinePose: this implementation has no guided search");
  }
};

class Compute {
 public:
  virtual ~Compute() = default;
  virtual void Detect(const Image& img, const uint8_t* mask, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps) = 0;
  // FrontEnd::DetectFeatures' mask (frontend.cpp:302-312) as its rectangles: boxes = n x (x0, y0, x1, y1), corners inclusive and inside
  // the image.  Default: rasterise on the host and call Detect (the CPU oracle's Compute); the GPU library takes the rectangles
  // themselves (ssx_orb_detect_boxes: 16 bytes per tracked feature over PCIe instead of a 466 KB mask).
  virtual void DetectBoxes(const Image& img, const std::vector<int32_t>& boxes, const ssx_orb_params& prm, std::vector<ssx_keypoint>& kps)
  {
    std::vector<uint8_t> mask((size_t)img.rows * img.cols, 255);
    for (size_t b = 0; b + 3 < boxes.size(); b += 4)
      for (long y = boxes[b + 1]; y <= boxes[b + 3]; ++y)
        for (long x = boxes[b]; x <= boxes[b + 2]; ++x) mask[(size_t)y * img.cols + x] = 0;
    Detect(img, mask.data(), prm, kps);
  }
  // Camera::UndistortImage on the frame's two images (frontend.cpp:39-45), prm[0] the left camera's, prm[1] the right one's.  An
  // implementation without it says so, and a FrontEnd with Camera.NeedUndistortion set refuses to be built on it (the CPU oracle of
  // the tests: there is no CPU fallback).  left_out / right_out get the size of the inputs; their ids are the caller's.
  virtual bool CanUndistort() const { return false; }
  virtual void UndistortPair(const Image& left, const Image& right, const ssx_undistort_params prm[2], Image& left_out, Image& right_out)
  {
    (void)left; (void)right; (void)prm; (void)left_out; (void)right_out;
    throw std::logic_error("Compute::UndistortPair: this implementation cannot undistort images (Camera.NeedUndistortion)");
  }
  // Camera.Rectify: the frame's raw pair warped into the common rectified camera, each image through its own lens (radtan or kb4) and
  // rectifying rotation -- prm[0], prm[1] as ssx_stereo_rectify returns them.  It takes the place of UndistortPair,
  // under the same rules: an implementation without it says so and a FrontEnd with the key set refuses to be built on it.
  virtual bool CanRectify() const { return false; }
  virtual void RectifyPair(const Image& left, const Image& right, const ssx_lens_params prm[2], Image& left_out, Image& right_out)
  {
    (void)left; (void)right; (void)prm; (void)left_out; (void)right_out;
    throw std::logic_error("Compute::RectifyPair: this implementation cannot rectify images (Camera.Rectify)");
  }
  // Dense.Open: the disparity map of a keyframe's rectified pair by census + semi-global matching (ssx_stereo_dense; the contract is
  // tools/dense_model.py): disp = rows x cols int16 in 1/16 pixel, -16 where a pixel is invalid.  The rules of UndistortPair: an
  // implementation without it says so and a FrontEnd with the key set refuses to be built on it.
  virtual bool CanDense() const { return false; }
  virtual void DenseDisparity(const Image& left, const Image& right, const ssx_dense_params& prm, std::vector<int16_t>& disp)
  {
    (void)left; (void)right; (void)prm; (void)disp;
    throw std::logic_error("Compute::DenseDisparity: this implementation has no dense stereo (Dense.Open)");
  }
  // Dense.Speckle.Size / Dense.Cloud.OnDevice: the keyframe's whole dense step in one call (ssx_stereo_dense_post; the
  // contract is tools/dense_post_model.py) -- the map of DenseDisparity, the speckle filter of post, and with post.cloud_stride > 0 the
  // samples of the filtered map in raster order.  want_map = false (only with samples): no map comes down and disp is left empty.
  virtual bool CanDensePost() const { return false; }
  virtual void DenseKeyframe(const Image& left, const Image& right, const ssx_dense_params& prm, const ssx_dense_post& post, bool want_map,
                             std::vector<int16_t>& disp, std::vector<ssx_dense_sample>& samples)
  {
    (void)left; (void)right; (void)prm; (void)post; (void)want_map; (void)disp; (void)samples;
    throw std::logic_error("Compute::DenseKeyframe: this implementation has no speckle filter and no samples on the device (Dense.Speckle.Size, Dense.Cloud.OnDevice)");
  }
  // 11x11 window, 3 levels, (COUNT+EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW: next_pts holds the guesses going in.
  // `temporal` marks the frame-to-frame call (the implementation may keep the previous frame's pyramid).
  virtual void TrackLK(const Image& prev, const Image& next, const std::vector<float>& prev_pts, std::vector<float>& next_pts,
                       std::vector<uint8_t>& status, bool temporal) = 0;
  // 4 rounds x 10 iterations, chi2 5.991, Huber 1.0; returns features.size() - outliers
  virtual int PoseOnly(double* pose_io, const double* K4, int M, const double* xyz, const double* uv, uint8_t* inlier) = 0;
  virtual void Triangulate(int n, const double* uvL, const double* uvR, const ssx_stereo_rig& rig, const double* T_wc, double* xyz,
                           uint8_t* ok) = 0;
  // res.poses_out / points_out / edge_outlier point at caller storage
  virtual void BundleAdjust(const ssx_ba_problem& prob, const ssx_ba_options& opt, ssx_ba_result& res) = 0;
  // a resident window with the first-observer rule of backend.cpp:125-130 switched on, or null when the implementation has
  // none (the backend then re-marshals its map per keyframe)
  virtual std::unique_ptr<BaWindow> MakeBaWindow(const double* K4, const double* cam_ext14, const ssx_ba_options& opt)
  {
    (void)K4; (void)cam_ext14; (void)opt;
    return nullptr;
  }
  // the loop-closing calls on a context of their own, with the vocabulary of DBOW2.VOC.Path loaded (throws when it cannot be read),
  // or null when the implementation has none (the CPU oracle of the tests: the system then runs without loop closing)
  virtual std::unique_ptr<LoopCompute> MakeLoopCompute(const std::string& voc_path)
  {
    (void)voc_path;
    return nullptr;
  }
};

// device: GPU ordinal.  Three contexts (streams): per-frame work, the temporal LK chain, the backend; loop closing adds a fourth.
std::unique_ptr<Compute> MakeSsxCompute(int device = 0);

}  // namespace ssx::host
