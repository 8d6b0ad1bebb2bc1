// ssvio_amd/host/frontend.hpp -- the tracking state machine around the compute calls:
//   Camera     /root/reference/src/ssvio/camera.cpp:9-50, include/ssvio/camera.hpp
//   FrontEnd   /root/reference/src/ssvio/frontend.cpp:34-128 (GrabSteroImage / Track), :130-182 TrackLastFrame,
//              :184-300 EstimateCurrentPose, :302-344 DetectFeatures, :346-428 FindFeaturesInRight, :430-446 SteroInit,
//              :448-498 BuidInitMap, :500-544 TriangulateNewPoints, :546-580 InsertKeyFrame
//              Relocalize: what the reference leaves as a TODO in state LOST (:62-66), behind Relocalization.Open
// Every arithmetic step of those functions is a Compute call; what is restated here is the bookkeeping between them.
// Camera.NeedUndistortion != 0 (:39-45): both images of a frame are replaced by Compute::UndistortPair's before anything looks at them; a
// Compute that cannot undistort (the CPU oracle of the tests) is refused at construction.
// Camera.Rectify != 0 (no reference behaviour): the raw pair of a frame is replaced by Compute::RectifyPair's, in the place and
// under the rules of undistortion; the two keys together are refused.
// Dense.Open != 0 (no reference behaviour): InsertKeyFrame hands the keyframe's pair to Compute::DenseDisparity while both images are
// at hand, keeps the cloud's samples on the keyframe and shows the full map to the sink, if there is one; nothing else looks at it.
// Dense.Speckle.Size / Dense.Cloud.OnDevice: one Compute::DenseKeyframe call instead; with the samples made on the device the
// full map comes down only when a sink is attached.
// Not carried over: the viewer hooks (Pangolin), cv::imshow debugging, and the mutexes -- the headless runner is single-threaded.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "compute.hpp"
#include "map.hpp"
#include "setting.hpp"

namespace ssx::host {

struct Camera {
  double fx = 0, fy = 0, cx = 0, cy = 0, baseline = 0;
  SE3 pose;                                          // extrinsic: camera <- rig
  void world2pixel(const double* p_w, const SE3& T_c_w, float* uv) const;   // cv::Point2f(p.x(), p.y()) of Camera::world2pixel
};

class Backend;
class LoopClosing;

enum class FrontendStatus { INITING, TRACKING_GOOD, TRACKING_BAD, LOST };

struct StageTimes {                                   // wall-clock seconds spent inside the compute calls
  double detect = 0, lk_temporal = 0, lk_stereo = 0, pose_only = 0, triangulate = 0, bundle_adjust = 0, undistort = 0, dense = 0;
  long n_detect = 0, n_lk_temporal = 0, n_lk_stereo = 0, n_pose_only = 0, n_triangulate = 0, n_bundle_adjust = 0, n_undistort = 0, n_dense = 0;
};

// Dense.* of the settings.  Every key is absent by default: Dense.Open is off, the matcher's parameters are ssx_dense_default_params',
// the cloud takes every 4th pixel of every 4th row up to 40 m.
// Dense.Speckle.Size (0: no filter), Dense.Speckle.Range (16, in 1/16 pixel) and Dense.Cloud.OnDevice (0): with a filter or
// the samples asked of the device, InsertKeyFrame makes ONE Compute::DenseKeyframe call in place of DenseDisparity; otherwise nothing changes.
struct DenseConfig {
  bool open = false;
  ssx_dense_params prm{};
  int cloud_stride = 4;
  double cloud_max_depth = 40.0;
  int speckle_size = 0, speckle_range = 16;
  bool cloud_on_device = false;
  explicit DenseConfig(const Setting& cfg);
  DenseConfig() { ssx_dense_default_params(&prm); }
  bool use_post() const { return open && (speckle_size > 0 || cloud_on_device); }
  // what DenseKeyframe is asked: the filter, and with Dense.Cloud.OnDevice the stride and the depth bar as one integer (bf = fx * baseline)
  ssx_dense_post PostFor(double bf) const;
};

// the samples a keyframe keeps of its map: every stride-th pixel of every stride-th row with disp16 > 0 and bf * 16 / disp16 <= max_depth (f64)
void SampleDense(const std::vector<int16_t>& disp, const Image& left, int stride, double bf, double max_depth, std::vector<DenseSample>& out);

class FrontEnd {
 public:
  // undistort: the two cameras' parameters (left, right) when Camera.NeedUndistortion is set (System reads Camera{1,2}.k1/k2/p1/p2);
  // with the key set, a null pointer or a Compute that cannot undistort throws, naming the key.
  // rectify: the two lenses (left, right) as ssx_stereo_rectify returns them when Camera.Rectify is set (System reads the raw rig); left
  // and right are then the rectified cameras.  The same refusals, naming that key; both keys set throws, naming both.
  FrontEnd(const Setting& cfg, Compute& compute, std::shared_ptr<Map> map, const Camera& left, const Camera& right,
           const ssx_undistort_params* undistort = nullptr, const ssx_lens_params* rectify = nullptr);
  void SetBackend(Backend* backend) { backend_ = backend; }
  // Relocalization.Open: 1 -- a LOST front-end asks the loop closing's keyframe database where it is (Relocalize below) instead of
  // ignoring every later frame.  Without a LoopClosing the state LOST is final, as in the reference (frontend.cpp:62-66: a TODO).
  void SetLoopClosing(LoopClosing* loop) { loop_ = loop; }

  bool GrabSteroImage(ImagePtr left, ImagePtr right, double timestamp);

  FrontendStatus status() const { return track_status_; }
  const FramePtr& current_frame() const { return current_frame_; }
  const KeyFramePtr& reference_kf() const { return reference_kf_; }
  StageTimes& times() { return times_; }
  const DenseConfig& dense() const { return dense_; }
  // Dense.Open: called with every keyframe's full map (rows x cols int16) at insertion; the map is not kept after the call
  using DenseSink = std::function<void(unsigned long key_frame_id, const std::vector<int16_t>& disp, int rows, int cols)>;
  void SetDenseSink(DenseSink sink) { dense_sink_ = std::move(sink); }

 private:
  bool SteroInit();
  bool BuidInitMap();
  bool Track();
  bool Relocalize();
  int TrackLastFrame();
  int EstimateCurrentPose();
  int DetectFeatures();
  int FindFeaturesInRight();
  int TriangulateNewPoints();
  bool InsertKeyFrame();

  Compute& compute_;
  std::shared_ptr<Map> map_;
  Backend* backend_ = nullptr;
  LoopClosing* loop_ = nullptr;
  Camera left_camera_, right_camera_;
  ssx_orb_params orb_, orb_init_;
  ssx_stereo_rig rig_;

  FrontendStatus track_status_ = FrontendStatus::INITING;
  FramePtr current_frame_, last_frame_;
  KeyFramePtr reference_kf_;
  SE3 relative_motion_;

  int num_features_init_good_, num_features_tracking_good_, num_features_tracking_bad_;
  unsigned min_init_landmark_;
  bool open_backend_optimization_;
  bool need_undistortion_ = false;           // Camera.NeedUndistortion
  ssx_undistort_params undistort_[2] = {};   // left, right
  bool need_rectify_ = false;                // Camera.Rectify
  ssx_lens_params rectify_[2] = {};          // left, right
  std::vector<int32_t> boxes_;               // DetectFeatures: the mask's rectangles (x0, y0, x1, y1)
  std::vector<unsigned long> condemned_;     // EstimateCurrentPose: the map points this frame condemned (taken back when it ends LOST and relocalisation is on)
  DenseConfig dense_;                        // Dense.*
  std::vector<int16_t> dense_disp_;          // the last keyframe's map (reused)
  std::vector<ssx_dense_sample> dense_smp_;  // the last keyframe's samples as the device wrote them (reused)
  DenseSink dense_sink_;
  StageTimes times_;
};

}  // namespace ssx::host
