// ssvio_amd/host/system.hpp -- ssvio::System without the viewer (/root/reference/src/ssvio/system.cpp:9-128):
// reads the settings file, builds the stereo rig (GenerateSteroCamera :54-113), the two extractor settings
// (GenerateORBextractor :115-128), the distortion coefficients when Camera.NeedUndistortion is set (:73-94), Map, Backend, FrontEnd and -- with Loop.Closing.Open set -- LoopClosing (:17-41);
// RunStep = FrontEnd::GrabSteroImage (:46-52).
// SaveTrajectoryTUM is the trajectory writer the reference keeps in its viewer
// (/root/reference/src/ui/pangolin_window_impl.cpp:362-395): every keyframe in id order,
// "timestamp tx ty tz qx qy qz qw" of T_wc, fixed notation with 6 decimals.
#pragma once
#include <memory>
#include <string>

#include "backend.hpp"
#include "compute.hpp"
#include "frontend.hpp"
#include "loopclosing.hpp"
#include "map.hpp"
#include "setting.hpp"

namespace ssx::host {

class System {
 public:
  // compute: the implementation to run on; null = MakeSsxCompute(device)
  // Loop.Closing.Open != 0: LoopClosing is built on Compute::MakeLoopCompute(DBOW2.VOC.Path) and attached to the backend; throws,
  // naming the key, when the vocabulary cannot be read.  A Compute without loop closing (MakeLoopCompute returns null: the CPU
  // oracle of the tests) gets one warning line and a system without it.
  // Camera.Rectify != 0: the settings state a RAW rig -- Camera{1,2}.fx fy cx cy, Camera{1,2}.Model (radtan, the default, or
  // kb4), Camera{1,2}.k1 k2 p1 p2 k3 (radtan) or k1 k2 k3 k4 (kb4), Stereo.R21.0 .. .8 and Stereo.t21.0 .. .2 (X_right = R21 X_left +
  // t21), optionally Camera.Rectified.f / .cx / .cy -- all read as double.  ssx_stereo_rectify makes the common camera: both Camera
  // objects get its intrinsics, the right one sits at (-baseline, 0, 0), Camera.Base.Line is ignored (one line says so), and every
  // frame's pair goes through Compute::RectifyPair first.  The trajectory is in the RECTIFIED left frame; R_l is printed once.  A rig
  // ssx_stereo_rectify refuses, an unknown Model, or both keys (with Camera.NeedUndistortion) throw, naming the keys.
  explicit System(const std::string& config_file_path, std::unique_ptr<Compute> compute = nullptr, int device = 0);
  ~System();

  bool RunStep(ImagePtr left, ImagePtr right, double timestamp);
  // One synthetic keyframe + two tracked frames of rows x cols through every compute call the loop makes (masked detection, stereo
  // and chained temporal LK, triangulation, pose-only LM, a window that grows to Map.ActiveMap.Size keyframes and slides once), results discarded: the GPU library loads
  // its kernels and sizes its workspaces here (15 - 20 ms for the first window solve alone) instead of inside the first frames.
  // Touches neither the map nor the tracker; a run with and without it writes the same trajectory.
  void Warmup(int rows, int cols);
  void SaveTrajectoryTUM(const std::string& path = std::string()) const;   // empty: Trajectory.Save.Path of the settings
  // Dense.Open: the dense cloud of the run as one binary little-endian PLY (x y z float, intensity uchar), every keyframe in id order
  // and its samples in row order.  Per sample in f64: z = bf * 16 / disp16 with bf = fx * baseline, Xc = ((u - cx) z / fx, (v - cy) z / fy,
  // z), Xw = T_wc Xc with the keyframe's pose as it is NOW (after BA and any loop correction), then cast to float.  Under
  // Camera.Rectify this is the rectified left frame, as the trajectory is.  Returns the number of points written.
  size_t SaveDenseCloud(const std::string& path) const;

  const Setting& setting() const { return setting_; }
  Map& map() { return *map_; }
  FrontEnd& frontend() { return *frontend_; }
  Backend& backend() { return *backend_; }
  const Camera& left_camera() const { return left_camera_; }
  const Camera& right_camera() const { return right_camera_; }
  const ssx_stereo_rectified* rectified() const { return need_rectify_ ? &rectified_ : nullptr; }   // null: Camera.Rectify is off
  LoopClosing* loop_closing() { return loop_closing_.get(); }              // null: loop closing is off
  void WaitIdle();                                                         // the backend's thread, then the loop thread

 private:
  Setting setting_;
  std::unique_ptr<Compute> compute_;
  Camera left_camera_, right_camera_;
  bool need_undistortion_ = false;                                         // Camera.NeedUndistortion
  ssx_undistort_params undistort_[2] = {};                                 // left, right: K as the cameras', Camera{1,2}.k1/k2/p1/p2, k3 = 0, R = I
  bool need_rectify_ = false;                                              // Camera.Rectify
  ssx_stereo_rectified rectified_ = {};                                    // ssx_stereo_rectify of the raw rig the settings state
  std::shared_ptr<Map> map_;
  std::unique_ptr<Backend> backend_;
  std::unique_ptr<FrontEnd> frontend_;
  std::unique_ptr<LoopClosing> loop_closing_;
};

}  // namespace ssx::host
