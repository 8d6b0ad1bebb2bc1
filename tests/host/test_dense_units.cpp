// tests/host/test_dense_units.cpp -- CPU: the host path of Dense.Open (FrontEnd::InsertKeyFrame, the keyframe's samples, System::Warmup,
// System::SaveDenseCloud) on a Compute that records what it is asked.  No device: the stub's detector returns a grid, its LK and
// triangulation accept everything, its pose-only step returns a made pose and too few inliers for TRACKING_GOOD (so every frame
// becomes a keyframe), and its disparity map is a formula of (u, v, call) that tests/test_dense_host.py restates.
// Prints "name value..." lines; the Python test asserts on them.
//   argv: <settings with Dense.Open: 1 and the Dense.* keys> <the same without any Dense.* key> <output PLY> <output PLY of the run without the key>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>

#include "ssvio_amd/host/system.hpp"

using namespace ssx::host;

namespace {

constexpr int ROWS = 64, COLS = 96;

struct Recorder {
  int dense_calls = 0, pose_calls = 0;
  bool quiet = false;                                   // System::Warmup: the detector finds nothing, so only the warmed calls run
  std::vector<uint64_t> left_ids, right_ids;
  std::vector<ssx_dense_params> prm;
};

class StubCompute final : public Compute {
 public:
  StubCompute(Recorder& r, bool can) : r_(r), can_(can) {}
  bool CanDense() const override { return can_; }
  void DenseDisparity(const Image& left, const Image& right, const ssx_dense_params& prm, std::vector<int16_t>& disp) override
  {
    const int call = r_.dense_calls++;
    r_.left_ids.push_back(left.id); r_.right_ids.push_back(right.id); r_.prm.push_back(prm);
    disp.resize((size_t)left.rows * left.cols);
    for (int v = 0; v < left.rows; ++v)
      for (int u = 0; u < left.cols; ++u)
        disp[(size_t)v * left.cols + u] = (u * 7 + v * 13 + call) % 11 == 0 ? (int16_t)-16 : (int16_t)(16 + (u * 5 + v * 3 + 40 * call) % 900);
  }
  void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override { kps.clear(); }
  void DetectBoxes(const Image& img, const std::vector<int32_t>& boxes, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override
  {
    kps.clear();
    if (r_.quiet) return;
    const bool init = boxes.empty();
    for (int i = 0; i < (init ? 12 : 2); ++i)
      for (int j = 0; j < 25; ++j) kps.push_back(ssx_keypoint{8.f + 3.4f * j + (init ? 0.f : 1.7f), 4.f + 4.9f * i, 7.f, -1.f, 0.f, 0, 0});
    (void)img;
  }
  void TrackLK(const Image&, const Image&, const std::vector<float>& prev, std::vector<float>& next, std::vector<uint8_t>& status, bool temporal) override
  {
    status.assign(prev.size() / 2, 1);
    if (!temporal)
      for (size_t i = 0; i < prev.size(); i += 2) { next[i] = prev[i] - 4.f; next[i + 1] = prev[i + 1]; }
  }
  int PoseOnly(double* pose_io, const double*, int M, const double*, const double*, uint8_t* inlier) override
  {
    const int k = ++r_.pose_calls;
    const double a = 0.1 * k, n = std::sqrt(0.2 * 0.2 + 0.9 * 0.9 + 0.1 * 0.1), s = std::sin(a / 2) / n;
    const double pose[7] = {0.2 * s, 0.9 * s, 0.1 * s, std::cos(a / 2), 0.3 * k, -0.1 * k, 0.5 * k};
    std::memcpy(pose_io, pose, sizeof pose);
    for (int i = 0; i < M; ++i) inlier[i] = 1;
    return 30;                                          // above numFeatures.trackingBad, below trackingGood: the frame becomes a keyframe
  }
  void Triangulate(int n, const double* uvL, const double*, const ssx_stereo_rig&, const double*, double* xyz, uint8_t* ok) override
  {
    for (int i = 0; i < n; ++i) { xyz[3 * i] = (uvL[2 * i] - 48.0) / 50.0; xyz[3 * i + 1] = (uvL[2 * i + 1] - 32.0) / 50.0; xyz[3 * i + 2] = 10.0; ok[i] = 1; }
  }
  void BundleAdjust(const ssx_ba_problem&, const ssx_ba_options&, ssx_ba_result&) override { throw std::logic_error("BundleAdjust: not reached (Backend.Open: 0)"); }

 private:
  Recorder& r_;
  bool can_;
};

ImagePtr make_image(uint64_t id, int salt)
{
  auto im = std::make_shared<Image>();
  im->rows = ROWS; im->cols = COLS; im->id = id; im->data.resize((size_t)ROWS * COLS);
  for (size_t i = 0; i < im->data.size(); ++i) im->data[i] = (uint8_t)((i * 31 + (size_t)salt * 17) % 251);
  return im;
}

void drive(System& sys, int frames)
{
  for (int k = 0; k < frames; ++k) sys.RunStep(make_image(1001 + 2 * k, k), make_image(1002 + 2 * k, k + 100), 0.1 * k);
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc != 5) return 2;
  const std::string on = argv[1], off = argv[2], ply_on = argv[3], ply_off = argv[4];
  // 1. the key set on a Compute without dense stereo: refused at construction, naming the key
  {
    Recorder r;
    try {
      System sys(on, std::make_unique<StubCompute>(r, false));
      std::printf("refused 0\n");
    } catch (const std::exception& e) {
      std::printf("refused %d\n", std::strstr(e.what(), "Dense.Open") ? 1 : -1);
    }
  }
  // 2. the key set: one call per keyframe with the frame's own pair and the settings' parameters; the samples; the cloud
  {
    Recorder r;
    System sys(on, std::make_unique<StubCompute>(r, true));
    int sink_calls = 0, sink_ok = 1;
    sys.frontend().SetDenseSink([&](unsigned long kf_id, const std::vector<int16_t>& disp, int rows, int cols) {
      if ((int)kf_id != sink_calls || rows != ROWS || cols != COLS || disp.size() != (size_t)ROWS * COLS) sink_ok = 0;
      ++sink_calls;
    });
    drive(sys, 4);
    const auto& kfs = sys.map().GetAllKeyFrames();
    std::printf("on_keyframes %zu\non_dense_calls %d\non_stopwatch %ld\non_sink %d %d\n", kfs.size(), r.dense_calls, sys.frontend().times().n_dense, sink_calls, sink_ok);
    for (int c = 0; c < r.dense_calls; ++c) {
      const ssx_dense_params& p = r.prm[(size_t)c];
      std::printf("on_call%d %lu %lu %d %d %d %d %d %d %d %d\n", c, (unsigned long)r.left_ids[(size_t)c], (unsigned long)r.right_ids[(size_t)c], p.disparities, p.p1, p.p2,
                  p.uniqueness, p.lr_tolerance, p.paths, p.reserved[0], p.reserved[1]);
    }
    const DenseConfig& dc = sys.frontend().dense();
    std::printf("on_cloud_config %d %.17g\n", dc.cloud_stride, dc.cloud_max_depth);
    std::printf("on_camera %.17g %.17g %.17g %.17g %.17g\n", sys.left_camera().fx, sys.left_camera().fy, sys.left_camera().cx, sys.left_camera().cy, sys.right_camera().baseline);
    // the poses move after insertion (what BA and a loop correction do): the cloud is written with the poses as they are at the end
    std::map<unsigned long, KeyFramePtr> ordered(kfs.begin(), kfs.end());
    for (auto& kv : ordered) {
      kv.second->pose = SE3::translation(0.01 * (double)(kv.first + 1), 0.02, -0.03) * kv.second->pose;
      std::printf("on_kf %lu %lu", kv.first, kv.second->frame_id);
      for (double v : kv.second->pose.d) std::printf(" %.17g", v);
      std::printf("\n");
      std::printf("on_samples %lu", kv.first);
      for (const DenseSample& s : kv.second->dense_samples) std::printf(" %d %d %d %d", (int)s.u, (int)s.v, (int)s.disp16, (int)s.intensity);
      std::printf("\n");
    }
    std::printf("on_cloud_points %zu\n", sys.SaveDenseCloud(ply_on));
    const int before = r.dense_calls;
    r.quiet = true;
    sys.Warmup(ROWS, COLS);
    std::printf("on_warmup_calls %d\non_stopwatch_after_warmup %ld\n", r.dense_calls - before, sys.frontend().times().n_dense);
  }
  // 3. no Dense.* key at all: nothing new is called, whatever the Compute can do; the keyframes carry no samples; the cloud is empty
  for (int can = 0; can < 2; ++can) {
    Recorder r;
    System sys(off, std::make_unique<StubCompute>(r, can != 0));
    drive(sys, 4);
    r.quiet = true;
    sys.Warmup(ROWS, COLS);
    size_t samples = 0;
    for (auto& kv : sys.map().GetAllKeyFrames()) samples += kv.second->dense_samples.size();
    std::printf("off%d %zu %d %zu %d %zu\n", can, sys.map().GetAllKeyFrames().size(), r.dense_calls, samples, sys.frontend().dense().open ? 1 : 0, sys.SaveDenseCloud(ply_off));
    const ssx_dense_params& p = sys.frontend().dense().prm;
    std::printf("off%d_defaults %d %d %d %d %d %d %d %.17g\n", can, p.disparities, p.p1, p.p2, p.uniqueness, p.lr_tolerance, p.paths, sys.frontend().dense().cloud_stride,
                sys.frontend().dense().cloud_max_depth);
  }
  // 4. the default of the interface throws a logic_error that names the key
  {
    struct Plain final : Compute {
      void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>&) override {}
      void TrackLK(const Image&, const Image&, const std::vector<float>&, std::vector<float>&, std::vector<uint8_t>&, bool) override {}
      int PoseOnly(double*, const double*, int, const double*, const double*, uint8_t*) override { return 0; }
      void Triangulate(int, const double*, const double*, const ssx_stereo_rig&, const double*, double*, uint8_t*) override {}
      void BundleAdjust(const ssx_ba_problem&, const ssx_ba_options&, ssx_ba_result&) override {}
    } plain;
    Image a, b;
    ssx_dense_params prm;
    ssx_dense_default_params(&prm);
    std::vector<int16_t> d;
    int verdict = plain.CanDense() ? -2 : 0;
    try { plain.DenseDisparity(a, b, prm, d); } catch (const std::logic_error& e) { if (verdict == 0) verdict = std::strstr(e.what(), "Dense.Open") ? 1 : -1; }
    std::printf("default_throws %d\n", verdict);
  }
  return 0;
}
