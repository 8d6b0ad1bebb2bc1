// tests/host/test_rectify_units.cpp -- CPU: the host path of Camera.Rectify (System, FrontEnd::GrabSteroImage, System::Warmup) on a Compute
// that records what it is asked.  No device: ssx_stereo_rectify is host arithmetic, the Compute's rectification is a marker (255 - v),
// its detector finds nothing.  Prints "name value" lines; tests/test_rectify_host.py asserts on them.
//   argv: <settings with Camera.Rectify set> <the same with the key 0> <the same with both keys set>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ssvio_amd/host/system.hpp"

using namespace ssx::host;

namespace {

struct Recorder {
  int rectify_calls = 0, undistort_calls = 0, detect_calls = 0;
  ssx_lens_params prm[2] = {};
  uint64_t in_left_id = 0, in_right_id = 0, detect_id = 0;
  int detect_first_byte = -1, order_ok = 1;
};

class StubCompute final : public Compute {
 public:
  StubCompute(Recorder& r, bool can) : r_(r), can_(can) {}
  bool CanUndistort() const override { return true; }
  void UndistortPair(const Image&, const Image&, const ssx_undistort_params*, Image&, Image&) override { ++r_.undistort_calls; }
  bool CanRectify() const override { return can_; }
  void RectifyPair(const Image& left, const Image& right, const ssx_lens_params prm[2], Image& lo, Image& ro) override
  {
    if (r_.detect_calls != r_.rectify_calls) r_.order_ok = 0;        // nothing looked at this frame before it was rectified (a frame here: one call of each)
    ++r_.rectify_calls;
    r_.prm[0] = prm[0]; r_.prm[1] = prm[1];
    r_.in_left_id = left.id; r_.in_right_id = right.id;
    lo.rows = ro.rows = left.rows; lo.cols = ro.cols = left.cols;
    lo.data.resize(left.data.size()); ro.data.resize(right.data.size());
    for (size_t i = 0; i < left.data.size(); ++i) { lo.data[i] = (uint8_t)(255 - left.data[i]); ro.data[i] = (uint8_t)(255 - right.data[i]); }
  }
  void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override { kps.clear(); }
  void DetectBoxes(const Image& img, const std::vector<int32_t>&, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override
  {
    ++r_.detect_calls;
    r_.detect_id = img.id; r_.detect_first_byte = img.data.empty() ? -1 : img.data[0];
    kps.clear();
  }
  void TrackLK(const Image&, const Image&, const std::vector<float>&, std::vector<float>&, std::vector<uint8_t>&, bool) override { throw std::logic_error("TrackLK: not reached"); }
  int PoseOnly(double*, const double*, int, const double*, const double*, uint8_t*) override { throw std::logic_error("PoseOnly: not reached"); }
  void Triangulate(int, const double*, const double*, const ssx_stereo_rig&, const double*, double*, uint8_t*) override { throw std::logic_error("Triangulate: not reached"); }
  void BundleAdjust(const ssx_ba_problem&, const ssx_ba_options&, ssx_ba_result&) override { throw std::logic_error("BundleAdjust: not reached"); }

 private:
  Recorder& r_;
  bool can_;
};

ImagePtr make_image(uint64_t id, uint8_t v)
{
  auto im = std::make_shared<Image>();
  im->rows = 64; im->cols = 96; im->id = id; im->data.assign((size_t)64 * 96, v);
  return im;
}

void print_lens(const char* name, const ssx_lens_params& p)
{
  std::printf("%s %d %d", name, p.model, p.reserved);
  for (double v : p.K) std::printf(" %.17g", v);
  for (double v : p.coeffs) std::printf(" %.17g", v);
  for (double v : p.iR) std::printf(" %.17g", v);
  std::printf("\n");
}

void print_camera(const char* name, const Camera& c)
{
  std::printf("%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", name, c.fx, c.fy, c.cx, c.cy, c.baseline, c.pose.d[4], c.pose.d[5], c.pose.d[6]);
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc != 4) return 2;
  const std::string on = argv[1], off = argv[2], both = argv[3];
  // 1. the key set on a Compute that cannot rectify: refused at construction, naming the key
  {
    Recorder r;
    try {
      System sys(on, std::make_unique<StubCompute>(r, false));
      std::printf("refused 0\n");
    } catch (const std::exception& e) {
      std::printf("refused %d\n", std::strstr(e.what(), "Camera.Rectify") ? 1 : -1);
    }
  }
  // 2. both keys: refused, naming both
  {
    Recorder r;
    try {
      System sys(both, std::make_unique<StubCompute>(r, true));
      std::printf("both_refused 0\n");
    } catch (const std::exception& e) {
      std::printf("both_refused %d\n", std::strstr(e.what(), "Camera.Rectify") && std::strstr(e.what(), "Camera.NeedUndistortion") ? 1 : -1);
    }
  }
  // 3. the key set on one that can: one call per frame, before anything else, with what ssx_stereo_rectify returns; the rectified cameras
  {
    Recorder r;
    System sys(on, std::make_unique<StubCompute>(r, true));
    sys.RunStep(make_image(1001, 10), make_image(1002, 20), 0.0);
    std::printf("on_rectify_calls %d\non_undistort_calls %d\non_detect_calls %d\non_order_ok %d\n", r.rectify_calls, r.undistort_calls, r.detect_calls, r.order_ok);
    std::printf("on_inputs %lu %lu\n", (unsigned long)r.in_left_id, (unsigned long)r.in_right_id);
    const auto& f = sys.frontend().current_frame();
    std::printf("on_frame_ids %lu %lu\n", (unsigned long)f->left_image->id, (unsigned long)f->right_image->id);
    std::printf("on_frame_bytes %d %d\n", (int)f->left_image->data[0], (int)f->right_image->data[0]);
    std::printf("on_detect %lu %d\n", (unsigned long)r.detect_id, r.detect_first_byte);
    print_lens("on_left", r.prm[0]);
    print_lens("on_right", r.prm[1]);
    print_camera("on_left_camera", sys.left_camera());
    print_camera("on_right_camera", sys.right_camera());
    const ssx_stereo_rectified* rect = sys.rectified();
    std::printf("on_rectified %d\n", rect ? 1 : 0);
    if (rect) {
      std::printf("on_R_l");
      for (double v : rect->R_l) std::printf(" %.17g", v);
      std::printf("\n");
    }
    std::printf("on_stopwatch %ld\n", sys.frontend().times().n_undistort);
    sys.RunStep(make_image(1003, 30), make_image(1004, 40), 0.1);
    std::printf("on_second_frame_calls %d\n", r.rectify_calls);
    const int before = r.rectify_calls;
    sys.Warmup(64, 96);
    std::printf("on_warmup_calls %d\non_stopwatch_after_warmup %ld\n", r.rectify_calls - before, sys.frontend().times().n_undistort);
  }
  // 4. the key 0 (the raw rig's keys all present): nothing new is called, the cameras are the settings', the frame keeps its images
  for (int can = 0; can < 2; ++can) {
    Recorder r;
    System sys(off, std::make_unique<StubCompute>(r, can != 0));
    sys.RunStep(make_image(2001, 10), make_image(2002, 20), 0.0);
    sys.Warmup(64, 96);
    std::printf("off%d_calls %d %d\n", can, r.rectify_calls, r.undistort_calls);
    std::printf("off%d_frame_ids %lu %lu\n", can, (unsigned long)sys.frontend().current_frame()->left_image->id, (unsigned long)sys.frontend().current_frame()->right_image->id);
    std::printf("off%d_rectified %d\n", can, sys.rectified() ? 1 : 0);
    print_camera(can ? "off1_right_camera" : "off0_right_camera", sys.right_camera());
  }
  // 5. the default of the interface throws a logic_error that names the key
  {
    struct Plain final : Compute {
      void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>&) override {}
      void TrackLK(const Image&, const Image&, const std::vector<float>&, std::vector<float>&, std::vector<uint8_t>&, bool) override {}
      int PoseOnly(double*, const double*, int, const double*, const double*, uint8_t*) override { return 0; }
      void Triangulate(int, const double*, const double*, const ssx_stereo_rig&, const double*, double*, uint8_t*) override {}
      void BundleAdjust(const ssx_ba_problem&, const ssx_ba_options&, ssx_ba_result&) override {}
    } plain;
    Image a, b;
    const ssx_lens_params prm[2] = {};
    int verdict = plain.CanRectify() ? -2 : 0;
    try { plain.RectifyPair(a, b, prm, a, b); } catch (const std::logic_error& e) { if (verdict == 0) verdict = std::strstr(e.what(), "Camera.Rectify") ? 1 : -1; }
    std::printf("default_throws %d\n", verdict);
  }
  return 0;
}
