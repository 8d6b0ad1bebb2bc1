// tests/host/test_dense_post_units.cpp -- CPU: the host path of Dense.Speckle.Size / Dense.Speckle.Range / Dense.Cloud.OnDevice
// (FrontEnd::InsertKeyFrame, System::Warmup) on a Compute that records what it is asked, in the pattern of test_dense_units.cpp: every
// frame becomes a keyframe, the stub's map is a formula of (u, v, call) and its samples a formula of (i, call) that
// tests/test_dense_post_host.py restates.  Prints "name value..." lines; the Python test asserts on them.
//   argv: settings with <both keys> <Dense.Speckle.Size only> <Dense.Cloud.OnDevice only> <Dense.Open and Dense.Speckle.Range only>
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

struct Call {
  uint64_t left_id, right_id;
  ssx_dense_params prm;
  ssx_dense_post post;
  int want_map;
};

struct Recorder {
  int plain_calls = 0, pose_calls = 0;
  bool quiet = false;
  std::vector<Call> calls;                              // DenseKeyframe
};

int16_t stub_disp(int u, int v, int call) { return (u * 7 + v * 13 + call) % 11 == 0 ? (int16_t)-16 : (int16_t)(16 + (u * 5 + v * 3 + 40 * call) % 900); }

class StubCompute final : public Compute {
 public:
  StubCompute(Recorder& r, bool can_post) : r_(r), can_post_(can_post) {}
  bool CanDense() const override { return true; }
  bool CanDensePost() const override { return can_post_; }
  void DenseDisparity(const Image& left, const Image&, const ssx_dense_params&, std::vector<int16_t>& disp) override
  {
    const int call = r_.plain_calls++;
    disp.resize((size_t)left.rows * left.cols);
    for (int v = 0; v < left.rows; ++v)
      for (int u = 0; u < left.cols; ++u) disp[(size_t)v * left.cols + u] = stub_disp(u, v, call);
  }
  void DenseKeyframe(const Image& left, const Image& right, const ssx_dense_params& prm, const ssx_dense_post& post, bool want_map, std::vector<int16_t>& disp,
                     std::vector<ssx_dense_sample>& samples) override
  {
    const int call = (int)r_.calls.size();
    r_.calls.push_back(Call{left.id, right.id, prm, post, want_map ? 1 : 0});
    disp.clear();
    if (want_map) {
      disp.resize((size_t)left.rows * left.cols);
      for (int v = 0; v < left.rows; ++v)
        for (int u = 0; u < left.cols; ++u) disp[(size_t)v * left.cols + u] = stub_disp(u, v, call);
    }
    samples.clear();
    if (post.cloud_stride > 0)
      for (int i = 0; i < 5 + call; ++i) samples.push_back(ssx_dense_sample{(uint16_t)(3 * i), (uint16_t)call, (int16_t)(100 + i), (uint8_t)(7 * i + call), 0});
  }
  void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override { kps.clear(); }
  void DetectBoxes(const Image&, const std::vector<int32_t>& boxes, const ssx_orb_params&, std::vector<ssx_keypoint>& kps) override
  {
    kps.clear();
    if (r_.quiet) return;
    const bool init = boxes.empty();
    for (int i = 0; i < (init ? 12 : 2); ++i)
      for (int j = 0; j < 25; ++j) kps.push_back(ssx_keypoint{8.f + 3.4f * j + (init ? 0.f : 1.7f), 4.f + 4.9f * i, 7.f, -1.f, 0.f, 0, 0});
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
  bool can_post_;
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

void print_calls(const char* tag, const Recorder& r)
{
  for (size_t c = 0; c < r.calls.size(); ++c) {
    const Call& k = r.calls[c];
    std::printf("%s_call%zu %lu %lu %d %d %d %d %d %d %d %d %d %d %d\n", tag, c, (unsigned long)k.left_id, (unsigned long)k.right_id, k.prm.disparities, k.prm.paths,
                k.post.speckle_size, k.post.speckle_range, k.post.cloud_stride, k.post.cloud_min_disp16, k.post.reserved[0], k.post.reserved[1], k.post.reserved[2],
                k.post.reserved[3], k.want_map);
  }
}

void print_samples(const char* tag, System& sys)
{
  const auto& kfs = sys.map().GetAllKeyFrames();
  std::map<unsigned long, KeyFramePtr> ordered(kfs.begin(), kfs.end());
  for (auto& kv : ordered) {
    std::printf("%s_samples%lu", tag, kv.first);
    for (const DenseSample& s : kv.second->dense_samples) std::printf(" %d %d %d %d", (int)s.u, (int)s.v, (int)s.disp16, (int)s.intensity);
    std::printf("\n");
  }
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc != 5) return 2;
  const std::string both = argv[1], speckle = argv[2], on_device = argv[3], classic = argv[4];
  // 1. a Compute without CanDensePost is refused at construction, naming the key that asks for it
  for (const std::string* cfg : {&both, &speckle, &on_device}) {
    Recorder r;
    const char* tag = cfg == &both ? "both" : (cfg == &speckle ? "speckle" : "on_device");
    try {
      System sys(*cfg, std::make_unique<StubCompute>(r, false));
      std::printf("refused_%s 0\n", tag);
    } catch (const std::exception& e) {
      std::printf("refused_%s %d %d\n", tag, std::strstr(e.what(), "Dense.Speckle.Size") ? 1 : 0, std::strstr(e.what(), "Dense.Cloud.OnDevice") ? 1 : 0);
    }
  }
  // 2. both keys, no sink: one DenseKeyframe call per keyframe, no map asked for, the keyframe keeps exactly what was handed back
  {
    Recorder r;
    System sys(both, std::make_unique<StubCompute>(r, true));
    drive(sys, 4);
    std::printf("both_keyframes %zu\nboth_plain_calls %d\nboth_post_calls %zu\nboth_stopwatch %ld\n", sys.map().GetAllKeyFrames().size(), r.plain_calls, r.calls.size(),
                sys.frontend().times().n_dense);
    print_calls("both", r);
    print_samples("both", sys);
    std::printf("camera %.17g %.17g\n", sys.left_camera().fx, sys.right_camera().baseline);
    const size_t before = r.calls.size();
    r.quiet = true;
    sys.Warmup(ROWS, COLS);
    std::printf("both_warmup %zu %d %d %ld\n", r.calls.size() - before, r.calls.back().want_map, r.plain_calls, sys.frontend().times().n_dense);
  }
  // 3. both keys and a sink: the map is asked for and the sink sees the stub's map
  {
    Recorder r;
    System sys(both, std::make_unique<StubCompute>(r, true));
    int sink_calls = 0, sink_ok = 1;
    sys.frontend().SetDenseSink([&](unsigned long kf_id, const std::vector<int16_t>& disp, int rows, int cols) {
      if ((int)kf_id != sink_calls || rows != ROWS || cols != COLS || disp.size() != (size_t)ROWS * COLS || disp[5 * COLS + 9] != stub_disp(9, 5, sink_calls)) sink_ok = 0;
      ++sink_calls;
    });
    drive(sys, 4);
    std::printf("sink %d %d %d\n", sink_calls, sink_ok, r.plain_calls);
    print_calls("sink", r);
    print_samples("sink", sys);
  }
  // 4. the filter alone: one DenseKeyframe call with no stride, the map always, the samples taken on the host as before
  {
    Recorder r;
    System sys(speckle, std::make_unique<StubCompute>(r, true));
    drive(sys, 4);
    std::printf("speckle_plain_calls %d\n", r.plain_calls);
    print_calls("speckle", r);
    print_samples("speckle", sys);
    const size_t before = r.calls.size();
    r.quiet = true;
    sys.Warmup(ROWS, COLS);
    std::printf("speckle_warmup %zu %d %d\n", r.calls.size() - before, r.calls.back().want_map, r.plain_calls);
  }
  // 5. the samples on the device alone: no filter
  {
    Recorder r;
    System sys(on_device, std::make_unique<StubCompute>(r, true));
    drive(sys, 2);
    std::printf("on_device_plain_calls %d\n", r.plain_calls);
    print_calls("on_device", r);
  }
  // 6. the keys absent or off (Dense.Speckle.Range alone switches nothing on): DenseKeyframe is never called, whatever the Compute can do
  for (int can = 0; can < 2; ++can) {
    Recorder r;
    System sys(classic, std::make_unique<StubCompute>(r, can != 0));
    drive(sys, 4);
    r.quiet = true;
    sys.Warmup(ROWS, COLS);
    std::printf("classic%d %d %zu %d\n", can, r.plain_calls, r.calls.size(), sys.frontend().dense().use_post() ? 1 : 0);
    print_samples(can ? "classic1" : "classic0", sys);
  }
  // 7. the defaults of the interface: cannot, and the call throws a logic_error that names the keys
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
    ssx_dense_post post;
    ssx_dense_default_post(&post);
    std::vector<int16_t> d;
    std::vector<ssx_dense_sample> s;
    int verdict = plain.CanDensePost() ? -2 : 0;
    try { plain.DenseKeyframe(a, b, prm, post, true, d, s); } catch (const std::logic_error& e) {
      if (verdict == 0) verdict = std::strstr(e.what(), "Dense.Speckle.Size") && std::strstr(e.what(), "Dense.Cloud.OnDevice") ? 1 : -1;
    }
    std::printf("default_throws %d\n", verdict);
    std::printf("layout %zu %zu %zu %zu %zu %zu\n", sizeof(ssx_dense_sample), sizeof(DenseSample), offsetof(DenseSample, u), offsetof(DenseSample, v), offsetof(DenseSample, disp16),
                offsetof(DenseSample, intensity));
  }
  return 0;
}
