// include/ssx_shim.hpp -- header-only C++ wrappers over the C ABI (ssx.h) with the method names and argument
// meaning of the reference classes they replace, for a maintainer who wants to swap ssvio's compute bodies
// without touching its callers.  No OpenCV / g2o / Sophus types: images are (pointer, stride, rows, cols),
// keypoints are ssx_keypoint (binary layout of cv::KeyPoint), poses are 7 doubles in Sophus::SE3d::data() order.
// INTEGRATION.md shows the two-line adapters from cv::Mat / std::vector<cv::KeyPoint> / Sophus::SE3d.
//
//   ssx::Context                 one GPU + one stream (create one per ssvio thread: front-end, backend)
//   ssx::ORBextractor            ssvio::ORBextractor (include/ssvio/orbextractor.hpp:44-59)
//   ssx::triangulation           ssvio::triangulation (include/ssvio/algorithm.hpp:23-25) for the stereo rig
//   ssx::BundleAdjuster          the optimisation of Backend::OptimizeActiveMap (src/ssvio/backend.cpp:78-245)
//   ssx::StereoFrontEnd          DetectFeatures + FindFeaturesInRight + triangulation in one device-resident call
//   ssx::calcOpticalFlowPyrLK    cv::calcOpticalFlowPyrLK as frontend.cpp:156-166 / :374-384 call it
//   ssx::Camera                  Camera::UndistortImage (src/ssvio/camera.cpp:43-55), one image or the frame's pair
//   ssx::DenseDisparity          a disparity per pixel of a rectified pair (census + SGM; no counterpart in the reference)
//   ssx::ORBVocabulary           DBoW2 vocabulary: loadFromTextFile / transform / score (loopclosing.cpp:33-41, :84, :633)
//   ssx::KeyframeDatabase        key_frame_database_ with AddToKeyframeDatabase / DetectLoop / MatchFeatures (loopclosing.cpp:72-145, :646)
//   ssx::ComputeCorrectPose      LoopClosing::ComputeCorrectPose / OptimizeCurrentPose (loopclosing.cpp:147-351)
#pragma once
#include <algorithm>
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ssx.h"

namespace ssx {

class Context {
 public:
  explicit Context(int device = 0, void* hip_stream = nullptr)
  {
    if (ssx_abi_check(SSX_VERSION, sizeof(ssx_config), sizeof(ssx_ba_problem), sizeof(ssx_ba_options), sizeof(ssx_ba_result),
                      sizeof(ssx_ba_window_update)) != SSX_OK)
      throw std::runtime_error("libssx.so was built from another version of include/ssx.h than this caller");
    ssx_config cfg{};
    cfg.device = device; cfg.stream = hip_stream;
    const ssx_status st = ssx_ctx_create(&cfg, &ctx_);
    if (st != SSX_OK) throw std::runtime_error("ssx_ctx_create failed (no gfx950 device? there is no CPU fallback)");
  }
  ~Context() { ssx_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  ssx_ctx* get() const { return ctx_; }
  // the reference's compute code signals errors by assert / LOG(FATAL); the shim throws instead of aborting
  void check(ssx_status st) const
  {
    if (st != SSX_OK) throw std::runtime_error(std::string("ssx: ") + ssx_last_error(ctx_));
  }

 private:
  ssx_ctx* ctx_ = nullptr;
};

// ssvio::ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
class ORBextractor {
 public:
  ORBextractor(Context& ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
      : ctx_(ctx), prm_{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST}
  {
  }

  // void Detect(cv::InputArray image, cv::InputArray mask, std::vector<cv::KeyPoint>& keypoints)
  // (orbextractor.cpp:755-842).  Empty image: returns with `keypoints` untouched, like the reference.
  void Detect(const uint8_t* image, int stride, int rows, int cols, const uint8_t* mask, int mask_stride,
              std::vector<ssx_keypoint>& keypoints)
  {
    if (!image || rows <= 0 || cols <= 0) return;
    std::vector<ssx_keypoint> out(capacity());
    int32_t n = 0;
    ctx_.check(ssx_orb_detect(ctx_.get(), image, stride, rows, cols, mask, mask_stride, &prm_, (int32_t)out.size(), out.data(), &n));
    out.resize(n);
    keypoints.swap(out);
  }

  // void DetectAndCompute(InputArray image, InputArray mask, vector<KeyPoint>& keypoints, OutputArray descriptors)
  // (orbextractor.cpp:687-753); descriptors = N x 32 bytes, row-major (CV_8U N x 32)
  void DetectAndCompute(const uint8_t* image, int stride, int rows, int cols, const uint8_t* mask, int mask_stride,
                        std::vector<ssx_keypoint>& keypoints, std::vector<uint8_t>& descriptors)
  {
    if (!image || rows <= 0 || cols <= 0) return;
    std::vector<ssx_keypoint> out(capacity());
    std::vector<uint8_t> desc(out.size() * 32);
    int32_t n = 0;
    ctx_.check(ssx_orb_extract(ctx_.get(), image, stride, rows, cols, mask, mask_stride, &prm_, (int32_t)out.size(), out.data(),
                               desc.data(), &n));
    out.resize(n);
    desc.resize((size_t)n * 32);
    keypoints.swap(out);
    descriptors.swap(desc);
  }

  int GetLevels() const { return prm_.nlevels; }            // orbextractor.hpp:73
  float GetScaleFactor() const { return prm_.scale_factor; }  // orbextractor.hpp:75
  const ssx_orb_params& params() const { return prm_; }

 private:
  // a level can return up to max(budget + 3, 4 * nIni <= 256) keypoints (the first quadtree subdivision)
  size_t capacity() const { return (size_t)prm_.nfeatures + 260 * (size_t)prm_.nlevels + 64; }
  Context& ctx_;
  ssx_orb_params prm_;
};

// bool triangulation(const std::vector<SE3d>& poses, const std::vector<Vector3d> points, Vector3d& pt_world)
// for poses = {left = identity, right = (I, (-baseline,0,0))} (system.cpp:63,71) and pixel inputs; `ok` already
// includes the z > 0 test the callers add (frontend.cpp:466,528).  T_wc (nullable) = current pose inverse.
inline void triangulation(Context& ctx, const ssx_stereo_rig& rig, const std::vector<double>& uvL, const std::vector<double>& uvR,
                          const double* T_wc, std::vector<double>& xyz, std::vector<uint8_t>& ok)
{
  const int32_t n = (int32_t)(uvL.size() / 2);
  xyz.resize((size_t)n * 3);
  ok.resize(n);
  ctx.check(ssx_triangulate(ctx.get(), n, uvL.data(), uvR.data(), &rig, T_wc, xyz.data(), ok.data()));
}

// The optimisation of Backend::OptimizeActiveMap: the caller marshals its active keyframes / map points into flat
// arrays exactly where backend.cpp:88-169 creates vertices and edges, calls Optimize(), and writes the results back
// where backend.cpp:207-244 does.
class BundleAdjuster {
 public:
  explicit BundleAdjuster(Context& ctx) : ctx_(ctx) { ssx_ba_default_options(&opt); }
  ssx_ba_options opt;   // outer_rounds 5, iters 10, chi2 5.891, Huber 5.891, inlier ratio 0.7 (backend.cpp:109,163,175-195)

  // poses / points are updated in place; edge_outlier[e] = 1 where backend.cpp:209 would unlink the observation
  void Optimize(std::vector<double>& poses7, const std::vector<uint8_t>& pose_fixed, std::vector<double>& points3,
                const std::vector<uint8_t>& point_fixed, const std::vector<int32_t>& edge_pose,
                const std::vector<int32_t>& edge_point, const std::vector<double>& edge_uv, const std::vector<uint8_t>& edge_cam,
                const double K[4], const double cam_ext[14], std::vector<uint8_t>& edge_outlier, ssx_ba_result* stats = nullptr)
  {
    ssx_ba_problem p{};
    p.P = (int32_t)(poses7.size() / 7); p.poses = poses7.data(); p.pose_fixed = pose_fixed.empty() ? nullptr : pose_fixed.data();
    p.L = (int32_t)(points3.size() / 3); p.points = points3.data(); p.point_fixed = point_fixed.empty() ? nullptr : point_fixed.data();
    p.E = (int32_t)edge_pose.size(); p.edge_pose = edge_pose.data(); p.edge_point = edge_point.data(); p.edge_uv = edge_uv.data();
    p.edge_cam = edge_cam.empty() ? nullptr : edge_cam.data();
    for (int i = 0; i < 4; ++i) p.K[i] = K[i];
    for (int i = 0; i < 14; ++i) p.cam_ext[i] = cam_ext[i];
    std::vector<double> po(poses7.size()), pt(points3.size());
    edge_outlier.assign(edge_pose.size(), 0);
    ssx_ba_result local{};
    ssx_ba_result* r = stats ? stats : &local;
    r->poses_out = po.data(); r->points_out = pt.data(); r->edge_chi2 = nullptr; r->edge_outlier = edge_outlier.data();
    ctx_.check(ssx_ba_solve(ctx_.get(), &p, &opt, r));
    poses7.swap(po);
    points3.swap(pt);
  }

 private:
  Context& ctx_;
};

// DetectFeatures + FindFeaturesInRight + BuidInitMap/TriangulateNewPoints of the north_star pipeline in one call
class StereoFrontEnd {
 public:
  StereoFrontEnd(Context& ctx, const ssx_orb_params& orb, const ssx_stereo_rig& rig) : ctx_(ctx), orb_(orb), rig_(rig)
  {
    ssx_match_default_params(&mp);
    mp.scale_factor = orb.scale_factor;
  }
  ssx_match_params mp;

  struct Result {
    std::vector<ssx_keypoint> kpsL, kpsR;
    std::vector<uint8_t> descL, descR, ok;
    std::vector<int32_t> match_idx, match_dist;
    std::vector<double> xyz;
    int n_matched = 0, n_triangulated = 0;
  };

  Result Process(const uint8_t* imgL, const uint8_t* imgR, int stride, int rows, int cols, const double* T_wc = nullptr)
  {
    const size_t cap = (size_t)orb_.nfeatures + 260 * (size_t)orb_.nlevels + 64;   // see ORBextractor::capacity()
    Result r;
    r.kpsL.resize(cap); r.kpsR.resize(cap); r.descL.resize(cap * 32); r.descR.resize(cap * 32);
    r.match_idx.resize(cap); r.match_dist.resize(cap); r.xyz.resize(cap * 3); r.ok.resize(cap);
    ssx_stereo_frame_out o{};
    o.cap = (int32_t)cap; o.kpsL = r.kpsL.data(); o.kpsR = r.kpsR.data(); o.descL = r.descL.data(); o.descR = r.descR.data();
    o.match_idx = r.match_idx.data(); o.match_dist = r.match_dist.data(); o.xyz = r.xyz.data(); o.ok = r.ok.data();
    ctx_.check(ssx_stereo_frame(ctx_.get(), imgL, imgR, stride, rows, cols, &orb_, &mp, &rig_, T_wc, &o));
    r.kpsL.resize(o.nL); r.descL.resize((size_t)o.nL * 32); r.kpsR.resize(o.nR); r.descR.resize((size_t)o.nR * 32);
    r.match_idx.resize(o.nL); r.match_dist.resize(o.nL); r.xyz.resize((size_t)o.nL * 3); r.ok.resize(o.nL);
    r.n_matched = o.n_matched; r.n_triangulated = o.n_triangulated;
    return r;
  }

 private:
  Context& ctx_;
  ssx_orb_params orb_;
  ssx_stereo_rig rig_;
};

// cv::calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, status, err, Size(win, win), maxLevel,
//                          TermCriteria(COUNT+EPS, maxCount, epsilon), OPTFLOW_USE_INITIAL_FLOW)
// with cv::Point2f passed as interleaved floats (same layout).  nextPts must hold the initial guesses (as both call
// sites of the reference prepare them); status / err are resized.
inline void calcOpticalFlowPyrLK(Context& ctx, const uint8_t* prevImg, int prevStep, const uint8_t* nextImg, int nextStep,
                                 int rows, int cols, const std::vector<float>& prevPts, std::vector<float>& nextPts,
                                 std::vector<uint8_t>& status, std::vector<float>& err, int win = 11, int maxLevel = 3,
                                 int maxCount = 30, double epsilon = 0.01, bool useInitialFlow = true)
{
  if (prevPts.size() != nextPts.size() || (prevPts.size() & 1)) throw std::invalid_argument("calcOpticalFlowPyrLK: point vectors");
  const int n = (int)(prevPts.size() / 2);
  status.assign(n, 0); err.assign(n, 0.f);
  ssx_lk_params p;
  ssx_lk_default_params(&p);
  p.win = win; p.max_level = maxLevel; p.max_iters = maxCount; p.eps = epsilon; p.use_initial_flow = useInitialFlow ? 1 : 0;
  ctx.check(ssx_lk_track(ctx.get(), prevImg, prevStep, nextImg, nextStep, rows, cols, n, prevPts.data(), nextPts.data(),
                         status.data(), err.data(), &p, nullptr));
}

// The same call for consecutive frames (TrackLastFrame): prevImg is the nextImg of the last call on ctx and is not
// passed again -- its pyramid is still on the device (ssx_lk_track_next).
inline void calcOpticalFlowPyrLKNext(Context& ctx, const uint8_t* nextImg, int nextStep, int rows, int cols,
                                     const std::vector<float>& prevPts, std::vector<float>& nextPts,
                                     std::vector<uint8_t>& status, std::vector<float>& err, int win = 11, int maxLevel = 3,
                                     int maxCount = 30, double epsilon = 0.01, bool useInitialFlow = true)
{
  if (prevPts.size() != nextPts.size() || (prevPts.size() & 1)) throw std::invalid_argument("calcOpticalFlowPyrLK: point vectors");
  const int n = (int)(prevPts.size() / 2);
  status.assign(n, 0); err.assign(n, 0.f);
  ssx_lk_params p;
  ssx_lk_default_params(&p);
  p.win = win; p.max_level = maxLevel; p.max_iters = maxCount; p.eps = epsilon; p.use_initial_flow = useInitialFlow ? 1 : 0;
  ctx.check(ssx_lk_track_next(ctx.get(), nextImg, nextStep, rows, cols, n, prevPts.data(), nextPts.data(), status.data(),
                              err.data(), &p, nullptr));
}

// ssvio::Camera as far as it computes on images: void Camera::UndistortImage(cv::Mat& src, cv::Mat& dst) (camera.cpp:43-55).  The
// constructor takes what Camera's does -- fx fy cx cy and dist_coef_ = (k1, k2, p1, p2), floats widened, as K_cv is built -- and
// fixes R = I, new camera matrix = K (ssx_undistort_default).  src and dst are two buffers (the reference undistorts through a
// clone); host memory unless imagesOnDevice.  UndistortPair is the frame's two images (frontend.cpp:39-45) in one call.
class Camera {
 public:
  Camera(Context& ctx, float fx, float fy, float cx, float cy, float k1 = 0.f, float k2 = 0.f, float p1 = 0.f, float p2 = 0.f) : ctx_(ctx)
  {
    const double K4[4] = {fx, fy, cx, cy}, dist5[5] = {k1, k2, p1, p2, 0.0};
    ssx_undistort_default(K4, dist5, &prm_);
  }
  void UndistortImage(const uint8_t* src, int srcStep, uint8_t* dst, int dstStep, int rows, int cols, bool imagesOnDevice = false) const
  {
    ssx_undistort_job job{src, srcStep, dst, dstStep, prm_};
    ctx_.check(ssx_undistort(ctx_.get(), 1, &job, rows, cols, imagesOnDevice ? 1 : 0));
  }
  const ssx_undistort_params& params() const { return prm_; }

  static void UndistortPair(const Camera& left, const uint8_t* srcLeft, int srcLeftStep, uint8_t* dstLeft, int dstLeftStep, const Camera& right,
                            const uint8_t* srcRight, int srcRightStep, uint8_t* dstRight, int dstRightStep, int rows, int cols,
                            bool imagesOnDevice = false)
  {
    const ssx_undistort_job jobs[2] = {{srcLeft, srcLeftStep, dstLeft, dstLeftStep, left.prm_}, {srcRight, srcRightStep, dstRight, dstRightStep, right.prm_}};
    left.ctx_.check(ssx_undistort(left.ctx_.get(), 2, jobs, rows, cols, imagesOnDevice ? 1 : 0));
  }

  // The raw pair of an unrectified rig warped into its common rectified camera (no counterpart in the reference): lenses[0], lenses[1]
  // are StereoRectify(rig).cam -- either lens model each, the rectifying rotation in iR -- and the two images are one call.
  static void RectifyPair(Context& ctx, const ssx_lens_params lenses[2], const uint8_t* srcLeft, int srcLeftStep, uint8_t* dstLeft, int dstLeftStep,
                          const uint8_t* srcRight, int srcRightStep, uint8_t* dstRight, int dstRightStep, int rows, int cols, bool imagesOnDevice = false)
  {
    const ssx_lens_job jobs[2] = {{srcLeft, srcLeftStep, dstLeft, dstLeftStep, lenses[0]}, {srcRight, srcRightStep, dstRight, dstRightStep, lenses[1]}};
    ctx.check(ssx_undistort_lens(ctx.get(), 2, jobs, rows, cols, imagesOnDevice ? 1 : 0));
  }

 private:
  Context& ctx_;
  ssx_undistort_params prm_{};
};

// ssx_stereo_rectify: the common rectified camera of a raw rig (host arithmetic, no Context); throws std::invalid_argument with the
// reason for a rig that cannot be rectified
inline ssx_stereo_rectified StereoRectify(const ssx_stereo_raw_rig& rig)
{
  ssx_stereo_rectified out{};
  char why[160];
  if (ssx_stereo_rectify(&rig, &out, why, (int32_t)sizeof why) != SSX_OK) throw std::invalid_argument(std::string("ssx::StereoRectify: ") + why);
  return out;
}

// ssx_stereo_dense for one rectified pair (no counterpart in the reference): census + semi-global matching, the bits of
// tools/dense_model.py.  disp: rows x cols int16 at a pitch of dispStep ELEMENTS, in 1/16 pixel, -16 where a pixel is invalid.
// prm = nullptr: ssx_dense_default_params.  Host memory unless imagesOnDevice.
inline void DenseDisparity(Context& ctx, const uint8_t* left, int leftStep, const uint8_t* right, int rightStep, int16_t* disp, int dispStep, int rows,
                           int cols, const ssx_dense_params* prm = nullptr, bool imagesOnDevice = false)
{
  ssx_dense_params def;
  ssx_dense_default_params(&def);
  const ssx_dense_job job = {left, leftStep, right, rightStep, disp, dispStep};
  ctx.check(ssx_stereo_dense(ctx.get(), 1, &job, rows, cols, prm ? prm : &def, imagesOnDevice ? 1 : 0));
}

// ssx_stereo_dense_post for one rectified pair of host images: the map of DenseDisparity, the speckle filter, and with
// post.cloud_stride > 0 the samples of the filtered map in raster order (the bits of tools/dense_post_model.py).  disp may be null
// when samples are asked for: then no map comes down.  samples: null iff post.cloud_stride == 0; resized to what was found.
inline void DenseDisparity(Context& ctx, const uint8_t* left, int leftStep, const uint8_t* right, int rightStep, int16_t* disp, int dispStep, int rows,
                           int cols, const ssx_dense_params& prm, const ssx_dense_post& post, std::vector<ssx_dense_sample>* samples)
{
  const ssx_dense_job job = {left, leftStep, right, rightStep, disp, dispStep};
  ssx_dense_cloud cloud = {nullptr, 0, 0};
  if (samples && post.cloud_stride > 0) {
    const int s = post.cloud_stride;
    samples->resize((size_t)((rows + s - 1) / s) * (size_t)((cols + s - 1) / s));
    cloud.samples = samples->data();
    cloud.capacity = (int32_t)samples->size();
  }
  ctx.check(ssx_stereo_dense_post(ctx.get(), 1, &job, samples ? &cloud : nullptr, rows, cols, &prm, &post, 0));
  if (samples) samples->resize((size_t)cloud.count);
}

// ssx_dense_postprocess on one host map, filtered in place; left is needed only with post.cloud_stride > 0 (samples as above)
inline void DensePostprocess(Context& ctx, int16_t* disp, int dispStep, const uint8_t* left, int leftStep, int rows, int cols, const ssx_dense_post& post,
                             std::vector<ssx_dense_sample>* samples = nullptr)
{
  const ssx_dense_job job = {left, leftStep, nullptr, 0, disp, dispStep};
  ssx_dense_cloud cloud = {nullptr, 0, 0};
  if (samples && post.cloud_stride > 0) {
    const int s = post.cloud_stride;
    samples->resize((size_t)((rows + s - 1) / s) * (size_t)((cols + s - 1) / s));
    cloud.samples = samples->data();
    cloud.capacity = (int32_t)samples->size();
  }
  ctx.check(ssx_dense_postprocess(ctx.get(), 1, &job, samples ? &cloud : nullptr, rows, cols, &post, 0));
  if (samples) samples->resize((size_t)cloud.count);
}

// Many streams' frames in one call (ssx_undistort_plan_*): the plan keeps one stored map per camera it was shown (Add: equal parameter
// bytes -> the index they have) for ONE image size, and Apply undistorts n images, each naming its map, in one launch -- the bytes
// of Camera::UndistortImage.  Destroy the plan before its Context.
class UndistortPlan {
 public:
  UndistortPlan(Context& ctx, int rows, int cols) : ctx_(ctx) { ctx_.check(ssx_undistort_plan_create(ctx_.get(), rows, cols, &plan_)); }
  ~UndistortPlan() { ssx_undistort_plan_destroy(plan_); }
  UndistortPlan(const UndistortPlan&) = delete;
  UndistortPlan& operator=(const UndistortPlan&) = delete;

  int Add(const ssx_undistort_params& prm)
  {
    int32_t m = -1;
    ctx_.check(ssx_undistort_plan_add(plan_, &prm, &m));
    return m;
  }
  int Add(const Camera& camera) { return Add(camera.params()); }
  int AddLens(const ssx_lens_params& lens)              // a lens of either model, e.g. StereoRectify(rig).cam[side]
  {
    int32_t m = -1;
    ctx_.check(ssx_undistort_plan_add_lens(plan_, &lens, &m));
    return m;
  }
  void Apply(const std::vector<ssx_undistort_plan_job>& jobs, bool imagesOnDevice = false)
  {
    ctx_.check(ssx_undistort_plan_apply(plan_, (int32_t)jobs.size(), jobs.data(), imagesOnDevice ? 1 : 0));
  }
  int maps() const
  {
    int32_t n = 0;
    ssx_undistort_plan_size(plan_, nullptr, nullptr, &n);
    return n;
  }
  ssx_undistort_plan* get() const { return plan_; }

 private:
  Context& ctx_;
  ssx_undistort_plan* plan_ = nullptr;
};

// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, include/ssvio/orbvocabulary.hpp:10) as LoopClosing
// uses it: loadFromTextFile, transform(descriptors, BowVector), score(BowVector, BowVector).  A BowVector here is the
// sorted (word id, value) pairs of DBoW2::BowVector (a std::map<WordId, WordValue>).
struct BowVector {
  std::vector<int32_t> ids;
  std::vector<double> values;
  bool empty() const { return ids.empty(); }
};

class ORBVocabulary {
 public:
  explicit ORBVocabulary(Context& ctx) : ctx_(ctx) {}
  ~ORBVocabulary() { ssx_voc_destroy(voc_); }
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;

  bool loadFromTextFile(const std::string& filename)                 // loopclosing.cpp:33-41
  {
    ssx_voc_destroy(voc_);
    voc_ = nullptr;
    return ssx_voc_load_text(ctx_.get(), filename.c_str(), &voc_) == SSX_OK;
  }
  // descriptors: n x 32 bytes (the rows of the CV_8U n x 32 descriptor matrix)
  void transform(const uint8_t* descriptors, int n, BowVector& v) const
  {
    v.ids.assign((size_t)std::max(n, 1), 0);
    v.values.assign((size_t)std::max(n, 1), 0.0);
    int32_t m = 0;
    if (voc_) ctx_.check(ssx_voc_transform(voc_, descriptors, n, nullptr, nullptr, (int32_t)v.ids.size(), v.ids.data(), v.values.data(), &m));
    v.ids.resize(m);
    v.values.resize(m);
  }
  double score(const BowVector& a, const BowVector& b) const
  {
    return ssx_bow_score_l1((int32_t)a.ids.size(), a.ids.data(), a.values.data(), (int32_t)b.ids.size(), b.ids.data(), b.values.data());
  }
  ssx_vocabulary* get() const { return voc_; }               // null until loadFromTextFile has succeeded

 private:
  Context& ctx_;
  ssx_vocabulary* voc_ = nullptr;
};

// LoopClosing's key_frame_database_ (a std::map<unsigned long, KeyFrame::Ptr>) together with the two functions that read it,
// kept on the device.  AddToKeyframeDatabase (loopclosing.cpp:646-649) stores what DetectLoop and MatchFeatures need of a
// keyframe: bow2_vec_, ORBDescriptors_ (n x 32 bytes) and the class_id of every entry of pyramid_key_points_.
class KeyframeDatabase {
 public:
  explicit KeyframeDatabase(Context& ctx, int keyframes_hint = 1024) : ctx_(ctx) { ctx_.check(ssx_kfdb_create(ctx_.get(), keyframes_hint, &db_)); }
  ~KeyframeDatabase() { ssx_kfdb_destroy(db_); }
  KeyframeDatabase(const KeyframeDatabase&) = delete;
  KeyframeDatabase& operator=(const KeyframeDatabase&) = delete;

  // key_frame_database_.insert({current_keyframe_->key_frame_id_, current_keyframe_}); ids ascend as the reference's do
  void AddToKeyframeDatabase(unsigned long key_frame_id, const BowVector& bow, const std::vector<uint8_t>& descriptors,
                             const std::vector<int32_t>& class_ids)
  {
    if (descriptors.size() != class_ids.size() * 32) throw std::invalid_argument("AddToKeyframeDatabase: one class_id per 32-byte descriptor");
    static const uint8_t none = 0;                           // an empty descriptor matrix is still a matrix
    ctx_.check(ssx_kfdb_add(db_, (int64_t)key_frame_id, (int32_t)bow.ids.size(), bow.ids.data(), bow.values.data(), (int32_t)class_ids.size(),
                            class_ids.empty() ? &none : descriptors.data(), class_ids.empty() ? reinterpret_cast<const int32_t*>(&none) : class_ids.data()));
  }

  // bool DetectLoop(): true when a stored keyframe at least 20 ids back scores >= loop_threshold_heigher_ against the current
  // one; loop_key_frame_id is then the id of loop_keyframe_ and *max_score (nullable) the float the reference logs
  bool DetectLoop(unsigned long current_key_frame_id, const BowVector& current_bow, float loop_threshold_heigher, unsigned long& loop_key_frame_id,
                  float* max_score = nullptr, int min_id_gap = 20)
  {
    int32_t found = 0;
    int64_t best = 0;
    float score = 0.f;
    ctx_.check(ssx_kfdb_detect_loop(db_, (int64_t)current_key_frame_id, (int32_t)current_bow.ids.size(), current_bow.ids.data(), current_bow.values.data(),
                                    min_id_gap, loop_threshold_heigher, &found, &best, &score, 0, nullptr, nullptr));
    if (!found) return false;
    loop_key_frame_id = (unsigned long)best;
    if (max_score) *max_score = score;
    return true;
  }

  // MatchFeatures() up to its verdict: set_valid_feature_matches_ = {(current feature id, loop feature id)}; the caller
  // keeps `return set.size() >= 10` (loopclosing.cpp:139)
  std::set<std::pair<int, int>> MatchFeatures(unsigned long loop_key_frame_id, const std::vector<uint8_t>& current_descriptors,
                                              const std::vector<int32_t>& current_class_ids, int* min_distance = nullptr)
  {
    if (current_descriptors.size() != current_class_ids.size() * 32) throw std::invalid_argument("MatchFeatures: one class_id per 32-byte descriptor");
    std::vector<int32_t> pairs(2 * std::max<size_t>(4096, current_class_ids.size()));   // room for a keyframe of the usual size
    int32_t n = 0, md = 0;
    ssx_status st = ssx_kfdb_match_features(db_, (int64_t)loop_key_frame_id, (int32_t)current_class_ids.size(), current_descriptors.data(),
                                            current_class_ids.data(), (int32_t)(pairs.size() / 2), pairs.data(), &n, &md);
    if (st == SSX_ERR_CAPACITY) {                            // a larger loop keyframe: its size is known now
      pairs.resize((size_t)n * 2);
      st = ssx_kfdb_match_features(db_, (int64_t)loop_key_frame_id, (int32_t)current_class_ids.size(), current_descriptors.data(),
                                   current_class_ids.data(), n, pairs.data(), &n, &md);
    }
    ctx_.check(st);
    if (min_distance) *min_distance = md;
    std::set<std::pair<int, int>> out;
    for (int32_t i = 0; i < n; ++i) out.emplace_hint(out.end(), pairs[2 * i], pairs[2 * i + 1]);
    return out;
  }

  // What one pass of LoopClosingThread's loop body decides (loopclosing.cpp:44-66) up to the "fewer than 10 pairs" verdict
  struct KeyframeStep {
    ssx_kfdb_step_result result;                             // counts, DetectLoop's verdict, loop_kf_id, score, min_distance
    std::set<std::pair<int, int>> set_valid_feature_matches; // MatchFeatures' set; empty when no loop was detected
  };

  // ProcessNewKeyframe() (:596-634) + DetectLoop() when key_frame_database_.size() > min_db_size (:48) + MatchFeatures(), one call.  image =
  // current_keyframe_->image_left_, features[i] = features_left_[i]->kp_position_.  Nothing of the keyframe comes back: its
  // pyramid_key_points_, ORBDescriptors_ and bow2_vec_ stay on the device as the pending keyframe (Pending() downloads them).
  KeyframeStep ProcessNewKeyframe(const ORBVocabulary& voc, unsigned long key_frame_id, const uint8_t* image, int stride, int rows, int cols,
                                  const ORBextractor& extractor, const std::vector<ssx_keypoint>& features, float loop_threshold_heigher, int pyramid_levels = 8,
                                  int min_db_size = 50, int min_id_gap = 20)
  {
    if (!voc.get()) throw std::invalid_argument("ProcessNewKeyframe: no vocabulary loaded");
    KeyframeStep out{};
    std::vector<int32_t> pairs(2 * std::max<size_t>(4096, features.size() * (size_t)pyramid_levels));
    auto call = [&]() {
      return ssx_kfdb_process_keyframe(db_, voc.get(), (int64_t)key_frame_id, image, stride, rows, cols, &extractor.params(), (int32_t)features.size(),
                                       features.data(), pyramid_levels, min_db_size, min_id_gap, loop_threshold_heigher, (int32_t)(pairs.size() / 2),
                                       pairs.data(), &out.result);
    };
    ssx_status st = call();
    if (st == SSX_ERR_CAPACITY) {                            // a larger loop keyframe: the count is known now
      pairs.resize((size_t)out.result.n_pairs * 2);
      st = call();
    }
    ctx_.check(st);
    for (int32_t i = 0; i < out.result.n_pairs; ++i) out.set_valid_feature_matches.emplace_hint(out.set_valid_feature_matches.end(), pairs[2 * i], pairs[2 * i + 1]);
    return out;
  }

  // Relocalisation (the reference has a TODO at frontend.cpp:62-66): the stored keyframes a frame that lost tracking resembles, best first,
  // and MatchFeatures against each of them, in ONE call (ssx_kfdb_relocalize_query).  features[i] = the frame's keypoints, as for
  // ProcessNewKeyframe.  Candidates: float score > 0, >= threshold and >= ratio * the best, at most max_candidates.  The database and its
  // pending keyframe are only read.
  struct RelocCandidate {
    unsigned long key_frame_id;
    float score;
    bool has_descriptors;
    int min_distance;
    std::set<std::pair<int, int>> set_valid_feature_matches;   // (feature of the frame, feature of the keyframe)
  };
  std::vector<RelocCandidate> RelocalizeQuery(const ORBVocabulary& voc, const uint8_t* image, int stride, int rows, int cols, const ORBextractor& extractor,
                                              const std::vector<ssx_keypoint>& features, int max_candidates, float threshold, float ratio = 0.75f,
                                              int pyramid_levels = 8, ssx_reloc_query_result* result = nullptr)
  {
    if (!voc.get()) throw std::invalid_argument("RelocalizeQuery: no vocabulary loaded");
    const size_t K = (size_t)std::max(max_candidates, 1);
    size_t cap = std::max<size_t>(4096, features.size() * (size_t)std::max(pyramid_levels, 1));
    std::vector<int32_t> pairs(2 * K * cap);
    ssx_reloc_query_result res{};
    auto call = [&]() {
      return ssx_kfdb_relocalize_query(db_, voc.get(), image, stride, rows, cols, &extractor.params(), (int32_t)features.size(), features.data(), pyramid_levels,
                                       max_candidates, threshold, ratio, (int32_t)cap, pairs.data(), &res);
    };
    ssx_status st = call();
    if (st == SSX_ERR_CAPACITY) {                            // a larger stored keyframe: the counts are known now
      for (int32_t c = 0; c < res.n_candidates; ++c) cap = std::max(cap, (size_t)res.cand[c].n_pairs);
      pairs.assign(2 * K * cap, 0);
      st = call();
    }
    ctx_.check(st);
    if (result) *result = res;
    std::vector<RelocCandidate> out((size_t)res.n_candidates);
    for (int32_t c = 0; c < res.n_candidates; ++c) {
      const ssx_reloc_candidate& q = res.cand[c];
      out[(size_t)c].key_frame_id = (unsigned long)q.kf_id; out[(size_t)c].score = q.score; out[(size_t)c].has_descriptors = q.no_descriptors == 0;
      out[(size_t)c].min_distance = q.min_distance;
      const int32_t* p = pairs.data() + 2 * (size_t)c * cap;
      auto& set = out[(size_t)c].set_valid_feature_matches;
      for (int32_t i = 0; i < q.n_pairs; ++i) set.emplace_hint(set.end(), p[2 * i], p[2 * i + 1]);
    }
    return out;
  }

  // The second step of relocalisation (ssx_kfdb_guided_search; the rule: tools/guided_model.py): map points projected into the frame
  // with the pose just found, T_cw12 = [R|t] row-major, and matched in a window round each projection against the frame's features that
  // are not `taken` (empty: none is).  Point p's descriptors are the stored descriptors of keyframe point_kf[p] with class id
  // point_cls[p]; a keyframe that is not stored (yet) gives SSX_GUIDED_NO_DESCRIPTOR and no error.  The database is only read.
  struct GuidedResult {
    std::vector<int32_t> feature, d1, d2, status;            // per point: the frame's feature (-1 unless SSX_GUIDED_MATCHED), distances, ssx_guided_status
    std::vector<double> uv;                                  // per point: its projection
    int n_matched = 0;
  };
  GuidedResult GuidedSearch(const uint8_t* image, int stride, int rows, int cols, const ORBextractor& extractor, const std::vector<ssx_keypoint>& features,
                            const std::vector<uint8_t>& taken, const double K4[4], const double T_cw12[12], const std::vector<int64_t>& point_kf,
                            const std::vector<int32_t>& point_cls, const std::vector<double>& xyz, double radius, int max_distance, int ratio_pct,
                            int pyramid_levels = 8)
  {
    const size_t P = point_kf.size();
    if (point_cls.size() != P || xyz.size() != 3 * P) throw std::invalid_argument("GuidedSearch: one keyframe, one class id and one position per point");
    if (!taken.empty() && taken.size() != features.size()) throw std::invalid_argument("GuidedSearch: one taken flag per feature");
    GuidedResult out;
    out.feature.assign(P, -1); out.d1.assign(P, -1); out.d2.assign(P, -1); out.status.assign(P, 0); out.uv.assign(2 * P, 0.0);
    int32_t n = 0;
    ctx_.check(ssx_kfdb_guided_search(db_, image, stride, rows, cols, &extractor.params(), (int32_t)features.size(), features.data(), pyramid_levels,
                                      taken.empty() ? nullptr : taken.data(), K4, T_cw12, (int32_t)P, point_kf.data(), point_cls.data(), xyz.data(), radius,
                                      max_distance, ratio_pct, out.feature.data(), out.d1.data(), out.d2.data(), out.status.data(), out.uv.data(), &n));
    out.n_matched = n;
    return out;
  }

  // AddToKeyframeDatabase() (:646-649) for the keyframe ProcessNewKeyframe left on the device: no byte crosses PCIe
  void AddToKeyframeDatabase() { ctx_.check(ssx_kfdb_add_pending(db_)); }

  // current_keyframe_->pyramid_key_points_ / ORBDescriptors_ (n x 32) / bow2_vec_ of the pending keyframe, for a caller that keeps them
  void Pending(std::vector<ssx_keypoint>& pyramid_key_points, std::vector<uint8_t>& descriptors, BowVector& bow)
  {
    int32_t n = 0, nb = 0;
    ctx_.check(ssx_kfdb_pending(db_, nullptr, 0, nullptr, nullptr, nullptr, &n, 0, nullptr, nullptr, &nb));
    pyramid_key_points.resize((size_t)n); descriptors.resize((size_t)n * 32); bow.ids.resize((size_t)nb); bow.values.resize((size_t)nb);
    ctx_.check(ssx_kfdb_pending(db_, nullptr, n, pyramid_key_points.data(), descriptors.data(), nullptr, nullptr, nb, bow.ids.data(), bow.values.data(), nullptr));
  }

  int size() const
  {
    int32_t n = 0;
    ssx_kfdb_size(db_, &n, nullptr, nullptr);
    return n;
  }
  ssx_kf_database* get() const { return db_; }
  Context& context() const { return ctx_; }

 private:
  Context& ctx_;
  ssx_kf_database* db_ = nullptr;
};

// One keyframe of each of several streams: KeyframeDatabase::ProcessNewKeyframe for every entry in ONE call (ssx_kfdb_process_keyframe_batch:
// one launch chain and one synchronisation for all of them, two when a loop was found).  The databases and the vocabulary belong to one
// Context, the images share rows, cols and stride.  add_to_database_first: AddToKeyframeDatabase() of the keyframe the database's last
// step left pending, inside the same call.  Per entry the bytes of the single call.
struct KeyframeStepRequest {
  KeyframeDatabase* database;
  unsigned long key_frame_id;
  const uint8_t* image;
  const std::vector<ssx_keypoint>* features;
  bool add_to_database_first;
};
inline std::vector<KeyframeDatabase::KeyframeStep> ProcessNewKeyframes(const ORBVocabulary& voc, const KeyframeStepRequest* requests, size_t n, int stride, int rows,
                                                                       int cols, const ORBextractor& extractor, float loop_threshold_heigher, int pyramid_levels = 8,
                                                                       int min_db_size = 50, int min_id_gap = 20)
{
  if (!voc.get()) throw std::invalid_argument("ProcessNewKeyframes: no vocabulary loaded");
  std::vector<KeyframeDatabase::KeyframeStep> out(n);
  if (n == 0) return out;
  std::vector<std::vector<int32_t>> pairs(n);
  std::vector<int32_t> status(n, SSX_OK);
  std::vector<ssx_kfdb_step_job> jobs(n);
  for (size_t j = 0; j < n; ++j) {
    const KeyframeStepRequest& q = requests[j];
    if (!q.database || !q.features) throw std::invalid_argument("ProcessNewKeyframes: a request without database or features");
    pairs[j].resize(2 * std::max<size_t>(4096, q.features->size() * (size_t)pyramid_levels));
    jobs[j] = ssx_kfdb_step_job{q.database->get(), (int64_t)q.key_frame_id, q.image, stride, (int32_t)q.features->size(), q.features->data(),
                                q.add_to_database_first ? 1 : 0, (int32_t)(pairs[j].size() / 2), pairs[j].data(), &out[j].result, &status[j]};
  }
  Context& ctx = requests[0].database->context();
  ssx_status st = ssx_kfdb_process_keyframe_batch(voc.get(), (int32_t)n, jobs.data(), rows, cols, &extractor.params(), pyramid_levels, min_db_size, min_id_gap,
                                                  loop_threshold_heigher, 0);
  for (size_t j = 0; j < n && st == SSX_ERR_CAPACITY; ++j) {
    if (status[j] != SSX_ERR_CAPACITY) continue;             // a larger loop keyframe: the count is known now, that step once more (its commit is done)
    pairs[j].resize((size_t)out[j].result.n_pairs * 2);
    jobs[j].commit_pending = 0; jobs[j].pairs_cap = out[j].result.n_pairs; jobs[j].pairs_out = pairs[j].data();
    const ssx_status again = ssx_kfdb_process_keyframe_batch(voc.get(), 1, &jobs[j], rows, cols, &extractor.params(), pyramid_levels, min_db_size, min_id_gap,
                                                             loop_threshold_heigher, 0);
    if (again != SSX_OK) ctx.check(again);
  }
  for (size_t j = 0; j < n; ++j)
    if (status[j] != SSX_OK) ctx.check((ssx_status)status[j]);
  if (st != SSX_OK && st != SSX_ERR_CAPACITY) ctx.check(st);
  for (size_t j = 0; j < n; ++j)
    for (int32_t i = 0; i < out[j].result.n_pairs; ++i)
      out[j].set_valid_feature_matches.emplace_hint(out[j].set_valid_feature_matches.end(), pairs[j][2 * i], pairs[j][2 * i + 1]);
  return out;
}

// The candidate query of several streams that lost tracking: KeyframeDatabase::RelocalizeQuery for every entry in ONE call
// (ssx_kfdb_relocalize_query_batch: one launch chain and one synchronisation for all of them).  The databases and the vocabulary belong to
// one Context, the images share rows, cols and stride.  add_to_database_first: AddToKeyframeDatabase() of the keyframe the database's last
// step left pending, inside the same call -- that keyframe is a candidate like any stored one.  Per entry the bytes of the single call.
struct RelocalizeRequest {
  KeyframeDatabase* database;
  const uint8_t* image;
  const std::vector<ssx_keypoint>* features;
  bool add_to_database_first;
};
inline std::vector<std::vector<KeyframeDatabase::RelocCandidate>> RelocalizeQueries(const ORBVocabulary& voc, const RelocalizeRequest* requests, size_t n, int stride, int rows,
                                                                                    int cols, const ORBextractor& extractor, int max_candidates, float threshold,
                                                                                    float ratio = 0.75f, int pyramid_levels = 8)
{
  if (!voc.get()) throw std::invalid_argument("RelocalizeQueries: no vocabulary loaded");
  std::vector<std::vector<KeyframeDatabase::RelocCandidate>> out(n);
  if (n == 0) return out;
  const size_t K = (size_t)std::max(max_candidates, 1);
  std::vector<std::vector<int32_t>> pairs(n);
  std::vector<size_t> cap(n);
  std::vector<int32_t> status(n, SSX_OK);
  std::vector<ssx_reloc_query_result> res(n);
  std::vector<ssx_reloc_query_job> jobs(n);
  for (size_t j = 0; j < n; ++j) {
    const RelocalizeRequest& q = requests[j];
    if (!q.database || !q.features) throw std::invalid_argument("RelocalizeQueries: a request without database or features");
    cap[j] = std::max<size_t>(4096, q.features->size() * (size_t)std::max(pyramid_levels, 1));
    pairs[j].resize(2 * K * cap[j]);
    jobs[j] = ssx_reloc_query_job{q.database->get(), q.image, stride, (int32_t)q.features->size(), q.features->data(), q.add_to_database_first ? 1 : 0,
                                  (int32_t)cap[j], pairs[j].data(), &res[j], &status[j]};
  }
  Context& ctx = requests[0].database->context();
  ssx_status st = ssx_kfdb_relocalize_query_batch(voc.get(), (int32_t)n, jobs.data(), rows, cols, &extractor.params(), pyramid_levels, max_candidates, threshold, ratio, 0);
  for (size_t j = 0; j < n && st == SSX_ERR_CAPACITY; ++j) {
    if (status[j] != SSX_ERR_CAPACITY) continue;             // a larger stored keyframe: the counts are known now, that query once more (its commit is done)
    for (int32_t c = 0; c < res[j].n_candidates; ++c) cap[j] = std::max(cap[j], (size_t)res[j].cand[c].n_pairs);
    pairs[j].assign(2 * K * cap[j], 0);
    jobs[j].commit_pending = 0; jobs[j].pairs_cap = (int32_t)cap[j]; jobs[j].pairs_out = pairs[j].data();
    const ssx_status again = ssx_kfdb_relocalize_query_batch(voc.get(), 1, &jobs[j], rows, cols, &extractor.params(), pyramid_levels, max_candidates, threshold, ratio, 0);
    if (again != SSX_OK) ctx.check(again);
  }
  for (size_t j = 0; j < n; ++j)
    if (status[j] != SSX_OK) ctx.check((ssx_status)status[j]);
  if (st != SSX_OK && st != SSX_ERR_CAPACITY) ctx.check(st);
  for (size_t j = 0; j < n; ++j) {
    out[j].resize((size_t)res[j].n_candidates);
    for (int32_t c = 0; c < res[j].n_candidates; ++c) {
      const ssx_reloc_candidate& q = res[j].cand[c];
      KeyframeDatabase::RelocCandidate& o = out[j][(size_t)c];
      o.key_frame_id = (unsigned long)q.kf_id; o.score = q.score; o.has_descriptors = q.no_descriptors == 0; o.min_distance = q.min_distance;
      const int32_t* p = pairs[j].data() + 2 * (size_t)c * cap[j];
      for (int32_t i = 0; i < q.n_pairs; ++i) o.set_valid_feature_matches.emplace_hint(o.set_valid_feature_matches.end(), p[2 * i], p[2 * i + 1]);
    }
  }
  return out;
}

// The pose of several candidates in ONE call (ssx_pnp_pose_batch): per job solvePnPRansac under the contract of ssx_pnp_ransac (100
// iterations, 5.991 px as the reference passes them) and, where it found a pose, OptimizeCurrentPose over all pairs from it.  xyz / uv /
// inlier_out of every job are the caller's arrays; the results are written into the jobs.
inline void PnpPoseBatch(Context& ctx, const double K4[4], std::vector<ssx_pnp_pose_job>& jobs, int iterations = 100, double reproj_px = 5.991,
                         double chi2_th = 5.991, double huber_delta = 1.0)
{
  ctx.check(ssx_pnp_pose_batch(ctx.get(), K4, (int32_t)jobs.size(), jobs.data(), iterations, reproj_px, chi2_th, huber_delta));
}

// What LoopClosing::ComputeCorrectPose reads of one entry of set_valid_feature_matches_: the pair itself, the position of
// loop_keyframe_->features_left_[loop_feature_id]->map_point_ (has_map_point = false when the weak_ptr has expired) and
// current_keyframe_->features_left_[current_feature_id]->kp_position_.pt
struct LoopMatch {
  int current_feature_id, loop_feature_id;
  bool has_map_point;
  double map_point[3];
  float pt_x, pt_y;
};

// bool LoopClosing::ComputeCorrectPose() (loopclosing.cpp:147-243) with the OptimizeCurrentPose it calls: solvePnPRansac(100 iterations,
// 5.991 px) under the contract of ssx_pnp_ransac, then g2o over all pairs.  The members the reference writes come back as fields:
struct CorrectPoseResult {
  bool ok = false;                                     // the return value
  ssx_loop_verdict verdict = SSX_LOOP_FEW_MAP_POINTS;  // why not
  std::set<std::pair<int, int>> set_valid_feature_matches;   // after the two erasures (:172, :338-344)
  double corrected_current_pose[7] = {0, 0, 0, 1, 0, 0, 0};
  bool need_correct_loop_pose = false;
  double error = 0.0;                                  // the "Loop Error" the reference logs
  double relative_pose_to_loop_KF[7] = {0, 0, 0, 1, 0, 0, 0};
  int cnt_inliner = 0;
};
inline CorrectPoseResult ComputeCorrectPose(Context& ctx, const std::vector<LoopMatch>& matches, const double current_pose[7], const double loop_pose[7],
                                            const double K4[4], int iterations = 100, uint32_t seed = 0)
{
  const size_t n = matches.size();
  std::vector<double> xyz(3 * n), uv(2 * n);
  std::vector<uint8_t> has(n), kept(n);
  for (size_t i = 0; i < n; ++i) {
    has[i] = matches[i].has_map_point ? 1 : 0;
    for (int k = 0; k < 3; ++k) xyz[3 * i + k] = matches[i].has_map_point ? matches[i].map_point[k] : 0.0;
    uv[2 * i] = matches[i].pt_x; uv[2 * i + 1] = matches[i].pt_y;
  }
  ssx_loop_pose_result r;
  ctx.check(ssx_loop_compute_pose(ctx.get(), (int32_t)n, xyz.data(), has.data(), uv.data(), current_pose, loop_pose, K4, iterations, seed, kept.data(), &r));
  CorrectPoseResult out;
  out.verdict = (ssx_loop_verdict)r.verdict;
  out.ok = r.verdict == SSX_LOOP_OK;
  for (size_t i = 0; i < n; ++i)
    if (kept[i]) out.set_valid_feature_matches.emplace(matches[i].current_feature_id, matches[i].loop_feature_id);
  std::copy(r.corrected_pose, r.corrected_pose + 7, out.corrected_current_pose);
  std::copy(r.relative_to_loop, r.relative_to_loop + 7, out.relative_pose_to_loop_KF);
  out.need_correct_loop_pose = r.need_correct != 0;
  out.error = r.error;
  out.cnt_inliner = r.n_inliers;
  return out;
}

// void LoopClosing::LoopCorrect() (loopclosing.cpp:353-594) without its pointer-level map fusion (:427-453, which moves no number):
// CorrectActivateKeyframeAndMappoint, PoseGraphOptimization and the re-anchoring of every map point, over ssx_loop_correct.
// The caller gathers indices for the reference's pointers: a row per keyframe of Map::GetAllKeyFrames() and a row per map point of
// Map::GetAllMapPoints().  poses and points are corrected in place; the caller writes them back with SetPose / SetPosition.
struct LoopCorrectInput {
  std::vector<double> poses;            // 7 per keyframe: getPose().data()
  std::vector<uint8_t> kf_active;       // Map::GetActiveKeyFrames().count(id)
  int cur_kf = -1, loop_kf = -1;        // rows of current_keyframe_, loop_keyframe_
  int initial_kf = -1;                  // row of key_frame_id_ == 0 (:483), -1 when it is not in the map
  int keep_kf = -1;                     // row of frontend_->getReferenceKF() (:568), -1 when it is not in the map
  double corrected_current_pose[7] = {0, 0, 0, 1, 0, 0, 0};
  std::vector<int32_t> edge_i, edge_j;  // as for ssx_pose_graph_opt (:492-529)
  std::vector<double> edge_meas;        // 7 per edge
  std::vector<double> points;           // 3 per map point: getPosition()
  std::vector<int32_t> point_anchor;    // row of GetActiveObservations().front()'s keyframe for an active point (:408), of
                                        // GetObservations().front()'s otherwise (:554); -1 when that keyframe has no row (:556-561)
  std::vector<uint8_t> point_active;    // Map::GetActiveMapPoints().count(id)
};
inline ssx_loop_correct_result LoopCorrect(Context& ctx, LoopCorrectInput& in, int iterations = 20)
{
  const size_t n = in.kf_active.size(), e = in.edge_i.size(), m = in.point_anchor.size();
  if (in.poses.size() != 7 * n || in.edge_j.size() != e || in.edge_meas.size() != 7 * e || in.points.size() != 3 * m || in.point_active.size() != m)
    throw std::invalid_argument("LoopCorrect: array sizes disagree");
  ssx_loop_correct_problem p{};
  p.n_keyframes = (int32_t)n; p.n_edges = (int32_t)e; p.n_points = (int32_t)m;
  p.cur_kf = in.cur_kf; p.loop_kf = in.loop_kf; p.initial_kf = in.initial_kf; p.keep_kf = in.keep_kf;
  p.poses = in.poses.data(); p.kf_active = in.kf_active.data(); p.corrected_pose = in.corrected_current_pose;
  p.edge_i = in.edge_i.data(); p.edge_j = in.edge_j.data(); p.edge_meas = in.edge_meas.data();
  p.points = in.points.data(); p.point_anchor = in.point_anchor.data(); p.point_active = in.point_active.data();
  ssx_loop_correct_result r;
  ctx.check(ssx_loop_correct(ctx.get(), &p, iterations, &r));
  return r;
}

// CorrectActivateKeyframeAndMappoint (loopclosing.cpp:378-453) for the backend's resident window, over ssx_ba_window_loop_correct:
// after LoopCorrect has corrected the map, the window's keyframes and landmarks get the same bits where they lie.  fused_map_point_ids:
// the ids of the current keyframe's map points that :439-448 merged into a loop map point (Map::RemoveMapPoint): they leave the window;
// the loop map points come back through an ordinary push with new_fixed = 1.  poses / points / anchor_keyframe_ids receive the
// corrected window in export order when given.
inline ssx_ba_window_loop_result CorrectActiveWindow(ssx_ba_window* win, int64_t current_keyframe_id, const double corrected_current_pose[7],
                                                     const std::vector<int64_t>& fused_map_point_ids = {}, std::vector<double>* poses = nullptr,
                                                     std::vector<double>* points = nullptr, std::vector<int64_t>* anchor_keyframe_ids = nullptr)
{
  int32_t n_kf = 0, n_lm = 0;
  if (ssx_ba_window_size(win, &n_kf, &n_lm, nullptr) != SSX_OK) throw std::invalid_argument("CorrectActiveWindow: no window");
  ssx_ba_window_loop_result r{};
  if (poses) { poses->assign(7 * (size_t)n_kf, 0.0); r.poses_out = poses->data(); }
  if (points) { points->assign(3 * (size_t)n_lm, 0.0); r.points_out = points->data(); }
  if (anchor_keyframe_ids) { anchor_keyframe_ids->assign((size_t)n_lm, -1); r.anchor_kf_out = anchor_keyframe_ids->data(); }
  const ssx_status st = ssx_ba_window_loop_correct(win, current_keyframe_id, corrected_current_pose, (int32_t)fused_map_point_ids.size(),
                                                   fused_map_point_ids.empty() ? nullptr : fused_map_point_ids.data(), &r);
  if (st != SSX_OK) throw std::runtime_error("ssx_ba_window_loop_correct failed with status " + std::to_string((int)st));
  return r;
}

// int LoopClosing::OptimizeCurrentPose() (loopclosing.cpp:245-351) on its own: every match must have its map point.
// corrected_current_pose is refined in place, the matches that end as outliers are erased; returns what is left (cnt_inliner).
inline int OptimizeCurrentPose(Context& ctx, std::vector<LoopMatch>& matches, double corrected_current_pose[7], const double K4[4])
{
  const size_t n = matches.size();
  std::vector<double> xyz(3 * n), uv(2 * n);
  std::vector<uint8_t> in(n);
  for (size_t i = 0; i < n; ++i) {
    if (!matches[i].has_map_point) throw std::invalid_argument("OptimizeCurrentPose: a match without a map point");
    for (int k = 0; k < 3; ++k) xyz[3 * i + k] = matches[i].map_point[k];
    uv[2 * i] = matches[i].pt_x; uv[2 * i + 1] = matches[i].pt_y;
  }
  int32_t cnt = 0;
  ctx.check(ssx_loop_pose_opt(ctx.get(), corrected_current_pose, K4, (int32_t)n, xyz.data(), uv.data(), 5.991, 1.0, in.data(), &cnt));
  size_t w = 0;
  for (size_t i = 0; i < n; ++i)
    if (in[i]) matches[w++] = matches[i];
  matches.resize(w);
  return cnt;
}

}  // namespace ssx
