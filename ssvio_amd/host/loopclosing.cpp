// ssvio_amd/host/loopclosing.cpp -- see loopclosing.hpp
#include "loopclosing.hpp"

#include <chrono>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>

#include "backend.hpp"

namespace ssx::host {

namespace {
struct Timed {
  double& acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit Timed(double& a) : acc(a) {}
  ~Timed() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

LoopClosing::LoopClosing(const Setting& cfg, std::unique_ptr<LoopCompute> compute, std::shared_ptr<Map> map, const Camera& left)
    : compute_(std::move(compute)), map_(std::move(map)), camera_left_(left)
{
  if (!compute_) throw std::invalid_argument("LoopClosing: no LoopCompute");
  // loopclosing.cpp:689-698 GenerateORBextractor, :700-715 LoadParam
  orb_.nfeatures = cfg.Get<int>("ORBextractor.nNewFeatures");
  orb_.scale_factor = cfg.Get<float>("ORBextractor.scaleFactor");
  orb_.nlevels = cfg.Get<int>("ORBextractor.nLevels");
  orb_.ini_th_fast = cfg.Get<int>("ORBextractor.iniThFAST");
  orb_.min_th_fast = cfg.Get<int>("ORBextractor.minThFAST");
  threshold_ = cfg.Get<float>("Loop.Threshold.Heigher");
  pyramid_levels_ = cfg.Get<int>("Pyramid.Level");
  min_db_size_ = cfg.Get<int>("Loop.Closig.Keyframe.Database.Min.Size");
  min_id_gap_ = cfg.Has("Loop.Min.Keyframe.Gap") ? cfg.Get<int>("Loop.Min.Keyframe.Gap") : 20;
  (void)cfg.Get<int>("Loop.Show.Closing.Result");                      // the headless system has nothing to show
  if (pyramid_levels_ < 1) throw std::runtime_error("LoopClosing: Pyramid.Level must be at least 1");
  async_ = cfg.Get<int>("Loop.Closing.Async") != 0;
  if (async_) worker_ = std::thread([this] { Worker(); });
}

LoopClosing::~LoopClosing()
{
  if (worker_.joinable()) {
    {
      std::lock_guard<std::mutex> lk(queue_mutex_);
      stop_ = true;
    }
    queue_cv_.notify_all();
    worker_.join();
  }
}

// loopclosing.cpp:657-669
void LoopClosing::InsertNewKeyFrame(const KeyFramePtr& kf)
{
  {
    std::lock_guard<std::mutex> lk(queue_mutex_);
    RethrowWorkerError();
    if (last_closed_id_ >= 0 && kf->key_frame_id - (unsigned long)last_closed_id_ <= 5) {
      kf->left_image.reset();                                          // never processed: nothing needs its image
      stats_.dropped++;
      return;
    }
    if (async_) queue_.push_back(kf);
  }
  if (async_) {
    queue_cv_.notify_one();
    return;
  }
  Step(kf);
}

void LoopClosing::WaitIdle()
{
  if (!async_) return;
  std::unique_lock<std::mutex> lk(queue_mutex_);
  idle_cv_.wait(lk, [this] { return queue_.empty() && !busy_; });
  RethrowWorkerError();
}

void LoopClosing::RethrowWorkerError()
{
  if (!worker_error_) return;
  std::exception_ptr e = worker_error_;
  worker_error_ = nullptr;
  std::rethrow_exception(e);
}

// loopclosing.cpp:39-70 without the polling sleep, one keyframe at a time
void LoopClosing::Worker()
{
  for (;;) {
    KeyFramePtr kf;
    {
      std::unique_lock<std::mutex> lk(queue_mutex_);
      queue_cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
      if (queue_.empty()) return;                                      // stop requested and nothing left to do
      kf = queue_.front();
      queue_.pop_front();
      busy_ = true;
    }
    std::exception_ptr err;
    try {
      Step(kf);
    } catch (...) {
      err = std::current_exception();
    }
    {
      std::lock_guard<std::mutex> lk(queue_mutex_);
      busy_ = false;
      if (err && !worker_error_) worker_error_ = err;
    }
    idle_cv_.notify_all();
  }
}

// The body of LoopClosingThread's loop (:43-66).  Synchronous mode: the caller holds the map mutex; asynchronous: it is taken here
// wherever the map is read or written.
void LoopClosing::Step(const KeyFramePtr& kf)
{
  Timed tm(stats_.t_step);
  stats_.steps++;
  Record rec;
  rec.kf_id = kf->key_frame_id;
  rec.db_size = db_size_;
  ImagePtr img = kf->left_image;
  if (!img || img->empty()) throw std::logic_error("LoopClosing: keyframe " + std::to_string(kf->key_frame_id) + " carries no left image");
  // :607-619: features_left_[i]->kp_position_ (the library replicates it over the pyramid levels with class_id = i)
  std::vector<ssx_keypoint> feats(kf->features_left.size());
  for (size_t i = 0; i < feats.size(); ++i) feats[i] = ssx_keypoint{kf->features_left[i]->x, kf->features_left[i]->y, 7.f, -1.f, 0.f, 0, (int32_t)i};
  ssx_kfdb_step_result step{};
  std::vector<int32_t> pairs;
  compute_->ProcessKeyframe((int64_t)kf->key_frame_id, *img, feats, orb_, pyramid_levels_, min_db_size_, min_id_gap_, threshold_, step, pairs);
  kf->left_image.reset();                                              // its descriptors are on the device now
  img.reset();
  rec.found = step.found ? 1 : 0;
  rec.pairs = step.found ? step.n_pairs : 0;
  if (step.found) { rec.loop_kf_id = (long)step.loop_kf_id; rec.score = step.score; }

  bool confirmed = false;
  if (step.found && step.n_pairs >= 10) {                              // :139
    const size_t n = (size_t)step.n_pairs;
    std::vector<double> xyz(3 * n, 0.0), uv(2 * n);
    std::vector<uint8_t> has(n, 0), kept(n, 0);
    KeyFramePtr loop_kf;
    SE3 T_cur, T_loop;
    {
      std::unique_lock<std::mutex> map_lock(map_->update_mutex, std::defer_lock);
      if (async_) map_lock.lock();
      auto it = map_->GetAllKeyFrames().find((unsigned long)step.loop_kf_id);
      if (it == map_->GetAllKeyFrames().end()) throw std::logic_error("LoopClosing: the database named keyframe " + std::to_string(step.loop_kf_id) + ", which the map does not hold");
      loop_kf = it->second;
      for (size_t i = 0; i < n; ++i) {                                 // :153-174
        const FeaturePtr& cur_feat = kf->features_left.at((size_t)pairs[2 * i]);
        if (MapPointPtr mp = map_->Lock(loop_kf->features_left.at((size_t)pairs[2 * i + 1]))) {
          has[i] = 1;
          std::memcpy(&xyz[3 * i], mp->position, 3 * sizeof(double));
        }
        uv[2 * i] = cur_feat->x; uv[2 * i + 1] = cur_feat->y;
      }
      T_cur = kf->pose; T_loop = loop_kf->pose;
    }
    const double K4[4] = {camera_left_.fx, camera_left_.fy, camera_left_.cx, camera_left_.cy};
    ssx_loop_pose_result pose{};
    compute_->ComputePose((int)n, xyz.data(), has.data(), uv.data(), T_cur.data(), T_loop.data(), K4, kept.data(), pose);
    rec.verdict = pose.verdict; rec.with_point = pose.n_with_point; rec.inliers = pose.n_inliers;
    std::vector<int32_t> valid;                                        // set_valid_feature_matches_ after :172 and :338-344
    for (size_t i = 0; i < n; ++i)
      if (kept[i]) { valid.push_back(pairs[2 * i]); valid.push_back(pairs[2 * i + 1]); }
    if (pose.verdict == SSX_LOOP_OK) {
      rec.error = pose.error; rec.need_correct = pose.need_correct ? 1 : 0;
      {
        std::unique_lock<std::mutex> map_lock(map_->update_mutex, std::defer_lock);
        if (async_) map_lock.lock();
        kf->loop_key_frame = (long)loop_kf->key_frame_id;              // :236-238
        kf->relative_pose_to_loop_kf = SE3(pose.relative_to_loop);
      }
      {
        std::lock_guard<std::mutex> lk(queue_mutex_);
        last_closed_id_ = (long)kf->key_frame_id;                      // :240
      }
      confirmed = true;
      if (pose.need_correct) LoopCorrect(kf, loop_kf, SE3(pose.corrected_pose), valid, rec);   // :355
    }
  }
  if (!confirmed) {                                                    // :62-65
    compute_->AddPending();
    ++db_size_;
  }
  records_.push_back(rec);
}

// loopclosing.cpp:353-594.  The map mutex is held from :380 to the end of the write-back of :539: the correction is one library call,
// and the front-end must not track against a map that is half corrected.
void LoopClosing::LoopCorrect(const KeyFramePtr& cur, const KeyFramePtr& loop, const SE3& corrected, const std::vector<int32_t>& pairs, Record& rec)
{
  Timed tm(stats_.t_correct);
  // the inline step runs inside the backend, which is at rest by construction; the thread asks it to come to rest (:361-366)
  struct Pause {
    Backend* b;
    explicit Pause(Backend* backend) : b(backend) { if (b) b->RequestPause(); }
    ~Pause() { if (b) b->Resume(); }
  } pause(async_ ? backend_ : nullptr);
  std::unique_lock<std::mutex> map_lock(map_->update_mutex, std::defer_lock);
  if (async_) map_lock.lock();

  const auto& active_kfs = map_->GetActiveKeyFrames();
  const auto& active_mps = map_->GetActiveMapPoints();
  // (asynchronous mode: the window may have slid past the keyframe while it waited in the queue; the library refuses a current
  // keyframe that is not active, as :422-425 sets poses for active keyframes only.  The loop edge stays recorded.)
  if (!active_kfs.count(cur->key_frame_id)) return;

  // (a) the whole map as one ssx_loop_correct_problem: keyframes and map points in ascending id order
  const std::map<unsigned long, KeyFramePtr> kfs(map_->GetAllKeyFrames().begin(), map_->GetAllKeyFrames().end());
  const std::map<unsigned long, MapPointPtr> mps(map_->GetAllMapPoints().begin(), map_->GetAllMapPoints().end());
  std::unordered_map<unsigned long, int32_t> row;
  std::vector<KeyFramePtr> kf_rows;
  std::vector<double> poses, edge_meas, points;
  std::vector<uint8_t> kf_active, point_active;
  std::vector<int32_t> edge_i, edge_j, point_anchor;
  for (auto& kv : kfs) {
    row[kv.first] = (int32_t)kf_rows.size();
    kf_rows.push_back(kv.second);
    poses.insert(poses.end(), kv.second->pose.data(), kv.second->pose.data() + 7);
    kf_active.push_back(active_kfs.count(kv.first) ? 1 : 0);
  }
  auto row_of = [&](long id) { auto it = id < 0 ? row.end() : row.find((unsigned long)id); return it == row.end() ? -1 : it->second; };
  auto add_edge = [&](int32_t i, long to, const SE3& meas) {
    const int32_t j = row_of(to);
    if (j < 0) return;                                                 // (lock() of an expired keyframe: no edge)
    edge_i.push_back(i); edge_j.push_back(j);
    edge_meas.insert(edge_meas.end(), meas.data(), meas.data() + 7);
  };
  for (size_t i = 0; i < kf_rows.size(); ++i) {                        // :495-529: first the last-keyframe edge, then the loop edge
    add_edge((int32_t)i, kf_rows[i]->last_key_frame, kf_rows[i]->relative_pose_to_last_kf);
    add_edge((int32_t)i, kf_rows[i]->loop_key_frame, kf_rows[i]->relative_pose_to_loop_kf);
  }
  std::vector<MapPointPtr> mp_rows;
  for (auto& kv : mps) {
    const MapPointPtr& mp = kv.second;
    const bool active = active_mps.count(kv.first) != 0;
    const auto& obs = active ? mp->active_observations : mp->observations;   // :408 / :554
    mp_rows.push_back(mp);
    points.insert(points.end(), mp->position, mp->position + 3);
    point_active.push_back(active ? 1 : 0);
    point_anchor.push_back(obs.empty() ? -1 : row_of(obs.front()->keyframe));
  }
  ssx_loop_correct_problem prob{};
  prob.n_keyframes = (int32_t)kf_rows.size(); prob.n_edges = (int32_t)edge_i.size(); prob.n_points = (int32_t)mp_rows.size();
  prob.cur_kf = row_of((long)cur->key_frame_id); prob.loop_kf = row_of((long)loop->key_frame_id);
  prob.initial_kf = row_of(0);                                         // :483
  prob.keep_kf = reference_kf_ ? row_of(reference_kf_()) : -1;         // :568
  prob.poses = poses.data(); prob.kf_active = kf_active.data(); prob.corrected_pose = corrected.data();
  prob.edge_i = edge_i.data(); prob.edge_j = edge_j.data(); prob.edge_meas = edge_meas.data();
  prob.points = points.data(); prob.point_anchor = point_anchor.data(); prob.point_active = point_active.data();

  // (b) one call; poses and points back
  ssx_loop_correct_result res{};
  compute_->LoopCorrect(prob, res);
  for (size_t i = 0; i < kf_rows.size(); ++i) kf_rows[i]->pose = SE3(&poses[7 * i]);
  for (size_t j = 0; j < mp_rows.size(); ++j) std::memcpy(mp_rows[j]->position, &points[3 * j], 3 * sizeof(double));

  // (c) :427-453
  const Map::LoopFusion fusion = map_->FuseLoopMapPoints(cur, loop, pairs);

  // (d) the resident window and the backend's mirrors of it
  if (backend_) backend_->LoopCorrectWindow(cur->key_frame_id, corrected, fusion.removed);

  stats_.corrections++;
  rec.corrected = 1;
  rec.fused = (int)fusion.removed.size();
  rec.same_point_skipped = fusion.same_point_skipped;
  rec.duplicate_skipped = fusion.duplicate_skipped;
  rec.pg_iterations = res.pg.n_iters;
  rec.active_points_moved = res.n_active_points_moved;
  rec.other_points_moved = res.n_other_points_moved;
  rec.points_skipped = res.n_points_skipped;
}

}  // namespace ssx::host
