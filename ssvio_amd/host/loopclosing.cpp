// ssvio_amd/host/loopclosing.cpp -- see loopclosing.hpp
#include "loopclosing.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
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
  // relocalisation (the reference has a TODO at frontend.cpp:62-66): no constant of its own but the share of the best score
  reloc_open_ = cfg.Get<int>("Relocalization.Open") != 0;
  reloc_candidates_ = cfg.Has("Relocalization.Candidates") ? cfg.Get<int>("Relocalization.Candidates") : 4;
  reloc_threshold_ = cfg.Has("Relocalization.Threshold") ? cfg.Get<float>("Relocalization.Threshold") : threshold_;
  reloc_ratio_ = cfg.Has("Relocalization.Score.Ratio") ? cfg.Get<float>("Relocalization.Score.Ratio") : 0.75f;
  // the bar: the reference's own boundary between LOST and TRACKING_BAD (frontend.cpp:99-110) unless the settings name another
  reloc_min_inliers_ = cfg.Has("Relocalization.Min.Inliers") ? cfg.Get<int>("Relocalization.Min.Inliers") : cfg.Get<int>("numFeatures.trackingBad");
  if (reloc_open_ && (reloc_candidates_ < 1 || reloc_candidates_ > SSX_RELOC_MAX_CANDIDATES || !(reloc_ratio_ >= 0.f && reloc_ratio_ <= 1.f) || !(reloc_threshold_ >= 0.f)))
    throw std::runtime_error("LoopClosing: Relocalization.Candidates must lie in [1, " + std::to_string(SSX_RELOC_MAX_CANDIDATES) +
                             "], Relocalization.Score.Ratio in [0, 1], and Relocalization.Threshold must not be negative");
  // the guided search behind an accepted candidate (tools/guided_model.py): off unless its key is set
  guided_open_ = cfg.Get<int>("Relocalization.Guided.Open") != 0;
  if (cfg.Has("Relocalization.Guided.Neighbours")) guided_neighbours_ = cfg.Get<int>("Relocalization.Guided.Neighbours");
  if (cfg.Has("Relocalization.Guided.Radius")) guided_.radius = cfg.Get<double>("Relocalization.Guided.Radius");
  if (cfg.Has("Relocalization.Guided.Max.Distance")) guided_.max_distance = cfg.Get<int>("Relocalization.Guided.Max.Distance");
  if (cfg.Has("Relocalization.Guided.Ratio")) guided_.ratio_pct = cfg.Get<int>("Relocalization.Guided.Ratio");
  if (guided_open_ && (guided_neighbours_ < 0 || !std::isfinite(guided_.radius) || guided_.radius < 0.0 || guided_.max_distance < 0 || guided_.max_distance > 256 ||
                       guided_.ratio_pct < 0 || guided_.ratio_pct > 100))
    throw std::runtime_error("LoopClosing: Relocalization.Guided.Neighbours and Relocalization.Guided.Radius must not be negative, "
                             "Relocalization.Guided.Max.Distance must lie in [0, 256] and Relocalization.Guided.Ratio in [0, 100]");
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
  {
    std::lock_guard<std::mutex> compute_lock(compute_mutex_);
    compute_->ProcessKeyframe((int64_t)kf->key_frame_id, *img, feats, orb_, pyramid_levels_, min_db_size_, min_id_gap_, threshold_, step, pairs);
  }
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
    {
      std::lock_guard<std::mutex> compute_lock(compute_mutex_);
      compute_->ComputePose((int)n, xyz.data(), has.data(), uv.data(), T_cur.data(), T_loop.data(), K4, kept.data(), pose);
    }
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
    std::lock_guard<std::mutex> compute_lock(compute_mutex_);
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
  {
    std::lock_guard<std::mutex> compute_lock(compute_mutex_);      // (behind the map mutex: the order everywhere)
    compute_->LoopCorrect(prob, res);
  }
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

// The second step behind an accepted candidate (tools/guided_model.py: gather_points, search_by_projection, refine_accept), under the
// map mutex Relocalize's caller holds.  Gathered: the accepted keyframe, then its guided_neighbours_ neighbours before and after it in
// the map's id order by increasing distance, the lower id first; of each, in feature order, every feature whose map point is alive, no
// outlier, not matched by the first pass and not gathered yet, as (position, that keyframe's id, the feature's index = the class id its
// descriptors were stored under).  One GuidedSearch with the first pass's pose, the first pass's features taken; one RefinePose from
// that pose over the first pass's surviving pairs followed by the new ones; the result replaces the first iff it has a pose and no
// fewer inliers.
void LoopClosing::GuidedStep(const Image& img, const std::vector<ssx_keypoint>& features, const double* K4, RelocResult& out, RelocRecord& rec)
{
  std::vector<unsigned long> ids;
  ids.reserve(map_->GetAllKeyFrames().size());
  for (const auto& kv : map_->GetAllKeyFrames()) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());
  const long at = (long)(std::lower_bound(ids.begin(), ids.end(), (unsigned long)out.kf_id) - ids.begin());
  std::vector<long> order{at};
  for (long step = 1; step <= (long)guided_neighbours_; ++step)
    for (long i : {at - step, at + step})
      if (i >= 0 && i < (long)ids.size()) order.push_back(i);
  std::unordered_map<long, int> seen;
  std::vector<uint8_t> taken(features.size(), 0);
  for (const auto& m : out.matches) { seen[m.second] = 1; taken.at((size_t)m.first) = 1; }
  std::vector<int64_t> point_kf; std::vector<int32_t> point_cls; std::vector<double> xyz; std::vector<long> point_mp;
  for (long i : order) {
    const KeyFramePtr& kf = map_->GetAllKeyFrames().at(ids[(size_t)i]);
    for (size_t f = 0; f < kf->features_left.size(); ++f) {
      MapPointPtr mp = map_->Lock(kf->features_left[f]);
      if (!mp || mp->is_outlier || seen.count((long)mp->id)) continue;
      seen[(long)mp->id] = 1;
      point_kf.push_back((int64_t)kf->key_frame_id); point_cls.push_back((int32_t)f); point_mp.push_back((long)mp->id);
      xyz.insert(xyz.end(), mp->position, mp->position + 3);
    }
  }
  // the model and the kernel share every f64 operation from the matrix on: the 7-vector is converted here
  double T12[12], R[9];
  ssx::quat_to_R(out.T_cw.d, R);
  for (int r = 0; r < 3; ++r) { T12[4 * r] = R[3 * r]; T12[4 * r + 1] = R[3 * r + 1]; T12[4 * r + 2] = R[3 * r + 2]; T12[4 * r + 3] = out.T_cw.d[4 + r]; }
  // the refinement's pairs: the first pass's survivors, then the new ones
  std::vector<double> r_xyz, r_uv; std::vector<std::pair<int32_t, long>> r_pair;
  for (const auto& m : out.matches) {
    MapPointPtr mp = map_->Lock(m.second);
    if (!mp) throw std::logic_error("LoopClosing: a map point of the first pass has left the map under the map mutex");
    r_xyz.insert(r_xyz.end(), mp->position, mp->position + 3);
    r_uv.push_back(features[(size_t)m.first].x); r_uv.push_back(features[(size_t)m.first].y);
    r_pair.push_back(m);
  }
  LoopCompute::GuidedMatches g;
  SE3 pose = out.T_cw;
  std::vector<uint8_t> inlier;
  int n_after = 0, found = 0;
  {
    std::lock_guard<std::mutex> compute_lock(compute_mutex_);
    compute_->GuidedSearch(img, features, orb_, pyramid_levels_, taken, K4, T12, point_kf, point_cls, xyz, guided_, g);
    for (size_t p = 0; p < point_kf.size(); ++p) {
      if (g.status.at(p) != SSX_GUIDED_MATCHED) continue;
      const int32_t f = g.feat.at(p);
      r_xyz.insert(r_xyz.end(), xyz.begin() + 3 * (long)p, xyz.begin() + 3 * (long)p + 3);
      r_uv.push_back(features.at((size_t)f).x); r_uv.push_back(features[(size_t)f].y);
      r_pair.emplace_back(f, point_mp[p]);
    }
    inlier.assign(r_pair.size(), 0);
    compute_->RefinePose(K4, (int)r_pair.size(), r_xyz.data(), r_uv.data(), pose.d, inlier.data(), &n_after, &found);
  }
  rec.guided_points = (int)point_kf.size(); rec.guided_matches = g.n_matched; rec.guided_inliers = found ? n_after : -1;
  out.guided = true; out.guided_points = rec.guided_points; out.guided_matches = rec.guided_matches; out.guided_inliers = rec.guided_inliers;
  out.first_inliers = out.inliers; out.first_matches = (int)out.matches.size();
  if (!found || n_after < out.inliers) return;               // refine_accept: the pose, the inliers and the matches of the first result stand untouched
  out.guided_accepted = true;
  out.T_cw = pose; out.inliers = n_after;
  out.matches.clear();
  std::unordered_map<long, int> taken_mp;
  std::unordered_map<int32_t, int> taken_feat;
  for (size_t i = 0; i < r_pair.size(); ++i) {                // one map point per feature, one feature per map point, first come
    if (!inlier[i] || taken_mp.count(r_pair[i].second) || taken_feat.count(r_pair[i].first)) continue;
    taken_mp[r_pair[i].second] = 1; taken_feat[r_pair[i].first] = 1;
    out.matches.push_back(r_pair[i]);
  }
}

// The caller (the front-end, in state LOST) holds Map::update_mutex; the compute lock is taken behind it.  One query, one gather per
// candidate as Step's for ComputePose, one pose batch, one verdict.
bool LoopClosing::Relocalize(unsigned long frame_id, const Image& img, const std::vector<ssx_keypoint>& features, const double* K4, RelocResult& out)
{
  out = RelocResult{};
  RelocRecord rec;
  rec.frame_id = frame_id;
  struct Job { int rank; KeyFramePtr kf; std::vector<double> xyz, uv; std::vector<int32_t> feat; std::vector<long> mp; std::vector<uint8_t> inlier; };
  std::vector<Job> gathered;
  std::vector<ssx_pnp_pose_job> jobs;
  {
    std::lock_guard<std::mutex> compute_lock(compute_mutex_);
    ssx_reloc_query_result q{};
    std::vector<std::vector<int32_t>> pairs;
    compute_->RelocalizeQuery(img, features, orb_, pyramid_levels_, reloc_candidates_, reloc_threshold_, reloc_ratio_, q, pairs);
    rec.candidates = q.n_candidates;
    for (int c = 0; c < q.n_candidates; ++c) {
      rec.pairs += q.cand[c].n_pairs;
      auto it = map_->GetAllKeyFrames().find((unsigned long)q.cand[c].kf_id);
      if (it == map_->GetAllKeyFrames().end()) throw std::logic_error("LoopClosing: the database named keyframe " + std::to_string(q.cand[c].kf_id) + ", which the map does not hold");
      Job j;
      j.rank = c; j.kf = it->second;
      const std::vector<int32_t>& pr = pairs.at((size_t)c);
      for (size_t i = 0; i + 1 < pr.size(); i += 2) {                  // the live, not condemned map point of the keyframe's feature of every pair
        MapPointPtr mp = map_->Lock(j.kf->features_left.at((size_t)pr[i + 1]));
        if (!mp || mp->is_outlier) continue;
        const ssx_keypoint& kp = features.at((size_t)pr[i]);
        j.xyz.insert(j.xyz.end(), mp->position, mp->position + 3);
        j.uv.push_back(kp.x); j.uv.push_back(kp.y);
        j.feat.push_back(pr[i]); j.mp.push_back((long)mp->id);
      }
      if (j.feat.size() < 10) continue;                                // loopclosing.cpp:193
      j.inlier.assign(j.feat.size(), 0);
      gathered.push_back(std::move(j));
    }
    jobs.resize(gathered.size());
    for (size_t k = 0; k < gathered.size(); ++k) {
      Job& j = gathered[k];
      ssx_pnp_pose_job& p = jobs[k];
      p = ssx_pnp_pose_job{};
      p.M = (int32_t)j.feat.size(); p.xyz = j.xyz.data(); p.uv = j.uv.data(); p.inlier_out = j.inlier.data();
      p.seed = 0u + (uint32_t)j.rank;                                  // ComputePose's seed (0) plus the candidate's rank
    }
    if (!jobs.empty()) compute_->PosesBatch(K4, jobs);
  }
  // the most refined inliers, the lower rank on a tie (the jobs are in rank order), and MORE than the bar (tools/reloc_model.py: accept)
  int best = -1, best_n = reloc_min_inliers_;
  for (size_t k = 0; k < jobs.size(); ++k) {
    if (jobs[k].found) rec.inliers = std::max(rec.inliers, (int)jobs[k].n_inliers);
    if (jobs[k].found && jobs[k].n_inliers > best_n) { best = (int)k; best_n = jobs[k].n_inliers; }
  }
  rec.poses = (int)jobs.size();
  if (best >= 0) {
    const Job& j = gathered[(size_t)best];
    out.ok = true;
    out.kf_id = (long)j.kf->key_frame_id;
    out.T_cw = SE3(jobs[(size_t)best].pose_out);
    out.inliers = jobs[(size_t)best].n_inliers;
    // the surviving pairs: one map point per feature and one feature per map point (a keyframe observes a map point once), first come
    std::unordered_map<long, int> taken_mp;
    std::unordered_map<int32_t, int> taken_feat;
    for (size_t i = 0; i < j.feat.size(); ++i) {
      if (!j.inlier[i] || taken_mp.count(j.mp[i]) || taken_feat.count(j.feat[i])) continue;
      taken_mp[j.mp[i]] = 1; taken_feat[j.feat[i]] = 1;
      out.matches.emplace_back(j.feat[i], j.mp[i]);
    }
    rec.accepted = out.kf_id;
    if (guided_open_) GuidedStep(img, features, K4, out, rec);
  }
  out.candidates = rec.candidates; out.pairs = rec.pairs;
  if (!out.ok) out.inliers = rec.inliers;
  reloc_records_.push_back(rec);
  return out.ok;
}

}  // namespace ssx::host
