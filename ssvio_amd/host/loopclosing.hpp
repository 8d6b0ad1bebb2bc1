// ssvio_amd/host/loopclosing.hpp -- LoopClosing (reference: src/ssvio/loopclosing.cpp:18-70, 147-243, 353-456, 596-669): the thread
// that looks at every keyframe the backend has inserted, finds an earlier keyframe of the same place, computes the pose the current
// keyframe should have, and corrects the map.  Every arithmetic step is a LoopCompute call (compute.hpp); what is restated here is
// the bookkeeping between them:
//   InsertNewKeyFrame   :657-669   a keyframe is dropped while fewer than 6 ids lie between it and the last closed one
//   the loop body       :43-66     ProcessKeyframe (ProcessNewKeyframe + DetectLoop + MatchFeatures, one call); with a loop found and
//                                  >= 10 pairs (:139) ComputePose (:147-243); a confirmed keyframe records its loop edge and is NOT added
//                                  to the database, every other one is (AddPending)
//   LoopCorrect         :353-594   with the backend paused: the whole map marshalled into one ssx_loop_correct_problem, one call, poses
//                                  and points written back, the map fusion of :427-453 (Map::FuseLoopMapPoints), and the same correction
//                                  on the backend's resident window (Backend::LoopCorrectWindow)
// Two modes, in the manner of the backend's:
//   synchronous (default)    InsertNewKeyFrame runs the step inline: in Backend, after the window optimisation of the keyframe, under the
//                            map mutex its caller holds.  Deterministic; what the tests use.
//   Loop.Closing.Async: 1    the reference's layout: a thread of its own takes keyframes from a queue.  It takes Map::update_mutex to
//                            read the map for ComputePose and -- where :380 takes it, held through the write-back of :539 -- for the
//                            whole correction, after the backend has come to rest (RequestPause; the reference polls, and polls the
//                            inverted condition).  A failure of the thread is parked and rethrown by the next InsertNewKeyFrame / WaitIdle,
//                            like Backend::worker_error_.
// Relocalisation settings: Relocalization.Open (absent = 0), Relocalization.Candidates (absent = 4), Relocalization.Threshold (absent =
// Loop.Threshold.Heigher), Relocalization.Score.Ratio (absent = 0.75), Relocalization.Min.Inliers (absent = numFeatures.trackingBad).
// The guided search behind an accepted candidate: Relocalization.Guided.Open (absent = 0), .Neighbours (absent = 2),
// .Radius (absent = 10.0 px), .Max.Distance (absent = 50), .Ratio (absent = 90, per cent).
// Settings: Loop.Threshold.Heigher, Loop.Closig.Keyframe.Database.Min.Size, Pyramid.Level (the reference's keys and spelling),
// Loop.Min.Keyframe.Gap (absent = 20, the constant of :79), Loop.Closing.Async (absent = 0); Loop.Show.Closing.Result is read and ignored.
// The extractor parameters are those of :689-698 (ORBextractor.nNewFeatures).  The 1 / 15 gates of :226 are the library's.
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "compute.hpp"
#include "frontend.hpp"
#include "map.hpp"
#include "setting.hpp"

namespace ssx::host {

class Backend;

class LoopClosing {
 public:
  // one per keyframe the loop step handled, in order (the runner's --loop_log)
  struct Record {
    unsigned long kf_id = 0;
    int db_size = 0;                   // keyframes in the database when the step began
    int found = 0;                     // DetectLoop
    long loop_kf_id = -1;
    float score = 0;
    int pairs = 0;                     // MatchFeatures
    int verdict = -1;                  // ssx_loop_verdict of ComputePose, -1 = not called
    int with_point = 0, inliers = 0;
    double error = 0;
    int need_correct = 0, corrected = 0, fused = 0, same_point_skipped = 0, duplicate_skipped = 0;
    int pg_iterations = 0, active_points_moved = 0, other_points_moved = 0, points_skipped = 0;
  };
  struct Stats {
    long steps = 0, corrections = 0, dropped = 0;
    double t_step = 0, t_correct = 0;  // seconds: the whole step (correction included), the corrections alone
  };

  LoopClosing(const Setting& cfg, std::unique_ptr<LoopCompute> compute, std::shared_ptr<Map> map, const Camera& left);
  ~LoopClosing();
  LoopClosing(const LoopClosing&) = delete;
  LoopClosing& operator=(const LoopClosing&) = delete;

  void SetBackend(Backend* backend) { backend_ = backend; }
  // the id of the front-end's reference keyframe (:568), -1 = none; called with the map mutex held
  void SetReferenceKeyFrame(std::function<long()> f) { reference_kf_ = std::move(f); }

  // called by the backend WITH Map::update_mutex held
  void InsertNewKeyFrame(const KeyFramePtr& kf);

  // Relocalisation (Relocalization.Open: 1): where is a frame that lost tracking?  One candidate query over the whole keyframe database
  // (LoopCompute::RelocalizeQuery), per candidate the live, not condemned map point of the keyframe's feature of every pair (fewer than
  // 10: skipped, :193), ONE pose batch over the rest (LoopCompute::PosesBatch, seed = ComputePose's + the candidate's rank).  Accepted: the
  // most refined inliers, the lower rank on a tie, and more than Relocalization.Min.Inliers (tools/reloc_model.py).  Called by the
  // front-end WITH Map::update_mutex held; the compute lock is taken behind it.
  struct RelocResult {
    bool ok = false;
    long kf_id = -1;                   // the accepted keyframe
    SE3 T_cw;                          // the frame's pose
    std::vector<std::pair<int32_t, long>> matches;   // (feature of the frame, map point) of the pairs that survive the refinement: each feature and each map point once
    int candidates = 0, pairs = 0, inliers = 0;      // of the attempt: candidates named, their pairs in all, the most refined inliers
    // the guided search, when it ran (Relocalization.Guided.Open: 1 and a candidate accepted): what it gathered and matched, the
    // second refinement's inliers (-1: no pose), whether its result replaced the first pass's, and the first pass's own figures
    bool guided = false, guided_accepted = false;
    int guided_points = 0, guided_matches = 0, guided_inliers = 0, first_inliers = 0, first_matches = 0;
  };
  struct RelocRecord {                 // one per attempt, in order (the runner's --loop_log)
    unsigned long frame_id = 0;
    int candidates = 0, pairs = 0, poses = 0, inliers = 0;
    long accepted = -1;
    // the guided search behind an accepted candidate (Relocalization.Guided.Open: 1): map points gathered, points it matched to a
    // feature, inliers of the second refinement (-1: it found no pose)
    int guided_points = 0, guided_matches = 0, guided_inliers = 0;
  };
  bool relocalization() const { return reloc_open_; }
  bool guided() const { return guided_open_; }
  bool Relocalize(unsigned long frame_id, const Image& img, const std::vector<ssx_keypoint>& features, const double* K4, RelocResult& out);
  const std::vector<RelocRecord>& reloc_records() const { return reloc_records_; }   // read with the front-end at rest
  void WaitIdle();                     // asynchronous mode: returns when the queue is empty and the thread idle
  bool async() const { return async_; }
  // valid after WaitIdle (asynchronous mode: the thread appends)
  const std::vector<Record>& records() const { return records_; }
  const Stats& stats() const { return stats_; }

 private:
  void Step(const KeyFramePtr& kf);
  void LoopCorrect(const KeyFramePtr& cur, const KeyFramePtr& loop, const SE3& corrected, const std::vector<int32_t>& pairs, Record& rec);
  void GuidedStep(const Image& img, const std::vector<ssx_keypoint>& features, const double* K4, RelocResult& out, RelocRecord& rec);
  void Worker();
  void RethrowWorkerError();           // queue_mutex_ held

  std::unique_ptr<LoopCompute> compute_;
  std::shared_ptr<Map> map_;
  Backend* backend_ = nullptr;
  std::function<long()> reference_kf_;
  Camera camera_left_;
  ssx_orb_params orb_{};
  int pyramid_levels_ = 0, min_db_size_ = 0, min_id_gap_ = 20;
  float threshold_ = 0;
  int db_size_ = 0;
  bool reloc_open_ = false;
  int reloc_candidates_ = 4, reloc_min_inliers_ = 0;
  float reloc_threshold_ = 0, reloc_ratio_ = 0.75f;
  bool guided_open_ = false;
  int guided_neighbours_ = 2;
  LoopCompute::GuidedParams guided_;
  std::vector<RelocRecord> reloc_records_;
  // compute_ is one context, used by one thread at a time: the loop step (this thread or the loop thread) and Relocalize (the
  // front-end's thread).  Lock order everywhere: Map::update_mutex, then this; nothing waits for the map mutex while holding it.
  std::mutex compute_mutex_;
  std::vector<Record> records_;
  Stats stats_;

  bool async_ = false;
  std::thread worker_;
  std::mutex queue_mutex_;             // the queue, last_closed_id_, busy_, worker_error_
  std::condition_variable queue_cv_, idle_cv_;
  std::deque<KeyFramePtr> queue_;
  long last_closed_id_ = -1;           // last_closed_keyframe_, -1 = none yet
  bool stop_ = false, busy_ = false;
  std::exception_ptr worker_error_;
};

}  // namespace ssx::host
