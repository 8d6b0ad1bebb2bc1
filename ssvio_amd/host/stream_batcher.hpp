// ssvio_amd/host/stream_batcher.hpp -- S independent streams (one System each: BASELINE configs[4], "8 concurrent KITTI streams,
// full frontend + backend") sharing ONE GPU through BATCHED compute calls.
//
// A single stream is a chain of small dependent launches (System::RunStep -> TrackLastFrame -> EstimateCurrentPose,
// /root/reference/src/ssvio/frontend.cpp:100-300, system.cpp:46-52): 0.4 - 0.55 ms per frame of which the GPU is busy for a
// fraction; S streams that each issue their own launches (round 4's `--streams`) share the launch path and four hardware queues
// and reach 4.7 k frames/s at S = 8.  Here every stream still runs its own unmodified System on its own thread, but its two
// per-frame compute calls -- the temporal LK (Compute::TrackLK, temporal) and the pose-only LM (Compute::PoseOnly) -- and its
// window optimisations (BaWindow::Solve) do not go to the GPU one by one: the stream files a request and sleeps; a dispatcher
// thread waits until no stream is running host code any more (every live stream is asleep on a request, or busy in a keyframe's
// own calls), gathers the pending requests of one kind and issues them as ONE library call
//     ssx_lk_track_batch / ssx_pose_only_opt_batch / ssx_ba_window_solve_batch        (include/ssx.h)
// whose per-job results are, bit for bit, those of the single calls -- so every stream's trajectory is byte-identical to its
// single-stream run, whatever S and whatever the interleaving (tests/test_host_gpu.py).  The keyframe path of a stream (masked
// detection, stereo LK, triangulation: ssx_orb_detect_boxes_batch / ssx_lk_track_batch / ssx_triangulate_batch) is batched by a
// second dispatcher on contexts of its own, beside the per-frame batches; a stream's images are read by the GPU from the stream's
// pinned buffers (filled by the stream's own thread), nothing is staged inside the batched calls.  Loop closing's keyframe step
// (LoopCompute::ProcessKeyframe) is one more request kind of that dispatcher: the streams of a cohort share one loop context and ONE
// vocabulary, each has its keyframe database there, and their steps go out as ssx_kfdb_process_keyframe_batch; the calls of a
// correction are rare and are made by the dispatcher one at a time.  Relocalisation (Relocalization.Open: 1) is two more kinds there: the
// candidate queries of the streams that lost tracking go out as ONE ssx_kfdb_relocalize_query_batch -- a stream's pending keyframe is
// committed inside it -- and the pose jobs of their candidates are packed into ssx_pnp_pose_batch calls.
//
// Camera.NeedUndistortion: a frame's pair goes through the lenses' stored maps first (Compute::UndistortPair), as one more request kind of the
// per-frame dispatcher: ONE ssx_undistort_plan_apply for the cohort, two jobs per stream, the maps shared by all streams of one rig.
// The raw pairs go up from the pinned arena in one DMA copy and the results come down into the arena buffers the LK calls read.
//
// A cohort may mix image sizes: an LK context holds chains for one size, so the batcher keeps LK contexts per (rows, cols) and a frame
// costs one LK call per size; the streams of one size still share it.
//
// Two pairs of files.  batch_dispatch.{hpp,cpp} is the protocol and knows no library call: the request slots and their states, the
// streams' sleep and wake-up, the ONE dispatcher loop that both dispatcher threads run (each with its kinds in priority order, its
// slots and its rest condition), the per-kind counters, the retry that isolates a faulty request, and the rule for which slot a
// thread files in; tests/host/test_dispatch_units.cpp holds it to its ordering on the CPU, under ThreadSanitizer too.
// stream_batcher.cpp is a table of the request kinds -- each one's per-slot request, what the jobs of a call must share, and its
// library call -- and the three adapters (Compute, BaWindow, LoopCompute) that file them.
//
// Dispatch order: pose-only before LK before undistortion (the later stage first).  Measured with undistortion last: 64 streams, every
// undistortion call carries all 128 jobs (profiles/undistort_plan/time.txt) -- no order can carry more, so no other was tried.  A stream that comes back from a keyframe is half a frame out of phase with the cohort; with
// the pose-only batch served first the cohort arrives at its next LK request while the straggler still waits there, and they merge.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "compute.hpp"

namespace ssx::host {

class StreamBatcher {
 public:
  // cohorts > 1: the streams are dealt to that many independent batchers (stream k -> cohort k mod cohorts), each with its own
  // dispatchers and contexts: one cohort's batched call runs on the GPU while the other cohort's streams run their host code
  StreamBatcher(int device, int streams, int cohorts = 1);
  ~StreamBatcher();
  StreamBatcher(const StreamBatcher&) = delete;
  StreamBatcher& operator=(const StreamBatcher&) = delete;

  // the Compute of stream k (0 <= k < streams); call once per stream, from any thread, before the stream starts.  The stream's
  // thread must call Finish(k) when it has run its last frame (or died): the dispatcher stops waiting for it.
  std::unique_ptr<Compute> MakeCompute(int k);
  void Finish(int k);

  // (calls: the library calls made that did not fail; jobs: the requests in them -- one counter per request kind, batch_dispatch.hpp)
  struct Stats {
    long lk_calls = 0, lk_jobs = 0, po_calls = 0, po_jobs = 0, ba_calls = 0, ba_jobs = 0, kf_calls = 0, kf_jobs = 0;   // kf: detection, stereo LK, triangulation
    double lk_s = 0, po_s = 0, ba_s = 0, kf_s = 0;  // seconds inside the batched library calls
    double wait_s = 0;                               // seconds the per-frame dispatcher waited for the streams' host code
    long loop_calls = 0, loop_jobs = 0;              // loop closing's keyframe step: ssx_kfdb_process_keyframe_batch calls and their jobs
    double loop_s = 0;
    long single_calls = 0;                           // a correction's calls (ComputeCorrectPose, LoopCorrect, the window's), one at a time
    double single_s = 0;
    long und_calls = 0, und_jobs = 0;                // undistortion (Camera.NeedUndistortion): ssx_undistort_plan_apply calls and their jobs, two per frame
    double und_s = 0;
    long reloc_calls = 0, reloc_jobs = 0;            // relocalisation: ssx_kfdb_relocalize_query_batch calls and their jobs (one per lost stream and frame)
    long pose_calls = 0, pose_jobs = 0;              // ssx_pnp_pose_batch calls of the lost streams' candidates and the pose jobs in them
    double reloc_s = 0, pose_s = 0;
  };
  Stats stats();
  void ResetStats();                                 // (after the streams' warm-up: the counters then describe the frames alone)

  // the slice of the pinned image arena of stream k's cohort, in bytes: 0 until the cohort's first stream has pinned its first image
  // (that stream's image size sets it, see Impl::PinSlice -- tests order the streams' first calls by it)
  size_t PinnedSliceBytes(int k);

  struct Impl;

 private:
  std::vector<std::unique_ptr<Impl>> impls_;
  int n_streams_ = 0;
};

}  // namespace ssx::host
