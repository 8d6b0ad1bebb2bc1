// ssvio_amd/host/run_kitti.cpp -- headless equivalent of the reference's test_system
// (/root/reference/test/test_system.cpp:18-53): load a KITTI-layout stereo sequence, feed every pair to System::RunStep,
// save the keyframe trajectory in TUM format.  Same two flags (gflags spelling), plus a frame limit and an output path.
//
//   ssx_run_kitti --config_yaml_path=cfg.yaml --kitti_dataset_path=<sequence dir> [--max_frames=N] [--trajectory=out.txt]
//                 [--device=0] [--decode_threads=8] [--streams=1] [--preload=0] [--batched=0] [--loop_batched=0] [--undistort_batched=0] [--warmup=1] [--loop_log=FILE]
//                 [--dense_dir=DIR] [--dense_ply=FILE]
// The PNG pairs are decoded ahead of the tracker on worker threads (StereoPrefetcher); everything else is the
// reference's single loop.  --streams=K runs K independent copies of the loop in K threads of this process (each with
// its own System, GPU contexts and prefetcher) on the same sequence: a single stream is latency-bound, several fill the
// GPU (BASELINE configs[4] runs one stream per GPU; this is the one-GPU version of it).  --kitti_dataset_path may be a
// comma-separated list: stream k then runs sequence k mod (number of sequences) -- several DIFFERENT sequences at once.
// --batched=C (with --streams=K): the streams' per-frame compute calls and window optimisations go to the GPU as batched library
// calls (StreamBatcher, stream_batcher.hpp), the streams dealt to C cohorts that are batched independently (C = 2: one cohort's call
// on the GPU while the other's streams run their host code); every stream's trajectory stays byte-identical to its single-stream run.
// --warmup=1 (default): System::Warmup before the first frame -- the library's kernels are loaded and its workspaces sized on a
// synthetic frame, outside the frame loop and its clock (a stream's first window solve alone costs 15 - 20 ms cold, 0.5 ms warm);
// the trajectory is the same with --warmup=0.
// --loop_log=FILE (with Loop.Closing.Open: 1): one line per keyframe the loop step handled (stream k of --streams writes FILE.k):
//   kf <id> db <database size> found <0|1> loop <id|-1> score <float, 9 digits> pairs <n> pose <ssx_loop_verdict|-1> with_point <n> inliers <n>
//   error <17 digits> need_correct <0|1> corrected <0|1> fused <n> same_point <n> pg_iters <n> moved_active <n> moved_other <n> skipped <n> duplicate <n>
//   and, with Relocalization.Open: 1, behind them one line per attempt of a lost front-end:
//   reloc_frame <frame id> candidates <n> pairs <n> poses <n> inliers <n> accepted <keyframe id|-1>
//   and, only with Relocalization.Guided.Open: 1, on the same line: guided_points <n> guided_matches <n> guided_inliers <n|-1>
//   (--batched >= 1 with that key is refused: the batched dispatcher has no guided search)
// Relocalization.Open: 1 works per stream of an unbatched --streams.  --batched >= 1 with the key set is refused unless --loop_batched=1 is
// given (the rule of loop closing): the candidate queries of the streams that lost tracking then go out as ssx_kfdb_relocalize_query_batch
// calls and the poses of their candidates as packed ssx_pnp_pose_batch calls, and every stream still writes the bytes of its single run.
// The cohort shares one vocabulary there: with loop closing on, a DBOW2.VOC.Path that is missing or cannot be read is refused at once.
// Camera.NeedUndistortion: 1 (every frame's pair goes through ssx_undistort first) works per stream of an unbatched --streams.  --batched >= 1 with the key
// set is refused unless --undistort_batched=1 is given: the pairs of a cohort's streams then go through the lenses' stored maps in ONE
// ssx_undistort_plan_apply call per frame (two jobs a stream, one map per camera of the rig), and every stream still writes the bytes of its
// single-stream run.  With the key 0 or absent the flag changes nothing; without --batched >= 1 it is refused.
// Camera.Rectify: 1 (a raw rig: every frame's pair goes through ssx_undistort_lens into the common rectified camera first; system.hpp)
// stands under the same rules and the same flag: its maps are stored maps like any other.
// Loop closing is per stream.  --batched >= 1 with Loop.Closing.Open: 1 is refused unless --loop_batched=1 is given: the streams of a cohort
// then share one loop context and one vocabulary, and their inline keyframe steps go to the GPU as ssx_kfdb_process_keyframe_batch calls
// (every stream still writes the bytes of its single-stream run).  The loop thread (Loop.Closing.Async: 1) is not batched: refused with it.
// Dense.Open: 1: every keyframe's pair goes through ssx_stereo_dense at insertion.  --dense_dir=DIR writes each keyframe's full map
// then, as DIR/kf_%06ld.disp16 by keyframe id: raw little-endian int16, rows x cols, 1/16 pixel, -16 = invalid.  --dense_ply=FILE writes the
// run's dense cloud at the end (System::SaveDenseCloud).  Stream k of --streams writes DIR.k and FILE.k; the directories must exist.
// --batched >= 1 with the key set is refused: the dispatcher has no dense request kind.
// Dense.Speckle.Size: N / Dense.Speckle.Range: R: components of at most N pixels leave every map (and the cloud).
// Dense.Cloud.OnDevice: 1: the cloud's samples are made on the device; the full map then comes down only with --dense_dir.
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "stream_batcher.hpp"
#include "system.hpp"

namespace {

bool flag(const char* arg, const char* name, std::string& out)
{
  std::string a(arg);
  while (!a.empty() && a[0] == '-') a.erase(0, 1);
  const size_t n = std::strlen(name);
  if (a.compare(0, n, name) != 0 || a.size() <= n || a[n] != '=') return false;
  out = a.substr(n + 1);
  return true;
}

// --dense_dir: each keyframe's map leaves for its file when the front-end shows it
void AttachDenseDir(ssx::host::System& sys, const std::string& dir)
{
  if (dir.empty() || !sys.frontend().dense().open) return;
  sys.frontend().SetDenseSink([dir](unsigned long kf_id, const std::vector<int16_t>& disp, int rows, int cols) {
    char name[32];
    std::snprintf(name, sizeof name, "/kf_%06ld.disp16", (long)kf_id);
    std::FILE* f = std::fopen((dir + name).c_str(), "wb");
    if (!f) throw std::runtime_error("--dense_dir: cannot write " + dir + name);
    const size_t n = (size_t)rows * cols, put = std::fwrite(disp.data(), sizeof(int16_t), n, f);
    if (std::fclose(f) != 0 || put != n) throw std::runtime_error("--dense_dir: writing " + dir + name + " failed");
  });
}

void WriteLoopLog(ssx::host::System& sys, const std::string& path)
{
  if (path.empty() || !sys.loop_closing()) return;
  sys.WaitIdle();
  std::FILE* f = std::fopen(path.c_str(), "w");
  if (!f) throw std::runtime_error("--loop_log: cannot write " + path);
  for (const auto& r : sys.loop_closing()->records())
    std::fprintf(f, "kf %lu db %d found %d loop %ld score %.9g pairs %d pose %d with_point %d inliers %d error %.17g need_correct %d corrected %d fused %d same_point %d "
                 "pg_iters %d moved_active %d moved_other %d skipped %d duplicate %d\n", r.kf_id, r.db_size, r.found, r.loop_kf_id, (double)r.score, r.pairs, r.verdict, r.with_point,
                 r.inliers, r.error, r.need_correct, r.corrected, r.fused, r.same_point_skipped, r.pg_iterations, r.active_points_moved, r.other_points_moved,
                 r.points_skipped, r.duplicate_skipped);
  // then one line per relocalisation attempt of the front-end (Relocalization.Open: 1), in the same key / value form
  // (with Relocalization.Guided.Open: 1 the guided search's counts behind them; with the key off the line is as it was)
  const bool guided = sys.loop_closing()->guided();
  for (const auto& r : sys.loop_closing()->reloc_records()) {
    std::fprintf(f, "reloc_frame %lu candidates %d pairs %d poses %d inliers %d accepted %ld", r.frame_id, r.candidates, r.pairs, r.poses, r.inliers, r.accepted);
    if (guided) std::fprintf(f, " guided_points %d guided_matches %d guided_inliers %d", r.guided_points, r.guided_matches, r.guided_inliers);
    std::fprintf(f, "\n");
  }
  std::fclose(f);
}

}  // namespace

int main(int argc, char** argv)
{
  std::string config, dataset, max_frames_s, trajectory, device_s, threads_s, streams_s, preload_s, batched_s, warmup_s, loop_log, loop_batched_s, undistort_batched_s, dense_dir, dense_ply;
  for (int i = 1; i < argc; ++i) {
    if (flag(argv[i], "config_yaml_path", config) || flag(argv[i], "kitti_dataset_path", dataset) || flag(argv[i], "max_frames", max_frames_s) ||
        flag(argv[i], "trajectory", trajectory) || flag(argv[i], "device", device_s) || flag(argv[i], "decode_threads", threads_s) || flag(argv[i], "streams", streams_s) || flag(argv[i], "preload", preload_s) || flag(argv[i], "batched", batched_s) || flag(argv[i], "warmup", warmup_s) || flag(argv[i], "loop_log", loop_log) || flag(argv[i], "loop_batched", loop_batched_s) ||
        flag(argv[i], "undistort_batched", undistort_batched_s) || flag(argv[i], "dense_dir", dense_dir) || flag(argv[i], "dense_ply", dense_ply))
      continue;
    std::fprintf(stderr, "unknown argument %s\n", argv[i]);
    return 2;
  }
  if (config.empty() || dataset.empty()) {
    std::fprintf(stderr, "usage: %s --config_yaml_path=<yaml> --kitti_dataset_path=<sequence dir> [--max_frames=N] [--trajectory=<tum file>] [--device=0] [--decode_threads=8] [--streams=1] [--preload=0] [--batched=0] [--loop_batched=0] [--undistort_batched=0] [--warmup=1] [--loop_log=<file>] [--dense_dir=<dir>] [--dense_ply=<file>]\n",
                 argv[0]);
    return 2;
  }
  using namespace ssx::host;
  using clk = std::chrono::steady_clock;
  try {
    // one sequence, or a comma-separated list of sequences for --streams
    struct Sequence {
      std::vector<std::string> left_paths, right_paths;
      std::vector<double> timestamps;
      size_t num_images = 0;
      std::vector<StereoPrefetcher::Pair> preloaded;
    };
    std::vector<Sequence> seqs;
    for (size_t pos = 0; pos <= dataset.size();) {
      const size_t comma = std::min(dataset.find(',', pos), dataset.size());
      Sequence sq;
      LoadKittiImagesTimestamps(dataset.substr(pos, comma - pos), sq.left_paths, sq.right_paths, sq.timestamps);
      sq.num_images = sq.left_paths.size();
      if (!max_frames_s.empty()) sq.num_images = std::min(sq.num_images, (size_t)std::atol(max_frames_s.c_str()));
      seqs.push_back(std::move(sq));
      pos = comma + 1;
    }
    std::vector<std::string>& left_paths = seqs[0].left_paths;
    std::vector<std::string>& right_paths = seqs[0].right_paths;
    std::vector<double>& timestamps = seqs[0].timestamps;
    const size_t num_images = seqs[0].num_images;
    std::printf("Num Images: %zu\n", num_images);

    const int streams = streams_s.empty() ? 1 : std::max(1, std::atoi(streams_s.c_str()));
    const bool loop_batched = !loop_batched_s.empty() && std::atoi(loop_batched_s.c_str()) != 0;
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Relocalization.Guided.Open") != 0) {
      std::fprintf(stderr, "--batched=%s with Relocalization.Guided.Open: 1 is not supported (the dispatcher of a batched cohort has no guided search); "
                   "run --streams unbatched, or switch the guided search off\n", batched_s.c_str());
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Dense.Open") != 0) {
      std::fprintf(stderr, "--batched=%s with Dense.Open: 1 is not supported (the dispatcher of a batched cohort has no dense request kind); "
                   "run --streams unbatched, or switch dense stereo off\n", batched_s.c_str());
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Relocalization.Open") != 0 && !loop_batched) {
      std::fprintf(stderr, "--batched=%s with Relocalization.Open: 1 is not supported without --loop_batched=1 (the lost streams' queries and poses go through the "
                   "dispatcher, on the cohort's loop context); or run --streams unbatched, or switch relocalisation off\n", batched_s.c_str());
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Loop.Closing.Open") != 0 && !loop_batched) {
      std::fprintf(stderr, "--batched=%s with Loop.Closing.Open: 1 is not supported without --loop_batched=1 (the loop step batched over the streams); "
                   "or run --streams unbatched, or switch loop closing off\n", batched_s.c_str());
      return 2;
    }
    const bool undistort_batched = !undistort_batched_s.empty() && std::atoi(undistort_batched_s.c_str()) != 0;
    if (undistort_batched && (batched_s.empty() || std::atoi(batched_s.c_str()) <= 0)) {
      std::fprintf(stderr, "--undistort_batched=1 needs --batched >= 1 (with --streams): it chooses how a batched cohort undistorts its images\n");
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Camera.NeedUndistortion") != 0 && !undistort_batched) {
      std::fprintf(stderr, "--batched=%s with Camera.NeedUndistortion: 1 is not supported without --undistort_batched=1 (the cohort's pairs undistorted in one call "
                   "per frame); or run --streams unbatched, or feed rectified images\n", batched_s.c_str());
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && Setting(config).Get<int>("Camera.Rectify") != 0 && !undistort_batched) {
      std::fprintf(stderr, "--batched=%s with Camera.Rectify: 1 is not supported without --undistort_batched=1 (the cohort's pairs rectified in one call "
                   "per frame); or run --streams unbatched, or feed rectified images\n", batched_s.c_str());
      return 2;
    }
    if (loop_batched && Setting(config).Get<int>("Loop.Closing.Open") != 0 && Setting(config).Get<int>("Loop.Closing.Async") != 0) {
      std::fprintf(stderr, "--loop_batched=1 with Loop.Closing.Async: 1 is not supported: the batched loop step is the inline one (no third thread per stream)\n");
      return 2;
    }
    if (!batched_s.empty() && std::atoi(batched_s.c_str()) > 0 && loop_batched && Setting(config).Get<int>("Relocalization.Open") != 0 &&
        Setting(config).Get<int>("Loop.Closing.Open") != 0) {
      // a lost stream asks the cohort's loop context, which loads ONE vocabulary for all streams when the first of them is built: said
      // here, before a context is made, and not by every stream's thread in turn
      const std::string voc_path = Setting(config).Get<std::string>("DBOW2.VOC.Path");
      if (voc_path.empty() || !std::ifstream(voc_path).is_open()) {
        std::fprintf(stderr, "--batched=%s --loop_batched=1 with Relocalization.Open: 1 is not supported without a vocabulary the cohort can share: "
                     "DBOW2.VOC.Path \"%s\" cannot be read\n", batched_s.c_str(), voc_path.c_str());
        return 2;
      }
    }
    const bool warmup = warmup_s.empty() || std::atoi(warmup_s.c_str()) != 0;
    if (streams > 1) {
      const int device = device_s.empty() ? 0 : std::atoi(device_s.c_str());
      const int dthreads = threads_s.empty() ? 8 : std::atoi(threads_s.c_str());
      std::vector<double> seconds(streams, 0.0);
      std::vector<size_t> keyframes(streams, 0), frames(streams, 0);
      std::vector<std::string> errors(streams);
      // --preload=1: decode every sequence once, before the clock starts (isolates tracking from PNG decoding)
      if (!preload_s.empty() && std::atoi(preload_s.c_str()) != 0)
        for (Sequence& sq : seqs) {
          StereoPrefetcher pf(sq.left_paths, sq.right_paths, sq.num_images, 32);
          for (size_t ni = 0; ni < sq.num_images; ++ni) sq.preloaded.push_back(pf.Next());
        }
      const int cohorts = batched_s.empty() ? 0 : std::atoi(batched_s.c_str());      // --batched=C: C cohorts of streams, each batched on its own
      const bool batched = cohorts > 0;
      std::unique_ptr<StreamBatcher> batcher;
      if (batched) batcher = std::make_unique<StreamBatcher>(device, streams, cohorts);
      // every stream builds its System (GPU contexts, window) first; the clock of the aggregate figure starts when all are ready
      std::mutex bm;
      std::condition_variable bcv;
      int ready = 0;
      clk::time_point t_go;
      std::vector<clk::time_point> t_end(streams);
      std::vector<std::thread> workers;
      const auto t_all0 = clk::now();
      for (int k = 0; k < streams; ++k)
        workers.emplace_back([&, k] {
          struct Fin { StreamBatcher* b; int k; ~Fin() { if (b) b->Finish(k); } } fin{batcher.get(), k};   // the dispatcher must not wait for a stream that is gone
          bool counted = false;
          auto arrive = [&] {
            std::unique_lock<std::mutex> lk(bm);
            if (!counted) { counted = true; if (++ready == streams) { if (batcher) batcher->ResetStats(); t_go = clk::now(); bcv.notify_all(); } }
            return lk;
          };
          try {
            const Sequence& sq = seqs[(size_t)k % seqs.size()];
            const size_t num_images = sq.num_images;
            frames[k] = num_images;
            System sys(config, batcher ? batcher->MakeCompute(k) : nullptr, device);
            AttachDenseDir(sys, dense_dir.empty() ? dense_dir : dense_dir + "." + std::to_string(k));
            std::unique_ptr<StereoPrefetcher> pf;
            if (sq.preloaded.empty()) pf = std::make_unique<StereoPrefetcher>(sq.left_paths, sq.right_paths, num_images, dthreads);
            StereoPrefetcher::Pair first;
            if (num_images > 0) first = pf ? pf->Next() : sq.preloaded[0];
            if (warmup && first.left && !first.left->empty()) sys.Warmup(first.left->rows, first.left->cols);   // (batched: the streams' warm-up calls are batched too)
            {
              auto lk = arrive();
              bcv.wait(lk, [&] { return ready == streams; });
            }
            const auto t0 = clk::now();
            for (size_t ni = 0; ni < num_images; ++ni) {
              StereoPrefetcher::Pair pair = ni == 0 ? first : pf ? pf->Next() : sq.preloaded[ni];
              if (pair.left->empty() || pair.right->empty()) throw std::runtime_error("Failed to load image " + sq.left_paths[ni]);
              sys.RunStep(pair.left, pair.right, sq.timestamps[ni]);
            }
            sys.WaitIdle();
            t_end[k] = clk::now();
            seconds[k] = std::chrono::duration<double>(t_end[k] - t0).count();
            keyframes[k] = sys.map().GetAllKeyFrames().size();
            fin.b = nullptr;
            if (batcher) batcher->Finish(k);                                  // before the trajectory is written and the System is torn down
            if (!trajectory.empty()) sys.SaveTrajectoryTUM(trajectory + "." + std::to_string(k));
            if (!loop_log.empty()) WriteLoopLog(sys, loop_log + "." + std::to_string(k));
            if (!dense_ply.empty() && sys.frontend().dense().open) sys.SaveDenseCloud(dense_ply + "." + std::to_string(k));
          } catch (const std::exception& e) {
            errors[k] = e.what();
            arrive();
          }
        });
      for (auto& w : workers) w.join();
      const double wall = std::chrono::duration<double>(clk::now() - t_all0).count();
      double sum = 0;
      size_t total_frames = 0;
      clk::time_point last = t_go;
      for (int k = 0; k < streams; ++k) {
        if (!errors[k].empty()) { std::fprintf(stderr, "fatal (stream %d): %s\n", k, errors[k].c_str()); return 1; }
        sum += frames[k] / std::max(seconds[k], 1e-9);
        total_frames += frames[k];
        last = std::max(last, t_end[k]);
        if (streams <= 16) std::printf("stream %d: %.1f frames/s, %zu keyframes\n", k, frames[k] / std::max(seconds[k], 1e-9), keyframes[k]);
      }
      const double span = std::chrono::duration<double>(last - t_go).count();
      std::printf("%d streams: aggregate %.1f frames/s (sum of the streams' loops incl. decoding), wall %.2f s incl. context creation\n", streams, sum, wall);
      std::printf("%d streams%s: %zu frames in %.4f s from the common start to the last stream's end = %.1f frames/s\n", streams, batched ? " (batched)" : "",
                  total_frames, span, total_frames / std::max(span, 1e-9));
      if (batcher) {
        const StreamBatcher::Stats bs = batcher->stats();
        std::printf("batched calls: LK %ld (%.1f jobs each), pose-only %ld (%.1f), window solves %ld (%.1f)\n", bs.lk_calls, bs.lk_jobs / std::max(1.0, (double)bs.lk_calls),
                    bs.po_calls, bs.po_jobs / std::max(1.0, (double)bs.po_calls), bs.ba_calls, bs.ba_jobs / std::max(1.0, (double)bs.ba_calls));
        std::printf("batched time: LK %.1f ms (%.3f per call), pose-only %.1f ms (%.3f), window solves %.1f ms (%.3f), keyframe calls (detection, stereo LK, "
                    "triangulation) %ld x %.1f jobs, %.1f ms (%.3f per call), dispatcher waiting for the streams' host code %.1f ms\n",
                    1e3 * bs.lk_s, 1e3 * bs.lk_s / std::max(1L, bs.lk_calls), 1e3 * bs.po_s, 1e3 * bs.po_s / std::max(1L, bs.po_calls), 1e3 * bs.ba_s,
                    1e3 * bs.ba_s / std::max(1L, bs.ba_calls), bs.kf_calls, bs.kf_jobs / std::max(1.0, (double)bs.kf_calls), 1e3 * bs.kf_s,
                    1e3 * bs.kf_s / std::max(1L, bs.kf_calls), 1e3 * bs.wait_s);
        if (bs.und_calls)
          std::printf("batched calls: undistort %ld (%.1f jobs each); und_calls %ld und_jobs %ld und_s %.6f (%.3f ms per call)\n", bs.und_calls,
                      bs.und_jobs / std::max(1.0, (double)bs.und_calls), bs.und_calls, bs.und_jobs, bs.und_s, 1e3 * bs.und_s / std::max(1L, bs.und_calls));
        if (bs.loop_calls || bs.single_calls)
          std::printf("batched loop steps: loop_calls %ld loop_jobs %ld loop_s %.6f (%.3f ms per call, %.1f jobs each); a correction's single calls %ld, %.1f ms\n",
                      bs.loop_calls, bs.loop_jobs, bs.loop_s, 1e3 * bs.loop_s / std::max(1L, bs.loop_calls), bs.loop_jobs / std::max(1.0, (double)bs.loop_calls),
                      bs.single_calls, 1e3 * bs.single_s);
        if (bs.reloc_calls || bs.pose_calls)
          std::printf("batched relocalisation: reloc_calls %ld reloc_jobs %ld pose_calls %ld pose_jobs %ld reloc_s %.6f pose_s %.6f\n", bs.reloc_calls, bs.reloc_jobs,
                      bs.pose_calls, bs.pose_jobs, bs.reloc_s, bs.pose_s);
      }
      return 0;
    }
    System system(config, nullptr, device_s.empty() ? 0 : std::atoi(device_s.c_str()));
    AttachDenseDir(system, dense_dir);
    double t_io = 0, t_step = 0;
    StereoPrefetcher prefetch(left_paths, right_paths, num_images, threads_s.empty() ? 8 : std::atoi(threads_s.c_str()));
    StereoPrefetcher::Pair first;
    if (num_images > 0) first = prefetch.Next();
    if (warmup && first.left && !first.left->empty()) {
      const auto tw = clk::now();
      system.Warmup(first.left->rows, first.left->cols);
      std::printf("warm-up (kernels loaded, workspaces sized; outside the frame loop): %.1f ms\n", std::chrono::duration<double, std::milli>(clk::now() - tw).count());
    }
    const auto t_begin = clk::now();
    for (size_t ni = 0; ni < num_images; ++ni) {
      const auto t0 = clk::now();
      StereoPrefetcher::Pair pair = ni == 0 ? first : prefetch.Next();
      ImagePtr left = pair.left, right = pair.right;
      if (left->empty() || right->empty()) {
        std::fprintf(stderr, "Failed to load image at: %s\n", (left->empty() ? left_paths[ni] : right_paths[ni]).c_str());
        return 1;
      }
      const auto t1 = clk::now();
      system.RunStep(left, right, timestamps[ni]);
      const auto t2 = clk::now();
      t_io += std::chrono::duration<double>(t1 - t0).count();
      t_step += std::chrono::duration<double>(t2 - t1).count();
      if (ni % 100 == 99) std::printf("Has processed %zu frames.\n", ni + 1);
    }
    system.SaveTrajectoryTUM(trajectory);
    WriteLoopLog(system, loop_log);
    if (!dense_ply.empty() && system.frontend().dense().open)
      std::printf("dense cloud: %zu points in %s\n", system.SaveDenseCloud(dense_ply), dense_ply.c_str());

    const StageTimes& st = system.frontend().times();
    const Backend::Stats& bs = system.backend().stats();
    const char* status[] = {"INITING", "TRACKING_GOOD", "TRACKING_BAD", "LOST"};
    std::printf("frames %zu  keyframes %zu  map points %zu  final status %s\n", num_images, system.map().GetAllKeyFrames().size(),
                system.map().GetAllMapPoints().size(), status[(int)system.frontend().status()]);
    const double t_all = std::chrono::duration<double>(clk::now() - t_begin).count();
    std::printf("RunStep %.3f ms/frame (%.1f frames/s); waiting for decoded images %.3f ms/frame; whole loop %.1f frames/s\n",
                1e3 * t_step / std::max<size_t>(num_images, 1), num_images / std::max(t_step, 1e-9), 1e3 * t_io / std::max<size_t>(num_images, 1),
                num_images / std::max(t_all, 1e-9));
    auto line = [](const char* name, double s, long n) {
      if (n) std::printf("  %-24s %6ld calls  %8.3f ms/call\n", name, n, 1e3 * s / n);
    };
    line("undistort (pair)", st.undistort, st.n_undistort);
    line("Detect", st.detect, st.n_detect);
    line("LK last -> current", st.lk_temporal, st.n_lk_temporal);
    line("LK left -> right", st.lk_stereo, st.n_lk_stereo);
    line("pose-only LM", st.pose_only, st.n_pose_only);
    line("triangulation", st.triangulate, st.n_triangulate);
    line("dense (keyframe pair)", st.dense, st.n_dense);
    line("keyframe insert + BA", st.bundle_adjust, st.n_bundle_adjust);
    std::printf("  local BA: %ld windows, %ld LM iterations, %ld edges, %ld outlier edges\n", bs.windows, bs.lm_iterations, bs.edges, bs.outlier_edges);
    if (bs.windows)
      std::printf("  per window on the host side: map + window edits %.3f ms, export + solve call %.3f ms, write-back %.3f ms\n", 1e3 * bs.t_insert / bs.windows,
                  1e3 * bs.t_solve / bs.windows, 1e3 * bs.t_apply / bs.windows);
    if (LoopClosing* lc = system.loop_closing()) {
      const LoopClosing::Stats& ls = lc->stats();
      long found = 0;
      for (const auto& r : lc->records()) found += r.found;
      std::printf("  loop closing%s: %ld steps, %.3f ms/step (corrections included), %ld keyframes dropped by the 5-id rule, %ld loops found, %ld corrections, %.3f ms/correction\n",
                  lc->async() ? " (own thread)" : "", ls.steps, 1e3 * ls.t_step / std::max(1L, ls.steps), ls.dropped, found, ls.corrections,
                  1e3 * ls.t_correct / std::max(1L, ls.corrections));
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fatal: %s\n", e.what());
    return 1;
  }
  return 0;
}
