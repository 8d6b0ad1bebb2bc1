// tests/host/test_loop_units.cpp -- TEST INFRASTRUCTURE: LoopClosing, Backend and Map of the host layer against a SCRIPTED LoopCompute
// (records its inputs, returns canned results) and a recording BaWindow.  No GPU, no Python, no oracle.
//   test_loop_units <scenario file>
// The scenario (tests/test_loop_host.py writes it from tools/mapmodel.make_window_scenario) is a list of commands, one per line:
//   setup <n_active> <loop async> <backend async> <keep kf id>
//   point <id> x y z                                   a new map point
//   kf <id> <last id|-1> <pose7> <n>  + n lines "<map point id|-1> u v"      a keyframe through Backend::InsertKeyFrame (no optimisation)
//   condemn <map point id> / flush                     the front-end condemns a map point / the end of an optimisation deletes them
//   unlink <kf id> <feature index>                     an outlier edge: the observation goes, the feature loses its map point
//   script <kf id> <found> <loop id> <score> <n_pairs> <pairs...> <verdict> <need_correct> <error> <corrected7> <relative7> <kept...>
// Everything the run did is printed; the Python test compares it with the model.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

#include "../../ssvio_amd/host/backend.hpp"
#include "../../ssvio_amd/host/loopclosing.hpp"

using namespace ssx::host;

namespace {

std::mutex g_out;                                     // the loop thread and the main thread both print

struct Script {
  int found = 0; long loop = -1; float score = 0; std::vector<int32_t> pairs;
  int verdict = 0, need_correct = 0; double error = 0, corrected[7] = {0, 0, 0, 1, 0, 0, 0}, relative[7] = {0, 0, 0, 1, 0, 0, 0};
  std::vector<uint8_t> kept;
};

class ScriptedLoopCompute final : public LoopCompute {
 public:
  std::map<long, Script> scripts;
  long current = -1;
  void ProcessKeyframe(int64_t kf_id, const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int levels, int min_db, int gap,
                       float thr, ssx_kfdb_step_result& res, std::vector<int32_t>& pairs) override
  {
    std::lock_guard<std::mutex> lk(g_out);
    std::printf("call process kf %ld image %dx%d features %zu first_class %d nfeatures %d levels %d min_db %d gap %d thr %.3f\n", (long)kf_id, img.cols, img.rows, features.size(),
                features.empty() ? -1 : features[0].class_id, prm.nfeatures, levels, min_db, gap, thr);
    current = (long)kf_id;
    res = ssx_kfdb_step_result{};
    pairs.clear();
    auto it = scripts.find(current);
    if (it == scripts.end()) return;
    res.found = it->second.found; res.loop_kf_id = it->second.loop; res.score = it->second.score; res.n_pairs = (int32_t)(it->second.pairs.size() / 2);
    pairs = it->second.pairs;
  }
  void AddPending() override
  {
    std::lock_guard<std::mutex> lk(g_out);
    std::printf("call add_pending kf %ld\n", current);
  }
  void ComputePose(int n, const double* xyz, const uint8_t* has, const double* uv, const double* T_cur, const double* T_loop, const double* K4, uint8_t* kept,
                   ssx_loop_pose_result& out) override
  {
    const Script& s = scripts.at(current);
    std::lock_guard<std::mutex> lk(g_out);
    std::printf("call compute_pose kf %ld n %d has", current, n);
    for (int i = 0; i < n; ++i) std::printf(" %d", has[i]);
    std::printf(" xyz0 %.17g uv0 %.9g %.9g tcur %.17g tloop %.17g fx %.6f\n", xyz[0], uv[0], uv[1], T_cur[4], T_loop[4], K4[0]);
    out = ssx_loop_pose_result{};
    out.verdict = s.verdict; out.need_correct = s.need_correct; out.error = s.error;
    for (int i = 0; i < n; ++i) { kept[i] = s.kept.at((size_t)i); out.n_with_point += has[i]; out.n_inliers += kept[i]; }
    std::copy(s.corrected, s.corrected + 7, out.corrected_pose);
    std::copy(s.relative, s.relative + 7, out.relative_to_loop);
  }
  void LoopCorrect(const ssx_loop_correct_problem& p, ssx_loop_correct_result& res) override
  {
    std::lock_guard<std::mutex> lk(g_out);
    std::printf("problem n_keyframes %d n_edges %d n_points %d cur %d loop %d initial %d keep %d corrected_tx %.17g\n", p.n_keyframes, p.n_edges, p.n_points, p.cur_kf, p.loop_kf,
                p.initial_kf, p.keep_kf, p.corrected_pose[4]);
    std::printf("problem kf_active");
    for (int i = 0; i < p.n_keyframes; ++i) std::printf(" %d", p.kf_active[i]);
    std::printf("\nproblem pose_tx");
    for (int i = 0; i < p.n_keyframes; ++i) std::printf(" %.17g", p.poses[7 * i + 4]);
    std::printf("\nproblem edges");
    for (int e = 0; e < p.n_edges; ++e) std::printf(" %d:%d:%.17g", p.edge_i[e], p.edge_j[e], p.edge_meas[7 * e + 4]);
    std::printf("\nproblem anchors");
    for (int j = 0; j < p.n_points; ++j) std::printf(" %d", p.point_anchor[j]);
    std::printf("\nproblem point_active");
    for (int j = 0; j < p.n_points; ++j) std::printf(" %d", p.point_active[j]);
    std::printf("\n");
    for (int i = 0; i < p.n_keyframes; ++i) p.poses[7 * i + 5] += 0.25;      // a recognisable "correction": the write-back is checked against it
    for (int j = 0; j < p.n_points; ++j) p.points[3 * j + 1] += 0.125;
    res = ssx_loop_correct_result{};
    res.pg.n_iters = 7; res.n_active_kf = 5; res.n_active_points_moved = 11; res.n_other_points_moved = 13; res.n_points_skipped = 17;
  }
};

class RecordingWindow final : public BaWindow {
 public:
  void Push(int64_t, const double*, int, const int64_t*, const double*, const uint8_t*, int, const int64_t*, const double*, const uint8_t*) override {}
  void Pop(int64_t) override {}
  void RemoveLandmarks(int, const int64_t*) override {}
  void RemoveFlagged(int, const uint8_t*) override {}
  void Size(int& a, int& b, int& c) override { a = b = c = 0; }
  void Export(int64_t*, int64_t*, uint8_t*, int32_t*, int32_t*, double*) override {}
  void Solve(ssx_ba_result&) override {}
  void LoopCorrect(int64_t cur, const double* pose7, int n, const int64_t* ids, ssx_ba_window_loop_result*) override
  {
    std::lock_guard<std::mutex> lk(g_out);
    std::printf("window_loop_correct cur %ld tx %.17g fused", (long)cur, pose7[4]);
    for (int i = 0; i < n; ++i) std::printf(" %ld", (long)ids[i]);
    std::printf("\n");
  }
};

class NoCompute final : public Compute {
 public:
  void Detect(const Image&, const uint8_t*, const ssx_orb_params&, std::vector<ssx_keypoint>&) override { throw std::logic_error("not scripted"); }
  void TrackLK(const Image&, const Image&, const std::vector<float>&, std::vector<float>&, std::vector<uint8_t>&, bool) override { throw std::logic_error("not scripted"); }
  int PoseOnly(double*, const double*, int, const double*, const double*, uint8_t*) override { throw std::logic_error("not scripted"); }
  void Triangulate(int, const double*, const double*, const ssx_stereo_rig&, const double*, double*, uint8_t*) override { throw std::logic_error("not scripted"); }
  void BundleAdjust(const ssx_ba_problem&, const ssx_ba_options&, ssx_ba_result&) override { throw std::logic_error("not scripted"); }
  std::unique_ptr<BaWindow> MakeBaWindow(const double*, const double*, const ssx_ba_options&) override { return std::make_unique<RecordingWindow>(); }
};

}  // namespace

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in.is_open()) return 2;
  try {
    std::string line, cmd;
    std::getline(in, line);
    std::istringstream hs(line);
    int n_active = 5, loop_async = 0, backend_async = 0;
    long keep = -1;
    hs >> cmd >> n_active >> loop_async >> backend_async >> keep;
    if (cmd != "setup") throw std::runtime_error("the scenario must begin with setup");
    Setting cfg;
    cfg.Set("Backend.Async", std::to_string(backend_async)); cfg.Set("Loop.Closing.Async", std::to_string(loop_async));
    cfg.Set("ORBextractor.nNewFeatures", "100"); cfg.Set("ORBextractor.scaleFactor", "1.2"); cfg.Set("ORBextractor.nLevels", "8");
    cfg.Set("ORBextractor.iniThFAST", "20"); cfg.Set("ORBextractor.minThFAST", "7");
    cfg.Set("Loop.Threshold.Heigher", "0.375"); cfg.Set("Pyramid.Level", "4"); cfg.Set("Loop.Closig.Keyframe.Database.Min.Size", "3");
    cfg.Set("Loop.Min.Keyframe.Gap", "6");
    const Camera left{718.856, 718.856, 607.1928, 185.2157, 0.0, SE3()}, right{718.856, 718.856, 607.1928, 185.2157, 0.5, SE3::translation(-0.5, 0, 0)};
    auto map = std::make_shared<Map>((unsigned)n_active);
    map->keep_keyframe_images = true;
    NoCompute compute;
    auto scripted = std::make_unique<ScriptedLoopCompute>();
    ScriptedLoopCompute* sc = scripted.get();
    // every script first: the loop thread reads them while later commands are still being replayed
    std::vector<std::string> commands;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      ls >> cmd;
      if (cmd != "script") { commands.push_back(line); continue; }
      long kf; size_t n_pairs;
      ls >> kf;
      Script& s = sc->scripts[kf];
      ls >> s.found >> s.loop >> s.score >> n_pairs;
      s.pairs.resize(2 * n_pairs);
      for (auto& p : s.pairs) ls >> p;
      ls >> s.verdict >> s.need_correct >> s.error;
      for (double& v : s.corrected) ls >> v;
      for (double& v : s.relative) ls >> v;
      s.kept.resize(n_pairs);
      for (auto& k : s.kept) { int v; ls >> v; k = (uint8_t)v; }
      if (!ls) throw std::runtime_error("bad script line for keyframe " + std::to_string(kf));
    }
    Backend backend(cfg, compute, map, left, right);
    LoopClosing loop(cfg, std::move(scripted), map, left);
    loop.SetBackend(&backend);
    loop.SetReferenceKeyFrame([keep] { return keep; });
    backend.SetLoopClosing(&loop);
    auto image = std::make_shared<Image>();
    image->rows = 8; image->cols = 16; image->data.assign(128, 7);

    size_t at = 0;
    std::map<long, KeyFramePtr> created;                               // (an asynchronous backend inserts a keyframe into the map later)
    auto next_line = [&]() -> std::string { if (at >= commands.size()) throw std::runtime_error("scenario ends inside a keyframe"); return commands[at++]; };
    while (at < commands.size()) {
      std::istringstream ls(next_line());
      ls >> cmd;
      std::unique_lock<std::mutex> map_lock(map->update_mutex);        // the front-end holds it while it works on a frame
      if (cmd == "point") {
        auto mp = std::make_shared<MapPoint>();
        ls >> mp->id >> mp->position[0] >> mp->position[1] >> mp->position[2];
        map->InsertMapPoint(mp);
      } else if (cmd == "kf") {
        auto kf = std::make_shared<KeyFrame>();
        double p[7]; size_t n;
        ls >> kf->key_frame_id >> kf->last_key_frame;
        for (double& v : p) ls >> v;
        ls >> n;
        kf->frame_id = kf->key_frame_id; kf->timestamp = 0.1 * kf->key_frame_id; kf->pose = SE3(p); kf->left_image = image;
        if (kf->last_key_frame >= 0) kf->relative_pose_to_last_kf = kf->pose * created.at(kf->last_key_frame)->pose.inverse();
        created[(long)kf->key_frame_id] = kf;
        for (size_t i = 0; i < n; ++i) {                               // KeyFrame::CreateKF
          std::istringstream fs(next_line());
          auto f = std::make_shared<Feature>();
          fs >> f->map_point >> f->x >> f->y;
          f->keyframe = (long)kf->key_frame_id;
          if (MapPointPtr mp = map->Lock(f)) mp->AddObservation(f);
          kf->features_left.push_back(f);
        }
        backend.InsertKeyFrame(kf, false);
      } else if (cmd == "condemn") {
        unsigned long id; ls >> id;
        MapPointPtr mp = map->Lock((long)id);
        if (mp && !mp->is_outlier) { mp->is_outlier = true; map->AddOutlierMapPoint(id); }
      } else if (cmd == "flush") {
        map->RemoveAllOutlierMapPoints();
        map->RemoveOldActiveMapPoints();
      } else if (cmd == "unlink") {
        unsigned long kf; size_t idx; ls >> kf >> idx;
        FeaturePtr f = map->GetAllKeyFrames().at(kf)->features_left.at(idx);
        if (MapPointPtr mp = map->Lock(f)) { mp->RemoveActiveObservation(f); mp->RemoveObservation(f); }
        f->map_point = kNoMapPoint;
      } else {
        throw std::runtime_error("unknown command " + cmd);
      }
    }
    backend.WaitIdle();
    loop.WaitIdle();

    std::lock_guard<std::mutex> map_lock(map->update_mutex);
    const std::map<unsigned long, KeyFramePtr> kfs(map->GetAllKeyFrames().begin(), map->GetAllKeyFrames().end());
    const std::map<unsigned long, MapPointPtr> mps(map->GetAllMapPoints().begin(), map->GetAllMapPoints().end());
    for (auto& kv : kfs) {
      std::printf("keyframe %lu active %d image %d loop %ld rel_tx %.17g ty %.17g feats", kv.first, (int)map->GetActiveKeyFrames().count(kv.first), kv.second->left_image ? 1 : 0,
                  kv.second->loop_key_frame, kv.second->relative_pose_to_loop_kf.d[4], kv.second->pose.d[5]);
      for (auto& f : kv.second->features_left) std::printf(" %ld", f->map_point);
      std::printf("\n");
    }
    for (auto& kv : mps) {
      std::printf("mappoint %lu active %d y %.17g obs", kv.first, (int)map->GetActiveMapPoints().count(kv.first), kv.second->position[1]);
      for (auto& f : kv.second->observations) {
        const auto& feats = kfs.at((unsigned long)f->keyframe)->features_left;
        size_t idx = 0;
        while (idx < feats.size() && feats[idx] != f) ++idx;
        std::printf(" %ld:%zu", f->keyframe, idx);
      }
      std::printf(" | active_obs %zu\n", kv.second->active_observations.size());
    }
    for (const auto& r : loop.records())
      std::printf("record kf %lu db %d found %d loop %ld pairs %d pose %d with_point %d inliers %d need_correct %d corrected %d fused %d same_point %d duplicate %d pg_iters %d moved %d %d %d\n",
                  r.kf_id, r.db_size, r.found, r.loop_kf_id, r.pairs, r.verdict, r.with_point, r.inliers, r.need_correct, r.corrected, r.fused, r.same_point_skipped,
                  r.duplicate_skipped, r.pg_iterations, r.active_points_moved, r.other_points_moved, r.points_skipped);
    std::printf("stats steps %ld corrections %ld dropped %ld paused %d\n", loop.stats().steps, loop.stats().corrections, loop.stats().dropped, (int)backend.HasPaused());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fatal: %s\n", e.what());
    return 1;
  }
  return 0;
}
