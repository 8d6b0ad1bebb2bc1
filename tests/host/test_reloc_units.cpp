// tests/host/test_reloc_units.cpp -- TEST INFRASTRUCTURE: LoopClosing::Relocalize against a SCRIPTED LoopCompute (records what it is asked,
// returns canned candidates and poses).  No GPU, no Python, no oracle.
//   test_reloc_units <scenario file>
// The scenario (tests/test_reloc_host.py writes it) is a list of commands, one per line:
//   setting <key> <value>                 a settings key for the cases that follow
//   reset                                 forget every setting
//   case <n>  + n lines "<live> <condemned> <none> <found> <n_inliers>"
//        n candidates, best first.  Candidate c is a keyframe whose first <live> features have a live map point, the next <condemned> a
//        map point the front-end has condemned, the last <none> no map point; the query pairs feature i of the frame with feature i of
//        the keyframe.  <found> / <n_inliers> is what the pose batch answers for it, should it be asked.
// Everything the run did is printed; the Python test compares it with tools/reloc_model.py.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../ssvio_amd/host/loopclosing.hpp"

using namespace ssx::host;

namespace {

struct Cand { int live = 0, condemned = 0, none = 0, found = 0, n_inliers = 0; long kf_id = -1; };

class ScriptedReloc final : public LoopCompute {
 public:
  std::vector<Cand> cands;
  void ProcessKeyframe(int64_t, const Image&, const std::vector<ssx_keypoint>&, const ssx_orb_params&, int, int, int, float, ssx_kfdb_step_result&,
                       std::vector<int32_t>&) override { throw std::logic_error("not scripted"); }
  void AddPending() override { throw std::logic_error("not scripted"); }
  void ComputePose(int, const double*, const uint8_t*, const double*, const double*, const double*, const double*, uint8_t*, ssx_loop_pose_result&) override
  {
    throw std::logic_error("not scripted");
  }
  void LoopCorrect(const ssx_loop_correct_problem&, ssx_loop_correct_result&) override { throw std::logic_error("not scripted"); }
  void RelocalizeQuery(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int levels, int max_candidates, float threshold,
                       float ratio, ssx_reloc_query_result& res, std::vector<std::vector<int32_t>>& pairs) override
  {
    std::printf("query image %dx%d features %zu class_last %d nfeatures %d levels %d K %d threshold %.6f ratio %.6f\n", img.cols, img.rows, features.size(),
                features.empty() ? -1 : features.back().class_id, prm.nfeatures, levels, max_candidates, threshold, ratio);
    res = ssx_reloc_query_result{};
    pairs.clear();
    for (size_t c = 0; c < cands.size() && (int)c < max_candidates; ++c) {
      const int n = cands[c].live + cands[c].condemned + cands[c].none;
      res.cand[c].kf_id = cands[c].kf_id; res.cand[c].row = (int32_t)c; res.cand[c].score = 1.f - 0.01f * c; res.cand[c].n_pairs = n;
      pairs.emplace_back();
      for (int i = 0; i < n; ++i) { pairs.back().push_back(i); pairs.back().push_back(i); }
      res.n_candidates = (int32_t)c + 1;
    }
  }
  void PosesBatch(const double* K4, std::vector<ssx_pnp_pose_job>& jobs) override
  {
    std::printf("poses fx %.3f jobs %zu", K4[0], jobs.size());
    size_t c = 0;
    for (ssx_pnp_pose_job& j : jobs) {
      while (c < cands.size() && cands[c].live < 10) ++c;                // the candidates that are asked, in rank order
      const Cand& s = cands.at(c);
      std::printf(" [rank %zu M %d seed %u xyz0 %.1f uv0 %.1f]", c, j.M, j.seed, j.xyz[0], j.uv[0]);
      j.found = s.found; j.n_inliers = s.found ? s.n_inliers : 0; j.n_ransac_inliers = j.n_inliers; j.best_hypothesis = s.found ? 0 : -1;
      const double pose[7] = {0, 0, 0, 1, (double)(c + 1), 0, 0};
      std::copy(pose, pose + 7, j.pose_out);
      for (int i = 0; i < j.M; ++i) j.inlier_out[i] = s.found && i < s.n_inliers ? 1 : 0;
      ++c;
    }
    std::printf("\n");
  }
};

void RunCase(const Setting& cfg, std::vector<Cand> cands)
{
  auto map = std::make_shared<Map>(5u);
  auto image = std::make_shared<Image>();
  image->rows = 20; image->cols = 32; image->data.assign(640, 7);
  int most = 0;
  for (Cand& c : cands) {
    // map point ids run on from candidate to candidate: a candidate's first point has the number of the earlier candidates' points
    FramePtr frame = map->NewFrame(image, image, 0.0);
    const int n = c.live + c.condemned + c.none;
    most = std::max(most, n);
    for (int i = 0; i < n; ++i) {
      auto f = std::make_shared<Feature>();
      f->x = (float)i; f->y = 1.f;
      if (i < c.live + c.condemned) {
        const double p[3] = {(double)i, 2.0, 3.0};
        MapPointPtr mp = map->NewMapPoint(p);
        mp->is_outlier = i >= c.live;
        map->InsertMapPoint(mp);
        f->map_point = (long)mp->id;
      }
      frame->features_left.push_back(f);
    }
    KeyFramePtr kf = map->CreateKF(frame);
    map->InsertKeyFrame(kf);
    c.kf_id = (long)kf->key_frame_id;
  }
  auto compute = std::make_unique<ScriptedReloc>();
  compute->cands = cands;
  Camera left{450.0, 450.0, 160.0, 100.0, 0.0, SE3()};
  LoopClosing lc(cfg, std::move(compute), map, left);
  std::vector<ssx_keypoint> feats((size_t)most);
  for (int i = 0; i < most; ++i) feats[(size_t)i] = ssx_keypoint{(float)i + 0.5f, 4.f, 7.f, -1.f, 0.f, 0, i};
  const double K4[4] = {left.fx, left.fy, left.cx, left.cy};
  LoopClosing::RelocResult r;
  const bool ok = lc.Relocalize(42, *image, feats, K4, r);
  std::printf("result ok %d open %d kf %ld tx %.1f inliers %d matches %zu candidates %d pairs %d first_match %d:%ld\n", ok ? 1 : 0, lc.relocalization() ? 1 : 0, r.kf_id,
              r.T_cw.d[4], r.inliers, r.matches.size(), r.candidates, r.pairs, r.matches.empty() ? -1 : r.matches[0].first, r.matches.empty() ? -1L : r.matches[0].second);
  const LoopClosing::RelocRecord& rec = lc.reloc_records().back();
  std::printf("record frame %lu candidates %d pairs %d poses %d inliers %d accepted %ld\n", rec.frame_id, rec.candidates, rec.pairs, rec.poses, rec.inliers, rec.accepted);
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in.is_open()) return 2;
  Setting cfg;
  std::string line;
  try {
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string cmd;
      if (!(ss >> cmd)) continue;
      if (cmd == "setting") {
        std::string key, value;
        ss >> key >> value;
        cfg.Set(key, value);
      } else if (cmd == "reset") {                                       // forget every setting (Setting has no erase: the test writes its keys anew)
        cfg = Setting();
      } else if (cmd == "case") {
        int n = 0;
        ss >> n;
        std::vector<Cand> cands((size_t)n);
        for (Cand& c : cands) {
          if (!std::getline(in, line)) return 2;
          std::istringstream cs(line);
          cs >> c.live >> c.condemned >> c.none >> c.found >> c.n_inliers;
        }
        std::printf("case %d\n", n);
        try {
          RunCase(cfg, cands);
        } catch (const std::exception& e) {
          std::printf("error %s\n", e.what());
        }
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fatal: %s\n", e.what());
    return 1;
  }
  return 0;
}
