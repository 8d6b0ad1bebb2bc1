// tests/host/test_guided_units.cpp -- TEST INFRASTRUCTURE: the guided search of LoopClosing::Relocalize against a SCRIPTED LoopCompute
// (records what it is asked, returns canned answers), built like test_reloc_units.  No GPU, no Python, no oracle.
//   test_guided_units <scenario file>
// The scenario (tests/test_guided_host.py writes it) is a list of commands, one per line:
//   setting <key> <value> / reset         as test_reloc_units
//   kf <token> ...                        the next keyframe of the map, one token per feature: "-" no map point, "<n>" the live map
//                                         point number n, "<n>!" that point condemned (is_outlier), "<n>~" that point no longer in the map.
//                                         A point's position is (n, 2, 3), so that the calls can be printed in the script's numbers.
//   run <accepted> <pairs> <inliers> <matched> <found> <after>
//        one Relocalize: the query names keyframe number <accepted> (in the order of the kf lines) with the pairs (i, i), i < <pairs>;
//        its pose has <inliers> inliers, the first pairs.  The guided search matches the first <matched> points it is given, each to
//        the lowest feature that is not taken; the refinement answers found = <found> with <after> inliers, the LAST <after> of its pairs.
//        The map is forgotten afterwards.
// Everything the run did is printed; the Python test compares it with tools/guided_model.py.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../ssvio_amd/host/loopclosing.hpp"

using namespace ssx::host;

namespace {

struct Script { long accepted_kf = -1; int pairs = 0, inliers = 0, matched = 0, found = 0, after = 0; };
struct Calls { int guided = 0, refine = 0; };

class ScriptedGuided final : public LoopCompute {
 public:
  Script s;
  Calls* calls = nullptr;
  void ProcessKeyframe(int64_t, const Image&, const std::vector<ssx_keypoint>&, const ssx_orb_params&, int, int, int, float, ssx_kfdb_step_result&,
                       std::vector<int32_t>&) override { throw std::logic_error("not scripted"); }
  void AddPending() override { throw std::logic_error("not scripted"); }
  void ComputePose(int, const double*, const uint8_t*, const double*, const double*, const double*, const double*, uint8_t*, ssx_loop_pose_result&) override
  {
    throw std::logic_error("not scripted");
  }
  void LoopCorrect(const ssx_loop_correct_problem&, ssx_loop_correct_result&) override { throw std::logic_error("not scripted"); }
  void RelocalizeQuery(const Image&, const std::vector<ssx_keypoint>&, const ssx_orb_params&, int, int, float, float, ssx_reloc_query_result& res,
                       std::vector<std::vector<int32_t>>& pairs) override
  {
    res = ssx_reloc_query_result{};
    res.n_candidates = 1;
    res.cand[0].kf_id = s.accepted_kf; res.cand[0].score = 1.f; res.cand[0].n_pairs = s.pairs;
    pairs.assign(1, {});
    for (int i = 0; i < s.pairs; ++i) { pairs[0].push_back(i); pairs[0].push_back(i); }
  }
  void PosesBatch(const double*, std::vector<ssx_pnp_pose_job>& jobs) override
  {
    for (ssx_pnp_pose_job& j : jobs) {
      j.found = 1; j.n_inliers = s.inliers; j.n_ransac_inliers = s.inliers; j.best_hypothesis = 0;
      const double h = 0.70710678118654757;                              // a quarter turn about z, t = (1, 2, 3)
      const double pose[7] = {0, 0, h, h, 1, 2, 3};
      std::copy(pose, pose + 7, j.pose_out);
      for (int i = 0; i < j.M; ++i) j.inlier_out[i] = i < s.inliers ? 1 : 0;
    }
  }
  void GuidedSearch(const Image& img, const std::vector<ssx_keypoint>& features, const ssx_orb_params& prm, int levels, const std::vector<uint8_t>& taken,
                    const double* K4, const double* T, const std::vector<int64_t>& point_kf, const std::vector<int32_t>& point_cls, const std::vector<double>& xyz,
                    const GuidedParams& gp, GuidedMatches& out) override
  {
    ++calls->guided;
    std::printf("guided image %dx%d features %zu nfeatures %d levels %d fx %.1f radius %.3f max_distance %d ratio %d\n", img.cols, img.rows, features.size(), prm.nfeatures,
                levels, K4[0], gp.radius, gp.max_distance, gp.ratio_pct);
    std::printf("pose");
    for (int k = 0; k < 12; ++k) std::printf(" %.6f", T[k] + 0.0);
    std::printf("\ntaken ");
    for (uint8_t t : taken) std::printf("%d", t ? 1 : 0);
    std::printf("\ngather");
    for (size_t p = 0; p < point_kf.size(); ++p) std::printf(" %.0f:%ld:%d", xyz[3 * p], (long)point_kf[p], point_cls[p]);
    std::printf("\n");
    const size_t P = point_kf.size();
    out.feat.assign(P, -1); out.d1.assign(P, -1); out.d2.assign(P, -1); out.status.assign(P, SSX_GUIDED_NO_FEATURE);
    out.n_matched = 0;
    size_t f = 0;
    for (size_t p = 0; p < P && (int)p < s.matched; ++p) {
      while (f < taken.size() && taken[f]) ++f;
      if (f == taken.size()) break;
      out.feat[p] = (int32_t)f++; out.d1[p] = 7; out.status[p] = SSX_GUIDED_MATCHED; ++out.n_matched;
    }
  }
  void RefinePose(const double* K4, int M, const double* xyz, const double* uv, double* pose_io, uint8_t* inlier_out, int* n_inliers, int* found) override
  {
    ++calls->refine;
    std::printf("refine fx %.1f tx %.1f M %d pairs", K4[0], pose_io[4], M);
    for (int i = 0; i < M; ++i) std::printf(" %.0f:%.1f", xyz[3 * i], uv[2 * i]);
    std::printf("\n");
    for (int i = 0; i < M; ++i) inlier_out[i] = i >= M - s.after ? 1 : 0;
    *n_inliers = std::min(s.after, M); *found = s.found;
    pose_io[4] = 77.0;
  }
};

void Run(const Setting& cfg, const std::vector<std::string>& kf_lines, Script s, int accepted)
{
  auto map = std::make_shared<Map>(5u);
  auto image = std::make_shared<Image>();
  image->rows = 20; image->cols = 32; image->data.assign(640, 7);
  std::unordered_map<long, MapPointPtr> points;                          // by the script's number
  std::vector<long> kf_ids;
  for (const std::string& line : kf_lines) {
    FramePtr frame = map->NewFrame(image, image, 0.0);
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      auto f = std::make_shared<Feature>();
      f->x = (float)frame->features_left.size(); f->y = 1.f;
      if (tok != "-") {
        const char flag = tok.back();
        const long n = std::stol(tok);
        MapPointPtr& mp = points[n];
        if (!mp) {
          const double p[3] = {(double)n, 2.0, 3.0};
          mp = map->NewMapPoint(p);
          mp->is_outlier = flag == '!';
          if (flag != '~') map->InsertMapPoint(mp);
        }
        f->map_point = (long)mp->id;
      }
      frame->features_left.push_back(f);
    }
    KeyFramePtr kf = map->CreateKF(frame);
    map->InsertKeyFrame(kf);
    kf_ids.push_back((long)kf->key_frame_id);
  }
  std::printf("keyframes");
  for (long id : kf_ids) std::printf(" %ld", id);
  std::printf("\n");
  s.accepted_kf = kf_ids.at((size_t)accepted);
  Calls calls;
  auto compute = std::make_unique<ScriptedGuided>();
  compute->s = s; compute->calls = &calls;
  Camera left{450.0, 450.0, 160.0, 100.0, 0.0, SE3()};
  LoopClosing lc(cfg, std::move(compute), map, left);
  std::vector<ssx_keypoint> feats(48);
  for (int i = 0; i < 48; ++i) feats[(size_t)i] = ssx_keypoint{(float)i + 0.5f, 4.f, 7.f, -1.f, 0.f, 0, i};
  const double K4[4] = {left.fx, left.fy, left.cx, left.cy};
  LoopClosing::RelocResult r;
  const bool ok = lc.Relocalize(42, *image, feats, K4, r);
  std::printf("result ok %d guided %d kf %ld tx %.1f qz %.17g inliers %d matches %zu list", ok ? 1 : 0, lc.guided() ? 1 : 0, r.kf_id, r.T_cw.d[4], r.T_cw.d[2], r.inliers,
              r.matches.size());
  for (const auto& m : r.matches) {
    MapPointPtr mp = map->Lock(m.second);
    std::printf(" %d:%.0f", m.first, mp ? mp->position[0] : -1.0);
  }
  const LoopClosing::RelocRecord& rec = lc.reloc_records().back();
  std::printf("\nrecord frame %lu inliers %d accepted %ld guided_points %d guided_matches %d guided_inliers %d\n", rec.frame_id, rec.inliers, rec.accepted, rec.guided_points,
              rec.guided_matches, rec.guided_inliers);
  std::printf("calls guided %d refine %d\n", calls.guided, calls.refine);
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in.is_open()) return 2;
  Setting cfg;
  std::vector<std::string> kf_lines;
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
      } else if (cmd == "reset") {
        cfg = Setting();
      } else if (cmd == "kf") {
        std::string rest;
        std::getline(ss, rest);
        kf_lines.push_back(rest);
      } else if (cmd == "run") {
        Script s;
        int accepted = 0;
        ss >> accepted >> s.pairs >> s.inliers >> s.matched >> s.found >> s.after;
        std::printf("run\n");
        try {
          Run(cfg, kf_lines, s, accepted);
        } catch (const std::exception& e) {
          std::printf("error %s\n", e.what());
        }
        kf_lines.clear();
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fatal: %s\n", e.what());
    return 1;
  }
  return 0;
}
