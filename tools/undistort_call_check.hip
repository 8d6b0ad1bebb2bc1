// tools/undistort_call_check.hip -- the host side of csrc/undistort.hip that plans a call (ud_check with the overlap search, ud_build) in a
// program of its own, for the host sanitizers: no GPU, no Python, no preloaded library.
//
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import undistort_call_cases as c; sys.stdout.write(c.as_text())" > cases.txt
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -DSSX_BUILD -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/undistort_call_check.hip -o undistort_call_check
//   ./undistort_call_check cases.txt
//
// Every case of tests/undistort_call_cases.py at 45 x 67 goes through ssx_undistort_debug_plan, then the refusals: null pointers, short
// strides, bad tags, the three overlaps, images of unknown kind, and tables of 1024 jobs in ascending, descending and shuffled order with
// and without one overlapping pair.  Prints what it ran; exit 1 when a status is not the expected one.
#include "../ssvio_amd/csrc/undistort.hip"

#include <cstdio>
#include <memory>

namespace {

int failures = 0;

void expect(const char* what, int32_t got, int32_t want, const ssx_undistort_call_info& info)
{
  if (got != want) { std::printf("FAILED %s: status %d, expected %d (%s)\n", what, got, want, info.error); ++failures; }
}

}  // namespace

int main(int argc, char** argv)
{
  const int32_t rows = 45, cols = 67, img = rows * cols;
  auto info = std::make_unique<ssx_undistort_call_info>();
  int cases = 0, refusals = 0;
  std::FILE* f = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
  if (!f) { std::printf("usage: undistort_call_check cases.txt\n"); return 2; }
  int entry, on_device, n, src_one, dst_one;
  while (std::fscanf(f, "%d %d %d %d %d", &entry, &on_device, &n, &src_one, &dst_one) == 5) {
    std::vector<ssx_undistort_job_facts> jobs((size_t)n);
    std::vector<int8_t> sk((size_t)n), dk((size_t)n);
    for (int k = 0; k < n; ++k) {
      long long so, dof;
      int ss, ds, tag, a, b;
      if (std::fscanf(f, "%lld %d %lld %d %d %d %d", &so, &ss, &dof, &ds, &tag, &a, &b) != 7) return 2;
      jobs[k] = ssx_undistort_job_facts{so, dof, ss, ds, tag, 0};
      sk[k] = (int8_t)a; dk[k] = (int8_t)b;
    }
    const ssx_undistort_side_facts sf{src_one, 0, sk.data()}, df{dst_one, 0, dk.data()};
    expect("case", ssx_undistort_debug_plan(entry, rows, cols, on_device, n, jobs.data(), 2, &sf, &df, info.get()), SSX_OK, *info);
    ++cases;
  }
  std::fclose(f);

  const ssx_undistort_job_facts good{0, 2 * img, cols, cols, 0, 0};
  const auto refuse = [&](const char* what, std::vector<ssx_undistort_job_facts> jobs, int32_t want = SSX_ERR_INVALID_ARG, int32_t n = -2, int8_t kind = UD_DEVICE) {
    const std::vector<int8_t> kinds(jobs.size() + 1, kind);
    const ssx_undistort_side_facts facts{0, 0, kinds.data()};
    for (int entry = 0; entry < 3; ++entry) {
      if ((kind != UD_DEVICE) && entry != SSX_UD_ENTRY_PLAN_APPLY) continue;
      expect(what, ssx_undistort_debug_plan(entry, rows, cols, kind != UD_DEVICE, n == -2 ? (int32_t)jobs.size() : n, jobs.data(), 2, &facts, &facts, info.get()), want, *info);
      ++refusals;
    }
  };
  refuse("n < 0", {good}, SSX_ERR_INVALID_ARG, -1);
  refuse("n above the limit", {good}, SSX_ERR_INVALID_ARG, SSX_UNDISTORT_MAX_JOBS + 1);
  refuse("no jobs", {}, SSX_OK);
  refuse("null src", {ssx_undistort_job_facts{0, 2 * img, cols, cols, 0, SSX_UD_SRC_IS_NULL}});
  refuse("null dst", {good, ssx_undistort_job_facts{img, 0, cols, cols, 1, SSX_UD_DST_IS_NULL}});
  refuse("src stride", {ssx_undistort_job_facts{0, 2 * img, cols - 1, cols, 0, 0}});
  refuse("dst stride", {ssx_undistort_job_facts{0, 2 * img, cols, cols - 1, 0, 0}});
  refuse("tag", {ssx_undistort_job_facts{0, 2 * img, cols, cols, 7, 0}});
  refuse("in place", {ssx_undistort_job_facts{0, 0, cols, cols, 0, 0}});
  refuse("overlap by one byte", {ssx_undistort_job_facts{0, img - 1, cols, cols, 0, 0}});
  refuse("dst on another job's src", {good, ssx_undistort_job_facts{img, 0, cols, cols, 1, 0}});
  refuse("neighbours", {ssx_undistort_job_facts{0, img, cols, cols, 0, 0}}, SSX_OK);
  refuse("neither", {good}, SSX_ERR_INVALID_ARG, -2, UD_NEITHER);
  // full tables for the sorted search: sources in slices, destinations behind them; then one destination moved onto a source
  for (int order = 0; order < 3; ++order) {
    std::vector<ssx_undistort_job_facts> jobs((size_t)SSX_UNDISTORT_MAX_JOBS);
    const int32_t n = (int32_t)jobs.size();
    for (int32_t k = 0; k < n; ++k) {
      const int64_t at = order == 0 ? k : order == 1 ? n - 1 - k : (int64_t)((uint32_t)k * 389u % (uint32_t)n);      // (389 and 1024 are coprime: a permutation)
      jobs[k] = ssx_undistort_job_facts{at * 3072, (n + at) * 3072, cols, cols, (int32_t)(k % 2), 0};
    }
    refuse("full table", jobs, SSX_OK);
    jobs[n / 2].dst_off = jobs[n / 3].src_off + 100;
    refuse("full table with one overlapping pair", jobs);
  }
  std::printf("undistort_call_check: %d cases, %d refusal calls, %d failed\n", cases, refusals, failures);
  return failures ? 1 : 0;
}
