// tests/host/test_reloc_dispatch_units.cpp -- relocalisation in the stream batcher's dispatch core (ssvio_amd/host/batch_dispatch.hpp),
// without a GPU: the rule that packs the lost streams' pose jobs into calls (PackPoseCalls), and the keyframe dispatcher's rest rule
// when a stream's own thread files a request while it holds the stream's map mutex and the thread of its backend is blocked on that
// mutex.  Built by tests/test_pose_packing.py; a hang is a failure, so that file runs it under a time limit.
#include <array>
#include <atomic>
#include <cstdio>
#include <memory>
#include <mutex>
#include <stdexcept>

#include "../../ssvio_amd/host/batch_dispatch.hpp"

using namespace ssx::host;

static std::atomic<int> g_failed{0};
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); g_failed = 1; } } while (0)

namespace {

using Calls = std::vector<PoseCall>;
using Key = std::array<double, 4>;                  // (the batcher's key is the bytes of K4)
const Key A{450., 450., 160., 100.}, B{700., 700., 620., 188.};

void Packing()
{
  const int MAX = 64;                               // SSX_PNP_BATCH_MAX
  // requests of 8, 8, 0 and 3 jobs with one key: one call, the empty request takes no part
  CHECK((PackPoseCalls(std::vector<int>{8, 8, 0, 3}, std::vector<Key>{A, A, A, A}, MAX) == Calls{{{0, 0, 8}, {1, 0, 8}, {3, 0, 3}}}));
  // nine requests of 8 jobs: 64 + 8
  {
    const Calls got = PackPoseCalls(std::vector<int>(9, 8), std::vector<Key>(9, A), MAX);
    CHECK(got.size() == 2 && got[0].size() == 8 && got[1] == PoseCall{{8, 0, 8}});
    for (size_t r = 0; r < 8 && got.size() == 2 && got[0].size() == 8; ++r) CHECK((got[0][r] == PosePart{r, 0, 8}));
  }
  // two keys interleaved: two calls, in order of first appearance
  CHECK((PackPoseCalls(std::vector<int>{3, 5, 2, 4}, std::vector<Key>{B, A, B, A}, MAX) == Calls{{{0, 0, 3}, {2, 0, 2}}, {{1, 0, 5}, {3, 0, 4}}}));
  // an empty dispatch, and one whose requests have no jobs
  CHECK(PackPoseCalls(std::vector<int>{}, std::vector<Key>{}, MAX).empty());
  CHECK(PackPoseCalls(std::vector<int>{0, 0}, std::vector<Key>{A, B}, MAX).empty());
  // a request that does not fit is cut, and the cut does not cross into another key's call
  CHECK((PackPoseCalls(std::vector<int>{5, 7, 2}, std::vector<Key>{A, A, B}, 8) == Calls{{{0, 0, 5}, {1, 0, 3}}, {{1, 3, 4}}, {{2, 0, 2}}}));
  CHECK((PackPoseCalls(std::vector<int>{20}, std::vector<Key>{A}, 8) == Calls{{{0, 0, 8}}, {{0, 8, 8}}, {{0, 16, 4}}}));
  bool threw = false;
  try { PackPoseCalls(std::vector<int>{1}, std::vector<Key>{A}, 0); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
}

enum { LK, DET, BA, RELOC, POSES, N_KINDS };
const char* const NAMES[N_KINDS] = {"LK", "DET", "BA", "RELOC", "POSES"};

struct Latch {
  std::mutex mu; std::condition_variable cv; bool open = false;
  void Open() { { std::lock_guard<std::mutex> lk(mu); open = true; } cv.notify_all(); }
  void Wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return open; }); }
};

// The front-end of stream 0 is LOST: it holds the map mutex and files its query and then its poses from slot 0.  The thread of its
// backend (slot S + 0) wants the map mutex meanwhile: it files nothing, so its slot rests IDLE and nobody waits for it.  Stream 1 is lost
// at the same frame and stream 2 is tracking.  The queries meet in one dispatch, the poses in the next, and the backend's window solve
// comes after the front-end has let go of the mutex: the rest rule needs no case for relocalisation.
void LostUnderTheMapMutex()
{
  std::mutex log_mu, map_mu;
  std::vector<std::string> log;
  std::vector<BatchDispatch::Kind> kinds;
  for (int i = 0; i < N_KINDS; ++i)
    kinds.push_back({NAMES[i], [&, i](const std::vector<int>& slots, std::vector<std::string>&, long& calls, long& jobs) {
                       std::string s = std::string(NAMES[i]) + "{";
                       for (size_t j = 0; j < slots.size(); ++j) s += (j ? "," : "") + std::to_string(slots[j]);
                       { std::lock_guard<std::mutex> lk(log_mu); log.push_back(s + "}"); }
                       ++calls; jobs += (long)slots.size();
                     }});
  const int S = 3;
  BatchDispatch d(S, kinds, BatchDispatch::Dispatcher{{LK}, false, false}, BatchDispatch::Dispatcher{{RELOC, POSES, DET, BA}, true, true});
  Latch held, backend_started;
  std::atomic<bool> backend_has_mutex{false};
  std::vector<std::thread> th;
  th.emplace_back([&] {                             // stream 0's own thread
    d.Bind(0);
    {
      std::lock_guard<std::mutex> map_lock(map_mu);
      held.Open();
      backend_started.Wait();
      d.SubmitAndWait(d.Slot(0), RELOC);
      CHECK(!backend_has_mutex);
      d.SubmitAndWait(d.Slot(0), POSES);
      CHECK(!backend_has_mutex);
    }
    d.SubmitAndWait(d.Slot(0), LK);
    d.Finish(0);
  });
  th.emplace_back([&] {                             // the thread of stream 0's backend: not bound, so it files in slot S + 0
    held.Wait();
    backend_started.Open();
    CHECK(d.Slot(0) == S + 0);
    {
      std::lock_guard<std::mutex> map_lock(map_mu);
      backend_has_mutex = true;
    }
    d.SubmitAndWait(d.Slot(0), BA);
  });
  th.emplace_back([&] { d.Bind(1); held.Wait(); d.SubmitAndWait(1, RELOC); d.SubmitAndWait(1, POSES); d.SubmitAndWait(1, LK); d.Finish(1); });
  th.emplace_back([&] { d.Bind(2); held.Wait(); d.SubmitAndWait(2, LK); d.Finish(2); });
  for (auto& t : th) t.join();
  std::printf("lost under the map mutex:");
  for (const auto& l : log) std::printf(" %s", l.c_str());
  std::printf("\n");
  // stream 2's first LK request is served when all three are at rest; the queries share a dispatch and so do the poses
  auto at = [&](const std::string& what) { for (size_t i = 0; i < log.size(); ++i) if (log[i] == what) return (long)i; return -1L; };
  CHECK(at("RELOC{0,1}") >= 0 && at("POSES{0,1}") > at("RELOC{0,1}") && at("BA{3}") > at("POSES{0,1}"));
  CHECK(d.counters(RELOC).calls == 1 && d.counters(RELOC).jobs == 2 && d.counters(POSES).calls == 1 && d.counters(POSES).jobs == 2 && d.counters(BA).jobs == 1);
}

}  // namespace

int main()
{
  Packing();
  LostUnderTheMapMutex();
  if (g_failed) return 1;
  std::printf("reloc dispatch units: ok\n");
  return 0;
}
