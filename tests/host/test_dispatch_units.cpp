// tests/host/test_dispatch_units.cpp -- the stream batcher's dispatch core (ssvio_amd/host/batch_dispatch.hpp) without a GPU: the kinds
// are fakes that write (kind, slots) into a log, the streams are threads sequenced so that the state at every moment of rest is
// determined, and the log is compared exactly.  Built plain and under ThreadSanitizer by tests/test_batch_dispatch.py; a hang is the
// failure under test, so that file runs it under a time limit.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <stdexcept>

#include "../../ssvio_amd/host/batch_dispatch.hpp"

using namespace ssx::host;

static std::atomic<int> g_failed{0};
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed = 1; } } while (0)

namespace {

enum { LK, PO, DET, LKS, TRI, BA, N_KINDS };
const char* const NAMES[N_KINDS] = {"LK", "PO", "DET", "LKS", "TRI", "BA"};

struct Latch {
  std::mutex mu; std::condition_variable cv; bool open = false;
  void Open() { { std::lock_guard<std::mutex> lk(mu); open = true; } cv.notify_all(); }
  void Wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return open; }); }
};

std::string Fmt(const std::string& name, std::vector<int> slots)
{
  std::sort(slots.begin(), slots.end());
  std::string s = name + "{";
  for (size_t i = 0; i < slots.size(); ++i) s += (i ? "," : "") + std::to_string(slots[i]);
  return s + "}";
}

// a core with the batcher's two dispatchers (per frame: PO before LK, the streams' slots; keyframe path: DET, LKS, TRI, BA, all slots,
// waits for longops) over fake kinds: a dispatch is logged, then "called" through Isolated -- the call throws while `fail` names one
// of its slots
struct Rig {
  explicit Rig(int S) : fail(2 * (size_t)S)
  {
    for (auto& f : fail) f = false;
    std::vector<BatchDispatch::Kind> kinds;
    for (int i = 0; i < N_KINDS; ++i)
      kinds.push_back({NAMES[i], [this, i](const std::vector<int>& slots, std::vector<std::string>& errs, long& calls, long& jobs) {
                         { std::lock_guard<std::mutex> lk(mu); log.push_back(Fmt(NAMES[i], slots)); }
                         std::vector<size_t> all(slots.size());
                         for (size_t j = 0; j < all.size(); ++j) all[j] = j;
                         Isolated(all, errs, calls, jobs, [&](const std::vector<size_t>& sub) {
                           for (size_t j : sub) if (fail[slots[j]]) throw std::runtime_error("slot " + std::to_string(slots[j]) + " is at fault");
                         });
                       }});
    d = std::make_unique<BatchDispatch>(S, kinds, BatchDispatch::Dispatcher{{PO, LK}, false, false}, BatchDispatch::Dispatcher{{DET, LKS, TRI, BA}, true, true});
  }
  std::vector<std::string> Log() { std::lock_guard<std::mutex> lk(mu); return log; }
  // stream k's thread: binds itself, runs body, finishes
  template <class F> void Stream(int k, F body)
  {
    threads.emplace_back([this, k, body] {
      d->Bind(k);
      try { body(); } catch (const std::exception& e) { std::fprintf(stderr, "stream %d: unexpected %s\n", k, e.what()); g_failed = 1; }
      d->Finish(k);
    });
  }
  void Join() { for (auto& t : threads) t.join(); threads.clear(); }
  std::mutex mu;
  std::vector<std::string> log;
  std::vector<std::atomic<bool>> fail;
  std::unique_ptr<BatchDispatch> d;
  std::vector<std::thread> threads;
};

using Log = std::vector<std::string>;

void Report(const char* what, const Log& got)
{
  std::printf("%s:", what);
  for (const auto& l : got) std::printf(" %s", l.c_str());
  std::printf("\n");
}

// 1. pose-only before LK, and the straggler merges
void PoseOnlyFirst()
{
  Rig r(5);
  r.Stream(0, [&] { r.d->SubmitAndWait(0, LK); });
  for (int k = 1; k < 5; ++k) r.Stream(k, [&r, k] { r.d->SubmitAndWait(k, PO); r.d->SubmitAndWait(k, LK); });
  r.Join();
  Report("pose-only first", r.Log());
  CHECK((r.Log() == Log{"PO{1,2,3,4}", "LK{0,1,2,3,4}"}));
  const BatchDispatch::Counters po = r.d->counters(PO), lk = r.d->counters(LK);
  CHECK(po.calls == 1 && po.jobs == 4 && lk.calls == 1 && lk.jobs == 5 && po.seconds >= 0 && r.d->wait_s() >= 0);
  CHECK(r.d->counters(DET).calls == 0);
  r.d->ResetCounters();
  CHECK(r.d->counters(LK).calls == 0 && r.d->counters(LK).jobs == 0 && r.d->wait_s() == 0);
}   // 10. (teardown after work)

// 2. the earliest keyframe stage first, later streams catch up
void EarliestStageFirst()
{
  Rig r(4);
  for (int k = 0; k < 4; ++k)
    r.Stream(k, [&r, k] { for (int stage = DET + k; stage <= BA; ++stage) r.d->SubmitAndWait(k, stage); });
  r.Join();
  Report("earliest stage first", r.Log());
  CHECK((r.Log() == Log{"DET{0}", "LKS{0,1}", "TRI{0,1,2}", "BA{0,1,2,3}"}));
}

// 3. a stream in a call of its own holds the keyframe dispatcher back, not the per-frame one
void LongOpHoldsTheKeyframePath()
{
  Rig r(3);
  Latch entered, release;
  r.Stream(0, [&] {
    { BatchDispatch::LongOp op(*r.d, 0); entered.Open(); release.Wait(); }
    r.d->SubmitAndWait(0, DET);
  });
  r.threads.emplace_back([&] {                      // stream 1 (it finishes BEFORE it lets stream 0 go on: nobody waits for it then)
    r.d->Bind(1);
    entered.Wait();
    r.d->SubmitAndWait(1, LK);
    CHECK((r.Log() == Log{"LK{1}"}));               // served beside the longop; DET{2} is not
    r.d->Finish(1);
    release.Open();
  });
  r.Stream(2, [&] { r.d->SubmitAndWait(2, DET); });
  r.Join();
  Report("longop", r.Log());
  CHECK((r.Log() == Log{"LK{1}", "DET{0,2}"}));
}

// 4. a request in a backend slot is served after 2 ms although the stream's thread keeps running (it waits for that very request)
void BackendSlotIsServedAnyway()
{
  Rig r(1);
  Latch bound, served;
  r.Stream(0, [&] { bound.Open(); served.Wait(); });
  std::thread worker([&] {
    bound.Wait();
    const int slot = r.d->Slot(0);
    CHECK(slot == 1);
    r.d->SubmitAndWait(slot, BA);
    served.Open();
  });
  worker.join();
  r.Join();
  Report("backend slot", r.Log());
  CHECK((r.Log() == Log{"BA{1}"}));
}

// 5. without a backend request nothing is served early
void NoEarlyServiceWithoutBackendRequest()
{
  Rig r(2);
  r.Stream(0, [&] { r.d->SubmitAndWait(0, DET); });
  r.Stream(1, [&] { std::this_thread::sleep_for(std::chrono::milliseconds(20)); r.d->SubmitAndWait(1, DET); });
  r.Join();
  Report("no early service", r.Log());
  CHECK((r.Log() == Log{"DET{0,1}"}));
}

// 6. Isolated
void IsolatedRetries()
{
  Log made;
  auto call = [&](const std::vector<size_t>& sub) {
    made.push_back(Fmt("", std::vector<int>(sub.begin(), sub.end())));
    for (size_t i : sub) if (i == 2) throw std::runtime_error("request 2 is at fault");
  };
  std::vector<std::string> errs(4);
  long calls = 0, jobs = 0;
  Isolated({0, 1, 2, 3}, errs, calls, jobs, call);
  Report("isolated", made);
  CHECK((made == Log{"{0,1,2,3}", "{0}", "{1}", "{2}", "{3}"}));
  CHECK(errs[0].empty() && errs[1].empty() && errs[3].empty() && errs[2] == "request 2 is at fault");
  CHECK(calls == 3 && jobs == 3);                  // (a failed call is not counted)
  made.clear(); errs.assign(4, ""); calls = jobs = 0;
  Isolated({2}, errs, calls, jobs, call);           // a group of one: the error, and no second call
  CHECK((made == Log{"{2}"}) && errs[2] == "request 2 is at fault" && calls == 0 && jobs == 0);
  made.clear(); errs.assign(4, "");
  Isolated({0, 3}, errs, calls, jobs, call);
  CHECK((made == Log{"{0,3}"}) && errs[0].empty() && errs[3].empty() && calls == 1 && jobs == 2);
}

// 7. Groups
void GroupsOfEqualKey()
{
  const auto g = Groups(std::vector<char>{'a', 'b', 'a', 'c', 'b'});
  CHECK((g == std::vector<std::vector<size_t>>{{0, 2}, {1, 4}, {3}}));
  CHECK(Groups(std::vector<int>{}).empty());
}

// 8. a finished stream is not waited for, and an error leaves the stream usable
void FinishAndErrors()
{
  Rig r(3);
  std::string what;
  r.Stream(2, [] {});
  r.Stream(0, [&] {
    r.d->SubmitAndWait(0, LK);
    r.fail[0] = true;
    try { r.d->SubmitAndWait(0, PO); } catch (const std::runtime_error& e) { what = e.what(); }
    r.fail[0] = false;
    r.d->SubmitAndWait(0, PO);
  });
  r.Stream(1, [&] { r.d->SubmitAndWait(1, LK); });
  r.Join();
  Report("finish and errors", r.Log());
  CHECK((r.Log() == Log{"LK{0,1}", "PO{0}", "PO{0}"}));
  CHECK(what == "slot 0 is at fault");
  CHECK(r.d->counters(PO).calls == 1 && r.d->counters(PO).jobs == 1);
}

// 9. Slot(k): k for the bound thread, S + k for any other -- read by the other thread WHILE the stream's thread binds itself again
// (every front-end call does), which ThreadSanitizer must not object to
void SlotRule()
{
  Rig r(2);
  std::atomic<bool> stop{false};
  Latch bound;
  r.Stream(0, [&] {
    bound.Open();
    for (int i = 0; i < 20000; ++i) { r.d->Bind(0); CHECK(r.d->Slot(0) == 0); CHECK(r.d->Slot(1) == 3); }
    stop = true;
  });
  r.Stream(1, [] {});
  std::thread other([&] {
    bound.Wait();
    int n = 0;
    do { CHECK(r.d->Slot(0) == 2); ++n; } while (!stop);
    CHECK(n > 0);
  });
  other.join();
  r.Join();
}

// 10. teardown with idle dispatchers, nothing ever filed
void Teardown()
{
  { Rig r(1); }
  { Rig r(64); }
}

}  // namespace

int main()
{
  PoseOnlyFirst();
  EarliestStageFirst();
  LongOpHoldsTheKeyframePath();
  BackendSlotIsServedAnyway();
  NoEarlyServiceWithoutBackendRequest();
  IsolatedRetries();
  GroupsOfEqualKey();
  FinishAndErrors();
  SlotRule();
  Teardown();
  PoseOnlyFirst();                                  // (a fresh core after all that)
  if (g_failed) { std::printf("FAILED\n"); return 1; }
  std::printf("dispatch units: ok\n");
  return 0;
}
