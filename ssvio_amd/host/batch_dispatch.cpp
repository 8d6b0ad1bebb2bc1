// ssvio_amd/host/batch_dispatch.cpp -- see batch_dispatch.hpp
#include "batch_dispatch.hpp"

#include <algorithm>
#include <chrono>
#include <stdexcept>

namespace ssx::host {

void Isolated(const std::vector<size_t>& idx, std::vector<std::string>& errs, long& calls, long& jobs, const std::function<void(const std::vector<size_t>&)>& call)
{
  try {
    call(idx);
    ++calls; jobs += (long)idx.size();
    return;
  } catch (const std::exception& e) {
    if (idx.size() == 1) { errs[idx[0]] = e.what(); return; }
  }
  for (size_t i : idx) {
    try { call(std::vector<size_t>{i}); ++calls; ++jobs; } catch (const std::exception& e) { errs[i] = e.what(); }
  }
}

std::vector<PoseCall> PackPoseCalls(const std::vector<int>& n_jobs, const std::vector<std::vector<size_t>>& groups, int max_jobs)
{
  std::vector<PoseCall> calls;
  if (max_jobs < 1) throw std::invalid_argument("PackPoseCalls: a call holds at least one job");
  for (const std::vector<size_t>& g : groups) {
    int room = 0;                                   // (every group begins a call of its own)
    for (size_t r : g)
      for (int first = 0; first < n_jobs.at(r);) {
        if (room == 0) { calls.emplace_back(); room = max_jobs; }
        const int count = std::min(n_jobs[r] - first, room);
        calls.back().push_back(PosePart{r, first, count});
        first += count; room -= count;
      }
  }
  return calls;
}

BatchDispatch::BatchDispatch(int streams, std::vector<Kind> kinds, Dispatcher frame, Dispatcher keyframe)
    : S_(streams), kinds_(std::move(kinds)), disp_{std::move(frame), std::move(keyframe)}, bound_(new Bound[(size_t)streams]),
      state_(2 * (size_t)streams, RUNNING), n_in_(PENDING + kinds_.size(), 0), error_(2 * (size_t)streams), count_(kinds_.size())
{
  n_in_[RUNNING] = n_in_[IDLE] = S_;
  for (int k = 0; k < S_; ++k) { state_[(size_t)S_ + k] = IDLE; Bind(k); }
  for (int k = 0; k < 2 * S_; ++k) sleeper_.push_back(std::make_unique<Sleeper>());
  thread_[0] = std::thread([this] { Loop(disp_[0], true); });
  thread_[1] = std::thread([this] { Loop(disp_[1], false); });
}

BatchDispatch::~BatchDispatch()
{
  {
    std::lock_guard<std::mutex> lk(m_);
    quit_ = true;
  }
  cv_.notify_all();
  for (std::thread& t : thread_) if (t.joinable()) t.join();
}

// (m_ held) -- the dispatchers' conditions can only BECOME true when the last running stream stops running: they are woken then,
// not at every one of the S state changes of a round
bool BatchDispatch::Move(int slot, int state)
{
  --n_in_[state_[slot]]; ++n_in_[state];
  state_[slot] = state;
  return n_in_[RUNNING] == 0;
}

void BatchDispatch::SetState(int slot, int state)
{
  bool wake;
  {
    std::lock_guard<std::mutex> lk(m_);
    wake = Move(slot, state);
  }
  if (wake) cv_.notify_all();
}

// Every thread sleeps on a condition variable of its own: S streams woken through one shared mutex queue up behind each other (64
// wake-ups x a futex round trip each: more than the batched call they waited for).
void BatchDispatch::SubmitAndWait(int slot, int kind)
{
  bool wake;
  {
    std::lock_guard<std::mutex> lk(m_);
    error_[slot].clear();
    wake = Move(slot, PENDING + kind);
  }
  if (wake) cv_.notify_all();
  Sleeper& sl = *sleeper_[slot];
  std::unique_lock<std::mutex> lk(sl.mu);
  sl.cv.wait(lk, [&] { return sl.done; });
  sl.done = false;
  if (!error_[slot].empty()) throw std::runtime_error(error_[slot]);
}

void BatchDispatch::Loop(const Dispatcher& d, bool counts_wait)
{
  using clk = std::chrono::steady_clock;
  const int n_slots = d.backend_slots ? 2 * S_ : S_;
  auto first_pending = [&] { for (int kind : d.kinds) if (n_in_[PENDING + kind] > 0) return kind; return -1; };
  auto rested = [&] { return quit_ || (first_pending() >= 0 && n_in_[RUNNING] == 0 && !(d.waits_for_longop && n_in_[LONGOP] > 0)); };
  std::unique_lock<std::mutex> lk(m_);
  std::vector<int> who;
  for (;;) {
    const auto tw0 = clk::now();
    bool at_rest = true;
    if (d.waits_for_longop) at_rest = cv_.wait_for(lk, std::chrono::milliseconds(2), rested); else cv_.wait(lk, rested);
    if (quit_) return;
    if (!at_rest) {
      bool backend_waits = false;
      for (int k = S_; k < n_slots; ++k) backend_waits = backend_waits || state_[k] >= PENDING;
      if (!backend_waits || first_pending() < 0) continue;
    }
    if (counts_wait) wait_s_ += std::chrono::duration<double>(clk::now() - tw0).count();
    const int kind = first_pending();
    who.clear();
    for (int k = 0; k < n_slots; ++k) if (state_[k] == PENDING + kind) { who.push_back(k); Move(k, INFLIGHT); }
    lk.unlock();
    if (d.waits_for_longop) cv_.notify_all();
    std::vector<std::string> errs(who.size());
    long calls = 0, jobs = 0;
    const auto tc0 = clk::now();
    kinds_[kind].serve(who, errs, calls, jobs);
    const double dt = std::chrono::duration<double>(clk::now() - tc0).count();
    lk.lock();
    count_[kind].calls += calls; count_[kind].jobs += jobs; count_[kind].seconds += dt;
    // the threads of a finished batch run again
    for (size_t i = 0; i < who.size(); ++i) { error_[who[i]] = errs[i]; Move(who[i], who[i] < S_ ? RUNNING : IDLE); }
    lk.unlock();
    for (int k : who) {
      Sleeper& sl = *sleeper_[k];
      { std::lock_guard<std::mutex> g(sl.mu); sl.done = true; }
      sl.cv.notify_one();
    }
    lk.lock();
  }
}

}  // namespace ssx::host
