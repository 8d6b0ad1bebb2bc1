// ssvio_amd/host/batch_dispatch.hpp -- the synchronisation protocol of the stream batcher (stream_batcher.hpp), without the GPU:
// who is waited for, what is served first, error isolation and wake-ups.  It knows no library call: a request KIND is a name and one
// callable, and tests/host/test_dispatch_units.cpp drives it with fakes, under ThreadSanitizer too.
//
// S streams, 2 S request slots: slot k < S is stream k's own thread (one request at a time); slot S + k is any other thread that
// files for stream k -- the worker of its asynchronous backend, which solves windows while the stream's thread goes on tracking.
// A backend slot rests IDLE, which no dispatcher waits for.  A thread files a request (SubmitAndWait) and sleeps; a dispatcher
// thread waits until its streams have come to rest, takes ALL pending requests of the first kind of its list that has any, and hands
// their slots to the kind's callable in one go; then the slots' threads run again.
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace ssx::host {

// One call for the requests idx (positions in a dispatch's slots).  If it throws, every request goes once more in a call of its own:
// only the request at fault gets the error text, the others get their results (the library validates a job table before it touches
// anything, so a rejected call has not run any of its jobs).  calls / jobs count the calls that did not throw.
void Isolated(const std::vector<size_t>& idx, std::vector<std::string>& errs, long& calls, long& jobs, const std::function<void(const std::vector<size_t>&)>& call);

// positions 0 .. keys.size() in groups of equal key (image size, extractor settings ...), in order of first appearance
template <class Key>
std::vector<std::vector<size_t>> Groups(const std::vector<Key>& keys)
{
  std::vector<std::vector<size_t>> g;
  std::vector<char> taken(keys.size(), 0);
  for (size_t a = 0; a < keys.size(); ++a) {
    if (taken[a]) continue;
    g.emplace_back();
    for (size_t b = a; b < keys.size(); ++b) if (!taken[b] && keys[a] == keys[b]) { g.back().push_back(b); taken[b] = 1; }
  }
  return g;
}

// The pose jobs of a dispatch's requests (the candidates of every stream that lost tracking) packed into calls of at most max_jobs jobs:
// a call is a list of (request, first job, count).  The requests of one group (equal key: the intrinsics a call's jobs share) fill calls
// in the order they stand in, a request that does not fit is cut, and a request without jobs takes no part; the groups follow each other
// in order of first appearance.  The library makes every job independent of its place in a call, so packing changes no bits.
struct PosePart {
  size_t request; int first, count;
  bool operator==(const PosePart& o) const { return request == o.request && first == o.first && count == o.count; }
};
using PoseCall = std::vector<PosePart>;
std::vector<PoseCall> PackPoseCalls(const std::vector<int>& n_jobs, const std::vector<std::vector<size_t>>& groups, int max_jobs);
template <class Key>
std::vector<PoseCall> PackPoseCalls(const std::vector<int>& n_jobs, const std::vector<Key>& keys, int max_jobs) { return PackPoseCalls(n_jobs, Groups(keys), max_jobs); }

class BatchDispatch {
 public:
  // serve(slots, errs, calls, jobs): the requests of `slots` (ascending), all of this kind; errs[i] is what the thread of slots[i]
  // is to throw (empty: nothing); calls / jobs: the library calls made and the jobs in them.  Called without the core's lock.
  struct Kind {
    std::string name;
    std::function<void(const std::vector<int>& slots, std::vector<std::string>& errs, long& calls, long& jobs)> serve;
  };
  struct Dispatcher {
    std::vector<int> kinds;                         // indices into the kind table, in priority order
    bool backend_slots;                             // it looks at the slots 0 .. 2 S, not 0 .. S
    // Rest is "no slot is running and one of my kinds is pending"; with this flag also "no slot is in a LongOp" (a stream in a call of
    // its own is about to file the next request of this dispatcher's path).  Such a dispatcher serves after 2 ms all the same if a
    // backend slot has a request pending (the streams' threads may be waiting for THAT: Backend::WaitIdle, the map mutex), and it
    // notifies the other dispatcher when it has taken its slots.
    bool waits_for_longop;
  };
  struct Counters { long calls = 0, jobs = 0; double seconds = 0; };   // seconds: inside the kind's callable

  // two dispatcher threads: `frame` (its wait for rest is wait_s) and `keyframe`
  BatchDispatch(int streams, std::vector<Kind> kinds, Dispatcher frame, Dispatcher keyframe);
  ~BatchDispatch();
  BatchDispatch(const BatchDispatch&) = delete;
  BatchDispatch& operator=(const BatchDispatch&) = delete;

  int streams() const { return S_; }
  // The calling thread is stream k's thread from now on; Slot(k) is k for that thread and S + k for any other.
  void Bind(int k) { bound_[k].id.store(std::this_thread::get_id(), std::memory_order_relaxed); }
  int Slot(int k) const { return std::this_thread::get_id() == bound_[k].id.load(std::memory_order_relaxed) ? k : S_ + k; }

  // the calling thread sleeps until a dispatcher has served its request; throws std::runtime_error with what the callable reported
  void SubmitAndWait(int slot, int kind);
  // a call that stream k makes on its own (a keyframe's path): not running, not waiting for a dispatcher
  struct LongOp {
    LongOp(BatchDispatch& d, int k) : d_(d), k_(k) { d_.SetState(k_, LONGOP); }
    ~LongOp() { d_.SetState(k_, RUNNING); }
    LongOp(const LongOp&) = delete;
    BatchDispatch& d_; int k_;
  };
  void Finish(int k) { SetState(k, DONE); }         // stream k has run its last frame (or died): nobody waits for it any more

  Counters counters(int kind) { std::lock_guard<std::mutex> lk(m_); return count_[kind]; }
  double wait_s() { std::lock_guard<std::mutex> lk(m_); return wait_s_; }
  void ResetCounters() { std::lock_guard<std::mutex> lk(m_); count_.assign(count_.size(), Counters{}); wait_s_ = 0; }

 private:
  enum { RUNNING, LONGOP, INFLIGHT, DONE, IDLE, PENDING };   // a slot's state; PENDING + i: a request of kind i waits for its dispatcher
  bool Move(int slot, int state);
  void SetState(int slot, int state);
  void Loop(const Dispatcher& d, bool counts_wait);

  const int S_;
  const std::vector<Kind> kinds_;
  const Dispatcher disp_[2];
  // (a stream's thread writes its id at every front-end call: a cache line each, so that the streams do not write into each other's)
  struct alignas(64) Bound { std::atomic<std::thread::id> id; };
  std::unique_ptr<Bound[]> bound_;
  std::mutex m_;                                    // everything below but the sleepers
  std::condition_variable cv_;                      // the dispatchers
  struct Sleeper { std::mutex mu; std::condition_variable cv; bool done = false; };
  std::vector<std::unique_ptr<Sleeper>> sleeper_;
  std::vector<int> state_, n_in_;                   // per slot; slots per state
  std::vector<std::string> error_;
  std::vector<Counters> count_;
  double wait_s_ = 0;
  bool quit_ = false;
  std::thread thread_[2];
};

}  // namespace ssx::host
