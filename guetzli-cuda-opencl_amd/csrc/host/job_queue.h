// A bounded FIFO of jobs run by a fixed set of worker threads, with a result
// table that hands every result out exactly once: the queue under gz_encoder
// (capi.cc), which supplies the encode as the job function.  Nothing here
// knows about HIP or images (tests/native/job_queue_check.cc drives it with
// a function of its own).
//
//  - Submit: blocks while `capacity` accepted jobs have not started; ids
//    count from 1 in acceptance order, and jobs start in that order.
//  - Wait(id): blocks for that job's result.  Next(block): finished results
//    in completion order.  A result leaves through exactly one of them.
//  - Close (and the destructor): accepts nothing more, drops the jobs that
//    have not started, lets running ones finish, joins the workers; results
//    not collected are destroyed with the queue.
// All members may be called from any threads at once, except that Close and
// the destructor must not race with other calls.  `run` must not throw.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace gz {

template <class Job, class Result>
class JobQueue {
 public:
  struct Done {
    uint64_t id = 0;  // 0: no result
    double seconds_queued = 0.0;  // Submit -> a worker took it
    Result result{};
  };
  using Run = std::function<Result(const Job&)>;

  JobQueue(int workers, int capacity, Run run)
      : capacity_(static_cast<size_t>(capacity < 1 ? 1 : capacity)), run_(std::move(run)) {
    for (int i = 0; i < (workers < 1 ? 1 : workers); ++i) threads_.emplace_back([this] { Work(); });
  }
  ~JobQueue() { Close(); }
  JobQueue(const JobQueue&) = delete;
  JobQueue& operator=(const JobQueue&) = delete;

  // The job's id, or 0 once the queue is closed.
  uint64_t Submit(Job job) {
    std::unique_lock<std::mutex> lk(mu_);
    ++waiting_submitters_;
    not_full_.wait(lk, [&] { return closed_ || queue_.size() < capacity_; });
    --waiting_submitters_;
    if (closed_) return 0;
    const uint64_t id = ++last_id_;
    Entry& e = entries_[id];
    e.job = std::move(job);
    e.submitted = Clock::now();
    queue_.push_back(id);
    work_.notify_one();
    return id;
  }

  // False if the id is unknown or its result has been delivered (also when
  // another call takes it while this one waits, or Close drops the job).
  bool Wait(uint64_t id, Done* out) {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      auto it = entries_.find(id);
      if (it == entries_.end()) return false;
      if (it->second.state == kFinished) {
        Deliver(it, out);
        return true;
      }
      done_.wait(lk);
    }
  }

  // The next finished result in completion order.  False (out->id = 0) when
  // there is none: at once if !block, else once nothing is outstanding.
  bool Next(bool block, Done* out) {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      while (!finished_.empty()) {
        auto it = entries_.find(finished_.front());
        finished_.pop_front();
        if (it == entries_.end()) continue;  // went through Wait
        Deliver(it, out);
        return true;
      }
      if (!block || entries_.empty()) {
        *out = Done();
        return false;
      }
      done_.wait(lk);
    }
  }

  void Close() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (closed_) return;
      closed_ = true;
      for (uint64_t id : queue_) entries_.erase(id);
      queue_.clear();
    }
    work_.notify_all();
    not_full_.notify_all();
    done_.notify_all();
    for (auto& t : threads_) t.join();
  }

  // Observers (tests, diagnostics).
  size_t queued() const {
    std::lock_guard<std::mutex> lk(mu_);
    return queue_.size();
  }
  size_t outstanding() const {  // accepted, result not delivered
    std::lock_guard<std::mutex> lk(mu_);
    return entries_.size();
  }
  int waiting_submitters() const {  // threads inside Submit that hold no id yet
    std::lock_guard<std::mutex> lk(mu_);
    return waiting_submitters_;
  }

 private:
  using Clock = std::chrono::steady_clock;
  enum State { kQueued, kRunning, kFinished };
  struct Entry {
    Job job{};
    State state = kQueued;
    Clock::time_point submitted;
    double seconds_queued = 0.0;
    Result result{};
  };
  using Entries = std::map<uint64_t, Entry>;

  void Deliver(typename Entries::iterator it, Done* out) {
    out->id = it->first;
    out->seconds_queued = it->second.seconds_queued;
    out->result = std::move(it->second.result);
    entries_.erase(it);
    done_.notify_all();  // a blocking Next may have nothing left to wait for
  }

  void Work() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      work_.wait(lk, [&] { return closed_ || !queue_.empty(); });
      if (closed_) return;
      const uint64_t id = queue_.front();
      queue_.pop_front();
      Entry& e = entries_.find(id)->second;  // (std::map: stays put while others come and go)
      e.state = kRunning;
      e.seconds_queued = std::chrono::duration<double>(Clock::now() - e.submitted).count();
      not_full_.notify_one();
      lk.unlock();
      Result r = run_(e.job);
      lk.lock();
      e.result = std::move(r);
      e.job = Job();
      e.state = kFinished;
      finished_.push_back(id);
      done_.notify_all();
    }
  }

  const size_t capacity_;
  const Run run_;
  mutable std::mutex mu_;
  std::condition_variable not_full_, work_, done_;
  bool closed_ = false;
  uint64_t last_id_ = 0;
  int waiting_submitters_ = 0;
  std::deque<uint64_t> queue_;     // accepted, not started
  std::deque<uint64_t> finished_;  // completion order (ids Wait took are skipped)
  Entries entries_;                // every job whose result has not been delivered
  std::vector<std::thread> threads_;
};

}  // namespace gz
