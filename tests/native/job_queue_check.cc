// gz::JobQueue (host/job_queue.h) on its own: backpressure, FIFO start order,
// exactly-once delivery under concurrent submitters and waiters, Next with
// and without blocking, Close with queued jobs.  The job function blocks on
// gates this program opens, so every scenario is decided by the program's
// own steps (no sleeps); where it has to see another thread block, it polls
// the queue's observers.  Also built with -fsanitize=thread
// (tests/test_job_queue.py).
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "host/job_queue.h"

namespace {

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

std::atomic<int> g_live_results{0};

struct Result {
  int value = -1;
  Result() { ++g_live_results; }
  Result(const Result& o) : value(o.value) { ++g_live_results; }
  Result& operator=(const Result&) = default;
  ~Result() { --g_live_results; }
};

struct Job {
  int value = 0;
  int gate = -1;  // -1: runs through
};

// What the job function sees: gates it waits at, and the order jobs started.
struct World {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<int> permits;
  std::vector<int> started;  // job values, in start order

  explicit World(int gates) : permits(gates, 0) {}

  Result Run(const Job& job) {
    std::unique_lock<std::mutex> lk(mu);
    started.push_back(job.value);
    cv.notify_all();
    if (job.gate >= 0) {
      cv.wait(lk, [&] { return permits[job.gate] > 0; });
      --permits[job.gate];
    }
    Result r;
    r.value = 2 * job.value + 1;
    return r;
  }
  void Open(int gate, int n = 1) {
    std::lock_guard<std::mutex> lk(mu);
    permits[gate] += n;
    cv.notify_all();
  }
  void AwaitStarted(size_t n) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return started.size() >= n; });
  }
  std::vector<int> Started() {
    std::lock_guard<std::mutex> lk(mu);
    return started;
  }
};

using Queue = gz::JobQueue<Job, Result>;

std::unique_ptr<Queue> MakeQueue(World* w, int workers, int capacity) {
  return std::unique_ptr<Queue>(new Queue(workers, capacity, [w](const Job& j) { return w->Run(j); }));
}

template <class F>
void SpinUntil(F&& f) {
  while (!f()) std::this_thread::yield();
}

void Backpressure() {
  World w(1);
  auto q = MakeQueue(&w, 1, 2);
  CHECK(q->Submit({1, 0}) == 1);
  w.AwaitStarted(1);  // the worker holds job 1 at the gate
  CHECK(q->Submit({2, 0}) == 2);
  CHECK(q->Submit({3, 0}) == 3);
  CHECK(q->queued() == 2);
  std::atomic<uint64_t> fourth{0};
  std::thread t([&] { fourth = q->Submit({4, 0}); });
  SpinUntil([&] { return q->waiting_submitters() == 1; });
  // `capacity` jobs have not started: the submit stays blocked
  CHECK(fourth == 0 && q->queued() == 2 && w.Started().size() == 1);
  w.Open(0);  // job 1 ends, the worker takes job 2, and only then ...
  t.join();
  CHECK(fourth == 4);
  w.AwaitStarted(2);
  CHECK(w.Started()[1] == 2);
  w.Open(0, 3);
  for (uint64_t id = 1; id <= 4; ++id) {
    Queue::Done d;
    CHECK(q->Wait(id, &d) && d.id == id && d.result.value == 2 * static_cast<int>(id) + 1);
    CHECK(d.seconds_queued >= 0.0);
  }
  CHECK(q->outstanding() == 0);
}

void FifoStart() {
  {  // one worker: the start order is the submission order
    World w(1);
    auto q = MakeQueue(&w, 1, 64);
    for (int i = 1; i <= 40; ++i) CHECK(q->Submit({i, -1}) == static_cast<uint64_t>(i));
    Queue::Done d;
    for (int i = 1; i <= 40; ++i) CHECK(q->Next(true, &d) && d.id == static_cast<uint64_t>(i));
    const std::vector<int> s = w.Started();
    CHECK(s.size() == 40);
    for (int i = 0; i < 40; ++i) CHECK(s[i] == i + 1);
  }
  {  // three workers: the first three jobs start, the fourth when one ends
    World w(1);
    auto q = MakeQueue(&w, 3, 64);
    for (int i = 1; i <= 6; ++i) q->Submit({i, 0});
    w.AwaitStarted(3);
    std::vector<int> s = w.Started();
    CHECK(s.size() == 3 && s[0] + s[1] + s[2] == 6 && s[0] != s[1] && s[1] != s[2] && s[0] != s[2]);
    CHECK(q->queued() == 3);
    w.Open(0);
    w.AwaitStarted(4);
    CHECK(w.Started()[3] == 4);
    w.Open(0, 5);
    Queue::Done d;
    int n = 0;
    while (q->Next(true, &d)) ++n;
    CHECK(n == 6);
  }
}

void ExactlyOnce() {
  constexpr int kSubmitters = 4, kPer = 200, kTotal = kSubmitters * kPer, kWaiters = 3;
  World w(0);
  auto q = MakeQueue(&w, 3, 5);
  std::vector<std::atomic<int>> seen(kTotal + 1);
  for (auto& s : seen) s = 0;
  std::atomic<int> delivered{0};
  std::vector<int> value_of(kTotal + 1, 0);  // id -> job value (each id written once, read after join)
  auto take = [&](const Queue::Done& d) {
    CHECK(d.id >= 1 && d.id <= static_cast<uint64_t>(kTotal));
    ++seen[d.id];
    ++delivered;
  };
  std::vector<std::pair<uint64_t, int>> got[kSubmitters + kWaiters];
  std::vector<std::thread> threads;
  for (int s = 0; s < kSubmitters; ++s)
    threads.emplace_back([&, s] {
      for (int i = 0; i < kPer; ++i) {
        const int v = s * kPer + i;
        const uint64_t id = q->Submit({v, -1});
        CHECK(id != 0);
        value_of[id] = v;
        if (i % 4 == 0) {  // races with the waiters' Next: one of them gets it
          Queue::Done d;
          if (q->Wait(id, &d)) {
            CHECK(d.id == id);
            got[s].emplace_back(id, d.result.value);
            take(d);
          }
        }
      }
    });
  for (int k = 0; k < kWaiters; ++k)
    threads.emplace_back([&, k] {
      while (delivered < kTotal) {
        Queue::Done d;
        if (q->Next(true, &d)) {
          got[kSubmitters + k].emplace_back(d.id, d.result.value);
          take(d);
        } else {
          CHECK(d.id == 0);
          std::this_thread::yield();  // nothing outstanding right now
        }
      }
    });
  for (auto& t : threads) t.join();
  CHECK(delivered == kTotal);
  for (int id = 1; id <= kTotal; ++id) CHECK(seen[id] == 1);
  for (auto& g : got)
    for (auto& p : g) CHECK(p.second == 2 * value_of[p.first] + 1);
  CHECK(q->outstanding() == 0);
  Queue::Done d;
  CHECK(!q->Next(false, &d) && !q->Next(true, &d) && !q->Wait(1, &d) && !q->Wait(kTotal + 1, &d));
}

void NextSemantics() {
  World w(2);
  auto q = MakeQueue(&w, 2, 4);
  Queue::Done d;
  d.id = 99;
  CHECK(!q->Next(false, &d) && d.id == 0);
  d.id = 99;
  CHECK(!q->Next(true, &d) && d.id == 0);  // nothing outstanding: returns at once
  const uint64_t a = q->Submit({10, 0}), b = q->Submit({11, 1});
  w.AwaitStarted(2);
  CHECK(!q->Next(false, &d) && d.id == 0);  // running, not finished
  Queue::Done blocked;
  std::thread t([&] { CHECK(q->Next(true, &blocked)); });
  w.Open(1);  // b finishes first
  t.join();
  CHECK(blocked.id == b && blocked.result.value == 23);
  CHECK(!q->Wait(b, &d));  // delivered
  w.Open(0);
  CHECK(q->Wait(a, &d) && d.id == a && d.result.value == 21);
  CHECK(!q->Wait(a, &d) && !q->Wait(0, &d) && !q->Wait(77, &d));
  // completion order, not submission order
  const uint64_t c = q->Submit({12, 0}), e = q->Submit({13, 1});
  w.AwaitStarted(4);
  w.Open(1);
  SpinUntil([&] { return q->Next(false, &d); });
  CHECK(d.id == e);
  w.Open(0);
  CHECK(q->Next(true, &d) && d.id == c);
  CHECK(!q->Next(true, &d));
}

void CloseWithQueued() {
  const int before = g_live_results;
  {
    World w(1);
    auto q = MakeQueue(&w, 2, 4);
    for (int i = 1; i <= 6; ++i) CHECK(q->Submit({i, 0}) != 0);
    w.AwaitStarted(2);
    CHECK(q->queued() == 4 && q->outstanding() == 6);
    std::thread closer([&] { q->Close(); });
    SpinUntil([&] { return q->queued() == 0; });  // the queued jobs are dropped ...
    CHECK(q->outstanding() == 2);
    w.Open(0, 2);  // ... the running ones finish
    closer.join();
    CHECK(w.Started().size() == 2);
    CHECK(q->Submit({7, -1}) == 0);
    Queue::Done d;
    CHECK(!q->Wait(5, &d));          // dropped
    CHECK(q->Wait(1, &d) && d.id == 1);  // a finished result can still be collected
    CHECK(q->outstanding() == 1);    // the other one goes with the queue
  }
  CHECK(g_live_results == before);
  {  // the destructor alone: whatever has started finishes, the rest is dropped
    World w(0);
    auto q = MakeQueue(&w, 1, 8);
    for (int i = 1; i <= 5; ++i) q->Submit({i, -1});
    Queue::Done d;
    CHECK(q->Wait(2, &d));
    for (int i = 6; i <= 9; ++i) q->Submit({i, -1});
    q.reset();
    const std::vector<int> s = w.Started();
    CHECK(s.size() >= 2 && s.size() <= 9);
    for (size_t i = 0; i < s.size(); ++i) CHECK(s[i] == static_cast<int>(i) + 1);
  }
  CHECK(g_live_results == before);
}

}  // namespace

int main() {
  Backpressure();
  FifoStart();
  ExactlyOnce();
  NextSemantics();
  CloseWithQueued();
  std::puts("job_queue_check ok");
  return 0;
}
