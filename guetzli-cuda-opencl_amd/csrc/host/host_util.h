// Small helpers of the host code: wall / thread-CPU timers and the
// environment knobs.
#pragma once

#include <stdint.h>
#include <time.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

namespace gz {

using Clock = std::chrono::steady_clock;
inline double Since(Clock::time_point t0) {
  return std::chrono::duration<double>(Clock::now() - t0).count();
}
// CPU seconds of the calling thread (host-cost accounting in the detail map)
inline double ThreadCpu() {
  timespec ts;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
  return static_cast<double>(ts.tv_sec) + 1e-9 * static_cast<double>(ts.tv_nsec);
}

inline int Log2FloorNonZero(uint32_t n) { return 31 ^ __builtin_clz(n); }

// The environment knobs (tests and A/B runs).  Callers keep the result in a
// function-local static: a knob is parsed once per process.
// EnvInt: the value when it is set to a positive integer, else fallback.
inline int EnvInt(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e && std::atoi(e) > 0 ? std::atoi(e) : fallback;
}
// EnvFlag: set to a non-zero integer.
inline bool EnvFlag(const char* name) {
  const char* e = std::getenv(name);
  return e && std::atoi(e) != 0;
}
// EnvIs: set to exactly this word.
inline bool EnvIs(const char* name, const char* word) {
  const char* e = std::getenv(name);
  return e && std::strcmp(e, word) == 0;
}

}  // namespace gz
