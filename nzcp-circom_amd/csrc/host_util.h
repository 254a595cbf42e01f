// Small host helpers the routes share: the wall clock of the trace lines, the owner of a buffer that came back from a
// C-ABI call, and the thread splitter.  Standard library only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <chrono>
#include <memory>
#include <thread>
#include <vector>

namespace g16 {

inline double ms_since(const std::chrono::steady_clock::time_point& t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// an image a C-ABI call handed out (g16_free's contract: malloc'd), freed unless release()d to the next caller
struct FreeImage { void operator()(uint8_t* p) const { free(p); } };
using MallocPtr = std::unique_ptr<uint8_t, FreeImage>;

// host threads for n items: one below `single_below` items, else the machine's, at most 16
inline int host_threads(size_t n, size_t single_below = 2) {
  const unsigned hw = std::thread::hardware_concurrency();
  return n < single_below ? 1 : (int)(hw < 1 ? 1 : hw > 16 ? 16 : hw);
}

// fn(lo, hi) over [0, n) cut into `threads` even ranges, each on a thread of its own
template <class Fn> void parallel_for(size_t n, int threads, Fn fn) {
  if (threads < 1) threads = 1;
  if ((size_t)threads > n) threads = n ? (int)n : 1;
  std::vector<std::thread> th;
  const size_t chunk = (n + threads - 1) / threads;
  for (int t = 0; t < threads; t++) {
    const size_t lo = (size_t)t * chunk, hi = lo + chunk < n ? lo + chunk : n;
    if (lo >= hi) break;
    th.emplace_back([=]() { fn(lo, hi); });
  }
  for (auto& x : th) x.join();
}

}  // namespace g16
