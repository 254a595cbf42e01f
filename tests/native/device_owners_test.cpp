// Stand-alone test of the owners in csrc/device_job.h, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_device_owners_native.py) and WITHOUT the HIP runtime: the HIP entry points the header uses are
// defined here, as fakes over malloc / free that write every call into a log and fail on request.  So the order of the
// releases, and that each acquisition is released exactly once, can be read from the log on a machine without a
// device; a release the fakes do not know, a double release or a leak is a failure (the last also the sanitizer's).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "device_job.h"

static std::string g_err;
namespace g16 {
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace g16
using namespace g16;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

// ---------------------------------------------------------------- the fakes
enum Call { kMalloc, kFree, kHostMalloc, kHostFree, kStreamCreate, kStreamSync, kStreamDestroy, kEventCreate, kEventDestroy, kMemcpy };
struct Rec { Call call; void* p; size_t bytes; };
static std::vector<Rec> g_log;
static std::set<void*> g_live[4];   // device, pinned, streams, events
static int g_acquired = 0;          // acquisitions asked for so far
static int g_fail_at = -1;          // the acquisition (counted from 0) that fails; -1: none
static bool g_elapsed_fails = false;

static hipError_t acquire(Call call, int kind, void** out, size_t bytes) {
  if (g_acquired++ == g_fail_at) {
    *out = (void*)(uintptr_t)0xbad0;   // (a failing call may leave anything there: the owner must not keep it)
    return hipErrorOutOfMemory;
  }
  *out = malloc(bytes ? bytes : 1);
  g_live[kind].insert(*out);
  g_log.push_back({call, *out, bytes});
  return hipSuccess;
}
static hipError_t release(Call call, int kind, void* p) {
  g_log.push_back({call, p, 0});
  if (!g_live[kind].erase(p)) { printf("FAIL: call %d releases %p, which is not held\n", (int)call, p); g_fail++; return hipErrorInvalidValue; }
  free(p);
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return acquire(kMalloc, 0, p, n); }
hipError_t hipFree(void* p) { return release(kFree, 0, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return acquire(kHostMalloc, 1, p, n); }
hipError_t hipHostFree(void* p) { return release(kHostFree, 1, p); }
hipError_t hipStreamCreate(hipStream_t* s) { return acquire(kStreamCreate, 2, (void**)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(kStreamDestroy, 2, s); }
hipError_t hipStreamSynchronize(hipStream_t s) {
  CHECK(g_live[2].count(s) == 1);
  g_log.push_back({kStreamSync, s, 0});
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return acquire(kEventCreate, 3, (void**)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(kEventDestroy, 3, e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  CHECK(g_live[3].count(e) == 1 && g_live[2].count(s) == 1);
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  CHECK(g_live[3].count(a) == 1 && g_live[3].count(b) == 1);
  *ms = 7.f;   // (written also when the call fails: ms() must not pass it on)
  return g_elapsed_fails ? hipErrorNotReady : hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) {
  memcpy(dst, src, n);   // (past the allocation: the sanitizer's)
  g_log.push_back({kMemcpy, dst, n});
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake"; }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
}

static void fresh(int fail_at = -1) {
  g_log.clear();
  g_acquired = 0;
  g_fail_at = fail_at;
}
static size_t count_of(Call c) {
  size_t n = 0;
  for (const Rec& r : g_log) n += r.call == c;
  return n;
}
static bool nothing_live() { return g_live[0].empty() && g_live[1].empty() && g_live[2].empty() && g_live[3].empty(); }

// ---------------------------------------------------------------- a handle laid out by THE RULE
struct Handle {
  DeviceBuf<uint64_t> d_a, d_b;
  PinnedBuf<uint32_t> h_out;
  PhaseEvents<2> ev;
  DeviceEvent ready;
  DeviceStream st;
};
constexpr int kAcquisitions = 8;   // two device buffers, one pinned, three events and one more, the stream
static hipError_t fill(Handle& h) {
  hipError_t e;
  if ((e = h.st.create()) != hipSuccess || (e = h.ev.create()) != hipSuccess || (e = h.d_a.alloc(5)) != hipSuccess ||
      (e = h.h_out.alloc(3)) != hipSuccess || (e = h.d_b.alloc(9)) != hipSuccess || (e = h.ready.create()) != hipSuccess)
    return e;
  return hipSuccess;
}
static bool is_release(Call c) { return c == kFree || c == kHostFree || c == kStreamDestroy || c == kEventDestroy; }

// 1: out of scope = one wait, the stream destroyed, then the frees; every acquisition released once
static void test_scope_order() {
  fresh();
  std::vector<void*> got;
  {
    Handle h;
    CHECK(fill(h) == hipSuccess);
    CHECK(g_acquired == kAcquisitions && g_log.size() == (size_t)kAcquisitions);
    for (const Rec& r : g_log) got.push_back(r.p);
    CHECK(h.ev.record(0, h.st) == hipSuccess && h.ev.record(2, h.st) == hipSuccess && h.ready.record(h.st) == hipSuccess);
    g_log.clear();
  }
  CHECK(g_log.size() == (size_t)kAcquisitions + 1);
  CHECK(g_log.size() > 2 && g_log[0].call == kStreamSync && g_log[1].call == kStreamDestroy && g_log[0].p == g_log[1].p);
  CHECK(count_of(kStreamSync) == 1 && count_of(kStreamDestroy) == 1 && count_of(kFree) == 2 && count_of(kHostFree) == 1 &&
        count_of(kEventDestroy) == 4);
  std::multiset<void*> released;
  for (const Rec& r : g_log)
    if (is_release(r.call)) released.insert(r.p);
  CHECK(released == std::multiset<void*>(got.begin(), got.end()));   // (each once: a second release is not in `got` twice)
  CHECK(nothing_live());
}

// 2: the k-th acquisition fails: what came before it is released once, nothing else, the failing owner holds null
static void test_every_failure() {
  for (int k = 0; k < kAcquisitions; k++) {
    fresh(k);
    std::vector<void*> got;
    {
      Handle h;
      CHECK(fill(h) == hipErrorOutOfMemory);
      CHECK(g_acquired == k + 1 && g_log.size() == (size_t)k);
      for (const Rec& r : g_log) got.push_back(r.p);
      // the order of fill(): stream, events 0 1 2, d_a, h_out, d_b, ready
      const void* held[kAcquisitions] = {h.st.s, h.ev.e[0], h.ev.e[1], h.ev.e[2], h.d_a.p, h.h_out.p, h.d_b.p, h.ready.e};
      for (int j = 0; j < kAcquisitions; j++) CHECK(j < k ? held[j] == got[j] : held[j] == nullptr);
      g_log.clear();
    }
    std::multiset<void*> released;
    for (const Rec& r : g_log) {
      CHECK(is_release(r.call) || r.call == kStreamSync);
      if (is_release(r.call)) released.insert(r.p);
    }
    CHECK(released == std::multiset<void*>(got.begin(), got.end()));
    CHECK(count_of(kStreamSync) == (k > 0 ? 1u : 0u));   // (no stream, no wait)
    CHECK(nothing_live());
  }
}

// 3: growing frees the old block before it asks for the new one; a count of 0 still allocates an element
template <class Buf> static void grow_one(Call get, Call put) {
  fresh();
  {
    Buf b;
    CHECK(b.alloc(4) == hipSuccess);
    void* p0 = b.p;
    CHECK(b.alloc(8) == hipSuccess);
    CHECK(g_log.size() == 3 && g_log[0].call == get && g_log[1].call == put && g_log[1].p == p0 && g_log[2].call == get);
    CHECK(g_log[0].bytes == 4 * sizeof(*b.p) && g_log[2].bytes == 8 * sizeof(*b.p));
    CHECK(b.alloc(0) == hipSuccess);
    CHECK(b.p != nullptr && g_log.back().call == get && g_log.back().bytes >= sizeof(*b.p));
    g_fail_at = g_acquired;   // a growth that fails: the old block is gone, the owner holds null, nothing is freed twice
    CHECK(b.alloc(16) == hipErrorOutOfMemory && b.p == nullptr);
  }
  CHECK(count_of(get) == 3 && count_of(put) == 3 && nothing_live());
}
static void test_growth_and_upload() {
  grow_one<DeviceBuf<uint64_t>>(kMalloc, kFree);
  grow_one<PinnedBuf<uint32_t>>(kHostMalloc, kHostFree);
  fresh();
  {
    DeviceBuf<uint32_t> b;
    const std::vector<uint32_t> src = {1, 2, 3};
    CHECK(upload(b, src) == hipSuccess);   // one element more than the vector
    CHECK(g_log.size() == 2 && g_log[0].bytes == 4 * sizeof(uint32_t) && g_log[1].call == kMemcpy && g_log[1].bytes == 3 * sizeof(uint32_t));
    CHECK(memcmp(b.p, src.data(), 12) == 0);
    CHECK(upload(b, std::vector<uint32_t>()) == hipSuccess);   // an empty one: an address, no copy
    CHECK(b.p != nullptr && g_log.back().call == kMalloc && g_log.back().bytes == sizeof(uint32_t));
  }
  CHECK(nothing_live());
}

// 4: the drain guard waits once on an early exit, not at all once dismissed; an unreadable time is 0
static int early(hipStream_t st, bool leave) {
  StreamDrain drain(st);
  if (leave) return 1;
  CHECK(hipStreamSynchronize(st) == hipSuccess);   // the scope's own wait
  drain.dismiss();
  return 0;
}
static void test_drain_and_timer() {
  fresh();
  {
    PhaseEvents<1> ev;
    DeviceStream st;
    CHECK(st.create() == hipSuccess && ev.create() == hipSuccess);
    g_log.clear();
    CHECK(early(st, true) == 1);
    CHECK(g_log.size() == 1 && g_log[0].call == kStreamSync && g_log[0].p == st.s);
    g_log.clear();
    CHECK(early(st, false) == 0);
    CHECK(g_log.size() == 1);   // its own, none from the guard
    CHECK(ev.ms(0) == 7.f);
    g_elapsed_fails = true;
    CHECK(ev.ms(0) == 0.f);
    g_elapsed_fails = false;
  }
  CHECK(nothing_live());
}

int main() {
  test_scope_order();
  test_every_failure();
  test_growth_and_upload();
  test_drain_and_timer();
  CHECK(require_hip_device("route", 1) == G16_E_ARG && g_err == "route: bad device ordinal");
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
