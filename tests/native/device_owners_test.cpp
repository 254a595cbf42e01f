// Stand-alone test of the owners in csrc/device_job.h, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_device_owners_native.py) and WITHOUT the HIP runtime: the HIP entry points the header uses are
// defined here, as fakes over malloc / free that write every call into a log and fail on request.  So the order of the
// releases, and that each acquisition is released exactly once, can be read from the log on a machine without a
// device; a release the fakes do not know, a double release or a leak is a failure (the last also the sanitizer's).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <set>
#include <utility>
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
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return acquire(kStreamCreate, 2, (void**)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(kStreamDestroy, 2, s); }
hipError_t hipStreamSynchronize(hipStream_t s) {
  CHECK(g_live[2].count(s) == 1);
  g_log.push_back({kStreamSync, s, 0});
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return acquire(kEventCreate, 3, (void**)e, 1); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return acquire(kEventCreate, 3, (void**)e, 1); }
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

// 5: moves.  Construction and assignment, into an empty and into a held target: the target's old resource is released
// once and first, the source is left empty, and what moved is released once, by its new owner
static void* raw(const DeviceBuf<uint64_t>& o) { return o.p; }
static void* raw(const DeviceBuf<void>& o) { return o.p; }
static void* raw(const PinnedBuf<uint32_t>& o) { return o.p; }
static void* raw(const DeviceEvent& o) { return o.e; }
static void* raw(const DeviceStream& o) { return o.s; }
template <class Owner, class Make> static void move_one(Make make, Call put, size_t per_release) {
  fresh();
  {
    Owner a, b, held;
    CHECK(make(a) == hipSuccess && make(b) == hipSuccess && make(held) == hipSuccess);
    void *pa = raw(a), *pb = raw(b), *ph = raw(held);
    g_log.clear();
    Owner c(std::move(a));   // construction
    CHECK(raw(a) == nullptr && raw(c) == pa && g_log.empty());
    Owner d;
    d = std::move(b);        // assignment into an empty target
    CHECK(raw(b) == nullptr && raw(d) == pb && g_log.empty());
    held = std::move(c);     // ... into a held one: its own goes first, once
    CHECK(raw(c) == nullptr && raw(held) == pa && g_log.size() == per_release && g_log.back().call == put && g_log.back().p == ph);
    held = Owner();          // "release, then start from defaults"
    CHECK(raw(held) == nullptr && g_log.size() == 2 * per_release && g_log.back().p == pa);
    Owner& self = d;
    d = std::move(self);     // onto itself: nothing happens
    CHECK(raw(d) == pb && g_log.size() == 2 * per_release);
  }
  CHECK(count_of(put) == 3 && g_log.size() == 3 * per_release && nothing_live());
}
static void test_moves() {
  move_one<DeviceBuf<uint64_t>>([](DeviceBuf<uint64_t>& o) { return o.alloc(3); }, kFree, 1);
  move_one<DeviceBuf<void>>([](DeviceBuf<void>& o) { return o.alloc_bytes(40); }, kFree, 1);
  move_one<PinnedBuf<uint32_t>>([](PinnedBuf<uint32_t>& o) { return o.alloc(3); }, kHostFree, 1);
  move_one<DeviceEvent>([](DeviceEvent& o) { return o.create(hipEventDisableTiming); }, kEventDestroy, 1);
  move_one<DeviceStream>([](DeviceStream& o) { return o.create(hipStreamNonBlocking, -1); }, kStreamDestroy, 2);   // (wait, destroy)
  // an allocation in bytes asks for exactly those bytes, typed or not; both convert to their pointer
  fresh();
  {
    DeviceBuf<void> v;
    DeviceBuf<uint64_t> t;
    CHECK(v.alloc_bytes(100) == hipSuccess && t.alloc_bytes(20) == hipSuccess);
    CHECK(g_log[0].bytes == 100 && g_log[1].bytes == 20);
    void* pv = v;
    uint64_t* pt = t;
    CHECK(pv == v.p && pt == t.p && (uint32_t*)v == (uint32_t*)v.p && t + 1 == t.p + 1);
  }
  CHECK(nothing_live());
  // a vector of owners grown twice by resize, a reset() in between: each buffer is released once
  fresh();
  {
    std::vector<DeviceBuf<uint32_t>> slots;
    std::multiset<void*> got;
    slots.resize(2);
    for (auto& b : slots) { CHECK(b.alloc(4) == hipSuccess); got.insert(b.p); }
    void* p0 = slots[0].p;
    slots[0].reset();
    CHECK(slots[0].p == nullptr && g_log.back().call == kFree && g_log.back().p == p0);
    slots.resize(5);    // (reallocates: the elements move)
    CHECK(slots[0].p == nullptr && slots[1].p != nullptr && count_of(kFree) == 1);
    CHECK(slots[0].alloc(4) == hipSuccess && slots[4].alloc(4) == hipSuccess);
    got.insert(slots[0].p);
    got.insert(slots[4].p);
    slots.resize(64);
    CHECK(count_of(kFree) == 1 && slots[4].p != nullptr && slots[63].p == nullptr);
    slots.clear();
    std::multiset<void*> released;
    for (const Rec& r : g_log)
      if (r.call == kFree) released.insert(r.p);
    CHECK(released == got && got.size() == 4);
  }
  CHECK(nothing_live());
}

// 6: a composite shaped like an MSM lane -- buffers, a pinned block, events, and its stream LAST -- created in the
// lane's order (the stream in the middle), and reset by move-assigning a default-constructed one over it
struct Lane {
  PinnedBuf<uint32_t> h_stat;
  DeviceBuf<uint32_t> d_off;
  DeviceBuf<void> d_partial;
  DeviceEvent ev_fork, ev_join;
  PinnedBuf<uint8_t> h_pinned;
  DeviceEvent ev0, ev_done;
  DeviceStream st_dup;
  Lane() = default;
  Lane(Lane&&) = default;
  // a composite that is reassigned releases in its destructor's order, the stream first: memberwise assignment would
  // free the buffers first (MsmLaneWs, which nothing assigns, declares no assignment of its own)
  Lane& operator=(Lane&& o) noexcept {
    if (this != &o) { this->~Lane(); new (this) Lane(std::move(o)); }
    return *this;
  }
};
constexpr int kLaneAcquisitions = 9;
static hipError_t lane_fill(Lane& ln) {
  hipError_t e;
  if ((e = ln.h_stat.alloc_bytes(64)) != hipSuccess || (e = ln.d_off.alloc_bytes(5 * 4)) != hipSuccess ||
      (e = ln.d_partial.alloc_bytes(300)) != hipSuccess || (e = ln.st_dup.create(hipStreamNonBlocking, -1)) != hipSuccess ||
      (e = ln.ev_fork.create(hipEventDisableTiming)) != hipSuccess || (e = ln.ev_join.create(hipEventDisableTiming)) != hipSuccess ||
      (e = ln.h_pinned.alloc_bytes(256)) != hipSuccess || (e = ln.ev0.create()) != hipSuccess || (e = ln.ev_done.create()) != hipSuccess)
    return e;
  return hipSuccess;
}
static void check_lane_release(const std::vector<void*>& got, bool had_stream) {
  std::multiset<void*> released;
  size_t first_free = g_log.size(), stream_gone = 0;
  for (size_t i = 0; i < g_log.size(); i++) {
    const Rec& r = g_log[i];
    CHECK(is_release(r.call) || r.call == kStreamSync);
    if (is_release(r.call)) released.insert(r.p);
    if (r.call == kStreamDestroy) stream_gone = i;
    if (r.call != kStreamSync && r.call != kStreamDestroy && i < first_free) first_free = i;
  }
  CHECK(released == std::multiset<void*>(got.begin(), got.end()));
  CHECK(count_of(kStreamSync) == (had_stream ? 1u : 0u) && count_of(kStreamDestroy) == (had_stream ? 1u : 0u));
  if (had_stream) CHECK(g_log[0].call == kStreamSync && stream_gone == 1 && first_free == 2);   // waited for and gone before any free
  CHECK(nothing_live());
}
static void test_lane_composite() {
  fresh();
  std::vector<void*> got;
  {
    Lane ln;
    CHECK(lane_fill(ln) == hipSuccess && g_acquired == kLaneAcquisitions);
    for (const Rec& r : g_log) got.push_back(r.p);
    CHECK(ln.ev_fork.record(ln.st_dup) == hipSuccess);
    g_log.clear();
    ln = Lane();   // the reset
    CHECK(ln.st_dup.s == nullptr && ln.d_partial.p == nullptr && ln.h_pinned.p == nullptr && ln.ev_done.e == nullptr);
    check_lane_release(got, true);
    g_log.clear();
  }
  CHECK(g_log.empty());   // (nothing left for the destructor)
  // the k-th acquisition of the create fails: what came before is held once and released once, the rest is null
  for (int k = 0; k < kLaneAcquisitions; k++) {
    fresh(k);
    got.clear();
    {
      Lane ln;
      CHECK(lane_fill(ln) == hipErrorOutOfMemory && g_acquired == k + 1 && g_log.size() == (size_t)k);
      for (const Rec& r : g_log) got.push_back(r.p);
      const void* held[kLaneAcquisitions] = {ln.h_stat.p, ln.d_off.p, ln.d_partial.p, ln.st_dup.s, ln.ev_fork.e, ln.ev_join.e,
                                             ln.h_pinned.p, ln.ev0.e, ln.ev_done.e};
      for (int j = 0; j < kLaneAcquisitions; j++) CHECK(j < k ? held[j] == got[j] : held[j] == nullptr);
      CHECK(std::set<void*>(got.begin(), got.end()).size() == got.size());   // (nothing held twice)
      g_log.clear();
    }
    check_lane_release(got, k > 3);
  }
}

int main() {
  test_scope_order();
  test_every_failure();
  test_growth_and_upload();
  test_drain_and_timer();
  test_moves();
  test_lane_composite();
  CHECK(require_hip_device("route", 1) == G16_E_ARG && g_err == "route: bad device ordinal");
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
