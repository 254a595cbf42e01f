// What device code's host side owns: device and pinned buffers, its stream, its timing events, its status.
// THE RULE, for every one-shot route: whatever work on the stream reads or writes -- a DeviceBuf, a NttTables, a
// MsmGroup and its workspace -- is declared AHEAD of the DeviceStream.  Destructors run in reverse order, the stream's
// waits for its work and then destroys it, so the stream has drained before anything is freed, on every path out of the
// route.
// ... and for every long-lived handle (a verifier, a witness checker or calculator): the members that work on its stream
// touches -- DeviceBuf, PinnedBuf, PhaseEvents -- come BEFORE its DeviceStream member, and the handle's destructor body
// does hipSetDevice(device) and nothing else: the members release themselves, the stream first.  A batch entry holds a
// StreamDrain from its first enqueue to its own successful wait, so that no failing call returns while the stream still
// reads or writes the caller's memory, or a temporary of the entry's.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/g16_prover.h"

namespace g16 {

void set_error(const std::string& msg);

// ---------------------------------------------------------------- the device check
inline int hip_device_rc(int device) {   // G16_OK, G16_E_NOGPU or G16_E_ARG; no text
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_E_NOGPU;
  return device < 0 || device >= ndev ? G16_E_ARG : G16_OK;
}
// ... with the caller's two texts
inline int require_hip_device(int device, const std::string& no_device, const std::string& bad_ordinal) {
  const int rc = hip_device_rc(device);
  if (rc) set_error(rc == G16_E_NOGPU ? no_device : bad_ordinal);
  return rc;
}
// ... of the routes without a CPU path; called after every input check
inline int require_hip_device(const char* route, int device) {
  return require_hip_device(device, std::string(route) + ": no HIP device (there is no CPU path)",
                            std::string(route) + ": bad device ordinal");
}

// ---------------------------------------------------------------- status: the first HIP failure ends the route
struct DeviceJob {
  const char* route;
  int rc = G16_OK;
  explicit DeviceJob(const char* route_name) : route(route_name) {}
  bool fail(hipError_t e) {   // "<route> (device): <hip error string>"
    if (e == hipSuccess) return false;
    set_error(std::string(route) + " (device): " + hipGetErrorString(e));
    rc = G16_E_HIP;
    return true;
  }
};

// ---------------------------------------------------------------- owners
// Movable, not copyable: a move leaves its source empty, and a move assignment releases what the target held first
// (so `x = X()` is "release, then start from defaults").  Each converts to the raw pointer or handle it holds.
template <class T> struct DeviceBuf {   // T = void: an allocation in bytes (the MSM's point buffers)
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  T* p = nullptr;
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  DeviceBuf& operator=(DeviceBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); } return *this; }
  ~DeviceBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t alloc(size_t count) { return alloc_bytes((count ? count : 1) * kElem); }   // (never empty)
  hipError_t alloc_bytes(size_t bytes) {   // exactly `bytes`; frees what it held first; null when it fails
    reset();
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  operator T*() const { return p; }
  template <class U> explicit operator U*() const { return (U*)p; }
};
// src on the device, in an allocation one element larger than src (so an empty array still has an address)
template <class T> hipError_t upload(DeviceBuf<T>& dst, const std::vector<T>& src) {
  const hipError_t e = dst.alloc(src.size() + 1);
  return e != hipSuccess || src.empty() ? e : hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

template <class T> struct PinnedBuf {   // page-locked host memory, as DeviceBuf
  T* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); } return *this; }
  ~PinnedBuf() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; }
  hipError_t alloc(size_t count) { return alloc_bytes((count ? count : 1) * sizeof(T)); }
  hipError_t alloc_bytes(size_t bytes) {
    reset();
    const hipError_t e = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  operator T*() const { return p; }
  template <class U> explicit operator U*() const { return (U*)p; }
};

struct DeviceStream {
  hipStream_t s = nullptr;
  DeviceStream() = default;
  DeviceStream(DeviceStream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
  DeviceStream& operator=(DeviceStream&& o) noexcept { if (this != &o) { reset(); s = std::exchange(o.s, nullptr); } return *this; }
  ~DeviceStream() { reset(); }
  void reset() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } s = nullptr; }
  hipError_t created(hipError_t e) { if (e != hipSuccess) s = nullptr; return e; }
  hipError_t create() { reset(); return created(hipStreamCreate(&s)); }
  hipError_t create(unsigned flags, int priority) { reset(); return created(hipStreamCreateWithPriority(&s, flags, priority)); }
  operator hipStream_t() const { return s; }
};

// waits for a stream when its scope ends, unless the scope reached its own successful wait and said so
struct StreamDrain {
  hipStream_t s;
  bool armed = true;
  explicit StreamDrain(hipStream_t st) : s(st) {}
  StreamDrain(const StreamDrain&) = delete;
  StreamDrain& operator=(const StreamDrain&) = delete;
  ~StreamDrain() { if (armed) (void)hipStreamSynchronize(s); }
  void dismiss() { armed = false; }
};

struct DeviceEvent {   // one event: a hand-over to another stream or to the host
  hipEvent_t e = nullptr;
  DeviceEvent() = default;
  DeviceEvent(DeviceEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  DeviceEvent& operator=(DeviceEvent&& o) noexcept { if (this != &o) { reset(); e = std::exchange(o.e, nullptr); } return *this; }
  ~DeviceEvent() { reset(); }
  void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  hipError_t created(hipError_t r) { if (r != hipSuccess) e = nullptr; return r; }
  hipError_t create() { reset(); return created(hipEventCreate(&e)); }
  hipError_t create(unsigned flags) { reset(); return created(hipEventCreateWithFlags(&e, flags)); }
  operator hipEvent_t() const { return e; }
  hipError_t record(hipStream_t st) { return hipEventRecord(e, st); }
};

template <int N> struct PhaseEvents {   // the N + 1 events around the N phases of a batch
  static_assert(N >= 1, "PhaseEvents times phases; a single event is a DeviceEvent");
  hipEvent_t e[N + 1] = {};
  PhaseEvents() = default;
  PhaseEvents(const PhaseEvents&) = delete;
  PhaseEvents& operator=(const PhaseEvents&) = delete;
  ~PhaseEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  hipError_t create() {
    for (hipEvent_t& x : e) {
      const hipError_t r = hipEventCreate(&x);
      if (r != hipSuccess) { x = nullptr; return r; }
    }
    return hipSuccess;
  }
  hipError_t record(int k, hipStream_t st) { return hipEventRecord(e[k], st); }
  float ms(int k) const {   // phase k, once the stream has passed event k + 1; 0 when it cannot be read
    float v = 0.f;
    return hipEventElapsedTime(&v, e[k], e[k + 1]) == hipSuccess ? v : 0.f;
  }
};

struct DeviceTimer {   // two events around a stretch of a stream's work
  hipEvent_t e0 = nullptr, e1 = nullptr;
  DeviceTimer() = default;
  DeviceTimer(const DeviceTimer&) = delete;
  DeviceTimer& operator=(const DeviceTimer&) = delete;
  ~DeviceTimer() { for (hipEvent_t e : {e0, e1}) if (e) (void)hipEventDestroy(e); }
  hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
  hipError_t start(hipStream_t st) { return hipEventRecord(e0, st); }
  hipError_t stop(hipStream_t st) { return hipEventRecord(e1, st); }
  float ms() const {   // once the stream has passed stop(); 0 when it cannot be read
    float v = 0.f;
    return hipEventElapsedTime(&v, e0, e1) == hipSuccess ? v : 0.f;
  }
};

}  // namespace g16
