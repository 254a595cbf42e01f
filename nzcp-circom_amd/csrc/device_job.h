// What a one-shot device route owns (host code only): device buffers, its stream, its timing events, its status.
// THE RULE, for every route: whatever work on the stream reads or writes -- a DeviceBuf, a NttTablesOwned, a MsmJob --
// is declared AHEAD of the DeviceStream.  Destructors run in reverse order, the stream's waits for its work and then
// destroys it, so the stream has drained before anything is freed, on every path out of the route.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

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
template <class T> struct DeviceBuf {
  T* p = nullptr;
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t alloc(size_t count) { reset(); return hipMalloc(&p, (count ? count : 1) * sizeof(T)); }   // (never empty)
};

struct DeviceStream {
  hipStream_t s = nullptr;
  DeviceStream() = default;
  DeviceStream(const DeviceStream&) = delete;
  DeviceStream& operator=(const DeviceStream&) = delete;
  ~DeviceStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
  hipError_t create() { return hipStreamCreate(&s); }
  operator hipStream_t() const { return s; }
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
