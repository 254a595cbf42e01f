// XYZZ -> affine on the device for the setup kernels (setup_gpu.hip, setup_ptau.hip): one lane per kBatch consecutive
// points, Montgomery's trick on their ZZZ (3 products per point + one Fermat inversion per batch), then
// x = X (ZZ/ZZZ)^2, y = Y / ZZZ.  Canonical fp.cuh arithmetic: the affine bytes are unique, so they equal the host's.
#pragma once
#include <hip/hip_runtime.h>

#include "ec.cuh"

namespace g16 {
namespace {

constexpr int kBatch = 8;

template <class FC>
__global__ __launch_bounds__(256) void setup_to_affine_kernel(const XYZZ<FC>* __restrict__ in, Affine<FC>* __restrict__ out,
                                                               uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lo = t * kBatch;
  if (lo >= n) return;
  const uint32_t cnt = n - lo < (uint32_t)kBatch ? n - lo : (uint32_t)kBatch;
  typename FC::T pref[kBatch];
  typename FC::T acc = FC::one();
  for (uint32_t e = 0; e < cnt; e++) {
    pref[e] = acc;
    const typename FC::T zzz = in[lo + e].zzz;
    if (!FC::is_zero(zzz)) acc = FC::mul(acc, zzz);
  }
  typename FC::T inv = FC::inv(acc);
  for (uint32_t e = cnt; e-- > 0;) {
    const XYZZ<FC> p = in[lo + e];
    Affine<FC> a;
    if (xyzz_is_inf(p)) {
      a.x = FC::zero();
      a.y = FC::zero();
    } else {
      const typename FC::T zi = FC::mul(inv, pref[e]);
      inv = FC::mul(inv, p.zzz);
      const typename FC::T zzi = FC::sqr(FC::mul(zi, p.zz));
      a.x = FC::mul(p.x, zzi);
      a.y = FC::mul(p.y, zi);
    }
    out[lo + e] = a;
  }
}

}  // namespace
}  // namespace g16
