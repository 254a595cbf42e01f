// The per-lane scalar multiplication of the ceremony kernels (ptau_prepare.hip, ptau_scale.hip): fixed signed windows of
// W bits -- digits -(2^(W-1) - 1) .. 2^(W-1), ceil(254 / W) of them -- so the loop structure is the same for every lane
// and only zero digits diverge.  Canonical fp.cuh / ec.cuh arithmetic (complete XYZZ formulas): the result does not
// depend on W.
#pragma once
#include <hip/hip_runtime.h>

#include "ec.cuh"

namespace g16 {

// acc = [k] base, k standard form < r (read where indexed: a private copy would go to scratch); tbl = the lane's
// table slots, `stride` elements apart
template <class FC, int kWin>
__device__ __forceinline__ void pp_scalar_mul(XYZZ<FC>& acc, const XYZZ<FC>& base, const uint32_t* __restrict__ k,
                                              XYZZ<FC>* __restrict__ tbl, uint32_t stride) {
  constexpr int kTbl = 1 << (kWin - 1), kDigits = (254 + kWin - 1) / kWin;
  xyzz_set_inf(acc);
  if (xyzz_is_inf(base)) return;
  {
    XYZZ<FC> t = base;
    tbl[0] = t;
    xyzz_dbl(t);
    tbl[stride] = t;
    for (int e = 2; e < kTbl; e++) {
      xyzz_add(t, base);
      tbl[(size_t)e * stride] = t;
    }
  }
  // signed digits d_j in [-(2^(W-1) - 1), 2^(W-1)], k = sum d_j 2^(W j): a window above 2^(W-1) becomes window - 2^W and
  // carries one into the next; k < r < 2^254, so the top window (W = 3: bits 252-254, at most 3; W = 4: bits 252-255, at
  // most 3; W = 5: bits 250-254, at most 12) takes its carry without producing one
  auto window = [&](int j) -> uint32_t {
    const int pos = j * kWin;
    uint64_t v = k[pos >> 5];
    if ((pos >> 5) + 1 < 8) v |= (uint64_t)k[(pos >> 5) + 1] << 32;
    return (uint32_t)(v >> (pos & 31)) & ((1u << kWin) - 1);
  };
  uint64_t carry_lo = 0, carry_hi = 0;   // (kDigits <= 85 < 128)
  {
    uint32_t c = 0;
    for (int j = 0; j < kDigits; j++) {
      const uint32_t d = window(j) + c;
      c = d > (uint32_t)kTbl ? 1u : 0u;
      if (c) {
        if (j < 64) carry_lo |= 1ull << j;
        else carry_hi |= 1ull << (j - 64);
      }
    }
  }
  auto carry = [&](int j) -> uint32_t {
    if (j < 0) return 0;
    return (uint32_t)((j < 64 ? carry_lo >> j : carry_hi >> (j - 64)) & 1);
  };
  for (int j = kDigits - 1; j >= 0; j--) {
    if (j != kDigits - 1)
      for (int s = 0; s < kWin; s++) xyzz_dbl(acc);
    const int d = (int)(window(j) + carry(j - 1)) - (int)(carry(j) << kWin);
    if (d) {
      XYZZ<FC> e = tbl[(size_t)((d < 0 ? -d : d) - 1) * stride];
      if (d < 0) xyzz_neg(e);
      xyzz_add(acc, e);
    }
  }
}

}  // namespace g16
