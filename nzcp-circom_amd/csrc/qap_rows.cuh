// The sparse row sum the QAP evaluation (qap.hip) and the witness checker (wtns_check.hip) share: one matrix in the
// resident CSR layout of QapCsr, and the lazy sum of one row's records against a witness.
#pragma once
#include "fr29.cuh"
#include "internal.h"

namespace g16 {

// One matrix as the kernel sees it, and the sum of one row's records [k0, k1) taken with stride `step` from lane offset `lane`:
// the +-1 records add or subtract the Montgomery image of their witness word (a 40-byte gather and nine limb additions instead
// of a repack and a 229-instruction product: r03, 79 % of the records), the general ones multiply.  Lazy sums: an added term is
// below 1.1r, a subtracted one adds 2r - x <= 2r; a weak reduction (-> 1.0001r) whenever seven units have gone in keeps the
// sum below 1 + 6 * 1.1 + 2 = 9.6r < 16r.
struct QapMat { const uint32_t *rp, *mid, *vptr, *col; const F29* val; };
__device__ __forceinline__ F29 qap_row_sum(const QapMat& M, uint32_t c, uint32_t lane, uint32_t step,
                                            const Fr* __restrict__ w, const F29* __restrict__ wm) {
  F29 s = f29_zero();
  uint32_t cnt = 0;
  const uint32_t k0 = M.rp[c], km = M.mid[c], k1 = M.rp[c + 1];
  for (uint32_t k = k0 + lane; k < km; k += step) {
    const uint32_t ci = M.col[k];
    const F29 x = wm[ci & 0x7fffffffu];
    if (ci >> 31) { s = fr29_sub<2>(s, x); cnt += 2; }
    else { s = fr29_add(s, x); cnt += 1; }
    if (cnt >= 7) { s = fr29_weak_reduce(s); cnt = 0; }
  }
  const uint32_t vp = M.vptr[c];
  for (uint32_t k = km + lane; k < k1; k += step) {
    s = fr29_add(s, fr29_mul(M.val[vp + (k - km)], fr29_repack(w[M.col[k]])));
    if (++cnt >= 7) { s = fr29_weak_reduce(s); cnt = 0; }
  }
  return s;
}

__device__ __forceinline__ F29 f29_shfl_xor(const F29& v, int mask) {
  F29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (uint32_t)__shfl_xor((int)v.l[i], mask, 64);
  r.pad_ = 0;
  return r;
}

}  // namespace g16
