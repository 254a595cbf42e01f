// Fixed-base multiplication of the curve generators for the test-only setups (host code, threaded; the arithmetic is
// the product's own fp.cuh / ec.cuh compiled for the host), the Lagrange basis at a known tau, and FixedBaseMul, which
// sends a batch to host threads or to a HIP device (setup_gpu.hip).
#pragma once
#include "circuit.h"
#include "host_util.h"

namespace g16 {

template <class F> struct FixedBase {
  int wb = 8, nwin = 32;
  std::vector<Affine<F>> tbl;  // [nwin][2^wb - 1]
  size_t row() const { return ((size_t)1 << wb) - 1; }
};

template <class F> void batch_to_affine(const XYZZ<F>* in, Affine<F>* out, size_t n) {
  // one inversion per batch: x = X*(ZZ/ZZZ)^2, y = Y/ZZZ
  std::vector<typename F::T> pref(n);
  typename F::T acc = F::one();
  for (size_t i = 0; i < n; i++) {
    pref[i] = acc;
    if (!xyzz_is_inf(in[i])) acc = F::mul(acc, in[i].zzz);
  }
  typename F::T inv = F::inv(acc);
  for (size_t i = n; i-- > 0;) {
    if (xyzz_is_inf(in[i])) { out[i].x = F::zero(); out[i].y = F::zero(); continue; }
    const typename F::T zi = F::mul(inv, pref[i]);
    inv = F::mul(inv, in[i].zzz);
    const typename F::T zzi = F::sqr(F::mul(zi, in[i].zz));
    out[i].x = F::mul(in[i].x, zzi);
    out[i].y = F::mul(in[i].y, zi);
  }
}

template <class F> void build_table(FixedBase<F>& fb, const Affine<F>& gen, int wb, int threads) {
  fb.wb = wb;
  fb.nwin = (254 + wb - 1) / wb;
  const size_t row = fb.row();
  fb.tbl.resize((size_t)fb.nwin * row);
  std::vector<Affine<F>> bases(fb.nwin);
  XYZZ<F> b;
  xyzz_from_affine(b, gen);
  for (int j = 0; j < fb.nwin; j++) {
    xyzz_to_affine(bases[j], b);
    for (int k = 0; k < wb; k++) xyzz_dbl(b);
  }
  parallel_for((size_t)fb.nwin, threads, [&](size_t lo, size_t hi) {
    std::vector<XYZZ<F>> tmp(row);
    for (size_t j = lo; j < hi; j++) {
      XYZZ<F> acc;
      xyzz_set_inf(acc);
      for (size_t d = 0; d < row; d++) {
        xyzz_madd(acc, bases[j]);
        tmp[d] = acc;
      }
      batch_to_affine<F>(tmp.data(), &fb.tbl[j * row], row);
    }
  });
}

// out[i] = [k_i] G, k in Montgomery Fr; affine Montgomery bytes written at out + i*sizeof(Affine)
template <class F>
void fixed_mul_many(const FixedBase<F>& fb, const FrM* ks, size_t n, uint8_t* out, int threads) {
  const size_t row = fb.row();
  const uint32_t mask = (1u << fb.wb) - 1;
  parallel_for(n, threads, [&](size_t lo, size_t hi) {
    const size_t B = 512;
    std::vector<XYZZ<F>> acc(B);
    std::vector<Affine<F>> aff(B);
    for (size_t base = lo; base < hi; base += B) {
      const size_t cnt = base + B < hi ? B : hi - base;
      for (size_t i = 0; i < cnt; i++) {
        const Fr k = fp_from_mont(ks[base + i]);
        XYZZ<F>& a = acc[i];
        xyzz_set_inf(a);
        for (int j = 0; j < fb.nwin; j++) {
          const int pos = j * fb.wb;
          uint64_t v = k.v[pos >> 5];
          if ((pos >> 5) + 1 < 8) v |= (uint64_t)k.v[(pos >> 5) + 1] << 32;
          const uint32_t d = (uint32_t)(v >> (pos & 31)) & mask;
          if (d) xyzz_madd(a, fb.tbl[(size_t)j * row + d - 1]);
        }
      }
      batch_to_affine<F>(acc.data(), aff.data(), cnt);
      memcpy(out + base * sizeof(Affine<F>), aff.data(), cnt * sizeof(Affine<F>));
    }
  });
}

inline void batch_inverse(std::vector<FrM>& v) {
  const size_t n = v.size();
  std::vector<FrM> pref(n);
  FrM acc = fr_one();
  for (size_t i = 0; i < n; i++) { pref[i] = acc; acc = fp_mul(acc, v[i]); }
  FrM inv = fp_inv(acc);
  for (size_t i = n; i-- > 0;) {
    const FrM t = fp_mul(inv, pref[i]);
    inv = fp_mul(inv, v[i]);
    v[i] = t;
  }
}

inline FrM host_root(int L) {
  Fr w = {G16_FR_W28};
  for (int i = 28; i > L; i--) w = fp_sqr(w);
  return w;
}

// L_c(tau) over the size-2^L domain, c = first, first+step, ... (count values)
inline void lagrange_at(int L, const FrM& tau, size_t first, size_t step, size_t count, std::vector<FrM>& out) {
  const size_t N = (size_t)1 << L;
  const FrM w = host_root(L);
  const FrM zt = fp_sub(fp_pow_u64(tau, N), fr_one());
  const FrM scale = fp_mul(zt, fp_inv(fr_u64(N)));
  const FrM wstep = fp_pow_u64(w, step);
  std::vector<FrM> wc(count), den(count);
  FrM cur = fp_pow_u64(w, first);
  for (size_t i = 0; i < count; i++) {
    wc[i] = cur;
    den[i] = fp_sub(tau, cur);
    cur = fp_mul(cur, wstep);
  }
  batch_inverse(den);
  out.resize(count);
  for (size_t i = 0; i < count; i++) out[i] = fp_mul(fp_mul(scale, wc[i]), den[i]);
}

inline G1Affine g1_generator() {
  G1Affine g;
  g.x = fp_one<FqParams>();
  g.y = fp_add(g.x, g.x);
  return g;
}
inline G2Affine g2_generator() {
  G2Affine g;
  g.x.a = Fq{G16_G2X0}; g.x.b = Fq{G16_G2X1}; g.y.a = Fq{G16_G2Y0}; g.y.b = Fq{G16_G2Y1};
  return g;
}

// Both generator tables of window width wb, and where a batch [k_i]G runs: on HIP device `device` when that is >= 0
// and the batch holds at least device_min scalars, else on `threads` host threads (<= 0: all of them).  rc keeps the
// first device error, after which mul1 / mul2 do nothing; the caller checks it once.
struct FixedBaseMul {
  FixedBase<FqOps> g1;
  FixedBase<Fq2Ops> g2;
  int threads, device;
  size_t device_min;
  int rc = G16_OK;
  FixedBaseMul(int wb, int threads_, int device_, size_t device_min_ = 0)
      : threads(threads_), device(device_), device_min(device_min_) {
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    if (threads <= 0) threads = 1;
    build_table(g1, g1_generator(), wb, threads);
    build_table(g2, g2_generator(), wb, threads);
  }
  void mul1(const FrM* ks, size_t cnt, uint8_t* out) { mul(g1, setup_fixed_mul_g1, ks, cnt, out); }
  void mul2(const FrM* ks, size_t cnt, uint8_t* out) { mul(g2, setup_fixed_mul_g2, ks, cnt, out); }
  template <class F, class Dev> void mul(const FixedBase<F>& fb, Dev on_device, const FrM* ks, size_t cnt, uint8_t* out) {
    if (rc) return;
    if (device < 0 || cnt < device_min) fixed_mul_many(fb, ks, cnt, out, threads);
    else rc = on_device(device, fb.tbl.data(), fb.wb, fb.nwin, ks, cnt, out);
  }
};

}  // namespace g16
