// NIST P-256 for ES256 (ECDSA with SHA-256, RFC 7518 3.4 / COSE alg -7): the base field p, the scalar field n, the curve
// y^2 = x^3 - 3x + b in Jacobian coordinates, and the pieces of one signature verification.  8 x 32-bit Montgomery limbs,
// R = 2^256, like fp.cuh -- but NOT fp.cuh's forms: both moduli are above 2^255, so a + b reaches 2^257 (a carry out of limb
// 7) and the CIOS running value, below 2m, needs a second carry word.  The forms here keep that carry, on the device's
// 8 x 32 path and on the host's 4 x 64 path alike.
//
// Everything is __host__ __device__: the kernels of es256_verify.hip and the host-thread route of es256_host.cpp (device
// -1) run the same code, which is what lets a machine without a GPU test the arithmetic the kernels run.
//
// gfx950 notes: for p, -p^-1 mod 2^32 = 1, so the Montgomery factor of a round is the low word itself, and three limbs of
// p are zero: after unrolling the compiler drops those products.  Values stay fully reduced in [0, m) between operations.
#pragma once
#include <stdint.h>

#include "p256_consts.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef G16_HD
#define G16_HD __host__ __device__ __forceinline__
#endif
#define G16_P256_FN __host__ __device__ inline
#else
#ifndef G16_HD
#define G16_HD inline
#endif
#define G16_P256_FN inline
#endif

namespace g16 {

struct P256FpParams {
  static constexpr uint32_t P[8] = G16_P256_FP_P;
  static constexpr uint32_t ONE[8] = G16_P256_FP_ONE;
  static constexpr uint32_t R2[8] = G16_P256_FP_R2;
  static constexpr uint32_t INV = G16_P256_FP_INV;
};
struct P256FnParams {
  static constexpr uint32_t P[8] = G16_P256_FN_P;
  static constexpr uint32_t ONE[8] = G16_P256_FN_ONE;
  static constexpr uint32_t R2[8] = G16_P256_FN_R2;
  static constexpr uint32_t INV = G16_P256_FN_INV;
};

template <class PM>
struct alignas(16) PF {
  uint32_t v[8];
};
using P256Fp = PF<P256FpParams>;   // coordinates
using P256Fn = PF<P256FnParams>;   // scalars (the group order)

template <class PM> G16_HD PF<PM> pf_zero() {
  PF<PM> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
  return r;
}
template <class PM> G16_HD PF<PM> pf_one() {
  PF<PM> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = PM::ONE[i];
  return r;
}
template <class PM> G16_HD bool pf_is_zero(const PF<PM>& a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}
template <class PM> G16_HD bool pf_eq(const PF<PM>& a, const PF<PM>& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}
// a >= m, for any 256-bit a (the range checks of keys and signatures)
template <class PM> G16_HD bool pf_geq_mod(const PF<PM>& a) {
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    br += (int64_t)a.v[i] - (int64_t)PM::P[i];
    br >>= 32;
  }
  return br == 0;
}

// (hi * 2^256 + a) - m if that is >= 0 else a, for a value below 2m with hi its ninth word (0 or 1)
template <class PM> G16_HD void pf_reduce_once(PF<PM>& a, uint32_t hi) {
  uint32_t d[8];
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    br += (int64_t)a.v[i] - (int64_t)PM::P[i];
    d[i] = (uint32_t)br;
    br >>= 32;  // arithmetic: 0 or -1
  }
  const bool ge = hi != 0 || br == 0;   // with hi set the difference wraps to the right low 256 bits
#pragma unroll
  for (int i = 0; i < 8; i++) a.v[i] = ge ? d[i] : a.v[i];
}

template <class PM> G16_HD PF<PM> pf_add(const PF<PM>& a, const PF<PM>& b) {
  PF<PM> r;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  pf_reduce_once(r, (uint32_t)c);   // m > 2^255: the sum can pass 2^256, c is its ninth word
  return r;
}

template <class PM> G16_HD PF<PM> pf_sub(const PF<PM>& a, const PF<PM>& b) {
  PF<PM> r;
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    br += (int64_t)a.v[i] - (int64_t)b.v[i];
    r.v[i] = (uint32_t)br;
    br >>= 32;
  }
  const uint32_t mask = (uint32_t)br;  // all ones when a < b
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)r.v[i] + (PM::P[i] & mask);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
  return r;
}

template <class PM> G16_HD PF<PM> pf_dbl(const PF<PM>& a) { return pf_add(a, a); }

// Montgomery product a*b*R^-1 mod m, CIOS.  The running value stays below 2m < 2^257: word 8 holds its top bit, and
// the sum of a round (below 2m + 2^32 m) can carry once more, into `t9`.
template <class PM> G16_HD PF<PM> pf_mul(const PF<PM>& a, const PF<PM>& b) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__SIZEOF_INT128__) && !defined(G16_HOST_MUL32)
  // host build: the same CIOS on 4 x 64-bit limbs
  typedef unsigned __int128 u128;
  uint64_t A[4], B[4], P[4], t[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    A[i] = a.v[2 * i] | ((uint64_t)a.v[2 * i + 1] << 32);
    B[i] = b.v[2 * i] | ((uint64_t)b.v[2 * i + 1] << 32);
    P[i] = PM::P[2 * i] | ((uint64_t)PM::P[2 * i + 1] << 32);
  }
  // -m^-1 mod 2^64 from the 32-bit constant by one Newton step: x' = x (2 + m x)  (x = -m^-1)
  const uint64_t inv32 = PM::INV;
  const uint64_t inv64 = inv32 * (2 + P[0] * inv32);
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) { c += (u128)A[j] * B[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[4];
    const uint64_t t4 = (uint64_t)c, t5 = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * inv64;
    c = (u128)m * P[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; j++) { c += (u128)m * P[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t4;
    t[3] = (uint64_t)c;
    t[4] = (uint64_t)(c >> 64) + t5;
  }
  PF<PM> r;
  for (int i = 0; i < 4; i++) { r.v[2 * i] = (uint32_t)t[i]; r.v[2 * i + 1] = (uint32_t)(t[i] >> 32); }
  pf_reduce_once(r, (uint32_t)t[4]);
  return r;
#else
  uint32_t t[9];
#pragma unroll
  for (int i = 0; i < 9; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    const uint32_t bi = b.v[i];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a.v[j] * bi + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    c += t[8];
    const uint32_t t8 = (uint32_t)c, t9 = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * PM::INV;
    c = (uint64_t)m * PM::P[0] + t[0];
    c >>= 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * PM::P[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    c += t8;
    t[7] = (uint32_t)c;
    t[8] = (uint32_t)(c >> 32) + t9;
  }
  PF<PM> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  pf_reduce_once(r, t[8]);
  return r;
#endif
}

template <class PM> G16_HD PF<PM> pf_sqr(const PF<PM>& a) { return pf_mul(a, a); }

// standard integer (below m) -> Montgomery and back
template <class PM> G16_HD PF<PM> pf_to_mont(const PF<PM>& a) {
  PF<PM> r2;
#pragma unroll
  for (int i = 0; i < 8; i++) r2.v[i] = PM::R2[i];
  return pf_mul(a, r2);
}
template <class PM> G16_HD PF<PM> pf_from_mont(const PF<PM>& a) {
  PF<PM> one = pf_zero<PM>();
  one.v[0] = 1;
  return pf_mul(a, one);
}

// Fermat inverse a^(m-2) of a Montgomery value, bit by bit (the exponent is the same on every lane: no divergence);
// inv(0) = 0.  256 squarings and one product per set bit: about a fifth of a verification.
template <class PM> G16_P256_FN PF<PM> pf_inv(const PF<PM>& a) {
  PF<PM> r = pf_one<PM>();
#pragma unroll
  for (int l = 7; l >= 0; l--) {
    const uint32_t w = PM::P[l] - (l == 0 ? 2u : 0u);   // both moduli are odd with a low limb above 2
#pragma unroll 1
    for (int i = 31; i >= 0; i--) {
      r = pf_sqr(r);
      if ((w >> i) & 1) r = pf_mul(r, a);
    }
  }
  return r;
}

// 32 big-endian bytes <-> limbs (no reduction)
template <class PM> G16_HD PF<PM> pf_load_be(const uint8_t* p) {
  PF<PM> r;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = p + 28 - 4 * i;
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  return r;
}
template <class PM> G16_HD void pf_store_be(uint8_t* p, const PF<PM>& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint8_t* q = p + 28 - 4 * i;
    q[0] = (uint8_t)(a.v[i] >> 24);
    q[1] = (uint8_t)(a.v[i] >> 16);
    q[2] = (uint8_t)(a.v[i] >> 8);
    q[3] = (uint8_t)a.v[i];
  }
}

// ------------------------------------------------------------------ the curve y^2 = x^3 - 3x + b
struct alignas(16) P256Affine {
  P256Fp x, y;   // Montgomery; (0, 0) = infinity (not a point: b != 0)
};
struct alignas(16) P256Jac {
  P256Fp X, Y, Z;   // x = X / Z^2, y = Y / Z^3; Z = 0 = infinity
};

G16_HD bool p256_aff_is_inf(const P256Affine& a) { return pf_is_zero(a.x) && pf_is_zero(a.y); }
G16_HD bool p256_is_inf(const P256Jac& a) { return pf_is_zero(a.Z); }
G16_HD void p256_set_inf(P256Jac& a) {
  a.X = pf_one<P256FpParams>();
  a.Y = pf_one<P256FpParams>();
  a.Z = pf_zero<P256FpParams>();
}
G16_HD void p256_from_affine(P256Jac& r, const P256Affine& a) {
  if (p256_aff_is_inf(a)) { p256_set_inf(r); return; }
  r.X = a.x;
  r.Y = a.y;
  r.Z = pf_one<P256FpParams>();
}
G16_P256_FN bool p256_on_curve(const P256Affine& a) {   // of a point that is not infinity
  P256Fp b;
  const uint32_t kB[8] = G16_P256_B;
#pragma unroll
  for (int i = 0; i < 8; i++) b.v[i] = kB[i];
  const P256Fp x2 = pf_sqr(a.x);
  const P256Fp three_x = pf_add(pf_dbl(a.x), a.x);
  const P256Fp rhs = pf_add(pf_sub(pf_mul(x2, a.x), three_x), b);
  return pf_eq(pf_sqr(a.y), rhs);
}

// a <- 2a, the a = -3 doubling (3 (X - Z^2)(X + Z^2) for the slope's numerator): 4 products, 4 squarings.  Infinity
// stays infinity; the group has prime order, so no finite point has Y = 0.
G16_P256_FN void p256_dbl(P256Jac& a) {
  const P256Fp delta = pf_sqr(a.Z), gamma = pf_sqr(a.Y);
  const P256Fp beta = pf_mul(a.X, gamma);
  const P256Fp t = pf_mul(pf_sub(a.X, delta), pf_add(a.X, delta));
  const P256Fp alpha = pf_add(pf_dbl(t), t);
  const P256Fp beta4 = pf_dbl(pf_dbl(beta));
  const P256Fp X3 = pf_sub(pf_sqr(alpha), pf_dbl(beta4));
  const P256Fp yz = pf_add(a.Y, a.Z);
  const P256Fp Z3 = pf_sub(pf_sub(pf_sqr(yz), gamma), delta);
  const P256Fp g2 = pf_sqr(gamma);
  const P256Fp g8 = pf_dbl(pf_dbl(pf_dbl(g2)));
  a.Y = pf_sub(pf_mul(alpha, pf_sub(beta4, X3)), g8);
  a.X = X3;
  a.Z = Z3;
}

// the tail shared by both additions: H = U2 - U1 != 0, r = S2 - S1, Zf = the product of the Z's
G16_HD void p256_add_tail(P256Jac& a, const P256Fp& U1, const P256Fp& S1, const P256Fp& H, const P256Fp& r, const P256Fp& Zf) {
  const P256Fp HH = pf_sqr(H);
  const P256Fp HHH = pf_mul(H, HH);
  const P256Fp V = pf_mul(U1, HH);
  const P256Fp X3 = pf_sub(pf_sub(pf_sqr(r), HHH), pf_dbl(V));
  a.Y = pf_sub(pf_mul(r, pf_sub(V, X3)), pf_mul(S1, HHH));
  a.X = X3;
  a.Z = pf_mul(Zf, H);
}

// a <- a + q, q affine.  Every case: q infinity, a infinity, a = q (doubling), a = -q (infinity).
G16_P256_FN void p256_madd(P256Jac& a, const P256Affine& q) {
  if (p256_aff_is_inf(q)) return;
  if (p256_is_inf(a)) { p256_from_affine(a, q); return; }
  const P256Fp zz = pf_sqr(a.Z);
  const P256Fp U2 = pf_mul(q.x, zz);
  const P256Fp S2 = pf_mul(q.y, pf_mul(a.Z, zz));
  const P256Fp H = pf_sub(U2, a.X), r = pf_sub(S2, a.Y);
  if (pf_is_zero(H)) {
    if (pf_is_zero(r)) p256_dbl(a);
    else p256_set_inf(a);
    return;
  }
  p256_add_tail(a, a.X, a.Y, H, r, a.Z);
}

// a <- a + b, both Jacobian, the same cases
G16_P256_FN void p256_add(P256Jac& a, const P256Jac& b) {
  if (p256_is_inf(b)) return;
  if (p256_is_inf(a)) { a = b; return; }
  const P256Fp z1z1 = pf_sqr(a.Z), z2z2 = pf_sqr(b.Z);
  const P256Fp U1 = pf_mul(a.X, z2z2), U2 = pf_mul(b.X, z1z1);
  const P256Fp S1 = pf_mul(a.Y, pf_mul(b.Z, z2z2)), S2 = pf_mul(b.Y, pf_mul(a.Z, z1z1));
  const P256Fp H = pf_sub(U2, U1), r = pf_sub(S2, S1);
  if (pf_is_zero(H)) {
    if (pf_is_zero(r)) p256_dbl(a);
    else p256_set_inf(a);
    return;
  }
  p256_add_tail(a, U1, S1, H, r, pf_mul(a.Z, b.Z));
}

G16_P256_FN void p256_to_affine(P256Affine& r, const P256Jac& a) {
  if (p256_is_inf(a)) {
    r.x = pf_zero<P256FpParams>();
    r.y = pf_zero<P256FpParams>();
    return;
  }
  const P256Fp zi = pf_inv(a.Z), zi2 = pf_sqr(zi);
  r.x = pf_mul(a.X, zi2);
  r.y = pf_mul(a.Y, pf_mul(zi, zi2));
}

// ------------------------------------------------------------------ the resident window tables
// row[d - 1] = d * 16^w * P (d = 1..15), affine: one (point, window) unit of work.  P is a point of the curve and not
// infinity; the group order is a 256-bit prime, so no entry is infinity.
constexpr int kP256Win = 64;   // 4-bit windows of a 256-bit scalar
constexpr int kP256Row = 15;   // non-zero digits
constexpr int kP256TblPoint = kP256Win * kP256Row;   // entries per point (61 440 bytes)

G16_P256_FN void p256_table_row(const P256Affine& P, uint32_t w, P256Affine* row) {
  P256Jac b;
  p256_from_affine(b, P);
  for (uint32_t k = 0; k < 4 * w; k++) p256_dbl(b);
  P256Affine base;
  p256_to_affine(base, b);
  P256Jac acc;
  p256_set_inf(acc);
  for (int d = 0; d < kP256Row; d++) {
    p256_madd(acc, base);   // (d = 1 doubles: acc = base)
    p256_to_affine(row[d], acc);
  }
}

// ------------------------------------------------------------------ one ES256 verification, in its two phases
// Phase 1, a signature per lane: the range check 1 <= r, s < n, e = digest mod n (a digest can exceed n: one
// subtraction, 2^256 < 2n), w = 1 / s, u1 = e w, u2 = r w -- standard form (a Montgomery product of a standard and a
// Montgomery operand).  false = rejected by the range check (u1, u2 are then zero).
G16_P256_FN bool es256_scalars(const uint8_t* hash, const uint8_t* sig, P256Fn& u1, P256Fn& u2) {
  const P256Fn r = pf_load_be<P256FnParams>(sig), s = pf_load_be<P256FnParams>(sig + 32);
  u1 = pf_zero<P256FnParams>();
  u2 = u1;
  if (pf_is_zero(r) || pf_is_zero(s) || pf_geq_mod(r) || pf_geq_mod(s)) return false;
  P256Fn e = pf_load_be<P256FnParams>(hash);
  pf_reduce_once(e, 0);
  const P256Fn w = pf_inv(pf_to_mont(s));
  u1 = pf_mul(e, w);
  u2 = pf_mul(r, w);
  return true;
}

// Phase 2, `lanes` lanes per signature: u1 G + u2 Q is 128 table entries (64 windows of each scalar, a zero digit
// contributes nothing) and no doubling; lane `lane` sums entries lane, lane + lanes, ...: entry t < 64 is window t of
// u1 in G's table (point 0), entry 64 + w window w of u2 in the key's (point 1 + key).  The caller adds the lanes' sums.
// u1 / u2: the scalars' 8 words in memory (read by window: no register array is indexed).
G16_P256_FN void es256_slice_sum(P256Jac& acc, const P256Affine* tbl, uint32_t key, const uint32_t* u1, const uint32_t* u2,
                                 uint32_t lane, uint32_t lanes) {
  p256_set_inf(acc);
  for (uint32_t t = lane; t < 2 * kP256Win; t += lanes) {
    const uint32_t w = t & (kP256Win - 1);
    const uint32_t* u = t < (uint32_t)kP256Win ? u1 : u2;
    const uint32_t d = (u[w >> 3] >> (4 * (w & 7))) & 15u;
    if (!d) continue;
    const size_t point = t < (uint32_t)kP256Win ? 0 : 1 + (size_t)key;
    p256_madd(acc, tbl[(point * kP256Win + w) * kP256Row + d - 1]);
  }
}

// x(R) mod n == r without an inversion: r Z^2 == X, and -- p - n is a 127-bit number, so x(R) can be r + n --
// (r + n) Z^2 == X whenever r + n < p.  X, Z Montgomery; r the standard-form integer, 1 <= r < n.  Infinity: false.
G16_P256_FN bool p256_x_equals_r(const P256Fp& X, const P256Fp& Z, const P256Fn& r) {
  if (pf_is_zero(Z)) return false;
  const P256Fp zz = pf_sqr(Z);
  P256Fp rp;
#pragma unroll
  for (int i = 0; i < 8; i++) rp.v[i] = r.v[i];   // r < n < p
  if (pf_eq(pf_mul(pf_to_mont(rp), zz), X)) return true;
  // r < p - n ?
  const uint32_t kPmN[8] = G16_P256_PMN;
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    br += (int64_t)r.v[i] - (int64_t)kPmN[i];
    br >>= 32;
  }
  if (br == 0) return false;
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)r.v[i] + P256FnParams::P[i];
    rp.v[i] = (uint32_t)c;
    c >>= 32;
  }
  return pf_eq(pf_mul(pf_to_mont(rp), zz), X);
}

}  // namespace g16
