// One op of a witness program (witness_program.h) evaluated in Fr: the code the host route and the kernel of
// wtns_calc.hip both run (fp.cuh is __host__ __device__), so that the two routes cannot drift apart.  Wire values are
// canonical STANDARD-form words -- what a .wtns body and the prover's witness slot hold -- and the coefficients
// Montgomery images, so that one fp_mul of a wire with a coefficient gives the standard-form product.
#pragma once
#include "fp.cuh"

namespace g16 {

enum WpKind : uint32_t { WP_INPUT = 0, WP_QUAD = 1, WP_BITS = 2, WP_INV0 = 3, WP_ISZ = 4, WP_CHECK = 5, WP_KINDS = 6 };
static constexpr uint32_t kWpNoCheck = 0xffffffffu;

struct WpOp { uint32_t kind, dst, n, check, t_off, na, nb, nc; };
struct WpEvalTerm { uint32_t wire, coef; };   // coef: an index into the coefficient table; 0 = +1, 1 = -1
struct WpView {
  const WpOp* ops;
  const WpEvalTerm* terms;
  const Fr* coefs;        // Montgomery images of the distinct coefficients ...
  const int64_t* icoefs;  // ... and the integers themselves
  const uint32_t* targets;
  const Fr* inv_small;    // inv_small[k] = 1 / k in standard form, k < kWpInvSmall (entry 0 is 0)
};
static constexpr uint32_t kWpInvSmall = 4096;

// |c| * x for a wire value x below 2^64: below 2^127, so the plain integer is the field element
G16_HD Fr wp_small_product(uint64_t x, uint64_t mag) {
  const uint64_t a0 = (uint32_t)x, a1 = x >> 32, b0 = (uint32_t)mag, b1 = mag >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  const uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  Fr r = fp_zero<FrParams>();
  r.v[0] = (uint32_t)p00; r.v[1] = (uint32_t)mid; r.v[2] = (uint32_t)hi; r.v[3] = (uint32_t)(hi >> 32);
  return r;
}

// s + coefficient * x for one term
G16_HD Fr wp_acc(const WpView& p, const Fr& s, uint32_t coef, const Fr& x) {
  if (coef == 0) return fp_add(s, x);
  if (coef == 1) return fp_sub(s, x);
  if ((x.v[2] | x.v[3] | x.v[4] | x.v[5] | x.v[6] | x.v[7]) == 0) {
    // A small wire (nearly all are bits or bytes) times an integer coefficient: a 64 x 64 product instead of a
    // Montgomery one.  The 1 549 levels are led by the ~230-term sums of the SHA-256 additions (powers of two times
    // bits), one op to a thread: measured together with the inverse table below, DESIGN.md 3.1c.
    const int64_t c = p.icoefs[coef];
    const Fr m = wp_small_product((uint64_t)x.v[0] | ((uint64_t)x.v[1] << 32), c < 0 ? 0 - (uint64_t)c : (uint64_t)c);
    return c < 0 ? fp_sub(s, m) : fp_add(s, m);
  }
  return fp_add(s, fp_mul(x, p.coefs[coef]));
}

G16_HD Fr wp_lin(const WpView& p, uint32_t off, uint32_t cnt, const Fr* w) {
  Fr s = fp_zero<FrParams>();
  uint32_t i = off;
  const uint32_t end = off + cnt;
  for (; i + 4 <= end; i += 4) {   // four terms' wires in flight at once: a long form is a chain of dependent loads otherwise
    const WpEvalTerm t0 = p.terms[i], t1 = p.terms[i + 1], t2 = p.terms[i + 2], t3 = p.terms[i + 3];
    const Fr x0 = w[t0.wire], x1 = w[t1.wire], x2 = w[t2.wire], x3 = w[t3.wire];
    s = wp_acc(p, s, t0.coef, x0);
    s = wp_acc(p, s, t1.coef, x1);
    s = wp_acc(p, s, t2.coef, x2);
    s = wp_acc(p, s, t3.coef, x3);
  }
  for (; i < end; i++) {
    const WpEvalTerm t = p.terms[i];
    s = wp_acc(p, s, t.coef, w[t.wire]);
  }
  return s;
}

G16_HD Fr wp_small(uint32_t v) {
  Fr r = fp_zero<FrParams>();
  r.v[0] = v;
  return r;
}

// op `k` of the program on the wires w (every wire it reads is final); -> the check it violates, or kWpNoCheck
G16_HD uint32_t wp_eval_op(const WpView& p, uint32_t k, const Fr* inputs, Fr* w) {
  const WpOp op = p.ops[k];
  switch (op.kind) {
    case WP_INPUT:
      w[op.dst] = inputs[op.n];
      return kWpNoCheck;
    case WP_QUAD: {
      Fr r = wp_lin(p, op.t_off + op.na + op.nb, op.nc, w);
      if (op.na && op.nb) {   // (an empty form is 0, and so is the product)
        const Fr a = wp_lin(p, op.t_off, op.na, w), b = wp_lin(p, op.t_off + op.na, op.nb, w);
        r = fp_add(r, fp_mul(fp_to_mont(a), b));
      }
      w[op.dst] = r;
      return kWpNoCheck;
    }
    case WP_BITS: {
      Fr v = wp_lin(p, op.t_off, op.na, w);
      uint32_t over = 0;   // the bits of v from n on
      for (uint32_t i = 0; i < 8; i++) {
        const uint32_t lo = 32 * i;
        if (lo >= op.n) over |= v.v[i];
        else if (lo + 32 > op.n) over |= v.v[i] >> (op.n - lo);
      }
      if (over) v = fp_zero<FrParams>();
      for (uint32_t i = 0; i < op.n; i++) w[p.targets[op.dst + i]] = wp_small((v.v[i >> 5] >> (i & 31)) & 1u);
      return over ? op.check : kWpNoCheck;
    }
    case WP_INV0: {
      // The circuits invert differences of positions and of bytes (IsZero of i - index): of the 175 151 inversions of
      // a live-size witness nearly all are of k or -k with k below a few hundred, and a Fermat inversion is ~380
      // products.  Those come from a table; everything else takes the exponentiation.
      const Fr v = wp_lin(p, op.t_off, op.na, w);
      const Fr n = fp_neg(v);
      if ((v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < kWpInvSmall)
        w[op.dst] = p.inv_small[v.v[0]];
      else if ((n.v[1] | n.v[2] | n.v[3] | n.v[4] | n.v[5] | n.v[6] | n.v[7]) == 0 && n.v[0] < kWpInvSmall)
        w[op.dst] = fp_neg(p.inv_small[n.v[0]]);
      else
        w[op.dst] = fp_from_mont(fp_inv(fp_to_mont(v)));   // (fp_inv(0) = 0)
      return kWpNoCheck;
    }
    case WP_ISZ:
      w[op.dst] = wp_small(fp_is_zero(wp_lin(p, op.t_off, op.na, w)) ? 1u : 0u);
      return kWpNoCheck;
    default:   // WP_CHECK (the loader admits no other kind)
      return fp_is_zero(wp_lin(p, op.t_off, op.na, w)) ? kWpNoCheck : op.check;
  }
}

}  // namespace g16
