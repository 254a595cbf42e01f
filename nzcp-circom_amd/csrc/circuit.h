// What the circuit generators, the builders and the setup routes share: Montgomery-form Fr helpers, the seeded generator
// Xo (the synthetic circuit, the trapdoor draw, the PLONK tau draw), the R1CS and its .r1cs / .wtns images (circuit.cpp).
#pragma once
#include "binfile.h"
#include "internal.h"

namespace g16 {

struct Xo {
  uint64_t s[4];
  explicit Xo(uint64_t seed) {
    uint64_t z = seed;
    for (int i = 0; i < 4; i++) {
      z += 0x9E3779B97F4A7C15ull;
      uint64_t x = z;
      x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
      x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
      s[i] = x ^ (x >> 31);
    }
  }
  static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  uint64_t next() {
    const uint64_t res = rotl(s[1] * 5, 7) * 9;
    const uint64_t t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
    return res;
  }
  uint64_t below(uint64_t k) { return next() % k; }
  Fr rand_fr_std() {  // (u0 | u1<<64 | u2<<128 | u3<<192) mod r, standard form
    Fr x;
    for (int i = 0; i < 4; i++) {
      const uint64_t u = next();
      x.v[2 * i] = (uint32_t)u;
      x.v[2 * i + 1] = (uint32_t)(u >> 32);
    }
    while (!fr_below_modulus(x.v)) {  // 2^256 / r < 6
      int64_t br = 0;
      for (int i = 0; i < 8; i++) {
        br += (int64_t)x.v[i] - (int64_t)kFrP[i];
        x.v[i] = (uint32_t)br;
        br >>= 32;
      }
    }
    return x;
  }
  Fr rand_fr() { return fp_to_mont(rand_fr_std()); }  // Montgomery
};

using FrM = Fr;  // Montgomery-form Fr in all host setup code

inline FrM fr_u64(uint64_t v) {
  Fr a = fp_zero<FrParams>();
  a.v[0] = (uint32_t)v;
  a.v[1] = (uint32_t)(v >> 32);
  return fp_to_mont(a);
}
inline FrM fr_one() { return fp_one<FrParams>(); }
inline FrM fr_neg_one() { return fp_neg(fp_one<FrParams>()); }

struct Term { uint32_t s; FrM cf; };
struct Circuit {
  uint32_t n, p, m;
  std::vector<uint8_t> cls;
  std::vector<uint32_t> rowA, rowB, rowC;  // row offsets (m+1) into the term arrays
  std::vector<Term> tA, tB, tC;
  struct Slack { uint32_t row, sw, j1; FrM c1; };
  std::vector<Slack> slacks;  // in constraint order
};

int g16_domain_log(const Circuit& c);   // smallest L with 2^L >= m + p + 1
// (allow_empty: a file without constraints is read, for the witness checker; every setup route refuses it)
int read_r1cs(const uint8_t* buf, size_t len, Circuit& c, bool allow_empty = false);
Buf write_r1cs(const Circuit& c, uint32_t n_pub_out, uint32_t n_pub_in);
Buf write_wtns(const std::vector<FrM>& w);   // w in Montgomery form

// Trapdoor Groth16 setup of `c` (setup_groth16.cpp), which every generator keys its circuit with: snarkjs zkey layout
// out, plus the verification-key points (vkey may be NULL).  td = (tau, alpha, beta, gamma, delta), Montgomery;
// setup_core draws it from stream seed + 1, all non-zero.
int setup_core_td(const Circuit& c, const FrM td[5], int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** vkey,
                  size_t* vkey_len);
int setup_core(const Circuit& c, uint64_t seed, int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** vkey,
               size_t* vkey_len);

}  // namespace g16
