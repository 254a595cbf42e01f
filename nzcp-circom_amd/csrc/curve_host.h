// Host arithmetic on FILE IMAGES of curve points -- affine little-endian Montgomery, 64 bytes (G1) / 128 bytes (G2), the
// point at infinity as zero bytes -- for the ceremony routes: validity, the big-endian forms of the transcripts and
// exchange files, scalar multiples, the transcript's point on G2 and the random generators (curve_host.cpp).  The
// arithmetic is the product's own fp.cuh / ec.cuh compiled for the host; no HIP header, no internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ec.cuh"

namespace g16 {

bool all_zero(const uint8_t* p, size_t n);
bool limbs_below(const uint32_t a[8], const uint32_t m[8]);   // a < m, 8 x 32-bit little-endian limbs
// coordinates below q and the point on its curve; infinity passes
bool g1_image_ok(const uint8_t* p);
bool g2_image_ok(const uint8_t* p);

// uncompressed big-endian standard form (G1: x | y; G2: x.c1 | x.c0 | y.c1 | y.c0; infinity = 0x40 then zeros)
void g1_uncompressed(const uint8_t lem[64], uint8_t out[64]);
void g2_uncompressed(const uint8_t lem[128], uint8_t out[128]);
// the inverse (psz = 64 / 128): false for a flag other than a clean 0x40, a coordinate >= q or a point off its curve
bool image_from_be(const uint8_t* be, size_t psz, uint8_t* lem);

// [k] P on the host, k in standard form; F = FqOps (G1) / Fq2Ops (G2).  out may be lem.
template <class F> void mul_image(const uint8_t* lem, const Fr& k_std, uint8_t* out) {
  Affine<F> p, r;
  memcpy(&p, lem, sizeof(p));
  XYZZ<F> acc;
  xyzz_mul_scalar(acc, p, k_std.v);
  xyzz_to_affine(r, acc);
  memcpy(out, &r, sizeof(r));
}

struct Gens { uint8_t g1[64], g2[128]; };   // the generators (1, 2) and G2
const Gens& gens();

// square roots (q = 3 mod 4; false: not a square) and the sign rule of the transcript's point: "negative" = the
// standard value is above (q - 1) / 2, for Fq2 that of c1 unless c1 = 0
bool fq_sqrt(const Fq& a, Fq& root);
bool fq2_sqrt(const Fq2& a, Fq2& root);
bool fq2_is_negative(const Fq2& a);
void hash_to_g2(const uint8_t transcript[64], G2Affine& out);

// ChaCha20 block function as a word stream
struct ChaCha {
  uint32_t key[8];
  uint64_t counter = 0;
  uint32_t buf[16];
  int have = 0;
  void refill();
  uint32_t next_u32() {
    if (!have) refill();
    return buf[16 - have--];
  }
  uint64_t next_u64() { const uint64_t hi = next_u32(); return hi << 32 | next_u32(); }
  // sum_i next_u64 2^(64 i) masked to 254 bits, redrawn until below the modulus
  void next_below(const uint32_t mod[8], uint32_t out[8]);
};
int os_random(uint8_t* out, size_t n);     // /dev/urandom; G16_E_STATE with a text when it cannot be read
int random_fr(uint8_t* out, uint64_t n);   // n fresh standard-form scalars below r: ChaCha20 keyed from the OS CSPRNG

}  // namespace g16
