// Host arithmetic on file images of curve points (curve_host.h).
#include "curve_host.h"

#include <fcntl.h>
#include <unistd.h>

#include "binfile.h"

namespace g16 {

namespace {
Fq fq_load(const uint8_t* p) { Fq x; memcpy(x.v, p, 32); return x; }
Fq fq_b3() { Fq t = fp_zero<FqParams>(); t.v[0] = 3; return fp_to_mont(t); }
Fq2 twist_b() { return Fq2{Fq{G16_G2B_C0}, Fq{G16_G2B_C1}}; }

void be32(const Fq& std_form, uint8_t out[32]) {
  for (int i = 0; i < 8; i++) {
    const uint32_t w = std_form.v[7 - i];
    out[4 * i] = (uint8_t)(w >> 24); out[4 * i + 1] = (uint8_t)(w >> 16); out[4 * i + 2] = (uint8_t)(w >> 8); out[4 * i + 3] = (uint8_t)w;
  }
}

bool fq_is_negative(const Fq& a_mont) {
  uint32_t half[8];
  for (int i = 0; i < 8; i++) half[i] = (kFqP[i] >> 1) | (i < 7 ? kFqP[i + 1] << 31 : 0);   // (q - 1) / 2, q odd
  const Fq s = fp_from_mont(a_mont);
  return !limbs_below(s.v, half) && memcmp(s.v, half, 32) != 0;
}

uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
}  // namespace

bool all_zero(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) if (p[i]) return false;
  return true;
}
bool limbs_below(const uint32_t a[8], const uint32_t m[8]) {
  for (int i = 7; i >= 0; i--)
    if (a[i] != m[i]) return a[i] < m[i];
  return false;
}

bool g1_image_ok(const uint8_t* p) {
  const Fq x = fq_load(p), y = fq_load(p + 32);
  if (!limbs_below(x.v, kFqP) || !limbs_below(y.v, kFqP)) return false;
  if (fp_is_zero(x) && fp_is_zero(y)) return true;
  return fp_eq(fp_sqr(y), fp_add(fp_mul(fp_sqr(x), x), fq_b3()));
}
bool g2_image_ok(const uint8_t* p) {
  Fq c[4];
  for (int i = 0; i < 4; i++) {
    c[i] = fq_load(p + 32 * i);
    if (!limbs_below(c[i].v, kFqP)) return false;
  }
  const Fq2 x{c[0], c[1]}, y{c[2], c[3]};
  if (Fq2Ops::is_zero(x) && Fq2Ops::is_zero(y)) return true;
  return Fq2Ops::eq(Fq2Ops::sqr(y), Fq2Ops::add(Fq2Ops::mul(Fq2Ops::sqr(x), x), twist_b()));
}

void g1_uncompressed(const uint8_t lem[64], uint8_t out[64]) {
  if (all_zero(lem, 64)) { memset(out, 0, 64); out[0] = 0x40; return; }
  be32(fp_from_mont(fq_load(lem)), out);
  be32(fp_from_mont(fq_load(lem + 32)), out + 32);
}
void g2_uncompressed(const uint8_t lem[128], uint8_t out[128]) {   // x.c1 | x.c0 | y.c1 | y.c0
  if (all_zero(lem, 128)) { memset(out, 0, 128); out[0] = 0x40; return; }
  be32(fp_from_mont(fq_load(lem + 32)), out);
  be32(fp_from_mont(fq_load(lem)), out + 32);
  be32(fp_from_mont(fq_load(lem + 96)), out + 64);
  be32(fp_from_mont(fq_load(lem + 64)), out + 96);
}

bool image_from_be(const uint8_t* be, size_t psz, uint8_t* lem) {
  if (be[0] & 0xc0) {
    if (be[0] != 0x40 || !all_zero(be + 1, psz - 1)) return false;
    memset(lem, 0, psz);
    return true;
  }
  const int nc = (int)(psz / 32);
  for (int c = 0; c < nc; c++) {
    Fq s;
    for (int i = 0; i < 8; i++) {
      const uint8_t* w = be + 32 * c + 4 * (7 - i);
      s.v[i] = (uint32_t)w[0] << 24 | (uint32_t)w[1] << 16 | (uint32_t)w[2] << 8 | w[3];
    }
    if (!limbs_below(s.v, kFqP)) return false;
    s = fp_to_mont(s);
    memcpy(lem + 32 * (nc == 2 ? c : c ^ 1), s.v, 32);
  }
  if (all_zero(lem, psz)) return false;   // (infinity is the flagged image alone)
  return nc == 2 ? g1_image_ok(lem) : g2_image_ok(lem);
}

const Gens& gens() {
  static const Gens g = [] {
    Gens o;
    G1Affine a;   // (1, 2)
    a.x = fp_one<FqParams>();
    a.y = fp_add(a.x, a.x);
    G2Affine b;
    b.x.a = Fq{G16_G2X0}; b.x.b = Fq{G16_G2X1}; b.y.a = Fq{G16_G2Y0}; b.y.b = Fq{G16_G2Y1};
    memcpy(o.g1, &a, 64);
    memcpy(o.g2, &b, 128);
    return o;
  }();
  return g;
}

// a^((q + 1) / 4): the square root when a is a square (q = 3 mod 4)
bool fq_sqrt(const Fq& a, Fq& root) {
  uint32_t e[8];
  uint64_t c = 1;
  for (int i = 0; i < 8; i++) { c += kFqP[i]; e[i] = (uint32_t)c; c >>= 32; }
  for (int i = 0; i < 8; i++) e[i] = (e[i] >> 2) | (i < 7 ? e[i + 1] << 30 : 0);
  root = fp_pow(a, e);
  return fp_eq(fp_sqr(root), a);
}
bool fq2_sqrt(const Fq2& a, Fq2& root) {
  const Fq zero = fp_zero<FqParams>();
  if (fp_is_zero(a.b)) {
    Fq s;
    if (fq_sqrt(a.a, s)) { root = Fq2{s, zero}; return true; }
    if (fq_sqrt(fp_neg(a.a), s)) { root = Fq2{zero, s}; return true; }   // (s u)^2 = -s^2
    return false;
  }
  Fq n;
  if (!fq_sqrt(fp_add(fp_sqr(a.a), fp_sqr(a.b)), n)) return false;   // the norm of a square is a square
  const Fq two_inv = fp_inv(fp_add(fp_one<FqParams>(), fp_one<FqParams>()));
  Fq x0;
  if (!fq_sqrt(fp_mul(fp_add(a.a, n), two_inv), x0) && !fq_sqrt(fp_mul(fp_sub(a.a, n), two_inv), x0)) return false;
  const Fq x1 = fp_mul(a.b, fp_inv(fp_add(x0, x0)));
  root = Fq2{x0, x1};
  return Fq2Ops::eq(Fq2Ops::sqr(root), a);
}
bool fq2_is_negative(const Fq2& a) { return fp_is_zero(a.b) ? fq_is_negative(a.a) : fq_is_negative(a.b); }

// The transcript's point on G2, ffjavascript's construction as far as it can be restated without the package: a
// ChaCha20 word stream keyed with the first 32 transcript bytes (eight big-endian words), field elements drawn as four
// 64-bit words (low word first, each word = first u32 * 2^32 + second u32) masked to 254 bits and redrawn until below
// q, THE DRAWN VALUE TAKEN AS THE MONTGOMERY IMAGE; x = (c0, c1), then one bit `greatest`; both redrawn until
// x^3 + b' is a square; y = the root that is negative exactly when `greatest`; the point times the cofactor 2q - r.
// NOT CROSS-CHECKED AGAINST snarkjs (ffjavascript is not available to the tests): the twin in tests/zkey_mpc_ref.py is
// written from the same description.  The whole derivation lives in this one function, so a correction is a one-place
// change (and one in the twin).
void hash_to_g2(const uint8_t transcript[64], G2Affine& out) {
  ChaCha rng;
  for (int i = 0; i < 8; i++)
    rng.key[i] = (uint32_t)transcript[4 * i] << 24 | (uint32_t)transcript[4 * i + 1] << 16 | (uint32_t)transcript[4 * i + 2] << 8 |
                 transcript[4 * i + 3];
  G2Affine p;
  for (;;) {
    rng.next_below(kFqP, p.x.a.v);
    rng.next_below(kFqP, p.x.b.v);
    const bool greatest = rng.next_u32() & 1;
    const Fq2 rhs = Fq2Ops::add(Fq2Ops::mul(Fq2Ops::sqr(p.x), p.x), twist_b());
    if (!fq2_sqrt(rhs, p.y)) continue;
    if (fq2_is_negative(p.y) != greatest) p.y = Fq2Ops::neg(p.y);
    break;
  }
  uint32_t cof[8];   // 2q - r
  {
    int64_t c = 0;
    for (int i = 0; i < 8; i++) {
      c += 2 * (int64_t)kFqP[i] - (int64_t)kFrP[i];
      cof[i] = (uint32_t)c;
      c >>= 32;
    }
  }
  G2XYZZ acc;
  xyzz_mul_scalar(acc, p, cof);
  xyzz_to_affine(out, acc);
}

void ChaCha::refill() {
  uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  for (int i = 0; i < 8; i++) s[4 + i] = key[i];
  s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = 0; s[15] = 0;
  uint32_t x[16];
  memcpy(x, s, sizeof(x));
  auto qr = [&](int a, int b, int c, int d) {
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
  };
  for (int r = 0; r < 10; r++) {
    qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
    qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
  }
  for (int i = 0; i < 16; i++) buf[i] = x[i] + s[i];
  counter++;
  have = 16;
}
void ChaCha::next_below(const uint32_t mod[8], uint32_t out[8]) {
  for (;;) {
    for (int i = 0; i < 4; i++) { const uint64_t w = next_u64(); out[2 * i] = (uint32_t)w; out[2 * i + 1] = (uint32_t)(w >> 32); }
    out[7] &= 0x3fffffffu;
    if (limbs_below(out, mod)) return;
  }
}

int os_random(uint8_t* out, size_t n) {
  const int fd = open("/dev/urandom", O_RDONLY);
  if (fd < 0) { set_error("cannot open /dev/urandom"); return G16_E_STATE; }
  const bool ok = read(fd, out, n) == (ssize_t)n;
  close(fd);
  if (!ok) { set_error("short read from /dev/urandom"); return G16_E_STATE; }
  return G16_OK;
}
int random_fr(uint8_t* out, uint64_t n) {
  ChaCha rng;
  if (const int rc = os_random((uint8_t*)rng.key, 32)) return rc;
  for (uint64_t i = 0; i < n; i++) rng.next_below(kFrP, (uint32_t*)(out + i * 32));
  return G16_OK;
}

}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_hash_to_g2(const uint8_t transcript[64], uint8_t out[128]) {
  if (!transcript || !out) { set_error("NULL argument"); return G16_E_ARG; }
  G2Affine p;
  hash_to_g2(transcript, p);
  memcpy(out, &p, 128);
  return G16_OK;
}
