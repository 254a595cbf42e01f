// Blake2b-512 (RFC 7693), whole and streaming, and its two C entries.  The streaming form serves the circuit hash,
// whose feed arrives chunk by chunk from the device (zkey_cshash_host.cpp).
#include "blake2b.h"

#include <algorithm>

#include "binfile.h"

namespace g16 {

namespace {
const uint64_t kB2Iv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                           0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
const uint8_t kB2Sigma[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
inline uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

void b2_compress(uint64_t h[8], const uint8_t block[128], uint64_t t, bool last) {
  uint64_t m[16], v[16];
  for (int i = 0; i < 16; i++) m[i] = rd64(block + 8 * i);
  for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = kB2Iv[i]; }
  v[12] ^= t;   // (t < 2^64: the high counter word stays zero)
  if (last) v[14] = ~v[14];
  auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
    v[a] = v[a] + v[b] + x; v[d] = rotr64(v[d] ^ v[a], 32);
    v[c] = v[c] + v[d];     v[b] = rotr64(v[b] ^ v[c], 24);
    v[a] = v[a] + v[b] + y; v[d] = rotr64(v[d] ^ v[a], 16);
    v[c] = v[c] + v[d];     v[b] = rotr64(v[b] ^ v[c], 63);
  };
  for (int r = 0; r < 12; r++) {
    const uint8_t* s = kB2Sigma[r];
    G(0, 4, 8, 12, m[s[0]], m[s[1]]);
    G(1, 5, 9, 13, m[s[2]], m[s[3]]);
    G(2, 6, 10, 14, m[s[4]], m[s[5]]);
    G(3, 7, 11, 15, m[s[6]], m[s[7]]);
    G(0, 5, 10, 15, m[s[8]], m[s[9]]);
    G(1, 6, 11, 12, m[s[10]], m[s[11]]);
    G(2, 7, 8, 13, m[s[12]], m[s[13]]);
    G(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
}  // namespace

// The streaming form.  A full block is compressed only once a byte beyond it has arrived: the block that turns out to
// be the last must carry the final flag, also when the total length is a non-zero multiple of 128.
Blake2b512::Blake2b512() {
  for (int i = 0; i < 8; i++) h_[i] = kB2Iv[i];
  h_[0] ^= 0x01010000ull ^ 64;   // digest length 64, no key, fanout = depth = 1
}
void Blake2b512::update(const uint8_t* data, size_t len) {
  if (!len) return;
  if (have_) {   // top up the held-back bytes first
    const size_t take = std::min(len, (size_t)128 - have_);
    memcpy(buf_ + have_, data, take);
    have_ += take; data += take; len -= take;
    if (!len) return;   // (a full buffer stays: it may be the last block)
    t_ += 128;
    b2_compress(h_, buf_, t_, false);
    have_ = 0;
  }
  while (len > 128) {   // whole blocks where they lie, all but a last full one
    t_ += 128;
    b2_compress(h_, data, t_, false);
    data += 128; len -= 128;
  }
  memcpy(buf_, data, len);
  have_ = len;
}
void Blake2b512::final(uint8_t out[64]) {
  memset(buf_ + have_, 0, 128 - have_);
  b2_compress(h_, buf_, t_ + have_, true);
  memcpy(out, h_, 64);   // little-endian words
}

void blake2b512(const uint8_t* data, size_t len, uint8_t out[64]) {
  Blake2b512 b;
  b.update(data, len);
  b.final(out);
}

}  // namespace g16

using namespace g16;

extern "C" int g16_blake2b512(const uint8_t* data, size_t len, uint8_t out[64]) {
  if ((!data && len) || !out) { set_error("NULL argument"); return G16_E_ARG; }
  blake2b512(data, len, out);
  return G16_OK;
}

extern "C" int g16_blake2b512_parts(const uint8_t* data, size_t len, const size_t* cuts, size_t n_cuts, uint8_t out[64]) {
  if ((!data && len) || (!cuts && n_cuts) || !out) { set_error("NULL argument"); return G16_E_ARG; }
  size_t at = 0;
  for (size_t i = 0; i < n_cuts; i++) {
    if (cuts[i] < at || cuts[i] > len) { set_error("blake2b512 parts: the cuts must ascend and lie within the data"); return G16_E_ARG; }
    at = cuts[i];
  }
  Blake2b512 b;
  at = 0;
  for (size_t i = 0; i < n_cuts; i++) {
    b.update(data + at, cuts[i] - at);
    at = cuts[i];
  }
  b.update(data + at, len - at);
  b.final(out);
  return G16_OK;
}
