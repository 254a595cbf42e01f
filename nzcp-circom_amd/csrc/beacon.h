// The public part of a beacon contribution (`snarkjs powersoftau beacon`, `zkey beacon`): the delay function and the
// record's params.  Host code, header only, nothing but the C library: tests/native/beacon_test.cpp builds it alone.
//   seed   = SHA-256 applied 2^e times to the beacon hash (the first application hashes the raw 1 to 255 bytes, every
//            later one 32 bytes).  One thread: the applications depend on each other.
//   params = [byte 1, len, name] | byte 2, byte e | byte 3, len, beacon hash -- ids ascending, as snarkjs's readers
//            demand.
// The secret scalars drawn from the seed are mpc_beacon_scalars' (zkey_mpc.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

namespace g16 {

constexpr uint32_t kBeaconExpMin = 10, kBeaconExpMax = 63;   // snarkjs's range of numIterationsExp
constexpr size_t kBeaconHashMax = 255;                       // what the one length byte of id 3 can hold

namespace beacon_detail {
constexpr uint32_t kShaK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
constexpr uint32_t kShaIv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// FIPS 180-4 compression of one block given as sixteen big-endian words
inline void sha256_compress(uint32_t h[8], const uint32_t block[16]) {
  uint32_t w[64];
  for (int i = 0; i < 16; i++) w[i] = block[i];
  for (int i = 16; i < 64; i++) {
    const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
    const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
    w[i] = w[i - 16] + s0 + w[i - 7] + s1;
  }
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  for (int i = 0; i < 64; i++) {
    const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kShaK[i] + w[i];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
}  // namespace beacon_detail

// SHA-256 of len bytes -> eight big-endian words
inline void sha256_words(const uint8_t* data, size_t len, uint32_t h[8]) {
  using namespace beacon_detail;
  for (int i = 0; i < 8; i++) h[i] = kShaIv[i];
  const size_t blocks = (len + 9 + 63) / 64;
  for (size_t b = 0; b < blocks; b++) {
    uint8_t buf[64] = {0};
    const size_t at = b * 64;
    if (at < len) memcpy(buf, data + at, len - at < 64 ? len - at : 64);
    if (len >= at && len - at < 64) buf[len - at] = 0x80;
    if (b + 1 == blocks) {
      const uint64_t bits = (uint64_t)len * 8;
      for (int i = 0; i < 8; i++) buf[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
    }
    uint32_t w[16];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)buf[4 * i] << 24 | (uint32_t)buf[4 * i + 1] << 16 | (uint32_t)buf[4 * i + 2] << 8 | buf[4 * i + 3];
    sha256_compress(h, w);
  }
}

// The delay function: seed (eight big-endian words) = SHA-256^(2^exp)(beacon).  The caller has checked the ranges.
inline void beacon_chain(const uint8_t* beacon, size_t beacon_len, uint32_t exp, uint32_t seed[8]) {
  using namespace beacon_detail;
  sha256_words(beacon, beacon_len, seed);
  uint32_t block[16] = {0};   // a 32-byte message: its words, the 0x80 byte, zeros, the length 256 bits
  block[8] = 0x80000000u;
  block[15] = 256;
  for (uint64_t i = 1, n = (uint64_t)1 << exp; i < n; i++) {
    for (int k = 0; k < 8; k++) { block[k] = seed[k]; seed[k] = kShaIv[k]; }
    sha256_compress(seed, block);
  }
}

// the ids 2 and 3 of a beacon record's params, to follow the name's (mpc_name_params)
inline std::string beacon_params(const uint8_t* beacon, size_t beacon_len, uint32_t exp) {
  std::string p;
  p += (char)2; p += (char)(uint8_t)exp;
  p += (char)3; p += (char)(uint8_t)beacon_len;
  p.append((const char*)beacon, beacon_len);
  return p;
}

// Walks params p[0, n) by snarkjs's rule: id 1 (len, name), id 2 (one byte e), id 3 (len, beacon hash), ids strictly
// ascending, nothing else and nothing cut short.  -> whether the block states a beacon: ids 2 and 3 both found, e in
// snarkjs's range, the hash not empty.  Reads no byte outside p[0, n).
struct BeaconStated { uint32_t exp = 0; const uint8_t* hash = nullptr; size_t hash_len = 0; };
inline bool beacon_params_walk(const uint8_t* p, size_t n, BeaconStated& out) {
  out = BeaconStated{};
  bool have2 = false;
  int last = 0;
  size_t i = 0;
  while (i < n) {
    const int id = p[i];
    if (id <= last || id > 3 || n - i < 2) return false;
    last = id;
    if (id == 2) {
      out.exp = p[i + 1];
      have2 = true;
      i += 2;
      continue;
    }
    const size_t len = p[i + 1];
    if (n - i - 2 < len) return false;
    if (id == 3) { out.hash = p + i + 2; out.hash_len = len; }
    i += 2 + len;
  }
  return have2 && out.hash && out.hash_len >= 1 && out.exp >= kBeaconExpMin && out.exp <= kBeaconExpMax;
}

}  // namespace g16
