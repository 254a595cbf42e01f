// SHA-256 (FIPS 180-4) for host and device: the compression function, and a streaming context that pulls the message
// through a byte source instead of a buffer, so that a message made of pieces (ToBeSigned, "given,family,dob") is
// hashed where it lies.  The schedule's 16 words and the state are indexed by constants only after unrolling: registers
// on the device, no scratch.  beacon.h keeps the host-only SHA-256 of the beacon routes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef G16_HD
#define G16_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef G16_HD
#define G16_HD inline
#endif
#endif

namespace g16 {

G16_HD uint32_t sha256_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// the round constants: the device's unrolled rounds name each one directly (no table in memory there)
#define G16_SHA256_K                                                                                                    \
  {0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, \
   0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, \
   0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, \
   0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, \
   0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, \
   0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, \
   0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, \
   0xc67178f2u}

// one block: w = the 16 message words (consumed), h = the running state
G16_HD void sha256_compress(uint32_t h[8], uint32_t w[16]) {
  constexpr uint32_t K[64] = G16_SHA256_K;
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 64; t++) {
    if (t >= 16) {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = k + S1 + ch + K[t] + w[t & 15];
    const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
    const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
    k = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + S0 + maj;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += k;
}

// The streaming context: the state, and how far the message has been read.  sha256_stream pulls bytes [0, len) of the
// message from `src(pos)` (positions ascend), block by block, pads, and leaves the digest in out (big-endian).
struct Sha256 {
  uint32_t h[8];
  uint32_t pos;
};
G16_HD void sha256_init(Sha256& c) {
  constexpr uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  for (int k = 0; k < 8; k++) c.h[k] = iv[k];
  c.pos = 0;
}
// byte `pos` of the padded message of `len` bytes that ends at `total` (a multiple of 64)
template <class Src> G16_HD uint32_t sha256_padded_byte(const Src& src, uint32_t len, uint32_t total, uint32_t pos) {
  if (pos < len) return src(pos) & 0xffu;
  if (pos == len) return 0x80u;
  if (pos < total - 8) return 0u;
  const uint64_t bits = (uint64_t)len * 8;
  return (uint32_t)(bits >> (8 * (total - 1 - pos))) & 0xffu;
}
template <class Src> G16_HD void sha256_stream(const Src& src, uint32_t len, uint8_t out[32]) {
  Sha256 c;
  sha256_init(c);
  const uint32_t total = (len + 9 + 63) / 64 * 64;
  while (c.pos < total) {
    uint32_t w[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; j++) {
      const uint32_t p = c.pos + 4 * (uint32_t)j;
      w[j] = sha256_padded_byte(src, len, total, p) << 24 | sha256_padded_byte(src, len, total, p + 1) << 16 |
             sha256_padded_byte(src, len, total, p + 2) << 8 | sha256_padded_byte(src, len, total, p + 3);
    }
    sha256_compress(c.h, w);
    c.pos += 64;
  }
  for (int k = 0; k < 8; k++) {
    out[4 * k] = (uint8_t)(c.h[k] >> 24);
    out[4 * k + 1] = (uint8_t)(c.h[k] >> 16);
    out[4 * k + 2] = (uint8_t)(c.h[k] >> 8);
    out[4 * k + 3] = (uint8_t)c.h[k];
  }
}

}  // namespace g16
