// The uncompressed big-endian standard-form image of a point, as the ceremony's challenge hash and the challenge /
// response files hold it (device code of ptau_scale.hip and ptau_points.hip): 32-byte coordinates x | y (G1),
// x.c1 | x.c0 | y.c1 | y.c0 (G2); infinity = zeros with bit 0x40 of byte 0.
#pragma once
#include "fp.cuh"

namespace g16 {

// a point as NC coordinates of Fq in the file's order (x.c0, x.c1, y.c0, y.c1 on G2); the big-endian images hold c1
// ahead of c0
template <int NC> __device__ __forceinline__ int be_slot(int c) { return NC == 2 ? c : c ^ 1; }
__device__ __forceinline__ Fq load_be(const uint32_t* p) {   // (every coordinate lies on a 32-byte boundary)
  const uint4 hi = reinterpret_cast<const uint4*>(p)[0], lo = reinterpret_cast<const uint4*>(p)[1];
  const uint32_t w[8] = {hi.x, hi.y, hi.z, hi.w, lo.x, lo.y, lo.z, lo.w};
  Fq s;
#pragma unroll
  for (int k = 0; k < 8; k++) s.v[7 - k] = __builtin_bswap32(w[k]);
  return s;
}
__device__ __forceinline__ void store_be(uint32_t* p, const Fq& s) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = __builtin_bswap32(s.v[7 - k]);
  reinterpret_cast<uint4*>(p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
__device__ __forceinline__ void store_inf(uint32_t* p, int words) {
  for (int w = 0; w < words; w++) p[w] = w == 0 ? 0x40u : 0u;   // (byte 0 of the little-endian word)
}

}  // namespace g16
