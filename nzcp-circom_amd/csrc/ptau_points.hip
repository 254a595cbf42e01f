// The point conversions of the phase-1 challenge / response exchange (`snarkjs powersoftau export challenge`,
// `challenge contribute`, `import response`; ptau_mpc.cpp), one lane per point:
//   ptau_from_be_kernel     uncompressed big-endian standard form -> the file form (affine little-endian Montgomery,
//                           infinity = zero bytes): the inverse of ptau_be_kernel (ptau_scale.hip), with the checks a
//                           stranger's file needs -- every coordinate below q, no flag but a clean 0x40, the point on
//                           its curve;
//   ptau_to_be_kernel       the file form -> uncompressed big-endian standard form, the inverse of the above (the
//                           MPCParams files of the phase-2 exchange, zkey_bellman.cpp; grid-stride, unlike
//                           ptau_scale.hip's ptau_be_kernel, which runs inside that route's own launch);
//   ptau_compress_kernel    the file form -> x alone, big-endian (G1: 32 bytes; G2: x.c1 | x.c0, 64 bytes), bit 0x80 of
//                           byte 0 set when y is "negative" (Fq: y > (q - 1) / 2; Fq2: that of c1, or of c0 when c1 = 0),
//                           infinity = zeros with bit 0x40 of byte 0;
//   ptau_decompress_kernel  the inverse: y = sqrt(x^3 + b), verified by squaring, negated where its sign disagrees with
//                           the flag; writes the file form and -- optionally -- the uncompressed big-endian image the
//                           next challenge hash is taken over.  x >= q, a 0x40 flag with any other bit set in the image,
//                           or x^3 + b without a root: a bad point.
// The first bad index of a section is an atomic minimum on one device word over GLOBAL indices (chunk base + lane
// index), so the order in which chunks and lanes arrive does not matter; the host reads the word once, after the last
// chunk's copies (a bad point is the rare case, and its outputs are discarded anyway).
//
// Square roots.  q = 3 mod 4, so in Fq the candidate root of a is s = a^((q+1)/4) = t a with t = a^((q-3)/4): ONE
// exponentiation by a constant (251 squarings and the products its set bits ask for -- about 380 Fq products), and
// t = 1/s for free when a is a non-zero square (t s = a^((q-1)/2) = 1).  In Fq2 = Fq[u]/(u^2+1), for a = a0 + a1 u with
// a1 != 0 (the norm route of the host's fq2_sqrt, folded so that no lane retries and nothing is inverted):
//   n = sqrt(a0^2 + a1^2) in Fq               (exponentiation 1; the norm of a square is a square)
//   c = (a0 + n) / 2,  t = c^((q-3)/4),  s = t c     (exponentiation 2; c != 0 because a1 != 0)
//   s^2 =  c:  root = (s, a1 t / 2)           (t = 1 / s)
//   s^2 = -c:  root = (-a1 t / 2, s)          (c is no square; then -c = x1^2 of the root with x0^2 = (a0 - n) / 2, and
//                                              t = -1 / s)
// exactly one of the two holds when a is a square: the candidates' product -(a1/2)^2 is a non-residue.  With a1 = 0 the
// same lines run with c = a0: the root is (s, 0) or (0, s) (the norm's exponentiation is then spent for nothing: a
// branch around it would diverge, and no curve point has such an a).  Whatever comes out is squared and compared with a, which
// is the whole test for "has a root".  Two Fq exponentiations, ~770 Fq products, against ~1800 for two exponentiations
// in Fq2.  The exponent is a compile-time constant: the loop bound and every "multiply here?" decision are scalar
// (uniform across the wavefront); there is no table indexed by a runtime value.  Which of the two roots is stored is
// fixed by the flag, so the bytes do not depend on the route.
//
// One driver for all stages (points_device): chunks (G16_PTAU_CHUNK) through the pipeline of chunk_pipeline.h; the
// grid is G16_PTAU_LANES lanes (whole wavefronts) or one lane per point of the chunk, grid-stride.  A stage is a
// functor that launches its kernel on (in, out, out2).
// As built for gfx950 (the compiler's resource usage; DESIGN.md 3.7f has the table): 0 B scratch in every kernel.
// Measured on one MI355X at power 20 (tools/ptau_challenge_bench.py, kernel events): decompress G1 4.6 ns,
// G2 9.6 - 9.7 ns per point against ptau_scale's 46.7 - 47.1 / 197.6 - 199.4 ns per product in the same process.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "chunk_pipeline.h"
#include "ec.cuh"
#include "internal.h"
#include "ptau_be.cuh"

namespace g16 {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoBad = 0xffffffffu;     // the device word while every point is good

// (q - 3) / 4 and (q - 1) / 2 as limbs, from the modulus
struct QConst {
  uint32_t e34[8], half[8];
};
constexpr QConst make_qconst() {
  QConst o{};
  const uint32_t p[8] = G16_FQ_P;
  uint32_t t[8] = {};
  for (int i = 0; i < 8; i++) t[i] = p[i];
  t[0] -= 3;   // (the low limb is above 3)
  for (int i = 0; i < 8; i++) {
    o.e34[i] = (t[i] >> 2) | (i < 7 ? t[i + 1] << 30 : 0u);
    o.half[i] = (p[i] >> 1) | (i < 7 ? p[i + 1] << 31 : 0u);
  }
  return o;
}
constexpr int top_bit(const uint32_t e[8]) {
  int t = 0;
  for (int i = 0; i < 256; i++)
    if ((e[i >> 5] >> (i & 31)) & 1) t = i;
  return t;
}
struct QC {
  static constexpr QConst K = make_qconst();
  static constexpr int kTop = top_bit(make_qconst().e34);   // 251
};

// a^((q-3)/4), from the exponent's top bit down: every branch below depends on the constant exponent and the loop
// counter alone
__device__ __forceinline__ Fq fq_pow_q34(const Fq& a) {
  Fq r = a;
#pragma unroll
  for (int w = QC::kTop / 32; w >= 0; w--) {
    const uint32_t word = QC::K.e34[w];
#pragma unroll 1
    for (int b = w == QC::kTop / 32 ? QC::kTop % 32 - 1 : 31; b >= 0; b--) {
      r = fp_sqr(r);
      if ((word >> b) & 1) r = fp_mul(r, a);
    }
  }
  return r;
}

__device__ __forceinline__ Fq fq_half(const Fq& a) {   // a / 2 (any residue form): (a + q) / 2 when a is odd
  const uint32_t mask = 0u - (a.v[0] & 1u);
  uint32_t s[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + (FqParams::P[i] & mask);
    s[i] = (uint32_t)c;
    c >>= 32;
  }
  Fq r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (s[i] >> 1) | (i < 7 ? s[i + 1] << 31 : 0u);   // (a + q < 2^255)
  return r;
}

__device__ __forceinline__ bool field_sqrt(const Fq& a, Fq& root) {
  root = fp_mul(fq_pow_q34(a), a);
  return fp_eq(fp_sqr(root), a);
}
__device__ __forceinline__ bool field_sqrt(const Fq2& a, Fq2& root) {
  const Fq norm = fp_add(fp_sqr(a.a), fp_sqr(a.b));
  const Fq n = fp_mul(fq_pow_q34(norm), norm);
  const Fq c = fp_is_zero(a.b) ? a.a : fq_half(fp_add(a.a, n));
  const Fq t = fq_pow_q34(c), s = fp_mul(t, c);
  const Fq h = fq_half(fp_mul(a.b, t));
  if (fp_eq(fp_sqr(s), c)) root = Fq2{s, h};
  else root = Fq2{fp_neg(h), s};
  return Fq2Ops::eq(Fq2Ops::sqr(root), a);
}

// standard-form limbs
__device__ __forceinline__ bool limbs_below(const uint32_t a[8], const uint32_t m[8]) {   // a < m
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) br = ((int64_t)a[i] - (int64_t)m[i] + br) >> 32;
  return br != 0;
}
__device__ __forceinline__ bool fq_below_q(const Fq& s) { return limbs_below(s.v, FqParams::P); }
__device__ __forceinline__ bool fq_negative(const Fq& s) { return limbs_below(QC::K.half, s.v); }   // s > (q - 1) / 2
__device__ __forceinline__ bool y_negative(const Fq& ys) { return fq_negative(ys); }
__device__ __forceinline__ bool y_negative(const Fq2& ys) { return fp_is_zero(ys.b) ? fq_negative(ys.a) : fq_negative(ys.b); }

template <class FC> __device__ __forceinline__ typename FC::T curve_b();
template <> __device__ __forceinline__ Fq curve_b<FqOps>() {
  const Fq one = fp_one<FqParams>();
  return fp_add(fp_add(one, one), one);
}
template <> __device__ __forceinline__ Fq2 curve_b<Fq2Ops>() { return Fq2{Fq{G16_G2B_C0}, Fq{G16_G2B_C1}}; }
template <class FC> __device__ __forceinline__ typename FC::T curve_rhs(const typename FC::T& x) {   // x^3 + b
  return FC::add(FC::mul(FC::sqr(x), x), curve_b<FC>());
}

template <class FC>
__global__ __launch_bounds__(kBlock) void ptau_from_be_kernel(const uint32_t* __restrict__ in, Affine<FC>* __restrict__ out,
                                                              uint32_t n, uint32_t base, uint32_t* __restrict__ bad) {
  constexpr int NC = sizeof(Affine<FC>) / 32;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t* p = in + (size_t)i * NC * 8;
    Affine<FC> P;
    Fq* co = reinterpret_cast<Fq*>(&P);
    uint32_t any = 0;   // every bit of the image but the two flags
#pragma unroll
    for (int c = 0; c < NC; c++) {
      Fq s = load_be(p + c * 8);
      if (c == 0) s.v[7] &= 0x3fffffffu;
#pragma unroll
      for (int w = 0; w < 8; w++) any |= s.v[w];
      co[be_slot<NC>(c)] = s;
    }
    const uint32_t flags = p[0] & 0xc0u;
    bool ok;
    if (flags) {
      ok = flags == 0x40u && any == 0;   // infinity, and nothing else in the image (P is zero then)
    } else {
      ok = true;
#pragma unroll
      for (int c = 0; c < NC; c++) {
        ok = ok && fq_below_q(co[c]);
        co[c] = fp_to_mont(co[c]);
      }
      ok = ok && FC::eq(FC::sqr(P.y), curve_rhs<FC>(P.x));
    }
    if (!ok) {
      atomicMin(bad, base + i);
      P.x = FC::zero(); P.y = FC::zero();
    }
    out[i] = P;
  }
}

template <class FC>
__global__ __launch_bounds__(kBlock) void ptau_to_be_kernel(const Affine<FC>* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  constexpr int NC = sizeof(Affine<FC>) / 32;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Affine<FC> P = in[i];
    const Fq* co = reinterpret_cast<const Fq*>(&P);
    uint32_t* o = out + (size_t)i * NC * 8;
    if (aff_is_inf(P)) {
      store_inf(o, NC * 8);
      continue;
    }
#pragma unroll
    for (int c = 0; c < NC; c++) store_be(o + c * 8, fp_from_mont(co[be_slot<NC>(c)]));
  }
}

template <class FC>
__global__ __launch_bounds__(kBlock) void ptau_compress_kernel(const Affine<FC>* __restrict__ in, uint32_t* __restrict__ out,
                                                               uint32_t n) {
  constexpr int NX = sizeof(Affine<FC>) / 64;   // coordinates of x
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Affine<FC> P = in[i];
    uint32_t* o = out + (size_t)i * NX * 8;
    if (aff_is_inf(P)) {
      store_inf(o, NX * 8);
      continue;
    }
    const Fq* xc = reinterpret_cast<const Fq*>(&P.x);
    const Fq* yc = reinterpret_cast<const Fq*>(&P.y);
    typename FC::T ys;
    Fq* ysc = reinterpret_cast<Fq*>(&ys);
    uint32_t first = 0;
#pragma unroll
    for (int c = 0; c < NX; c++) {
      ysc[c] = fp_from_mont(yc[c]);
      const Fq s = fp_from_mont(xc[be_slot<2 * NX>(c)]);
      if (c == 0) first = __builtin_bswap32(s.v[7]);
      store_be(o + c * 8, s);
    }
    if (y_negative(ys)) o[0] = first | 0x80u;
  }
}

template <class FC>
__global__ __launch_bounds__(kBlock) void ptau_decompress_kernel(const uint32_t* __restrict__ in, Affine<FC>* __restrict__ out,
                                                                 uint32_t* __restrict__ out_be, uint32_t n, uint32_t base,
                                                                 uint32_t* __restrict__ bad) {
  constexpr int NX = sizeof(Affine<FC>) / 64;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint32_t* p = in + (size_t)i * NX * 8;
    Affine<FC> P;
    P.y = FC::zero();
    Fq* xc = reinterpret_cast<Fq*>(&P.x);
    Fq xs[NX];   // x in standard form, in the image's order
    uint32_t any = 0;
#pragma unroll
    for (int c = 0; c < NX; c++) {
      xs[c] = load_be(p + c * 8);
      if (c == 0) xs[c].v[7] &= 0x3fffffffu;
#pragma unroll
      for (int w = 0; w < 8; w++) any |= xs[c].v[w];
    }
    const uint32_t flags = p[0] & 0xc0u;
    typename FC::T ys = FC::zero();
    bool ok, inf = false;
    if (flags & 0x40u) {
      ok = inf = flags == 0x40u && any == 0;
    } else {
      ok = true;
#pragma unroll
      for (int c = 0; c < NX; c++) {
        ok = ok && fq_below_q(xs[c]);
        xc[be_slot<2 * NX>(c)] = fp_to_mont(xs[c]);
      }
      typename FC::T y;
      ok = field_sqrt(curve_rhs<FC>(P.x), y) && ok;
      Fq* yc = reinterpret_cast<Fq*>(&y);
      Fq* ysc = reinterpret_cast<Fq*>(&ys);
#pragma unroll
      for (int c = 0; c < NX; c++) ysc[c] = fp_from_mont(yc[c]);
      if (y_negative(ys) != ((flags & 0x80u) != 0)) {
        y = FC::neg(y);
        ys = FC::neg(ys);
      }
      P.y = y;
    }
    if (!ok) atomicMin(bad, base + i);
    if (!ok || inf) {
      P.x = FC::zero(); P.y = FC::zero();
    }
    out[i] = P;
    if (out_be) {
      uint32_t* o = out_be + (size_t)i * NX * 16;
      if (!ok || inf) {
        store_inf(o, NX * 16);
      } else {
        const Fq* ysc = reinterpret_cast<const Fq*>(&ys);
#pragma unroll
        for (int c = 0; c < NX; c++) {
          store_be(o + c * 8, xs[c]);
          store_be(o + (NX + c) * 8, ysc[be_slot<2 * NX>(c)]);
        }
      }
    }
  }
}

// TEST-ONLY: square roots of raw field elements (standard little-endian form in and out; Fq2 = c0 | c1)
template <class FC>
__global__ __launch_bounds__(kBlock) void fq_sqrt_kernel(const typename FC::T* __restrict__ in, typename FC::T* __restrict__ out,
                                                         uint8_t* __restrict__ has_root, uint32_t n) {
  constexpr int NX = sizeof(typename FC::T) / 32;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    typename FC::T a = in[i], r;
    Fq* ac = reinterpret_cast<Fq*>(&a);
    Fq* rc = reinterpret_cast<Fq*>(&r);
#pragma unroll
    for (int c = 0; c < NX; c++) ac[c] = fp_to_mont(ac[c]);
    const bool ok = field_sqrt(a, r);
#pragma unroll
    for (int c = 0; c < NX; c++) rc[c] = ok ? fp_from_mont(rc[c]) : fp_zero<FqParams>();
    out[i] = r;
    has_root[i] = ok ? 1 : 0;
  }
}

// n items of in_sz bytes (host) through launch(grid, block, stream, d_in, d_out, d_out2, cnt, base, d_bad) into out
// (out_sz bytes each) and -- when out2 -- out2 (out2_sz each); *first_bad = the device word after the last chunk, or -1
template <class Launch>
int points_device(const char* what, int device, const uint8_t* in, size_t in_sz, uint64_t n, uint8_t* out, size_t out_sz,
                  uint8_t* out2, size_t out2_sz, int64_t* first_bad, ChunkStats* st, Launch launch,
                  const ChunkSink* sink = nullptr) {
  if (first_bad) *first_bad = -1;
  if (st) *st = ChunkStats{};
  if (n >= ((uint64_t)1 << 31)) { set_error(std::string(what) + ": more than 2^31 items"); return G16_E_ARG; }
  if (const int rc = require_hip_device(what, device)) return rc;
  if (n == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  const ChunkPlan plan = chunk_plan("G16_PTAU_CHUNK", "G16_PTAU_LANES", n, 0);

  DeviceBuf<uint32_t> bad;
  uint32_t h_bad = kNoBad;
  ChunkPipeline pipe(what);
  if (!pipe.open(n, plan.chunk, in_sz, out_sz, out2 ? out2_sz : 0) || pipe.fail(bad.alloc(1)) ||
      pipe.fail(hipMemcpyAsync(bad.p, &h_bad, sizeof(uint32_t), hipMemcpyHostToDevice, pipe.stream())))
    return pipe.rc;
  const ChunkPipeline::Sink landed = [&](uint64_t lo, uint32_t cnt) { (*sink)(out + lo * out_sz, (size_t)cnt * out_sz); };
  const int rc = pipe.run(in, out, out2, st, [&](hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t* o2, uint32_t cnt, uint64_t lo) {
    launch(plan.grid(cnt), plan.block, s, i, o, o2, cnt, (uint32_t)lo, bad.p);
  }, sink ? &landed : nullptr);
  if (rc) return rc;
  if (pipe.fail(hipMemcpy(&h_bad, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost))) {
    if (st) *st = ChunkStats{};
    return pipe.rc;
  }
  if (first_bad && h_bad != kNoBad) *first_bad = (int64_t)h_bad;
  return G16_OK;
}

template <class FC>
int from_be(int device, const uint8_t* in, uint64_t n, uint8_t* out, int64_t* first_bad, ChunkStats* st) {
  constexpr size_t PSZ = sizeof(Affine<FC>);
  return points_device("ptau points from-be", device, in, PSZ, n, out, PSZ, nullptr, 0, first_bad, st,
                       [](uint32_t grid, uint32_t block, hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t*, uint32_t cnt,
                          uint32_t base, uint32_t* bad) {
                         ptau_from_be_kernel<FC><<<grid, block, 0, s>>>((const uint32_t*)i, (Affine<FC>*)o, cnt, base, bad);
                       });
}
template <class FC> int to_be(int device, const uint8_t* in, uint64_t n, uint8_t* out, ChunkStats* st, const ChunkSink* sink) {
  constexpr size_t PSZ = sizeof(Affine<FC>);
  return points_device("ptau points to-be", device, in, PSZ, n, out, PSZ, nullptr, 0, nullptr, st,
                       [](uint32_t grid, uint32_t block, hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t*, uint32_t cnt, uint32_t,
                          uint32_t*) { ptau_to_be_kernel<FC><<<grid, block, 0, s>>>((const Affine<FC>*)i, (uint32_t*)o, cnt); },
                       sink);
}
template <class FC> int compress(int device, const uint8_t* in, uint64_t n, uint8_t* out, ChunkStats* st) {
  constexpr size_t PSZ = sizeof(Affine<FC>);
  return points_device("ptau points compress", device, in, PSZ, n, out, PSZ / 2, nullptr, 0, nullptr, st,
                       [](uint32_t grid, uint32_t block, hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t*, uint32_t cnt, uint32_t,
                          uint32_t*) { ptau_compress_kernel<FC><<<grid, block, 0, s>>>((const Affine<FC>*)i, (uint32_t*)o, cnt); });
}
template <class FC>
int decompress(int device, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* out_be, int64_t* first_bad, ChunkStats* st) {
  constexpr size_t PSZ = sizeof(Affine<FC>);
  return points_device("ptau points decompress", device, in, PSZ / 2, n, out, PSZ, out_be, PSZ, first_bad, st,
                       [](uint32_t grid, uint32_t block, hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t* o2, uint32_t cnt,
                          uint32_t base, uint32_t* bad) {
                         ptau_decompress_kernel<FC><<<grid, block, 0, s>>>((const uint32_t*)i, (Affine<FC>*)o, (uint32_t*)o2, cnt, base, bad);
                       });
}
template <class FC> int sqrt_batch(int device, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* has_root) {
  constexpr size_t ESZ = sizeof(typename FC::T);
  return points_device("fq sqrt batch", device, in, ESZ, n, out, ESZ, has_root, 1, nullptr, nullptr,
                       [](uint32_t grid, uint32_t block, hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t* o2, uint32_t cnt, uint32_t,
                          uint32_t*) {
                         fq_sqrt_kernel<FC><<<grid, block, 0, s>>>((const typename FC::T*)i, (typename FC::T*)o, o2, cnt);
                       });
}

}  // namespace

int ptau_points_from_be(int device, bool g2, const uint8_t* in, uint64_t n, uint8_t* out, int64_t* first_bad, ChunkStats* st) {
  return g2 ? from_be<Fq2Ops>(device, in, n, out, first_bad, st) : from_be<FqOps>(device, in, n, out, first_bad, st);
}
int ptau_points_to_be(int device, bool g2, const uint8_t* in, uint64_t n, uint8_t* out, ChunkStats* st, const ChunkSink* sink) {
  return g2 ? to_be<Fq2Ops>(device, in, n, out, st, sink) : to_be<FqOps>(device, in, n, out, st, sink);
}
int ptau_points_compress(int device, bool g2, const uint8_t* in, uint64_t n, uint8_t* out, ChunkStats* st) {
  return g2 ? compress<Fq2Ops>(device, in, n, out, st) : compress<FqOps>(device, in, n, out, st);
}
int ptau_points_decompress(int device, bool g2, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* out_be, int64_t* first_bad,
                           ChunkStats* st) {
  return g2 ? decompress<Fq2Ops>(device, in, n, out, out_be, first_bad, st) : decompress<FqOps>(device, in, n, out, out_be, first_bad, st);
}

}  // namespace g16

using namespace g16;

namespace {
bool layer_args(const char* what, int group, const void* in, const void* out) {
  if (!in || !out) { set_error("NULL argument"); return false; }
  if (group != 1 && group != 2) { set_error(std::string(what) + ": group is 1 (G1) or 2 (G2)"); return false; }
  return true;
}
}  // namespace

extern "C" int g16_ptau_points_from_be(int group, const uint8_t* in, size_t n, int device, uint8_t* out, int64_t* first_bad,
                                       float* kernel_ms) {
  if (!layer_args("ptau points from-be", group, in, out)) return G16_E_ARG;
  ChunkStats st;
  const int rc = ptau_points_from_be(device, group == 2, in, n, out, first_bad, &st);
  if (kernel_ms) *kernel_ms = st.kern_ms;
  return rc;
}
extern "C" int g16_ptau_points_compress(int group, const uint8_t* in, size_t n, int device, uint8_t* out, int64_t* first_bad,
                                        float* kernel_ms) {
  if (!layer_args("ptau points compress", group, in, out)) return G16_E_ARG;
  if (first_bad) *first_bad = -1;   // (every file image has a compressed form)
  ChunkStats st;
  const int rc = ptau_points_compress(device, group == 2, in, n, out, &st);
  if (kernel_ms) *kernel_ms = st.kern_ms;
  return rc;
}
extern "C" int g16_ptau_points_decompress(int group, const uint8_t* in, size_t n, int device, uint8_t* out, uint8_t* out_be,
                                          int64_t* first_bad, float* kernel_ms) {
  if (!layer_args("ptau points decompress", group, in, out)) return G16_E_ARG;
  ChunkStats st;
  const int rc = ptau_points_decompress(device, group == 2, in, n, out, out_be, first_bad, &st);
  if (kernel_ms) *kernel_ms = st.kern_ms;
  return rc;
}
extern "C" int g16_fq_sqrt_batch(int ext, const uint8_t* in, size_t n, int device, uint8_t* out, uint8_t* has_root) {
  if (!in || !out || !has_root) { set_error("NULL argument"); return G16_E_ARG; }
  if (ext != 0 && ext != 1) { set_error("fq sqrt batch: ext is 0 (Fq) or 1 (Fq2)"); return G16_E_ARG; }
  const size_t words = n * (ext ? 2 : 1);
  for (size_t k = 0; k < words; k++) {
    uint32_t v[8];
    memcpy(v, in + 32 * k, 32);
    bool below = false;
    for (int i = 7; i >= 0; i--)
      if (v[i] != kFqP[i]) { below = v[i] < kFqP[i]; break; }
    if (!below) { set_error("fq sqrt batch: an element is not below q"); return G16_E_ARG; }
  }
  return ext ? sqrt_batch<Fq2Ops>(device, in, n, out, has_root) : sqrt_batch<FqOps>(device, in, n, out, has_root);
}
