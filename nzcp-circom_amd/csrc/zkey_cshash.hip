// The monomial H points of `zkey new`'s circuit hash (zkey_cshash_host.cpp; [EXT] snarkjs 0.4.12 zkey_new.js hashHPoints,
// restated from its description): with P_j = [tau^j] G1 the points of a ceremony's section 2 and N = 2^L the key's domain,
//   H_k = P_(k+N) - P_k = [tau^k (tau^N - 1)] G1,   k < N - 1,
// written straight into the form the hash is taken over: uncompressed big-endian standard form, x | y, infinity = 0x40
// and zeros (the image rules of ptau_to_be_kernel, ptau_points.hip).  Section 9 of the key is not read: this is the
// second device route to the bytes `zkey export bellman` derives from section 9 by its basis change (zkey_bellman.hip),
// and the two share no code beyond fp.cuh and the big-endian store.
//
// h_monomial_kernel: a batched AFFINE subtraction.  One lane owns a run of kHBatch consecutive k (as
// setup_to_affine_kernel owns kBatch points) and inverts the denominators of its run with ONE Fermat inversion
// (Montgomery's trick), then forms lambda, x3, y3 and stores big-endian: no XYZZ intermediate, no second pass.
// With A = P_(k+N), B = P_k, the sum A + (-B):
//   ordinary    x_A != x_B            lambda = (y_A + y_B) / (x_A - x_B)
//   doubling    A = -B  (opposite)    lambda = 3 x_A^2 / (2 y_A)           every k when tau^N = -1
//   infinity    A = B   (equal)                                            every k when tau^N = 1 (tau = 1: powersoftau new)
//   one operand infinity: the other operand, B negated; both: infinity
//   x3 = lambda^2 - x_A - x_B,  y3 = lambda (x_A - x3) - y_A
// Only ordinary and doubling entries have a denominator, and only theirs enter the running product, so a run may mix
// all five kinds.  (A denominator 2 y_A = 0 cannot occur on this curve -- its group has odd prime order -- and for
// unchecked input that claims it the entry is written as infinity instead of poisoning the run.)
// A run's kinds and denominators are formed twice, on the way up and on the way down, from the same loads: the second
// pass re-reads its operands from cache instead of keeping kHBatch points in registers beside the prefix products.
// Cost per point: ~48 products of the shared inversion (380 / 8) + ~12 of its own.  Canonical fp.cuh arithmetic, so the
// bytes are unique.
//
// Run through the chunked pipeline (chunk_pipeline.h) with its second input range: a chunk of k needs P[lo, lo + cnt)
// and P[lo + N, lo + N + cnt), two copies up per chunk.  G16_CSHASH_CHUNK / G16_CSHASH_LANES override the chunk and the
// grid (lanes = threads, each owning runs grid-stride).  Runs are cut inside a chunk, from its first k; how the k are
// grouped changes no byte.
// As built for gfx950: 188 VGPRs, 0 B scratch.  Measured on one MI355X at L = 20 (tools/zkey_new_bench.py, kernel events;
// DESIGN.md 3.7b): 2.04 ms for 1 048 575 points, 1.9 ns per point, behind a hash that takes 236 ms.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "chunk_pipeline.h"
#include "ec.cuh"
#include "internal.h"
#include "ptau_be.cuh"

namespace g16 {
namespace {

constexpr int kHBatch = 8;
constexpr int kMaxLog = 24;

enum : int { kInf = 0, kTakeA = 1, kTakeNegB = 2, kAdd = 3, kDbl = 4 };

// the kind of A - B and, for kAdd / kDbl, its denominator
__device__ __forceinline__ int h_kind(const G1Affine& A, const G1Affine& B, Fq& den) {
  const bool ainf = aff_is_inf(A), binf = aff_is_inf(B);
  if (ainf) return binf ? kInf : kTakeNegB;
  if (binf) return kTakeA;
  if (!fp_eq(A.x, B.x)) {
    den = fp_sub(A.x, B.x);
    return kAdd;
  }
  if (fp_eq(A.y, B.y)) return kInf;
  den = fp_add(A.y, A.y);
  return fp_is_zero(den) ? kInf : kDbl;
}

// the way up: pref[e] = the product of the denominators before entry e.  Unrolled by recursion: the compiler declines
// to unroll the loop form in full ("unrolled size is too large"), and a run-time index would put pref into scratch.
template <int E>
__device__ __forceinline__ void h_prefix(Fq (&pref)[kHBatch], Fq& acc, const G1Affine* __restrict__ lo,
                                         const G1Affine* __restrict__ hi, uint32_t cnt) {
  pref[E] = acc;
  if ((uint32_t)E < cnt) {
    Fq den;
    if (h_kind(hi[E], lo[E], den) >= kAdd) acc = fp_mul(acc, den);
  }
  if constexpr (E + 1 < kHBatch) h_prefix<E + 1>(pref, acc, lo, hi, cnt);
}

__global__ __launch_bounds__(256) void h_monomial_kernel(const G1Affine* __restrict__ lo, const G1Affine* __restrict__ hi,
                                                         uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t nruns = (n + kHBatch - 1) / kHBatch, stride = gridDim.x * blockDim.x;
  for (uint32_t run = blockIdx.x * blockDim.x + threadIdx.x; run < nruns; run += stride) {
    const uint32_t k0 = run * kHBatch;
    const uint32_t cnt = n - k0 < (uint32_t)kHBatch ? n - k0 : (uint32_t)kHBatch;
    Fq pref[kHBatch];
    Fq acc = fp_one<FqParams>();
    h_prefix<0>(pref, acc, lo + k0, hi + k0, cnt);
    Fq inv = fp_inv(acc);
#pragma unroll
    for (int e = kHBatch - 1; e >= 0; e--) {
      if ((uint32_t)e >= cnt) continue;
      const G1Affine A = hi[k0 + e], B = lo[k0 + e];
      uint32_t* o = out + (size_t)(k0 + e) * 16;
      Fq den, x3, y3;
      const int kind = h_kind(A, B, den);
      if (kind == kInf) {
        store_inf(o, 16);
        continue;
      }
      if (kind == kTakeA) {
        x3 = A.x; y3 = A.y;
      } else if (kind == kTakeNegB) {
        x3 = B.x; y3 = fp_neg(B.y);
      } else {
        const Fq di = fp_mul(inv, pref[e]);
        inv = fp_mul(inv, den);
        Fq num;
        if (kind == kAdd) {
          num = fp_add(A.y, B.y);
        } else {
          const Fq xx = fp_sqr(A.x);
          num = fp_add(fp_add(xx, xx), xx);
        }
        const Fq lambda = fp_mul(num, di);
        x3 = fp_sub(fp_sub(fp_sqr(lambda), A.x), B.x);
        y3 = fp_sub(fp_mul(lambda, fp_sub(A.x, x3)), A.y);
      }
      store_be(o, fp_from_mont(x3));
      store_be(o + 8, fp_from_mont(y3));
    }
  }
}

}  // namespace

int zkey_h_monomial(int device, const uint8_t* points, int L, uint8_t* out, ChunkStats* st, const ChunkSink* sink) {
  if (st) *st = ChunkStats{};
  if (L < 0 || L > kMaxLog) { set_error("zkey h monomial: log_n out of range (need 0..24)"); return G16_E_ARG; }
  if (const int rc = require_hip_device("zkey h monomial", device)) return rc;
  const uint64_t N = (uint64_t)1 << L, n = N - 1;
  if (n == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  const ChunkPlan plan = chunk_plan("G16_CSHASH_CHUNK", "G16_CSHASH_LANES", n, 0);

  ChunkPipeline pipe("zkey h monomial");
  pipe.second(N);
  if (!pipe.open(n, plan.chunk, sizeof(G1Affine), 64, 0)) return pipe.rc;
  const ChunkPipeline::Sink landed = [&](uint64_t lo, uint32_t cnt) { (*sink)(out + lo * 64, (size_t)cnt * 64); };
  return pipe.run(points, out, nullptr, st, [&](hipStream_t s, const uint8_t* i, uint8_t* o, uint8_t*, uint32_t cnt, uint64_t) {
    const uint32_t nruns = (cnt + kHBatch - 1) / kHBatch;   // a lane per run, no more than the plan's lanes
    const uint32_t grid = std::min(plan.lanes / plan.block, (nruns + plan.block - 1) / plan.block);
    h_monomial_kernel<<<grid, plan.block, 0, s>>>((const G1Affine*)i, (const G1Affine*)(i + (size_t)plan.chunk * sizeof(G1Affine)),
                                                 (uint32_t*)o, cnt);
  }, sink ? &landed : nullptr);
}

}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_h_monomial(int device, const uint8_t* points, uint32_t log_n, uint8_t* out) {
  if (!points || (!out && log_n)) { set_error("NULL argument"); return G16_E_ARG; }
  if (log_n > (uint32_t)kMaxLog) { set_error("zkey h monomial: log_n out of range (need 0..24)"); return G16_E_ARG; }
  return no_bad_alloc("zkey h monomial", [&]() { return zkey_h_monomial(device, points, (int)log_n, out, nullptr); });
}
