// Inverse Fourier transform over group elements on the device: `snarkjs powersoftau prepare phase2`
// (ptau.cpp::g16_ptau_prepare).  One call transforms one section of a .ptau file:
//   block k (k = 0 .. kmax, 2^k points, first point 2^k - 1) holds  out_j = (1/2^k) sum_{i<2^k} w_k^(-ij) P_i
// with P_i the i-th point of the source section (infinity from index nsrc on: the top block of section 12 has one
// input less than points) and w_k = the 2^k-th root of unity of oracle/groth16.py::fr_root (w_k = w_{k+1}^2).
//
// All blocks live in ONE device array in the file's own layout (block k at 2^k - 1), so a stage is one launch over
// every block that has it and the result is copied out as it stands:
//   pp_load_kernel   work[block k][j] = P_bitrev_k(j)                           (affine file bytes -> XYZZ)
//   stage s = 0 .. kmax - 1, blocks k > s (radix-2 decimation in time, natural order out):
//     pp_mul_kernel  b <- [w_{s+1}^(-pos)] b  for the upper operand of every butterfly with pos != 0 (s >= 1)
//     pp_bfly_kernel (a, b) <- (a + b, a - b)
//   pp_mul_kernel    block k <- [2^-k] block k                                  (k >= 1)
//   setup_to_affine_kernel (setup_affine.cuh), then one copy to the host.
// The twiddle of a butterfly depends on (s, pos) alone, not on its block: one table w_kmax^(-i), i < 2^(kmax - 1),
// standard form, serves every stage (entry pos << (kmax - 1 - s)).  pp_mul_kernel numbers its lanes with pos in the
// HIGH bits of a block's range: a wavefront then shares one twiddle (one digit pattern, no divergence on zero
// digits) and the pos = 0 lanes, which need no product, are whole wavefronts that leave at once.  The strided point
// accesses this costs do not matter: a product is ~3500 field multiplications on 128 / 256 bytes.
//
// The product (pp_scalar_mul, scalar_mul.cuh) is sp_full_kernel's (setup_ptau.hip) signed 3-bit fixed window -- digits -3..4, 254 doublings + at most
// 85 additions + 3 for the table [1..4]P -- over a projective base.  A lane's table lives in global memory, one slot
// per lane of a fixed persistent grid (grid-stride loop), not in LDS: 4 x 256 B per G2 lane would cap a workgroup at
// one wavefront.  Exact canonical arithmetic (fp.cuh / ec.cuh): the XYZZ formulas there are complete (infinity
// operands, equal operands -> doubling, opposite operands -> infinity), which tau = 1 or a root of unity exercises in
// every butterfly, and the affine result is unique, so the bytes equal the oracle's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "ec.cuh"
#include "internal.h"
#include "scalar_mul.cuh"
#include "setup_affine.cuh"

namespace g16 {
namespace {

constexpr int kWin = 3, kTbl = 1 << (kWin - 1);
constexpr int kMulBlock = 256;

// element t of the block layout: block k = floor(log2(t + 1)), point j = t + 1 - 2^k
__device__ __forceinline__ int block_of(uint32_t t) { return 31 - __clz(t + 1); }

template <class FC>
__global__ __launch_bounds__(256) void pp_load_kernel(const Affine<FC>* __restrict__ src, uint32_t nsrc, uint32_t total,
                                                      XYZZ<FC>* __restrict__ work) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int k = block_of(t);
  const uint32_t j = t + 1 - (1u << k);
  const uint32_t i = k ? __brev(j) >> (32 - k) : 0u;
  XYZZ<FC> p;
  if (i < nsrc) xyzz_from_affine(p, src[i]);
  else xyzz_set_inf(p);
  work[t] = p;
}

// Lane t of n (grid-stride).  s >= 1, the twiddle products of stage s: v = t + 2^s, block k = floor(log2 v) + 1,
// tb = v - 2^(k-1) in [0, 2^(k-1)) numbers the block's butterflies with pos = tb >> (k-1-s) on top and the group g
// below; the operand is point (g << (s+1)) + 2^s + pos of the block and the scalar sc[pos << tw_shift].
// s < 0, the scaling: element t + 1 (block k >= 1) times sc[k].
template <class FC>
__global__ __launch_bounds__(kMulBlock) void pp_mul_kernel(XYZZ<FC>* __restrict__ work, const Fr* __restrict__ sc, uint32_t n,
                                                           int s, int tw_shift, XYZZ<FC>* __restrict__ tbl) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t t = gid; t < n; t += stride) {
    uint32_t e, si;
    if (s >= 0) {
      const uint32_t v = t + (1u << s);
      const int k1 = 31 - __clz(v);
      const uint32_t tb = v - (1u << k1);
      const uint32_t pos = tb >> (k1 - s), g = tb & ((1u << (k1 - s)) - 1);
      if (pos == 0) continue;
      e = ((2u << k1) - 1) + (g << (s + 1)) + (1u << s) + pos;
      si = pos << tw_shift;
    } else {
      e = t + 1;
      si = (uint32_t)block_of(e);
    }
    const XYZZ<FC> base = work[e];
    XYZZ<FC> acc;
    pp_scalar_mul<FC, kWin>(acc, base, sc[si].v, tbl + gid, stride);
    work[e] = acc;
  }
}

// stage s, one lane per butterfly of every block k > s: v = t + 2^s, block k = floor(log2 v) + 1, butterfly
// b = v - 2^(k-1) = g << s | pos
template <class FC>
__global__ __launch_bounds__(256) void pp_bfly_kernel(XYZZ<FC>* __restrict__ work, uint32_t n, int s) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t v = t + (1u << s);
  const int k1 = 31 - __clz(v);
  const uint32_t b = v - (1u << k1);
  const uint32_t pos = b & ((1u << s) - 1), g = b >> s;
  const uint32_t i0 = ((2u << k1) - 1) + (g << (s + 1)) + pos, i1 = i0 + (1u << s);
  const XYZZ<FC> x = work[i0];
  XYZZ<FC> y = work[i1];
  XYZZ<FC> sum = x, diff = x;
  xyzz_add(sum, y);
  xyzz_neg(y);
  xyzz_add(diff, y);
  work[i0] = sum;
  work[i1] = diff;
}

Fr root_of_unity(int k) {   // order 2^k, Montgomery form (oracle/groth16.py::fr_root)
  Fr w = {G16_FR_W28};
  for (int i = 28; i > k; i--) w = fp_sqr(w);
  return w;
}

template <class FC>
int prepare_device(int device, const uint8_t* src, uint64_t nsrc, int kmax, uint8_t* out, PtauPrepareStats* stats) {
  if (kmax < 0 || kmax > 26) { set_error("ptau prepare: bad block count"); return G16_E_ARG; }
  const uint32_t total = (2u << kmax) - 1;   // points of blocks 0 .. kmax
  if (nsrc == 0 || nsrc > ((uint64_t)1 << kmax)) { set_error("ptau prepare: bad source length"); return G16_E_ARG; }
  if (const int rc = require_hip_device("ptau prepare", device)) return rc;
  G16_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  G16_HIP(hipGetDeviceProperties(&prop, device));

  // scalars, standard form: sc[0, ntw) = w_kmax^(-i); sc[ntw + k] = 2^(-k)
  const uint32_t ntw = kmax >= 1 ? 1u << (kmax - 1) : 0u;
  std::vector<Fr> sc((size_t)ntw + kmax + 1);
  {
    const Fr winv = fp_inv(root_of_unity(kmax));
    Fr x = fp_one<FrParams>();
    for (uint32_t i = 0; i < ntw; i++) { sc[i] = fp_from_mont(x); x = fp_mul(x, winv); }
    Fr two = fp_one<FrParams>();
    two = fp_add(two, two);
    const Fr half = fp_inv(two);
    x = fp_one<FrParams>();
    for (int k = 0; k <= kmax; k++) { sc[ntw + k] = fp_from_mont(x); x = fp_mul(x, half); }
  }
  // persistent grid of the products: four wavefronts per SIMD at most
  const uint32_t max_mul = std::max(total, 1u);
  const uint32_t grid_cap = (uint32_t)std::max(prop.multiProcessorCount, 1) * 4;
  const uint32_t mul_blocks = std::min(grid_cap, (max_mul + kMulBlock - 1) / kMulBlock);
  const size_t mul_lanes = (size_t)mul_blocks * kMulBlock;

  DeviceJob job("ptau prepare");
  DeviceBuf<Affine<FC>> d_src, d_aff;
  DeviceBuf<XYZZ<FC>> d_work, d_tbl;
  DeviceBuf<Fr> d_sc;
  DeviceTimer timer;
  DeviceStream st;
  uint64_t muls = 0, adds = 0;
  if (job.fail(st.create()) || job.fail(timer.create()) || job.fail(d_src.alloc(nsrc)) || job.fail(d_work.alloc(total)) ||
      job.fail(d_aff.alloc(total)) || job.fail(d_tbl.alloc(mul_lanes * kTbl)) || job.fail(d_sc.alloc(sc.size())) ||
      job.fail(hipMemcpyAsync(d_src.p, src, nsrc * sizeof(Affine<FC>), hipMemcpyHostToDevice, st)) ||
      job.fail(hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(Fr), hipMemcpyHostToDevice, st)) || job.fail(timer.start(st)))
    return job.rc;
  pp_load_kernel<FC><<<(total + 255) / 256, 256, 0, st>>>(d_src.p, (uint32_t)nsrc, total, d_work.p);
  for (int s = 0; s < kmax; s++) {
    const uint32_t n = (1u << kmax) - (1u << s);   // butterflies of stage s over blocks s + 1 .. kmax
    if (s >= 1) {
      pp_mul_kernel<FC><<<std::min(mul_blocks, (n + kMulBlock - 1) / kMulBlock), kMulBlock, 0, st>>>(d_work.p, d_sc.p, n, s,
                                                                                                     kmax - 1 - s, d_tbl.p);
      for (int k = s + 1; k <= kmax; k++) muls += ((uint64_t)1 << (k - 1)) - ((uint64_t)1 << (k - 1 - s));
    }
    pp_bfly_kernel<FC><<<(n + 255) / 256, 256, 0, st>>>(d_work.p, n, s);
    adds += 2 * (uint64_t)n;
  }
  if (kmax >= 1) {
    const uint32_t n = total - 1;
    pp_mul_kernel<FC><<<std::min(mul_blocks, (n + kMulBlock - 1) / kMulBlock), kMulBlock, 0, st>>>(d_work.p, d_sc.p + ntw, n, -1, 0,
                                                                                                   d_tbl.p);
    muls += n;
  }
  const uint32_t nb = (total + kBatch - 1) / kBatch;
  setup_to_affine_kernel<FC><<<(nb + 255) / 256, 256, 0, st>>>(d_work.p, d_aff.p, total);
  if (job.fail(hipGetLastError()) || job.fail(timer.stop(st)) ||
      job.fail(hipMemcpyAsync(out, d_aff.p, (size_t)total * sizeof(Affine<FC>), hipMemcpyDeviceToHost, st)) ||
      job.fail(hipStreamSynchronize(st)))
    return job.rc;
  if (stats) {
    stats->kern_ms = timer.ms();
    stats->muls = muls;
    stats->adds = adds;
  }
  return G16_OK;
}

}  // namespace

int ptau_prepare_g1(int device, const uint8_t* src, uint64_t nsrc, int kmax, uint8_t* out, PtauPrepareStats* st) {
  return prepare_device<FqOps>(device, src, nsrc, kmax, out, st);
}
int ptau_prepare_g2(int device, const uint8_t* src, uint64_t nsrc, int kmax, uint8_t* out, PtauPrepareStats* st) {
  return prepare_device<Fq2Ops>(device, src, nsrc, kmax, out, st);
}

}  // namespace g16
