// The H basis change of the phase-2 file exchange (`snarkjs zkey export bellman` / `zkey import bellman`;
// zkey_bellman_host.cpp): a Fourier transform of ONE size N = 2^L over G1 points with a twist per point, both directions.
//   S9[i] = point i of a key's section 9 = [L^{2N}_{2i+1}(tau) / delta] G   (odd-coset Lagrange basis)
//   T[k]  = [tau^k (tau^N - 1) / delta] G                                    (monomial basis, the MPCParams file's H)
// With w = the primitive 2N-th root of unity (oracle/groth16.py::fr_root(L + 1)) and W = w^2:
//   forward   T[k]  = [-2 w^k] sum_{i<N} W^(ik) S9[i]                         k < N (T[N-1] is NOT infinity in general)
//   inverse   S9[i] = (1/N) sum_{k<N} W^(-ik) [-(1/2) w^(-k)] T[k]
// Radix-2 decimation in time, natural order out, as ptau_prepare.hip does for all its blocks at once; here one block:
//   hb_load_kernel   work[j] = P_bitrev(j)                                    (affine file bytes -> XYZZ)
//   inverse only     hb_twist_kernel  work[j] <- [-(1/2N) w^(-bitrev(j))] work[j]   (twist and 1/N: ONE product per point)
//   stage s = 0 .. L - 1:
//     hb_mul_kernel  b <- [W_{2^(s+1)}^(+-pos)] b  for the upper operand of every butterfly with pos != 0 (s >= 1)
//     hb_bfly_kernel (a, b) <- (a + b, a - b)
//   forward only     hb_twist_kernel  work[k] <- [-2 w^k] work[k]
//   setup_to_affine_kernel (setup_affine.cuh), then one copy to the host.
// At L = 0 the transform is the twist alone.  Products: N + sum_{s>=1} (N/2 - N/2^(s+1)) < N + L N/2.
//
// Scalars.  One table tw[i] = W^(+-i), i < N/2, standard form, serves every stage (entry pos << (L - 1 - s)) AND the
// twist: w^(+-k) = tw[k >> 1] times (k odd: w^(+-1)), so a lane forms its twist scalar with one Montgomery product of the
// table entry and one of two constants (c, c w^(+-1) in Montgomery form: standard x Montgomery -> standard).
//
// Lane numbering of hb_mul_kernel, judged against the wavefront model of CDNA (64 lanes, one program counter; a branch
// taken by some lanes costs every lane both sides): pos sits in the HIGH bits of the lane index, the group in the low
// bits, as in pp_mul_kernel.  While a stage has 64 groups or more (s <= L - 7) a wavefront shares ONE twiddle: the
// digit string of pp_scalar_mul is the same in every lane, so "is this digit zero" and "is it negative" do not diverge,
// and the pos = 0 lanes, which need no product, are whole wavefronts that leave at once.  The price is the operand
// stride of 2^(s+1) points (128 B each): no two lanes of a load share a cache line from stage 0 on -- but a product is
// ~3500 field multiplications on 256 bytes of traffic, the loads are nowhere near the bound.  The last six stages mix
// up to 64 twiddles per wavefront whatever the numbering; there, and in the twist (every lane its own scalar), only the
// zero digits (one in eight) diverge.  The other numbering (pos low) would coalesce nothing either (128-byte points)
// and diverge in every stage.
//
// The product is pp_scalar_mul (scalar_mul.cuh; signed 3-bit windows, the lane's table in global memory, one slot per
// lane of a persistent grid: G16_BELLMAN_LANES lanes, rounded up to whole wavefronts, or four workgroups of 256 per
// compute unit).  Exact canonical arithmetic (fp.cuh / ec.cuh): the XYZZ formulas are complete (infinity, equal and
// opposite operands, which tau = 1 or a root of unity put into every butterfly), the affine bytes are unique.
// As built for gfx950: 198 / 202 VGPRs in the two product kernels, 180 in the butterfly, 0 B scratch in all four.
// Measured on one MI355X at L = 20, one run (tools/zkey_bellman_bench.py): 463 ms forward, 461 ms inverse
// for 10 485 761 products, 44 ns per product against ptau_scale's 47.8 ns per G1 product in the same process.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ec.cuh"
#include "internal.h"
#include "scalar_mul.cuh"
#include "setup_affine.cuh"

namespace g16 {
namespace {

constexpr int kWin = 3, kTbl = 1 << (kWin - 1);
constexpr int kMulBlock = 256;
constexpr int kMaxLog = 24;

__device__ __forceinline__ uint32_t bitrev(uint32_t j, int L) { return L ? __brev(j) >> (32 - L) : 0u; }

__global__ __launch_bounds__(256) void hb_load_kernel(const G1Affine* __restrict__ src, uint32_t n, int L,
                                                      G1XYZZ* __restrict__ work) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  G1XYZZ p;
  xyzz_from_affine(p, src[bitrev(t, L)]);
  work[t] = p;
}

// Lane t of n (grid-stride): work[t] times c tw[k >> 1], c = c_even / c_odd (Montgomery form) by the parity of k;
// k = t, or bitrev(t) when the array holds the points in bit-reversed order.  sc = one scalar slot per lane of the grid
// (pp_scalar_mul indexes its scalar: a private copy would go to scratch).
__global__ __launch_bounds__(kMulBlock) void hb_twist_kernel(G1XYZZ* __restrict__ work, const Fr* __restrict__ tw, uint32_t n, int L,
                                                             int reversed, Fr c_even, Fr c_odd, Fr* __restrict__ sc,
                                                             G1XYZZ* __restrict__ tbl) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t t = gid; t < n; t += stride) {
    const G1XYZZ base = work[t];
    if (xyzz_is_inf(base)) continue;
    const uint32_t k = reversed ? bitrev(t, L) : t;
    sc[gid] = fp_mul(tw[k >> 1], (k & 1) ? c_odd : c_even);
    G1XYZZ acc;
    pp_scalar_mul<FqOps, kWin>(acc, base, sc[gid].v, tbl + gid, stride);
    work[t] = acc;
  }
}

// Stage s >= 1, lane t of half = N/2 (grid-stride), sh = L - 1 - s: pos = t >> sh on top, the group g below; the
// operand is point (g << (s+1)) + 2^s + pos <= N - 1 and the scalar tw[pos << sh], pos << sh < N/2.
__global__ __launch_bounds__(kMulBlock) void hb_mul_kernel(G1XYZZ* __restrict__ work, const Fr* __restrict__ tw, uint32_t half, int s,
                                                           int sh, G1XYZZ* __restrict__ tbl) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t t = gid; t < half; t += stride) {
    const uint32_t pos = t >> sh, g = t & ((1u << sh) - 1);
    if (pos == 0) continue;
    const uint32_t e = (g << (s + 1)) + (1u << s) + pos;
    const G1XYZZ base = work[e];
    G1XYZZ acc;
    pp_scalar_mul<FqOps, kWin>(acc, base, tw[pos << sh].v, tbl + gid, stride);
    work[e] = acc;
  }
}

// stage s, one lane per butterfly b = g << s | pos
__global__ __launch_bounds__(256) void hb_bfly_kernel(G1XYZZ* __restrict__ work, uint32_t half, int s) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= half) return;
  const uint32_t pos = t & ((1u << s) - 1), g = t >> s;
  const uint32_t i0 = (g << (s + 1)) + pos, i1 = i0 + (1u << s);
  const G1XYZZ x = work[i0];
  G1XYZZ y = work[i1];
  G1XYZZ sum = x, diff = x;
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

}  // namespace

int zkey_h_basis(int device, const uint8_t* in, int L, bool inverse, uint8_t* out, ZkeyBasisStats* stats) {
  if (L < 0 || L > kMaxLog) { set_error("zkey h basis: log_n out of range (need 0..24)"); return G16_E_ARG; }
  if (const int rc = require_hip_device("zkey h basis", device)) return rc;
  G16_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  G16_HIP(hipGetDeviceProperties(&prop, device));
  const uint32_t N = 1u << L, half = N >> 1;

  // scalars: tw[i] = W^(+-i) in standard form (one entry, 1, at L = 0); the twist's two constants in Montgomery form
  const uint32_t ntw = std::max(half, 1u);
  std::vector<Fr> tw(ntw);
  Fr c_even, c_odd;
  {
    Fr w = root_of_unity(L + 1);
    if (inverse) w = fp_inv(w);
    const Fr W = fp_sqr(w);
    Fr x = fp_one<FrParams>();
    for (uint32_t i = 0; i < ntw; i++) { tw[i] = fp_from_mont(x); x = fp_mul(x, W); }
    Fr two = fp_one<FrParams>();
    two = fp_add(two, two);
    if (inverse) {   // -1 / (2N)
      Fr d = two;
      for (int k = 0; k < L; k++) d = fp_add(d, d);
      c_even = fp_neg(fp_inv(d));
    } else {
      c_even = fp_neg(two);
    }
    c_odd = fp_mul(c_even, w);
  }
  // persistent grid of the products: four workgroups of 256 per compute unit at most
  uint32_t block = kMulBlock, lanes = (uint32_t)std::max(prop.multiProcessorCount, 1) * 4 * kMulBlock;
  if (const uint32_t forced = env_u32("G16_BELLMAN_LANES")) {
    lanes = std::min((forced + 63) / 64 * 64, lanes);
    if (lanes % block) block = 64;
  }
  lanes = std::min(lanes, (N + block - 1) / block * block);
  auto grid = [&](uint32_t n) { return std::min(lanes / block, (n + block - 1) / block); };

  DeviceJob job("zkey h basis");
  DeviceBuf<G1Affine> d_aff;   // the input, then the output
  DeviceBuf<G1XYZZ> d_work, d_tbl;
  DeviceBuf<Fr> d_tw, d_sc;
  DeviceTimer timer;
  DeviceStream st;
  uint64_t muls = 0, adds = 0;
  if (job.fail(st.create()) || job.fail(timer.create()) || job.fail(d_aff.alloc(N)) || job.fail(d_work.alloc(N)) ||
      job.fail(d_tbl.alloc((size_t)lanes * kTbl)) || job.fail(d_tw.alloc(ntw)) || job.fail(d_sc.alloc(lanes)) ||
      job.fail(hipMemcpyAsync(d_aff.p, in, (size_t)N * sizeof(G1Affine), hipMemcpyHostToDevice, st)) ||
      job.fail(hipMemcpyAsync(d_tw.p, tw.data(), (size_t)ntw * sizeof(Fr), hipMemcpyHostToDevice, st)) || job.fail(timer.start(st)))
    return job.rc;
  hb_load_kernel<<<(N + 255) / 256, 256, 0, st>>>(d_aff.p, N, L, d_work.p);
  if (inverse) {
    hb_twist_kernel<<<grid(N), block, 0, st>>>(d_work.p, d_tw.p, N, L, 1, c_even, c_odd, d_sc.p, d_tbl.p);
    muls += N;
  }
  for (int s = 0; s < L; s++) {
    if (s >= 1) {
      hb_mul_kernel<<<grid(half), block, 0, st>>>(d_work.p, d_tw.p, half, s, L - 1 - s, d_tbl.p);
      muls += half - (half >> s);
    }
    hb_bfly_kernel<<<(half + 255) / 256, 256, 0, st>>>(d_work.p, half, s);
    adds += N;
  }
  if (!inverse) {
    hb_twist_kernel<<<grid(N), block, 0, st>>>(d_work.p, d_tw.p, N, L, 0, c_even, c_odd, d_sc.p, d_tbl.p);
    muls += N;
  }
  const uint32_t nb = (N + kBatch - 1) / kBatch;
  setup_to_affine_kernel<FqOps><<<(nb + 255) / 256, 256, 0, st>>>(d_work.p, d_aff.p, N);
  if (job.fail(hipGetLastError()) || job.fail(timer.stop(st)) ||
      job.fail(hipMemcpyAsync(out, d_aff.p, (size_t)N * sizeof(G1Affine), hipMemcpyDeviceToHost, st)) ||
      job.fail(hipStreamSynchronize(st)))
    return job.rc;
  if (stats) {
    stats->kern_ms = timer.ms();
    stats->muls = muls;
    stats->adds = adds;
  }
  return G16_OK;
}

}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_h_basis(int device, const uint8_t* points, uint32_t log_n, int inverse, uint8_t* out) {
  if (!points || !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (log_n > (uint32_t)kMaxLog) { set_error("zkey h basis: log_n out of range (need 0..24)"); return G16_E_ARG; }
  return no_bad_alloc("zkey h basis", [&]() { return zkey_h_basis(device, points, (int)log_n, inverse != 0, out, nullptr); });
}
