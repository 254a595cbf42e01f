// out[i] = [k] P[i] for ONE scalar k and n affine G1 points: the section scaling of `snarkjs zkey contribute`
// (zkey_new / zkey_contribute.js applyKeyToSection(.., invDelta, 1) over sections 8 and 9; zkey_mpc.cpp).  File bytes
// in, file bytes out (affine little-endian Montgomery, infinity = zero bytes in and out).
//
// Unlike pp_scalar_mul (ptau_prepare.hip), whose lanes each recode a scalar of their own, the digit string here is the
// same for the whole grid: the HOST recodes k once (width-kWin non-adjacent form, odd digits |d| < 2^(kWin-1), at most
// 255 positions) and uploads the digits once (a small device array: as a by-value kernel argument the compiler copies
// the array to per-lane scratch to index it).  The kernel reads them through uniform loads, so the
// loop control -- how many doublings, whether a position adds, which table entry, which sign -- lives in scalar
// registers: no divergence, no per-lane recoding, no carry masks.
//
// Window: kWin = 5, a table of the odd multiples {1, 3, .., 15}P (the input itself serves as 1 P).  Costs per product,
// in point operations (a wNAF of width w has one non-zero digit per w + 1 positions on average), and measured on one
// MI355X over the 1 898 062 points of an nzcp_live-shaped key (tools/zkey_contribute_bench.py, three repeats, twice,
// alternating):
//   w = 3:  table 1 dbl + 1 add,  254 dbl + ~63 add   (1 stored entry)            46.3 - 47.0 ns per product
//   w = 4:  table 1 dbl + 3 add,  254 dbl + ~51 add   (3 entries, 384 B per lane) 45.1 - 45.8 ns
//   w = 5:  table 1 dbl + 7 add,  254 dbl + ~42 add   (7 entries, 896 B per lane) 44.1 - 45.1 ns
// The measured steps follow the counts (5 of ~310 operations between 4 and 5); w = 6 would add 16 table additions to
// save 6.  pp_scalar_mul's fixed signed 3-bit windows pay 254 dbl + up to 85 add + 3 and measured 60.9 ns per product
// in the same process.  G16_CONTRIBUTE_WINDOW = 3 / 4 / 5 selects the width (sweeps and tests; the bytes are the same).
// A digit of +-1 adds the affine input itself (xyzz_madd: 8M + 2S instead of 12M + 2S), which costs no table slot.
// A lane's table lives in global memory, one slot per lane of a fixed persistent grid (grid-stride loop), as in
// pp_mul_kernel and for its reason: in LDS 7 x 128 B per lane would cap a workgroup at one wavefront.  The lane count is
// G16_CONTRIBUTE_LANES (rounded up to whole wavefronts) or four workgroups of 256 per compute unit.
//
// Arithmetic: the canonical fp.cuh / ec.cuh XYZZ formulas.  They are complete (infinity, equal and opposite operands
// are handled), so no argument about k or the order of the inputs is needed, and the affine result is unique: the
// bytes equal the host's and the oracle's.
//
// A section of any size runs in chunks of kChunk points through two buffer sets: the copies of chunk c + 1 (up) and
// c - 1 (down) go over a second stream while chunk c computes, and the device never holds more than two chunks.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "binfile.h"
#include "ec.cuh"
#include "internal.h"
#include "setup_affine.cuh"

namespace g16 {
namespace {

constexpr int kWin = 5;          // window width; G16_CONTRIBUTE_WINDOW = 3 / 4 / 5 overrides it (sweeps)
constexpr int kWinMax = 5;
constexpr int table_entries(int w) { return 1 << (w - 2); }   // entries e = 0 .. hold (2e + 1) P
constexpr int kMaxDigits = 256;
constexpr int kScaleBlock = 256;
constexpr uint32_t kChunk = 1u << 18;             // points per chunk: 16 MB up, 32 MB XYZZ, 16 MB down

struct ScaleDigits {
  int32_t top;                 // position of the highest non-zero digit (always positive)
  int8_t d[kMaxDigits];        // odd or zero, |d| < 2^(w - 1)
};

// k (standard form, 1 <= k < 2^255) -> width-w NAF
void recode(const Fr& k, int w, ScaleDigits& out) {
  uint32_t v[9];
  for (int i = 0; i < 8; i++) v[i] = k.v[i];
  v[8] = 0;
  memset(out.d, 0, sizeof(out.d));
  out.top = 0;
  auto is_zero = [&]() { for (int i = 0; i < 9; i++) if (v[i]) return false; return true; };
  for (int pos = 0; pos < kMaxDigits && !is_zero(); pos++) {
    if (v[0] & 1) {
      int d = (int)(v[0] & ((1u << w) - 1));
      if (d >= (1 << (w - 1))) d -= 1 << w;
      out.d[pos] = (int8_t)d;
      out.top = pos;
      // v -= d
      int64_t c = -(int64_t)d;
      for (int i = 0; i < 9 && c; i++) {
        const int64_t t = (int64_t)v[i] + c;
        v[i] = (uint32_t)t;
        c = t >> 32;   // arithmetic: -1 borrows on
      }
    }
    for (int i = 0; i < 8; i++) v[i] = (v[i] >> 1) | (v[i + 1] << 31);
    v[8] >>= 1;
  }
}

template <int W>
__global__ __launch_bounds__(kScaleBlock) void zkey_scale_kernel(const G1Affine* __restrict__ in, G1XYZZ* __restrict__ work,
                                                                uint32_t n, const int8_t* __restrict__ digits, int top,
                                                                G1XYZZ* __restrict__ tbl) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  G1XYZZ* const slot = tbl + gid;   // entry e at slot[e * stride]
  for (uint32_t i = gid; i < n; i += stride) {
    const G1Affine p = in[i];
    G1XYZZ acc;
    if (aff_is_inf(p)) {
      xyzz_set_inf(acc);
      work[i] = acc;
      continue;
    }
    {
      G1XYZZ two, t;
      xyzz_dbl_affine(two, p);
      xyzz_from_affine(t, p);
      for (int e = 1; e < table_entries(W); e++) {
        xyzz_add(t, two);
        slot[(size_t)e * stride] = t;
      }
    }
    // (the first doubling works on infinity, which xyzz_dbl keeps: one of every operation in the loop body)
    xyzz_set_inf(acc);
    for (int j = top; j >= 0; j--) {
      xyzz_dbl(acc);
      const int d = digits[j];   // uniform: odd or zero
      if (d == 0) continue;
      const int m = d < 0 ? -d : d;
      if (m == 1) {
        G1Affine q = in[i];
        if (d < 0) aff_neg(q);
        xyzz_madd(acc, q);
      } else {
        G1XYZZ q = slot[(size_t)(m >> 1) * stride];
        if (d < 0) xyzz_neg(q);
        xyzz_add(acc, q);
      }
    }
    work[i] = acc;
  }
}

uint32_t env_u32(const char* name) {
  const char* e = getenv(name);
  if (!e) return 0;
  const long v = atol(e);
  return v > 0 ? (uint32_t)std::min<long>(v, 1l << 30) : 0;
}

}  // namespace

int zkey_scale_g1(int device, const uint8_t* in, uint64_t n, const Fr& k_std, uint8_t* out, ZkeyScaleStats* st) {
  if (fp_is_zero(k_std) || !fr_below_modulus(k_std.v)) { set_error("zkey scale: the multiplier is not in [1, r)"); return G16_E_ARG; }
  if (const int rc = require_hip_device("zkey scale", device)) return rc;
  if (st) *st = ZkeyScaleStats{};
  if (n == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  G16_HIP(hipGetDeviceProperties(&prop, device));
  int win = (int)env_u32("G16_CONTRIBUTE_WINDOW");
  if (win < 3 || win > kWinMax) win = kWin;
  const int ntbl = table_entries(win);
  ScaleDigits dg;
  recode(k_std, win, dg);

  // chunk and persistent grid (both overridable, so that a small test runs several chunks and grid-stride passes)
  uint32_t chunk = env_u32("G16_CONTRIBUTE_CHUNK");
  if (!chunk) chunk = kChunk;
  chunk = (uint32_t)std::min<uint64_t>(chunk, n);
  const uint32_t lanes_cap = (uint32_t)std::max(prop.multiProcessorCount, 1) * 4 * kScaleBlock;
  uint32_t lanes = env_u32("G16_CONTRIBUTE_LANES");
  uint32_t block = kScaleBlock;
  if (lanes) {
    lanes = std::min((lanes + 63) / 64 * 64, lanes_cap);
    if (lanes % kScaleBlock) block = 64;
  } else {
    lanes = lanes_cap;
  }
  lanes = std::min(lanes, (chunk + block - 1) / block * block);
  const uint32_t blocks = lanes / block;
  const uint64_t nchunks = (n + chunk - 1) / chunk;

  G1Affine* d_in[2] = {nullptr, nullptr};
  G1Affine* d_aff[2] = {nullptr, nullptr};
  G1XYZZ* d_work = nullptr;
  G1XYZZ* d_tbl = nullptr;
  int8_t* d_digits = nullptr;
  hipStream_t cst = nullptr, xst = nullptr;   // compute, copies
  hipEvent_t ev_up[2] = {}, ev_k[2] = {}, ev_down[2] = {};
  std::vector<hipEvent_t> tk(2 * nchunks, nullptr), tx(4 * nchunks, nullptr);   // timing: kernel / copy begin-end pairs
  int rc = G16_OK;
  auto fail = [&](hipError_t e) {
    if (e == hipSuccess) return false;
    set_error(std::string("zkey scale (device): ") + hipGetErrorString(e));
    rc = G16_E_HIP;
    return true;
  };
  auto upload = [&](uint64_t c) {
    const int b = (int)(c & 1);
    const uint64_t lo = c * chunk, cnt = std::min<uint64_t>(chunk, n - lo);
    // the buffer's last reader (the kernel of chunk c - 2) has finished
    if (c >= 2 && fail(hipStreamWaitEvent(xst, ev_k[b], 0))) return false;
    if (fail(hipEventRecord(tx[4 * c], xst))) return false;
    if (fail(hipMemcpyAsync(d_in[b], in + lo * 64, cnt * 64, hipMemcpyHostToDevice, xst))) return false;
    if (fail(hipEventRecord(tx[4 * c + 1], xst))) return false;
    return !fail(hipEventRecord(ev_up[b], xst));
  };
  do {
    if (fail(hipStreamCreateWithFlags(&cst, hipStreamNonBlocking)) || fail(hipStreamCreateWithFlags(&xst, hipStreamNonBlocking))) break;
    bool bad = false;
    for (int b = 0; b < 2 && !bad; b++)
      bad = fail(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming)) ||
            fail(hipEventCreateWithFlags(&ev_k[b], hipEventDisableTiming)) ||
            fail(hipEventCreateWithFlags(&ev_down[b], hipEventDisableTiming));
    for (auto& e : tk) if (!bad) bad = fail(hipEventCreate(&e));
    for (auto& e : tx) if (!bad) bad = fail(hipEventCreate(&e));
    if (bad) break;
    const int nbuf = nchunks > 1 ? 2 : 1;
    for (int b = 0; b < nbuf && !bad; b++)
      bad = fail(hipMalloc(&d_in[b], (size_t)chunk * sizeof(G1Affine))) || fail(hipMalloc(&d_aff[b], (size_t)chunk * sizeof(G1Affine)));
    if (bad) break;
    if (fail(hipMalloc(&d_work, (size_t)chunk * sizeof(G1XYZZ)))) break;
    if (fail(hipMalloc(&d_tbl, (size_t)lanes * ntbl * sizeof(G1XYZZ)))) break;
    if (fail(hipMalloc(&d_digits, sizeof(dg.d)))) break;
    if (fail(hipMemcpyAsync(d_digits, dg.d, sizeof(dg.d), hipMemcpyHostToDevice, xst))) break;   // (before ev_up of chunk 0)
    if (!upload(0)) break;
    for (uint64_t c = 0; c < nchunks; c++) {
      const int b = (int)(c & 1);
      const uint64_t lo = c * chunk;
      const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, n - lo);
      if (c + 1 < nchunks && !upload(c + 1)) break;
      if (fail(hipStreamWaitEvent(cst, ev_up[b], 0))) break;
      if (c >= 2 && fail(hipStreamWaitEvent(cst, ev_down[b], 0))) break;   // d_aff[b] has been copied out
      if (fail(hipEventRecord(tk[2 * c], cst))) break;
      const uint32_t grid = std::min(blocks, (cnt + block - 1) / block);
      if (win == 3) zkey_scale_kernel<3><<<grid, block, 0, cst>>>(d_in[b], d_work, cnt, d_digits, dg.top, d_tbl);
      else if (win == 5) zkey_scale_kernel<5><<<grid, block, 0, cst>>>(d_in[b], d_work, cnt, d_digits, dg.top, d_tbl);
      else zkey_scale_kernel<4><<<grid, block, 0, cst>>>(d_in[b], d_work, cnt, d_digits, dg.top, d_tbl);
      setup_to_affine_kernel<FqOps><<<((cnt + kBatch - 1) / kBatch + 255) / 256, 256, 0, cst>>>(d_work, d_aff[b], cnt);
      if (fail(hipGetLastError())) break;
      if (fail(hipEventRecord(tk[2 * c + 1], cst)) || fail(hipEventRecord(ev_k[b], cst))) break;
      if (fail(hipStreamWaitEvent(xst, ev_k[b], 0))) break;
      if (fail(hipEventRecord(tx[4 * c + 2], xst))) break;
      if (fail(hipMemcpyAsync(out + lo * 64, d_aff[b], (size_t)cnt * 64, hipMemcpyDeviceToHost, xst))) break;
      if (fail(hipEventRecord(tx[4 * c + 3], xst)) || fail(hipEventRecord(ev_down[b], xst))) break;
    }
    if (rc) break;
    if (fail(hipStreamSynchronize(xst)) || fail(hipStreamSynchronize(cst))) break;
    if (st) {
      for (uint64_t c = 0; c < nchunks; c++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tk[2 * c], tk[2 * c + 1]) == hipSuccess) st->kern_ms += ms;
        for (int h = 0; h < 2; h++)
          if (hipEventElapsedTime(&ms, tx[4 * c + 2 * h], tx[4 * c + 2 * h + 1]) == hipSuccess) st->xfer_ms += ms;
      }
      st->points = n;
    }
  } while (false);
  if (xst) (void)hipStreamSynchronize(xst);
  if (cst) (void)hipStreamSynchronize(cst);
  for (int b = 0; b < 2; b++) {
    hipEvent_t evs[3] = {ev_up[b], ev_k[b], ev_down[b]};
    for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
    if (d_in[b]) (void)hipFree(d_in[b]);
    if (d_aff[b]) (void)hipFree(d_aff[b]);
  }
  for (hipEvent_t e : tk) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : tx) if (e) (void)hipEventDestroy(e);
  if (d_work) (void)hipFree(d_work);
  if (d_tbl) (void)hipFree(d_tbl);
  if (d_digits) (void)hipFree(d_digits);
  if (xst) (void)hipStreamDestroy(xst);
  if (cst) (void)hipStreamDestroy(cst);
  return rc;
}

}  // namespace g16
