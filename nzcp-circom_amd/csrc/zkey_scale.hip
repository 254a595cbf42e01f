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
// A section of any size runs in chunks (G16_CONTRIBUTE_CHUNK) through the pipeline of chunk_pipeline.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "binfile.h"
#include "chunk_pipeline.h"
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

}  // namespace

int zkey_scale_g1(int device, const uint8_t* in, uint64_t n, const Fr& k_std, uint8_t* out, ChunkStats* st) {
  if (fp_is_zero(k_std) || !fr_below_modulus(k_std.v)) { set_error("zkey scale: the multiplier is not in [1, r)"); return G16_E_ARG; }
  if (const int rc = require_hip_device("zkey scale", device)) return rc;
  if (st) *st = ChunkStats{};
  if (n == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  G16_HIP(hipGetDeviceProperties(&prop, device));
  int win = (int)env_u32("G16_CONTRIBUTE_WINDOW");
  if (win < 3 || win > kWinMax) win = kWin;
  ScaleDigits dg;
  recode(k_std, win, dg);
  const ChunkPlan plan = chunk_plan("G16_CONTRIBUTE_CHUNK", "G16_CONTRIBUTE_LANES", n,
                                    (uint32_t)std::max(prop.multiProcessorCount, 1) * 4 * kScaleBlock);

  DeviceBuf<G1XYZZ> work, tbl;
  DeviceBuf<int8_t> digits;
  ChunkPipeline pipe("zkey scale");
  if (!pipe.open(n, plan.chunk, sizeof(G1Affine), sizeof(G1Affine), 0) || pipe.fail(work.alloc(plan.chunk)) ||
      pipe.fail(tbl.alloc((size_t)plan.lanes * table_entries(win))) || pipe.fail(digits.alloc(sizeof(dg.d))) ||
      pipe.fail(hipMemcpyAsync(digits.p, dg.d, sizeof(dg.d), hipMemcpyHostToDevice, pipe.stream())))
    return pipe.rc;
  return pipe.run(in, out, nullptr, st, [&](hipStream_t s, const uint8_t* d_in, uint8_t* d_out, uint8_t*, uint32_t cnt, uint64_t) {
    const G1Affine* pts = (const G1Affine*)d_in;
    const uint32_t grid = plan.grid(cnt), block = plan.block;
    if (win == 3) zkey_scale_kernel<3><<<grid, block, 0, s>>>(pts, work.p, cnt, digits.p, dg.top, tbl.p);
    else if (win == 5) zkey_scale_kernel<5><<<grid, block, 0, s>>>(pts, work.p, cnt, digits.p, dg.top, tbl.p);
    else zkey_scale_kernel<4><<<grid, block, 0, s>>>(pts, work.p, cnt, digits.p, dg.top, tbl.p);
    setup_to_affine_kernel<FqOps><<<((cnt + kBatch - 1) / kBatch + 255) / 256, 256, 0, s>>>(work.p, (G1Affine*)d_out, cnt);
  });
}

}  // namespace g16
