// out[i] = [c k^(first + i)] P[i] for n affine points of G1 or G2: the section scaling of `snarkjs powersoftau
// contribute` (snarkjs's batchApplyKey(buff, first, inc) with first = c k^first and inc = k; ptau_mpc.cpp).  File bytes
// in, file bytes out (affine little-endian Montgomery, infinity = zero bytes in and out), and -- optionally -- the
// uncompressed big-endian standard-form image of every output point, which the ceremony's challenge hash is taken over:
// the device holds the point anyway, and a lane per point is cheaper than ~14 M host conversions at power 20.
//
// Scalars: every lane forms its own on the device.  c and k arrive as two Montgomery residues (kernel arguments); lane
// i runs the square-and-multiply ladder over the bits of e = first + i (at most 25 at power 24; the loop bound is the
// bit length of the chunk's last exponent, so it is uniform), converts to standard form and parks the eight words in
// its slot of a small global array, where the window reads index them (a private copy indexed by the loop variable
// would go to scratch).  At most 25 + 25 Fr products next to the ~3500 Fq products of the multiplication itself.
//
// Product: pp_scalar_mul (scalar_mul.cuh), the fixed signed windows of ptau_prepare.hip -- the scalars differ per lane,
// so zkey_scale.hip's uniform digit string does not apply.  Point operations per product for width W (254 or 255
// doublings; a signed window is zero with probability 2^-W):
//   W = 3:  table 1 dbl + 2 add,   85 windows  -> ~74 add    (4 entries)
//   W = 4:  table 1 dbl + 6 add,   64 windows  -> ~60 add    (8 entries)
//   W = 5:  table 1 dbl + 14 add,  51 windows  -> ~49 add    (16 entries)
// G16_PTAU_WINDOW = 3 / 4 / 5 selects the width (sweeps and tests; the bytes are the same); the default is kWin = 5.
// Measured on one MI355X (tools/ptau_contribute_bench.py: one contribution to the generator file of power 20 --
// 5 242 879 products on G1, 1 048 577 on G2 -- three repeats per width, every width twice, alternating, one process;
// kernel events, the conversion to affine and the big-endian images included), ns per product:
//   W = 3:  G1 50.5 - 53.2   G2 220.0 - 224.1
//   W = 4:  G1 46.7 - 47.1   G2 203.2 - 207.7
//   W = 5:  G1 45.4 - 46.1   G2 197.0 - 200.2     (16 entries: 2 KB per G1 lane, 4 KB per G2 lane, 1 GB for the G2 grid)
// The yardstick in the same process, pp_mul_kernel inside one `prepare phase2` of the same power 20 (W = 3, a wavefront
// shares one scalar there, so zero digits do not diverge, and the pos = 0 lanes leave at once; butterflies included):
// G1 44.0 - 44.1 ns, G2 204.2 - 204.6 ns per product.  So per product this kernel is 3 - 4 % SLOWER than that path on
// G1 and 2 - 4 % faster on G2: the per-lane scalars cost the divergence on zero digits, the Fr ladder and the scalar's
// round trip through memory, which W = 5's fewer additions do not quite buy back on G1.  Not tuned further.
// As built: 173 VGPRs (G1) / 511 + spills to AGPRs (G2), 0 B scratch, for W = 3, 4, 5 alike.
// A lane's table lives in global memory, one slot per lane of a fixed persistent grid (grid-stride loop), as in
// pp_mul_kernel and for its reason: in LDS 4 x 256 B per G2 lane would cap a workgroup at one wavefront.  The lane count
// is G16_PTAU_LANES (rounded up to whole wavefronts) or four workgroups of 256 per compute unit.
//
// Arithmetic: the canonical fp.cuh / ec.cuh XYZZ formulas.  They are complete (infinity, equal and opposite operands
// are handled: tau = 1, tau = r - 1 or a root of unity need no argument), and the affine result is unique: the bytes
// equal the host's and the oracle's.
//
// A section of any size runs in chunks (G16_PTAU_CHUNK) through the pipeline of chunk_pipeline.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "binfile.h"
#include "chunk_pipeline.h"
#include "ec.cuh"
#include "internal.h"
#include "ptau_be.cuh"
#include "scalar_mul.cuh"
#include "setup_affine.cuh"

namespace g16 {
namespace {

constexpr int kWin = 5;   // G16_PTAU_WINDOW = 3 / 4 / 5 overrides it
constexpr int kScaleBlock = 256;

template <class FC, int W>
__global__ __launch_bounds__(kScaleBlock) void ptau_scale_kernel(const Affine<FC>* __restrict__ in, XYZZ<FC>* __restrict__ work,
                                                                uint32_t n, uint32_t first, Fr c_mont, Fr k_mont, int nbits,
                                                                Fr* __restrict__ sc, XYZZ<FC>* __restrict__ tbl) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (uint32_t i = gid; i < n; i += stride) {
    XYZZ<FC> base, acc;
    xyzz_from_affine(base, in[i]);
    if (xyzz_is_inf(base)) {
      work[i] = base;
      continue;
    }
    {
      const uint32_t e = first + i;
      Fr x = c_mont, pw = k_mont;
      for (int j = 0; j < nbits; j++) {
        if ((e >> j) & 1) x = fp_mul(x, pw);
        pw = fp_sqr(pw);
      }
      sc[gid] = fp_from_mont(x);
    }
    pp_scalar_mul<FC, W>(acc, base, sc[gid].v, tbl + gid, stride);
    work[i] = acc;
  }
}

// affine file image -> uncompressed big-endian standard form (ptau_be.cuh); the inverse of ptau_from_be_kernel
// (ptau_points.hip)
template <class FC>
__global__ __launch_bounds__(256) void ptau_be_kernel(const Affine<FC>* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  constexpr int NC = sizeof(Affine<FC>) / 32;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<FC> p = in[i];
  const Fq* co = reinterpret_cast<const Fq*>(&p);
  uint32_t* o = out + (size_t)i * NC * 8;
  if (aff_is_inf(p)) {
    store_inf(o, NC * 8);
    return;
  }
#pragma unroll
  for (int c = 0; c < NC; c++) store_be(o + c * 8, fp_from_mont(co[be_slot<NC>(c)]));
}

template <class FC, int W>
void launch_scale(uint32_t grid, uint32_t block, hipStream_t st, const Affine<FC>* in, XYZZ<FC>* work, uint32_t n, uint32_t first,
                  const Fr& c, const Fr& k, int nbits, Fr* sc, XYZZ<FC>* tbl) {
  ptau_scale_kernel<FC, W><<<grid, block, 0, st>>>(in, work, n, first, c, k, nbits, sc, tbl);
}

template <class FC>
int scale_device(int device, const uint8_t* in, uint64_t n, const Fr& c_std, const Fr& k_std, uint64_t first, uint8_t* out,
                 uint8_t* out_be, ChunkStats* st) {
  constexpr size_t PSZ = sizeof(Affine<FC>);
  if (fp_is_zero(c_std) || !fr_below_modulus(c_std.v) || fp_is_zero(k_std) || !fr_below_modulus(k_std.v)) {
    set_error("ptau scale: a multiplier is not in [1, r)");
    return G16_E_ARG;
  }
  if (first + n > ((uint64_t)1 << 31)) { set_error("ptau scale: exponent range above 2^31"); return G16_E_ARG; }
  if (const int rc = require_hip_device("ptau scale", device)) return rc;
  if (st) *st = ChunkStats{};
  if (n == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  G16_HIP(hipGetDeviceProperties(&prop, device));
  int win = (int)env_u32("G16_PTAU_WINDOW");
  if (win < 3 || win > 5) win = kWin;
  const Fr c_mont = fp_to_mont(c_std), k_mont = fp_to_mont(k_std);
  const ChunkPlan plan = chunk_plan("G16_PTAU_CHUNK", "G16_PTAU_LANES", n, (uint32_t)std::max(prop.multiProcessorCount, 1) * 4 * kScaleBlock);

  DeviceBuf<XYZZ<FC>> work, tbl;
  DeviceBuf<Fr> sc;
  ChunkPipeline pipe("ptau scale");
  if (!pipe.open(n, plan.chunk, PSZ, PSZ, out_be ? PSZ : 0) || pipe.fail(work.alloc(plan.chunk)) ||
      pipe.fail(tbl.alloc((size_t)plan.lanes << (win - 1))) || pipe.fail(sc.alloc(plan.lanes)))
    return pipe.rc;
  return pipe.run(in, out, out_be, st, [&](hipStream_t s, const uint8_t* d_in, uint8_t* d_out, uint8_t* d_be, uint32_t cnt, uint64_t lo) {
    const Affine<FC>* pts = (const Affine<FC>*)d_in;
    Affine<FC>* aff = (Affine<FC>*)d_out;
    const uint32_t grid = plan.grid(cnt), block = plan.block;
    const uint32_t cfirst = (uint32_t)(first + lo);   // a chunk carries its `first`
    int nbits = 0;
    while (nbits < 32 && ((uint64_t)cfirst + cnt - 1) >> nbits) nbits++;
    if (win == 3) launch_scale<FC, 3>(grid, block, s, pts, work.p, cnt, cfirst, c_mont, k_mont, nbits, sc.p, tbl.p);
    else if (win == 4) launch_scale<FC, 4>(grid, block, s, pts, work.p, cnt, cfirst, c_mont, k_mont, nbits, sc.p, tbl.p);
    else launch_scale<FC, 5>(grid, block, s, pts, work.p, cnt, cfirst, c_mont, k_mont, nbits, sc.p, tbl.p);
    setup_to_affine_kernel<FC><<<((cnt + kBatch - 1) / kBatch + 255) / 256, 256, 0, s>>>(work.p, aff, cnt);
    if (d_be) ptau_be_kernel<FC><<<(cnt + 255) / 256, 256, 0, s>>>(aff, (uint32_t*)d_be, cnt);
  });
}

}  // namespace

int ptau_scale_g1(int device, const uint8_t* in, uint64_t n, const Fr& c_std, const Fr& k_std, uint64_t first, uint8_t* out,
                  uint8_t* out_be, ChunkStats* st) {
  return scale_device<FqOps>(device, in, n, c_std, k_std, first, out, out_be, st);
}
int ptau_scale_g2(int device, const uint8_t* in, uint64_t n, const Fr& c_std, const Fr& k_std, uint64_t first, uint8_t* out,
                  uint8_t* out_be, ChunkStats* st) {
  return scale_device<Fq2Ops>(device, in, n, c_std, k_std, first, out, out_be, st);
}

}  // namespace g16
