// Witness check on the device (g16_wtns_check): does w satisfy (A_i.w)(B_i.w) = C_i.w for every row i of an R1CS?
//
// The twin of later snarkjs releases' `wtns check` (the pinned 0.4.12 has none).  The three matrices stay resident in
// the layout of the QAP evaluation (qap_rows.cuh: +-1 records add the witness word's Montgomery image, the general ones
// multiply); the kernel forms the three row sums, tests a*b - c on the CANONICAL value -- lazy values compare unequal
// when they are equal mod r -- and writes nothing but the verdict: per witness the lowest failing row (atomicMin) and
// the number of failing rows (atomicAdd).  A satisfied witness causes no store at all.
//
// The lazy-sum bound, restated for three matrices: every matrix is summed on its own by qap_row_sum, so each of the
// three sums obeys its bound (an added term below 1.1r, a subtracted one at most 2r, a weak reduction to 1.0001r
// whenever seven units have gone in: below 1 + 6 * 1.1 + 2 = 9.6r < 16r).  In the grouped rows the partial sums are
// weak-reduced before the shuffle tree and after its steps 8 and 1, so at most 8 partials below ~2r meet between
// reductions.  The product takes a, b < 16r and gives a*b / 2^261 + r < 1.6r; c is weak-reduced to 1.0001r before it
// is subtracted with the constant 2r, so the difference is below 3.6r, inside what fr29_to_plain accepts (< 16r).
#include <memory>

#include "qap_rows.cuh"
#include "wtns_check.h"

namespace g16 {

__device__ __forceinline__ void wc_verdict(const F29& sa, const F29& sb, const F29& sc, uint32_t c,
                                           uint32_t* __restrict__ first, uint32_t* __restrict__ n_failed) {
  const Fr d = fr29_to_plain(fr29_sub<2>(fr29_mul(sa, sb), fr29_weak_reduce(sc)));
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) nz |= d.v[i];
  if (nz) {
    atomicMin(first, c);
    atomicAdd(n_failed, 1u);
  }
}

// a row per thread: the rows of at most kQapLongRow terms in A, B and C
__device__ __forceinline__ void wc_short_rows(uint32_t block, const QapMat& A, const QapMat& B, const QapMat& Cm,
                                              const Fr* __restrict__ w, const F29* __restrict__ wm, uint32_t m,
                                              uint32_t* first, uint32_t* n_failed) {
  const uint32_t c = block * blockDim.x + threadIdx.x;
  if (c >= m) return;
  if (A.rp[c + 1] - A.rp[c] > kQapLongRow || B.rp[c + 1] - B.rp[c] > kQapLongRow || Cm.rp[c + 1] - Cm.rp[c] > kQapLongRow)
    return;   // the grouped rows below
  const F29 sa = qap_row_sum(A, c, 0u, 1u, w, wm), sb = qap_row_sum(B, c, 0u, 1u, w, wm), sc = qap_row_sum(Cm, c, 0u, 1u, w, wm);
  wc_verdict(sa, sb, sc, c, first, n_failed);
}

// GW lanes per row (64: a wavefront; 8: eight rows per wavefront), as qap_long_rows: the lanes stride over a row's records
// and the partial sums meet in a __shfl_xor tree
template <int GW>
__device__ __forceinline__ void wc_long_rows(uint32_t block, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                             const QapMat& A, const QapMat& B, const QapMat& Cm, const Fr* __restrict__ w,
                                             const F29* __restrict__ wm, uint32_t* first, uint32_t* n_failed) {
  const uint32_t tid = block * blockDim.x + threadIdx.x, gid = tid / GW, lane = tid % GW;
  if (gid >= n_rows) return;   // (whole groups leave together: the shuffles below stay inside a group)
  const uint32_t c = rows[gid];
  F29 s[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s[k] = fr29_weak_reduce(qap_row_sum(k == 0 ? A : k == 1 ? B : Cm, c, lane, (uint32_t)GW, w, wm));
    for (int d = GW / 2; d >= 1; d >>= 1) {
      s[k] = fr29_add(s[k], f29_shfl_xor(s[k], d));
      if (d == 8 || d == 1) s[k] = fr29_weak_reduce(s[k]);   // at most 8 partials below ~2r between reductions
    }
  }
  if (lane == 0) wc_verdict(s[0], s[1], s[2], c, first, n_failed);
}

// ONE launch for the three kinds of rows and for every witness of a chunk (blockIdx.y): blocks [0, nb_long) take the
// rows above kQapWaveRow terms, then nb_mid blocks the rows of 17-64 terms in eight-lane groups, the rest a row per thread.
struct WcRows { const uint32_t* rows; uint32_t n_mid, n_long, nb_long, nb_mid; };
__global__ __launch_bounds__(256) void wtns_check_kernel(WcRows lr, QapMat A, QapMat B, QapMat Cm, const Fr* __restrict__ w,
                                                         const F29* __restrict__ wm, uint32_t n_w, uint32_t m,
                                                         uint32_t* __restrict__ first, uint32_t* __restrict__ n_failed) {
  const uint32_t y = blockIdx.y, blk = blockIdx.x;   // (uniform per block: no divergence between the three bodies)
  w += (size_t)y * n_w;
  wm += (size_t)y * n_w;
  first += y;
  n_failed += y;
  if (blk < lr.nb_long)
    wc_long_rows<64>(blk, lr.rows + lr.n_mid, lr.n_long - lr.n_mid, A, B, Cm, w, wm, first, n_failed);
  else if (blk < lr.nb_long + lr.nb_mid)
    wc_long_rows<8>(blk - lr.nb_long, lr.rows, lr.n_mid, A, B, Cm, w, wm, first, n_failed);
  else
    wc_short_rows(blk - lr.nb_long - lr.nb_mid, A, B, Cm, w, wm, m, first, n_failed);
}
// wm[i] = Montgomery image of witness word i (lazy format), all witnesses of a chunk behind each other
__global__ __launch_bounds__(256) void wtns_check_mont_kernel(const Fr* __restrict__ w, F29* __restrict__ wm, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) wm[i] = fr29_from_plain(w[i]);
}

struct WcDevice {
  int device = 0;
  uint32_t m = 0, n_w = 0, chunk = 1;
  DeviceBuf<uint32_t> rp[3], mid[3], vptr[3], col[3], rows;
  DeviceBuf<F29> val[3];
  uint32_t n_mid = 0, n_long = 0;
  DeviceBuf<Fr> d_w;       // chunk * n_w plain words
  DeviceBuf<F29> d_wm;     // ... and their Montgomery images
  DeviceBuf<uint32_t> d_first, d_nfail;   // chunk words each
  PinnedBuf<uint32_t> h_out;              // 2 * chunk
  PhaseEvents<2> ev;
  DeviceStream st;   // (device_job.h: after everything its work touches)
  ~WcDevice() { (void)hipSetDevice(device); }
};

void wc_device_destroy(WcDevice* d) { delete d; }

static int wc_device_fill(WcDevice* d, const WcCsr& q) {
  G16_HIP(hipSetDevice(d->device));
  G16_HIP(d->st.create());
  G16_HIP(d->ev.create());
  for (int k = 0; k < 3; k++) {
    G16_HIP(upload(d->rp[k], q.rp[k]));
    G16_HIP(upload(d->mid[k], q.mid[k]));
    G16_HIP(upload(d->vptr[k], q.vptr[k]));
    G16_HIP(upload(d->col[k], q.col[k]));
    G16_HIP(upload(d->val[k], q.val[k]));
  }
  G16_HIP(upload(d->rows, q.long_rows));
  const size_t words = (size_t)d->chunk * d->n_w;
  G16_HIP(d->d_w.alloc(words + 1));
  G16_HIP(d->d_wm.alloc(words + 1));
  G16_HIP(d->d_first.alloc(d->chunk));
  G16_HIP(d->d_nfail.alloc(d->chunk));
  G16_HIP(d->h_out.alloc((size_t)d->chunk * 2));
  return G16_OK;
}

int wc_device_create(int device, const WcCsr& q, uint32_t chunk, WcDevice** out) {
  if (const int rc = require_hip_device("wtns check", device)) return rc;
  std::unique_ptr<WcDevice> d(new WcDevice);
  d->device = device;
  d->m = q.m;
  d->n_w = q.n_w;
  d->chunk = chunk < 1 ? 1 : (chunk > 65535 ? 65535 : chunk);   // (a chunk is the y dimension of one grid)
  d->n_mid = q.n_mid;
  d->n_long = q.n_long;
  if (const int rc = wc_device_fill(d.get(), q)) return rc;
  *out = d.release();
  return G16_OK;
}

int wc_device_check(WcDevice* d, const uint8_t* const* bodies, size_t count, uint32_t* first, uint32_t* n_failed, float ms[2]) {
  G16_HIP(hipSetDevice(d->device));
  if (ms) ms[0] = ms[1] = 0.f;
  WcRows lr;
  lr.rows = d->rows.p;
  lr.n_mid = d->n_mid;
  lr.n_long = d->n_long;
  lr.nb_long = (d->n_long - d->n_mid + 3) / 4;
  lr.nb_mid = (d->n_mid + 31) / 32;
  const QapMat A{d->rp[0].p, d->mid[0].p, d->vptr[0].p, d->col[0].p, d->val[0].p},
      B{d->rp[1].p, d->mid[1].p, d->vptr[1].p, d->col[1].p, d->val[1].p},
      Cm{d->rp[2].p, d->mid[2].p, d->vptr[2].p, d->col[2].p, d->val[2].p};
  hipStream_t st = d->st;
  StreamDrain drain(st);   // (the bodies are the caller's)
  for (size_t at = 0; at < count; at += d->chunk) {
    const uint32_t cnt = (uint32_t)(count - at < d->chunk ? count - at : d->chunk);
    G16_HIP(d->ev.record(0, st));
    for (uint32_t i = 0; i < cnt; i++)
      if (d->n_w) G16_HIP(hipMemcpyAsync(d->d_w.p + (size_t)i * d->n_w, bodies[at + i], (size_t)d->n_w * 32, hipMemcpyHostToDevice, st));
    G16_HIP(d->ev.record(1, st));
    G16_HIP(hipMemsetAsync(d->d_first.p, 0xff, (size_t)cnt * 4, st));   // the verdict of the call before is gone
    G16_HIP(hipMemsetAsync(d->d_nfail.p, 0, (size_t)cnt * 4, st));
    if (d->m) {
      const size_t words = (size_t)cnt * d->n_w;
      wtns_check_mont_kernel<<<(unsigned)((words + 255) / 256), 256, 0, st>>>(d->d_w.p, d->d_wm.p, words);
      const dim3 grid(lr.nb_long + lr.nb_mid + (d->m + 255) / 256, cnt);
      wtns_check_kernel<<<grid, 256, 0, st>>>(lr, A, B, Cm, d->d_w.p, d->d_wm.p, d->n_w, d->m, d->d_first.p, d->d_nfail.p);
      G16_HIP(hipGetLastError());
    }
    G16_HIP(d->ev.record(2, st));
    G16_HIP(hipMemcpyAsync(d->h_out.p, d->d_first.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    G16_HIP(hipMemcpyAsync(d->h_out.p + cnt, d->d_nfail.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    G16_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < cnt; i++) {
      first[at + i] = d->h_out.p[i];
      n_failed[at + i] = d->h_out.p[cnt + i];
    }
    if (ms)
      for (int k = 0; k < 2; k++) ms[k] += d->ev.ms(k);
  }
  drain.dismiss();
  return G16_OK;
}

}  // namespace g16
