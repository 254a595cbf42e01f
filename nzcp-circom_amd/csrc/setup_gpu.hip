// Fixed-base scalar multiplication on the device: out[i] = [k_i] G for the millions of trapdoor scalars of a
// TEST-ONLY Groth16 setup, the trapdoor route of setup_groth16.cpp::setup_core: the scalars
// u_i(tau), v_i(tau), (beta u_i + alpha v_i + w_i)/gamma|delta, L_{2i+1}(tau)/delta are evaluated on the host from a
// KNOWN trapdoor, so anyone holding it can forge proofs.  The real `snarkjs groth16 setup` ([EXT] snarkjs 0.4.12) takes
// its points from a prepared powers-of-tau file instead: that route is setup_groth16.cpp::g16_groth16_setup_ptau with the
// sparse point sums of setup_ptau.hip.  Also the generator of the test ceremonies (g16_ptau_synth).
//
// Two kernels per chunk of points, both on the canonical 8x32-bit Montgomery field (fp.cuh / ec.cuh: exact,
// complete additions -- this is create-time work, the bytes must equal the host path's bytes):
//   setup_fixed_mul_kernel : one lane per scalar; the scalar leaves Montgomery form, its `nwin` wb-bit digits index
//                            the table [nwin][2^wb - 1] of d * 2^(wb j) * G (a few hundred KB: L2 resident) and are
//                            mixed-added into an XYZZ accumulator.
//   setup_to_affine_kernel : (setup_affine.cuh) one lane per kBatch consecutive points, one inversion per batch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "ec.cuh"
#include "internal.h"
#include "setup_affine.cuh"

namespace g16 {
namespace {

template <class FC>
__global__ __launch_bounds__(256) void setup_fixed_mul_kernel(const Affine<FC>* __restrict__ tbl, int wb, int nwin,
                                                               const Fr* __restrict__ ks_mont, uint32_t n,
                                                               XYZZ<FC>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr k = fp_from_mont(ks_mont[i]);
  const uint32_t row = (1u << wb) - 1, mask = row;
  XYZZ<FC> acc;
  xyzz_set_inf(acc);
  for (int j = 0; j < nwin; j++) {
    const int pos = j * wb;
    uint64_t v = k.v[pos >> 5];
    if ((pos >> 5) + 1 < 8) v |= (uint64_t)k.v[(pos >> 5) + 1] << 32;
    const uint32_t d = (uint32_t)(v >> (pos & 31)) & mask;
    if (d) {
      const Affine<FC> q = tbl[(size_t)j * row + d - 1];
      xyzz_madd(acc, q);
    }
  }
  out[i] = acc;
}

template <class FC>
int fixed_mul_device(int device, const Affine<FC>* h_tbl, int wb, int nwin, const Fr* ks_mont, size_t n, uint8_t* out) {
  if (n == 0) return G16_OK;
  if (const int rc = require_hip_device(device, "setup: no HIP device (g16_setup_device selected the GPU path)",
                                        "setup: bad device ordinal"))
    return rc;
  G16_HIP(hipSetDevice(device));
  const size_t tbl_n = (size_t)nwin * (((size_t)1 << wb) - 1);
  const size_t chunk = n < ((size_t)1 << 20) ? n : ((size_t)1 << 20);
  static const bool trace = getenv("G16_TRACE_HOST") != nullptr;
  DeviceJob job("setup");
  DeviceBuf<Affine<FC>> d_tbl, d_aff;
  DeviceBuf<Fr> d_k;
  DeviceBuf<XYZZ<FC>> d_acc;
  DeviceTimer timer;
  DeviceStream st;
  float kern_ms = 0.f;
  if (job.fail(st.create()) || (trace && job.fail(timer.create())) || job.fail(d_tbl.alloc(tbl_n)) || job.fail(d_k.alloc(chunk)) ||
      job.fail(d_acc.alloc(chunk)) || job.fail(d_aff.alloc(chunk)) ||
      job.fail(hipMemcpyAsync(d_tbl.p, h_tbl, tbl_n * sizeof(Affine<FC>), hipMemcpyHostToDevice, st)))
    return job.rc;
  for (size_t base = 0; base < n; base += chunk) {
    const uint32_t cnt = (uint32_t)(base + chunk < n ? chunk : n - base);
    if (job.fail(hipMemcpyAsync(d_k.p, ks_mont + base, (size_t)cnt * sizeof(Fr), hipMemcpyHostToDevice, st))) return job.rc;
    if (trace) (void)timer.start(st);
    setup_fixed_mul_kernel<FC><<<(cnt + 255) / 256, 256, 0, st>>>(d_tbl.p, wb, nwin, d_k.p, cnt, d_acc.p);
    const uint32_t nb = (cnt + kBatch - 1) / kBatch;
    setup_to_affine_kernel<FC><<<(nb + 255) / 256, 256, 0, st>>>(d_acc.p, d_aff.p, cnt);
    if (trace) (void)timer.stop(st);
    if (job.fail(hipGetLastError()) ||
        job.fail(hipMemcpyAsync(out + base * sizeof(Affine<FC>), d_aff.p, (size_t)cnt * sizeof(Affine<FC>),
                                hipMemcpyDeviceToHost, st)) ||
        job.fail(hipStreamSynchronize(st)))
      return job.rc;
    if (trace) kern_ms += timer.ms();
  }
  if (trace)
    fprintf(stderr, "[g16 setup] %s fixed-base: %zu scalars, kernels %.3f ms (%.1f M points/s)\n",
            sizeof(Affine<FC>) == 64 ? "G1" : "G2", n, kern_ms, kern_ms > 0 ? n / kern_ms / 1e3 : 0.0);
  return G16_OK;
}

}  // namespace

int setup_fixed_mul_g1(int device, const G1Affine* tbl, int wb, int nwin, const Fr* ks_mont, size_t n, uint8_t* out) {
  return fixed_mul_device<FqOps>(device, tbl, wb, nwin, ks_mont, n, out);
}
int setup_fixed_mul_g2(int device, const G2Affine* tbl, int wb, int nwin, const Fr* ks_mont, size_t n, uint8_t* out) {
  return fixed_mul_device<Fq2Ops>(device, tbl, wb, nwin, ks_mont, n, out);
}

}  // namespace g16
