// The ptau leg of `snarkjs zkey verify` ([EXT] snarkjs 0.4.12 zkey_verify_frominit.js sectionHasSameRatioH): section 9
// of the key under test against the first 2N - 1 points of the ceremony's section 2 (zkey_mpc.cpp verify_core).
//
// N = 2^L, w = the primitive 2N-th root of the NTT tables, u = N standard-form values below r with u[N-1] = 0:
//   rho[i] = (1 / N) sum_k u[k] w^((2i+1) k),  i < N     import (bit-reversed) -> coset table -> ntt_dit_forward -> export
//   t      = u[0..N-2] | 0 | -u[0..N-2] mod r,  2N - 1   zkey_h_t_kernel
// so that, for the H points H_i of ANY key set up from the ceremony tau (point 2i+1 of block L+1 of section 12, the full
// Lagrange block or the one `prepare phase2` writes from 2N - 1 powers: they differ by a multiple of w^(2i+1), and
// sum_i rho[i] w^(2i+1) = u[N-1] = 0) and its powers P_j = [tau^j]G1:
//   2N sum_i rho[i] H_i = sum_j t[j] P_j.
// WHERE THE CONSTANT SITS: the combination the check draws is 2 sum_k u[k] w^((2i+1) k) = 2N rho[i].  The tables' coset
// vector already carries 1 / N, so rho keeps the factor 1 / 2N and the host multiplies the one point S = sum rho[i] H_i
// by 2N (L + 1 doublings) before the pairing.  tests/zkey_verify_ptau_ref.py restates the same choice.
// The transform is linear, so the standard-form words go through ntt_import / ntt_export (which read and write
// Montgomery images) unchanged: standard form in, standard form out.
#include <chrono>

#include "internal.h"

namespace g16 {

// One lane per k < N: lane k < N - 1 copies u[k] to t[k] and writes r - u[k] (0 for u[k] = 0) to t[N + k]; lane N - 1
// writes the zero between the halves.  16-byte loads and stores (Fr is alignas(16)), no LDS.
__global__ __launch_bounds__(256) void zkey_h_t_kernel(const Fr* __restrict__ u, Fr* __restrict__ t, uint32_t N) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= N) return;
  if (k == N - 1) { t[k] = fp_zero<FrParams>(); return; }
  const Fr x = u[k];
  t[k] = x;
  t[(size_t)N + k] = fp_neg(x);   // N + k <= 2N - 2
}

namespace {
struct HJob {   // (device_job.h: the stream last)
  NttTables tab;
  DeviceBuf<Fr> d_u, d_rho, d_t;
  DeviceBuf<F29> d_z;
  DeviceTimer timer;
  DeviceStream st;
  // u (host, N x 32 bytes) -> d_rho (N) and d_t (2N - 1), waited for; *ms = device time of tables, transform and kernel
  int form(int device, const uint8_t* u, int L, float* ms) {
    if (L < 1 || L > 27) { set_error("zkey h scalars: log_n out of range (need 1..27)"); return G16_E_ARG; }
    if (const int rc = require_hip_device("zkey h scalars", device)) return rc;
    G16_HIP(hipSetDevice(device));
    const size_t N = (size_t)1 << L;
    DeviceJob job("zkey h scalars");
    if (job.fail(st.create()) || job.fail(timer.create()) || job.fail(d_u.alloc(N)) || job.fail(d_rho.alloc(N)) ||
        job.fail(d_t.alloc(2 * N - 1)) || job.fail(d_z.alloc(N)) ||
        job.fail(hipMemcpyAsync(d_u.p, u, N * sizeof(Fr), hipMemcpyHostToDevice, st)) || job.fail(timer.start(st)))
      return job.rc;
    F29* vz[1] = {d_z.p};
    int rc = ntt_tables_create(tab, L, st);
    if (rc || (rc = ntt_import(tab, d_u.p, d_z.p, /*bitrev=*/true, st)) || (rc = ntt_coset_scale(tab, vz, 1, st)) ||
        (rc = ntt_dit_forward(tab, vz, 1, st)) || (rc = ntt_export(tab, d_z.p, d_rho.p, /*bitrev=*/false, /*scale_ninv=*/false, st)))
      return rc;
    zkey_h_t_kernel<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(d_u.p, d_t.p, (uint32_t)N);
    if (job.fail(hipGetLastError()) || job.fail(timer.stop(st)) || job.fail(hipStreamSynchronize(st))) return job.rc;
    if (ms) *ms = timer.ms();
    return G16_OK;
  }
};
}  // namespace

int zkey_verify_h(int device, const uint8_t* u, int log_n, const uint8_t* sec9, const uint8_t* tau_g1, uint8_t S[64],
                  uint8_t T[64], ZkeyHStats* stats) {
  HJob job;
  float ntt_ms = 0.f;
  if (const int rc = job.form(device, u, log_n, &ntt_ms)) return rc;
  const size_t N = (size_t)1 << log_n;
  const auto t0 = std::chrono::steady_clock::now();
  if (const int rc = g1_multiexp_device(sec9, job.d_rho.p, N, 0, S)) return rc;
  if (const int rc = g1_multiexp_device(tau_g1, job.d_t.p, 2 * N - 1, 0, T)) return rc;
  if (stats) {
    stats->ntt_ms = ntt_ms;
    stats->msm_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return G16_OK;
}

int zkey_h_rho(int device, const uint8_t* u, int log_n, uint8_t* rho_out) {
  HJob job;
  if (const int rc = job.form(device, u, log_n, nullptr)) return rc;
  G16_HIP(hipMemcpy(rho_out, job.d_rho.p, ((size_t)1 << log_n) * sizeof(Fr), hipMemcpyDeviceToHost));
  return G16_OK;
}

}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_h_scalars(int device, const uint8_t* u, uint32_t log_n, uint8_t* rho_out, uint8_t* t_out) {
  if (!u || !rho_out || !t_out) { set_error("NULL argument"); return G16_E_ARG; }
  if (log_n < 1 || log_n > 27) { set_error("zkey h scalars: log_n out of range (need 1..27)"); return G16_E_ARG; }
  const size_t N = (size_t)1 << log_n;
  for (int i = 0; i < 32; i++)
    if (u[(N - 1) * 32 + i]) { set_error("zkey h scalars: u[N-1] must be zero"); return G16_E_ARG; }
  HJob job;
  if (const int rc = job.form(device, u, (int)log_n, nullptr)) return rc;
  G16_HIP(hipMemcpy(rho_out, job.d_rho.p, N * sizeof(Fr), hipMemcpyDeviceToHost));
  G16_HIP(hipMemcpy(t_out, job.d_t.p, (2 * N - 1) * sizeof(Fr), hipMemcpyDeviceToHost));
  return G16_OK;
}
