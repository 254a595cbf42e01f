// ES256 (ECDSA over NIST P-256 with SHA-256) batch verification on the device: the pass signature half of an NZCP
// relying party's check (the circuit publishes toBeSignedSha256 so that the verifier can check the Ministry's signature;
// @vaxxnz/nzcp does the same one pass at a time on the CPU).
//
// Device schedule (p256.cuh, the canonical 8 x 32 Montgomery limbs):
//   create   es256_table_kernel   : 4-bit window tables d * 16^w * P (d = 1..15, w < 64), affine, resident, for G and
//                                   every key: the shape of verify_ic_table_kernel, 61 KB per point
//   batch 1  es256_scalars_kernel : a lane per signature: range check, e = digest mod n, w = 1 / s (Fermat, ~390
//                                   products in the scalar field), u1 = e w, u2 = r w
//         2  es256_sum_kernel     : kEs256Lanes = 16 lanes per signature: a lane adds its 8 of the 128 table entries by
//                                   mixed additions (no doublings), a shuffle tree of 4 full additions joins the 16
//                                   sums, lane 0 compares r Z^2 (and (r + n) Z^2) with X
// A signature is ~2 k field products: accumulators live in registers, nothing is called through scratch-heavy chains.
// Signatures are attacker-chosen, so the additions' exceptional cases (equal operands, opposite operands, infinity)
// are reachable and handled in p256_madd / p256_add; lanes that take them diverge from their wavefront for one addition.
#include <hip/hip_runtime.h>

#include <memory>

#include "es256.h"
#include "internal.h"

namespace g16 {
namespace {

constexpr uint32_t kBlock = 64;

// tbl[(j * 64 + w) * 15 + d - 1] = d * 16^w * points[j]
__global__ __launch_bounds__(64) void es256_table_kernel(const P256Affine* __restrict__ points, uint32_t n,
                                                         P256Affine* __restrict__ tbl) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kP256Win) return;
  P256Affine row[kP256Row];
  p256_table_row(points[t / kP256Win], t % kP256Win, row);
  for (int d = 0; d < kP256Row; d++) tbl[(size_t)t * kP256Row + d] = row[d];
}

// u[i] = u1 | u2 (16 words, standard form), live[i] = passed the range check
__global__ __launch_bounds__(64) void es256_scalars_kernel(const uint8_t* __restrict__ hashes, const uint8_t* __restrict__ sigs,
                                                           uint32_t count, uint32_t* __restrict__ u, uint8_t* __restrict__ live) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  P256Fn u1, u2;
  live[i] = es256_scalars(hashes + (size_t)i * 32, sigs + (size_t)i * 64, u1, u2) ? 1 : 0;
  for (int k = 0; k < 8; k++) {
    u[(size_t)i * 16 + k] = u1.v[k];
    u[(size_t)i * 16 + 8 + k] = u2.v[k];
  }
}

__device__ __forceinline__ P256Fp shfl_down_fp(const P256Fp& a, uint32_t s) {
  P256Fp r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] = (uint32_t)__shfl_down((int)a.v[k], s, (int)kEs256Lanes);
  return r;
}

// groups of kEs256Lanes lanes never straddle a wavefront (64 = 4 groups); a group past the batch, or of a signature
// the range check rejected, sums nothing but still takes part in the shuffles
__global__ __launch_bounds__(64) void es256_sum_kernel(const P256Affine* __restrict__ tbl, const uint32_t* __restrict__ u,
                                                       const uint8_t* __restrict__ live, const uint8_t* __restrict__ sigs,
                                                       const uint32_t* __restrict__ key_idx, uint32_t count,
                                                       uint8_t* __restrict__ ok) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = g / kEs256Lanes, lane = g % kEs256Lanes;
  const bool on = i < count && live[i];
  P256Jac acc;
  p256_set_inf(acc);
  if (on) es256_slice_sum(acc, tbl, key_idx ? key_idx[i] : 0u, u + (size_t)i * 16, u + (size_t)i * 16 + 8, lane, kEs256Lanes);
  for (uint32_t s = kEs256Lanes / 2; s >= 1; s >>= 1) {
    P256Jac o;
    o.X = shfl_down_fp(acc.X, s);
    o.Y = shfl_down_fp(acc.Y, s);
    o.Z = shfl_down_fp(acc.Z, s);
    if (lane < s) p256_add(acc, o);
  }
  if (lane == 0 && i < count)
    ok[i] = on && p256_x_equals_r(acc.X, acc.Z, pf_load_be<P256FnParams>(sigs + (size_t)i * 64)) ? 1 : 0;
}

__global__ __launch_bounds__(64) void es256_op_kernel(int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                      uint8_t* __restrict__ out, uint32_t n, uint32_t sa, uint32_t sb, uint32_t so) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  p256_op_one(op, a + (size_t)i * sa, b + (size_t)i * sb, out + (size_t)i * so);
}

}  // namespace

struct Es256Device {
  int device = 0;
  uint32_t n_keys = 0;
  DeviceBuf<P256Affine> d_tbl;
  // per-batch scratch, grown on demand
  size_t cap = 0;
  DeviceBuf<uint8_t> d_hashes, d_sigs;
  DeviceBuf<uint32_t> d_key, d_u;
  DeviceBuf<uint8_t> d_live, d_ok;
  PhaseEvents<2> ev;
  DeviceStream st;   // (device_job.h: after everything its work touches)
  size_t in_flight = 0;
  ~Es256Device() { (void)hipSetDevice(device); }
};

int es256_device_create(int device, const P256Affine* points, uint32_t n_points, Es256Device** out) {
  if (const int rc = require_hip_device(device, "es256 verifier: no HIP device (device -1 selects the host route)",
                                        "es256 verifier: bad device ordinal"))
    return rc;
  std::unique_ptr<Es256Device> D(new Es256Device());
  D->device = device;
  D->n_keys = n_points - 1;
  G16_HIP(hipSetDevice(device));
  G16_HIP(D->st.create());
  G16_HIP(D->ev.create());
  DeviceBuf<P256Affine> d_points;
  G16_HIP(d_points.alloc(n_points));
  G16_HIP(D->d_tbl.alloc((size_t)n_points * kP256TblPoint));
  StreamDrain drain(D->st);   // (points is the caller's, d_points a temporary)
  G16_HIP(hipMemcpyAsync(d_points.p, points, (size_t)n_points * sizeof(P256Affine), hipMemcpyHostToDevice, D->st));
  const uint32_t nt = n_points * kP256Win;
  es256_table_kernel<<<(nt + kBlock - 1) / kBlock, kBlock, 0, D->st>>>(d_points.p, n_points, D->d_tbl.p);
  G16_HIP(hipGetLastError());
  G16_HIP(hipStreamSynchronize(D->st));
  drain.dismiss();
  *out = D.release();
  return G16_OK;
}

void es256_device_destroy(Es256Device* D) { delete D; }

static int ensure_scratch(Es256Device* D, size_t count) {
  if (count <= D->cap) return G16_OK;
  D->cap = 0;
  G16_HIP(D->d_hashes.alloc(count * 32));
  G16_HIP(D->d_sigs.alloc(count * 64));
  G16_HIP(D->d_key.alloc(count));
  G16_HIP(D->d_u.alloc(count * 16));
  G16_HIP(D->d_live.alloc(count));
  G16_HIP(D->d_ok.alloc(count));
  D->cap = count;
  return G16_OK;
}

// a batch that cannot be finished: wait for what it enqueued and forget it
void es256_device_abandon(Es256Device* D) {
  (void)hipSetDevice(D->device);
  (void)hipStreamSynchronize(D->st);
  D->in_flight = 0;
}

// the two kernels over the digests, signatures and key indices in the scratch (key: NULL = key 0 for every signature)
static int launch_scratch(Es256Device* D, const uint32_t* key, size_t count) {
  const uint32_t n = (uint32_t)count;
  hipStream_t st = D->st;
  G16_HIP(D->ev.record(0, st));
  es256_scalars_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, st>>>(D->d_hashes.p, D->d_sigs.p, n, D->d_u.p, D->d_live.p);
  G16_HIP(D->ev.record(1, st));
  const uint64_t lanes = (uint64_t)n * kEs256Lanes;
  es256_sum_kernel<<<(uint32_t)((lanes + kBlock - 1) / kBlock), kBlock, 0, st>>>(D->d_tbl.p, D->d_u.p, D->d_live.p, D->d_sigs.p, key, n,
                                                                                 D->d_ok.p);
  G16_HIP(D->ev.record(2, st));
  G16_HIP(hipGetLastError());
  D->in_flight = count;
  return G16_OK;
}

int es256_device_launch(Es256Device* D, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx, size_t count) {
  G16_HIP(hipSetDevice(D->device));
  if (const int rc = ensure_scratch(D, count)) return rc;
  hipStream_t st = D->st;
  D->in_flight = 0;
  StreamDrain drain(st);   // (the host buffers are promised to a finish, which a failing launch does not get)
  G16_HIP(hipMemcpyAsync(D->d_hashes.p, hashes, count * 32, hipMemcpyHostToDevice, st));
  G16_HIP(hipMemcpyAsync(D->d_sigs.p, sigs, count * 64, hipMemcpyHostToDevice, st));
  if (key_idx) G16_HIP(hipMemcpyAsync(D->d_key.p, key_idx, count * 4, hipMemcpyHostToDevice, st));
  if (const int rc = launch_scratch(D, key_idx ? D->d_key.p : nullptr, count)) return rc;
  drain.dismiss();
  return G16_OK;
}

int es256_device_scratch(Es256Device* D, size_t count, Es256Scratch* out) {
  G16_HIP(hipSetDevice(D->device));
  if (const int rc = ensure_scratch(D, count)) return rc;
  *out = Es256Scratch{D->d_hashes.p, D->d_sigs.p, D->d_key.p, (void*)D->st.s};
  return G16_OK;
}

// the two kernels of es256_device_launch over digests, signatures and key indices that a kernel on the handle's stream
// has written into the scratch (count <= the capacity es256_device_scratch was asked for); the caller abandons the
// batch if this fails
int es256_device_launch_resident(Es256Device* D, size_t count) {
  G16_HIP(hipSetDevice(D->device));
  if (count > D->cap) { set_error("es256 verify: the resident batch is larger than the scratch"); return G16_E_STATE; }
  return launch_scratch(D, D->d_key.p, count);
}

int es256_device_finish(Es256Device* D, uint8_t* ok, float ms[2]) {
  G16_HIP(hipSetDevice(D->device));
  const size_t count = D->in_flight;
  D->in_flight = 0;
  StreamDrain drain(D->st);   // (ok is the caller's)
  G16_HIP(hipMemcpyAsync(ok, D->d_ok.p, count, hipMemcpyDeviceToHost, D->st));
  G16_HIP(hipStreamSynchronize(D->st));
  drain.dismiss();
  for (int k = 0; k < 2; k++) ms[k] = D->ev.ms(k);
  return G16_OK;
}

int es256_device_op(int device, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (const int rc = require_hip_device(device, "p256 operator: no HIP device (device -1 selects the host route)",
                                        "p256 operator: bad device ordinal"))
    return rc;
  G16_HIP(hipSetDevice(device));
  size_t sa, sb, so;
  p256_op_strides(op, &sa, &sb, &so);
  DeviceJob job("p256 operator");
  DeviceBuf<uint8_t> d_a, d_b, d_out;
  if (job.fail(d_a.alloc(n * sa)) || job.fail(d_b.alloc(n * sb)) || job.fail(d_out.alloc(n * so)) ||
      job.fail(hipMemcpy(d_a.p, a, n * sa, hipMemcpyHostToDevice)) ||
      (sb && job.fail(hipMemcpy(d_b.p, b, n * sb, hipMemcpyHostToDevice))))
    return job.rc;
  es256_op_kernel<<<(uint32_t)((n + kBlock - 1) / kBlock), kBlock>>>(op, d_a.p, d_b.p, d_out.p, (uint32_t)n, (uint32_t)sa,
                                                                     (uint32_t)sb, (uint32_t)so);
  if (job.fail(hipGetLastError()) || job.fail(hipMemcpy(out, d_out.p, n * so, hipMemcpyDeviceToHost))) return job.rc;
  return G16_OK;
}

}  // namespace g16
