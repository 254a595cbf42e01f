// Groth16 batch verifier on the device (the acceptance check of SURVEY 3.4).
//
// Replaces `snarkjs groth16 verify` ([EXT] snarkjs 0.4.12 groth16_verify.js: cpub = IC[0] + sum pub_i IC[i+1] by
// G1.timesFr / add, then curve.pairingEq(-A, B, cpub, gamma2, C, delta2, alpha1, beta2); pins
// /root/reference/yarn.lock:987-1001; in the reference repo only the README's "verify" step and the PLONK twin
// Makefile:30-33 point at it) for MANY proofs against ONE verification key: proof i is accepted iff
//     e(-A_i, B_i) e(vk_x_i, gamma2) e(C_i, delta2) e(alpha1, beta2) = 1,   vk_x_i = IC_0 + sum_j pub_ij IC_{j+1}.
// Every proof gets its own verdict (no random linear combination: a rejected proof is identified, and the verdicts
// are exactly the one-at-a-time verdicts).
//
// Device schedule (all on the canonical 8x32 Montgomery field, pairing.cuh / ec.cuh):
//   create   verify_ic_table_kernel : 4-bit window tables d * 16^w * IC_j (d = 1..15, w < 64), affine, resident
//            host                    : line coefficients of gamma2 and delta2 (the G2 sides that never change), the
//                                      Miller value of (alpha1, beta2)
//   batch 1  verify_vkx_kernel      : a 256-lane workgroup per proof: lanes stride over the public signals, add the
//                                      table entries of the non-zero digits, LDS tree of XYZZ sums, -> affine vk_x
//         2  verify_miller_kernel   : a lane per (proof, pairing): (-A, B) with the lines of B computed on the fly,
//                                      (vk_x, gamma2) and (C, delta2) from the resident coefficients
//         3  verify_final_kernel    : a lane per proof: product of the three Miller values and the key's fourth,
//                                      final exponentiation, == 1
// The pairing work is ~35 k Fq products per proof on lanes that each own a 384-byte Fq12 accumulator: the tower
// products are called (not inlined) and spill to scratch -- a latency-bound, embarrassingly parallel kernel whose
// throughput comes from the batch size (BASELINE config 3's 1 024 proofs fill 48 + 16 wavefronts).
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <vector>

#include "internal.h"
#include "pairing.cuh"

namespace g16 {
namespace {

constexpr int kIcWin = 64;          // 4-bit windows of a 256-bit scalar
constexpr int kIcRow = 15;          // non-zero digits

// tbl[(j * 64 + w) * 15 + d - 1] = d * 16^w * IC_j  (affine; all-zero = infinity)
__global__ __launch_bounds__(64) void verify_ic_table_kernel(const G1Affine* __restrict__ ic, uint32_t n,
                                                             G1Affine* __restrict__ tbl) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kIcWin) return;
  const uint32_t j = t / kIcWin, w = t % kIcWin;
  G1XYZZ b;
  xyzz_from_affine(b, ic[j]);
  for (uint32_t k = 0; k < 4 * w; k++) xyzz_dbl(b);
  G1Affine base;
  xyzz_to_affine(base, b);
  G1XYZZ acc;
  xyzz_set_inf(acc);
  for (int d = 0; d < kIcRow; d++) {
    G1Affine a;
    if (aff_is_inf(base)) {
      a.x = FqOps::zero();
      a.y = FqOps::zero();
    } else {
      xyzz_madd(acc, base);
      xyzz_to_affine(a, acc);
    }
    tbl[(size_t)t * kIcRow + d] = a;
  }
}

// vkx[i] = IC_0 + sum_j pub[i][j] * IC_{j+1}   (pub: standard-form 256-bit integers, any value)
__global__ __launch_bounds__(256) void verify_vkx_kernel(const G1Affine* __restrict__ ic, const G1Affine* __restrict__ tbl,
                                                          const uint32_t* __restrict__ pub, uint32_t n_public,
                                                          G1Affine* __restrict__ vkx) {
  __shared__ G1XYZZ sm[256];
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  G1XYZZ acc;
  xyzz_set_inf(acc);
  for (uint32_t j = t; j < n_public; j += 256) {
    const uint32_t* k = pub + ((size_t)i * n_public + j) * 8;
    for (int w = 0; w < kIcWin; w++) {
      const uint32_t d = (k[w >> 3] >> (4 * (w & 7))) & 15u;
      if (!d) continue;
      const G1Affine q = tbl[((size_t)(j + 1) * kIcWin + w) * kIcRow + d - 1];
      if (!aff_is_inf(q)) xyzz_madd(acc, q);
    }
  }
  sm[t] = acc;
  __syncthreads();
  for (uint32_t s = 128; s >= 1; s >>= 1) {
    if (t < s) {
      G1XYZZ a = sm[t];
      const G1XYZZ b = sm[t + s];
      xyzz_add(a, b);
      sm[t] = a;
    }
    __syncthreads();
  }
  if (t == 0) {
    G1XYZZ a = sm[0];
    const G1Affine ic0 = ic[0];
    if (!aff_is_inf(ic0)) xyzz_madd(a, ic0);
    G1Affine r;
    xyzz_to_affine(r, a);
    vkx[i] = r;
  }
}

struct ProofM {           // a proof in Montgomery form
  G1Affine a;
  G2Affine b;
  G1Affine c;
};

// standard-form proof bytes -> Montgomery, validity flags: bit 0 = a coordinate is not below q or a point is off its
// curve (the proof is rejected), bit 1 = A or B is infinity (their pairing is 1), bit 2 = C is infinity
__global__ __launch_bounds__(64) void verify_load_kernel(const g16_proof* __restrict__ proofs, uint32_t count,
                                                         PairingConsts pc, ProofM* __restrict__ out,
                                                         uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  static const uint32_t kQ[8] = G16_FQ_P;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&proofs[i]);
  Fq v[8];
  bool bad = false;
  for (int k = 0; k < 8; k++) {
    Fq x;
    bool lt = false, decided = false;
    for (int l = 7; l >= 0; l--) {
      x.v[l] = w[k * 8 + l];
      if (!decided && x.v[l] != kQ[l]) { lt = x.v[l] < kQ[l]; decided = true; }
    }
    bad |= !lt;
    v[k] = fp_to_mont(x);
  }
  ProofM p;
  p.a.x = v[0]; p.a.y = v[1];
  p.b.x = Fq2{v[2], v[3]}; p.b.y = Fq2{v[4], v[5]};
  p.c.x = v[6]; p.c.y = v[7];
  uint32_t f = 0;
  const bool a_inf = aff_is_inf(p.a), b_inf = aff_is_inf(p.b), c_inf = aff_is_inf(p.c);
  if (!a_inf && !g1_on_curve(p.a)) bad = true;
  if (!b_inf && !g2_on_curve(p.b, pc)) bad = true;
  if (!c_inf && !g1_on_curve(p.c)) bad = true;
  if (bad) f |= 1u;
  if (a_inf || b_inf) f |= 2u;
  if (c_inf) f |= 4u;
  out[i] = p;
  flags[i] = f;
}

// blockIdx.y = pairing: 0 = (-A, B), 1 = (vk_x, gamma2), 2 = (C, delta2); ml[3 i + pairing]
__global__ __launch_bounds__(64) void verify_miller_kernel(const ProofM* __restrict__ proofs, const uint32_t* __restrict__ flags,
                                                           const G1Affine* __restrict__ vkx,
                                                           const EllCoeffs* __restrict__ co_gamma,
                                                           const EllCoeffs* __restrict__ co_delta, uint32_t count,
                                                           PairingConsts pc, Fq12* __restrict__ ml) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t which = blockIdx.y;
  const uint32_t f = flags[i];
  Fq12 r = f12_one();
  if (!(f & 1u)) {
    if (which == 0) {
      if (!(f & 2u)) {
        G1Affine p = proofs[i].a;
        p.y = fp_neg(p.y);
        const G2Affine q = proofs[i].b;
        r = miller_loop(p, q, pc);
      }
    } else if (which == 1) {
      const G1Affine p = vkx[i];
      if (!aff_is_inf(p)) r = miller_loop_pre(p, co_gamma);
    } else {
      if (!(f & 4u)) {
        const G1Affine p = proofs[i].c;
        r = miller_loop_pre(p, co_delta);
      }
    }
  }
  ml[(size_t)i * 3 + which] = r;
}

__global__ __launch_bounds__(64) void verify_final_kernel(const Fq12* __restrict__ ml, const uint32_t* __restrict__ flags,
                                                          uint32_t count, PairingConsts pc, Fq12 ml_alphabeta,
                                                          uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (flags[i] & 1u) { ok[i] = 0; return; }
  Fq12 f = f12_mul(ml[(size_t)i * 3], ml[(size_t)i * 3 + 1]);
  f = f12_mul(f, ml[(size_t)i * 3 + 2]);
  f = f12_mul(f, ml_alphabeta);
  ok[i] = f12_is_one(final_exponentiation(f, pc)) ? 1 : 0;
}

// layer-test operator: out[i] = final_exponentiation(miller_loop(P_i, Q_i)) as 12 standard-form Fq words per pair,
// in the order of the W^k coefficients (a, b), k = 0..5 (tests/test_gpu_verify.py compares with oracle/bn254.py)
__global__ __launch_bounds__(64) void verify_pairing_op_kernel(const uint32_t* __restrict__ in, uint32_t count,
                                                               PairingConsts pc, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  Fq v[6];
  for (int k = 0; k < 6; k++) {
    Fq x;
    for (int l = 0; l < 8; l++) x.v[l] = in[(size_t)i * 48 + k * 8 + l];
    v[k] = fp_to_mont(x);
  }
  const G1Affine p{v[0], v[1]};
  const G2Affine q{Fq2{v[2], v[3]}, Fq2{v[4], v[5]}};
  const Fq12 e = final_exponentiation(miller_loop(p, q, pc), pc);
  const Fq2* w[6] = {&e.c0.c0, &e.c1.c0, &e.c0.c1, &e.c1.c1, &e.c0.c2, &e.c1.c2};
  for (int k = 0; k < 6; k++) {
    const Fq a = fp_from_mont(w[k]->a), b = fp_from_mont(w[k]->b);
    for (int l = 0; l < 8; l++) {
      out[(size_t)i * 96 + k * 16 + l] = a.v[l];
      out[(size_t)i * 96 + k * 16 + 8 + l] = b.v[l];
    }
  }
}

}  // namespace
}  // namespace g16

using namespace g16;

struct g16_verifier {
  int device = 0;
  uint32_t n_public = 0;
  PairingConsts pc;
  Fq12 ml_alphabeta;
  DeviceBuf<G1Affine> d_ic, d_tbl;
  DeviceBuf<EllCoeffs> d_co_gamma, d_co_delta;
  // per-batch scratch, grown on demand
  size_t cap = 0;
  DeviceBuf<g16_proof> d_raw;
  DeviceBuf<ProofM> d_proofs;
  DeviceBuf<uint32_t> d_flags, d_pub;
  DeviceBuf<G1Affine> d_vkx;
  DeviceBuf<Fq12> d_ml;
  DeviceBuf<uint8_t> d_ok;
  PhaseEvents<3> ev;
  DeviceStream st;                // (device_job.h: after everything its work touches)
  float last_ms[3] = {0, 0, 0};   // vk_x, Miller loops, final exponentiation of the last batch
  std::mutex mu;
  ~g16_verifier() { (void)hipSetDevice(device); }
};

static bool fq_canonical(const uint8_t* p) {
  static const uint32_t kQ[8] = G16_FQ_P;
  uint32_t w[8];
  memcpy(w, p, 32);
  for (int l = 7; l >= 0; l--)
    if (w[l] != kQ[l]) return w[l] < kQ[l];
  return false;
}

static int verifier_create_impl(const uint8_t* vkey, size_t vkey_len, uint32_t n_public, int montgomery, int device,
                                g16_verifier* V) {
  const size_t need = 64 + 3 * 128 + ((size_t)n_public + 1) * 64;
  if (vkey_len != need) {
    set_error("verification key: expected " + std::to_string(need) + " bytes (alpha1 | beta2 | gamma2 | delta2 | IC[0.." +
              std::to_string(n_public) + "]), got " + std::to_string(vkey_len));
    return G16_E_FORMAT;
  }
  if (const int rc = require_hip_device(device, "no HIP device: the verifier has no CPU path", "bad device ordinal")) return rc;
  V->device = device;
  V->n_public = n_public;
  // every coordinate as a Montgomery Fq
  const size_t nfq = vkey_len / 32;
  std::vector<Fq> co(nfq);
  for (size_t k = 0; k < nfq; k++) {
    if (!fq_canonical(vkey + 32 * k)) { set_error("verification key: coordinate not below the field modulus"); return G16_E_FORMAT; }
    Fq x;
    memcpy(x.v, vkey + 32 * k, 32);
    co[k] = montgomery ? x : fp_to_mont(x);
  }
  pairing_consts_init(V->pc);
  const G1Affine alpha{co[0], co[1]};
  const G2Affine beta{Fq2{co[2], co[3]}, Fq2{co[4], co[5]}};
  const G2Affine gamma{Fq2{co[6], co[7]}, Fq2{co[8], co[9]}};
  const G2Affine delta{Fq2{co[10], co[11]}, Fq2{co[12], co[13]}};
  if (aff_is_inf(alpha) || aff_is_inf(beta) || aff_is_inf(gamma) || aff_is_inf(delta) || !g1_on_curve(alpha) ||
      !g2_on_curve(beta, V->pc) || !g2_on_curve(gamma, V->pc) || !g2_on_curve(delta, V->pc)) {
    set_error("verification key: alpha1 / beta2 / gamma2 / delta2 is not a point of its curve");
    return G16_E_FORMAT;
  }
  std::vector<G1Affine> ic(n_public + 1);
  for (uint32_t j = 0; j <= n_public; j++) {
    ic[j] = G1Affine{co[14 + 2 * j], co[15 + 2 * j]};
    if (!aff_is_inf(ic[j]) && !g1_on_curve(ic[j])) { set_error("verification key: IC[" + std::to_string(j) + "] is not on the curve"); return G16_E_FORMAT; }
  }
  std::vector<EllCoeffs> cg(kEllSteps), cd(kEllSteps);
  g2_precompute(gamma, V->pc, cg.data());
  g2_precompute(delta, V->pc, cd.data());
  V->ml_alphabeta = miller_loop(alpha, beta, V->pc);
  G16_HIP(hipSetDevice(device));
  G16_HIP(V->st.create());
  G16_HIP(V->ev.create());
  const size_t tbl_n = (size_t)(n_public + 1) * kIcWin * kIcRow;
  G16_HIP(V->d_ic.alloc(ic.size()));
  G16_HIP(V->d_tbl.alloc(tbl_n));
  G16_HIP(V->d_co_gamma.alloc(kEllSteps));
  G16_HIP(V->d_co_delta.alloc(kEllSteps));
  StreamDrain drain(V->st);   // (ic, cg and cd are host temporaries)
  G16_HIP(hipMemcpyAsync(V->d_ic.p, ic.data(), ic.size() * sizeof(G1Affine), hipMemcpyHostToDevice, V->st));
  G16_HIP(hipMemcpyAsync(V->d_co_gamma.p, cg.data(), kEllSteps * sizeof(EllCoeffs), hipMemcpyHostToDevice, V->st));
  G16_HIP(hipMemcpyAsync(V->d_co_delta.p, cd.data(), kEllSteps * sizeof(EllCoeffs), hipMemcpyHostToDevice, V->st));
  const uint32_t nt = (n_public + 1) * kIcWin;
  verify_ic_table_kernel<<<(nt + 63) / 64, 64, 0, V->st>>>(V->d_ic.p, n_public + 1, V->d_tbl.p);
  G16_HIP(hipGetLastError());
  G16_HIP(hipStreamSynchronize(V->st));
  drain.dismiss();
  return G16_OK;
}

extern "C" int g16_verifier_create(const uint8_t* vkey, size_t vkey_len, uint32_t n_public, int montgomery, int device,
                                   g16_verifier** out) {
  if (!vkey || !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (n_public > (1u << 20)) { set_error("verification key: too many public signals"); return G16_E_ARG; }
  std::unique_ptr<g16_verifier> V(new g16_verifier());
  if (const int rc = verifier_create_impl(vkey, vkey_len, n_public, montgomery, device, V.get())) return rc;
  *out = V.release();
  return G16_OK;
}

static int ensure_scratch(g16_verifier* V, size_t count) {
  if (count <= V->cap) return G16_OK;
  V->cap = 0;
  G16_HIP(V->d_raw.alloc(count));
  G16_HIP(V->d_proofs.alloc(count));
  G16_HIP(V->d_flags.alloc(count));
  G16_HIP(V->d_pub.alloc(count * (size_t)(V->n_public ? V->n_public : 1) * 8));   // (32-byte words)
  G16_HIP(V->d_vkx.alloc(count));
  G16_HIP(V->d_ml.alloc(count * 3));
  G16_HIP(V->d_ok.alloc(count));
  V->cap = count;
  return G16_OK;
}

extern "C" int g16_verify_batch(g16_verifier* V, const g16_proof* proofs, const uint8_t* pubs, size_t count, uint8_t* ok) {
  if (!V || !ok || (count && (!proofs || (V->n_public && !pubs)))) { set_error("NULL argument"); return G16_E_ARG; }
  if (count == 0) return G16_OK;
  if (count > (1u << 24)) { set_error("verify: batch too large"); return G16_E_ARG; }
  std::lock_guard<std::mutex> lk(V->mu);
  G16_HIP(hipSetDevice(V->device));
  int rc = ensure_scratch(V, count);
  if (rc) return rc;
  const uint32_t n = (uint32_t)count;
  hipStream_t st = V->st;
  StreamDrain drain(st);   // (proofs, pubs and ok are the caller's)
  G16_HIP(hipMemcpyAsync(V->d_raw.p, proofs, count * sizeof(g16_proof), hipMemcpyHostToDevice, st));
  if (V->n_public) G16_HIP(hipMemcpyAsync(V->d_pub.p, pubs, count * (size_t)V->n_public * 32, hipMemcpyHostToDevice, st));
  G16_HIP(V->ev.record(0, st));
  verify_load_kernel<<<(n + 63) / 64, 64, 0, st>>>(V->d_raw.p, n, V->pc, V->d_proofs.p, V->d_flags.p);
  verify_vkx_kernel<<<n, 256, 0, st>>>(V->d_ic.p, V->d_tbl.p, V->d_pub.p, V->n_public, V->d_vkx.p);
  G16_HIP(V->ev.record(1, st));
  verify_miller_kernel<<<dim3((n + 63) / 64, 3), 64, 0, st>>>(V->d_proofs.p, V->d_flags.p, V->d_vkx.p, V->d_co_gamma.p,
                                                              V->d_co_delta.p, n, V->pc, V->d_ml.p);
  G16_HIP(V->ev.record(2, st));
  verify_final_kernel<<<(n + 63) / 64, 64, 0, st>>>(V->d_ml.p, V->d_flags.p, n, V->pc, V->ml_alphabeta, V->d_ok.p);
  G16_HIP(V->ev.record(3, st));
  G16_HIP(hipGetLastError());
  G16_HIP(hipMemcpyAsync(ok, V->d_ok.p, count, hipMemcpyDeviceToHost, st));
  G16_HIP(hipStreamSynchronize(st));
  drain.dismiss();
  for (int k = 0; k < 3; k++) V->last_ms[k] = V->ev.ms(k);
  return G16_OK;
}

extern "C" int g16_verifier_timings(const g16_verifier* V, float ms[3]) {
  if (!V || !ms) { set_error("NULL argument"); return G16_E_ARG; }
  for (int k = 0; k < 3; k++) ms[k] = V->last_ms[k];
  return G16_OK;
}

extern "C" void g16_verifier_destroy(g16_verifier* V) { delete V; }

void g16::verifier_info(const g16_verifier* V, int* device, uint32_t* n_public) {
  *device = V->device;
  *n_public = V->n_public;
}

// Layer-test operator (tests/test_gpu_verify.py): count pairs (P in G1, Q in G2) as 6 standard-form 32-byte words
// each -> the 12 standard-form words of the pairing value the verifier kernels compute.
extern "C" int g16_pairing_op(int device, const uint8_t* in, uint32_t count, uint8_t* out) {
  if (!in || !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (const int rc = require_hip_device(device, "no HIP device", "bad device ordinal")) return rc;
  if (count == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  PairingConsts pc;
  pairing_consts_init(pc);
  DeviceJob job("pairing operator");
  DeviceBuf<uint32_t> d_in, d_out;
  if (job.fail(d_in.alloc((size_t)count * 48)) || job.fail(d_out.alloc((size_t)count * 96)) ||
      job.fail(hipMemcpy(d_in.p, in, (size_t)count * 192, hipMemcpyHostToDevice)))
    return job.rc;
  verify_pairing_op_kernel<<<(count + 63) / 64, 64>>>(d_in.p, count, pc, d_out.p);
  if (job.fail(hipGetLastError()) || job.fail(hipMemcpy(out, d_out.p, (size_t)count * 384, hipMemcpyDeviceToHost))) return job.rc;
  return G16_OK;
}
