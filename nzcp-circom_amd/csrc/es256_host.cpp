// The ES256 verifier handle (g16_es256_*), the layer operator g16_p256_op, and the relying party's combined verdict
// g16_nzcp_pass_proof_verify_batch.  The checks of keys and arguments and the host-thread route (device -1: the same
// p256.cuh code the kernels run, on at most 16 threads, no GPU needed) live here; the device route is es256_verify.hip.
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "es256.h"
#include "fixed_base.h"
#include "internal.h"

using namespace g16;

struct g16_es256_verifier {
  int device = -1;
  uint32_t n_keys = 0;
  std::vector<P256Affine> tbl;   // host route: the window tables of G and the keys (the device route keeps its own)
  Es256Device* dev = nullptr;
  float last_ms[2] = {0, 0};
  std::mutex mu;
  ~g16_es256_verifier() { if (dev) es256_device_destroy(dev); }
};

Es256Device* es256_verifier_device(g16_es256_verifier* v) { return v->dev; }

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int create_impl(g16_es256_verifier* V, const uint8_t* keys, uint32_t n_keys, int device) {
  V->device = device;
  V->n_keys = n_keys;
  std::vector<P256Affine> points(n_keys + 1);
  const uint32_t gx[8] = G16_P256_GX, gy[8] = G16_P256_GY;
  for (int k = 0; k < 8; k++) { points[0].x.v[k] = gx[k]; points[0].y.v[k] = gy[k]; }
  for (uint32_t j = 0; j < n_keys; j++) {
    const uint8_t* p = keys + (size_t)j * 64;
    const P256Fp x = pf_load_be<P256FpParams>(p), y = pf_load_be<P256FpParams>(p + 32);
    if (pf_geq_mod(x) || pf_geq_mod(y)) {
      set_error("es256 verifier: key " + std::to_string(j) + ": coordinate not below the field modulus");
      return G16_E_FORMAT;
    }
    if (pf_is_zero(x) && pf_is_zero(y)) {
      set_error("es256 verifier: key " + std::to_string(j) + " is (0, 0), not a point");
      return G16_E_FORMAT;
    }
    points[j + 1] = P256Affine{pf_to_mont(x), pf_to_mont(y)};
    if (!p256_on_curve(points[j + 1])) {
      set_error("es256 verifier: key " + std::to_string(j) + " is not on the curve");
      return G16_E_FORMAT;
    }
  }
  if (device >= 0) return es256_device_create(device, points.data(), n_keys + 1, &V->dev);
  V->tbl.resize(points.size() * kP256TblPoint);
  const size_t rows = points.size() * kP256Win;
  parallel_for(rows, host_threads(rows), [&](size_t lo, size_t hi) {
    for (size_t t = lo; t < hi; t++) p256_table_row(points[t / kP256Win], (uint32_t)(t % kP256Win), &V->tbl[t * kP256Row]);
  });
  return G16_OK;
}

// the host route: the two phases of es256_verify.hip, a signature at a time
void host_batch(g16_es256_verifier* V, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx, size_t count,
                uint8_t* ok) {
  std::vector<P256Fn> u(2 * count);
  std::vector<uint8_t> live(count);
  const int threads = host_threads(count);
  const double t0 = now_ms();
  parallel_for(count, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) live[i] = es256_scalars(hashes + i * 32, sigs + i * 64, u[2 * i], u[2 * i + 1]) ? 1 : 0;
  });
  const double t1 = now_ms();
  parallel_for(count, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      ok[i] = 0;
      if (!live[i]) continue;
      P256Jac slot[kEs256Lanes];
      for (uint32_t l = 0; l < kEs256Lanes; l++)
        es256_slice_sum(slot[l], V->tbl.data(), key_idx ? key_idx[i] : 0u, u[2 * i].v, u[2 * i + 1].v, l, kEs256Lanes);
      es256_tree_sum(slot);
      ok[i] = p256_x_equals_r(slot[0].X, slot[0].Z, pf_load_be<P256FnParams>(sigs + i * 64)) ? 1 : 0;
    }
  });
  V->last_ms[0] = (float)(t1 - t0);
  V->last_ms[1] = (float)(now_ms() - t1);
}

int check_batch_args(const g16_es256_verifier* V, const uint32_t* key_idx, size_t count) {
  if (count > (1u << 24)) { set_error("es256 verify: batch too large"); return G16_E_ARG; }
  if (key_idx)
    for (size_t i = 0; i < count; i++)
      if (key_idx[i] >= V->n_keys) {
        set_error("es256 verify: item " + std::to_string(i) + ": key index " + std::to_string(key_idx[i]) + " of " +
                  std::to_string(V->n_keys) + " keys");
        return G16_E_ARG;
      }
  return G16_OK;
}

}  // namespace

extern "C" int g16_es256_verifier_create(const uint8_t* keys, uint32_t n_keys, int device, g16_es256_verifier** out) {
  if (!keys || !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (n_keys < 1 || n_keys > 16) { set_error("es256 verifier: 1 to 16 keys, got " + std::to_string(n_keys)); return G16_E_ARG; }
  if (device < -1) { set_error("es256 verifier: bad device ordinal"); return G16_E_ARG; }
  return no_bad_alloc("es256 verifier", [&]() {
    g16_es256_verifier* V = new g16_es256_verifier();
    const int rc = create_impl(V, keys, n_keys, device);
    if (rc) { delete V; return rc; }
    *out = V;
    return (int)G16_OK;
  });
}

extern "C" int g16_es256_verify_batch(g16_es256_verifier* V, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx,
                                      size_t count, uint8_t* ok) {
  if (!V || (count && (!hashes || !sigs || !ok))) { set_error("NULL argument"); return G16_E_ARG; }
  if (const int rc = check_batch_args(V, key_idx, count)) return rc;
  if (count == 0) return G16_OK;
  std::lock_guard<std::mutex> lk(V->mu);
  return no_bad_alloc("es256 verify", [&]() {
    if (!V->dev) { host_batch(V, hashes, sigs, key_idx, count, ok); return (int)G16_OK; }
    if (const int rc = es256_device_launch(V->dev, hashes, sigs, key_idx, count)) return rc;
    return es256_device_finish(V->dev, ok, V->last_ms);
  });
}

extern "C" int g16_es256_verifier_timings(const g16_es256_verifier* V, float ms[2]) {
  if (!V || !ms) { set_error("NULL argument"); return G16_E_ARG; }
  ms[0] = V->last_ms[0];
  ms[1] = V->last_ms[1];
  return G16_OK;
}

extern "C" void g16_es256_verifier_destroy(g16_es256_verifier* V) { delete V; }

extern "C" int g16_p256_op(int device, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) {
  if (op < 0 || op >= kP256OpCount) { set_error("p256 operator: unknown op " + std::to_string(op)); return G16_E_ARG; }
  size_t sa, sb, so;
  p256_op_strides(op, &sa, &sb, &so);
  if (!a || !out || (sb && !b)) { set_error("NULL argument"); return G16_E_ARG; }
  if (device < -1) { set_error("p256 operator: bad device ordinal"); return G16_E_ARG; }
  if (n > (1u << 24)) { set_error("p256 operator: too many items"); return G16_E_ARG; }
  // every value below its modulus: the scalar field for its ops and for r of the comparison, the base field otherwise
  const bool fn_a = op >= kP256FnAdd && op <= kP256FnInv, fn_b = fn_a || op == kP256XCmp;
  for (size_t i = 0; i < n; i++) {
    bool bad = false;
    for (size_t k = 0; k < sa; k += 32)
      bad |= fn_a ? pf_geq_mod(pf_load_be<P256FnParams>(a + i * sa + k)) : pf_geq_mod(pf_load_be<P256FpParams>(a + i * sa + k));
    for (size_t k = 0; k < sb; k += 32)
      bad |= fn_b ? pf_geq_mod(pf_load_be<P256FnParams>(b + i * sb + k)) : pf_geq_mod(pf_load_be<P256FpParams>(b + i * sb + k));
    if (bad) { set_error("p256 operator: item " + std::to_string(i) + ": a value is not below its modulus"); return G16_E_ARG; }
  }
  if (n == 0) return G16_OK;
  if (device >= 0) return es256_device_op(device, op, a, b, out, n);
  parallel_for(n, host_threads(n), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) p256_op_one(op, a + i * sa, b + i * sb, out + i * so);
  });
  return G16_OK;
}

// ---------------------------------------------------------------- proof + pass signature
// NZCPPubIdentity's public.json: signals 0..255 credSubjSha256, 256..511 toBeSignedSha256 (bits, MSB first), 512 exp
static constexpr uint32_t kNzcpPublic = 513;

extern "C" int g16_nzcp_pass_proof_verify_batch(g16_verifier* v, g16_es256_verifier* e, const g16_proof* proofs, const uint8_t* pubs,
                                                const uint8_t* sigs, const uint32_t* key_idx, uint64_t now, size_t count,
                                                uint8_t* verdict) {
  if (!v || !e || (count && (!proofs || !pubs || !sigs || !verdict))) { set_error("NULL argument"); return G16_E_ARG; }
  int vdev = 0;
  uint32_t n_public = 0;
  verifier_info(v, &vdev, &n_public);
  if (n_public != kNzcpPublic) {
    set_error("nzcp pass proof: the verification key has " + std::to_string(n_public) + " public signals, NZCPPubIdentity has 513");
    return G16_E_ARG;
  }
  if (e->device != vdev) {
    set_error("nzcp pass proof: the proof verifier is on device " + std::to_string(vdev) + ", the signature verifier on " +
              (e->device < 0 ? std::string("the host route") : "device " + std::to_string(e->device)));
    return G16_E_ARG;
  }
  if (const int rc = check_batch_args(e, key_idx, count)) return rc;
  if (count == 0) return G16_OK;
  std::lock_guard<std::mutex> lk(e->mu);
  return no_bad_alloc("nzcp pass proof", [&]() {
    // The digest a signature is checked against comes from the proof's own public signals: that is the binding.  The
    // packing is a scan of 16 KB per proof on the host, next to the upload the Groth16 path makes of the same bytes.
    std::vector<uint8_t> digest(count * 32, 0), bits_ok(count), expired(count), sig_ok(count), proof_ok(count);
    parallel_for(count, host_threads(count), [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        const uint8_t* p = pubs + i * (size_t)kNzcpPublic * 32;
        bool good = true;
        for (uint32_t j = 0; j < 512; j++) {
          const uint8_t* w = p + (size_t)j * 32;
          uint8_t rest = 0;
          for (int k = 1; k < 32; k++) rest |= w[k];
          good = good && rest == 0 && w[0] <= 1;
          if (j >= 256 && (w[0] & 1)) digest[i * 32 + ((j - 256) >> 3)] |= (uint8_t)(0x80u >> ((j - 256) & 7));
        }
        bits_ok[i] = good ? 1 : 0;
        const uint8_t* x = p + (size_t)512 * 32;   // exp: a 256-bit little-endian integer
        uint64_t lo64 = 0;
        uint8_t high = 0;
        for (int k = 0; k < 8; k++) lo64 |= (uint64_t)x[k] << (8 * k);
        for (int k = 8; k < 32; k++) high |= x[k];
        expired[i] = now != 0 && !high && lo64 <= now ? 1 : 0;
      }
    });
    // the signatures on their own stream, under the Groth16 batch's Miller loops
    if (const int rc = es256_device_launch(e->dev, digest.data(), sigs, key_idx, count)) return rc;
    const int rc_proofs = g16_verify_batch(v, proofs, pubs, count, proof_ok.data());
    const int rc_sigs = es256_device_finish(e->dev, sig_ok.data(), e->last_ms);
    if (rc_proofs) return rc_proofs;
    if (rc_sigs) return rc_sigs;
    for (size_t i = 0; i < count; i++)
      verdict[i] = !proof_ok[i] ? 1 : !bits_ok[i] ? 2 : !sig_ok[i] ? 3 : expired[i] ? 4 : 0;
    return (int)G16_OK;
  });
}
