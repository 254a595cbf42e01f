// Between es256_host.cpp (the handle, the checks, the host-thread route, the C ABI) and es256_verify.hip (the device
// route): the device side of an ES256 verifier, and the one-item core of the layer operator g16_p256_op that both routes run.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "p256.cuh"

namespace g16 {

// lanes that share one signature's 128 table entries ("ES256"): the device gives each group of kEs256Lanes
// lanes of a wavefront one signature and adds their sums in a shuffle tree; the host route adds the same slices in the
// same order
constexpr uint32_t kEs256Lanes = 16;

// sum of the kEs256Lanes slice sums in the order of the device's tree: step s = 8, 4, 2, 1 adds slot l + s into slot l
inline void es256_tree_sum(P256Jac* slot) {
  for (uint32_t s = kEs256Lanes / 2; s >= 1; s >>= 1)
    for (uint32_t l = 0; l < s; l++) p256_add(slot[l], slot[l + s]);
}

// ---------------------------------------------------------------- layer operator
enum P256Op {
  kP256FpAdd = 0, kP256FpSub = 1, kP256FpMul = 2,   // base field: a, b, out 32 bytes
  kP256FnAdd = 3, kP256FnSub = 4, kP256FnMul = 5,   // scalar field
  kP256FnInv = 6, kP256FpInv = 7,                   // a, out 32 bytes (b unused); inverse of 0 is 0
  kP256MAdd = 8,                                    // affine a + affine b by the mixed addition: 64, 64, 64 bytes
  kP256Add = 9,                                     // the same sum by the full addition, both operands with Z != 1
  kP256XCmp = 10,                                   // a = X | Z (64), b = r (32) -> 1 byte: x(X : Z) mod n == r
  kP256OpCount = 11
};
inline void p256_op_strides(int op, size_t* sa, size_t* sb, size_t* so) {
  const bool point = op == kP256MAdd || op == kP256Add, un = op == kP256FnInv || op == kP256FpInv;
  *sa = point || op == kP256XCmp ? 64 : 32;
  *sb = un ? 0 : point ? 64 : 32;
  *so = op == kP256XCmp ? 1 : point ? 64 : 32;
}

template <class PM> G16_P256_FN void p256_field_op_one(int k, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  const PF<PM> x = pf_load_be<PM>(a);
  if (k == 3) { pf_store_be(out, pf_from_mont(pf_inv(pf_to_mont(x)))); return; }
  const PF<PM> y = pf_load_be<PM>(b);
  pf_store_be(out, k == 0 ? pf_add(x, y) : k == 1 ? pf_sub(x, y) : pf_mul(pf_to_mont(x), y));
}
G16_P256_FN P256Affine p256_load_affine_be(const uint8_t* p) {   // standard big-endian x | y -> Montgomery
  return P256Affine{pf_to_mont(pf_load_be<P256FpParams>(p)), pf_to_mont(pf_load_be<P256FpParams>(p + 32))};
}
// (x, y) -> (x l^2, y l^3, l): the same point with Z = l
G16_P256_FN void p256_rescale(P256Jac& r, const P256Affine& a, uint32_t l) {
  p256_from_affine(r, a);
  if (p256_is_inf(r)) return;
  P256Fp z = pf_zero<P256FpParams>();
  z.v[0] = l;
  z = pf_to_mont(z);
  const P256Fp zz = pf_sqr(z);
  r.X = pf_mul(r.X, zz);
  r.Y = pf_mul(r.Y, pf_mul(z, zz));
  r.Z = z;
}
// one item; every field value is below its modulus (the caller checked)
G16_P256_FN void p256_op_one(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  if (op <= kP256FpMul) { p256_field_op_one<P256FpParams>(op, a, b, out); return; }
  if (op <= kP256FnMul) { p256_field_op_one<P256FnParams>(op - 3, a, b, out); return; }
  if (op == kP256FnInv) { p256_field_op_one<P256FnParams>(3, a, b, out); return; }
  if (op == kP256FpInv) { p256_field_op_one<P256FpParams>(3, a, b, out); return; }
  if (op == kP256XCmp) {
    const P256Fp X = pf_to_mont(pf_load_be<P256FpParams>(a)), Z = pf_to_mont(pf_load_be<P256FpParams>(a + 32));
    out[0] = p256_x_equals_r(X, Z, pf_load_be<P256FnParams>(b)) ? 1 : 0;
    return;
  }
  const P256Affine pa = p256_load_affine_be(a), pb = p256_load_affine_be(b);
  P256Jac acc;
  if (op == kP256MAdd) {
    p256_from_affine(acc, pa);
    p256_madd(acc, pb);
  } else {
    P256Jac other;
    p256_rescale(acc, pa, 3);
    p256_rescale(other, pb, 5);
    p256_add(acc, other);
  }
  P256Affine r;
  p256_to_affine(r, acc);
  pf_store_be(out, pf_from_mont(r.x));
  pf_store_be(out + 32, pf_from_mont(r.y));
}

// ---------------------------------------------------------------- the device route (es256_verify.hip)
struct Es256Device;   // resident tables, a stream of its own, per-batch scratch
// points: G then the keys (Montgomery affine, on the curve); builds the window tables on `device`
int es256_device_create(int device, const P256Affine* points, uint32_t n_points, Es256Device** out);
void es256_device_destroy(Es256Device* d);
// enqueue one batch on the handle's stream and return; the host buffers stay alive until the finish.  key_idx may be
// NULL (key 0), its entries are below the key count
int es256_device_launch(Es256Device* d, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx, size_t count);
// wait for it: ok[count], ms = device time of the two phases
int es256_device_finish(Es256Device* d, uint8_t* ok, float ms[2]);
int es256_device_op(int device, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
// For a front end that fills the inputs on the device (pass_verify.hip): the handle's scratch for `count` signatures
// (grown on demand) and its stream (a hipStream_t); then the two kernels over what lies there.  es256_device_finish
// ends such a batch as it ends any other.
struct Es256Scratch {
  uint8_t* hashes;     // count x 32
  uint8_t* sigs;       // count x 64
  uint32_t* key_idx;   // count
  void* stream;
};
int es256_device_scratch(Es256Device* d, size_t count, Es256Scratch* out);
int es256_device_launch_resident(Es256Device* d, size_t count);
// ... and when such a batch fails before its finish: wait for the handle's stream, nothing stays in flight
void es256_device_abandon(Es256Device* d);

}  // namespace g16

// of an ES256 verifier handle (es256_host.cpp): its device side, NULL on the host route
struct g16_es256_verifier;
g16::Es256Device* es256_verifier_device(g16_es256_verifier* v);
