// Between pass_verify_host.cpp (the handle, the checks, the host-thread route, the C ABI) and pass_verify.hip (the device
// route): the device side of a pass verifier, and the one-item cores of the layer operator g16_pass_op that both routes
// and tests/native/pass_test.cpp run.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include <vector>

#include "es256.h"
#include "nzcp_pass.cuh"

namespace g16 {

enum PassOp { kPassOpBase32 = 0, kPassOpSha256 = 1, kPassOpFront = 2, kPassOpCount = 3 };
inline size_t pass_op_stride(int op) {
  return op == kPassOpBase32 ? kPassB32Stride : op == kPassOpSha256 ? 32 : sizeof(g16_pass_result);
}

// op 0: out = u32 length (little-endian; kPassB32Invalid: not base32, or too long) then the bytes
G16_HD void pass_op_base32_one(const uint8_t* item, uint64_t n, uint8_t* out) {
  uint32_t len = kPassB32Invalid;
  if (n <= kPassUriMax) {
    const uint32_t body = pass_b32_body(item, (uint32_t)n), bytes = pass_b32_bytes(body);
    if (pass_b32_decode(item, body, out + 4, bytes)) len = bytes;
  }
  for (int k = 0; k < 4; k++) out[k] = (uint8_t)(len >> (8 * k));
}
// op 1
G16_HD void pass_op_sha256_one(const uint8_t* item, uint64_t n, uint8_t* out) {
  sha256_stream(PassBytesSource{item}, (uint32_t)n, out);
}
// Rules 1 and 2 of one pass on text[0, n): verdict 0 with the frame of its base32 characters, else the record's verdict
G16_HD uint32_t pass_uri_frame(const uint8_t* text, uint64_t n, uint32_t* start, uint32_t* n_chars) {
  if (n > kPassUriMax) return G16_PASS_TOO_LONG;
  return pass_text_frame(text, (uint32_t)n, start, n_chars) ? G16_PASS_OK : G16_PASS_MALFORMED;
}
// The whole front end of one pass, a lane or a thread on its own: dec = room for pass_b32_bytes(n_chars) bytes (at most
// kPassDecodedMax), stack = kPassCborDepth words.  sig = the 64 signature bytes, zero unless the verdict is 0: a zero
// signature fails the ES256 range check, which retires the pass there.
G16_HD void pass_uri_one(const uint8_t* text, uint64_t n, const PassKeyName* keys, uint32_t n_keys, uint8_t* dec, uint32_t* stack,
                         g16_pass_result* r, uint8_t* sig) {
  for (int k = 0; k < 64; k++) sig[k] = 0;
  uint32_t start = 0, n_chars = 0, sig_off = 0;
  const uint32_t v = pass_uri_frame(text, n, &start, &n_chars);
  if (v != G16_PASS_OK) { pass_result_clear(r, v); return; }
  const uint32_t bytes = pass_b32_bytes(n_chars);
  if (!pass_b32_decode(text + start, n_chars, dec, bytes)) { pass_result_clear(r, G16_PASS_MALFORMED); return; }
  const PassBuf b{dec, bytes};
  pass_front(b, keys, n_keys, stack, r, &sig_off);
  if (r->verdict == G16_PASS_OK)
    for (uint32_t k = 0; k < 64; k++) sig[k] = (uint8_t)pass_at(b, sig_off + k);
}

// ---------------------------------------------------------------- the device route (pass_verify.hip)
struct PassDevice;   // the key names, resident; per-batch scratch for text, offsets and records
int pass_device_create(int device, const PassKeyName* names, uint32_t n_keys, PassDevice** out);
void pass_device_destroy(PassDevice* d);
// One batch: the front-end kernel on es's stream writes into es's scratch, the two ES256 kernels follow, then the wait.
// records[count] with verdict 0 / 1 / 2 / 3 / 7, ok[count] the signatures' verdicts, ms = device time of the three phases
int pass_device_batch(PassDevice* d, Es256Device* es, const uint8_t* text, const uint64_t* offsets, size_t count,
                      g16_pass_result* records, uint8_t* ok, float ms[3]);
int pass_device_op(int device, int op, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* out);
// where the last batch's text and offsets lie on the device (until the next batch), for a kernel that reads them again
void pass_device_uploaded(const PassDevice* d, const uint8_t** d_text, const uint64_t** d_offsets);
int pass_device_id(const PassDevice* d);

// the checks of a batch of items, "<route>: ..." (G16_E_ARG)
int pass_check_items(const char* route, const uint8_t* text, const uint64_t* offsets, size_t count);

}  // namespace g16

// the handle of the C ABI (pass_verify_host.cpp; the pass prover in pass_prove_host.cpp reads it)
struct g16_pass_verifier {
  int device = -1;
  g16_es256_verifier* es = nullptr;   // owned: the tables of G and the keys, and on a device the scratch the front end fills
  std::vector<g16::PassKeyName> names;
  g16::PassDevice* dev = nullptr;
  float last_ms[3] = {0, 0, 0};
  std::mutex mu;
  ~g16_pass_verifier() {
    if (dev) pass_device_destroy(dev);
    if (es) g16_es256_verifier_destroy(es);
  }
};
