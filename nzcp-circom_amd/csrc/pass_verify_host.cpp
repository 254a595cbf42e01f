// The pass verifier handle (g16_pass_*) and the layer operator g16_pass_op.  The argument checks, the host-thread route
// (device -1: the same nzcp_pass.cuh code the kernel runs, on at most 16 threads, no GPU needed) and the merge of the
// signatures' verdicts with nbf / exp live here; the device route is pass_verify.hip.
#include <string.h>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fixed_base.h"
#include "internal.h"
#include "pass_verify.h"

using namespace g16;

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int take_name(const char* s, const char* what, uint32_t j, uint8_t* out, uint32_t* len) {
  const size_t n = s ? strnlen(s, kPassNameMax + 1) : 0;
  if (n < 1 || n > kPassNameMax) {
    set_error("pass verifier: key " + std::to_string(j) + ": " + what + " must be 1 to " + std::to_string(kPassNameMax) + " bytes");
    return G16_E_ARG;
  }
  memcpy(out, s, n);
  *len = (uint32_t)n;
  return G16_OK;
}

}  // namespace

// offsets ascend; a batch is at most 2^24 passes and its text below 2^32 bytes
int g16::pass_check_items(const char* route, const uint8_t* text, const uint64_t* offsets, size_t count) {
  if (count > (1u << 24)) { set_error(std::string(route) + ": batch too large"); return G16_E_ARG; }
  if (count == 0) return G16_OK;
  if (!text || !offsets) { set_error("NULL argument"); return G16_E_ARG; }
  for (size_t i = 0; i < count; i++)
    if (offsets[i + 1] < offsets[i]) {
      set_error(std::string(route) + ": item " + std::to_string(i) + ": offsets do not ascend");
      return G16_E_ARG;
    }
  if (offsets[count] - offsets[0] >= (1ull << 32)) { set_error(std::string(route) + ": more than 4 GiB of text"); return G16_E_ARG; }
  return G16_OK;
}

namespace {

// the host route's front end: a pass at a time, a thread's own decode buffer and stack
void host_front(const PassKeyName* keys, uint32_t n_keys, const uint8_t* text, const uint64_t* offsets, size_t count,
                g16_pass_result* records, uint8_t* sigs) {
  parallel_for(count, host_threads(count), [&](size_t lo, size_t hi) {
    uint8_t dec[kPassDecodedMax];
    uint32_t stack[kPassCborDepth];
    for (size_t i = lo; i < hi; i++)
      pass_uri_one(text + offsets[i], offsets[i + 1] - offsets[i], keys, n_keys, dec, stack, &records[i], sigs + i * 64);
  });
}

}  // namespace

extern "C" int g16_pass_verifier_create(const uint8_t* keys, const char* const* iss, const char* const* kid, uint32_t n_keys,
                                        int device, g16_pass_verifier** out) {
  if (!keys || !iss || !kid || !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (n_keys < 1 || n_keys > 16) { set_error("pass verifier: 1 to 16 keys, got " + std::to_string(n_keys)); return G16_E_ARG; }
  if (device < -1) { set_error("pass verifier: bad device ordinal"); return G16_E_ARG; }
  return no_bad_alloc("pass verifier", [&]() {
    g16_pass_verifier* V = new g16_pass_verifier();
    V->device = device;
    V->names.resize(n_keys);
    int rc = G16_OK;
    for (uint32_t j = 0; j < n_keys && !rc; j++) {
      memset(&V->names[j], 0, sizeof(PassKeyName));
      rc = take_name(iss[j], "iss", j, V->names[j].iss, &V->names[j].iss_len);
      if (!rc) rc = take_name(kid[j], "kid", j, V->names[j].kid, &V->names[j].kid_len);
    }
    if (!rc) rc = g16_es256_verifier_create(keys, n_keys, device, &V->es);
    if (!rc && device >= 0) rc = pass_device_create(device, V->names.data(), n_keys, &V->dev);
    if (rc) { delete V; return rc; }
    *out = V;
    return (int)G16_OK;
  });
}

extern "C" int g16_pass_verify_batch(g16_pass_verifier* V, const uint8_t* text, const uint64_t* offsets, size_t count, int64_t now,
                                     g16_pass_result* out) {
  if (!V || (count && !out)) { set_error("NULL argument"); return G16_E_ARG; }
  if (const int rc = pass_check_items("pass verify", text, offsets, count)) return rc;
  if (count == 0) return G16_OK;
  std::lock_guard<std::mutex> lk(V->mu);
  return no_bad_alloc("pass verify", [&]() {
    std::vector<uint8_t> ok(count);
    if (V->dev) {
      if (const int rc = pass_device_batch(V->dev, es256_verifier_device(V->es), text, offsets, count, out, ok.data(), V->last_ms))
        return rc;
    } else {
      std::vector<uint8_t> hashes(count * 32), sigs(count * 64);
      std::vector<uint32_t> key_idx(count);
      const double t0 = now_ms();
      host_front(V->names.data(), (uint32_t)V->names.size(), text, offsets, count, out, sigs.data());
      for (size_t i = 0; i < count; i++) {
        memcpy(&hashes[i * 32], out[i].tbs_sha256, 32);
        key_idx[i] = out[i].key_idx;
      }
      V->last_ms[0] = (float)(now_ms() - t0);
      if (const int rc = g16_es256_verify_batch(V->es, hashes.data(), sigs.data(), key_idx.data(), count, ok.data())) return rc;
      (void)g16_es256_verifier_timings(V->es, V->last_ms + 1);
    }
    for (size_t i = 0; i < count; i++) out[i].verdict = pass_merge(out[i].verdict, ok[i] != 0, out[i].nbf, out[i].exp, now);
    return (int)G16_OK;
  });
}

extern "C" int g16_pass_verifier_timings(const g16_pass_verifier* V, float ms[3]) {
  if (!V || !ms) { set_error("NULL argument"); return G16_E_ARG; }
  for (int k = 0; k < 3; k++) ms[k] = V->last_ms[k];
  return G16_OK;
}

extern "C" void g16_pass_verifier_destroy(g16_pass_verifier* V) { delete V; }

extern "C" int g16_pass_op(int device, int op, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* out) {
  if (op < 0 || op >= kPassOpCount) { set_error("pass operator: unknown op " + std::to_string(op)); return G16_E_ARG; }
  if (device < -1) { set_error("pass operator: bad device ordinal"); return G16_E_ARG; }
  if (count && !out) { set_error("NULL argument"); return G16_E_ARG; }
  if (const int rc = pass_check_items("pass operator", text, offsets, count)) return rc;
  if (count == 0) return G16_OK;
  if (device >= 0) return pass_device_op(device, op, text, offsets, count, out);
  return no_bad_alloc("pass operator", [&]() {
    const size_t stride = pass_op_stride(op);
    if (op == kPassOpFront) {
      std::vector<uint8_t> sigs(count * 64);
      std::vector<g16_pass_result> records(count);
      host_front(nullptr, 0, text, offsets, count, records.data(), sigs.data());
      memcpy(out, records.data(), count * stride);
      return (int)G16_OK;
    }
    memset(out, 0, count * stride);
    parallel_for(count, host_threads(count), [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        const uint8_t* item = text + offsets[i];
        const uint64_t n = offsets[i + 1] - offsets[i];
        if (op == kPassOpBase32) pass_op_base32_one(item, n, out + i * stride);
        else pass_op_sha256_one(item, n, out + i * stride);
      }
    });
    return (int)G16_OK;
  });
}
