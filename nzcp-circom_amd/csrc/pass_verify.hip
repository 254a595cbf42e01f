// The front end of NZCP pass verification on the device (nzcp_pass.cuh: text, base32, the COSE_Sign1 / CWT walk, the two
// SHA-256 digests, the key lookup), writing straight into the ES256 handle's scratch so that nothing returns to the
// host between the parse and the signature kernels.
//
// Device schedule, per workgroup of 64 lanes = kPassPerBlock passes:
//   frame    a lane per pass: length cap, trim, "NZCP:/1/", the trailing '=' (text read from global memory, a few
//            bytes at each end of a pass)
//   decode   all 64 lanes per pass in turn: lane l takes the 8-character groups l, l + 64, ... (consecutive lanes read
//            consecutive 8-byte runs of the text) and writes 5 bytes each into the pass's LDS slice
//   walk     a lane per pass over its own slice: a dependent load per byte costs an LDS access, not a trip to memory;
//            the skip stack is in LDS too, the SHA-256 schedule in registers; the record, the digest, r | s and the
//            key index go out with plain vector stores
// A slice is 1284 bytes: 1280 decoded bytes at most, and an odd count of words, so that lanes at the same place in
// their passes -- the common case, passes of one issuer look alike -- read different banks.  32 slices + 32 stacks =
// 43 KB of the CU's 160 KB: LDS admits 3 workgroups a CU.
// A pass whose verdict is decided gets a zero signature: the range check of es256_scalars_kernel retires its lanes.
#include <hip/hip_runtime.h>

#include <memory>

#include "internal.h"
#include "pass_verify.h"

namespace g16 {
namespace {

constexpr uint32_t kBlock = 64;
constexpr uint32_t kPassPerBlock = 32;
constexpr uint32_t kSlice = kPassDecodedMax + 4;
static_assert((kSlice / 4) % 2 == 1 && kSlice % 4 == 0, "a slice is an odd count of words");

constexpr uint32_t kStateNone = 0xffu;   // a slot past the batch

// records[i] always; hashes / sigs / key_idx (the ES256 scratch) when not NULL
__global__ __launch_bounds__(64) void pass_front_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offsets,
                                                        uint32_t count, const PassKeyName* __restrict__ keys, uint32_t n_keys,
                                                        g16_pass_result* __restrict__ records, uint8_t* __restrict__ hashes,
                                                        uint8_t* __restrict__ sigs, uint32_t* __restrict__ key_idx) {
  __shared__ uint8_t s_dec[kPassPerBlock][kSlice];
  __shared__ uint32_t s_stack[kPassPerBlock][kPassCborDepth];
  __shared__ uint64_t s_chars_at[kPassPerBlock];   // where a pass's base32 characters start in text
  __shared__ uint32_t s_chars[kPassPerBlock], s_state[kPassPerBlock];
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * kPassPerBlock + tid;
  const bool mine = tid < kPassPerBlock && i < count;
  const uint64_t base = offsets[0];   // text holds the bytes from offsets[0] on
  if (tid < kPassPerBlock) {
    uint32_t state = kStateNone, start = 0, n_chars = 0;
    uint64_t at = 0;
    if (mine) {
      at = offsets[i] - base;
      state = pass_uri_frame(text + at, offsets[i + 1] - offsets[i], &start, &n_chars);
    }
    s_state[tid] = state;
    s_chars_at[tid] = at + start;
    s_chars[tid] = n_chars;
  }
  __syncthreads();
  for (uint32_t p = 0; p < kPassPerBlock; p++) {
    if (s_state[p] != G16_PASS_OK) continue;   // (uniform: every lane reads the same word)
    const uint32_t n_chars = s_chars[p], n_out = pass_b32_bytes(n_chars);
    const uint8_t* chars = text + s_chars_at[p];
    bool good = true;
    for (uint32_t g = tid; g < (n_chars + 7) / 8; g += kBlock) good = pass_b32_group(chars, n_chars, g, s_dec[p], n_out) && good;
    if (!good) s_state[p] = G16_PASS_MALFORMED;   // (lanes that store, store the same value)
  }
  __syncthreads();
  if (!mine) return;
  g16_pass_result* r = &records[i];
  uint32_t sig_off = 0;
  const PassBuf b{s_dec[tid], pass_b32_bytes(s_chars[tid])};
  if (s_state[tid] == G16_PASS_OK) pass_front(b, keys, n_keys, s_stack[tid], r, &sig_off);
  else pass_result_clear(r, s_state[tid]);
  if (!hashes) return;
  const bool live = r->verdict == G16_PASS_OK;
  uint32_t* h = (uint32_t*)(hashes + (size_t)i * 32);
  const uint32_t* d = (const uint32_t*)r->tbs_sha256;
  for (int k = 0; k < 8; k++) h[k] = d[k];
  uint8_t* s = sigs + (size_t)i * 64;
  for (uint32_t k = 0; k < 64; k++) s[k] = live ? (uint8_t)pass_at(b, sig_off + k) : 0;
  key_idx[i] = live ? r->key_idx : 0u;
}

// ops 0 and 1 of the layer operator: a lane per item, on global memory
__global__ __launch_bounds__(64) void pass_op_kernel(int op, const uint8_t* __restrict__ text, const uint64_t* __restrict__ offsets,
                                                     uint32_t count, uint8_t* __restrict__ out, uint32_t stride) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint8_t* item = text + (offsets[i] - offsets[0]);
  const uint64_t n = offsets[i + 1] - offsets[i];
  if (op == kPassOpBase32) pass_op_base32_one(item, n, out + (size_t)i * stride);
  else pass_op_sha256_one(item, n, out + (size_t)i * stride);
}

}  // namespace

// (device_job.h) No stream of its own: a batch runs on the ES256 handle's, and pass_device_batch leaves on no path
// before that stream has passed the batch, so nothing is at work on these members between calls
struct PassDevice {
  int device = 0;
  uint32_t n_keys = 0;
  DeviceBuf<PassKeyName> d_keys;
  // per-batch scratch, grown on demand
  size_t cap = 0, text_cap = 0;
  DeviceBuf<uint64_t> d_offsets;
  DeviceBuf<g16_pass_result> d_records;
  DeviceBuf<uint8_t> d_text;
  PhaseEvents<1> ev;
  ~PassDevice() { (void)hipSetDevice(device); }
};

int pass_device_create(int device, const PassKeyName* names, uint32_t n_keys, PassDevice** out) {
  if (const int rc = require_hip_device(device, "pass verifier: no HIP device (device -1 selects the host route)",
                                        "pass verifier: bad device ordinal"))
    return rc;
  std::unique_ptr<PassDevice> D(new PassDevice());
  D->device = device;
  D->n_keys = n_keys;
  G16_HIP(hipSetDevice(device));
  G16_HIP(D->ev.create());
  G16_HIP(D->d_keys.alloc(n_keys));
  G16_HIP(hipMemcpy(D->d_keys.p, names, (size_t)n_keys * sizeof(PassKeyName), hipMemcpyHostToDevice));
  *out = D.release();
  return G16_OK;
}

void pass_device_destroy(PassDevice* D) { delete D; }

void pass_device_uploaded(const PassDevice* D, const uint8_t** d_text, const uint64_t** d_offsets) {
  *d_text = D->d_text.p;
  *d_offsets = D->d_offsets.p;
}
int pass_device_id(const PassDevice* D) { return D->device; }

static int ensure_scratch(PassDevice* D, size_t count, size_t text_bytes) {
  if (count > D->cap) {
    D->cap = 0;
    G16_HIP(D->d_offsets.alloc(count + 1));
    G16_HIP(D->d_records.alloc(count));
    D->cap = count;
  }
  if (text_bytes > D->text_cap) {
    D->text_cap = 0;
    G16_HIP(D->d_text.alloc(text_bytes));
    D->text_cap = text_bytes;
  }
  return G16_OK;
}

// the front end, then the signature kernels, on the ES256 handle's stream (enqueue only)
static int pass_enqueue(PassDevice* D, Es256Device* es, const Es256Scratch& sc, const uint8_t* text, const uint64_t* offsets,
                        size_t count, g16_pass_result* records) {
  hipStream_t st = (hipStream_t)sc.stream;
  const uint32_t n = (uint32_t)count;
  const size_t text_bytes = (size_t)(offsets[count] - offsets[0]);
  G16_HIP(hipMemcpyAsync(D->d_offsets.p, offsets, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (text_bytes) G16_HIP(hipMemcpyAsync(D->d_text.p, text + offsets[0], text_bytes, hipMemcpyHostToDevice, st));
  G16_HIP(D->ev.record(0, st));
  pass_front_kernel<<<(n + kPassPerBlock - 1) / kPassPerBlock, kBlock, 0, st>>>(D->d_text.p, D->d_offsets.p, n, D->d_keys.p, D->n_keys,
                                                                                D->d_records.p, sc.hashes, sc.sigs, sc.key_idx);
  G16_HIP(D->ev.record(1, st));
  G16_HIP(hipGetLastError());
  if (const int rc = es256_device_launch_resident(es, count)) return rc;
  G16_HIP(hipMemcpyAsync(records, D->d_records.p, count * sizeof(g16_pass_result), hipMemcpyDeviceToHost, st));
  return G16_OK;
}

int pass_device_batch(PassDevice* D, Es256Device* es, const uint8_t* text, const uint64_t* offsets, size_t count,
                      g16_pass_result* records, uint8_t* ok, float ms[3]) {
  G16_HIP(hipSetDevice(D->device));
  const size_t text_bytes = (size_t)(offsets[count] - offsets[0]);
  if (const int rc = ensure_scratch(D, count, text_bytes ? text_bytes : 1)) return rc;
  Es256Scratch sc;
  if (const int rc = es256_device_scratch(es, count, &sc)) return rc;
  if (const int rc = pass_enqueue(D, es, sc, text, offsets, count, records)) {
    es256_device_abandon(es);   // (text, offsets and records are the caller's; the scratch is the ES256 handle's)
    return rc;
  }
  if (const int rc = es256_device_finish(es, ok, ms + 1)) return rc;   // (waits for the stream, also when it fails)
  ms[0] = D->ev.ms(0);
  return G16_OK;
}

int pass_device_op(int device, int op, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* out) {
  if (const int rc = require_hip_device(device, "pass operator: no HIP device (device -1 selects the host route)",
                                        "pass operator: bad device ordinal"))
    return rc;
  G16_HIP(hipSetDevice(device));
  const size_t stride = pass_op_stride(op), text_bytes = (size_t)(offsets[count] - offsets[0]);
  const uint32_t n = (uint32_t)count;
  DeviceJob job("pass operator");
  DeviceBuf<uint8_t> d_text, d_out;
  DeviceBuf<uint64_t> d_offsets;
  if (job.fail(d_text.alloc(text_bytes ? text_bytes : 1)) || job.fail(d_offsets.alloc(count + 1)) || job.fail(d_out.alloc(count * stride)) ||
      job.fail(hipMemset(d_out.p, 0, count * stride)) ||
      (text_bytes && job.fail(hipMemcpy(d_text.p, text + offsets[0], text_bytes, hipMemcpyHostToDevice))) ||
      job.fail(hipMemcpy(d_offsets.p, offsets, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice)))
    return job.rc;
  if (op == kPassOpFront)
    pass_front_kernel<<<(n + kPassPerBlock - 1) / kPassPerBlock, kBlock>>>(d_text.p, d_offsets.p, n, nullptr, 0,
                                                                           (g16_pass_result*)d_out.p, nullptr, nullptr, nullptr);
  else
    pass_op_kernel<<<(n + kBlock - 1) / kBlock, kBlock>>>(op, d_text.p, d_offsets.p, n, d_out.p, (uint32_t)stride);
  if (job.fail(hipGetLastError()) || job.fail(hipMemcpy(out, d_out.p, count * stride, hipMemcpyDeviceToHost))) return job.rc;
  return G16_OK;
}

}  // namespace g16
