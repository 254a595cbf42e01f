// The holder's side of a pass on the device: pass URI text -> the input words of NZCPPubIdentity's witness, toBeSigned[8 M]
// (a bit a word, MSB first per byte, zero beyond the length) and toBeSignedLen, written where the witness calculator
// reads them (wtns_calc.hip's d_in), so that of a pass only its text crosses the bus -- under 2 KB instead of the
// (8 M + 1) x 32 bytes of its words.
//
// Device schedule, ONE workgroup of 256 lanes per selected pass (the host has run the front end and names the passes of
// this chunk in sel):
//   frame    lane 0: length cap, trim, "NZCP:/1/", the trailing '='
//   decode   all lanes stride over the 8-character groups, 5 bytes each into the pass's LDS slice (pass_verify.hip's
//            decode; the text is read again rather than kept: 600 characters a pass beside a proof of milliseconds)
//   walk     lane 0: the COSE_Sign1 array alone (pass_tbs_locate), the skip stack in LDS; the two byte strings' places and
//            the length of ToBeSigned go to the other lanes through LDS
//   expand   lane l takes words l, l + 256, ...: a word is 32 bytes, its low 32 bits the value and the rest zero, two
//            16-byte vector stores; consecutive lanes write consecutive words
// Every word of a row is written on every path -- a refused pass gets zeros and its word in `bad` set -- so a row that
// held a longer pass in an earlier chunk keeps nothing of it.  Decoded bytes are read through pass_at alone.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "pass_prove.h"

namespace g16 {
namespace {

constexpr uint32_t kInBlock = 256;
constexpr uint32_t kSlice = kPassDecodedMax + 4;
constexpr uint32_t kLayerChunk = 256;   // passes per launch of the layer operator: at most 256 x 129 KB of rows at a time

__global__ __launch_bounds__(kInBlock) void pass_inputs_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offsets,
                                                               const uint32_t* __restrict__ sel, uint32_t cnt, uint32_t max_bytes,
                                                               uint4* __restrict__ d_in, uint32_t* __restrict__ bad) {
  __shared__ uint8_t s_dec[kSlice];
  __shared__ uint32_t s_stack[kPassCborDepth];
  __shared__ uint64_t s_chars_at;
  __shared__ uint32_t s_chars, s_fail, s_not_b32, s_tbs[5];   // prot_off, prot_len, payload_off, payload_len, tbs_len
  const uint32_t tid = threadIdx.x, j = blockIdx.x;
  if (j >= cnt) return;   // (uniform: the grid is cnt workgroups)
  if (tid == 0) {
    const uint32_t i = sel[j];
    const uint64_t at = offsets[i] - offsets[0];   // text holds the bytes from offsets[0] on
    uint32_t start = 0, n_chars = 0;
    s_fail = pass_uri_frame(text + at, offsets[i + 1] - offsets[i], &start, &n_chars) != G16_PASS_OK;
    s_chars_at = at + start;
    s_chars = n_chars;
    s_not_b32 = 0;
  }
  __syncthreads();
  const uint32_t n_chars = s_fail ? 0u : s_chars, n_out = pass_b32_bytes(n_chars);   // (uniform)
  {
    const uint8_t* chars = text + s_chars_at;
    bool good = true;
    for (uint32_t g = tid; g < (n_chars + 7) / 8; g += kInBlock) good = pass_b32_group(chars, n_chars, g, s_dec, n_out) && good;
    if (!good) s_not_b32 = 1;   // (lanes that store, store the same value; s_fail is still being read)
  }
  __syncthreads();
  if (tid == 0 && !s_fail) {
    PassTbsSource t;
    if (!s_not_b32 && pass_tbs_locate(PassBuf{s_dec, n_out}, s_stack, &t) && t.length() <= max_bytes) {
      s_tbs[0] = t.prot_off; s_tbs[1] = t.prot_len; s_tbs[2] = t.payload_off; s_tbs[3] = t.payload_len;
      s_tbs[4] = t.length();
    } else {
      s_fail = 1;
    }
  }
  __syncthreads();
  const bool fail = s_fail != 0;
  const PassTbsSource tbs{PassBuf{s_dec, n_out}, fail ? 0u : s_tbs[0], fail ? 0u : s_tbs[1], fail ? 0u : s_tbs[2], fail ? 0u : s_tbs[3]};
  const uint32_t tbs_len = fail ? 0u : s_tbs[4], words = pass_input_count(max_bytes);
  uint4* row = d_in + (size_t)j * words * 2;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (uint32_t k = tid; k < words; k += kInBlock) {
    const uint32_t v = fail ? 0u : pass_input_word(tbs, tbs_len, max_bytes, k);
    row[2 * (size_t)k] = make_uint4(v, 0, 0, 0);
    row[2 * (size_t)k + 1] = zero;
  }
  if (tid == 0) bad[j] = fail ? 1u : 0u;
}

}  // namespace

int pass_inputs_enqueue(const uint8_t* d_text, const uint64_t* d_offsets, const uint32_t* d_sel, uint32_t cnt, uint32_t max_bytes,
                        void* d_in, uint32_t* d_bad, hipStream_t st) {
  if (cnt == 0) return G16_OK;
  pass_inputs_kernel<<<cnt, kInBlock, 0, st>>>(d_text, d_offsets, d_sel, cnt, max_bytes, (uint4*)d_in, d_bad);
  G16_HIP(hipGetLastError());
  return G16_OK;
}

int pass_device_inputs(int device, const uint8_t* text, const uint64_t* offsets, size_t count, const uint32_t* sel, size_t n_sel,
                       uint32_t max_bytes, uint8_t* out_words, uint32_t* bad) {
  if (const int rc = require_hip_device(device, "pass inputs: no HIP device (device -1 selects the host route)",
                                        "pass inputs: bad device ordinal"))
    return rc;
  G16_HIP(hipSetDevice(device));
  const size_t text_bytes = (size_t)(offsets[count] - offsets[0]), row_bytes = (size_t)pass_input_count(max_bytes) * 32;
  const size_t chunk = n_sel < kLayerChunk ? n_sel : kLayerChunk;
  DeviceJob job("pass inputs");
  DeviceBuf<uint8_t> d_text, d_rows;
  DeviceBuf<uint64_t> d_offsets;
  DeviceBuf<uint32_t> d_sel, d_bad;
  std::vector<uint8_t> rows(chunk * row_bytes);
  // (the rows are not cleared: the kernel writes every word of every row it is given)
  if (job.fail(d_text.alloc(text_bytes)) || job.fail(d_offsets.alloc(count + 1)) || job.fail(d_rows.alloc(chunk * row_bytes)) ||
      job.fail(d_sel.alloc(n_sel)) || job.fail(d_bad.alloc(n_sel)) ||
      (text_bytes && job.fail(hipMemcpy(d_text.p, text + offsets[0], text_bytes, hipMemcpyHostToDevice))) ||
      job.fail(hipMemcpy(d_offsets.p, offsets, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice)) ||
      (n_sel && job.fail(hipMemcpy(d_sel.p, sel, n_sel * 4, hipMemcpyHostToDevice))))
    return job.rc;
  for (size_t at = 0; at < n_sel; at += chunk) {
    const uint32_t cnt = (uint32_t)(n_sel - at < chunk ? n_sel - at : chunk);
    if (const int rc = pass_inputs_enqueue(d_text.p, d_offsets.p, d_sel.p + at, cnt, max_bytes, d_rows.p, d_bad.p + at, nullptr)) return rc;
    if (job.fail(hipMemcpy(rows.data(), d_rows.p, cnt * row_bytes, hipMemcpyDeviceToHost))) return job.rc;
    for (uint32_t j = 0; j < cnt; j++) memcpy(out_words + (size_t)sel[at + j] * row_bytes, &rows[j * row_bytes], row_bytes);
  }
  if (n_sel && job.fail(hipMemcpy(bad, d_bad.p, n_sel * 4, hipMemcpyDeviceToHost))) return job.rc;
  return G16_OK;
}

}  // namespace g16
