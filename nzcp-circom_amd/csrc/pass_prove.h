// Between pass_prove_host.cpp (the public calls g16_pass_inputs, g16_pass_fullprove_batch and its PLONK twin, their
// checks and the host-thread route) and pass_prove.hip (pass_inputs_kernel): a pass URI -> the input words of its proof,
// toBeSigned[8 M] and toBeSignedLen, formed on the device where the witness calculator reads them.
#pragma once
#include <hip/hip_runtime.h>

#include "pass_verify.h"

namespace g16 {

// One pass's row of 8 M + 1 words on a thread of its own (the host route; the kernel runs the same pieces with the
// decode and the expansion spread over its lanes): dec = kPassDecodedMax bytes, stack = kPassCborDepth words.  The row
// is written completely on every path; false: all zeros -- the text does not frame, is not base32, the COSE_Sign1
// walk fails or ToBeSigned exceeds max_bytes.
inline bool pass_inputs_one(const uint8_t* text, uint64_t n, uint32_t max_bytes, uint8_t* dec, uint32_t* stack, uint8_t* row) {
  const uint32_t words = pass_input_count(max_bytes);
  for (size_t k = 0; k < (size_t)words * 32; k++) row[k] = 0;
  uint32_t start = 0, n_chars = 0;
  if (pass_uri_frame(text, n, &start, &n_chars) != G16_PASS_OK) return false;
  const uint32_t bytes = pass_b32_bytes(n_chars);
  if (!pass_b32_decode(text + start, n_chars, dec, bytes)) return false;
  PassTbsSource tbs;
  if (!pass_tbs_locate(PassBuf{dec, bytes}, stack, &tbs)) return false;
  const uint32_t tbs_len = tbs.length();
  if (tbs_len > max_bytes) return false;
  for (uint32_t k = 0; k < words; k++) {
    const uint32_t v = pass_input_word(tbs, tbs_len, max_bytes, k);
    for (int j = 0; j < 4; j++) row[(size_t)k * 32 + j] = (uint8_t)(v >> (8 * j));
  }
  return true;
}

// ---------------------------------------------------------------- the device route (pass_prove.hip)
// cnt rows of 8 M + 1 words at d_in for the passes sel[0, cnt) of the uploaded text, bad[j] = 1 and a zero row where the
// device refuses pass sel[j]; on `st`, enqueue only.  Everything lies on the stream's device.
int pass_inputs_enqueue(const uint8_t* d_text, const uint64_t* d_offsets, const uint32_t* d_sel, uint32_t cnt, uint32_t max_bytes,
                        void* d_in, uint32_t* d_bad, hipStream_t st);
// the layer operator's device route: rows of the passes sel[0, n_sel) land at out_words + sel[j] * (8 M + 1) * 32, their
// bad words at bad[j]
int pass_device_inputs(int device, const uint8_t* text, const uint64_t* offsets, size_t count, const uint32_t* sel, size_t n_sel,
                       uint32_t max_bytes, uint8_t* out_words, uint32_t* bad);

}  // namespace g16
