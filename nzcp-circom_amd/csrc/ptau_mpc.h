// Phase-1 ceremony pieces of a .ptau file (ptau_mpc.cpp): section 7 in snarkjs's powersoftau_utils.js layout.  Host code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "binfile.h"

namespace g16 {

// One contribution record of section 7, as it lies in the file (p[0, len)); every point affine little-endian Montgomery:
//   tauG1 (64) | tauG2 (128) | alphaG1 (64) | betaG1 (64) | betaG2 (128) |
//   tau.g1_s | tau.g1_sx | alpha.g1_s | alpha.g1_sx | beta.g1_s | beta.g1_sx (64 each) |
//   tau.g2_spx | alpha.g2_spx | beta.g2_spx (128 each) |
//   partialHash (216) | nextChallenge (64) | u32 type | u32 paramsLen | params
struct PtauRecord {
  const uint8_t* p = nullptr;
  size_t len = 0;
  const uint8_t* tau_g1() const { return p; }
  const uint8_t* tau_g2() const { return p + 64; }
  const uint8_t* alpha_g1() const { return p + 192; }
  const uint8_t* beta_g1() const { return p + 256; }
  const uint8_t* beta_g2() const { return p + 320; }
  const uint8_t* g1_s(int key) const { return p + 448 + 128 * key; }      // key: tau = 0, alpha = 1, beta = 2
  const uint8_t* g1_sx(int key) const { return p + 448 + 128 * key + 64; }
  const uint8_t* g2_spx(int key) const { return p + 832 + 128 * key; }
  const uint8_t* next_challenge() const { return p + 1432; }
};
constexpr size_t kPtauKeysAt = 448, kPtauPartialHashAt = 1216, kPtauNextChallengeAt = 1432;
constexpr size_t kPtauRecordFixed = 1432 + 64 + 4 + 4;

// section 7 (u32 n, n records) -> out; G16_E_FORMAT "ptau: Invalid File format" for a section shorter than its records
// say, trailing bytes, a coordinate >= q or a point off its curve (the all-zero image is infinity and passes)
int ptau_records_parse(const BinSection& s7, std::vector<PtauRecord>& out);

}  // namespace g16
