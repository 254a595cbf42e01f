// Phase-2 ceremony pieces of a Groth16 .zkey (zkey_mpc.cpp): section 10 in snarkjs's zkey_utils.js layout, Blake2b-512,
// the public-key hash of a contribution and the transcript's point on G2.  Host code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "binfile.h"
#include "ec.cuh"

namespace g16 {

void blake2b512(const uint8_t* data, size_t len, uint8_t out[64]);   // RFC 7693, unkeyed

// One contribution record of section 10, as it lies in the file (p[0, len)):
//   deltaAfter G1 (64) | delta.g1_s (64) | delta.g1_sx (64) | delta.g2_spx (128) | transcript (64) | u32 type |
//   u32 paramsLen | params
struct MpcRecord {
  const uint8_t* p = nullptr;
  size_t len = 0;
  const uint8_t* delta_after() const { return p; }
  const uint8_t* g1_s() const { return p + 64; }
  const uint8_t* g1_sx() const { return p + 128; }
  const uint8_t* g2_spx() const { return p + 192; }
  const uint8_t* transcript() const { return p + 320; }
};
constexpr size_t kMpcRecordFixed = 64 + 64 + 64 + 128 + 64 + 4 + 4;

struct MpcSection {
  const uint8_t* cs_hash = nullptr;   // 64 bytes
  std::vector<MpcRecord> rec;
};
// section 10 -> out; G16_E_FORMAT "zkey: Invalid File format" for a section shorter than its records say, trailing
// bytes, a coordinate >= q or a point off its curve (the all-zero image is infinity and passes)
int mpc_parse(const BinSection& s10, MpcSection& out);

// snarkjs hashPubKey fed into a running buffer: the four points in uncompressed big-endian standard form, then the
// transcript
void mpc_hash_pubkey(std::vector<uint8_t>& feed, const MpcRecord& r);
void g1_uncompressed(const uint8_t lem[64], uint8_t out[64]);
void g2_uncompressed(const uint8_t lem[128], uint8_t out[128]);

void hash_to_g2(const uint8_t transcript[64], G2Affine& out);

// Shared with the .ptau ceremony (ptau_mpc.cpp).  File images are affine little-endian Montgomery, infinity = zeros.
bool mpc_g1_image_ok(const uint8_t* p);   // coordinates below q and the point on its curve (infinity passes)
bool mpc_g2_image_ok(const uint8_t* p);
void mpc_mul_g1(const uint8_t* lem, const Fr& k_std, uint8_t* out);   // [k] P on the host
void mpc_mul_g2(const uint8_t* lem, const Fr& k_std, uint8_t* out);
int mpc_os_random(uint8_t* out, size_t n);
int mpc_random_fr(uint8_t* out, uint64_t n);   // n fresh standard-form scalars below r: ChaCha20 keyed from the OS CSPRNG
std::string mpc_name_params(const char* name);   // a record's params for a contribution's name (or NULL)
// one pair of g16_pairing_op's input appended: six standard-form words
void mpc_pair_words(std::vector<uint8_t>& in, const uint8_t* g1_lem, const uint8_t* g2_lem);

}  // namespace g16
