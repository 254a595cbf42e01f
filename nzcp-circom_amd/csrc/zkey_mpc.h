// Phase-2 ceremony pieces of a Groth16 .zkey (zkey_mpc.cpp): section 10 in snarkjs's zkey_utils.js layout, the key as
// the ceremony routes read and rewrite it, the public-key hash of a contribution, and the secrets of a contribution or a
// beacon.  Host code.  Hashing is blake2b.h, arithmetic on file images curve_host.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "binfile.h"
#include "blake2b.h"
#include "curve_host.h"

namespace g16 {

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

// A Groth16 key as the ceremony routes read it (zkey_mpc.cpp, zkey_bellman_host.cpp).  Section 2: alpha1 at 84, beta1 at 148,
// beta2 at 212, gamma2 at 340, delta1 at 468, delta2 at 532.
constexpr size_t kHdrAlpha1 = 84, kHdrDelta1 = 468, kHdrDelta2 = 532, kHdrEnd = 660;
struct KeyView {
  BinView f;
  uint32_t nVars = 0, nPublic = 0, N = 0;
  MpcSection mpc;
};
// exact_89: sections 8 and 9 must have the header's sizes (the verifier only needs whole points: a short section is a
// verdict there, not a malformed file)
int open_key(const uint8_t* zkey, size_t len, KeyView& k, bool exact_89);
// The image of a key that continues the opened key k = zkey: every record of its section table in its order, copied,
// but the first section 10 `extra` bytes longer (room after its old bytes) and the first sections 8 and 9 left unfilled.
// sp[id] = the first section id in the image.  false: the reservation failed (the caller words the error).
bool key_image_layout(const uint8_t* zkey, const KeyView& k, size_t extra, Buf& z, uint8_t* sp[16]);

// A contribution's secret scalars: `count` of them behind each other in standard form, each in [1, r) (else G16_E_ARG
// "<route>: the secret scalars must be in [1, r)"), or NULL for the OS CSPRNG.  count 2: d | s; count 6: tau | alpha |
// beta | s_tau | s_alpha | s_beta.
int read_secrets(const char* route, const uint8_t* secret, Fr* out, int count);
// A contribution's own points (file images): g1_s = [s] G, g1_sx = [d] g1_s, transcript = Blake2b-512(feed | g1_s |
// g1_sx uncompressed) with feed = csHash | hashPubKey of every earlier record (extended here), g2_spx = [d] of the
// transcript's point on G2.
void mpc_contribution(std::vector<uint8_t>& feed, const Fr& d, const Fr& s, uint8_t g1_s[64], uint8_t g1_sx[64],
                      uint8_t g2_spx[128], uint8_t transcript[64]);

// A beacon contribution's public parameters, and its secret scalars (standard form, in [1, r)): count 2 (d, s) or 6
// (tau, alpha, beta, s_tau, s_alpha, s_beta) draws of ONE stream seeded by the delay function (beacon.h), which runs on
// the calling thread.  G16_E_ARG "beacon: the beacon hash must be 1 to 255 bytes" / "beacon: numIterationsExp must be
// between 10 and 63" / "beacon: count must be 2 or 6" before any hashing.
struct BeaconArg { const uint8_t* hash; size_t len; uint32_t exp; };
int mpc_beacon_scalars(const uint8_t* beacon, size_t beacon_len, uint32_t exp, int count, Fr* out);
// a beacon record's key under the verifiers: g1_s = [s] G1 and g1_sx = [x] g1_s (file images)
bool mpc_beacon_key_ok(const uint8_t* g1_s, const uint8_t* g1_sx, const Fr& x, const Fr& s);

std::string mpc_name_params(const char* name);   // a record's params for a contribution's name (or NULL)

}  // namespace g16
