// The MPCParams file of the phase-2 exchange (zkey_bellman_host.cpp; snarkjs 0.4.12 zkey_export_bellman.js): a Groth16 key
// without its coefficients, every point in uncompressed big-endian standard form (G1 64 bytes, G2 128 bytes, infinity =
// byte 0 = 0x40 and the rest zero), counts u32 big-endian:
//   alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2                                    (576 bytes)
//   u32 | IC    u32 | H    u32 | L    u32 | A    u32 | B1    u32 | B2 (G2)               (the six runs)
//   csHash (64) | u32 c | c x ( deltaAfter | g1_s | g1_sx | g2_spx (G2) | transcript (64) )   (384 bytes a record)
// A record is its hashPubKey feed as it stands.  Host code.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace g16 {

constexpr size_t kMpHeader = 576, kMpDelta1 = 384, kMpDelta2 = 448, kMpRecord = 384;
constexpr int kMpRuns = 6;                                             // IC, H, L, A, B1, B2
constexpr size_t kMpRunPoint[kMpRuns] = {64, 64, 64, 64, 64, 128};

struct MpView {
  const uint8_t* hdr = nullptr;
  const uint8_t* run[kMpRuns] = {};
  uint32_t cnt[kMpRuns] = {};
  const uint8_t* cs_hash = nullptr;
  uint32_t nrec = 0;
  const uint8_t* rec = nullptr;   // nrec x kMpRecord
};
// The walk by the file's own counts and what needs no point arithmetic: the length the counts ask for, every flag a
// clean 0x40 or none, every coordinate below q.  G16_E_FORMAT "mpcparams: Invalid File format".
int mp_open(const uint8_t* p, size_t len, MpView& m);

// The image's head from a key (the export's own; the circuit hash of `zkey new` is taken over it, zkey_cshash_host.cpp):
// the six header points of section 2, and the six counts p + 1, N - 1, n - p - 1, n, n, n.
void mp_header_image(const uint8_t* sec2, uint8_t out[kMpHeader]);
void mp_key_counts(uint32_t nVars, uint32_t nPublic, uint32_t N, uint32_t cnt[kMpRuns]);

}  // namespace g16
