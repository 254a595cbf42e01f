// `snarkjs powersoftau new`, `powersoftau contribute` and `powersoftau verify` ([EXT] snarkjs 0.4.12 powersoftau_new.js,
// powersoftau_contribute.js, powersoftau_verify.js, powersoftau_utils.js; keypair.js for the keys).
//   new:        sections 1-7 with every point the generator (host only).
//   contribute: point i of sections 2 / 3 <- [tau^i], 4 <- [alpha tau^i], 5 <- [beta tau^i], 6 <- [beta] (ptau_scale.hip,
//               every lane forms its scalar on the device), one record more in section 7.
//   verify:     the file is the generator file plus a chain of honest contributions -- the record walk (same-ratio
//               pairing checks), the challenge hash of the file, one random linear combination per section for the
//               powers (MSMs on the Pippenger operators, pairings on the verifier's device code) and, when the file is
//               prepared, sections 12-15 against a fresh transform.
// The record LAYOUT and the powers are snarkjs's.  The TRANSCRIPT is not: snarkjs hashes a challenge / response file
// exchange of compressed points and stores a hasher snapshot in partialHash; here
//   challengeHash(state, prev) = Blake2b-512(prev | every point of sections 2, 3, 4, 5, 6 in that order, uncompressed
//                                big-endian standard form),
// the first challenge is that of the file as it stands with prev = Blake2b-512(""), every later one the last record's
// nextChallenge; for key x (tau = 0, alpha = 1, beta = 2) g1_s = [s_x]G1, g1_sx = [x]g1_s, g2_sp =
// hash_to_g2(Blake2b-512(challenge | byte x | g1_s | g1_sx)), g2_spx = [x]g2_sp; responseHash = Blake2b-512(challenge |
// the nine key points in record order); nextChallenge = challengeHash(new state, responseHash); partialHash is 216 zero
// bytes that nothing reads.  snarkjs's `powersoftau verify` is NOT claimed to accept this transcript.
//   beacon:     a contribution whose six secret scalars anyone recomputes from a public beacon hash and an iteration
//               exponent (beacon.h, mpc_beacon_scalars): a record of type 1 that states both; verify recomputes them for
//               every such record.  The derivation is this library's, as the `-e` rule is: a snarkjs-made beacon record
//               fails that check here.
// The challenge / response file exchange ([EXT] powersoftau_export_challenge.js, powersoftau_challenge_contribute.js,
// powersoftau_import.js, restated without ffjavascript, which is not available here): the transcript above already IS
// that of the files --
//   challenge file = prev | every point of sections 2-6 uncompressed            (its Blake2b-512 = challengeHash)
//   response file  = challenge hash | the same points compressed | the nine key points uncompressed
//   export challenge:     host only; prev = Blake2b-512("") or the last record's responseHash, recomputed.
//   challenge contribute: from-be, ptau_scale, compress on the device (ptau_points.hip), the keys as in contribute.
//   import response:      decompress on the device (a square root per point), the record as contribute builds it, the
//                         record checks of verify before anything is written.
// import(old, contribute(export(old), secret), name) = contribute(old, name, secret) byte for byte.  DEPARTURE: the
// hash printed and returned is responseHash (the response's first 64 and last 768 bytes), not snarkjs's Blake2b-512 of
// the whole response file.
#include "ptau_mpc.h"

#include <algorithm>
#include <atomic>
#include <chrono>

#include "beacon.h"
#include "host_util.h"
#include "internal.h"
#include "mapped_file.h"
#include "pair_checks.h"
#include "ptau.h"
#include "zkey_mpc.h"

namespace g16 {

int ptau_records_parse(const BinSection& s7, std::vector<PtauRecord>& out) {
  out.clear();
  if (!s7.p) return G16_OK;   // (no section 7: no contributions, as g16_ptau_prepare reads it)
  if (s7.size < 4) return ptau_bad("Invalid File format");
  const uint32_t n = rd32(s7.p);
  uint64_t pos = 4;
  for (uint32_t i = 0; i < n; i++) {
    if (s7.size - pos < kPtauRecordFixed) return ptau_bad("Invalid File format");
    const uint8_t* r = s7.p + pos;
    const uint32_t plen = rd32(r + kPtauRecordFixed - 4);
    if (s7.size - pos - kPtauRecordFixed < plen) return ptau_bad("Invalid File format");
    const PtauRecord rec{r, kPtauRecordFixed + plen};
    bool ok = g1_image_ok(rec.tau_g1()) && g2_image_ok(rec.tau_g2()) && g1_image_ok(rec.alpha_g1()) &&
              g1_image_ok(rec.beta_g1()) && g2_image_ok(rec.beta_g2());
    for (int x = 0; x < 3 && ok; x++) ok = g1_image_ok(rec.g1_s(x)) && g1_image_ok(rec.g1_sx(x)) && g2_image_ok(rec.g2_spx(x));
    if (!ok) return ptau_bad("Invalid File format");
    out.push_back(rec);
    pos += rec.len;
  }
  if (pos != s7.size) return ptau_bad("Invalid File format");
  return G16_OK;
}

namespace {

constexpr uint32_t kPowerMax = 24;   // (what g16_ptau_prepare takes; the device arrays index with 32 bits)

int power_above_limit(const char* route, uint32_t power) {
  set_error(std::string(route) + ": power " + std::to_string(power) + " is above the supported limit of " + std::to_string(kPowerMax));
  return G16_E_ARG;
}

constexpr size_t kThreadedFrom = 8192;   // points of a section before the host loops over it take more than one thread

// the ceremony as the two routes read it
struct Ceremony {
  PtauView pv;
  uint64_t n = 0;          // 2^power
  uint64_t cnt[7] = {};    // points of sections 2-6
  std::vector<PtauRecord> rec;
  static size_t psz(int id) { return id == 3 || id == 6 ? 128 : 64; }
  size_t points_bytes() const {
    size_t t = 0;
    for (int id = 2; id <= 6; id++) t += cnt[id] * psz(id);
    return t;
  }
};

int open_ceremony(const uint8_t* ptau, size_t len, const char* route, Ceremony& c) {
  if (const int rc = ptau_open(ptau, len, c.pv, /*tau_sections=*/false)) return rc;
  if (c.pv.power > kPowerMax) return power_above_limit(route, c.pv.power);
  c.n = (uint64_t)1 << c.pv.power;
  c.cnt[2] = 2 * c.n - 1; c.cnt[3] = c.n; c.cnt[4] = c.n; c.cnt[5] = c.n; c.cnt[6] = 1;
  for (int id = 2; id <= 6; id++)
    if (!c.pv.sec[id].p || c.pv.sec[id].size != c.cnt[id] * Ceremony::psz(id)) return ptau_bad("Invalid File format");
  return ptau_records_parse(c.pv.sec[7], c.rec);
}

// the uncompressed big-endian images of sections 2-6 (sec[id] = cnt[id] file images), behind each other at q
void points_be_host(const uint8_t* const sec[7], const uint64_t cnt[7], uint8_t* q) {
  for (int id = 2; id <= 6; id++) {
    const uint8_t* s = sec[id];
    const int threads = host_threads(cnt[id], kThreadedFrom);
    if (Ceremony::psz(id) == 64) parallel_for(cnt[id], threads, [=](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) g1_uncompressed(s + i * 64, q + i * 64); });
    else parallel_for(cnt[id], threads, [=](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) g2_uncompressed(s + i * 128, q + i * 128); });
    q += cnt[id] * Ceremony::psz(id);
  }
}

// Blake2b-512(challenge | byte key | g1_s | g1_sx uncompressed) -> the key's point on G2
void key_g2_sp(const uint8_t challenge[64], int key, const uint8_t* g1_s, const uint8_t* g1_sx, G2Affine& sp) {
  uint8_t feed[64 + 1 + 128], h[64];
  memcpy(feed, challenge, 64);
  feed[64] = (uint8_t)key;
  g1_uncompressed(g1_s, feed + 65);
  g1_uncompressed(g1_sx, feed + 129);
  blake2b512(feed, sizeof(feed), h);
  hash_to_g2(h, sp);
}

// Blake2b-512(challenge | the nine key points of a record, uncompressed, in record order)
constexpr size_t kKeysBytes = 6 * 64 + 3 * 128;
void keys_uncompressed(const PtauRecord& r, uint8_t out[kKeysBytes]) {   // (how a response file ends)
  for (int x = 0; x < 3; x++) {
    g1_uncompressed(r.g1_s(x), out + 128 * x);
    g1_uncompressed(r.g1_sx(x), out + 128 * x + 64);
    g2_uncompressed(r.g2_spx(x), out + 384 + 128 * x);
  }
}
void response_hash(const uint8_t challenge[64], const PtauRecord& r, uint8_t out[64]) {
  uint8_t feed[64 + kKeysBytes];
  memcpy(feed, challenge, 64);
  keys_uncompressed(r, feed + 64);
  blake2b512(feed, sizeof(feed), out);
}

// the challenge of the generator file of this ceremony's size: what the first record's keys are bound to
void generator_challenge(const Ceremony& c, uint8_t out[64]) {
  std::vector<uint8_t> feed(64 + c.points_bytes());
  blake2b512(nullptr, 0, feed.data());
  uint8_t u1[64], u2[128];
  g1_uncompressed(gens().g1, u1);
  g2_uncompressed(gens().g2, u2);
  uint8_t* q = feed.data() + 64;
  for (int id = 2; id <= 6; id++)
    for (uint64_t i = 0; i < c.cnt[id]; i++) {
      if (Ceremony::psz(id) == 64) memcpy(q, u1, 64); else memcpy(q, u2, 128);
      q += Ceremony::psz(id);
    }
  blake2b512(feed.data(), feed.size(), out);
}

// the nine key points of a record (rec = its first byte) for the challenge it answers; key = tau, alpha, beta and
// sk = s_tau, s_alpha, s_beta: the two halves of the six secret scalars
void make_keys(const uint8_t challenge[64], const Fr key[3], const Fr sk[3], uint8_t* rec) {
  for (int x = 0; x < 3; x++) {
    uint8_t* g1_s = rec + kPtauKeysAt + 128 * x;
    mul_image<FqOps>(gens().g1, sk[x], g1_s);
    mul_image<FqOps>(g1_s, key[x], g1_s + 64);
    G2Affine sp2;
    key_g2_sp(challenge, x, g1_s, g1_s + 64, sp2);
    mul_image<Fq2Ops>((const uint8_t*)&sp2, key[x], rec + 832 + 128 * x);
  }
}

// Step 2 of the verifier for ONE record against the state before it (cur: tauG1, alphaG1, betaG1, advanced to the
// record's): the infinity test, then eight same-ratio checks with their texts appended to the batch.  -> the infinity
// text, or nullptr.  Shared by `verify` and `import response`, which differ in the texts' prefix alone.
struct RecordTexts { const char* inf; const char* key; const char* chain[3]; const char* tau_g2; const char* beta_g2; };
#define G16_RECORD_TEXTS(route)                                                                                      \
  {route ": a contribution holds the point at infinity", route ": a contribution's public key is not consistent",    \
   {route ": a contribution's tauG1 does not continue the chain", route ": a contribution's alphaG1 does not continue the chain", \
    route ": a contribution's betaG1 does not continue the chain"},                                                  \
   route ": a contribution's tauG2 does not match its tauG1", route ": a contribution's betaG2 does not match its betaG1"}
const char* record_checks(const RecordTexts& t, const PtauRecord& r, const uint8_t* cur[3], const uint8_t challenge[64],
                          PairChecks& checks) {
  bool inf = all_zero(r.tau_g1(), 64) || all_zero(r.tau_g2(), 128) || all_zero(r.alpha_g1(), 64) || all_zero(r.beta_g1(), 64) ||
             all_zero(r.beta_g2(), 128);
  for (int x = 0; x < 3; x++) inf = inf || all_zero(r.g1_s(x), 64) || all_zero(r.g1_sx(x), 64) || all_zero(r.g2_spx(x), 128);
  if (inf) return t.inf;
  const Gens& G = gens();
  const uint8_t* now[3] = {r.tau_g1(), r.alpha_g1(), r.beta_g1()};
  for (int x = 0; x < 3; x++) {
    G2Affine g2_sp;
    key_g2_sp(challenge, x, r.g1_s(x), r.g1_sx(x), g2_sp);
    checks.same_ratio(r.g1_s(x), r.g1_sx(x), (const uint8_t*)&g2_sp, r.g2_spx(x), t.key);
    checks.same_ratio(cur[x], now[x], (const uint8_t*)&g2_sp, r.g2_spx(x), t.chain[x]);
    cur[x] = now[x];
  }
  checks.same_ratio(G.g1, r.tau_g1(), G.g2, r.tau_g2(), t.tau_g2);
  checks.same_ratio(G.g1, r.beta_g1(), G.g2, r.beta_g2(), t.beta_g2);
  return nullptr;
}

// The output image of a contribution: sections 1-7 framed, section 1 and the old records copied, the count raised;
// -> where the new record (rec_len bytes) goes, or nullptr when the reservation failed
uint8_t* layout_with_record(const Ceremony& c, size_t rec_len, Buf& z, uint8_t* sp[16]) {
  static const uint8_t no_contributions[4] = {0, 0, 0, 0};
  const uint8_t* old7 = c.pv.sec[7].p ? c.pv.sec[7].p : no_contributions;
  const uint64_t old7_size = c.pv.sec[7].p ? c.pv.sec[7].size : 4;
  uint64_t sizes[16] = {};
  for (int id = 1; id <= 6; id++) sizes[id] = c.pv.sec[id].size;
  sizes[7] = old7_size + rec_len;
  static const int ids[7] = {1, 2, 3, 4, 5, 6, 7};
  if (!bin_layout(z, "ptau", 1, ids, 7, sizes, sp)) return nullptr;
  memcpy(sp[1], c.pv.sec[1].p, sizes[1]);
  memcpy(sp[7], old7, old7_size);
  const uint32_t count = (uint32_t)c.rec.size() + 1;
  memcpy(sp[7], &count, 4);
  return sp[7] + old7_size;
}

int new_core(uint32_t power, uint8_t** out, size_t* out_len) {
  if (power > kPowerMax) return power_above_limit("ptau new", power);
  const uint64_t n = (uint64_t)1 << power;
  const uint64_t sizes[16] = {0, 44, (2 * n - 1) * 64, n * 128, n * 64, n * 64, 128, 4};
  static const int ids[7] = {1, 2, 3, 4, 5, 6, 7};
  Buf z;
  uint8_t* sp[16] = {};
  if (!bin_layout(z, "ptau", 1, ids, 7, sizes, sp)) { set_error("ptau new: out of memory"); return G16_E_STATE; }
  uint8_t* q = bin_put_field(sp[1], kFqP);
  memcpy(q, &power, 4); memcpy(q + 4, &power, 4);
  for (int id = 2; id <= 6; id++) {
    const size_t psz = Ceremony::psz(id);
    for (uint64_t i = 0; i < sizes[id] / psz; i++) memcpy(sp[id] + i * psz, psz == 64 ? gens().g1 : gens().g2, psz);
  }
  memset(sp[7], 0, 4);
  z.give(out, out_len);
  return G16_OK;
}

// The challenge this file poses: without records that of its points with prev = Blake2b-512(""), else the last record's
// nextChallenge.  feed <- room for prev | the big-endian images of sections 2-6 (those of the file's points in the
// first case), which the next challenge is hashed over
void file_challenge(const Ceremony& c, std::vector<uint8_t>& feed, uint8_t challenge[64]) {
  feed.resize(64 + c.points_bytes());
  if (!c.rec.empty()) { memcpy(challenge, c.rec.back().next_challenge(), 64); return; }
  const uint8_t* in[7] = {};
  for (int id = 2; id <= 6; id++) in[id] = c.pv.sec[id].p;
  blake2b512(nullptr, 0, feed.data());
  points_be_host(in, c.cnt, feed.data() + 64);
  blake2b512(feed.data(), feed.size(), challenge);
}

// The tail of a new record (rec: its keys in place) from the new sections sp[2 .. 6], whose big-endian images lie in
// feed: the state after the contribution -- tauG1 / tauG2 are point 1 of sections 2 / 3, which a power-0 file does not
// hold (the caller has set them) --, response <- responseHash, and the seal: nextChallenge, type and params
void seal_record(const Ceremony& c, uint8_t* const sp[16], const uint8_t challenge[64], std::vector<uint8_t>& feed,
                 uint32_t type, const std::string& params, uint8_t* rec, uint8_t response[64]) {
  if (c.pv.power >= 1) {
    memcpy(rec, sp[2] + 64, 64);
    memcpy(rec + 64, sp[3] + 128, 128);
  }
  memcpy(rec + 192, sp[4], 64);
  memcpy(rec + 256, sp[5], 64);
  memcpy(rec + 320, sp[6], 128);
  response_hash(challenge, PtauRecord{rec, kPtauRecordFixed + params.size()}, response);
  memcpy(feed.data(), response, 64);
  blake2b512(feed.data(), feed.size(), rec + kPtauNextChallengeAt);
  const uint32_t plen = (uint32_t)params.size();
  memcpy(rec + kPtauNextChallengeAt + 64, &type, 4);
  memcpy(rec + kPtauNextChallengeAt + 68, &plen, 4);
  if (plen) memcpy(rec + kPtauRecordFixed, params.data(), plen);
}

// bc: `powersoftau beacon` -- the secret is the beacon's (the chain runs here, on this thread, before the device is
// touched), the record is of type 1 and states the beacon after the name; everything else is the contribution's
int contribute_core(const uint8_t* ptau, size_t len, const char* name, const uint8_t* secret, const BeaconArg* bc, int device,
                    uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  const auto t0 = std::chrono::steady_clock::now();
  const char* route = bc ? "ptau beacon" : "ptau contribute";
  Ceremony c;
  if (const int rc = open_ceremony(ptau, len, route, c)) return rc;
  Fr x[6];
  if (const int rc = bc ? mpc_beacon_scalars(bc->hash, bc->len, bc->exp, 6, x) : read_secrets(route, secret, x, 6)) return rc;
  const Fr *key = x, *sk = x + 3;
  if (const int rc = require_hip_device(route, device)) return rc;

  std::string params = mpc_name_params(name);
  if (bc) params += beacon_params(bc->hash, bc->len, bc->exp);
  const size_t rec_len = kPtauRecordFixed + params.size();
  Buf z;
  uint8_t* sp[16] = {};
  uint8_t* rec = layout_with_record(c, rec_len, z, sp);
  if (!rec) { set_error(std::string(route) + ": out of memory"); return G16_E_STATE; }
  memset(rec, 0, rec_len);   // (partialHash stays zero)

  // the challenge this contribution answers
  const auto th0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> feed;
  uint8_t challenge[64];
  file_challenge(c, feed, challenge);
  make_keys(challenge, key, sk, rec);
  double hash_ms = ms_since(th0);

  // device: the sections, and the big-endian images of the new points straight into the next challenge's feed
  Fr one = fp_zero<FrParams>();
  one.v[0] = 1;
  ChunkStats st[5];
  {
    uint8_t* be = feed.data() + 64;
    const Fr* cs[7] = {nullptr, nullptr, &one, &one, &key[1], &key[2], &key[2]};
    int rc = G16_OK;
    for (int id = 2; id <= 6 && !rc; id++) {
      const Fr& k = id == 6 ? one : key[0];
      rc = Ceremony::psz(id) == 64 ? ptau_scale_g1(device, c.pv.sec[id].p, c.cnt[id], *cs[id], k, 0, sp[id], be, &st[id - 2])
                                   : ptau_scale_g2(device, c.pv.sec[id].p, c.cnt[id], *cs[id], k, 0, sp[id], be, &st[id - 2]);
      be += c.cnt[id] * Ceremony::psz(id);
    }
    if (rc) return rc;
  }

  // the record; in a power-0 file tauG1 / tauG2 continue the last record's (or the generators)
  const auto th1 = std::chrono::steady_clock::now();
  if (c.pv.power == 0) {
    mul_image<FqOps>(c.rec.empty() ? gens().g1 : c.rec.back().tau_g1(), key[0], rec);
    mul_image<Fq2Ops>(c.rec.empty() ? gens().g2 : c.rec.back().tau_g2(), key[0], rec + 64);
  }
  uint8_t response[64];
  seal_record(c, sp, challenge, feed, bc ? 1 : 0, params, rec, response);
  if (contribution_hash) memcpy(contribution_hash, response, 64);
  hash_ms += ms_since(th1);

  if (getenv("G16_TRACE_HOST")) {
    uint64_t g1 = 0, g2 = 0;
    float k1 = 0, k2 = 0, xf = 0;
    for (int id = 2; id <= 6; id++) {
      const ChunkStats& s = st[id - 2];
      if (Ceremony::psz(id) == 64) { g1 += s.points; k1 += s.kern_ms; } else { g2 += s.points; k2 += s.kern_ms; }
      xf += s.xfer_ms;
    }
    fprintf(stderr,
            "[g16] %s: points G1 %llu G2 %llu; kernels G1 %.3f ms G2 %.3f ms, transfers %.3f ms; host hashing %.3f ms "
            "(big-endian images of the new points made on the device%s); call %.3f ms\n",
            route, (unsigned long long)g1, (unsigned long long)g2, k1, k2, xf, hash_ms,
            c.rec.empty() ? ", of the input on the host" : "", ms_since(t0));
  }
  z.give(out, out_len);
  return G16_OK;
}

// ------------------------------------------------------------------ the challenge / response exchange
// `prev` of the challenge file: Blake2b-512("") without records, else the last record's responseHash -- not stored,
// recomputed from its key points and the challenge IT answered
void last_response_hash(const Ceremony& c, uint8_t out[64]) {
  if (c.rec.empty()) { blake2b512(nullptr, 0, out); return; }
  uint8_t answered[64];
  if (c.rec.size() >= 2) memcpy(answered, c.rec[c.rec.size() - 2].next_challenge(), 64);
  else generator_challenge(c, answered);
  response_hash(answered, c.rec.back(), out);
}

int power_zero(const char* route) {
  set_error(std::string(route) + ": power 0 is not supported (a power-0 response holds no point 1 to take tauG1 from)");
  return G16_E_ARG;
}

int export_challenge_core(const uint8_t* ptau, size_t len, uint8_t** out, size_t* out_len, uint8_t challenge_hash[64]) {
  Ceremony c;
  if (const int rc = open_ceremony(ptau, len, "ptau export challenge", c)) return rc;
  Buf z;
  if (!z.reserve(64 + c.points_bytes())) { set_error("ptau export challenge: out of memory"); return G16_E_STATE; }
  last_response_hash(c, z.skip(64));
  const uint8_t* in[7] = {};
  for (int id = 2; id <= 6; id++) in[id] = c.pv.sec[id].p;
  points_be_host(in, c.cnt, z.skip(c.points_bytes()));
  uint8_t h[64];
  blake2b512(z.p, z.len, h);
  if (!c.rec.empty() && memcmp(h, c.rec.back().next_challenge(), 64) != 0) {
    set_error("ptau export challenge: the file's points are not the last contribution's challenge");
    return G16_E_FORMAT;
  }
  if (challenge_hash) memcpy(challenge_hash, h, 64);
  z.give(out, out_len);
  return G16_OK;
}

int bad_point(const char* route, int64_t i, int id) {
  set_error(std::string(route) + ": point " + std::to_string(i) + " of section " + std::to_string(id) + " is not a point of the curve");
  return G16_E_FORMAT;
}

void trace_points(const char* route, const char* const stage[3], const ChunkStats st[5][3], double call_ms) {
  if (!getenv("G16_TRACE_HOST")) return;
  std::string kernels;
  float xf = 0;
  for (int j = 0; j < 3; j++) {
    if (!stage[j]) continue;
    float ms = 0;
    for (int s = 0; s < 5; s++) { ms += st[s][j].kern_ms; xf += st[s][j].xfer_ms; }
    char buf[64];
    snprintf(buf, sizeof(buf), "%s %.3f ms, ", stage[j], ms);
    kernels += buf;
  }
  fprintf(stderr, "[g16] %s: kernels %stransfers %.3f ms; call %.3f ms\n", route, kernels.c_str(), xf, call_ms);
}

int challenge_contribute_core(const uint8_t* ch, size_t len, const uint8_t* secret, int device, uint8_t** out, size_t* out_len,
                              uint8_t contribution_hash[64]) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t n = len >= 128 + 384 && (len - 128) % 384 == 0 ? (len - 128) / 384 : 0;
  if (n == 0 || (n & (n - 1)) || n > ((uint64_t)1 << kPowerMax)) {
    set_error("ptau challenge: Invalid File format");
    return G16_E_FORMAT;
  }
  if (n == 1) return power_zero("ptau challenge contribute");
  Fr x[6];
  if (const int rc = read_secrets("ptau challenge contribute", secret, x, 6)) return rc;
  const Fr *key = x, *sk = x + 3;
  if (const int rc = require_hip_device("ptau challenge contribute", device)) return rc;

  const uint64_t cnt[7] = {0, 0, 2 * n - 1, n, n, n, 1};
  Buf z;
  if (!z.reserve(192 * n + 864)) { set_error("ptau challenge contribute: out of memory"); return G16_E_STATE; }
  uint8_t challenge[64];
  blake2b512(ch, len, challenge);
  z.put(challenge, 64);
  uint8_t rec[kPtauRecordFixed] = {};
  make_keys(challenge, key, sk, rec);

  // per section: big-endian -> file form (checked), scaled, compressed; three passes of the device over host buffers
  Fr one = fp_zero<FrParams>();
  one.v[0] = 1;
  const Fr* cs[7] = {nullptr, nullptr, &one, &one, &key[1], &key[2], &key[2]};
  std::vector<uint8_t> a(std::max<uint64_t>(cnt[2] * 64, n * 128)), b(a.size());
  ChunkStats st[5][3];
  const uint8_t* src = ch + 64;
  for (int id = 2; id <= 6; id++) {
    const size_t psz = Ceremony::psz(id);
    const bool g2 = psz == 128;
    int64_t bad = -1;
    if (const int rc = ptau_points_from_be(device, g2, src, cnt[id], a.data(), &bad, &st[id - 2][0])) return rc;
    if (bad >= 0) return bad_point("ptau challenge contribute", bad, id);
    const Fr& k = id == 6 ? one : key[0];
    if (const int rc = g2 ? ptau_scale_g2(device, a.data(), cnt[id], *cs[id], k, 0, b.data(), nullptr, &st[id - 2][1])
                          : ptau_scale_g1(device, a.data(), cnt[id], *cs[id], k, 0, b.data(), nullptr, &st[id - 2][1]))
      return rc;
    if (const int rc = ptau_points_compress(device, g2, b.data(), cnt[id], z.skip(cnt[id] * psz / 2), &st[id - 2][2])) return rc;
    src += cnt[id] * psz;
  }
  const PtauRecord R{rec, sizeof(rec)};
  keys_uncompressed(R, z.skip(kKeysBytes));
  if (contribution_hash) response_hash(challenge, R, contribution_hash);
  static const char* const stages[3] = {"from-be", "scale", "compress"};
  trace_points("ptau challenge contribute", stages, st, ms_since(t0));
  z.give(out, out_len);
  return G16_OK;
}

int import_response_core(const uint8_t* ptau, size_t len, const uint8_t* resp, size_t rlen, const char* name, int device,
                         uint8_t** out, size_t* out_len, uint8_t contribution_hash[64], int* ok) {
  const auto t0 = std::chrono::steady_clock::now();
  *ok = 0;
  *out = nullptr;
  *out_len = 0;
  Ceremony c;
  if (const int rc = open_ceremony(ptau, len, "ptau import response", c)) return rc;
  if (c.pv.power == 0) return power_zero("ptau import response");
  if (rlen != 192 * c.n + 864) { set_error("ptau import response: Invalid File format"); return G16_E_FORMAT; }
  auto verdict = [&](const char* why) { set_error(why); return G16_OK; };
  const Gens& G = gens();

  // the challenge the response must answer: the file's own
  std::vector<uint8_t> feed;
  uint8_t challenge[64];
  file_challenge(c, feed, challenge);
  if (memcmp(resp, challenge, 64) != 0) return verdict("ptau import response: the response does not answer this file's challenge");

  const std::string params = mpc_name_params(name);
  const size_t rec_len = kPtauRecordFixed + params.size();
  std::vector<uint8_t> recbuf(rec_len, 0);   // (partialHash stays zero)
  uint8_t* rec = recbuf.data();
  const PtauRecord R{rec, rec_len};
  {
    const uint8_t* kp = resp + rlen - kKeysBytes;
    bool good = true;
    for (int x = 0; x < 3 && good; x++)
      good = image_from_be(kp + 128 * x, 64, rec + kPtauKeysAt + 128 * x) && image_from_be(kp + 128 * x + 64, 64, rec + kPtauKeysAt + 128 * x + 64) &&
             image_from_be(kp + 384 + 128 * x, 128, rec + 832 + 128 * x);
    if (!good) { set_error("ptau import response: a key point is not a valid image"); return G16_E_FORMAT; }
  }
  if (const int rc = require_hip_device("ptau import response", device)) return rc;

  Buf z;
  uint8_t* sp[16] = {};
  uint8_t* rec_out = layout_with_record(c, rec_len, z, sp);
  if (!rec_out) { set_error("ptau import response: out of memory"); return G16_E_STATE; }

  // device: the sections, and the big-endian images of the new points straight into the next challenge's feed
  ChunkStats st[5][3];
  {
    const uint8_t* src = resp + 64;
    uint8_t* be = feed.data() + 64;
    for (int id = 2; id <= 6; id++) {
      const size_t psz = Ceremony::psz(id);
      int64_t bad = -1;
      if (const int rc = ptau_points_decompress(device, psz == 128, src, c.cnt[id], sp[id], be, &bad, &st[id - 2][2])) return rc;
      if (bad >= 0) return bad_point("ptau import response", bad, id);
      src += c.cnt[id] * psz / 2;
      be += c.cnt[id] * psz;
    }
  }

  // the record, as contribute builds it
  uint8_t response[64];
  seal_record(c, sp, challenge, feed, 0, params, rec, response);

  // step 2 of verify for this one record, against the record before it or the generators: ONE pairing call
  {
    static const RecordTexts texts = G16_RECORD_TEXTS("ptau import response");
    const bool first = c.rec.empty();
    const uint8_t* cur[3] = {first ? G.g1 : c.rec.back().tau_g1(), first ? G.g1 : c.rec.back().alpha_g1(),
                             first ? G.g1 : c.rec.back().beta_g1()};
    PairChecks checks;
    if (const char* inf = record_checks(texts, R, cur, challenge, checks)) return verdict(inf);
    if (const int rc = checks.run(device)) return rc;
    if (const char* why = checks.first_failure()) return verdict(why);
  }
  memcpy(rec_out, rec, rec_len);
  if (contribution_hash) memcpy(contribution_hash, response, 64);
  static const char* const stages[3] = {nullptr, nullptr, "decompress"};
  trace_points("ptau import response", stages, st, ms_since(t0));
  set_error("");
  *ok = 1;
  z.give(out, out_len);
  return G16_OK;
}

int verify_core(const uint8_t* ptau, size_t len, int device, int* ok) {
  const auto t0 = std::chrono::steady_clock::now();
  *ok = 0;
  Ceremony c;
  if (const int rc = open_ceremony(ptau, len, "ptau verify", c)) return rc;
  const uint8_t* sec[16] = {};
  for (int id = 0; id < 16; id++) sec[id] = c.pv.sec[id].p;
  {
    std::atomic<bool> bad{false};
    for (int id = 2; id <= 6; id++) {
      const uint8_t* s = sec[id];
      const bool g1 = Ceremony::psz(id) == 64;
      parallel_for(c.cnt[id], host_threads(c.cnt[id], kThreadedFrom), [&, s, g1](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi && !bad.load(std::memory_order_relaxed); i++)
          if (!(g1 ? g1_image_ok(s + i * 64) : g2_image_ok(s + i * 128))) bad = true;
      });
    }
    if (bad) return ptau_bad("Invalid File format");
  }
  if (const int rc = require_hip_device("ptau verify", device)) return rc;
  auto verdict = [&](const char* why) { set_error(why); return G16_OK; };
  const Gens& G = gens();

  // 1. the first powers
  if (memcmp(sec[2], G.g1, 64) != 0 || memcmp(sec[3], G.g2, 128) != 0)
    return verdict("ptau verify: the first point of section 2 or 3 is not the generator");

  // 2. the record walk: hashes on the host, the pairs of every same-ratio check collected for ONE device call.  A
  // record's keys are bound to its challenge: the generator file's for the first record, the nextChallenge of the
  // record before for every other.  nextChallenge itself can only be recomputed where the state it hashes is at hand:
  // for the last record, from the file (check 4)
  PairChecks checks;
  static const RecordTexts texts = G16_RECORD_TEXTS("ptau verify");
  const uint8_t* cur[3] = {G.g1, G.g1, G.g1};   // tauG1, alphaG1, betaG1 before the record
  uint8_t challenge[64];
  const char* beacon_fail = nullptr;
  for (size_t i = 0; i < c.rec.size(); i++) {
    if (i == 0) generator_challenge(c, challenge);
    else memcpy(challenge, c.rec[i - 1].next_challenge(), 64);
    if (const char* inf = record_checks(texts, c.rec[i], cur, challenge, checks)) return verdict(inf);
    const PtauRecord& r = c.rec[i];
    if (rd32(r.p + kPtauNextChallengeAt + 64) == 1 && !beacon_fail) {   // a beacon: the keys are what anyone recomputes
      BeaconStated st;
      Fr x[6];
      if (!beacon_params_walk(r.p + kPtauRecordFixed, r.len - kPtauRecordFixed, st)) {
        beacon_fail = "ptau verify: a beacon contribution does not state its beacon";
      } else {
        bool ok = mpc_beacon_scalars(st.hash, st.hash_len, st.exp, 6, x) == G16_OK;
        for (int k = 0; k < 3 && ok; k++) ok = mpc_beacon_key_ok(r.g1_s(k), r.g1_sx(k), x[k], x[3 + k]);
        if (!ok) beacon_fail = "ptau verify: a beacon contribution's key is not the beacon's";
      }
    }
  }

  // 3, 4 (host): a failure here, a beacon's included, is reported after the walk's pairings, and spares the sums of
  // check 5
  const char* host_fail = beacon_fail;
  if (c.rec.empty()) {
    bool gen = true;
    for (int id = 2; id <= 6 && gen; id++)
      for (uint64_t i = 0; i < c.cnt[id] && gen; i++)
        gen = Ceremony::psz(id) == 64 ? memcmp(sec[id] + i * 64, G.g1, 64) == 0 : memcmp(sec[id] + i * 128, G.g2, 128) == 0;
    if (!gen) host_fail = "ptau verify: a file without contributions is not the generator file";
  } else if (!host_fail) {
    const PtauRecord& r = c.rec.back();
    bool same = memcmp(r.alpha_g1(), sec[4], 64) == 0 && memcmp(r.beta_g1(), sec[5], 64) == 0 && memcmp(r.beta_g2(), sec[6], 128) == 0;
    if (c.pv.power >= 1) same = same && memcmp(r.tau_g1(), sec[2] + 64, 64) == 0 && memcmp(r.tau_g2(), sec[3] + 128, 128) == 0;
    if (!same) host_fail = "ptau verify: the file's points are not the last contribution's";
    if (!host_fail) {
      // (challenge = the last record's, from the walk)
      std::vector<uint8_t> feed(64 + c.points_bytes());
      response_hash(challenge, r, feed.data());
      points_be_host(sec, c.cnt, feed.data() + 64);
      uint8_t next[64];
      blake2b512(feed.data(), feed.size(), next);
      if (memcmp(next, r.next_challenge(), 64) != 0) host_fail = "ptau verify: the last contribution's challenge hash does not match the file";
    }
  }

  // 5. the powers: with fresh random rho_i, S1 = sum rho_i P_i, S2 = sum rho_i P_(i+1) must have the ratio tau
  double msm_ms = 0;
  uint64_t msm_points = 0;
  const char* inf_fail = nullptr;
  if (!host_fail && c.pv.power >= 1) {
    static const char* const power_text[6] = {nullptr, nullptr, "ptau verify: section 2 is not the powers of tau",
                                              "ptau verify: section 3 is not the powers of tau",
                                              "ptau verify: section 4 is not alpha times the powers of tau",
                                              "ptau verify: section 5 is not beta times the powers of tau"};
    static const char* const inf_text[6] = {nullptr, nullptr, "ptau verify: the combination of section 2 is the point at infinity",
                                            "ptau verify: the combination of section 3 is the point at infinity",
                                            "ptau verify: the combination of section 4 is the point at infinity",
                                            "ptau verify: the combination of section 5 is the point at infinity"};
    std::vector<uint8_t> rho((c.cnt[2] - 1) * 32);
    if (const int rc = random_fr(rho.data(), c.cnt[2] - 1)) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    const uint8_t *tau_g1 = sec[2] + 64, *tau_g2 = sec[3] + 128;
    for (int id = 2; id <= 5 && !inf_fail; id++) {
      const uint64_t m = c.cnt[id] - 1;
      uint8_t S1[128], S2[128];   // standard form
      if (id != 3) {
        if (const int rc = g16_g1_multiexp(device, sec[id], rho.data(), m, 0, S1)) return rc;
        if (const int rc = g16_g1_multiexp(device, sec[id] + 64, rho.data(), m, 0, S2)) return rc;
        if (all_zero(S1, 64) || all_zero(S2, 64)) { inf_fail = inf_text[id]; break; }
        checks.equal(pair_words(S1), pair_image(tau_g2), pair_words(S2), pair_image(G.g2), power_text[id]);   // e(S1, tauG2) = e(S2, G2)
      } else {
        if (const int rc = g16_g2_multiexp(device, sec[id], rho.data(), m, 0, S1)) return rc;
        if (const int rc = g16_g2_multiexp(device, sec[id] + 128, rho.data(), m, 0, S2)) return rc;
        if (all_zero(S1, 128) || all_zero(S2, 128)) { inf_fail = inf_text[id]; break; }
        checks.equal(pair_image(tau_g1), pair_words(S1), pair_image(G.g1), pair_words(S2), power_text[id]);   // e(tauG1, T1) = e(G1, T2)
      }
      msm_points += 2 * m;
    }
    msm_ms = ms_since(t1);
  }
  const auto t2 = std::chrono::steady_clock::now();
  if (const int rc = checks.run(device)) return rc;
  const double pair_ms = ms_since(t2);
  const uint32_t np = checks.pairs();
  if (getenv("G16_TRACE_HOST"))
    fprintf(stderr, "[g16] ptau verify: power %u, records %zu; MSM %.3f ms (%llu points), pairings %.3f ms (%u); call %.3f ms\n",
            c.pv.power, c.rec.size(), msm_ms, (unsigned long long)msm_points, pair_ms, np, ms_since(t0));
  // (a host failure has spared the sums: every pairing check is then the walk's, and comes first)
  if (const char* why = checks.first_failure()) return verdict(why);
  if (host_fail) return verdict(host_fail);
  if (inf_fail) return verdict(inf_fail);

  // 6. a prepared file: sections 12-15 against a fresh transform of sections 2-5
  int have = 0;
  for (int id = 12; id <= 15; id++) have += sec[id] ? 1 : 0;
  if (have) {
    if (have != 4) return verdict("ptau verify: the prepared sections 12 to 15 are not all present");
    uint8_t* prep = nullptr;
    size_t prep_len = 0;
    if (const int rc = g16_ptau_prepare(ptau, len, device, &prep, &prep_len)) return rc;
    const MallocPtr guard(prep);
    PtauView pp;
    if (const int rc = ptau_open(prep, prep_len, pp, false)) return rc;
    for (int id = 12; id <= 15; id++)
      if (!pp.sec[id].p || pp.sec[id].size != c.pv.sec[id].size || memcmp(pp.sec[id].p, sec[id], pp.sec[id].size) != 0)
        return verdict("ptau verify: the prepared sections are not the transform of sections 2 to 5");
  }
  set_error("");
  *ok = 1;
  return G16_OK;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" int g16_ptau_new(uint32_t power, uint8_t** out, size_t* out_len) {
  if (!out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau new", [&]() { return new_core(power, out, out_len); });
}

extern "C" int g16_ptau_new_file(uint32_t power, const char* path) {
  if (!path) { set_error("NULL argument"); return G16_E_ARG; }
  uint8_t* z = nullptr;
  size_t zl = 0;
  if (const int rc = g16_ptau_new(power, &z, &zl)) return rc;
  return write_key_file(path, z, zl);
}

extern "C" int g16_ptau_contribute(const uint8_t* ptau, size_t ptau_len, const char* name, const uint8_t secret[192], int device,
                                   uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!ptau || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau contribute",
                      [&]() { return contribute_core(ptau, ptau_len, name, secret, nullptr, device, out, out_len, contribution_hash); });
}

extern "C" int g16_ptau_contribute_files(const char* in_path, const char* out_path, const char* name, const uint8_t secret[192],
                                         int device, uint8_t contribution_hash[64]) {
  if (!in_path || !out_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&in_path, 1, out_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_ptau_contribute((const uint8_t*)m[0].p, m[0].len, name, secret, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_ptau_beacon(const uint8_t* ptau, size_t ptau_len, const char* name, const uint8_t* beacon, size_t beacon_len,
                               uint32_t num_iterations_exp, int device, uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!ptau || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  const BeaconArg bc{beacon, beacon_len, num_iterations_exp};
  return no_bad_alloc("ptau beacon",
                      [&]() { return contribute_core(ptau, ptau_len, name, nullptr, &bc, device, out, out_len, contribution_hash); });
}

extern "C" int g16_ptau_beacon_files(const char* in_path, const char* out_path, const char* name, const uint8_t* beacon,
                                     size_t beacon_len, uint32_t num_iterations_exp, int device, uint8_t contribution_hash[64]) {
  if (!in_path || !out_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&in_path, 1, out_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_ptau_beacon((const uint8_t*)m[0].p, m[0].len, name, beacon, beacon_len, num_iterations_exp, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_ptau_export_challenge(const uint8_t* ptau, size_t ptau_len, uint8_t** out, size_t* out_len,
                                         uint8_t challenge_hash[64]) {
  if (!ptau || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau export challenge", [&]() { return export_challenge_core(ptau, ptau_len, out, out_len, challenge_hash); });
}

extern "C" int g16_ptau_export_challenge_files(const char* ptau_path, const char* challenge_path, uint8_t challenge_hash[64]) {
  if (!ptau_path || !challenge_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&ptau_path, 1, challenge_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_ptau_export_challenge((const uint8_t*)m[0].p, m[0].len, z, zl, challenge_hash);
  });
}

extern "C" int g16_ptau_challenge_contribute(const uint8_t* challenge, size_t challenge_len, const uint8_t secret[192], int device,
                                             uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!challenge || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau challenge contribute", [&]() {
    return challenge_contribute_core(challenge, challenge_len, secret, device, out, out_len, contribution_hash);
  });
}

extern "C" int g16_ptau_challenge_contribute_files(const char* challenge_path, const char* response_path, const uint8_t secret[192],
                                                   int device, uint8_t contribution_hash[64]) {
  if (!challenge_path || !response_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&challenge_path, 1, response_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_ptau_challenge_contribute((const uint8_t*)m[0].p, m[0].len, secret, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_ptau_import_response(const uint8_t* ptau, size_t ptau_len, const uint8_t* response, size_t response_len,
                                        const char* name, int device, uint8_t** out, size_t* out_len, uint8_t contribution_hash[64],
                                        int* ok) {
  if (!ptau || !response || !out || !out_len || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau import response", [&]() {
    return import_response_core(ptau, ptau_len, response, response_len, name, device, out, out_len, contribution_hash, ok);
  });
}

extern "C" int g16_ptau_import_response_files(const char* ptau_path, const char* response_path, const char* out_path, const char* name,
                                              int device, uint8_t contribution_hash[64], int* ok) {
  if (!ptau_path || !response_path || !out_path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile old, resp;
  if (const int rc = old.open_ro(ptau_path)) return rc;
  if (const int rc = resp.open_ro(response_path)) return rc;
  uint8_t* z = nullptr;
  size_t zl = 0;
  if (const int rc = g16_ptau_import_response((const uint8_t*)old.p, old.len, (const uint8_t*)resp.p, resp.len, name, device, &z, &zl,
                                              contribution_hash, ok))
    return rc;
  if (!*ok) return G16_OK;   // a verdict: nothing is written, the text stays
  return write_key_file(out_path, z, zl);
}

extern "C" int g16_ptau_verify(const uint8_t* ptau, size_t ptau_len, int device, int* ok) {
  if (!ptau || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau verify", [&]() { return verify_core(ptau, ptau_len, device, ok); });
}

extern "C" int g16_ptau_verify_file(const char* path, int device, int* ok) {
  if (!path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile in;
  if (const int rc = in.open_ro(path)) return rc;
  return g16_ptau_verify((const uint8_t*)in.p, in.len, device, ok);
}

extern "C" int g16_ptau_secret_from_text(const char* text, uint8_t secret[192]) {
  if (!text || !secret) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau secret", [&]() {
    const size_t n = strlen(text);
    std::vector<uint8_t> feed(n + 1);
    memcpy(feed.data(), text, n);
    for (int j = 0; j < 3; j++) {
      uint8_t h[64];
      feed[n] = (uint8_t)j;
      blake2b512(feed.data(), feed.size(), h);
      for (int half = 0; half < 2; half++) {
        Fr x;
        memcpy(x.v, h + 32 * half, 32);
        x = fp_from_mont(fp_to_mont(x));   // (reduces a value >= r)
        if (fp_is_zero(x)) x.v[0] = 1;
        memcpy(secret + 96 * half + 32 * j, x.v, 32);
      }
    }
    return G16_OK;
  });
}
