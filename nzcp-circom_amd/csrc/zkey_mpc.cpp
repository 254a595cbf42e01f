// `snarkjs zkey contribute` and the chain check of `snarkjs zkey verify` for Groth16 keys ([EXT] snarkjs 0.4.12
// zkey_contribute.js, zkey_verify_frominit.js, zkey_utils.js, mpc_applykey.js; ffjavascript chacha.js / random point).
//   contribute: delta <- d delta in the header, sections 8 and 9 <- [1/d] section (zkey_scale.hip), one record more in
//               section 10; everything else byte for byte.
//   verify:     the key is the initial key plus a chain of honest contributions -- the hash chain and the same-ratio
//               pairing checks of every record, and one random linear combination over sections 8 and 9 (two MSMs on
//               the G1 Pippenger, pairings on the verifier's device code); with a .ptau also the ptau leg (snarkjs
//               sectionHasSameRatioH): section 9 is the H basis of THAT ceremony's section 2 scaled by 1 / delta
//               (zkey_verify_h.hip).  The leg reads section 2 only; whether the file is a sound ceremony is
//               `powersoftau verify`'s question.
//   beacon:     a contribution whose d and s anyone recomputes from a public beacon hash and an iteration exponent
//               (beacon.h, mpc_beacon_scalars): a record of type 1 that states both; verify recomputes them for every
//               such record.  The derivation is this library's, as the `-e` rule is: a snarkjs-made beacon record
//               fails that check here.
// The csHash of `zkey new` is built in zkey_cshash_host.cpp (g16_zkey_new; the legacy keys of g16_groth16_setup_ptau
// keep 64 zero bytes); here the chain is hashed from, and compared with, whatever section 10 holds.  The r1cs form of
// verify sets its in-memory initial key up with the real csHash when the key under test carries one.
// The hash is blake2b.cpp, the arithmetic on file images curve_host.cpp, the batch of pairing checks pair_checks.h.
// That the csHash equals snarkjs's own value is NOT claimed (restated without the package), so neither is `snarkjs zkey
// verify` of these keys: the file LAYOUT and the proofs are compatible.
#include "zkey_mpc.h"

#include <algorithm>
#include <chrono>

#include "beacon.h"
#include "host_util.h"
#include "internal.h"
#include "mapped_file.h"
#include "pair_checks.h"
#include "ptau.h"
#include "zkey_cshash.h"

namespace g16 {

// a record's params: byte 1, byte len, the name's UTF-8 bytes cut to 64 characters and to what one length byte can
// hold; nothing without a name
std::string mpc_name_params(const char* name) {
  std::string nm;
  if (name) {
    size_t chars = 0, i = 0;
    const size_t len = strlen(name);
    while (i < len && chars < 64) {
      size_t j = i + 1;
      while (j < len && ((uint8_t)name[j] & 0xc0) == 0x80) j++;
      if (j > 255) break;
      i = j;
      chars++;
    }
    nm.assign(name, i);
  }
  if (nm.empty()) return nm;
  return std::string(1, (char)1) + std::string(1, (char)(uint8_t)nm.size()) + nm;
}

void mpc_hash_pubkey(std::vector<uint8_t>& feed, const MpcRecord& r) {
  const size_t at = feed.size();
  feed.resize(at + 64 + 64 + 64 + 128 + 64);
  uint8_t* q = feed.data() + at;
  g1_uncompressed(r.delta_after(), q);
  g1_uncompressed(r.g1_s(), q + 64);
  g1_uncompressed(r.g1_sx(), q + 128);
  g2_uncompressed(r.g2_spx(), q + 192);
  memcpy(q + 320, r.transcript(), 64);
}

int mpc_parse(const BinSection& s10, MpcSection& out) {
  auto bad = []() { set_error("zkey: Invalid File format"); return G16_E_FORMAT; };
  out = MpcSection{};
  if (!s10.p || s10.size < 68) return bad();
  out.cs_hash = s10.p;
  const uint32_t n = rd32(s10.p + 64);
  uint64_t pos = 68;
  for (uint32_t i = 0; i < n; i++) {
    if (s10.size - pos < kMpcRecordFixed) return bad();
    const uint8_t* r = s10.p + pos;
    const uint32_t plen = rd32(r + kMpcRecordFixed - 4);
    if (s10.size - pos - kMpcRecordFixed < plen) return bad();
    if (!g1_image_ok(r) || !g1_image_ok(r + 64) || !g1_image_ok(r + 128) || !g2_image_ok(r + 192)) return bad();
    out.rec.push_back(MpcRecord{r, kMpcRecordFixed + plen});
    pos += kMpcRecordFixed + plen;
  }
  if (pos != s10.size) return bad();
  return G16_OK;
}

// ------------------------------------------------------------------ the key as the ceremony routes read it
int open_key(const uint8_t* zkey, size_t len, KeyView& k, bool exact_89) {
  auto bad = []() { set_error("zkey: Invalid File format"); return G16_E_FORMAT; };
  if (const int rc = bin_open(zkey, len, "zkey", 2, k.f)) return rc;
  const BinSection& s1 = k.f.sec[1];
  if (!s1.p) return bad();
  if (s1.size < 4 || rd32(s1.p) != 1) { set_error("zkey file is not groth16"); return G16_E_FORMAT; }
  const BinSection& s2 = k.f.sec[2];
  if (!s2.p || s2.size < kHdrEnd || rd32(s2.p) != 32 || rd32(s2.p + 36) != 32) return bad();
  if (!bin_is_field(s2.p, 36, kFqP) || !bin_is_field(s2.p + 36, 36, kFrP)) {
    set_error("Curve not supported: zkey is not over bn128");
    return G16_E_FORMAT;
  }
  k.nVars = rd32(s2.p + 72);
  k.nPublic = rd32(s2.p + 76);
  k.N = rd32(s2.p + 80);
  if (k.N == 0 || (k.N & (k.N - 1)) || (uint64_t)k.nPublic + 1 > (uint64_t)k.nVars) return bad();
  for (int id = 3; id <= 10; id++)
    if (!k.f.sec[id].p) return bad();
  const uint64_t nC = k.nVars - k.nPublic - 1;
  const uint64_t want[10] = {0, 0, 0, ((uint64_t)k.nPublic + 1) * 64, 0, (uint64_t)k.nVars * 64, (uint64_t)k.nVars * 64,
                             (uint64_t)k.nVars * 128, nC * 64, (uint64_t)k.N * 64};
  for (int id = 3; id <= 9; id++) {
    if (id == 4) continue;
    if (id >= 8 && !exact_89 ? k.f.sec[id].size % 64 != 0 : k.f.sec[id].size != want[id]) return bad();
  }
  const BinSection& s4 = k.f.sec[4];
  if (s4.size < 4 || (s4.size - 4) % 44 || (s4.size - 4) / 44 != rd32(s4.p)) return bad();
  const uint8_t* h = s2.p;
  if (!g1_image_ok(h + kHdrDelta1) || !g2_image_ok(h + kHdrDelta2) || all_zero(h + kHdrDelta1, 64) || all_zero(h + kHdrDelta2, 128))
    return bad();
  return mpc_parse(k.f.sec[10], k.mpc);
}

bool key_image_layout(const uint8_t* zkey, const KeyView& k, size_t extra, Buf& z, uint8_t* sp[16]) {
  const uint32_t nsec = rd32(zkey + 8);
  size_t end = 12;   // (bin_open has walked and bounded this table)
  for (uint32_t i = 0; i < nsec; i++) end += 12 + rd64(zkey + end + 4);
  if (!z.reserve(end + extra)) return false;
  z.put(zkey, 12);
  for (int id = 0; id < 16; id++) sp[id] = nullptr;
  for (size_t pos = 12; pos < end;) {
    const uint32_t id = rd32(zkey + pos);
    const uint64_t size = rd64(zkey + pos + 4);
    const uint8_t* p = zkey + pos + 12;
    const bool first = id < 16 && p == k.f.sec[id].p;
    z.u32(id);
    z.u64(first && id == 10 ? size + extra : size);
    uint8_t* q = z.skip(size);
    if (first) sp[id] = q;
    if (!(first && (id == 8 || id == 9))) memcpy(q, p, size);
    if (first && id == 10) z.skip(extra);
    pos += 12 + size;
  }
  return true;
}

int read_secrets(const char* route, const uint8_t* secret, Fr* out, int count) {
  for (int i = 0; i < count; i++) {
    Fr& x = out[i];
    if (secret) {   // standard form, in [1, r)
      memcpy(x.v, secret + 32 * i, 32);
      if (fp_is_zero(x) || !fr_below_modulus(x.v)) {
        set_error(std::string(route) + ": the secret scalars must be in [1, r)");
        return G16_E_ARG;
      }
    } else {
      do {
        if (const int rc = os_random((uint8_t*)x.v, 32)) return rc;
        x.v[7] &= 0x3fffffffu;
      } while (fp_is_zero(x) || !fr_below_modulus(x.v));
    }
  }
  return G16_OK;
}

// The ChaCha20 word stream keyed with the seed as hash_to_g2 keys it, from counter 0; every scalar one next_below(r), a
// zero draw mapped to 1.  count 2 = the first two of count 6: it is one stream.
int mpc_beacon_scalars(const uint8_t* beacon, size_t beacon_len, uint32_t exp, int count, Fr* out) {
  if (count != 2 && count != 6) { set_error("beacon: count must be 2 or 6"); return G16_E_ARG; }
  if (!beacon || beacon_len < 1 || beacon_len > kBeaconHashMax) { set_error("beacon: the beacon hash must be 1 to 255 bytes"); return G16_E_ARG; }
  if (exp < kBeaconExpMin || exp > kBeaconExpMax) { set_error("beacon: numIterationsExp must be between 10 and 63"); return G16_E_ARG; }
  ChaCha rng;
  beacon_chain(beacon, beacon_len, exp, rng.key);
  for (int i = 0; i < count; i++) {
    rng.next_below(kFrP, out[i].v);
    if (fp_is_zero(out[i])) out[i].v[0] = 1;
  }
  return G16_OK;
}

bool mpc_beacon_key_ok(const uint8_t* g1_s, const uint8_t* g1_sx, const Fr& x, const Fr& s) {
  uint8_t want[64];
  mul_image<FqOps>(gens().g1, s, want);
  if (memcmp(want, g1_s, 64) != 0) return false;
  mul_image<FqOps>(want, x, want);
  return memcmp(want, g1_sx, 64) == 0;
}

void mpc_contribution(std::vector<uint8_t>& feed, const Fr& d, const Fr& s, uint8_t g1_s[64], uint8_t g1_sx[64],
                      uint8_t g2_spx[128], uint8_t transcript[64]) {
  mul_image<FqOps>(gens().g1, s, g1_s);
  mul_image<FqOps>(g1_s, d, g1_sx);
  const size_t at = feed.size();
  feed.resize(at + 128);
  g1_uncompressed(g1_s, feed.data() + at);
  g1_uncompressed(g1_sx, feed.data() + at + 64);
  blake2b512(feed.data(), feed.size(), transcript);
  G2Affine sp2;
  hash_to_g2(transcript, sp2);
  mul_image<Fq2Ops>((const uint8_t*)&sp2, d, g2_spx);
}

namespace {

// csHash | hashPubKey of records [0, upto) | g1_s | g1_sx (uncompressed)  ->  the transcript of record `upto`
void transcript_of(const MpcSection& m, size_t upto, const uint8_t* g1_s, const uint8_t* g1_sx, uint8_t out[64]) {
  std::vector<uint8_t> feed(m.cs_hash, m.cs_hash + 64);
  for (size_t i = 0; i < upto; i++) mpc_hash_pubkey(feed, m.rec[i]);
  const size_t at = feed.size();
  feed.resize(at + 128);
  g1_uncompressed(g1_s, feed.data() + at);
  g1_uncompressed(g1_sx, feed.data() + at + 64);
  blake2b512(feed.data(), feed.size(), out);
}

// bc: `zkey beacon` -- the secret is the beacon's (the chain runs here, on this thread, before the device is touched),
// the record is of type 1 and states the beacon after the name; everything else is the contribution's
int contribute_core(const uint8_t* zkey, size_t zkey_len, const char* name, const uint8_t* secret, const BeaconArg* bc, int device,
                    uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  const auto t0 = std::chrono::steady_clock::now();
  const char* route = bc ? "zkey beacon" : "zkey contribute";
  KeyView k;
  if (const int rc = open_key(zkey, zkey_len, k, true)) return rc;
  Fr ds[2];
  if (const int rc = bc ? mpc_beacon_scalars(bc->hash, bc->len, bc->exp, 2, ds) : read_secrets(route, secret, ds, 2)) return rc;
  const Fr &d = ds[0], &s = ds[1];
  if (const int rc = require_hip_device(route, device)) return rc;

  std::string params = mpc_name_params(name);
  if (bc) params += beacon_params(bc->hash, bc->len, bc->exp);
  const uint32_t plen = (uint32_t)params.size();
  const size_t rec_len = kMpcRecordFixed + plen;

  // the image: the input's sections in their order, section 10 one record longer
  Buf z;
  uint8_t* sp[16];
  if (!key_image_layout(zkey, k, rec_len, z, sp)) { set_error(std::string(route) + ": out of memory"); return G16_E_STATE; }

  // host: the contribution's points and the header's delta
  uint8_t* rec = sp[10] + k.f.sec[10].size;
  const uint8_t* hdr = k.f.sec[2].p;
  {
    std::vector<uint8_t> earlier(k.mpc.cs_hash, k.mpc.cs_hash + 64);
    for (const MpcRecord& r : k.mpc.rec) mpc_hash_pubkey(earlier, r);
    mpc_contribution(earlier, d, s, rec + 64, rec + 128, rec + 192, rec + 320);
    mul_image<FqOps>(hdr + kHdrDelta1, d, sp[2] + kHdrDelta1);
    mul_image<Fq2Ops>(hdr + kHdrDelta2, d, sp[2] + kHdrDelta2);
    memcpy(rec, sp[2] + kHdrDelta1, 64);   // deltaAfter
    const uint32_t type = bc ? 1 : 0;
    memcpy(rec + 384, &type, 4);
    memcpy(rec + 388, &plen, 4);
    if (plen) memcpy(rec + 392, params.data(), plen);
    const uint32_t count = (uint32_t)k.mpc.rec.size() + 1;
    memcpy(sp[10] + 64, &count, 4);
    std::vector<uint8_t> feed;
    mpc_hash_pubkey(feed, MpcRecord{rec, rec_len});
    if (contribution_hash) blake2b512(feed.data(), feed.size(), contribution_hash);
  }

  // device: sections 8 and 9 times 1 / d
  const Fr dinv = fp_from_mont(fp_inv(fp_to_mont(d)));
  ChunkStats st[2];
  int rc = zkey_scale_g1(device, k.f.sec[8].p, k.f.sec[8].size / 64, dinv, sp[8], &st[0]);
  if (!rc) rc = zkey_scale_g1(device, k.f.sec[9].p, k.f.sec[9].size / 64, dinv, sp[9], &st[1]);
  if (rc) return rc;
  if (getenv("G16_TRACE_HOST"))
    fprintf(stderr, "[g16] %s: points %llu; kernels %.3f ms, transfers %.3f ms, MSM 0.000 ms, pairings 0.000 ms; call %.3f ms\n",
            route, (unsigned long long)(st[0].points + st[1].points), st[0].kern_ms + st[1].kern_ms, st[0].xfer_ms + st[1].xfer_ms, ms_since(t0));
  z.give(out, out_len);
  return G16_OK;
}

// ---- verify
// ptau != nullptr: the ptau leg as well (step 6): section 9 of the key under test against the first 2N - 1 points of
// the ceremony's section 2 -- prepared or not, no other section of the ptau is read
int verify_core(const uint8_t* init, size_t init_len, const uint8_t* ptau, size_t ptau_len, const uint8_t* zkey, size_t zkey_len,
                int device, int* ok) {
  const auto t0 = std::chrono::steady_clock::now();
  *ok = 0;
  KeyView a, b;   // a = init, b = the key under test
  if (const int rc = open_key(init, init_len, a, true)) return rc;
  if (const int rc = open_key(zkey, zkey_len, b, false)) return rc;
  auto verdict = [&](const char* why) { set_error(why); return G16_OK; };
  PtauView pv;
  int L = 0;   // log2 of the domain of the key under test
  while (((uint32_t)1 << L) < b.N) L++;
  if (ptau) {
    if (const int rc = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/false)) return rc;
    if ((int)pv.power < L) return verdict("zkey verify: the ptau is too small for this key");
    const uint64_t m = 2 * (uint64_t)b.N - 1;
    if (!pv.sec[2].p || pv.sec[2].size / 64 < m) return ptau_bad("Invalid File format");
    for (uint64_t j = 0; j < m; j++)
      if (!g1_image_ok(pv.sec[2].p + j * 64)) return ptau_bad("Invalid File format");
  }
  if (const int rc = require_hip_device("zkey verify", device)) return rc;

  // 1. everything a contribution leaves alone
  const uint8_t *ha = a.f.sec[2].p, *hb = b.f.sec[2].p;
  if (a.nVars != b.nVars || a.nPublic != b.nPublic || a.N != b.N || memcmp(ha, hb, kHdrDelta1) != 0)
    return verdict("zkey verify: the header differs from the initial key's (sizes, alpha, beta or gamma)");
  for (int id = 3; id <= 7; id++)
    if (a.f.sec[id].size != b.f.sec[id].size || memcmp(a.f.sec[id].p, b.f.sec[id].p, a.f.sec[id].size) != 0)
      return verdict("zkey verify: sections 3 to 7 differ from the initial key's");
  if (memcmp(a.mpc.cs_hash, b.mpc.cs_hash, 64) != 0) return verdict("zkey verify: the circuit hash differs from the initial key's");
  // 2. the initial key's own records
  if (b.mpc.rec.size() < a.mpc.rec.size()) return verdict("zkey verify: the contributions do not begin with the initial key's");
  for (size_t i = 0; i < a.mpc.rec.size(); i++)
    if (a.mpc.rec[i].len != b.mpc.rec[i].len || memcmp(a.mpc.rec[i].p, b.mpc.rec[i].p, a.mpc.rec[i].len) != 0)
      return verdict("zkey verify: the contributions do not begin with the initial key's");
  // 5 (lengths first: host checks before the device)
  if (a.f.sec[8].size != b.f.sec[8].size || a.f.sec[9].size != b.f.sec[9].size)
    return verdict("zkey verify: section 8 or 9 has not the initial key's length");

  // 3. the chain: hashes on the host, the pairs of every same-ratio check collected for ONE device call
  PairChecks checks;
  auto same_ratio = [&](const uint8_t* g1a, const uint8_t* g1b, const uint8_t* g2c, const uint8_t* g2d, const char* why) {
    if (all_zero(g1a, 64) || all_zero(g1b, 64) || all_zero(g2c, 128) || all_zero(g2d, 128)) return false;
    checks.same_ratio(g1a, g1b, g2c, g2d, why);
    return true;
  };
  const char* inf_text = "zkey verify: a contribution holds the point at infinity";
  const uint8_t* cur = ha + kHdrDelta1;
  const char* beacon_fail = nullptr;   // reported after the pairing checks: a beacon record passes its own checks first
  for (size_t i = a.mpc.rec.size(); i < b.mpc.rec.size(); i++) {
    const MpcRecord& r = b.mpc.rec[i];
    uint8_t tr[64];
    transcript_of(b.mpc, i, r.g1_s(), r.g1_sx(), tr);
    if (memcmp(tr, r.transcript(), 64) != 0) return verdict("zkey verify: a contribution's transcript hash does not match");
    G2Affine g2_sp;
    hash_to_g2(tr, g2_sp);
    const uint8_t* sp2 = (const uint8_t*)&g2_sp;
    if (!same_ratio(r.g1_s(), r.g1_sx(), sp2, r.g2_spx(), "zkey verify: a contribution's public key is not consistent")) return verdict(inf_text);
    if (!same_ratio(cur, r.delta_after(), sp2, r.g2_spx(), "zkey verify: a contribution's delta does not continue the chain")) return verdict(inf_text);
    cur = r.delta_after();
    if (rd32(r.p + 384) == 1 && !beacon_fail) {   // a beacon: the key is what anyone recomputes from the stated beacon
      BeaconStated st;
      Fr ds[2];
      if (!beacon_params_walk(r.p + kMpcRecordFixed, r.len - kMpcRecordFixed, st))
        beacon_fail = "zkey verify: a beacon contribution does not state its beacon";
      else if (mpc_beacon_scalars(st.hash, st.hash_len, st.exp, 2, ds) || !mpc_beacon_key_ok(r.g1_s(), r.g1_sx(), ds[0], ds[1]))
        beacon_fail = "zkey verify: a beacon contribution's key is not the beacon's";
    }
  }
  // 4. the header's delta
  if (memcmp(cur, hb + kHdrDelta1, 64) != 0) return verdict("zkey verify: delta1 of the header is not the last contribution's");
  if (!same_ratio(ha + kHdrDelta1, hb + kHdrDelta1, ha + kHdrDelta2, hb + kHdrDelta2, "zkey verify: delta2 does not match delta1"))
    return verdict(inf_text);

  // 5. sections 8 and 9: S = sum rho_i new_i, T = sum rho_i init_i, e(S, delta2) = e(T, delta2 of init).  Section 8
  // takes fully random rho.  Section 9 takes rho9[i] = (1/N) sum_k u[k] w^((2i+1) k) with u random and u[N-1] = 0, formed
  // on the device as the ptau leg forms it (zkey_verify_h.hip): the combinations sum e_i S9[i] of quotients of degree <=
  // N - 2, which are all a prover ever forms and all the MPCParams exchange carries (`zkey import bellman` writes the
  // projection of section 9 onto them: zkey_bellman.hip).  The infinity patterns are compared for section 8 alone -- the
  // projection moves section 9's.
  const uint64_t n8 = a.f.sec[8].size / 64, n9 = a.f.sec[9].size / 64, n = n8 + n9;
  double msm_ms = 0;
  uint8_t S[64], T[64];   // standard form
  {
    std::vector<uint8_t> bases_new(n * 64), bases_init(n * 64), rho(n * 32);
    memcpy(bases_init.data(), a.f.sec[8].p, n8 * 64);
    memcpy(bases_init.data() + n8 * 64, a.f.sec[9].p, n9 * 64);
    memcpy(bases_new.data(), b.f.sec[8].p, n8 * 64);
    memcpy(bases_new.data() + n8 * 64, b.f.sec[9].p, n9 * 64);
    for (uint64_t i = 0; i < n; i++) {
      if (!g1_image_ok(bases_new.data() + i * 64)) { set_error("zkey: Invalid File format"); return G16_E_FORMAT; }
      if (i < n8 && all_zero(bases_new.data() + i * 64, 64) != all_zero(bases_init.data() + i * 64, 64))
        return verdict("zkey verify: sections 8 and 9 are not the initial key's scaled by 1 / delta");
    }
    ChaCha rng;   // fresh scalars: a ChaCha20 stream keyed from the OS CSPRNG
    if (const int rc = os_random((uint8_t*)rng.key, 32)) return rc;
    for (uint64_t i = 0; i < n8; i++) rng.next_below(kFrP, (uint32_t*)(rho.data() + i * 32));
    if (L >= 1) {   // (a domain of one point has no quotient: rho9 = 0)
      std::vector<uint8_t> u(n9 * 32, 0);   // u[N-1] = 0
      for (uint64_t k = 0; k + 1 < n9; k++) rng.next_below(kFrP, (uint32_t*)(u.data() + k * 32));
      if (const int rc = zkey_h_rho(device, u.data(), L, rho.data() + n8 * 32)) return rc;
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (const int rc = g16_g1_multiexp(device, bases_new.data(), rho.data(), n, 0, S)) return rc;
    if (const int rc = g16_g1_multiexp(device, bases_init.data(), rho.data(), n, 0, T)) return rc;
    msm_ms = ms_since(t1);
  }
  const bool s_inf = all_zero(S, 64);
  if (!s_inf) {
    if (all_zero(T, 64)) return verdict("zkey verify: sections 8 and 9 are not the initial key's scaled by 1 / delta");
    checks.equal(pair_words(S), pair_image(hb + kHdrDelta2), pair_words(T), pair_image(ha + kHdrDelta2),
                 "zkey verify: sections 8 and 9 are not the initial key's scaled by 1 / delta");
  } else if (n8 || L >= 1) {   // (some scalar was drawn)
    return verdict("zkey verify: the combination of sections 8 and 9 is the point at infinity");
  }
  // 6. the ptau leg: S = sum rho_i new9_i, T = sum t_j tauG1_j with both scalar vectors formed on the device from one
  // draw u (zkey_verify_h.hip; rho keeps 1 / 2N, so S is multiplied by 2N here): e(2N S, delta2) = e(T, G2), or both
  // sums the point at infinity (the tau = 1 ceremony).  A domain of one point has no H relation to check.
  ZkeyHStats hst;
  const bool leg = ptau && L >= 1;
  if (leg) {
    const char* h_text = "zkey verify: section 9 is not the ceremony's H basis scaled by 1 / delta";
    std::vector<uint8_t> u((size_t)b.N * 32, 0);   // u[N-1] = 0
    ChaCha rng;
    if (const int rc = os_random((uint8_t*)rng.key, 32)) return rc;
    for (uint32_t k = 0; k + 1 < b.N; k++) rng.next_below(kFrP, (uint32_t*)(u.data() + (size_t)k * 32));
    uint8_t Sh[64], Th[64];   // standard form
    if (const int rc = zkey_verify_h(device, u.data(), L, b.f.sec[9].p, pv.sec[2].p, Sh, Th, &hst)) return rc;
    const bool sh_inf = all_zero(Sh, 64);
    if (sh_inf != all_zero(Th, 64)) return verdict(h_text);
    if (!sh_inf) {
      G1Affine s, s2n;
      memcpy(&s, Sh, 64);
      s.x = fp_to_mont(s.x); s.y = fp_to_mont(s.y);
      Fr two_n = fp_zero<FrParams>();
      two_n.v[0] = 2 * b.N;   // L <= 27
      mul_image<FqOps>((const uint8_t*)&s, two_n, (uint8_t*)&s2n);
      checks.equal(pair_image((const uint8_t*)&s2n), pair_image(hb + kHdrDelta2), pair_words(Th), pair_image(gens().g2), h_text);
    }
  }
  const auto t2 = std::chrono::steady_clock::now();
  if (const int rc = checks.run(device)) return rc;
  const double pair_ms = ms_since(t2);
  const uint32_t np = checks.pairs();
  if (getenv("G16_TRACE_HOST")) {
    if (leg)
      fprintf(stderr, "[g16] zkey verify: points %llu; kernels 0.000 ms, transfers 0.000 ms, MSM %.3f ms, pairings %.3f ms (%u); "
              "ptau leg: points %llu, NTT %.3f ms, MSM %.3f ms; call %.3f ms\n",
              (unsigned long long)n, msm_ms, pair_ms, np, 3 * (unsigned long long)b.N - 1, hst.ntt_ms, hst.msm_ms, ms_since(t0));
    else
      fprintf(stderr, "[g16] zkey verify: points %llu; kernels 0.000 ms, transfers 0.000 ms, MSM %.3f ms, pairings %.3f ms (%u); call %.3f ms\n",
              (unsigned long long)n, msm_ms, pair_ms, np, ms_since(t0));
  }
  if (const char* why = checks.first_failure()) return verdict(why);
  if (beacon_fail) return verdict(beacon_fail);
  set_error("");
  *ok = 1;
  return G16_OK;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_contribute(const uint8_t* zkey, size_t zkey_len, const char* name, const uint8_t secret[64], int device,
                                   uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!zkey || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey contribute",
                      [&]() { return contribute_core(zkey, zkey_len, name, secret, nullptr, device, out, out_len, contribution_hash); });
}

extern "C" int g16_zkey_contribute_files(const char* in_path, const char* out_path, const char* name, const uint8_t secret[64],
                                         int device, uint8_t contribution_hash[64]) {
  if (!in_path || !out_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&in_path, 1, out_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_zkey_contribute((const uint8_t*)m[0].p, m[0].len, name, secret, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_zkey_beacon(const uint8_t* zkey, size_t zkey_len, const char* name, const uint8_t* beacon, size_t beacon_len,
                               uint32_t num_iterations_exp, int device, uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!zkey || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  const BeaconArg bc{beacon, beacon_len, num_iterations_exp};
  return no_bad_alloc("zkey beacon",
                      [&]() { return contribute_core(zkey, zkey_len, name, nullptr, &bc, device, out, out_len, contribution_hash); });
}

extern "C" int g16_zkey_beacon_files(const char* in_path, const char* out_path, const char* name, const uint8_t* beacon,
                                     size_t beacon_len, uint32_t num_iterations_exp, int device, uint8_t contribution_hash[64]) {
  if (!in_path || !out_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&in_path, 1, out_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_zkey_beacon((const uint8_t*)m[0].p, m[0].len, name, beacon, beacon_len, num_iterations_exp, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_beacon_scalars(const uint8_t* beacon, size_t beacon_len, uint32_t num_iterations_exp, int count, uint8_t* out) {
  if (!out) { set_error("NULL argument"); return G16_E_ARG; }
  Fr x[6];
  if (const int rc = mpc_beacon_scalars(beacon, beacon_len, num_iterations_exp, count, x)) return rc;
  memcpy(out, x, (size_t)count * 32);
  return G16_OK;
}

extern "C" int g16_zkey_verify_from_init(const uint8_t* init, size_t init_len, const uint8_t* zkey, size_t zkey_len, int device,
                                         int* ok) {
  if (!init || !zkey || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey verify", [&]() { return verify_core(init, init_len, nullptr, 0, zkey, zkey_len, device, ok); });
}

extern "C" int g16_zkey_verify_from_init_files(const char* init_path, const char* zkey_path, int device, int* ok) {
  if (!init_path || !zkey_path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile in[2];
  if (const int rc = in[0].open_ro(init_path)) return rc;
  if (const int rc = in[1].open_ro(zkey_path)) return rc;
  return g16_zkey_verify_from_init((const uint8_t*)in[0].p, in[0].len, (const uint8_t*)in[1].p, in[1].len, device, ok);
}

extern "C" int g16_zkey_verify_from_init_ptau(const uint8_t* init, size_t init_len, const uint8_t* ptau, size_t ptau_len,
                                              const uint8_t* zkey, size_t zkey_len, int device, int* ok) {
  if (!init || !ptau || !zkey || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey verify", [&]() { return verify_core(init, init_len, ptau, ptau_len, zkey, zkey_len, device, ok); });
}

extern "C" int g16_zkey_verify_from_init_ptau_files(const char* init_path, const char* ptau_path, const char* zkey_path,
                                                    int device, int* ok) {
  if (!init_path || !ptau_path || !zkey_path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile in[3];
  if (const int rc = in[0].open_ro(init_path)) return rc;
  if (const int rc = in[1].open_ro(ptau_path)) return rc;
  if (const int rc = in[2].open_ro(zkey_path)) return rc;
  return g16_zkey_verify_from_init_ptau((const uint8_t*)in[0].p, in[0].len, (const uint8_t*)in[1].p, in[1].len,
                                        (const uint8_t*)in[2].p, in[2].len, device, ok);
}

// `snarkjs zkey verify c.r1cs pot.ptau c.zkey`: the initial key is set up again in memory (g16_groth16_setup_ptau, which
// needs the prepared sections), then the route above
extern "C" int g16_zkey_verify_r1cs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                                    const uint8_t* zkey, size_t zkey_len, int device, int* ok) {
  if (!r1cs || !ptau || !zkey || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  *ok = 0;
  uint8_t* init = nullptr;
  size_t init_len = 0;
  if (const int rc = g16_groth16_setup_ptau(r1cs, r1cs_len, ptau, ptau_len, device, &init, &init_len)) return rc;
  const MallocPtr guard(init);
  // A key that carries a circuit hash (anything but the legacy 64 zero bytes) is held against the initial key WITH its
  // real csHash.  Only where that can matter: the key parses and has the initial key's domain -- every other input
  // gets its error or verdict from the route below before section 10 is compared, exactly as without this step; and
  // with the same domain the hash's checks of the ptau are the ones the route below makes at the same point.
  const int rc = no_bad_alloc("zkey verify", [&]() -> int {
    KeyView a, b;
    if (open_key(zkey, zkey_len, b, false) != G16_OK || all_zero(b.mpc.cs_hash, 64)) return G16_OK;
    if (const int rc2 = open_key(init, init_len, a, true)) return rc2;
    if (a.N != b.N || a.N > ((uint32_t)1 << 24)) return G16_OK;
    PtauView pv;
    if (const int rc2 = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/false)) return rc2;
    int L = 0;
    while (((uint32_t)1 << L) < a.N) L++;
    if ((int)pv.power < L) return G16_OK;   // (the route below has the verdict)
    if (const int rc2 = cshash_check_ptau(pv, L)) return rc2;
    uint8_t h[64];
    if (const int rc2 = zkey_cs_hash_core(a, pv, device, h)) return rc2;
    memcpy(init + (a.mpc.cs_hash - init), h, 64);
    return G16_OK;
  });
  if (rc) return rc;
  return g16_zkey_verify_from_init_ptau(init, init_len, ptau, ptau_len, zkey, zkey_len, device, ok);
}

extern "C" int g16_zkey_verify_r1cs_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                                          int* ok) {
  if (!r1cs_path || !ptau_path || !zkey_path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile in[3];
  if (const int rc = in[0].open_ro(r1cs_path)) return rc;
  if (const int rc = in[1].open_ro(ptau_path)) return rc;
  if (const int rc = in[2].open_ro(zkey_path)) return rc;
  return g16_zkey_verify_r1cs((const uint8_t*)in[0].p, in[0].len, (const uint8_t*)in[1].p, in[1].len, (const uint8_t*)in[2].p,
                              in[2].len, device, ok);
}
