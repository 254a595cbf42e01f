// `snarkjs zkey export bellman`, `zkey bellman contribute`, `zkey import bellman` for Groth16 keys ([EXT] snarkjs 0.4.12
// zkey_export_bellman.js, zkey_bellman_contribute.js, zkey_import_bellman.js, restated from their description; the
// layout is in zkey_bellman.h): how somebody who does not hold the .zkey contributes to phase 2.
//   export:     the key's points as an MPCParams image.  H = T[0 .. N-2] of the forward basis change of section 9
//               (zkey_bellman.hip), every run through the to-be stage of ptau_points.hip.  A record's type and params
//               are not carried: the format has no room for them.
//   contribute: delta <- d delta; H and L from-be -> [1/d] (zkey_scale.hip) -> to-be; one record more, formed as
//               g16_zkey_contribute forms it (mpc_contribution), so the same (d, s) gives the same record and hash
//               through either route; everything else byte for byte.
//   import:     old key + response -> new key: sections 1, 3-7 and the header up to delta1 from the old key, delta1 and
//               delta2 from the file, section 8 through from-be, section 9 through the inverse basis change (infinity at
//               k = N - 1: the file drops T[N-1]), section 10 = the old records as they are, then the file's new ones
//               with type 0 and the name's params.  import(export(key)) is the PROJECTION of section 9 onto the
//               quotients of degree <= N - 2, not the identity: same proofs, other bytes, idempotent.  Whether the
//               contribution is honest is `zkey verify`'s question, as in snarkjs.
// Checks that need no point arithmetic run before the device is asked for; there is no CPU path for the rest.
// NOT claimed: an exchange with a snarkjs or bellman contributor (the files are restated without the package at hand,
// and csHash -- carried as section 10 holds it: g16_zkey_new's circuit hash, zkey_cshash_host.cpp, or the 64 zero bytes
// of a legacy _0000 key -- is not claimed to equal snarkjs's value).
#include "zkey_bellman.h"

#include <chrono>

#include "host_util.h"
#include "internal.h"
#include "mapped_file.h"
#include "zkey_mpc.h"

namespace g16 {
namespace {

int mp_bad() { set_error("mpcparams: Invalid File format"); return G16_E_FORMAT; }
uint32_t rd32be(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void wr32be(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// flags and coordinates of an uncompressed big-endian image: a clean 0x40 with nothing else, or every coordinate < q
bool be_plausible(const uint8_t* p, size_t psz) {
  static const struct QBe {
    uint8_t b[32];
    QBe() { for (int i = 0; i < 8; i++) wr32be(b + 4 * i, kFqP[7 - i]); }
  } q;
  if (p[0] & 0xc0) return p[0] == 0x40 && all_zero(p + 1, psz - 1);
  for (size_t c = 0; c < psz; c += 32)
    if (memcmp(p + c, q.b, 32) >= 0) return false;
  return true;
}
bool be_run_plausible(const uint8_t* p, uint64_t n, size_t psz) {
  for (uint64_t i = 0; i < n; i++)
    if (!be_plausible(p + i * psz, psz)) return false;
  return true;
}

int log2_domain(const char* route, uint32_t N, int& L) {
  L = 0;
  while (((uint32_t)1 << L) < N) L++;
  if (L > 24) { set_error(std::string(route) + ": the domain is above 2^24"); return G16_E_ARG; }
  return G16_OK;
}

// a key's record as the MPCParams file holds it: its hashPubKey feed
void record_image(const MpcRecord& r, uint8_t out[kMpRecord]) {
  g1_uncompressed(r.delta_after(), out);
  g1_uncompressed(r.g1_s(), out + 64);
  g1_uncompressed(r.g1_sx(), out + 128);
  g2_uncompressed(r.g2_spx(), out + 192);
  memcpy(out + 320, r.transcript(), 64);
}
void header_image(const uint8_t* h, uint8_t out[kMpHeader]) {   // h = section 2
  g1_uncompressed(h + kHdrAlpha1, out);
  g1_uncompressed(h + kHdrAlpha1 + 64, out + 64);
  g2_uncompressed(h + kHdrAlpha1 + 128, out + 128);
  g2_uncompressed(h + kHdrAlpha1 + 256, out + 256);
  g1_uncompressed(h + kHdrDelta1, out + kMpDelta1);
  g2_uncompressed(h + kHdrDelta2, out + kMpDelta2);
}
void key_counts(const KeyView& k, uint32_t cnt[kMpRuns]) {
  cnt[0] = k.nPublic + 1; cnt[1] = k.N - 1; cnt[2] = k.nVars - k.nPublic - 1;
  cnt[3] = cnt[4] = cnt[5] = k.nVars;
}

int export_core(const uint8_t* zkey, size_t len, int device, uint8_t** out, size_t* out_len) {
  const auto t0 = std::chrono::steady_clock::now();
  KeyView k;
  if (const int rc = open_key(zkey, len, k, true)) return rc;
  int L;
  if (const int rc = log2_domain("zkey export bellman", k.N, L)) return rc;
  if (const int rc = require_hip_device("zkey export bellman", device)) return rc;

  uint32_t cnt[kMpRuns];
  key_counts(k, cnt);
  size_t total = kMpHeader + 64 + 4 + k.mpc.rec.size() * kMpRecord;
  for (int r = 0; r < kMpRuns; r++) total += 4 + (size_t)cnt[r] * kMpRunPoint[r];
  Buf z;
  if (!z.reserve(total)) { set_error("zkey export bellman: out of memory"); return G16_E_STATE; }
  header_image(k.f.sec[2].p, z.skip(kMpHeader));

  std::vector<uint8_t> t((size_t)k.N * 64);
  ZkeyBasisStats bst;
  if (const int rc = zkey_h_basis(device, k.f.sec[9].p, L, /*inverse=*/false, t.data(), &bst)) return rc;
  const uint8_t* src[kMpRuns] = {k.f.sec[3].p, t.data(), k.f.sec[8].p, k.f.sec[5].p, k.f.sec[6].p, k.f.sec[7].p};
  ChunkStats st[kMpRuns];
  for (int r = 0; r < kMpRuns; r++) {
    wr32be(z.skip(4), cnt[r]);
    uint8_t* q = z.skip((size_t)cnt[r] * kMpRunPoint[r]);
    if (const int rc = ptau_points_to_be(device, kMpRunPoint[r] == 128, src[r], cnt[r], q, &st[r])) return rc;
  }
  z.put(k.mpc.cs_hash, 64);
  wr32be(z.skip(4), (uint32_t)k.mpc.rec.size());
  for (const MpcRecord& r : k.mpc.rec) record_image(r, z.skip(kMpRecord));
  if (getenv("G16_TRACE_HOST")) {
    float kern = 0, xfer = 0;
    for (const ChunkStats& s : st) { kern += s.kern_ms; xfer += s.xfer_ms; }
    fprintf(stderr, "[g16] zkey export bellman: basis %.3f ms (%llu products), to-be %.3f ms, transfers %.3f ms; call %.3f ms\n",
            bst.kern_ms, (unsigned long long)bst.muls, kern, xfer, ms_since(t0));
  }
  z.give(out, out_len);
  return G16_OK;
}

int contribute_core(const uint8_t* ch, size_t len, const uint8_t* secret, int device, uint8_t** out, size_t* out_len,
                    uint8_t contribution_hash[64]) {
  const auto t0 = std::chrono::steady_clock::now();
  MpView m;
  if (const int rc = mp_open(ch, len, m)) return rc;
  Fr ds[2];
  if (const int rc = read_secrets("zkey bellman contribute", secret, ds, 2)) return rc;
  const Fr &d = ds[0], &s = ds[1];
  uint8_t delta1[64], delta2[128];
  if (!image_from_be(m.hdr + kMpDelta1, 64, delta1) || !image_from_be(m.hdr + kMpDelta2, 128, delta2) ||
      all_zero(delta1, 64) || all_zero(delta2, 128))
    return mp_bad();
  if (const int rc = require_hip_device("zkey bellman contribute", device)) return rc;

  Buf z;
  if (!z.reserve(len + kMpRecord)) { set_error("zkey bellman contribute: out of memory"); return G16_E_STATE; }
  z.put(ch, len);
  uint8_t* rec = z.skip(kMpRecord);
  auto at = [&](const uint8_t* p) { return z.p + (p - ch); };   // the same place in the output

  // host: delta and the record
  {
    uint8_t nd1[64], nd2[128], g1_s[64], g1_sx[64], g2_spx[128];
    mul_image<FqOps>(delta1, d, nd1);
    mul_image<Fq2Ops>(delta2, d, nd2);
    g1_uncompressed(nd1, at(m.hdr + kMpDelta1));
    g2_uncompressed(nd2, at(m.hdr + kMpDelta2));
    std::vector<uint8_t> feed(m.cs_hash, m.cs_hash + 64);
    feed.insert(feed.end(), m.rec, m.rec + (size_t)m.nrec * kMpRecord);
    mpc_contribution(feed, d, s, g1_s, g1_sx, g2_spx, rec + 320);
    g1_uncompressed(nd1, rec);
    g1_uncompressed(g1_s, rec + 64);
    g1_uncompressed(g1_sx, rec + 128);
    g2_uncompressed(g2_spx, rec + 192);
    wr32be(at(m.cs_hash + 64), m.nrec + 1);
    if (contribution_hash) blake2b512(rec, kMpRecord, contribution_hash);
  }

  // device: H and L times 1 / d
  const Fr dinv = fp_from_mont(fp_inv(fp_to_mont(d)));
  ChunkStats st[2][3];
  std::vector<uint8_t> a((size_t)std::max(m.cnt[1], m.cnt[2]) * 64), b(a.size());
  for (int r = 1; r <= 2; r++) {
    int64_t bad = -1;
    if (const int rc = ptau_points_from_be(device, false, m.run[r], m.cnt[r], a.data(), &bad, &st[r - 1][0])) return rc;
    if (bad >= 0) return mp_bad();
    if (const int rc = zkey_scale_g1(device, a.data(), m.cnt[r], dinv, b.data(), &st[r - 1][1])) return rc;
    if (const int rc = ptau_points_to_be(device, false, b.data(), m.cnt[r], at(m.run[r]), &st[r - 1][2])) return rc;
  }
  if (getenv("G16_TRACE_HOST")) {
    float ms[3] = {0, 0, 0}, xfer = 0;
    for (int r = 0; r < 2; r++)
      for (int j = 0; j < 3; j++) { ms[j] += st[r][j].kern_ms; xfer += st[r][j].xfer_ms; }
    fprintf(stderr, "[g16] zkey bellman contribute: points %llu; kernels from-be %.3f ms, scale %.3f ms, to-be %.3f ms, transfers %.3f ms; call %.3f ms\n",
            (unsigned long long)m.cnt[1] + m.cnt[2], ms[0], ms[1], ms[2], xfer, ms_since(t0));
  }
  z.give(out, out_len);
  return G16_OK;
}

int import_core(const uint8_t* old, size_t old_len, const uint8_t* resp, size_t rlen, const char* name, int device, uint8_t** out,
                size_t* out_len, int* ok) {
  const auto t0 = std::chrono::steady_clock::now();
  *ok = 0;
  *out = nullptr;
  *out_len = 0;
  KeyView k;
  if (const int rc = open_key(old, old_len, k, true)) return rc;
  int L;
  if (const int rc = log2_domain("zkey import bellman", k.N, L)) return rc;
  MpView m;
  if (const int rc = mp_open(resp, rlen, m)) return rc;
  auto verdict = [&](const char* why) { set_error(why); return G16_OK; };
  static const char* const kSameText = "zkey import bellman: alpha, beta, gamma, IC, A, B1 or B2 differ from the key's";

  // host: what needs no point arithmetic
  uint32_t cnt[kMpRuns];
  key_counts(k, cnt);
  for (int r = 0; r < kMpRuns; r++)
    if (m.cnt[r] != cnt[r]) return verdict("zkey import bellman: a count is not the key's");
  const uint8_t* hdr = k.f.sec[2].p;
  {
    uint8_t h[kMpHeader];
    header_image(hdr, h);
    if (memcmp(h, m.hdr, kMpDelta1) != 0) return verdict(kSameText);
  }
  if (memcmp(m.cs_hash, k.mpc.cs_hash, 64) != 0) return verdict("zkey import bellman: the circuit hash differs from the key's");
  const size_t nold = k.mpc.rec.size();
  if (m.nrec <= nold) return verdict("zkey import bellman: the response holds no new contribution");
  for (size_t i = 0; i < nold; i++) {
    uint8_t r[kMpRecord];
    record_image(k.mpc.rec[i], r);
    if (memcmp(r, m.rec + i * kMpRecord, kMpRecord) != 0) return verdict("zkey import bellman: the contributions do not begin with the key's");
  }
  if ((m.hdr[kMpDelta1] & 0x40) || (m.hdr[kMpDelta2] & 0x40)) return verdict("zkey import bellman: delta1 or delta2 is the point at infinity");

  // host: the few points the key takes as they are -- delta and the new records
  uint8_t delta1[64], delta2[128];
  if (!image_from_be(m.hdr + kMpDelta1, 64, delta1) || !image_from_be(m.hdr + kMpDelta2, 128, delta2)) return mp_bad();
  const std::string params = mpc_name_params(name);
  const uint32_t plen = (uint32_t)params.size();
  const size_t rec_len = kMpcRecordFixed + plen, nnew = m.nrec - nold;
  std::vector<uint8_t> recs(nnew * rec_len);
  for (size_t i = 0; i < nnew; i++) {
    const uint8_t* r = m.rec + (nold + i) * kMpRecord;
    uint8_t* q = recs.data() + i * rec_len;
    if (!image_from_be(r, 64, q) || !image_from_be(r + 64, 64, q + 64) || !image_from_be(r + 128, 64, q + 128) ||
        !image_from_be(r + 192, 128, q + 192))
      return mp_bad();
    memcpy(q + 320, r + 320, 64);
    const uint32_t type = 0;
    memcpy(q + 384, &type, 4);
    memcpy(q + 388, &plen, 4);
    if (plen) memcpy(q + 392, params.data(), plen);
  }
  if (const int rc = require_hip_device("zkey import bellman", device)) return rc;

  // device: the runs the key must already hold, checked as any stranger's points and compared
  ChunkStats st[kMpRuns];
  {
    static const int same[4][2] = {{0, 3}, {3, 5}, {4, 6}, {5, 7}};   // run, section
    std::vector<uint8_t> tmp;
    for (const auto& rs : same) {
      const int r = rs[0];
      const BinSection& sec = k.f.sec[rs[1]];
      tmp.resize(std::max<size_t>(sec.size, 1));
      int64_t bad = -1;
      if (const int rc = ptau_points_from_be(device, kMpRunPoint[r] == 128, m.run[r], m.cnt[r], tmp.data(), &bad, &st[r])) return rc;
      if (bad >= 0) return mp_bad();
      if (memcmp(tmp.data(), sec.p, sec.size) != 0) return verdict(kSameText);
    }
  }

  // the image: the old key's sections in their order, section 10 longer by the new records
  Buf z;
  uint8_t* sp[16];
  if (!key_image_layout(old, k, recs.size(), z, sp)) { set_error("zkey import bellman: out of memory"); return G16_E_STATE; }
  memcpy(sp[10] + k.f.sec[10].size, recs.data(), recs.size());
  memcpy(sp[2] + kHdrDelta1, delta1, 64);
  memcpy(sp[2] + kHdrDelta2, delta2, 128);
  memcpy(sp[10] + 64, &m.nrec, 4);

  // device: section 8 as it comes, section 9 through the inverse basis change (T[N-1] = infinity)
  {
    int64_t bad = -1;
    if (const int rc = ptau_points_from_be(device, false, m.run[2], m.cnt[2], sp[8], &bad, &st[2])) return rc;
    if (bad >= 0) return mp_bad();
  }
  ZkeyBasisStats bst;
  {
    std::vector<uint8_t> t((size_t)k.N * 64, 0);
    int64_t bad = -1;
    if (const int rc = ptau_points_from_be(device, false, m.run[1], m.cnt[1], t.data(), &bad, &st[1])) return rc;
    if (bad >= 0) return mp_bad();
    if (const int rc = zkey_h_basis(device, t.data(), L, /*inverse=*/true, sp[9], &bst)) return rc;
  }
  if (getenv("G16_TRACE_HOST")) {
    float kern = 0, xfer = 0;
    for (const ChunkStats& s : st) { kern += s.kern_ms; xfer += s.xfer_ms; }
    fprintf(stderr, "[g16] zkey import bellman: basis %.3f ms (%llu products), from-be %.3f ms, transfers %.3f ms; call %.3f ms\n",
            bst.kern_ms, (unsigned long long)bst.muls, kern, xfer, ms_since(t0));
  }
  set_error("");
  *ok = 1;
  z.give(out, out_len);
  return G16_OK;
}

}  // namespace

void mp_header_image(const uint8_t* sec2, uint8_t out[kMpHeader]) { header_image(sec2, out); }
void mp_key_counts(uint32_t nVars, uint32_t nPublic, uint32_t N, uint32_t cnt[kMpRuns]) {
  KeyView k;
  k.nVars = nVars; k.nPublic = nPublic; k.N = N;
  key_counts(k, cnt);
}

int mp_open(const uint8_t* p, size_t len, MpView& m) {
  m = MpView{};
  if (!p || len < kMpHeader) return mp_bad();
  m.hdr = p;
  size_t pos = kMpHeader;
  for (int r = 0; r < kMpRuns; r++) {
    if (len - pos < 4) return mp_bad();
    m.cnt[r] = rd32be(p + pos);
    pos += 4;
    const uint64_t bytes = (uint64_t)m.cnt[r] * kMpRunPoint[r];
    if (len - pos < bytes) return mp_bad();
    m.run[r] = p + pos;
    pos += bytes;
  }
  if (len - pos < 68) return mp_bad();
  m.cs_hash = p + pos;
  m.nrec = rd32be(p + pos + 64);
  pos += 68;
  if (len - pos != (uint64_t)m.nrec * kMpRecord) return mp_bad();
  m.rec = p + pos;
  // flags and coordinates
  static const size_t hdr_psz[6] = {64, 64, 128, 128, 64, 128};
  size_t at = 0;
  for (const size_t psz : hdr_psz) {
    if (!be_plausible(p + at, psz)) return mp_bad();
    at += psz;
  }
  for (int r = 0; r < kMpRuns; r++)
    if (!be_run_plausible(m.run[r], m.cnt[r], kMpRunPoint[r])) return mp_bad();
  for (uint32_t i = 0; i < m.nrec; i++) {
    const uint8_t* r = m.rec + (size_t)i * kMpRecord;
    if (!be_run_plausible(r, 3, 64) || !be_plausible(r + 192, 128)) return mp_bad();
  }
  return G16_OK;
}

}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_export_bellman(const uint8_t* zkey, size_t zkey_len, int device, uint8_t** out, size_t* out_len) {
  if (!zkey || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey export bellman", [&]() { return export_core(zkey, zkey_len, device, out, out_len); });
}

extern "C" int g16_zkey_export_bellman_files(const char* zkey_path, const char* mpcparams_path, int device) {
  if (!zkey_path || !mpcparams_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&zkey_path, 1, mpcparams_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_zkey_export_bellman((const uint8_t*)m[0].p, m[0].len, device, z, zl);
  });
}

extern "C" int g16_zkey_bellman_contribute(const uint8_t* challenge, size_t challenge_len, const uint8_t secret[64], int device,
                                           uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]) {
  if (!challenge || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey bellman contribute",
                      [&]() { return contribute_core(challenge, challenge_len, secret, device, out, out_len, contribution_hash); });
}

extern "C" int g16_zkey_bellman_contribute_files(const char* challenge_path, const char* response_path, const uint8_t secret[64],
                                                 int device, uint8_t contribution_hash[64]) {
  if (!challenge_path || !response_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&challenge_path, 1, response_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_zkey_bellman_contribute((const uint8_t*)m[0].p, m[0].len, secret, device, z, zl, contribution_hash);
  });
}

extern "C" int g16_zkey_import_bellman(const uint8_t* zkey, size_t zkey_len, const uint8_t* response, size_t response_len,
                                       const char* name, int device, uint8_t** out, size_t* out_len, int* ok) {
  if (!zkey || !response || !out || !out_len || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey import bellman",
                      [&]() { return import_core(zkey, zkey_len, response, response_len, name, device, out, out_len, ok); });
}

extern "C" int g16_zkey_import_bellman_files(const char* zkey_path, const char* response_path, const char* out_path, const char* name,
                                             int device, int* ok) {
  if (!zkey_path || !response_path || !out_path || !ok) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile old, resp;
  if (const int rc = old.open_ro(zkey_path)) return rc;
  if (const int rc = resp.open_ro(response_path)) return rc;
  uint8_t* z = nullptr;
  size_t zl = 0;
  if (const int rc = g16_zkey_import_bellman((const uint8_t*)old.p, old.len, (const uint8_t*)resp.p, resp.len, name, device, &z, &zl, ok))
    return rc;
  return *ok ? write_key_file(out_path, z, zl) : G16_OK;
}
