// `snarkjs zkey new` with its circuit hash ([EXT] snarkjs 0.4.12 zkey_new.js, restated from its description):
//   csHash = Blake2b-512( alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2
//                         | u32be p+1 | IC | u32be N-1 | H | u32be n-p-1 | L | u32be n | A | u32be n | B1 | u32be n | B2 )
// every point in uncompressed big-endian standard form: byte for byte the MPCParams image of the fresh key
// (zkey_bellman.h) up to its csHash field.  H is NOT section 9: as in snarkjs (hashHPoints) it comes from the ceremony's
// section 2, H_k = P_(k+N) - P_k, k < N - 1 (zkey_cshash.hip).  `zkey export bellman` reaches the same H from section 9
// by its basis change; the two agree for k <= N - 2, which is all the image holds.
// The hash consumes the image in order and is serial: it is the floor of this stage.  Every run goes through the
// device in chunks (IC, L, A, B1, B2: the to-be stage of ptau_points.hip; H: zkey_cshash.hip) and a chunk is hashed on
// this thread as soon as it has come down, while the next one is converted and copied.
// The key itself is g16_groth16_setup_ptau's; only the first 64 bytes of section 10 differ.
// NOT claimed: that this is the value snarkjs computes for the same inputs.  The package is not at hand; the image and
// the H rule are restated from its description.
#include "zkey_cshash.h"

#include <chrono>
#include <memory>

#include "fixed_base.h"
#include "internal.h"
#include "mapped_file.h"
#include "zkey_bellman.h"

namespace g16 {
namespace {

void wr32be(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
int log2_of(uint32_t N) {
  int L = 0;
  while (((uint32_t)1 << L) < N) L++;
  return L;
}
int domain_too_large(const char* route) { set_error(std::string(route) + ": the domain is above 2^24"); return G16_E_ARG; }

}  // namespace

int cshash_check_ptau(const PtauView& pv, int log_n) {
  const uint64_t m = 2 * ((uint64_t)1 << log_n) - 1;
  if (!pv.sec[2].p || pv.sec[2].size / 64 < m) return ptau_bad("Invalid File format");
  for (uint64_t j = 0; j < m; j++)
    if (!g1_image_ok(pv.sec[2].p + j * 64)) return ptau_bad("Invalid File format");
  return G16_OK;
}

int zkey_cs_hash_core(const KeyView& k, const PtauView& pv, int device, uint8_t out[64]) {
  const auto t0 = std::chrono::steady_clock::now();
  if (const int rc = require_hip_device("zkey cs hash", device)) return rc;
  const int L = log2_of(k.N);
  uint32_t cnt[kMpRuns];
  mp_key_counts(k.nVars, k.nPublic, k.N, cnt);
  size_t largest = 1, bytes = kMpHeader;
  for (int r = 0; r < kMpRuns; r++) {
    largest = std::max(largest, (size_t)cnt[r] * kMpRunPoint[r]);
    bytes += 4 + (size_t)cnt[r] * kMpRunPoint[r];
  }
  const std::unique_ptr<uint8_t[]> be(new uint8_t[largest]);   // one run's image at a time (not zeroed: 105 MB at 2^20)

  Blake2b512 hash;
  double hash_ms = 0;
  const ChunkSink feed = [&](const uint8_t* p, size_t n) {
    const auto t1 = std::chrono::steady_clock::now();
    hash.update(p, n);
    hash_ms += ms_since(t1);
  };
  {
    uint8_t hdr[kMpHeader];
    mp_header_image(k.f.sec[2].p, hdr);
    feed(hdr, kMpHeader);
  }
  const uint8_t* src[kMpRuns] = {k.f.sec[3].p, nullptr, k.f.sec[8].p, k.f.sec[5].p, k.f.sec[6].p, k.f.sec[7].p};
  ChunkStats st[kMpRuns];
  for (int r = 0; r < kMpRuns; r++) {
    uint8_t c4[4];
    wr32be(c4, cnt[r]);
    feed(c4, 4);
    const int rc = r == 1 ? zkey_h_monomial(device, pv.sec[2].p, L, be.get(), &st[r], &feed)
                          : ptau_points_to_be(device, kMpRunPoint[r] == 128, src[r], cnt[r], be.get(), &st[r], &feed);
    if (rc) return rc;
  }
  hash.final(out);
  if (getenv("G16_TRACE_HOST")) {
    float kern = 0, xfer = 0;
    for (int r = 0; r < kMpRuns; r++)
      if (r != 1) { kern += st[r].kern_ms; xfer += st[r].xfer_ms; }
    fprintf(stderr, "[g16] zkey cs hash: domain 2^%d, image %zu bytes; kernels H %.3f ms, to-be %.3f ms, transfers %.3f ms; hash %.3f ms; call %.3f ms\n",
            L, bytes, st[1].kern_ms, kern, xfer + st[1].xfer_ms, hash_ms, ms_since(t0));
  }
  return G16_OK;
}

namespace {

int cs_hash_entry(const uint8_t* zkey, size_t zkey_len, const uint8_t* ptau, size_t ptau_len, int device, uint8_t out[64]) {
  KeyView k;
  if (const int rc = open_key(zkey, zkey_len, k, true)) return rc;
  {
    const G1Affine g1 = g1_generator();
    const G2Affine g2 = g2_generator();
    const uint8_t* h = k.f.sec[2].p;
    if (memcmp(h + kHdrDelta1, &g1, 64) != 0 || memcmp(h + kHdrDelta2, &g2, 128) != 0 || !k.mpc.rec.empty()) {
      set_error("zkey cs hash: not an initial key");
      return G16_E_ARG;
    }
  }
  const int L = log2_of(k.N);
  if (L > 24) return domain_too_large("zkey cs hash");
  PtauView pv;
  if (const int rc = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/false)) return rc;
  if ((int)pv.power < L) { set_error("zkey new: the ptau is too small for this key"); return G16_E_ARG; }
  if (const int rc = cshash_check_ptau(pv, L)) return rc;
  return zkey_cs_hash_core(k, pv, device, out);
}

int zkey_new_entry(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device, uint8_t** zkey,
                   size_t* zkey_len, uint8_t cs_hash[64]) {
  *zkey = nullptr;
  *zkey_len = 0;
  const SetupPtauCheck check = [](const PtauView& pv, int L) {
    if (L > 24) return domain_too_large("zkey new");
    return cshash_check_ptau(pv, L);
  };
  uint8_t* z = nullptr;
  size_t zl = 0;
  if (const int rc = groth16_setup_ptau_checked(r1cs, r1cs_len, ptau, ptau_len, device, &z, &zl, &check)) return rc;
  MallocPtr guard(z);
  KeyView k;
  PtauView pv;
  if (const int rc = open_key(z, zl, k, true)) return rc;
  if (const int rc = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/false)) return rc;
  uint8_t h[64];
  if (const int rc = zkey_cs_hash_core(k, pv, device, h)) return rc;
  memcpy(z + (k.mpc.cs_hash - z), h, 64);
  if (cs_hash) memcpy(cs_hash, h, 64);
  *zkey = guard.release();
  *zkey_len = zl;
  return G16_OK;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" int g16_zkey_cs_hash(const uint8_t* zkey, size_t zkey_len, const uint8_t* ptau, size_t ptau_len, int device,
                                uint8_t out[64]) {
  if (!zkey || !ptau || !out) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey cs hash", [&]() { return cs_hash_entry(zkey, zkey_len, ptau, ptau_len, device, out); });
}

extern "C" int g16_zkey_cs_hash_files(const char* zkey_path, const char* ptau_path, int device, uint8_t out[64]) {
  if (!zkey_path || !ptau_path || !out) { set_error("NULL argument"); return G16_E_ARG; }
  MappedFile in[2];
  if (const int rc = in[0].open_ro(zkey_path)) return rc;
  if (const int rc = in[1].open_ro(ptau_path)) return rc;
  return g16_zkey_cs_hash((const uint8_t*)in[0].p, in[0].len, (const uint8_t*)in[1].p, in[1].len, device, out);
}

extern "C" int g16_zkey_new(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                            uint8_t** zkey, size_t* zkey_len, uint8_t cs_hash[64]) {
  if (!r1cs || !ptau || !zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("zkey new", [&]() { return zkey_new_entry(r1cs, r1cs_len, ptau, ptau_len, device, zkey, zkey_len, cs_hash); });
}

extern "C" int g16_zkey_new_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                                  uint8_t cs_hash[64]) {
  if (!r1cs_path || !ptau_path || !zkey_path) { set_error("NULL argument"); return G16_E_ARG; }
  const char* in[2] = {r1cs_path, ptau_path};
  return files_form(in, 2, zkey_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_zkey_new((const uint8_t*)m[0].p, m[0].len, (const uint8_t*)m[1].p, m[1].len, device, z, zl, cs_hash);
  });
}
