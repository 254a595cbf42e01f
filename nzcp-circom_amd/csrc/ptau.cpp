// The .ptau reader (ptau.h), `snarkjs powersoftau prepare phase2` and the test-only writer of a known ceremony.
#include <chrono>

#include "fixed_base.h"
#include "mapped_file.h"
#include "ptau.h"

namespace g16 {

int ptau_bad(const char* why) { set_error(std::string("ptau: ") + why); return G16_E_FORMAT; }

int ptau_open(const uint8_t* ptau, size_t ptau_len, PtauView& v, bool tau_sections) {
  if (const int rc = bin_open(ptau, ptau_len, "ptau", 1, v)) return rc;
  const BinSection& s1 = v.sec[1];
  if (!s1.p || (tau_sections && (!v.sec[2].p || !v.sec[3].p)) || s1.size < 4 + 32 + 8 || !bin_is_field(s1.p, s1.size, kFqP))
    return ptau_bad("Invalid File format (bn128 powers of tau expected)");
  v.power = rd32(s1.p + 36);
  if (v.power > 28) return ptau_bad("Invalid File format");
  return G16_OK;
}

int ptau_open_prepared(const uint8_t* ptau, size_t ptau_len, PtauView& v) {
  if (const int rc = ptau_open(ptau, ptau_len, v, /*tau_sections=*/false)) return rc;
  if (!v.sec[12].p) { set_error("Powers of tau is not prepared."); return G16_E_FORMAT; }
  if (!v.sec[4].p || v.sec[4].size < 64 || !v.sec[5].p || v.sec[5].size < 64 || !v.sec[6].p || v.sec[6].size < 128)
    return ptau_bad("Invalid File format");
  for (int id = 12; id <= 15; id++) {
    if (!v.sec[id].p) return ptau_bad("Invalid File format");
    const uint64_t psz = id == 13 ? 128 : 64;
    if (v.sec[id].size % psz) return ptau_bad("Invalid File format");
    const uint64_t pts = v.sec[id].size / psz;   // blocks 0 .. K-1 hold 2^K - 1 points
    int K = 0;
    while (K < 40 && (((uint64_t)1 << K) - 1) < pts) K++;
    const int max_blocks = (int)v.power + (id == 12 ? 2 : 1);
    if ((((uint64_t)1 << K) - 1) != pts || K > max_blocks) return ptau_bad("Invalid File format");
    v.blocks[id] = K;
  }
  return G16_OK;
}

}  // namespace g16

using namespace g16;

// ------------------------------------------------------------------ powersoftau prepare phase2
// `snarkjs powersoftau prepare phase2 in.ptau out.ptau` ([EXT] snarkjs 0.4.12 powersoftau_preparephase2.js): the image
// with sections 1-7 of the input, byte for byte and in that order, then 12, 13, 14, 15 computed from sections 2, 3,
// 4, 5: block k of a section is the inverse Fourier transform of size 2^k of its source's first 2^k points (the layout
// of setup_groth16.cpp; ptau_prepare.hip).  Section 12 runs through block power + 1, whose last input -- section 2 holds
// 2^(power+1) - 1 points -- is the point at infinity, as in snarkjs: that block is [L_j(tau) - w^j tau^(M-1) / M]G1
// (M = 2^(power+1)), not the Lagrange basis itself; Groth16 reads its odd points as the H basis, against a polynomial
// of degree <= M - 2, where the extra term cancels.  Sections 12-15 of an input that is already prepared are ignored
// and recomputed, other section ids are dropped, and a missing section 7 is written as "no contributions" (four zero
// bytes).  Sections 2-6 must have exactly the sizes the header's power implies.  Powers up to kPreparePowerMax.
namespace {
constexpr uint32_t kPreparePowerMax = 24;   // (what g16_ptau_synth can produce; the device arrays index with 32 bits)

int ptau_prepare_core(const uint8_t* ptau, size_t ptau_len, int device, uint8_t** out, size_t* out_len) {
  const auto t0 = std::chrono::steady_clock::now();
  PtauView pv;
  if (const int rc = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/false)) return rc;
  if (pv.power > kPreparePowerMax) {
    set_error("ptau prepare: power " + std::to_string(pv.power) + " is above the supported limit of " +
              std::to_string(kPreparePowerMax));
    return G16_E_ARG;
  }
  const uint64_t n = (uint64_t)1 << pv.power;
  const uint64_t want[7] = {0, 0, (2 * n - 1) * 64, n * 128, n * 64, n * 64, 128};
  for (int id = 2; id <= 6; id++)
    if (!pv.sec[id].p || pv.sec[id].size != want[id]) return ptau_bad("Invalid File format");
  if (const int rc = require_hip_device("ptau prepare", device)) return rc;

  static const uint8_t no_contributions[4] = {0, 0, 0, 0};
  const uint8_t* in[8] = {};
  uint64_t sizes[16] = {};
  for (int id = 1; id <= 7; id++) { in[id] = pv.sec[id].p; sizes[id] = pv.sec[id].size; }
  if (!in[7]) { in[7] = no_contributions; sizes[7] = 4; }
  sizes[12] = (4 * n - 1) * 64;
  sizes[13] = (2 * n - 1) * 128;
  sizes[14] = sizes[15] = (2 * n - 1) * 64;
  static const int ids[11] = {1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15};
  Buf z;
  uint8_t* sp[16] = {};
  if (!bin_layout(z, "ptau", 1, ids, 11, sizes, sp)) { set_error("ptau prepare: out of memory"); return G16_E_STATE; }
  for (int id = 1; id <= 7; id++) memcpy(sp[id], in[id], sizes[id]);
  const int P = (int)pv.power;
  PtauPrepareStats st[4];
  int rc = ptau_prepare_g1(device, pv.sec[2].p, 2 * n - 1, P + 1, sp[12], &st[0]);
  if (!rc) rc = ptau_prepare_g2(device, pv.sec[3].p, n, P, sp[13], &st[1]);
  if (!rc) rc = ptau_prepare_g1(device, pv.sec[4].p, n, P, sp[14], &st[2]);
  if (!rc) rc = ptau_prepare_g1(device, pv.sec[5].p, n, P, sp[15], &st[3]);
  if (rc) return rc;
  if (getenv("G16_TRACE_HOST")) {
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr,
            "[g16] ptau prepare: power %d; kernels section 12 %.3f ms, 13 %.3f ms, 14 %.3f ms, 15 %.3f ms; point "
            "multiplications G1 %llu G2 %llu, additions G1 %llu G2 %llu; call %.3f ms\n",
            P, st[0].kern_ms, st[1].kern_ms, st[2].kern_ms, st[3].kern_ms,
            (unsigned long long)(st[0].muls + st[2].muls + st[3].muls), (unsigned long long)st[1].muls,
            (unsigned long long)(st[0].adds + st[2].adds + st[3].adds), (unsigned long long)st[1].adds, wall_ms);
  }
  z.give(out, out_len);
  return G16_OK;
}
}  // namespace

extern "C" int g16_ptau_prepare(const uint8_t* ptau, size_t ptau_len, int device, uint8_t** out, size_t* out_len) {
  if (!ptau || !out || !out_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("ptau prepare", [&]() { return ptau_prepare_core(ptau, ptau_len, device, out, out_len); });
}

extern "C" int g16_ptau_prepare_files(const char* in_path, const char* out_path, int device) {
  if (!in_path || !out_path) { set_error("NULL argument"); return G16_E_ARG; }
  return files_form(&in_path, 1, out_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_ptau_prepare((const uint8_t*)m[0].p, m[0].len, device, z, zl);
  });
}

// test-only: a .ptau v1 image for a known (tau, alpha, beta): sections 1-7 as snarkjs lays them out (2 = [tau^i]G1,
// i < 2^(power+1) - 1; 3 = [tau^i]G2, 4 = [alpha tau^i]G1, 5 = [beta tau^i]G1, i < 2^power; 6 = [beta]G2; 7 = no
// contributions) and, when prepared, 12-15 in the block layout (12 through block power + 1, 13-15 through block power)
extern "C" int g16_ptau_synth(uint32_t power, const uint8_t tab[3 * 32], int prepared, int device, uint8_t** ptau,
                              size_t* ptau_len) {
  if (!tab || !ptau || !ptau_len) { set_error("NULL argument"); return G16_E_ARG; }
  if (power > 24) { set_error("ptau synth: power above 24"); return G16_E_ARG; }
  if (device < -1) { set_error("ptau synth: bad device ordinal"); return G16_E_ARG; }
  FrM s[3];
  for (int k = 0; k < 3; k++) {
    Fr x;
    memcpy(x.v, tab + 32 * k, 32);
    s[k] = fp_to_mont(x);   // (reduces a value >= r)
  }
  const FrM tau = s[0], alpha = s[1], beta = s[2];
  return no_bad_alloc("ptau synth", [&]() -> int {
    const uint64_t n = (uint64_t)1 << power;
    const uint64_t sizes[16] = {0, 44, (2 * n - 1) * 64, n * 128, n * 64, n * 64, 128, 4, 0, 0, 0, 0,
                                (4 * n - 1) * 64, (2 * n - 1) * 128, (2 * n - 1) * 64, (2 * n - 1) * 64};
    static const int ids[11] = {1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15};
    Buf z;
    uint8_t* sp[16] = {};
    if (!bin_layout(z, "ptau", 1, ids, prepared ? 11 : 7, sizes, sp)) { set_error("ptau synth: out of memory"); return G16_E_STATE; }
    {
      uint8_t* q = bin_put_field(sp[1], kFqP);
      memcpy(q, &power, 4); memcpy(q + 4, &power, 4);
      memset(sp[7], 0, 4);
    }
    FixedBaseMul fm(8, 0, device);
    auto mul1 = [&](const std::vector<FrM>& ks, uint8_t* out) { fm.mul1(ks.data(), ks.size(), out); };
    auto mul2 = [&](const std::vector<FrM>& ks, uint8_t* out) { fm.mul2(ks.data(), ks.size(), out); };
    auto scaled = [](const std::vector<FrM>& v, const FrM& k, size_t cnt) {
      std::vector<FrM> o(cnt);
      for (size_t i = 0; i < cnt; i++) o[i] = fp_mul(v[i], k);
      return o;
    };
    {
      std::vector<FrM> pw(2 * n - 1);
      FrM x = fr_one();
      for (auto& y : pw) { y = x; x = fp_mul(x, tau); }
      mul1(pw, sp[2]);
      mul2(std::vector<FrM>(pw.begin(), pw.begin() + n), sp[3]);
      mul1(scaled(pw, alpha, n), sp[4]);
      mul1(scaled(pw, beta, n), sp[5]);
      mul2(std::vector<FrM>{beta}, sp[6]);
    }
    if (prepared) {
      // block k of the Lagrange basis of the size-2^k domain: all blocks in one scalar vector per section
      std::vector<FrM> lag(4 * n - 1), blk;
      for (uint32_t k = 0; k <= power + 1; k++) {
        lagrange_at((int)k, tau, 0, 1, (size_t)1 << k, blk);
        std::copy(blk.begin(), blk.end(), lag.begin() + (((size_t)1 << k) - 1));
      }
      mul1(lag, sp[12]);
      mul2(std::vector<FrM>(lag.begin(), lag.begin() + (2 * n - 1)), sp[13]);
      mul1(scaled(lag, alpha, 2 * n - 1), sp[14]);
      mul1(scaled(lag, beta, 2 * n - 1), sp[15]);
    }
    if (fm.rc) return fm.rc;
    z.give(ptau, ptau_len);
    return G16_OK;
  });
}
