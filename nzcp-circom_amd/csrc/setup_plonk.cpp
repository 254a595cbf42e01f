// PLONK key generation: test-only from a known tau (next paragraph), or from a ceremony file (g16_plonk_setup_ptau).
// Stands in for `snarkjs plonk setup c.r1cs pot.ptau c.zkey` (/root/reference/Makefile:31; [EXT] snarkjs 0.4.12
// plonk_setup.js): R1CS -> PLONK gates as snarkjs does it (public-input gates first; linear combinations reduced to
// one signal by addition gates taken from the front of a queue, results appended), copy-constraint permutation,
// selector / sigma polynomials as N coefficients + 4N evaluations, N + 6 powers of tau -- here from a KNOWN tau
// (seed), so the commitments are [Q(tau)]G by one fixed-base multiplication each.  Restated in oracle/plonk.py::setup,
// whose zkey this must equal byte for byte for the same tau (tests/test_gpu_plonk.py).  The transforms run on the
// device (plonk.hip::plonk_setup_polys); with_lagrange = 0 writes an EMPTY section 13.
#include <algorithm>

#include "fixed_base.h"
#include "mapped_file.h"
#include "ptau.h"

namespace g16 {
namespace {

struct PlonkGate { uint32_t sl, sr, so; FrM qm, ql, qr, qo, qc; };
struct PlonkAdd { uint32_t s1, s2; FrM f1, f2; };

struct PlonkBuilder {
  std::vector<PlonkGate> gates;
  std::vector<PlonkAdd> adds;
  uint32_t nv = 0;
  FrM zero = fp_zero<FrParams>(), one = fr_one();
  struct LC { FrM k; std::vector<Term> t; };   // constant + terms on distinct non-zero wires (first-appearance order)
  // merge duplicate wires, split the constant off, drop zero coefficients; keeps the order of first appearance (what
  // iterating a JS object with integer keys does NOT do -- snarkjs walks ascending signal ids -- so sort by id)
  LC lc_of(const Term* b, const Term* e) {
    LC r;
    r.k = zero;
    std::vector<Term> v(b, e);
    std::sort(v.begin(), v.end(), [](const Term& x, const Term& y) { return x.s < y.s; });
    size_t i = 0;
    while (i < v.size()) {
      FrM sum = zero;
      const uint32_t wire = v[i].s;
      while (i < v.size() && v[i].s == wire) sum = fp_add(sum, v[i++].cf);
      if (fp_is_zero(sum)) continue;
      if (wire == 0) r.k = sum;
      else r.t.push_back({wire, sum});
    }
    return r;
  }
  // reduceCoefs: while more than max_c terms, the first two become one addition gate whose output goes to the back
  void reduce(LC& lc, size_t max_c) {
    size_t head = 0;
    while (lc.t.size() - head > max_c) {
      const Term c1 = lc.t[head], c2 = lc.t[head + 1];
      head += 2;
      const uint32_t so = nv++;
      gates.push_back({c1.s, c2.s, so, zero, fp_neg(c1.cf), fp_neg(c2.cf), one, zero});
      adds.push_back({c1.s, c2.s, c1.cf, c2.cf});
      lc.t.push_back({so, one});
    }
    lc.t.erase(lc.t.begin(), lc.t.begin() + head);
    while (lc.t.size() < max_c) lc.t.push_back({0u, zero});
  }
  void add_sum(LC lc) {
    reduce(lc, 3);
    gates.push_back({lc.t[0].s, lc.t[1].s, lc.t[2].s, zero, lc.t[0].cf, lc.t[1].cf, lc.t[2].cf, lc.k});
  }
};

// where the powers of tau come from: a known tau (test-only), or the points of a .ptau file
struct PlonkTauSrc {
  bool known = true;
  uint64_t seed = 0;
  const uint8_t* tau_g1 = nullptr;   // .ptau section 2: [tau^i]G1, affine Montgomery LE
  uint64_t n_g1 = 0;
  const uint8_t* tau_g2_1 = nullptr; // .ptau section 3, point 1: [tau]G2
  uint32_t power = 0;
};
static int plonk_setup_core(const uint8_t* r1cs, size_t r1cs_len, const PlonkTauSrc& src, int device, int with_lagrange,
                            uint8_t** zkey, size_t* zkey_len) {
  const uint64_t seed = src.seed;
  Circuit c;
  int rc = read_r1cs(r1cs, r1cs_len, c);
  if (rc) return rc;
  PlonkBuilder pb;
  pb.nv = c.n;
  for (uint32_t s = 1; s <= c.p; s++) pb.gates.push_back({s, 0u, 0u, pb.zero, pb.one, pb.zero, pb.zero, pb.zero});
  for (uint32_t r = 0; r < c.m; r++) {
    PlonkBuilder::LC a = pb.lc_of(c.tA.data() + c.rowA[r], c.tA.data() + c.rowA[r + 1]);
    PlonkBuilder::LC b = pb.lc_of(c.tB.data() + c.rowB[r], c.tB.data() + c.rowB[r + 1]);
    PlonkBuilder::LC cc = pb.lc_of(c.tC.data() + c.rowC[r], c.tC.data() + c.rowC[r + 1]);
    const bool a0 = a.t.empty() && fp_is_zero(a.k), b0 = b.t.empty() && fp_is_zero(b.k);
    if (a0 || b0) {
      pb.add_sum(cc);
    } else if (a.t.empty() || b.t.empty()) {   // a constant times a linear combination: k * other - C = 0
      const FrM kk = a.t.empty() ? a.k : b.k;
      const PlonkBuilder::LC& other = a.t.empty() ? b : a;
      std::vector<Term> j;
      j.push_back({0u, fp_sub(fp_mul(kk, other.k), cc.k)});
      for (const Term& t : other.t) j.push_back({t.s, fp_mul(kk, t.cf)});
      for (const Term& t : cc.t) j.push_back({t.s, fp_neg(t.cf)});
      pb.add_sum(pb.lc_of(j.data(), j.data() + j.size()));
    } else {
      pb.reduce(a, 1);
      pb.reduce(b, 1);
      pb.reduce(cc, 1);
      pb.gates.push_back({a.t[0].s, b.t[0].s, cc.t[0].s, fp_mul(a.t[0].cf, b.t[0].cf), fp_mul(a.t[0].cf, b.k),
                          fp_mul(a.k, b.t[0].cf), fp_neg(cc.t[0].cf), fp_sub(fp_mul(a.k, b.k), cc.k)});
    }
  }
  const size_t ng = pb.gates.size();
  int L = 3;   // (the quotient polynomial has 3N + 6 coefficients and must fit 4N: snarkjs, too, starts at 2^3)
  while (((size_t)1 << L) < ng) L++;
  if (L > 24) { set_error("plonk setup: circuit too large (more than 2^24 gates)"); return G16_E_ARG; }
  const size_t N = (size_t)1 << L;
  if (!src.known && ((uint32_t)L > src.power || N + 6 > src.n_g1)) {
    set_error("circuit too big for this power of tau ceremony. " + std::to_string(ng) + " > 2**" + std::to_string(src.power));
    return G16_E_ARG;
  }
  Xo trng(seed + 1);
  FrM tau;
  do { tau = trng.rand_fr(); } while (fp_is_zero(tau));
  const FrM w1 = host_root(L);
  // k1, k2: smallest values whose cosets are disjoint from H and from each other
  auto pow_n = [&](FrM x) { for (int i = 0; i < L; i++) x = fp_sqr(x); return x; };
  const FrM one = fr_one();
  uint64_t k1v = 2;
  while (fp_eq(pow_n(fr_u64(k1v)), one)) k1v++;
  uint64_t k2v = k1v + 1;
  while (fp_eq(pow_n(fr_u64(k2v)), one) || fp_eq(pow_n(fp_mul(fr_u64(k2v), fp_inv(fr_u64(k1v)))), one)) k2v++;
  const FrM k1 = fr_u64(k1v), k2 = fr_u64(k2v);
  // evaluation vectors: 5 selectors, 3 sigmas
  std::vector<std::vector<Fr>> ev(8, std::vector<Fr>(N, fp_zero<FrParams>()));
  std::vector<uint32_t> maps[3];
  for (auto& m : maps) m.assign(N, 0u);
  for (size_t i = 0; i < ng; i++) {
    const PlonkGate& g = pb.gates[i];
    maps[0][i] = g.sl; maps[1][i] = g.sr; maps[2][i] = g.so;
    ev[0][i] = g.qm; ev[1][i] = g.ql; ev[2][i] = g.qr; ev[3][i] = g.qo; ev[4][i] = g.qc;
  }
  {
    std::vector<FrM> last(pb.nv);
    std::vector<uint32_t> first(pb.nv, 0xffffffffu);
    std::vector<uint8_t> seen(pb.nv, 0);
    FrM w = one;
    for (size_t i = 0; i < N; i++) {
      const FrM vals[3] = {w, fp_mul(w, k1), fp_mul(w, k2)};
      for (int col = 0; col < 3; col++) {
        const uint32_t sgn = maps[col][i];
        const size_t ppos = (size_t)col * N + i;
        if (seen[sgn]) ev[5 + col][i] = last[sgn];
        else { first[sgn] = (uint32_t)ppos; seen[sgn] = 1; }
        last[sgn] = vals[col];
      }
      w = fp_mul(w, w1);
    }
    for (uint32_t sgn = 0; sgn < pb.nv; sgn++)
      if (seen[sgn]) ev[5 + first[sgn] / N][first[sgn] % N] = last[sgn];
  }
  // file image
  const size_t nlag = with_lagrange ? (c.p > 0 ? c.p : 1) : 0;
  const size_t polb = N * 32 * 5;
  const size_t hdr = 4 + 32 + 4 + 32 + 20 + 64 + 8 * 64 + 128;
  const uint64_t sizes[16] = {0, 4, hdr, pb.adds.size() * 72, ng * 4, ng * 4, ng * 4, polb, polb, polb, polb, polb, 3 * polb,
                              nlag * polb, (N + 6) * 64};
  static const int ids[14] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14};
  Buf z;
  uint8_t* sp[16] = {};
  if (!bin_layout(z, "zkey", 1, ids, 14, sizes, sp)) { set_error("plonk setup: out of memory"); return G16_E_STATE; }
  { uint32_t two = 2; memcpy(sp[1], &two, 4); }
  for (size_t k = 0; k < pb.adds.size(); k++) {
    uint8_t* q = sp[3] + k * 72;
    memcpy(q, &pb.adds[k].s1, 4); memcpy(q + 4, &pb.adds[k].s2, 4);
    memcpy(q + 8, pb.adds[k].f1.v, 32); memcpy(q + 40, pb.adds[k].f2.v, 32);
  }
  for (int col = 0; col < 3; col++) memcpy(sp[4 + col], maps[col].data(), ng * 4);
  // polynomials on the device: coefficients + 4N evaluations straight into the sections
  {
    const Fr* evp[8];
    uint8_t* outp[8];
    for (int k = 0; k < 8; k++) {
      evp[k] = ev[k].data();
      outp[k] = k < 5 ? sp[7 + k] : sp[12] + (size_t)(k - 5) * polb;
    }
    if ((rc = plonk_setup_polys(device, L, evp, outp))) return rc;
    if (nlag) {   // Lagrange polynomials of the public inputs, 8 at a time
      std::vector<std::vector<Fr>> le(8, std::vector<Fr>(N));
      for (size_t j0 = 0; j0 < nlag; j0 += 8) {
        for (int k = 0; k < 8; k++) {
          std::fill(le[k].begin(), le[k].end(), fp_zero<FrParams>());
          const size_t j = j0 + k < nlag ? j0 + k : nlag - 1;
          le[k][j] = one;
          evp[k] = le[k].data();
          outp[k] = sp[13] + j * polb;
        }
        if ((rc = plonk_setup_polys(device, L, evp, outp))) return rc;
      }
    }
  }
  auto write_header = [&](const uint8_t* commitments /* 8 x 64 */, const uint8_t* x2 /* 128 */) {
    uint8_t* q = bin_put_field(bin_put_field(sp[2], kFqP), kFrP);
    const uint32_t hv[5] = {pb.nv, c.p, (uint32_t)N, (uint32_t)pb.adds.size(), (uint32_t)ng};
    memcpy(q, hv, 20); q += 20;
    memcpy(q, k1.v, 32); memcpy(q + 32, k2.v, 32); q += 64;
    memcpy(q, commitments, 8 * 64);
    memcpy(q + 8 * 64, x2, 128);
  };
  if (!src.known) {
    // a real ceremony's points: the first N + 6 powers are copied, the commitments are MSMs over them on the device
    memcpy(sp[14], src.tau_g1, (N + 6) * 64);
    const uint8_t* cf[8];
    for (int k = 0; k < 8; k++) cf[k] = k < 5 ? sp[7 + k] : sp[12] + (size_t)(k - 5) * polb;
    uint8_t cm[8 * 64];
    if ((rc = plonk_setup_commit(device, src.tau_g1, (uint32_t)N, cf, cm))) return rc;
    write_header(cm, src.tau_g2_1);
    z.give(zkey, zkey_len);
    return G16_OK;
  }
  // powers of tau and the commitments [P(tau)]G (tau is known: one fixed-base multiplication each)
  FixedBaseMul fm(8, 0, device);
  {
    std::vector<FrM> pw(N + 6);
    FrM x = one;
    for (size_t i = 0; i < N + 6; i++) { pw[i] = x; x = fp_mul(x, tau); }
    fm.mul1(pw.data(), N + 6, sp[14]);
    if (fm.rc) return fm.rc;
  }
  {
    FrM cm[8];
    for (int k = 0; k < 8; k++) {   // P(tau) by Horner over the coefficients just written
      const uint8_t* co = k < 5 ? sp[7 + k] : sp[12] + (size_t)(k - 5) * polb;
      FrM acc = fp_zero<FrParams>();
      for (size_t i = N; i-- > 0;) {
        FrM cf;
        memcpy(cf.v, co + i * 32, 32);
        acc = fp_add(fp_mul(acc, tau), cf);
      }
      cm[k] = acc;
    }
    uint8_t cmb[8 * 64], x2[128];
    fixed_mul_many(fm.g1, cm, 8, cmb, 1);
    fixed_mul_many(fm.g2, &tau, 1, x2, 1);
    write_header(cmb, x2);
  }
  z.give(zkey, zkey_len);
  return G16_OK;
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" int g16_plonk_setup(const uint8_t* r1cs, size_t r1cs_len, uint64_t seed, int device, int with_lagrange,
                               uint8_t** zkey, size_t* zkey_len) {
  if (!r1cs || !zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  PlonkTauSrc src;
  src.known = true;
  src.seed = seed;
  return no_bad_alloc("plonk setup", [&]() {
    return plonk_setup_core(r1cs, r1cs_len, src, device, with_lagrange, zkey, zkey_len);
  });
}

// `snarkjs plonk setup c.r1cs pot.ptau c.zkey` (/root/reference/Makefile:31) with a REAL powers-of-tau file: .ptau v1
// ([EXT] snarkjs powersoftau_utils.js: section 1 = n8, q, power, ceremonyPower; section 2 = 2^(power+1) - 1 points
// [tau^i]G1; section 3 = 2^power points [tau^i]G2; affine Montgomery LE).  The N + 6 powers are copied into the key and
// the eight selector / sigma commitments are MSMs over them on the device.
extern "C" int g16_plonk_setup_ptau(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                                    int with_lagrange, uint8_t** zkey, size_t* zkey_len) {
  if (!r1cs || !ptau || !zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  PtauView pv;
  if (const int rc = ptau_open(ptau, ptau_len, pv, /*tau_sections=*/true)) return rc;
  const BinSection &s2 = pv.sec[2], &s3 = pv.sec[3];
  if (s2.size < (((uint64_t)2 << pv.power) - 1) * 64 || s3.size < 2 * 128) return ptau_bad("Invalid File format");
  PlonkTauSrc src;
  src.known = false;
  src.power = pv.power;
  src.tau_g1 = s2.p;
  src.n_g1 = s2.size / 64;
  src.tau_g2_1 = s3.p + 128;
  return no_bad_alloc("plonk setup", [&]() {
    return plonk_setup_core(r1cs, r1cs_len, src, device, with_lagrange, zkey, zkey_len);
  });
}

extern "C" int g16_plonk_setup_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                                     int with_lagrange) {
  if (!r1cs_path || !ptau_path || !zkey_path) { set_error("NULL argument"); return G16_E_ARG; }
  const char* in[2] = {r1cs_path, ptau_path};
  return files_form(in, 2, zkey_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_plonk_setup_ptau((const uint8_t*)m[0].p, m[0].len, (const uint8_t*)m[1].p, m[1].len, device, with_lagrange, z, zl);
  });
}
