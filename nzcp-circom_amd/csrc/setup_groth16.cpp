// Groth16 key generation in snarkjs's zkey layout (H basis App. C.3): the zkey image, the test-only
// trapdoor route (setup_gpu.hip) and `snarkjs groth16 setup` from a prepared ceremony file (setup_ptau.hip).
#include <atomic>
#include <chrono>

#include "fixed_base.h"
#include "mapped_file.h"
#include "ptau.h"

namespace g16 {

// where the fixed-base multiplications of the *_setup entry points run: -1 = host threads, >= 0 = that HIP device
static std::atomic<int> g_setup_device{-1};

// The .zkey image of a Groth16 key for circuit `c` over the domain 2^L, shared by the trapdoor setups and the .ptau
// route (g16_groth16_setup_ptau) so both write the same bytes: every section laid out, section 1, the scalars of
// section 2, section 4 (the coefficient records: A terms then B terms in constraint order, then the p + 1 public-input
// binding rows (A, row m + i, wire i, 1)) and section 10 (64 zero bytes, u32 0) written.  The caller fills the six
// section-2 points (G16ZkeyImage::hdr_points) and sections 3 (IC), 5 (A), 6 (B1), 7 (B2), 8 (C) and 9 (H).
struct G16ZkeyImage {
  Buf z;
  uint8_t* sec[16] = {};
  uint8_t* hdr_points = nullptr;   // alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2 (64 / 64 / 128 / 128 / 64 / 128)
};
static int g16_zkey_layout(const Circuit& c, int L, G16ZkeyImage& im) {
  const uint32_t n = c.n, p = c.p, m = c.m;
  const size_t N = (size_t)1 << L;
  const size_t ncoef = c.tA.size() + c.tB.size() + (size_t)p + 1;
  const size_t nC = (size_t)n - p - 1;
  const size_t hdr2 = 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128;
  const uint64_t sizes[16] = {0, 4, hdr2, (uint64_t)(p + 1) * 64, 4 + ncoef * 44, (uint64_t)n * 64, (uint64_t)n * 64,
                              (uint64_t)n * 128, nC * 64, N * 64, 64 + 4};
  static const int ids[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
  if (!bin_layout(im.z, "zkey", 1, ids, 10, sizes, im.sec)) { set_error("synth: out of memory"); return G16_E_STATE; }
  { uint32_t one = 1; memcpy(im.sec[1], &one, 4); }
  {
    uint8_t* q = bin_put_field(bin_put_field(im.sec[2], kFqP), kFrP);
    uint32_t dom = (uint32_t)N;
    memcpy(q, &n, 4); memcpy(q + 4, &p, 4); memcpy(q + 8, &dom, 4); q += 12;
    im.hdr_points = q;
  }
  {
    uint32_t nc32 = (uint32_t)ncoef;
    memcpy(im.sec[4], &nc32, 4);
    uint8_t* q = im.sec[4] + 4;
    auto rec = [&](uint32_t mm, uint32_t cc, uint32_t ss, const FrM& cf) {
      memcpy(q, &mm, 4); memcpy(q + 4, &cc, 4); memcpy(q + 8, &ss, 4);
      const Fr raw = fp_to_mont(cf);  // Montgomery(coef) * R = coef * R^2, stored as a plain integer
      memcpy(q + 12, raw.v, 32);
      q += 44;
    };
    for (uint32_t r = 0; r < m; r++) {
      for (uint32_t k = c.rowA[r]; k < c.rowA[r + 1]; k++) rec(0, r, c.tA[k].s, c.tA[k].cf);
      for (uint32_t k = c.rowB[r]; k < c.rowB[r + 1]; k++) rec(1, r, c.tB[k].s, c.tB[k].cf);
    }
    for (uint32_t i = 0; i <= p; i++) rec(0, m + i, i, fr_one());
  }
  memset(im.sec[10], 0, sizes[10]);
  return G16_OK;
}

int setup_core_td(const Circuit& c, const FrM td[5], int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** vkey,
                  size_t* vkey_len) {
  const uint32_t n = c.n, p = c.p, m = c.m;
  const int L = g16_domain_log(c);
  if (L > 27) { set_error("setup: circuit too large"); return G16_E_ARG; }
  const size_t N = (size_t)1 << L;

  const FrM tau = td[0], alpha = td[1], beta = td[2], gamma = td[3], delta = td[4];
  std::vector<FrM> Lg;
  lagrange_at(L, tau, 0, 1, N, Lg);
  std::vector<FrM> u(n, fp_zero<FrParams>()), v(n, fp_zero<FrParams>()), t(n, fp_zero<FrParams>());
  for (uint32_t r = 0; r < m; r++) {
    for (uint32_t k = c.rowA[r]; k < c.rowA[r + 1]; k++)
      u[c.tA[k].s] = fp_add(u[c.tA[k].s], fp_mul(c.tA[k].cf, Lg[r]));
    for (uint32_t k = c.rowB[r]; k < c.rowB[r + 1]; k++)
      v[c.tB[k].s] = fp_add(v[c.tB[k].s], fp_mul(c.tB[k].cf, Lg[r]));
    for (uint32_t k = c.rowC[r]; k < c.rowC[r + 1]; k++)
      t[c.tC[k].s] = fp_add(t[c.tC[k].s], fp_mul(c.tC[k].cf, Lg[r]));
  }
  for (uint32_t i = 0; i <= p; i++) u[i] = fp_add(u[i], Lg[m + i]);   // public-input binding rows
  const FrM ginv = fp_inv(gamma), dinv = fp_inv(delta);
  std::vector<FrM> kic(p + 1), kc(n - p - 1), hs;
  for (uint32_t i = 0; i < n; i++) {
    const FrM kk = fp_add(fp_add(fp_mul(beta, u[i]), fp_mul(alpha, v[i])), t[i]);
    if (i <= p) kic[i] = fp_mul(kk, ginv);
    else kc[i - p - 1] = fp_mul(kk, dinv);
  }
  lagrange_at(L + 1, tau, 1, 2, N, hs);  // L^(2N)_{2i+1}(tau)
  for (auto& x : hs) x = fp_mul(x, dinv);

  // fixed-base multiplications: host threads, or the device selected by g16_setup_device (setup_gpu.hip; a
  // small-window table then -- the device has the lanes, the table should stay in its L2)
  const int dev = g_setup_device.load();
  const int wb = dev >= 0 ? 8 : (n >= 20000 ? 16 : 8);
  FixedBaseMul fm(wb, threads, dev, /*device_min=*/64);
  G16ZkeyImage im;
  int rc = g16_zkey_layout(c, L, im);
  if (rc) return rc;
  {
    uint8_t* q = im.hdr_points;
    const FrM hk[3] = {alpha, beta, delta};
    uint8_t g1pts[3 * 64], g2pts[3 * 128];
    fixed_mul_many(fm.g1, hk, 3, g1pts, 1);
    const FrM hk2[3] = {beta, gamma, delta};
    fixed_mul_many(fm.g2, hk2, 3, g2pts, 1);
    memcpy(q, g1pts, 64); q += 64;            // alpha1
    memcpy(q, g1pts + 64, 64); q += 64;       // beta1
    memcpy(q, g2pts, 128); q += 128;          // beta2
    memcpy(q, g2pts + 128, 128); q += 128;    // gamma2
    memcpy(q, g1pts + 128, 64); q += 64;      // delta1
    memcpy(q, g2pts + 256, 128);              // delta2
  }
  fm.mul1(kic.data(), kic.size(), im.sec[3]);
  fm.mul1(u.data(), n, im.sec[5]);
  fm.mul1(v.data(), n, im.sec[6]);
  fm.mul2(v.data(), n, im.sec[7]);
  fm.mul1(kc.data(), kc.size(), im.sec[8]);
  fm.mul1(hs.data(), hs.size(), im.sec[9]);
  if (fm.rc) return fm.rc;
  im.z.give(zkey, zkey_len);
  if (vkey && vkey_len) {
    // alpha1 | beta2 | gamma2 | delta2 | IC[0..p]   (affine Montgomery LE)
    Buf b;
    b.reserve(64 + 3 * 128 + (size_t)(p + 1) * 64);
    const uint8_t* h = im.hdr_points;
    b.put(h, 64);              // alpha1
    b.put(h + 128, 128);       // beta2
    b.put(h + 256, 128);       // gamma2
    b.put(h + 448, 128);       // delta2
    b.put(im.sec[3], (size_t)(p + 1) * 64);
    b.give(vkey, vkey_len);
  }
  return G16_OK;
}

int setup_core(const Circuit& c, uint64_t seed, int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** vkey,
               size_t* vkey_len) {
  Xo trng(seed + 1);
  FrM td[5];
  for (int k = 0; k < 5;) {
    const FrM v = trng.rand_fr();
    if (!fp_is_zero(v)) td[k++] = v;
  }
  return setup_core_td(c, td, threads, zkey, zkey_len, vkey, vkey_len);
}

}  // namespace g16

using namespace g16;

extern "C" int g16_setup_device(int device) {
  if (device < -1) { set_error("setup: bad device ordinal"); return G16_E_ARG; }
  g_setup_device.store(device);
  return G16_OK;
}

// Test-only trapdoor setup of a REAL circuit: .r1cs in, snarkjs-layout .zkey (+ vkey points) out.
extern "C" int g16_r1cs_setup(const uint8_t* r1cs, size_t r1cs_len, uint64_t seed, int threads, uint8_t** zkey,
                              size_t* zkey_len, uint8_t** vkey, size_t* vkey_len) {
  if (!zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("setup", [&]() -> int {
    Circuit c;
    int rc = read_r1cs(r1cs, r1cs_len, c);
    if (rc) return rc;
    uint64_t need = (uint64_t)c.m + c.p + 1;
    if (need > ((uint64_t)1 << 27)) { set_error("r1cs: circuit too large"); return G16_E_ARG; }
    return setup_core(c, seed, threads, zkey, zkey_len, vkey, vkey_len);
  });
}

// test-only: setup_core with the caller's trapdoor (standard-form LE scalars, each < r; gamma, delta non-zero)
extern "C" int g16_r1cs_setup_trapdoor(const uint8_t* r1cs, size_t r1cs_len, const uint8_t td[5 * 32], int threads,
                                       uint8_t** zkey, size_t* zkey_len, uint8_t** vkey, size_t* vkey_len) {
  if (!r1cs || !td || !zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  FrM tdm[5];
  for (int k = 0; k < 5; k++) {
    Fr x;
    memcpy(x.v, td + 32 * k, 32);
    if (!fr_below_modulus(x.v)) { set_error("setup: trapdoor scalar not below r"); return G16_E_ARG; }
    tdm[k] = fp_to_mont(x);
  }
  if (fp_is_zero(tdm[3]) || fp_is_zero(tdm[4])) { set_error("setup: gamma and delta must be non-zero"); return G16_E_ARG; }
  return no_bad_alloc("setup", [&]() -> int {
    Circuit c;
    int rc = read_r1cs(r1cs, r1cs_len, c);
    if (rc) return rc;
    if ((uint64_t)c.m + c.p + 1 > ((uint64_t)1 << 27)) { set_error("r1cs: circuit too large"); return G16_E_ARG; }
    return setup_core_td(c, tdm, threads, zkey, zkey_len, vkey, vkey_len);
  });
}

// ------------------------------------------------------------------ Groth16 setup from a prepared .ptau
// `snarkjs groth16 setup c.r1cs pot.ptau c_0000.zkey` ([EXT] snarkjs 0.4.12 zkey_new.js).  The prepared ceremony file
// (`powersoftau prepare phase2`) carries the Lagrange-basis sections 12 = [L_i(tau)]G1, 13 = [L_i(tau)]G2,
// 14 = [alpha L_i(tau)]G1, 15 = [beta L_i(tau)]G1, each stored as blocks k = 0, 1, ... of 2^k points (block k starts at
// point 2^k - 1).  The block count is derived from each section's length.  With N = 2^L the domain of setup_core:
//   A_j = sum a_cj [L_c] (+ [L_{m+j}] for j <= p),  B1_j = sum b_cj [L_c]G1,  B2_j = sum b_cj [L_c]G2,
//   K_j = sum (a_cj [beta L_c] + b_cj [alpha L_c] + c_cj [L_c]) (+ [beta L_{m+j}] for j <= p): IC for j <= p, C above,
//   H_i = point 2i + 1 of block L + 1 of section 12 ([L^(2N)_{2i+1}(tau)]G1),
// gamma = delta = 1 (a fresh _0000 key), section 10 as setup_core writes it.  The sums run on the device
// (setup_ptau.hip); the key for a ptau of a known (tau, alpha, beta) is byte for byte setup_core's with
// (tau, alpha, beta, 1, 1).
// before_device (optional; zkey_cshash_host.cpp): a caller's own checks of the ptau for this domain, run after every
// check of the setup and before the device is asked for
int g16::groth16_setup_ptau_checked(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                                    uint8_t** zkey, size_t* zkey_len, const SetupPtauCheck* before_device) {
  return no_bad_alloc("groth16 setup", [&]() -> int {
    // every input is checked before the device is touched
    Circuit c;
    int rc = read_r1cs(r1cs, r1cs_len, c);
    if (rc) return rc;
    PtauView pv;
    if ((rc = ptau_open_prepared(ptau, ptau_len, pv))) return rc;
    const uint32_t n = c.n, p = c.p, m = c.m;
    const int L = g16_domain_log(c);
    if (L > 27) { set_error("r1cs: circuit too large"); return G16_E_ARG; }
    if ((uint32_t)L > pv.power || pv.blocks[12] < L + 2 || pv.blocks[13] < L + 1 || pv.blocks[14] < L + 1 ||
        pv.blocks[15] < L + 1) {
      set_error("circuit too big for this power of tau ceremony. " + std::to_string((uint64_t)m + p + 1) + " > 2**" +
                std::to_string(pv.power));
      return G16_E_FORMAT;
    }
    if (before_device && (rc = (*before_device)(pv, L))) return rc;
    if ((rc = require_hip_device("groth16 setup", device))) return rc;
    const size_t N = (size_t)1 << L;
    const size_t blkL = N - 1, blkL1 = 2 * N - 1;   // first point of block L / L + 1
    const uint8_t* lag1 = pv.sec[12].p + blkL * 64;
    const uint8_t* lag2 = pv.sec[13].p + blkL * 128;
    const uint8_t* alag = pv.sec[14].p + blkL * 64;
    const uint8_t* blag = pv.sec[15].p + blkL * 64;
    const uint8_t* hblk = pv.sec[12].p + blkL1 * 64;

    // the term lists, CSC by output (counting sort): G1 outputs A_j = j, B1_j = n + j, K_j = 2n + j over the bases
    // [L_c] | [alpha L_c] | [beta L_c] (3N points); G2 outputs B2_j over [L_c]G2
    SparseTerms t1, t2;
    const uint64_t no1 = 3 * (uint64_t)n;
    t1.start.assign(no1 + 1, 0);
    t2.start.assign((uint64_t)n + 1, 0);
    for (const Term& x : c.tA) { t1.start[x.s + 1]++; t1.start[2 * (uint64_t)n + x.s + 1]++; }
    for (const Term& x : c.tB) { t1.start[(uint64_t)n + x.s + 1]++; t1.start[2 * (uint64_t)n + x.s + 1]++; t2.start[x.s + 1]++; }
    for (const Term& x : c.tC) t1.start[2 * (uint64_t)n + x.s + 1]++;
    for (uint32_t i = 0; i <= p; i++) { t1.start[i + 1]++; t1.start[2 * (uint64_t)n + i + 1]++; }
    for (uint64_t o = 0; o < no1; o++) t1.start[o + 1] += t1.start[o];
    for (uint64_t o = 0; o < n; o++) t2.start[o + 1] += t2.start[o];
    t1.base.resize(t1.start[no1]);
    t1.coef.resize(t1.start[no1]);
    t2.base.resize(t2.start[n]);
    t2.coef.resize(t2.start[n]);
    std::vector<uint64_t> f1(t1.start.begin(), t1.start.end() - 1), f2(t2.start.begin(), t2.start.end() - 1);
    auto put1 = [&](uint64_t o, uint32_t b, const Fr& cf) { const uint64_t k = f1[o]++; t1.base[k] = b; t1.coef[k] = cf; };
    auto put2 = [&](uint64_t o, uint32_t b, const Fr& cf) { const uint64_t k = f2[o]++; t2.base[k] = b; t2.coef[k] = cf; };
    const uint32_t NN = (uint32_t)N;
    for (uint32_t r = 0; r < m; r++) {
      for (uint32_t k = c.rowA[r]; k < c.rowA[r + 1]; k++) {
        const Fr cf = fp_from_mont(c.tA[k].cf);
        put1(c.tA[k].s, r, cf);
        put1(2 * (uint64_t)n + c.tA[k].s, 2 * NN + r, cf);
      }
      for (uint32_t k = c.rowB[r]; k < c.rowB[r + 1]; k++) {
        const Fr cf = fp_from_mont(c.tB[k].cf);
        put1((uint64_t)n + c.tB[k].s, r, cf);
        put1(2 * (uint64_t)n + c.tB[k].s, NN + r, cf);
        put2(c.tB[k].s, r, cf);
      }
      for (uint32_t k = c.rowC[r]; k < c.rowC[r + 1]; k++)
        put1(2 * (uint64_t)n + c.tC[k].s, r, fp_from_mont(c.tC[k].cf));
    }
    Fr one = fp_zero<FrParams>();
    one.v[0] = 1;
    for (uint32_t i = 0; i <= p; i++) {   // public-input binding rows
      put1(i, m + i, one);
      put1(2 * (uint64_t)n + i, 2 * NN + m + i, one);
    }

    G16ZkeyImage im;
    if ((rc = g16_zkey_layout(c, L, im))) return rc;
    {
      uint8_t* q = im.hdr_points;
      const G1Affine g1 = g1_generator();
      const G2Affine g2 = g2_generator();
      memcpy(q, pv.sec[4].p, 64);          // alpha1 = [alpha tau^0]G1
      memcpy(q + 64, pv.sec[5].p, 64);     // beta1
      memcpy(q + 128, pv.sec[6].p, 128);   // beta2
      memcpy(q + 256, &g2, 128);         // gamma2 = [1]G2
      memcpy(q + 384, &g1, 64);          // delta1 = [1]G1
      memcpy(q + 448, &g2, 128);         // delta2 = [1]G2
    }
    const auto t0 = std::chrono::steady_clock::now();
    SparseStats s1, s2;
    std::vector<uint8_t> o1((size_t)no1 * 64);
    {
      const uint8_t* seg[3] = {lag1, alag, blag};
      const size_t segn[3] = {N, N, N};
      rc = setup_sparse_g1(device, seg, segn, 3, t1, o1.data(), &s1);
    }
    if (!rc) {
      const uint8_t* seg[1] = {lag2};
      const size_t segn[1] = {N};
      rc = setup_sparse_g2(device, seg, segn, 1, t2, im.sec[7], &s2);
    }
    if (rc) return rc;
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    memcpy(im.sec[5], o1.data(), (size_t)n * 64);
    memcpy(im.sec[6], o1.data() + (size_t)n * 64, (size_t)n * 64);
    memcpy(im.sec[3], o1.data() + (size_t)2 * n * 64, (size_t)(p + 1) * 64);
    memcpy(im.sec[8], o1.data() + ((size_t)2 * n + p + 1) * 64, ((size_t)n - p - 1) * 64);
    for (size_t i = 0; i < N; i++) memcpy(im.sec[9] + i * 64, hblk + (2 * i + 1) * 64, 64);
    if (getenv("G16_TRACE_HOST"))
      fprintf(stderr,
              "[g16 groth16 setup ptau] domain 2^%d, nnz A %zu B %zu C %zu; G1 terms: +-1 %llu short %llu full %llu zero %llu; "
              "G2 terms: +-1 %llu short %llu full %llu zero %llu; kernels G1 %.3f ms G2 %.3f ms; device wall %.3f ms\n",
              L, c.tA.size(), c.tB.size(), c.tC.size(), (unsigned long long)s1.pm1, (unsigned long long)s1.shorts,
              (unsigned long long)s1.full, (unsigned long long)s1.zero, (unsigned long long)s2.pm1,
              (unsigned long long)s2.shorts, (unsigned long long)s2.full, (unsigned long long)s2.zero, s1.kern_ms,
              s2.kern_ms, wall_ms);
    im.z.give(zkey, zkey_len);
    return G16_OK;
  });
}

extern "C" int g16_groth16_setup_ptau(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                                      int device, uint8_t** zkey, size_t* zkey_len) {
  if (!r1cs || !ptau || !zkey || !zkey_len) { set_error("NULL argument"); return G16_E_ARG; }
  return groth16_setup_ptau_checked(r1cs, r1cs_len, ptau, ptau_len, device, zkey, zkey_len, nullptr);
}

extern "C" int g16_groth16_setup_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device) {
  if (!r1cs_path || !ptau_path || !zkey_path) { set_error("NULL argument"); return G16_E_ARG; }
  const char* in[2] = {r1cs_path, ptau_path};
  return files_form(in, 2, zkey_path, [&](const MappedFile* m, uint8_t** z, size_t* zl) {
    return g16_groth16_setup_ptau((const uint8_t*)m[0].p, m[0].len, (const uint8_t*)m[1].p, m[1].len, device, z, zl);
  });
}
