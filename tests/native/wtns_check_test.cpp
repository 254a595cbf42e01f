// Stand-alone test of the host side of g16_wtns_check, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_wtns_check_native.py) from csrc/wtns_check_host.cpp and csrc/circuit.cpp: the host route (device = -1), the
// r1cs -> CSR builder of the device route and the verdict plumbing.  There is no device here: the three device entry
// points are stubs that fail.  The builder's CSR is evaluated row by row with the host forms of the kernel's own
// arithmetic (fr29.cuh: +-1 records add or subtract the Montgomery image, general ones multiply, the sum weak-reduced
// every seven units) and must name the same failing rows, and the same a, b, c, as the host route, which works from
// the circuit's terms with the 8 x 32 Montgomery code.  Every input lives in a heap buffer of exactly its length, and
// the checker is fed every prefix of a witness and of an .r1cs.
#include <stdio.h>

#include "wtns_check.h"

static thread_local std::string g_err;
namespace g16 {
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }
int wc_device_create(int, const WcCsr&, uint32_t, WcDevice**) { set_error("no device in this program"); return G16_E_NOGPU; }
int wc_device_check(WcDevice*, const uint8_t* const*, size_t, uint32_t*, uint32_t*, float*) { return G16_E_NOGPU; }
void wc_device_destroy(WcDevice*) {}
}  // namespace g16
extern "C" const char* g16_last_error(void) { return g_err.c_str(); }
using namespace g16;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

struct Exact {   // a heap copy of exactly `len` bytes
  uint8_t* p;
  size_t len;
  Exact(const uint8_t* src, size_t n) : p((uint8_t*)malloc(n)), len(n) { if (n) memcpy(p, src, n); }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
};

// the kernel's row sum (qap_rows.cuh) with the host forms of its arithmetic -> the canonical value
static Fr csr_row_value(const WcCsr& q, int k, uint32_t r, const std::vector<Fr>& w) {
  F29 s = f29_zero();
  uint32_t cnt = 0;
  const uint32_t k0 = q.rp[k][r], km = q.mid[k][r], k1 = q.rp[k][r + 1];
  CHECK(k0 <= km && km <= k1 && k1 <= q.col[k].size());
  for (uint32_t i = k0; i < km; i++) {
    const uint32_t ci = q.col[k][i];
    const F29 x = fr29_from_plain(w[ci & 0x7fffffffu]);
    if (ci >> 31) { s = fr29_sub<2>(s, x); cnt += 2; }
    else { s = fr29_add(s, x); cnt += 1; }
    if (cnt >= 7) { s = fr29_weak_reduce(s); cnt = 0; }
  }
  const uint32_t vp = q.vptr[k][r];
  CHECK((size_t)vp + (k1 - km) <= q.val[k].size());
  for (uint32_t i = km; i < k1; i++) {
    s = fr29_add(s, fr29_mul(q.val[k][vp + (i - km)], fr29_repack(w[q.col[k][i]])));
    if (++cnt >= 7) { s = fr29_weak_reduce(s); cnt = 0; }
  }
  return fr29_to_plain(s);
}

static Fr std_mul(const Fr& a, const Fr& b) { return fp_mul(fp_to_mont(a), b); }   // standard form in and out

int main() {
  Xo rng(2024);
  // rows of 0 .. 400 terms on one side (across both class thresholds), the two other sides short; coefficients +1, -1, 0,
  // small and full-width; the C side of every row ends in a fresh wire with coefficient 1 that a witness can solve
  Circuit c;
  const uint32_t lens[] = {0, 1, 2, 15, 16, 17, 18, 63, 64, 65, 66, 200, 356, 400, 3, 5};
  // ... and 5000 short rows behind them, so that the host route runs on more than one thread
  const uint32_t nfree = 64, nlens = 3 * (uint32_t)(sizeof(lens) / sizeof(lens[0])), m = nlens + 5000;
  c.n = 1 + nfree + m;
  c.p = 0;
  c.m = m;
  c.rowA.assign(1, 0); c.rowB.assign(1, 0); c.rowC.assign(1, 0);
  auto coef = [&]() -> FrM {
    const uint64_t u = rng.below(10);
    if (u < 3) return fr_one();
    if (u < 6) return fr_neg_one();
    if (u == 6) return fp_zero<FrParams>();
    if (u == 7) return fr_u64(1 + rng.below(65535));
    return rng.rand_fr();
  };
  for (uint32_t r = 0; r < m; r++) {
    std::vector<Term>* side[3] = {&c.tA, &c.tB, &c.tC};
    for (int k = 0; k < 3; k++) {
      const uint32_t len = r < nlens && (int)(r % 3) == k ? lens[r / 3] : (uint32_t)rng.below(4);
      for (uint32_t t = 0; t < len; t++) side[k]->push_back({(uint32_t)rng.below(1 + nfree), coef()});
    }
    c.tC.push_back({1 + nfree + r, fr_one()});
    c.rowA.push_back((uint32_t)c.tA.size()); c.rowB.push_back((uint32_t)c.tB.size()); c.rowC.push_back((uint32_t)c.tC.size());
  }
  Buf rb = write_r1cs(c, 0, 0);
  Exact r1cs(rb.p, rb.len);

  // the file read back and the CSR built from it
  Circuit back;
  CHECK(read_r1cs(r1cs.p, r1cs.len, back, true) == G16_OK);
  CHECK(back.m == m && back.n == c.n && back.tA.size() == c.tA.size() && back.tC.size() == c.tC.size());
  WcCsr q;
  wc_build_csr(back, q);
  CHECK(q.m == m && q.n_w == c.n && q.n_long <= m && q.n_mid <= q.n_long);
  uint32_t want_mid = 0, want_long = 0;
  for (uint32_t i = 0; i < sizeof(lens) / sizeof(lens[0]); i++)
    for (uint32_t k = 0; k < 3; k++) {   // (the C side carries the row's own wire as one term more)
      const uint32_t len = lens[i] + (k == 2 ? 1 : 0);
      if (len > kQapWaveRow) want_long++;
      else if (len > kQapLongRow) want_mid++;
    }
  CHECK(q.n_mid == want_mid && q.n_long == want_mid + want_long);   // C drives the class as A and B do

  // a satisfying witness: the free wires random, the last wire of every row solved
  std::vector<Fr> w(c.n);
  w[0] = fp_zero<FrParams>();
  w[0].v[0] = 1;
  for (uint32_t i = 1; i <= nfree; i++) w[i] = rng.rand_fr_std();
  for (uint32_t r = 0; r < m; r++) {
    w[1 + nfree + r] = fp_zero<FrParams>();
    const Fr a = csr_row_value(q, 0, r, w), b = csr_row_value(q, 1, r, w), rest = csr_row_value(q, 2, r, w);
    w[1 + nfree + r] = fp_sub(std_mul(a, b), rest);
  }
  g16_r1cs_checker* k = nullptr;
  CHECK(g16_r1cs_checker_create(r1cs.p, r1cs.len, -1, &k) == G16_OK && k);
  g16_r1cs_checker* none = nullptr;
  CHECK(g16_r1cs_checker_create(r1cs.p, r1cs.len, 0, &none) == G16_E_NOGPU && !none);   // (the stub: nothing leaks)

  auto wtns_of = [&](const std::vector<Fr>& ws) {
    std::vector<FrM> wm(ws.size());
    for (size_t i = 0; i < ws.size(); i++) wm[i] = fp_to_mont(ws[i]);
    return write_wtns(wm);
  };
  // the verdict the CSR evaluation gives, against the host route's
  auto compare = [&](const std::vector<Fr>& ws) {
    int64_t first = -1;
    uint32_t n_failed = 0;
    Fr fa{}, fb{}, fc{};
    for (uint32_t r = 0; r < m; r++) {
      const Fr a = csr_row_value(q, 0, r, ws), b = csr_row_value(q, 1, r, ws), cc = csr_row_value(q, 2, r, ws);
      if (!fp_eq(std_mul(a, b), cc)) {
        if (first < 0) { first = r; fa = a; fb = b; fc = cc; }
        n_failed++;
      }
    }
    Buf wb = wtns_of(ws);
    Exact img(wb.p, wb.len);
    g16_wtns_verdict v;
    memset(&v, 0x5a, sizeof(v));
    CHECK(g16_wtns_check(k, img.p, img.len, &v) == G16_OK);
    CHECK(v.constraint == first && v.n_failed == n_failed);
    if (first >= 0) {
      CHECK(!memcmp(v.a, fa.v, 32) && !memcmp(v.b, fb.v, 32) && !memcmp(v.c, fc.v, 32));
      CHECK(g_err == "wtns check: constraint " + std::to_string(first) + " is not satisfied (" + std::to_string(n_failed) + " in all)");
    } else {
      static const uint8_t zero[32] = {0};
      CHECK(!memcmp(v.a, zero, 32) && !memcmp(v.b, zero, 32) && !memcmp(v.c, zero, 32));
    }
    return first;
  };
  CHECK(compare(w) == -1);
  for (uint32_t r : {0u, 7u, m - 1, 20u, 2600u}) {   // single rows, then several at once, then (nearly) all of them
    std::vector<Fr> bad = w;
    bad[1 + nfree + r].v[0] ^= 1;
    CHECK(compare(bad) == (int64_t)r);
  }
  {
    std::vector<Fr> bad = w;
    for (uint32_t r = 5; r < m; r += 4) bad[1 + nfree + r].v[0] ^= 1;
    CHECK(compare(bad) == 5);
    for (uint32_t i = 1; i < c.n; i++) bad[i] = rng.rand_fr_std();
    CHECK(compare(bad) >= 0);
  }

  // every prefix of a witness, alone and as the third of a batch
  {
    Buf wb = wtns_of(w);
    Exact good(wb.p, wb.len);
    for (size_t len = 0; len < wb.len; len += (len < 120 || len + 40 > wb.len) ? 1 : 97) {
      Exact cut(wb.p, len);
      g16_wtns_verdict v, vs[3];
      CHECK(g16_wtns_check(k, cut.p, cut.len, &v) == G16_E_FORMAT);
      const uint8_t* ptrs[3] = {good.p, good.p, cut.p};
      const size_t ls[3] = {good.len, good.len, cut.len};
      CHECK(g16_wtns_check_batch(k, ptrs, ls, 3, vs) == G16_E_FORMAT);
      CHECK(g_err.rfind("witness 2: ", 0) == 0);
    }
    const uint8_t* ptrs[2] = {good.p, good.p};
    const size_t ls[2] = {good.len, good.len};
    g16_wtns_verdict vs[2];
    CHECK(g16_wtns_check_batch(k, ptrs, ls, 2, vs) == G16_OK && vs[0].constraint == -1 && vs[1].constraint == -1);
  }
  g16_r1cs_checker_destroy(k);

  // every prefix of the .r1cs (sampled in its long middle): an error, never a read past the buffer
  for (size_t len = 0; len < r1cs.len; len += (len < 200 || len + 80 > r1cs.len) ? 1 : 1013) {
    Exact cut(r1cs.p, len);
    g16_r1cs_checker* kk = nullptr;
    CHECK(g16_r1cs_checker_create(cut.p, cut.len, -1, &kk) == G16_E_FORMAT && !kk);
  }
  // no constraints: every witness of the right length passes
  {
    Circuit e;
    e.n = 3; e.p = 0; e.m = 0;
    e.rowA.assign(1, 0); e.rowB.assign(1, 0); e.rowC.assign(1, 0);
    Buf eb = write_r1cs(e, 0, 0);
    Exact img(eb.p, eb.len);
    g16_r1cs_checker* kk = nullptr;
    CHECK(g16_r1cs_checker_create(img.p, img.len, -1, &kk) == G16_OK && kk);
    std::vector<Fr> ws(3, w[0]);
    Buf wb = wtns_of(ws);
    g16_wtns_verdict v;
    CHECK(g16_wtns_check(kk, wb.p, wb.len, &v) == G16_OK && v.constraint == -1 && v.n_failed == 0);
    Circuit back0;
    WcCsr q0;
    CHECK(read_r1cs(img.p, img.len, back0, true) == G16_OK && read_r1cs(img.p, img.len, back0, false) == G16_E_FORMAT);
    wc_build_csr(back0, q0);
    CHECK(q0.m == 0 && q0.n_long == 0 && q0.rp[2].size() == 1);
    g16_r1cs_checker_destroy(kk);
  }
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
