// g16_wtns_check: is a witness valid for an R1CS, and if not, where does it break?  (include/g16_prover.h)
// Here: the witness parser with g16_prove's texts, the r1cs -> CSR builder of the device route (wtns_check.hip), the host
// route (device = -1, and the confirmation of every failing row a device run reports) and the verdict.
#include "wtns_check.h"

#include <thread>

#include "fixed_base.h"
#include "mapped_file.h"

using namespace g16;

struct g16_r1cs_checker {
  Circuit c;
  int device = -1;
  WcDevice* dev = nullptr;
  float ms[3] = {0.f, 0.f, 0.f};
};

namespace g16 {

void wc_build_csr(const Circuit& c, WcCsr& q) {
  q.m = c.m;
  q.n_w = c.n;
  const std::vector<uint32_t>* rows[3] = {&c.rowA, &c.rowB, &c.rowC};
  const std::vector<Term>* terms[3] = {&c.tA, &c.tB, &c.tC};
  // (the circuit holds Montgomery images: +1 is R, -1 is r - R)
  const FrM one = fr_one(), mone = fr_neg_one();
  F29 r2;
  for (int i = 0; i < 9; i++) r2.l[i] = Fr29T::R2[i];
  r2.pad_ = 0;
  for (int k = 0; k < 3; k++) {
    const std::vector<uint32_t>& rp = *rows[k];
    const std::vector<Term>& t = *terms[k];
    q.rp[k] = rp;
    q.mid[k].assign(c.m, 0);
    q.vptr[k].assign(c.m, 0);
    q.col[k].assign(t.size(), 0);
    q.val[k].clear();
    for (uint32_t r = 0; r < c.m; r++) {
      uint32_t k2 = rp[r];
      for (uint32_t i = rp[r]; i < rp[r + 1]; i++) {
        if (fp_eq(t[i].cf, one)) q.col[k][k2++] = t[i].s;
        else if (fp_eq(t[i].cf, mone)) q.col[k][k2++] = t[i].s | 0x80000000u;
      }
      q.mid[k][r] = k2;
      q.vptr[k][r] = (uint32_t)q.val[k].size();
      for (uint32_t i = rp[r]; i < rp[r + 1]; i++)
        if (!fp_eq(t[i].cf, one) && !fp_eq(t[i].cf, mone)) {
          q.col[k][k2++] = t[i].s;
          // coef * 2^261 (fr29_from_plain), once more times 2^522 / 2^261: coef * 2^522
          q.val[k].push_back(fr29_mul(fr29_from_plain(fp_from_mont(t[i].cf)), r2));
        }
    }
  }
  std::vector<uint32_t> wave_rows;
  q.long_rows.clear();
  for (uint32_t r = 0; r < c.m; r++) {
    uint32_t mx = 0;
    for (int k = 0; k < 3; k++) {
      const uint32_t l = (*rows[k])[r + 1] - (*rows[k])[r];
      if (l > mx) mx = l;
    }
    if (mx > kQapWaveRow) wave_rows.push_back(r);
    else if (mx > kQapLongRow) q.long_rows.push_back(r);
  }
  q.n_mid = (uint32_t)q.long_rows.size();
  q.long_rows.insert(q.long_rows.end(), wave_rows.begin(), wave_rows.end());
  q.n_long = (uint32_t)q.long_rows.size();
}

}  // namespace g16

// ------------------------------------------------------------------ the witness file
// wtns_utils.readHeader and the checks of groth16.prove [EXT], with g16_prove's texts; the words must be canonical
// (the device sums assume values below r) and signal 0 must be the constant 1.  *body = the n words.
static int wc_parse_wtns(uint32_t n, const uint8_t* wtns, size_t len, const uint8_t** body) {
  auto bad = [](const std::string& why) { set_error(why); return G16_E_FORMAT; };
  BinView f;
  if (const int rc = bin_open(wtns, len, "wtns", 2, f)) return rc;
  const BinSection s1 = f.sec[1], s2 = f.sec[2];
  if (!s1.p) return bad("wtns: Missing section 1");
  if (s1.size < 8) return bad("wtns: Invalid File format");
  const uint32_t n8 = rd32(s1.p);
  if (s1.size < 8 + (uint64_t)n8) return bad("wtns: Invalid File format");
  if (!bin_is_field(s1.p, s1.size, kFrP)) return bad("Curve of the witness does not match the curve of the proving key");
  const uint32_t nw = rd32(s1.p + 4 + n8);
  if (nw != n) return bad("Invalid witness length. Circuit: " + std::to_string(n) + ", witness: " + std::to_string(nw));
  if (!s2.p) return bad("wtns: Missing section 2");
  if (s2.size != (uint64_t)nw * 32) return bad("wtns: Invalid File format");
  for (uint32_t i = 0; i < nw; i++) {
    uint32_t v[8];
    memcpy(v, s2.p + (size_t)i * 32, 32);
    if (!fr_below_modulus(v)) return bad("wtns: signal " + std::to_string(i) + " is not reduced modulo the scalar field");
  }
  static const uint8_t kOne[32] = {1};
  if (nw == 0 || memcmp(s2.p, kOne, 32) != 0) return bad("wtns check: signal 0 is not 1");
  *body = s2.p;
  return G16_OK;
}

// ------------------------------------------------------------------ host route (8 x 32 Montgomery code of fp.cuh)
// the standard-form values A_r.w, B_r.w, C_r.w of one row: a Montgomery coefficient times a plain word is the plain product
static void wc_row_values(const Circuit& c, uint32_t r, const uint8_t* body, Fr out[3]) {
  const std::vector<uint32_t>* rows[3] = {&c.rowA, &c.rowB, &c.rowC};
  const std::vector<Term>* terms[3] = {&c.tA, &c.tB, &c.tC};
  for (int k = 0; k < 3; k++) {
    Fr s = fp_zero<FrParams>();
    for (uint32_t i = (*rows[k])[r]; i < (*rows[k])[r + 1]; i++) {
      const Term& t = (*terms[k])[i];
      Fr w;
      memcpy(w.v, body + (size_t)t.s * 32, 32);
      s = fp_add(s, fp_mul(t.cf, w));
    }
    out[k] = s;
  }
}
static bool wc_row_holds(const Fr v[3]) { return fp_eq(fp_mul(fp_to_mont(v[0]), v[1]), v[2]); }

static void wc_host_check(const Circuit& c, const uint8_t* body, uint32_t* first, uint32_t* n_failed) {
  const unsigned hw = std::thread::hardware_concurrency();
  const int threads = c.m < 4096 ? 1 : (int)(hw < 1 ? 1 : hw > 16 ? 16 : hw);
  std::vector<uint32_t> lo_first((size_t)threads, 0xffffffffu), cnt((size_t)threads, 0);
  const size_t per = ((size_t)c.m + threads - 1) / threads;
  parallel_for((size_t)threads, threads, [&](size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; t++) {
      const size_t lo = t * per, hi = lo + per < c.m ? lo + per : c.m;
      for (size_t r = lo; r < hi; r++) {
        Fr v[3];
        wc_row_values(c, (uint32_t)r, body, v);
        if (!wc_row_holds(v)) {
          if (lo_first[t] == 0xffffffffu) lo_first[t] = (uint32_t)r;
          cnt[t]++;
        }
      }
    }
  });
  *first = 0xffffffffu;
  *n_failed = 0;
  for (int t = 0; t < threads; t++) {
    if (lo_first[t] < *first) *first = lo_first[t];
    *n_failed += cnt[t];
  }
}

// (first, n_failed) -> the verdict; a failing row is recomputed on the host, which fills a, b, c -- and contradicts a
// device that named a satisfied row
static int wc_fill_verdict(const Circuit& c, const uint8_t* body, uint32_t first, uint32_t n_failed, g16_wtns_verdict* out) {
  memset(out, 0, sizeof(*out));
  out->constraint = -1;
  if (first == 0xffffffffu && n_failed == 0) return G16_OK;
  if (first >= c.m || n_failed == 0) {
    set_error("wtns check: the device verdict is inconsistent (row " + std::to_string(first) + ", " + std::to_string(n_failed) + " failing)");
    return G16_E_STATE;
  }
  Fr v[3];
  wc_row_values(c, first, body, v);
  if (wc_row_holds(v)) {
    set_error("wtns check: the device reports constraint " + std::to_string(first) + " as not satisfied, the host finds it satisfied");
    return G16_E_STATE;
  }
  out->constraint = (int64_t)first;
  out->n_failed = n_failed;
  memcpy(out->a, v[0].v, 32);
  memcpy(out->b, v[1].v, 32);
  memcpy(out->c, v[2].v, 32);
  return G16_OK;
}
static std::string wc_verdict_text(const g16_wtns_verdict& v) {
  return "wtns check: constraint " + std::to_string(v.constraint) + " is not satisfied (" + std::to_string(v.n_failed) + " in all)";
}

// the device route of a checker: the CSR built and uploaded, the chunk buffers allocated
static int wc_attach_device(g16_r1cs_checker* k, int device) {
  WcCsr q;
  wc_build_csr(k->c, q);
  // witnesses per chunk: what 256 MB hold at 72 bytes per wire, at most 1024 (G16_WTNS_CHECK_CHUNK overrides)
  uint32_t chunk = env_u32("G16_WTNS_CHECK_CHUNK");
  if (!chunk) {
    const uint64_t fit = ((uint64_t)256 << 20) / (72 * (uint64_t)(q.n_w ? q.n_w : 1));
    chunk = (uint32_t)(fit < 1 ? 1 : fit > 1024 ? 1024 : fit);
  }
  k->device = device;
  return wc_device_create(device, q, chunk, &k->dev);
}

// ------------------------------------------------------------------ C ABI
extern "C" int g16_r1cs_checker_create(const uint8_t* r1cs, size_t len, int device, g16_r1cs_checker** out) {
  if (!out) { set_error("wtns check: null argument"); return G16_E_ARG; }
  *out = nullptr;
  if (device < -1) { set_error("wtns check: bad device ordinal"); return G16_E_ARG; }
  return no_bad_alloc("wtns check", [&]() -> int {
    g16_r1cs_checker* k = new g16_r1cs_checker;
    k->device = device;
    int rc = read_r1cs(r1cs, len, k->c, /*allow_empty=*/true);
    if (!rc && device >= 0) rc = wc_attach_device(k, device);
    if (rc) { delete k; return rc; }
    *out = k;
    return G16_OK;
  });
}

extern "C" void g16_r1cs_checker_destroy(g16_r1cs_checker* k) {
  if (!k) return;
  wc_device_destroy(k->dev);
  delete k;
}

extern "C" int g16_wtns_check_batch(g16_r1cs_checker* k, const uint8_t* const* wtns, const size_t* lens, size_t count,
                                    g16_wtns_verdict* out) {
  if (!k || (count && (!wtns || !lens || !out))) { set_error("wtns check: null argument"); return G16_E_ARG; }
  return no_bad_alloc("wtns check", [&]() -> int {
    // every witness is parsed before the device is touched; the lowest malformed one words the error
    std::vector<const uint8_t*> body(count, nullptr);
    std::vector<int> rcs(count, 0);
    std::vector<std::string> errs(count);
    const unsigned hw = std::thread::hardware_concurrency();
    parallel_for(count, count < 2 ? 1 : (int)(hw < 1 ? 1 : hw > 16 ? 16 : hw), [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++)
        if ((rcs[i] = wc_parse_wtns(k->c.n, wtns[i], lens[i], &body[i]))) errs[i] = get_error();   // (thread-local text)
    });
    for (size_t i = 0; i < count; i++)
      if (rcs[i]) {
        set_error("witness " + std::to_string(i) + ": " + errs[i]);
        return rcs[i];
      }
    std::vector<uint32_t> first(count, 0xffffffffu), n_failed(count, 0);
    k->ms[0] = k->ms[1] = 0.f;
    if (k->dev) {
      if (const int rc = wc_device_check(k->dev, body.data(), count, first.data(), n_failed.data(), k->ms)) return rc;
    } else {
      for (size_t i = 0; i < count; i++) wc_host_check(k->c, body[i], &first[i], &n_failed[i]);
    }
    int64_t bad = -1;
    for (size_t i = 0; i < count; i++) {
      if (const int rc = wc_fill_verdict(k->c, body[i], first[i], n_failed[i], &out[i])) return rc;
      if (bad < 0 && out[i].constraint >= 0) bad = (int64_t)i;
    }
    if (bad >= 0) set_error("witness " + std::to_string(bad) + ": " + wc_verdict_text(out[bad]));
    return G16_OK;
  });
}

extern "C" int g16_wtns_check(g16_r1cs_checker* k, const uint8_t* wtns, size_t len, g16_wtns_verdict* out) {
  if (!k || !out) { set_error("wtns check: null argument"); return G16_E_ARG; }
  const uint8_t* body = nullptr;
  if (const int rc = wc_parse_wtns(k->c.n, wtns, len, &body)) return rc;
  uint32_t first = 0xffffffffu, n_failed = 0;
  k->ms[0] = k->ms[1] = 0.f;
  if (k->dev) {
    if (const int rc = wc_device_check(k->dev, &body, 1, &first, &n_failed, k->ms)) return rc;
  } else {
    wc_host_check(k->c, body, &first, &n_failed);
  }
  if (const int rc = wc_fill_verdict(k->c, body, first, n_failed, out)) return rc;
  if (out->constraint >= 0) set_error(wc_verdict_text(*out));
  return G16_OK;
}

extern "C" int g16_r1cs_checker_timings(const g16_r1cs_checker* k, float ms[2]) {
  if (!k || !ms) { set_error("wtns check: null argument"); return G16_E_ARG; }
  ms[0] = k->ms[0];
  ms[1] = k->ms[1];
  return G16_OK;
}

extern "C" int g16_wtns_check_files(const char* r1cs_path, const char* wtns_path, int device, g16_wtns_verdict* out) {
  if (!r1cs_path || !wtns_path || !out) { set_error("wtns check: null argument"); return G16_E_ARG; }
  MappedFile r, w;
  if (const int rc = r.open_ro(r1cs_path)) return rc;
  if (const int rc = w.open_ro(wtns_path)) return rc;
  // (both inputs are checked before the device is touched: the checker starts on the host route)
  g16_r1cs_checker* k = nullptr;
  if (const int rc = g16_r1cs_checker_create((const uint8_t*)r.p, r.len, -1, &k)) return rc;
  const uint8_t* body = nullptr;
  int rc = device < -1 ? G16_E_ARG : wc_parse_wtns(k->c.n, (const uint8_t*)w.p, w.len, &body);
  if (device < -1) set_error("wtns check: bad device ordinal");
  if (!rc && device >= 0) rc = no_bad_alloc("wtns check", [&]() { return wc_attach_device(k, device); });
  if (!rc) rc = g16_wtns_check(k, (const uint8_t*)w.p, w.len, out);
  g16_r1cs_checker_destroy(k);
  return rc;
}
