// The .r1cs reader and writer, the .wtns writer and the domain size of a circuit (circuit.h).
#include "circuit.h"

namespace g16 {

int g16_domain_log(const Circuit& c) {
  int L = 0;
  while (((uint64_t)1 << L) < (uint64_t)c.m + c.p + 1) L++;
  return L;
}

Buf write_wtns(const std::vector<FrM>& w) {
  Buf b;
  const size_t n = w.size();
  b.reserve(12 + 12 + 40 + 12 + n * 32);
  b.put("wtns", 4); b.u32(2); b.u32(2);
  b.u32(1); b.u64(40);
  b.u32(32); b.put(kFrP, 32); b.u32((uint32_t)n);
  b.u32(2); b.u64((uint64_t)n * 32);
  for (size_t i = 0; i < n; i++) {
    const Fr s = fp_from_mont(w[i]);
    b.put(s.v, 32);
  }
  return b;
}

Buf write_r1cs(const Circuit& c, uint32_t n_pub_out, uint32_t n_pub_in) {
  Buf b;
  const size_t nnz = c.tA.size() + c.tB.size() + c.tC.size();
  const size_t s1 = 4 + 32 + 16 + 8 + 4, s2 = (size_t)c.m * 12 + nnz * 36, s3 = (size_t)c.n * 8;
  b.reserve(12 + 3 * 12 + s1 + s2 + s3);
  b.put("r1cs", 4); b.u32(1); b.u32(3);
  b.u32(1); b.u64(s1);
  b.u32(32); b.put(kFrP, 32); b.u32(c.n); b.u32(n_pub_out); b.u32(n_pub_in); b.u32(c.n - 1 - n_pub_out - n_pub_in);
  b.u64(c.n); b.u32(c.m);
  b.u32(2); b.u64(s2);
  const std::vector<Term>* ts[3] = {&c.tA, &c.tB, &c.tC};
  const std::vector<uint32_t>* rs[3] = {&c.rowA, &c.rowB, &c.rowC};
  for (uint32_t r = 0; r < c.m; r++)
    for (int k = 0; k < 3; k++) {
      const uint32_t lo = (*rs[k])[r], hi = (*rs[k])[r + 1];
      b.u32(hi - lo);
      for (uint32_t t = lo; t < hi; t++) {
        b.u32((*ts[k])[t].s);
        const Fr plain = fp_from_mont((*ts[k])[t].cf);
        b.put(plain.v, 32);
      }
    }
  b.u32(3); b.u64(s3);
  for (uint32_t i = 0; i < c.n; i++) b.u64(i);
  return b;
}

// ------------------------------------------------------------------ .r1cs reader
// iden3 r1cs v1: section 1 header {n8, prime, nWires, nPubOut, nPubIn, nPrvIn, nLabels u64,
// nConstraints}, section 2 constraints: A, B, C each {nTerms u32, nTerms x (wireId u32, coef n8 LE)}.
// nPublic of the zkey = nPubOut + nPubIn ([EXT] r1csfile 0.0.35, pin /root/reference/yarn.lock:909-917).
int read_r1cs(const uint8_t* buf, size_t len, Circuit& c, bool allow_empty) {
  auto bad = [](const char* why) { set_error(std::string("r1cs: ") + why); return G16_E_FORMAT; };
  BinView f;
  BinFault why;
  if (const int rc = bin_open(buf, len, "r1cs", 1, f, &why)) {
    if (why == BinFault::table) return bad("truncated section table");
    if (why == BinFault::section) return bad("truncated section");
    return rc;
  }
  const uint8_t *s1 = f.sec[1].p, *s2 = f.sec[2].p, *s3 = f.sec[3].p;
  const uint64_t l1 = f.sec[1].size, l2 = f.sec[2].size, l3 = f.sec[3].size;
  if (!s1 || !s2 || l1 < 4 + 32 + 16 + 8 + 4) return bad("missing header or constraint section");
  if (!bin_is_field(s1, l1, kFrP)) return bad("field is not the bn128 scalar field");
  uint32_t nWires, nPubOut, nPubIn, nPrvIn, nCons;
  memcpy(&nWires, s1 + 36, 4); memcpy(&nPubOut, s1 + 40, 4); memcpy(&nPubIn, s1 + 44, 4);
  memcpy(&nPrvIn, s1 + 48, 4); memcpy(&nCons, s1 + 60, 4);
  (void)nPrvIn;
  c.n = nWires; c.p = nPubOut + nPubIn; c.m = nCons;
  if (c.n < c.p + 1 || (c.m == 0 && !allow_empty) || (uint64_t)nPubOut + nPubIn >= nWires) return bad("inconsistent header");
  // an untrusted header must not size the allocations: every constraint takes >= 12 bytes of section 2, and a wire
  // that appears nowhere still has its 8-byte entry in the wire map (section 3) when the file carries one
  if ((uint64_t)nCons * 12 > l2) return bad("constraint count exceeds the constraint section");
  if (nWires > (1u << 28)) return bad("too many wires");
  if (s3 && l3 != (uint64_t)nWires * 8) return bad("wire map does not match the wire count");
  if (!s3 && (uint64_t)nWires > l2) return bad("wire count exceeds the file");
  c.rowA.assign(1, 0); c.rowB.assign(1, 0); c.rowC.assign(1, 0);
  const uint8_t* q = s2;
  const uint8_t* end = s2 + l2;
  std::vector<Term>* dst[3] = {&c.tA, &c.tB, &c.tC};
  std::vector<uint32_t>* rows[3] = {&c.rowA, &c.rowB, &c.rowC};
  for (uint32_t r = 0; r < nCons; r++) {
    for (int k = 0; k < 3; k++) {
      if (q + 4 > end) return bad("truncated constraint");
      uint32_t nt; memcpy(&nt, q, 4); q += 4;
      if ((uint64_t)nt * 36 > (uint64_t)(end - q)) return bad("truncated constraint");
      for (uint32_t t = 0; t < nt; t++) {
        uint32_t wire; memcpy(&wire, q, 4);
        if (wire >= nWires) return bad("wire id out of range");
        Fr cf; memcpy(cf.v, q + 4, 32);
        q += 36;
        dst[k]->push_back({wire, fp_to_mont(cf)});
      }
      rows[k]->push_back((uint32_t)dst[k]->size());
    }
  }
  return G16_OK;
}

}  // namespace g16
