// The NZCP circuit library restated as a native R1CS + witness builder (VERDICT r1 "missing" 1):
// /root/reference/circuits/cbortpl.circom (GetType :26, GetX :57, GetV :79, DecodeUint23 :95, DecodeUint :115,
// ReadType :243, SkipValueScalar :266, SkipValue :306, StringEquals :375, ReadStringLength :417,
// ReadMapLength :443, CopyString :469), /root/reference/circuits/quinSelector.circom:11-42 and
// /root/reference/circuits/nzcptpl.circom (FindVCAndExp :32, FindCredSubj :141, ReadCredSubj :221,
// ConcatCredSubj :345, NZCPPubIdentity :433), plus the circomlib gadgets they include (Num2Bits, Bits2Num,
// LessThan, IsZero, IsEqual -- published semantics; the sources are fetched at build time by the reference,
// /root/reference/Makefile:14-19, and absent here) and a variable-length SHA-256 with the I/O contract of
// sha256-var-circom's Sha256Var (hash of the first `len` bits of a zero-padded bit buffer; same absent repo).
//
// NOT a port of circom: signals assigned from linear expressions stay linear combinations (what circom -O2
// leaves of them), every product is one R1CS row, and the witness is computed while the rows are emitted.  The
// constraint COUNT therefore differs from circom's; the constrained RELATION per template is the reference's,
// template by template, and is pinned by the reference's own test vectors (tests/test_cpu_nzcp_circuit.py:
// /root/reference/test/cbor.js, quinSelector.js, nzcp.js) and its golden public signals.
//
// CBuilder extends sha_builder.h's ShaBuilder; the entry points are in circuit_builders.cpp.
#pragma once
#include <unordered_map>

#include "sha_builder.h"

namespace g16 {

struct CBuilder : ShaBuilder {
  // ShaBuilder::w holds small non-negative wire values; the few wires that carry a general field element (the
  // inverse witness of IsZero, "negative" indices such as k - givenNameLen - 1) live here, Montgomery form
  std::unordered_map<uint32_t, FrM> big;
  bool ok = true;
  std::string fail;   // the first unsatisfied constraint (the reference's `assert` / `===` failing)

  // a linear combination of wires together with its value
  struct V {
    Lin lin;
    FrM val;
  };

  void violate(const std::string& what) {
    if (ok) { ok = false; fail = what; }
  }
  static bool fr_eq(const FrM& a, const FrM& b) { return memcmp(a.v, b.v, sizeof(a.v)) == 0; }
  // the value as a non-negative integer below 2^63, if it is one
  static bool small_of(const FrM& x, uint64_t& out) {
    const Fr p = fp_from_mont(x);
    for (int i = 2; i < 8; i++)
      if (p.v[i]) return false;
    out = (uint64_t)p.v[0] | ((uint64_t)p.v[1] << 32);
    return out < ((uint64_t)1 << 63);
  }
  FrM wire_val(uint32_t wire) const {
    auto it = big.find(wire);
    return it != big.end() ? it->second : fr_u64(w[wire]);
  }
  uint32_t new_wire_fr(const FrM& v) {
    uint64_t s;
    if (small_of(v, s)) return new_wire(s);
    const uint32_t wire = new_wire(0);
    big[wire] = v;
    return wire;
  }

  // ---- linear algebra on V
  static V konst(int64_t k) {
    V r;
    if (k) r.lin.t.push_back({0u, k});
    r.val = coef_of(k);
    return r;
  }
  V of_wire(uint32_t wire) const {
    V r;
    r.lin.t.push_back({wire, 1});
    r.val = wire_val(wire);
    return r;
  }
  V of_bit(const Bit& b) const {
    V r;
    add(r.lin, b, 1);
    r.val = coef_of(val(b));
    return r;
  }
  static V vadd(const V& a, const V& b) {
    V r = a;
    r.lin.t.insert(r.lin.t.end(), b.lin.t.begin(), b.lin.t.end());
    r.val = fp_add(a.val, b.val);
    return r;
  }
  static V vscale(const V& a, int64_t k) {
    V r;
    if (k)
      for (const auto& t : a.lin.t) r.lin.t.push_back({t.first, t.second * k});
    r.val = fp_mul(a.val, coef_of(k));
    return r;
  }
  static V vsub(const V& a, const V& b) { return vadd(a, vscale(b, -1)); }
  static V vaddc(const V& a, int64_t k) { return vadd(a, konst(k)); }

  // z = a * b: a fresh wire and one row
  V mul(const V& a, const V& b) {
    const uint32_t z = new_wire_fr(fp_mul(a.val, b.val));
    if (rec) rec->quad(z, a.lin.t, b.lin.t, {});
    Lin cc;
    cc.t.push_back({z, 1});
    constrain(a.lin, b.lin, cc);
    return of_wire(z);
  }
  // a === b  (circom `===`, "hardcore_assert"): one linear row; remembered when the witness violates it
  void assert_eq(const V& a, const V& b, const char* what) {
    if (!fr_eq(a.val, b.val)) violate(what);
    if (rec) rec->check(vsub(a, b).lin.t, what);
    Lin one, z;
    one.t.push_back({0u, 1});
    constrain(vsub(a, b).lin, one, z);
  }
  // a wire for a long linear combination (keeps later rows short; circom has a signal here as well)
  V settle(const V& x) {
    if (x.lin.t.size() <= 4) return x;
    const uint32_t z = new_wire_fr(x.val);
    if (rec) rec->quad(z, {}, {}, x.lin.t);
    V r = of_wire(z);
    Lin one, zero;
    one.t.push_back({0u, 1});
    constrain(vsub(x, r).lin, one, zero);
    return r;
  }

  // ---- circomlib gadgets (published semantics)
  // IsZero: inv = 1/in or 0; out = -in*inv + 1; in*out = 0
  V is_zero(const V& x) {
    const bool z = fp_is_zero(x.val);
    const uint32_t inv = new_wire_fr(z ? fp_zero<FrParams>() : fp_inv(x.val));
    const uint32_t out = new_wire(z ? 1 : 0);
    if (rec) { rec->inv0(inv, x.lin.t); rec->isz(out, x.lin.t); }
    Lin cc;                                   // in * inv = 1 - out
    cc.t.push_back({0u, 1});
    cc.t.push_back({out, -1});
    constrain(x.lin, of_wire(inv).lin, cc);
    Lin zero;                                 // in * out = 0
    constrain(x.lin, of_wire(out).lin, zero);
    return of_wire(out);
  }
  V is_equal(const V& a, const V& b) { return is_zero(vsub(b, a)); }
  // Num2Bits(n): n boolean wires with sum 2^i b_i === in.  A value that does not fit violates the constraint
  // (circom's witness generator asserts here).
  std::vector<Bit> num2bits(const V& x, int n, const char* what) {
    uint64_t v = 0;
    const bool fits = small_of(x.val, v) && (n >= 63 || v < ((uint64_t)1 << n));
    if (!fits) { violate(what); v = 0; }
    std::vector<Bit> bits((size_t)n);
    std::vector<uint32_t> targets;
    Lin sum;
    for (int i = 0; i < n; i++) {
      const uint32_t wire = new_wire((v >> i) & 1);
      targets.push_back(wire);
      boolean(wire);
      bits[(size_t)i] = bit_wire(wire);
      sum.t.push_back({wire, (int64_t)1 << i});
    }
    if (rec) rec->bits(targets.data(), (uint32_t)n, x.lin.t, what);
    V s;
    s.lin = sum;
    s.val = x.val;
    Lin one, zero;
    one.t.push_back({0u, 1});
    constrain(vsub(s, x).lin, one, zero);
    return bits;
  }
  V bits2num(const std::vector<Bit>& bits, int lo, int n) const {   // sum_{i<n} 2^i bits[lo + i]
    V r = konst(0);
    for (int i = 0; i < n; i++) r = vadd(r, vscale(of_bit(bits[(size_t)(lo + i)]), (int64_t)1 << i));
    return r;
  }
  // LessThan(n): Num2Bits(n+1)(in0 + 2^n - in1), out = 1 - top bit
  V less_than(int n, const V& a, const V& b, const char* what) {
    const V t = vsub(vaddc(a, (int64_t)1 << n), b);
    const std::vector<Bit> bits = num2bits(t, n + 1, what);
    return vsub(konst(1), of_bit(bits[(size_t)n]));
  }
  static int log2_floor(uint64_t x) {   // /root/reference/circuits/log2.circom:5-12
    int z = -1;
    while (x) { z++; x >>= 1; }
    return z;
  }

  // ---- quinSelector.circom:11-42
  V quin_selector(const std::vector<V>& in, const V& index) {
    const size_t choices = in.size();
    if (choices == 0) return konst(0);
    const int bits = log2_floor(choices) + 1;
    assert_eq(less_than(bits, index, konst((int64_t)choices), "QuinSelector: index out of range"), konst(1),
              "QuinSelector: index < choices");
    V sum = konst(0);
    for (size_t i = 0; i < choices; i++) {
      const V eq = is_zero(vsub(konst((int64_t)i), index));
      sum = vadd(sum, mul(eq, in[i]));
    }
    return settle(sum);
  }

  // ---- cbortpl.circom
  static constexpr int kTypeInt = 0, kTypeString = 3, kTypeArray = 4, kTypeMap = 5;
  V get_type(const V& v) {   // :26  v >> 5
    const std::vector<Bit> b = num2bits(v, 8, "GetType: v is not a byte");
    return bits2num(b, 5, 3);
  }
  V get_x(const V& v) {      // :57  v & 31
    const std::vector<Bit> b = num2bits(v, 8, "GetX: v is not a byte");
    return bits2num(b, 0, 5);
  }
  V get_v(const std::vector<V>& bytes, const V& pos) { return quin_selector(bytes, pos); }   // :79
  V decode_uint23(const V& v) {   // :95
    const V x = get_x(v);
    assert_eq(less_than(8, x, konst(24), "DecodeUint23"), konst(1), "DecodeUint23: x < 24");
    return x;
  }
  struct UintOut { V value, next_pos; };
  UintOut decode_uint(const std::vector<V>& bytes, const V& pos, const V& v) {   // :115
    const V x = get_x(v);
    const V c23 = less_than(8, x, konst(24), "DecodeUint: x");
    const V c24 = is_equal(x, konst(24)), c25 = is_equal(x, konst(25)), c26 = is_equal(x, konst(26));
    // x == 24
    const V v24 = get_v(bytes, mul(c24, pos));
    // x == 25
    const V v25 = vadd(vscale(get_v(bytes, mul(c25, pos)), 256), get_v(bytes, mul(c25, vaddc(pos, 1))));
    // x == 26
    const V v26 = vadd(vadd(vscale(get_v(bytes, mul(c26, pos)), 16777216), vscale(get_v(bytes, mul(c26, vaddc(pos, 1))), 65536)),
                       vadd(vscale(get_v(bytes, mul(c26, vaddc(pos, 2))), 256), get_v(bytes, mul(c26, vaddc(pos, 3)))));
    UintOut o;
    o.value = settle(vadd(vadd(mul(c23, x), mul(c24, v24)), vadd(mul(c25, v25), mul(c26, v26))));
    o.next_pos = settle(vadd(vadd(mul(c23, pos), mul(c24, vaddc(pos, 1))), vadd(mul(c25, vaddc(pos, 2)), mul(c26, vaddc(pos, 4)))));
    return o;
  }
  struct TypeOut { V next_pos, type, v; };
  TypeOut read_type(const std::vector<V>& bytes, const V& pos) {   // :243
    TypeOut o;
    o.v = get_v(bytes, pos);
    o.type = get_type(o.v);
    o.next_pos = vaddc(pos, 1);
    return o;
  }
  V skip_value_scalar(const std::vector<V>& bytes, const V& pos) {   // :266
    const TypeOut rt = read_type(bytes, pos);
    const UintOut du = decode_uint(bytes, rt.next_pos, rt.v);
    const V is_int = is_equal(rt.type, konst(kTypeInt)), is_str = is_equal(rt.type, konst(kTypeString));
    return settle(vadd(mul(is_int, du.next_pos), mul(is_str, vadd(du.next_pos, du.value))));
  }
  V skip_value(const std::vector<V>& bytes, const V& pos, uint32_t max_array_len) {   // :306
    const TypeOut rt = read_type(bytes, pos);
    const UintOut du = decode_uint(bytes, rt.next_pos, rt.v);
    const V is_int = is_equal(rt.type, konst(kTypeInt)), is_str = is_equal(rt.type, konst(kTypeString));
    const V is_arr = is_equal(rt.type, konst(kTypeArray));
    V arr_term = konst(0);
    if (max_array_len) {
      std::vector<V> next((size_t)max_array_len);
      const V n_arr = mul(is_arr, du.value);
      const int bits = log2_floor(max_array_len) + 1;
      for (uint32_t i = 0; i < max_array_len; i++) {
        const V consider = mul(is_arr, less_than(bits, konst((int64_t)i), n_arr, "SkipValue: array length"));
        const V p = mul(i == 0 ? du.next_pos : next[(size_t)i - 1], consider);
        next[(size_t)i] = skip_value_scalar(bytes, p);
      }
      const V idx = mul(is_arr, vaddc(du.value, -1));
      arr_term = mul(is_arr, quin_selector(next, idx));
    }
    return settle(vadd(vadd(mul(is_int, du.next_pos), mul(is_str, vadd(du.next_pos, du.value))), arr_term));
  }
  V string_equals(const std::vector<V>& bytes, const V& pos, const V& len, const uint8_t* cbytes, uint32_t clen) {   // :375
    V sum = is_equal(len, konst((int64_t)clen));
    for (uint32_t i = 0; i < clen; i++)
      sum = vadd(sum, is_equal(konst((int64_t)cbytes[i]), get_v(bytes, vaddc(pos, (int64_t)i))));
    return is_zero(vsub(konst((int64_t)clen + 1), sum));
  }
  struct LenOut { V len, next_pos; };
  LenOut read_string_length(const std::vector<V>& bytes, const V& pos) {   // :417
    const TypeOut rt = read_type(bytes, pos);
    assert_eq(rt.type, konst(kTypeString), "ReadStringLength: not a string");
    LenOut o;
    o.next_pos = rt.next_pos;
    o.len = decode_uint(bytes, rt.next_pos, rt.v).value;
    return o;
  }
  LenOut read_map_length(const std::vector<V>& bytes, const V& pos) {   // :443
    const TypeOut rt = read_type(bytes, pos);
    assert_eq(rt.type, konst(kTypeMap), "ReadMapLength: not a map");
    LenOut o;
    o.next_pos = rt.next_pos;
    o.len = decode_uint23(rt.v);
    return o;
  }
  struct CopyOut { std::vector<V> out; V next_pos, len; };
  CopyOut copy_string(const std::vector<V>& bytes, const V& pos, uint32_t max_len) {   // :469
    const LenOut rs = read_string_length(bytes, pos);
    CopyOut o;
    o.out.resize((size_t)max_len);
    const int bits = log2_floor(max_len) + 1;
    for (uint32_t i = 0; i < max_len; i++) {
      const V ch = get_v(bytes, vaddc(rs.next_pos, (int64_t)i));
      o.out[(size_t)i] = mul(ch, less_than(bits, konst((int64_t)i), rs.len, "CopyString: length"));
    }
    o.next_pos = vadd(rs.next_pos, rs.len);
    o.len = rs.len;
    return o;
  }

  // ---- nzcptpl.circom
  struct FindOut { V needle_pos, exp_pos; };
  // FindVCAndExp :32 (needle "vc", also the position of claim key 4 = exp) and FindCredSubj :141 (needle
  // "credentialSubject") are the same loop; with_exp selects the former
  FindOut find_in_map(const std::vector<V>& bytes, const V& pos, const V& map_len, uint32_t max_arr, uint32_t max_map,
                      const uint8_t* needle, uint32_t needle_len, bool with_exp) {
    V found = konst(0), exp_found = konst(0), p = pos;
    for (uint32_t k = 0; k < max_map; k++) {
      const TypeOut rt = read_type(bytes, p);
      const UintOut du = decode_uint(bytes, rt.next_pos, rt.v);
      const V is_str = is_equal(rt.type, konst(kTypeString));
      const V next = skip_value(bytes, vadd(du.next_pos, mul(du.value, is_str)), max_arr);
      const V is_needle_str = string_equals(bytes, du.next_pos, du.value, needle, needle_len);
      const V within = less_than(8, konst((int64_t)k), map_len, "Find*: map length");
      const V accepted = mul(mul(is_str, is_needle_str), within);
      found = vadd(found, mul(accepted, vadd(du.next_pos, du.value)));
      if (with_exp) {
        const V is_int = is_equal(rt.type, konst(kTypeInt));
        const V is4 = is_equal(konst(4), du.value);
        const V exp_acc = mul(mul(is_int, is4), within);
        exp_found = vadd(exp_found, mul(exp_acc, du.next_pos));
      }
      p = next;
    }
    FindOut o;
    o.needle_pos = settle(found);
    o.exp_pos = settle(exp_found);
    return o;
  }
  struct CredSubj { std::vector<V> given, family, dob; V given_len, family_len, dob_len; };
  CredSubj read_cred_subj(const std::vector<V>& bytes, const V& pos, const V& map_len, uint32_t max_buffer_len) {   // :221
    static const uint8_t kGiven[9] = {103, 105, 118, 101, 110, 78, 97, 109, 101};
    static const uint8_t kFamily[10] = {102, 97, 109, 105, 108, 121, 78, 97, 109, 101};
    static const uint8_t kDob[3] = {100, 111, 98};
    const uint32_t max_str = max_buffer_len / 3;
    assert_eq(map_len, konst(3), "ReadCredSubj: credentialSubject map length is not 3");
    V is_g[3], is_f[3], is_d[3];
    CopyOut cs[3];
    for (int k = 0; k < 3; k++) {
      const LenOut rs = read_string_length(bytes, k == 0 ? pos : cs[k - 1].next_pos);
      is_g[k] = string_equals(bytes, rs.next_pos, rs.len, kGiven, 9);
      is_f[k] = string_equals(bytes, rs.next_pos, rs.len, kFamily, 10);
      is_d[k] = string_equals(bytes, rs.next_pos, rs.len, kDob, 3);
      cs[k] = copy_string(bytes, vadd(rs.next_pos, rs.len), max_str);
    }
    CredSubj o;
    auto pick = [&](const V sel[3], std::vector<V>& out, V& out_len) {
      out.assign((size_t)max_buffer_len, konst(0));
      for (uint32_t h = 0; h < max_str; h++) {
        V s = konst(0);
        for (int i = 0; i < 3; i++) s = vadd(s, mul(sel[i], cs[i].out[(size_t)h]));
        out[(size_t)h] = settle(s);
      }
      V l = konst(0);
      for (int i = 0; i < 3; i++) l = vadd(l, mul(sel[i], cs[i].len));
      out_len = settle(l);
    };
    pick(is_g, o.given, o.given_len);
    pick(is_f, o.family, o.family_len);
    pick(is_d, o.dob, o.dob_len);
    return o;
  }
  struct Concat { std::vector<V> result; V result_len; };
  Concat concat_cred_subj(const CredSubj& c, uint32_t max_buffer_len) {   // :345
    const int bits = log2_floor(max_buffer_len) + 1;
    const V sep1_end = vaddc(c.given_len, 1), fam_end = vadd(sep1_end, c.family_len), sep2_end = vaddc(fam_end, 1);
    Concat o;
    o.result.resize((size_t)max_buffer_len);
    auto not_of = [&](const V& x) { return vsub(konst(1), x); };
    for (uint32_t k = 0; k < max_buffer_len; k++) {
      const V kk = konst((int64_t)k);
      const V is_given = less_than(bits, kk, c.given_len, "ConcatCredSubj");
      const V under_sep1 = less_than(bits, kk, sep1_end, "ConcatCredSubj");
      const V under_fam = less_than(bits, kk, fam_end, "ConcatCredSubj");
      const V under_sep2 = less_than(bits, kk, sep2_end, "ConcatCredSubj");
      const V g_ch = quin_selector(c.given, kk);
      const V f_ch = quin_selector(c.family, vsub(kk, sep1_end));
      const V d_ch = quin_selector(c.dob, vsub(kk, sep2_end));
      const V is_sep1 = mul(under_sep1, not_of(is_given));
      const V is_fam = mul(under_fam, not_of(under_sep1));
      const V is_sep2 = mul(under_sep2, not_of(under_fam));
      const V is_dob = not_of(under_sep2);
      V r = mul(is_given, g_ch);
      r = vadd(r, vscale(is_sep1, 44));
      r = vadd(r, mul(is_fam, f_ch));
      r = vadd(r, vscale(is_sep2, 44));
      r = vadd(r, mul(is_dob, d_ch));
      o.result[(size_t)k] = settle(r);
    }
    o.result_len = vadd(vaddc(sep2_end, 0), c.dob_len);
    return o;
  }

  // ---- variable-length SHA-256 (the contract of Sha256Var(BlockSpace), nzcptpl.circom:494-500, :591-600):
  // digest of the first len_bits bits (a multiple of 8) of `in` (512 * 2^block_space bits, MSB-first per byte).
  // The FIPS 180-4 padding is built in-circuit: byte j keeps its bits while j < len/8, the byte at len/8 becomes
  // 0x80, everything after is 0; the block that ends the padded message gets len in its last 64 bits; all
  // 2^block_space compressions are chained and the state after that block is selected.  out_base: the 256 digest
  // bits land on the wires from out_base on (MSB-first).
  void sha256_var(const std::vector<Bit>& in, const V& len_bits, int block_space, uint32_t out_base) {
    using Word = ShaBuilder::Word;
    const uint32_t nblk = 1u << block_space, nbytes = 64 * nblk;
    const int lbits = 9 + block_space + 1;                     // len_bits <= 512 * nblk
    // len_bits = 8 * len_bytes: decompose, the low three bits must be zero
    const std::vector<Bit> lb = num2bits(len_bits, lbits, "Sha256Var: length out of range");
    for (int i = 0; i < 3; i++) assert_eq(of_bit(lb[(size_t)i]), konst(0), "Sha256Var: length is not a whole number of bytes");
    const V len_bytes = bits2num(lb, 3, lbits - 3);
    // final block index fb = (len_bits + 64) >> 9 (the 0x80 byte and the 64-bit length must fit)
    const std::vector<Bit> fbits = num2bits(vaddc(len_bits, 64), lbits + 1, "Sha256Var: length");
    const V fb = bits2num(fbits, 9, lbits + 1 - 9);
    assert_eq(less_than(block_space + 2, fb, konst((int64_t)nblk), "Sha256Var: message too long"), konst(1),
              "Sha256Var: message does not fit the block space");
    std::vector<V> is_final((size_t)nblk);
    for (uint32_t b = 0; b < nblk; b++) is_final[(size_t)b] = is_equal(fb, konst((int64_t)b));
    // padded message bits
    const int jbits = log2_floor(nbytes) + 1;
    std::vector<Bit> pm((size_t)nbytes * 8);
    for (uint32_t j = 0; j < nbytes; j++) {
      const V lt = less_than(jbits, konst((int64_t)j), len_bytes, "Sha256Var: byte index");
      const V eq = is_equal(konst((int64_t)j), len_bytes);
      for (int i = 0; i < 8; i++) {
        V bitv = mul(of_bit(in[(size_t)j * 8 + (size_t)i]), lt);
        if (i == 0) bitv = vadd(bitv, eq);                     // the 0x80 marker (lt and eq exclude each other)
        // a boolean wire for the padded bit (the compression gadgets take wires)
        const uint32_t wire = new_wire((uint64_t)val_small(bitv));
        if (rec) rec->quad(wire, {}, {}, bitv.lin.t);
        Lin one, zero;
        one.t.push_back({0u, 1});
        constrain(vsub(bitv, of_wire(wire)).lin, one, zero);
        pm[(size_t)j * 8 + (size_t)i] = bit_wire(wire);
      }
    }
    Word st[8];
    for (int j = 0; j < 8; j++) st[j] = ShaBuilder::word_const(kShaIV[j]);
    std::vector<std::array<Word, 8>> states((size_t)nblk);
    for (uint32_t blk = 0; blk < nblk; blk++) {
      Word W16[16], out[8];
      for (int j = 0; j < 16; j++)
        for (int k = 0; k < 32; k++) W16[j][31 - k] = pm[(size_t)blk * 512 + 32 * (size_t)j + (size_t)k];
      // the length field: the low lbits bits of word 15 (len_bits < 2^lbits <= 2^13) when this is the final block
      for (int i = 0; i < lbits; i++) {
        const V lv = mul(is_final[(size_t)blk], of_bit(lb[(size_t)i]));
        const V sum = vadd(of_bit(W16[15][i]), lv);            // the padded data is 0 there when the block is final
        const uint32_t wire = new_wire((uint64_t)val_small(sum));
        if (rec) rec->quad(wire, {}, {}, sum.lin.t);
        boolean(wire);
        Lin one, zero;
        one.t.push_back({0u, 1});
        constrain(vsub(sum, of_wire(wire)).lin, one, zero);
        W16[15][i] = bit_wire(wire);
      }
      sha_compress(*this, st, W16, out, 0u);
      for (int j = 0; j < 8; j++) { st[j] = out[j]; states[(size_t)blk][(size_t)j] = out[j]; }
    }
    // digest = the state after block fb
    for (int j = 0; j < 8; j++)
      for (int i = 0; i < 32; i++) {
        V s = konst(0);
        for (uint32_t b = 0; b < nblk; b++) s = vadd(s, mul(is_final[(size_t)b], of_bit(states[(size_t)b][(size_t)j][i])));
        const uint32_t wire = out_base + 32 * (uint32_t)j + (uint32_t)(31 - i);
        w[wire] = (uint64_t)val_small(s);
        if (rec) rec->quad(wire, {}, {}, s.lin.t);
        Lin one, zero;
        one.t.push_back({0u, 1});
        constrain(vsub(s, of_wire(wire)).lin, one, zero);
      }
  }
  int64_t val_small(const V& x) {
    uint64_t s = 0;
    if (!small_of(x.val, s)) { violate("internal: a bit-valued expression is not small"); return 0; }
    return (int64_t)s;
  }

  // ---- NZCPPubIdentity :433.  Wires: 0 = one; 1..256 credSubjSha256, 257..512 toBeSignedSha256, 513 exp (the
  // public signals, /root/reference/test/nzcp.js:41-47); then the private inputs toBeSigned[MaxBits] (MSB-first
  // bits, zero beyond the length) and toBeSignedLen.
  void nzcp_pub_identity(bool is_live, uint32_t max_tbs_bytes, uint32_t max_arr_vc, uint32_t max_map_vc,
                         uint32_t max_arr_cs, uint32_t max_map_cs, uint32_t cs_buffer_space, const uint8_t* tbs,
                         uint32_t tbs_len) {
    const uint32_t claims_skip = is_live ? 30 : 27;
    const int tbs_block_space = 3;
    const uint32_t max_bits = max_tbs_bytes * 8;
    const uint32_t cs_max_buffer = 1u << cs_buffer_space;
    for (int i = 0; i < 512; i++) new_wire(0);
    const uint32_t exp_wire = new_wire(0);
    std::vector<Bit> in_bits((size_t)512 * (1u << tbs_block_space), bit_const(0));
    for (uint32_t k = 0; k < max_bits; k++) {
      const uint32_t byte = k / 8;
      const uint32_t wire = new_wire(byte < tbs_len ? (tbs[byte] >> (7 - (k & 7))) & 1 : 0);
      if (rec) rec->input(wire);
      boolean(wire);                                          // :470  toBeSigned[i] * (toBeSigned[i] - 1) === 0
      in_bits[(size_t)k] = bit_wire(wire);
    }
    const V len = of_wire(new_wire(tbs_len));
    if (rec) {
      rec->name_inputs("toBeSigned", max_bits);
      rec->input(len.lin.t[0].first);
      rec->name_inputs("toBeSignedLen", 1);
    }
    // :477  toBeSignedLen < MaxToBeSignedBytes + 1
    assert_eq(less_than(log2_floor(max_tbs_bytes + 1) + 1, len, konst((int64_t)max_tbs_bytes + 1), "toBeSignedLen"),
              konst(1), "toBeSignedLen exceeds MaxToBeSignedBytes");
    // :485  ToBeSigned hash
    sha256_var(in_bits, vscale(len, 8), tbs_block_space, 257);
    // :503  bits -> bytes, zeroed after the length
    std::vector<V> bytes((size_t)max_tbs_bytes);
    const int kb = log2_floor(max_tbs_bytes) + 1;
    for (uint32_t k = 0; k < max_tbs_bytes; k++) {
      V b = konst(0);
      for (int i = 0; i < 8; i++) b = vadd(b, vscale(of_bit(in_bits[(size_t)k * 8 + (size_t)(7 - i)]), (int64_t)1 << i));
      bytes[(size_t)k] = mul(b, less_than(kb, konst((int64_t)k), len, "ToBeSigned byte index"));
    }
    const LenOut claims = read_map_length(bytes, konst((int64_t)claims_skip));
    static const uint8_t kVC[2] = {118, 99};
    static const uint8_t kCS[17] = {99, 114, 101, 100, 101, 110, 116, 105, 97, 108, 83, 117, 98, 106, 101, 99, 116};
    const FindOut fv = find_in_map(bytes, claims.next_pos, claims.len, max_arr_vc, max_map_vc, kVC, 2, true);
    // :544  exp
    const TypeOut ert = read_type(bytes, fv.exp_pos);
    const UintOut edu = decode_uint(bytes, ert.next_pos, ert.v);
    {
      uint64_t e = 0;
      if (!small_of(edu.value.val, e)) violate("exp is not a small integer");
      w[exp_wire] = e;
      if (rec) rec->quad(exp_wire, {}, {}, edu.value.lin.t);
      Lin one, zero;
      one.t.push_back({0u, 1});
      constrain(vsub(edu.value, of_wire(exp_wire)).lin, one, zero);
    }
    // :554  credential subject
    const LenOut vc = read_map_length(bytes, fv.needle_pos);
    const FindOut fc = find_in_map(bytes, vc.next_pos, vc.len, max_arr_cs, max_map_cs, kCS, 17, false);
    const LenOut csm = read_map_length(bytes, fc.needle_pos);
    const CredSubj cs = read_cred_subj(bytes, csm.next_pos, csm.len, cs_max_buffer);
    const Concat cc = concat_cred_subj(cs, cs_max_buffer);
    // :579  concat string -> bits -> hash
    std::vector<Bit> cbits((size_t)1024, bit_const(0));
    for (uint32_t k = 0; k < cs_max_buffer; k++) {
      const std::vector<Bit> b = num2bits(cc.result[(size_t)k], 8, "credential subject character is not a byte");
      for (int j = 0; j < 8; j++) cbits[(size_t)k * 8 + (size_t)(7 - j)] = b[(size_t)j];
    }
    sha256_var(cbits, vscale(cc.result_len, 8), 1, 1);
    if (rec)
      for (uint32_t i = 1; i <= 513; i++) rec->outputs.push_back(i);
    c.n = (uint32_t)w.size();
    c.p = 513;
    c.m = (uint32_t)c.rowA.size() - 1;
  }
};

}  // namespace g16
