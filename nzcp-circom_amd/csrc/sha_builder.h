// Bit-level R1CS + witness builder and its SHA-256 (described in circuit_builders.cpp); CBuilder extends it.
#pragma once
#include <algorithm>
#include <array>

#include "circuit.h"
#include "witness_program.h"

namespace g16 {

struct Lin { std::vector<std::pair<uint32_t, int64_t>> t; };   // sum of coef * wire (wire 0 = the constant 1)
struct Bit { int32_t wire; int8_t a, b; };                     // value = a * w[wire] + b,  a in {0, 1, -1}
inline Bit bit_const(int v) { return Bit{0, 0, (int8_t)v}; }
inline Bit bit_wire(uint32_t w) { return Bit{(int32_t)w, 1, 0}; }
inline Bit bit_not(const Bit& x) { return Bit{x.wire, (int8_t)-x.a, (int8_t)(1 - x.b)}; }
inline bool bit_is_const(const Bit& x) { return x.a == 0; }

struct ShaBuilder {
  std::vector<uint64_t> w;       // witness: one bit per wire (the NZCP circuit's `exp` output is the one wider value)
  Circuit c;
  WpRecorder* rec = nullptr;     // when set, every wire's computation is appended to it (witness_program.h); rows and wires are the same either way
  FrM pow2[40];                  // 2^k in Montgomery form, and small-coefficient cache
  ShaBuilder() {
    w.push_back(1);              // wire 0
    c.rowA.assign(1, 0); c.rowB.assign(1, 0); c.rowC.assign(1, 0);
  }
  int val(const Bit& x) const { return x.a * (int)w[x.wire] + x.b; }
  FrM wire_val(uint32_t i) const { return w[i] == 0 ? fp_zero<FrParams>() : (w[i] == 1 ? fr_one() : fr_u64(w[i])); }
  uint32_t new_wire(uint64_t v) { w.push_back(v); return (uint32_t)w.size() - 1; }
  static FrM coef_of(int64_t v) { return v >= 0 ? fr_u64((uint64_t)v) : fp_neg(fr_u64((uint64_t)(-v))); }
  static void add(Lin& l, const Bit& x, int64_t mul) {
    if (x.a) l.t.push_back({(uint32_t)x.wire, mul * x.a});
    if (x.b) l.t.push_back({0u, mul * x.b});
  }
  void push(std::vector<Term>& dst, std::vector<uint32_t>& rows, Lin& l) {
    // merge duplicate wires (the constant wire shows up several times), drop zeros
    std::sort(l.t.begin(), l.t.end());
    size_t i = 0;
    while (i < l.t.size()) {
      int64_t sum = 0;
      const uint32_t wire = l.t[i].first;
      while (i < l.t.size() && l.t[i].first == wire) sum += l.t[i++].second;
      if (sum) dst.push_back({wire, coef_of(sum)});
    }
    rows.push_back((uint32_t)dst.size());
  }
  void constrain(Lin a, Lin b, Lin cc) {   // <a,w> * <b,w> = <cc,w>
    push(c.tA, c.rowA, a); push(c.tB, c.rowB, b); push(c.tC, c.rowC, cc);
  }
  void boolean(uint32_t wire) {   // b * (b - 1) = 0
    Lin a, b, z;
    a.t.push_back({wire, 1});
    b.t.push_back({wire, 1}); b.t.push_back({0u, -1});
    constrain(a, b, z);
  }
  Bit xor2(const Bit& x, const Bit& y) {
    if (bit_is_const(x)) return x.b ? bit_not(y) : y;
    if (bit_is_const(y)) return y.b ? bit_not(x) : x;
    const uint32_t z = new_wire(val(x) ^ val(y));
    Lin a, b, cc;                 // (2x) * y = x + y - z
    add(a, x, 2); add(b, y, 1); add(cc, x, 1); add(cc, y, 1);
    if (rec) { Lin m; add(m, x, -2); rec->quad(z, m.t, b.t, cc.t); }   // z = (-2x) y + x + y
    cc.t.push_back({z, -1});
    constrain(a, b, cc);
    return bit_wire(z);
  }
  Bit xor3(const Bit& x, const Bit& y, const Bit& z) { return xor2(xor2(x, y), z); }
  Bit ch(const Bit& e, const Bit& f, const Bit& g) {   // e ? f : g  =  g + e (f - g)
    const uint32_t o = new_wire(val(e) ? val(f) : val(g));
    Lin a, b, cc;
    add(a, e, 1); add(b, f, 1); add(b, g, -1); cc.t.push_back({o, 1}); add(cc, g, -1);
    if (rec) { Lin gl; add(gl, g, 1); rec->quad(o, a.t, b.t, gl.t); }
    constrain(a, b, cc);
    return bit_wire(o);
  }
  Bit maj(const Bit& x, const Bit& y, const Bit& z) {  // mid = x y ; out = mid + z (x + y - 2 mid)
    const uint32_t mid = new_wire(val(x) & val(y));
    {
      Lin a, b, cc;
      add(a, x, 1); add(b, y, 1); cc.t.push_back({mid, 1});
      if (rec) rec->quad(mid, a.t, b.t, {});
      constrain(a, b, cc);
    }
    const int vx = val(x), vy = val(y), vz = val(z);
    const uint32_t o = new_wire((vx & vy) | (vx & vz) | (vy & vz));
    Lin a, b, cc;
    add(a, z, 1); add(b, x, 1); add(b, y, 1); b.t.push_back({mid, -2}); cc.t.push_back({o, 1}); cc.t.push_back({mid, -1});
    if (rec) rec->quad(o, a.t, b.t, {{mid, 1}});
    constrain(a, b, cc);
    return bit_wire(o);
  }
  using Word = std::array<Bit, 32>;   // bit i has weight 2^i
  static Word word_const(uint32_t v) {
    Word r;
    for (int i = 0; i < 32; i++) r[i] = bit_const((v >> i) & 1);
    return r;
  }
  static Word rotr(const Word& x, int k) { Word r; for (int i = 0; i < 32; i++) r[i] = x[(i + k) & 31]; return r; }
  static Word shr(const Word& x, int k) { Word r; for (int i = 0; i < 32; i++) r[i] = i + k < 32 ? x[i + k] : bit_const(0); return r; }
  Word xor3w(const Word& a, const Word& b, const Word& d) { Word r; for (int i = 0; i < 32; i++) r[i] = xor3(a[i], b[i], d[i]); return r; }
  uint32_t word_val(const Word& x) const { uint32_t v = 0; for (int i = 0; i < 32; i++) v |= (uint32_t)val(x[i]) << i; return v; }
  // sum of the operands mod 2^32: result bits (fresh wires, or `out_wires` when given) and carry bits are
  // constrained boolean; one linear row ties them to the operands
  Word add_mod32(const std::vector<Word>& ops, const uint32_t* out_wires = nullptr) {
    uint64_t sum = 0;
    for (const Word& o : ops) sum += word_val(o);
    int ncarry = 0;
    while (((uint64_t)ops.size() << 32) > ((uint64_t)1 << (32 + ncarry))) ncarry++;
    Lin a, b, z;
    for (const Word& o : ops)
      for (int i = 0; i < 32; i++) add(a, o[i], (int64_t)1 << i);
    Word r;
    uint32_t targets[64];
    const Lin operands = rec ? a : Lin();
    for (int i = 0; i < 32 + ncarry; i++) {
      const int v = (int)((sum >> i) & 1);
      uint32_t wire;
      if (i < 32 && out_wires) { wire = out_wires[i]; w[wire] = (uint64_t)v; }
      else wire = new_wire(v);
      boolean(wire);
      targets[i] = wire;
      a.t.push_back({wire, -((int64_t)1 << i)});
      if (i < 32) r[i] = bit_wire(wire);
    }
    if (rec) rec->bits(targets, (uint32_t)(32 + ncarry), operands.t, nullptr);   // (bit operands: the sum always fits)
    b.t.push_back({0u, 1});
    constrain(a, b, z);
    return r;
  }
};

inline const uint32_t kShaK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
inline const uint32_t kShaIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

// One compression: out = st + rounds(st, W16).
inline void sha_compress(ShaBuilder& sb, const ShaBuilder::Word st[8], const ShaBuilder::Word W16[16], ShaBuilder::Word out[8],
                  uint32_t out_base) {   // out_base != 0: the result bits are the 256 wires from out_base on
  using Word = ShaBuilder::Word;
  Word W[64];
  for (int j = 0; j < 16; j++) W[j] = W16[j];
  for (int t = 16; t < 64; t++) {
    const Word s0 = sb.xor3w(ShaBuilder::rotr(W[t - 15], 7), ShaBuilder::rotr(W[t - 15], 18), ShaBuilder::shr(W[t - 15], 3));
    const Word s1 = sb.xor3w(ShaBuilder::rotr(W[t - 2], 17), ShaBuilder::rotr(W[t - 2], 19), ShaBuilder::shr(W[t - 2], 10));
    W[t] = sb.add_mod32({W[t - 16], s0, W[t - 7], s1});
  }
  Word a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  for (int t = 0; t < 64; t++) {
    const Word S1 = sb.xor3w(ShaBuilder::rotr(e, 6), ShaBuilder::rotr(e, 11), ShaBuilder::rotr(e, 25));
    Word chw, mjw;
    for (int i = 0; i < 32; i++) chw[i] = bit_is_const(e[i]) ? (e[i].b ? f[i] : g[i]) : sb.ch(e[i], f[i], g[i]);
    const Word S0 = sb.xor3w(ShaBuilder::rotr(a, 2), ShaBuilder::rotr(a, 13), ShaBuilder::rotr(a, 22));
    for (int i = 0; i < 32; i++) {
      if (bit_is_const(a[i]) && bit_is_const(b[i]) && bit_is_const(c[i]))
        mjw[i] = bit_const((a[i].b & b[i].b) | (a[i].b & c[i].b) | (b[i].b & c[i].b));
      else
        mjw[i] = sb.maj(a[i], b[i], c[i]);
    }
    const Word kw = ShaBuilder::word_const(kShaK[t]);
    const Word ne = sb.add_mod32({d, h, S1, chw, kw, W[t]});
    const Word na = sb.add_mod32({h, S1, chw, kw, W[t], S0, mjw});
    h = g; g = f; f = e; e = ne; d = c; c = b; b = a; a = na;
  }
  const Word fin[8] = {a, b, c, d, e, f, g, h};
  for (int j = 0; j < 8; j++) {
    if (out_base) {
      uint32_t outw[32];   // result bit i (weight 2^i) of word j is output bit 32 j + (31 - i)
      for (int i = 0; i < 32; i++) outw[i] = out_base + 32 * j + (31 - i);
      out[j] = sb.add_mod32({st[j], fin[j]}, outw);
    } else {
      out[j] = sb.add_mod32({st[j], fin[j]});
    }
  }
}

// plain SHA-256 (FIPS 180-4 padding, multi-block) of a message given as bits (MSB-first per byte; wires or
// constants); the digest bits land on the 256 wires from out_base on
inline void sha256_bits(ShaBuilder& sb, const std::vector<Bit>& mbits, uint32_t out_base) {
  using Word = ShaBuilder::Word;
  const uint64_t bitlen = mbits.size();
  const uint32_t nb = (uint32_t)((bitlen / 8 + 9 + 63) / 64);
  auto padded_bit = [&](uint64_t k) -> Bit {   // bit k (MSB-first) of the padded message
    if (k < bitlen) return mbits[k];
    if (k == bitlen) return bit_const(1);
    const uint64_t total = (uint64_t)nb * 512;
    if (k >= total - 64) return bit_const((int)((bitlen >> (total - 1 - k)) & 1));
    return bit_const(0);
  };
  Word st[8];
  for (int j = 0; j < 8; j++) st[j] = ShaBuilder::word_const(kShaIV[j]);
  for (uint32_t blk = 0; blk < nb; blk++) {
    Word W16[16], out[8];
    for (int j = 0; j < 16; j++)
      for (int k = 0; k < 32; k++) W16[j][31 - k] = padded_bit((uint64_t)blk * 512 + 32 * j + k);
    sha_compress(sb, st, W16, out, blk + 1 == nb ? out_base : 0u);
    for (int j = 0; j < 8; j++) st[j] = out[j];
  }
}

}  // namespace g16
