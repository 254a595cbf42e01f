// The seeded synthetic circuit and witness generator: a shape-matched random R1CS, keyed with a known trapdoor in
// snarkjs's zkey layout (setup_groth16.cpp), for benchmark- and parity-sized proving keys where no compiled circuit is
// at hand.  Test-only.  The generator follows, draw for draw, the spec in
// oracle/synth.py's docstring; tests check the two produce byte-identical zkey/wtns for the same seed.
#include "circuit.h"

namespace g16 {
namespace {

FrM coef(Xo& rng) {
  const uint64_t u = rng.below(100);
  if (u < 40) return fr_one();
  if (u < 80) return fr_neg_one();
  if (u < 95) return fr_u64(1 + rng.below(65535));
  return rng.rand_fr();
}

enum : uint8_t { CONST = 0, PUB, BIT, SMALL, SLACK };
constexpr uint64_t EXP_EXAMPLE = 1951416330ull;

void gen_classes(Circuit& c, uint64_t seed) {
  Xo rng(seed);
  c.cls.assign(c.n, CONST);
  for (uint32_t i = 1; i < c.n; i++) {
    if (i <= c.p) c.cls[i] = PUB;
    else {
      const uint64_t u = rng.below(100);
      c.cls[i] = u < 60 ? BIT : (u < 68 ? SMALL : SLACK);
    }
  }
}

void gen_circuit(Circuit& c, uint64_t seed) {
  gen_classes(c, seed);
  Xo rng(seed + 3);
  const uint32_t n = c.n, p = c.p, m = c.m;
  std::vector<uint32_t> slack, bits, rank(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (c.cls[i] == SLACK) { rank[i] = (uint32_t)slack.size(); slack.push_back(i); }
    if (((c.cls[i] == PUB && i < p) || c.cls[i] == BIT) && i % 20 < 7) bits.push_back(i);
  }
  if (bits.empty()) bits.push_back(0);
  uint32_t nxt = 0;
  auto fix = [&](uint32_t s) { return (c.cls[s] == SLACK && rank[s] >= nxt) ? 0u : s; };
  auto pick = [&]() { return fix((uint32_t)rng.below(n)); };
  auto pick_b = [&]() {
    const uint32_t t = (uint32_t)rng.below(n);
    uint32_t s = t - t % 20 + (uint32_t)rng.below(7);
    if (s > n - 1) s = n - 1;
    return fix(s);
  };
  c.rowA.assign(1, 0); c.rowB.assign(1, 0); c.rowC.assign(1, 0);
  for (uint32_t r = 0; r < m; r++) {
    const uint64_t u = rng.below(100);
    const uint32_t rem = (uint32_t)slack.size() - nxt;
    if (rem > 0 && (u < 32 || rem >= m - r)) {
      const uint32_t sw = slack[nxt];
      const uint32_t ta = 1 + (uint32_t)rng.below(4);
      for (uint32_t k = 0; k < ta; k++) { const uint32_t s = pick(); c.tA.push_back({s, coef(rng)}); }
      const uint32_t tb = 1 + (uint32_t)rng.below(2);
      for (uint32_t k = 0; k < tb; k++) { const uint32_t s = pick_b(); c.tB.push_back({s, coef(rng)}); }
      const uint32_t j1 = pick();
      const FrM c1 = rng.rand_fr();
      c.tC.push_back({sw, fr_one()});
      c.tC.push_back({j1, c1});
      c.slacks.push_back({r, sw, j1, c1});
      nxt++;
    } else {
      const uint32_t x = bits[rng.below(bits.size())];
      const uint32_t y = bits[rng.below(bits.size())];
      const FrM ca = coef(rng), cb = coef(rng);
      c.tA.push_back({x, ca});
      c.tA.push_back({y, fp_neg(ca)});
      c.tB.push_back({x, cb});
      c.tB.push_back({y, cb});
      c.tB.push_back({0, fp_neg(cb)});
    }
    c.rowA.push_back((uint32_t)c.tA.size());
    c.rowB.push_back((uint32_t)c.tB.size());
    c.rowC.push_back((uint32_t)c.tC.size());
  }
}

// witness in Montgomery form
void gen_witness(const Circuit& c, uint64_t wseed, std::vector<FrM>& w) {
  Xo rng(wseed);
  w.assign(c.n, fp_zero<FrParams>());
  w[0] = fr_one();
  for (uint32_t i = 1; i < c.n; i++) {
    switch (c.cls[i]) {
      case PUB: w[i] = fr_u64(i == c.p ? EXP_EXAMPLE : rng.below(2)); break;
      case BIT: w[i] = fr_u64(rng.below(2)); break;
      case SMALL: w[i] = fr_u64(rng.below(1024)); break;
      default: w[i] = rng.rand_fr(); break;
    }
  }
  for (const auto& sl : c.slacks) {
    FrM a = fp_zero<FrParams>(), b = fp_zero<FrParams>();
    for (uint32_t k = c.rowA[sl.row]; k < c.rowA[sl.row + 1]; k++) a = fp_add(a, fp_mul(c.tA[k].cf, w[c.tA[k].s]));
    for (uint32_t k = c.rowB[sl.row]; k < c.rowB[sl.row + 1]; k++) b = fp_add(b, fp_mul(c.tB[k].cf, w[c.tB[k].s]));
    w[sl.sw] = fp_sub(fp_mul(a, b), fp_mul(sl.c1, w[sl.j1]));
  }
}

}  // namespace
}  // namespace g16

using namespace g16;

extern "C" int g16_synth_witness(uint32_t n, uint32_t p, uint32_t m, uint64_t seed, uint64_t wseed,
                                 uint8_t** wtns, size_t* wtns_len) {
  if (!wtns || !wtns_len || n < p + 1 || n < 2) { set_error("synth: bad arguments"); return G16_E_ARG; }
  Circuit c;
  c.n = n; c.p = p; c.m = m;
  gen_circuit(c, seed);
  std::vector<FrM> w;
  gen_witness(c, wseed, w);
  write_wtns(w).give(wtns, wtns_len);
  return G16_OK;
}

extern "C" int g16_synth_setup(uint32_t n, uint32_t p, uint32_t m, uint64_t seed, int threads, uint8_t** zkey,
                               size_t* zkey_len, uint8_t** wtns, size_t* wtns_len, uint8_t** vkey,
                               size_t* vkey_len) {
  if (!zkey || !zkey_len || n < p + 1 || n < 2 || m == 0) { set_error("synth: bad arguments"); return G16_E_ARG; }
  Circuit c;
  c.n = n; c.p = p; c.m = m;
  gen_circuit(c, seed);
  int rc = setup_core(c, seed, threads, zkey, zkey_len, vkey, vkey_len);
  if (rc) return rc;
  if (wtns && wtns_len) {
    std::vector<FrM> w;
    gen_witness(c, seed, w);
    write_wtns(w).give(wtns, wtns_len);
  }
  return G16_OK;
}
