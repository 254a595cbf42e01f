// g16_wtns_calc: witnesses computed from a recorded program (witness_program.h).  Here: the recorder's bookkeeping and
// the file image, the loader with its complete validation, the host route (device = -1) and the C ABI of the
// calculator.  The device route is wtns_calc.hip; the programs themselves are recorded in circuit_builders.cpp.
#include "witness_program.h"

#include <algorithm>
#include <thread>

#include "fixed_base.h"

using namespace g16;

namespace g16 {

// ------------------------------------------------------------------ recording
void WpRecorder::define(uint32_t wire, uint32_t level) {
  if (wire_level.empty()) wire_level.push_back(0);   // wire 0
  if (wire_level.size() <= wire) wire_level.resize((size_t)wire + 1, 0xffffffffu);
  wire_level[wire] = level;   // (a second definition is left to the loader to refuse)
}

uint32_t WpRecorder::put(const LinT& lin, uint32_t& level) {
  LinT l = lin;
  std::sort(l.begin(), l.end());
  uint32_t kept = 0;
  size_t i = 0;
  while (i < l.size()) {
    int64_t sum = 0;
    const uint32_t wire = l[i].first;
    while (i < l.size() && l[i].first == wire) sum += l[i++].second;
    if (!sum) continue;
    terms.push_back({wire, sum});
    kept++;
    const uint32_t lv = wire == 0 ? 0 : (wire < wire_level.size() ? wire_level[wire] : 0xffffffffu);
    if (lv != 0xffffffffu && lv > level) level = lv;   // (an undefined wire: the loader refuses the program)
  }
  return kept;
}

uint32_t WpRecorder::new_check(const char* what) {
  auto it = text_id.find(what);
  if (it == text_id.end()) {
    it = text_id.emplace(what, (uint32_t)texts.size()).first;
    texts.push_back(what);
  }
  check_text.push_back(it->second);
  return (uint32_t)check_text.size() - 1;
}

void WpRecorder::input(uint32_t wire) {
  recs.push_back({WP_INPUT, wire, n_inputs++, kWpNoCheck, 1, terms.size(), 0, 0, 0});
  define(wire, 1);
}
void WpRecorder::name_inputs(const char* name, uint32_t count) { inputs.push_back({name, n_inputs - count, count}); }

void WpRecorder::quad(uint32_t wire, const LinT& a, const LinT& b, const LinT& c) {
  Rec r{WP_QUAD, wire, 0, kWpNoCheck, 0, terms.size(), 0, 0, 0};
  r.na = put(a, r.level);
  r.nb = put(b, r.level);
  r.nc = put(c, r.level);
  r.level++;
  recs.push_back(r);
  define(wire, r.level);
}
void WpRecorder::bits(const uint32_t* wires, uint32_t n, const LinT& a, const char* what) {
  Rec r{WP_BITS, (uint32_t)targets.size(), n, what ? new_check(what) : kWpNoCheck, 0, terms.size(), 0, 0, 0};
  r.na = put(a, r.level);
  r.level++;
  recs.push_back(r);
  for (uint32_t i = 0; i < n; i++) { targets.push_back(wires[i]); define(wires[i], r.level); }
}
void WpRecorder::inv0(uint32_t wire, const LinT& a) {
  Rec r{WP_INV0, wire, 0, kWpNoCheck, 0, terms.size(), 0, 0, 0};
  r.na = put(a, r.level);
  r.level++;
  recs.push_back(r);
  define(wire, r.level);
}
void WpRecorder::isz(uint32_t wire, const LinT& a) {
  Rec r{WP_ISZ, wire, 0, kWpNoCheck, 0, terms.size(), 0, 0, 0};
  r.na = put(a, r.level);
  r.level++;
  recs.push_back(r);
  define(wire, r.level);
}
void WpRecorder::check(const LinT& a, const char* what) {
  Rec r{WP_CHECK, 0, 0, new_check(what), 0, terms.size(), 0, 0, 0};
  r.na = put(a, r.level);
  r.level++;
  recs.push_back(r);
}

Buf WpRecorder::finish(uint32_t n_wires, uint32_t n_public) const {
  uint32_t n_levels = 0;
  for (const Rec& r : recs) n_levels = std::max(n_levels, r.level);
  // counting sort by (level, kind); stable, so the ops of a level and kind keep the build order
  std::vector<uint32_t> start((size_t)(n_levels + 1) * WP_KINDS + 1, 0);
  auto key = [](const Rec& r) { return (size_t)r.level * WP_KINDS + r.kind; };
  for (const Rec& r : recs) start[key(r) + 1]++;
  for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
  std::vector<uint32_t> order(recs.size());
  {
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (size_t i = 0; i < recs.size(); i++) order[at[key(recs[i])]++] = (uint32_t)i;
  }
  size_t names = 0, text_bytes = 0;
  for (const WpInput& in : inputs) names += 12 + in.name.size();
  for (const std::string& t : texts) text_bytes += 4 + t.size();
  static const int ids[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  uint64_t sizes[16] = {};
  sizes[1] = 11 * 4;
  sizes[2] = (uint64_t)recs.size() * 32;
  sizes[3] = (uint64_t)terms.size() * 12;
  sizes[4] = ((uint64_t)n_levels + 1) * 4;
  sizes[5] = (uint64_t)targets.size() * 4;
  sizes[6] = (uint64_t)check_text.size() * 4 + text_bytes;
  sizes[7] = names;
  sizes[8] = (uint64_t)outputs.size() * 4;
  Buf z;
  uint8_t* sec[16] = {};
  if (!bin_layout(z, "wprg", 1, ids, 8, sizes, sec)) return Buf{};
  auto put32 = [](uint8_t*& q, uint32_t v) { memcpy(q, &v, 4); q += 4; };
  uint8_t* q = sec[1];
  const uint32_t hdr[11] = {n_wires, n_public, n_inputs, (uint32_t)recs.size(), n_levels, (uint32_t)terms.size(),
                            (uint32_t)targets.size(), (uint32_t)check_text.size(), (uint32_t)texts.size(),
                            (uint32_t)inputs.size(), (uint32_t)outputs.size()};
  for (uint32_t v : hdr) put32(q, v);
  q = sec[2];
  uint8_t* tq = sec[3];
  uint32_t t_at = 0;
  for (uint32_t k : order) {
    const Rec& r = recs[k];
    const uint32_t nt = r.na + r.nb + r.nc;
    const uint32_t rec[8] = {r.kind, r.dst, r.n, r.check, t_at, r.na, r.nb, r.nc};
    for (uint32_t v : rec) put32(q, v);
    for (uint32_t i = 0; i < nt; i++) {
      const auto& t = terms[r.t_off + i];
      put32(tq, t.first);
      put32(tq, (uint32_t)(uint64_t)t.second);
      put32(tq, (uint32_t)((uint64_t)t.second >> 32));
    }
    t_at += nt;
  }
  q = sec[4];
  for (uint32_t l = 1; l <= n_levels + 1; l++) put32(q, start[(size_t)l * WP_KINDS]);   // ops below level l (none at level 0)
  q = sec[5];
  for (uint32_t v : targets) put32(q, v);
  q = sec[6];
  for (uint32_t v : check_text) put32(q, v);
  for (const std::string& t : texts) { put32(q, (uint32_t)t.size()); memcpy(q, t.data(), t.size()); q += t.size(); }
  q = sec[7];
  for (const WpInput& in : inputs) {
    put32(q, in.first); put32(q, in.count); put32(q, (uint32_t)in.name.size());
    memcpy(q, in.name.data(), in.name.size());
    q += in.name.size();
  }
  q = sec[8];
  for (uint32_t v : outputs) put32(q, v);
  return z;
}

// ------------------------------------------------------------------ loading
int wp_load(const uint8_t* buf, size_t len, WitnessProgram& p) {
  auto bad = [](const std::string& why) { set_error("witness program: " + why); return G16_E_FORMAT; };
  BinView f;
  if (const int rc = bin_open(buf, len, "wprg", 1, f)) return rc;
  for (int id = 1; id <= 8; id++)
    if (!f.sec[id].p) return bad("Missing section " + std::to_string(id));
  if (f.sec[1].size != 44) return bad("the header section has the wrong size");
  uint32_t h[11];
  memcpy(h, f.sec[1].p, 44);
  const uint32_t n_wires = h[0], n_public = h[1], n_inputs = h[2], n_ops = h[3], n_levels = h[4], n_terms = h[5],
                 n_targets = h[6], n_checks = h[7], n_texts = h[8], n_names = h[9], n_outputs = h[10];
  if (n_wires == 0 || n_wires > (1u << 28)) return bad("the number of wires is out of range");
  if (n_public >= n_wires) return bad("the number of public signals is out of range");
  if (n_inputs >= n_wires) return bad("the number of input words is out of range");   // (a word feeds a wire of its own)
  if (f.sec[2].size != (uint64_t)n_ops * 32 || f.sec[3].size != (uint64_t)n_terms * 12 ||
      f.sec[4].size != ((uint64_t)n_levels + 1) * 4 || f.sec[5].size != (uint64_t)n_targets * 4 ||
      f.sec[8].size != (uint64_t)n_outputs * 4 || f.sec[6].size < (uint64_t)n_checks * 4)
    return bad("a section's size does not match the header");
  p = WitnessProgram{};
  p.n_wires = n_wires; p.n_public = n_public; p.n_inputs = n_inputs;
  p.ops.resize(n_ops);
  if (n_ops) memcpy(p.ops.data(), f.sec[2].p, (size_t)n_ops * 32);
  p.terms.resize(n_terms);
  if (n_terms) memcpy(p.terms.data(), f.sec[3].p, (size_t)n_terms * 12);
  p.levels.resize((size_t)n_levels + 1);
  memcpy(p.levels.data(), f.sec[4].p, ((size_t)n_levels + 1) * 4);
  p.targets.resize(n_targets);
  if (n_targets) memcpy(p.targets.data(), f.sec[5].p, (size_t)n_targets * 4);
  p.outputs.resize(n_outputs);
  if (n_outputs) memcpy(p.outputs.data(), f.sec[8].p, (size_t)n_outputs * 4);
  {  // checks and their texts
    p.check_text.resize(n_checks);
    if (n_checks) memcpy(p.check_text.data(), f.sec[6].p, (size_t)n_checks * 4);
    const uint8_t* q = f.sec[6].p + (size_t)n_checks * 4;
    uint64_t left = f.sec[6].size - (uint64_t)n_checks * 4;
    for (uint32_t i = 0; i < n_texts; i++) {
      if (left < 4) return bad("the check texts are cut short");
      const uint32_t l = rd32(q);
      if (l > left - 4) return bad("the check texts are cut short");
      p.texts.emplace_back((const char*)q + 4, l);
      q += 4 + l; left -= 4 + l;
    }
    if (left) return bad("bytes behind the check texts");
    for (uint32_t i = 0; i < n_checks; i++)
      if (p.check_text[i] >= n_texts) return bad("check " + std::to_string(i) + " names a text out of range");
  }
  {  // the input table
    const uint8_t* q = f.sec[7].p;
    uint64_t left = f.sec[7].size;
    for (uint32_t i = 0; i < n_names; i++) {
      if (left < 12) return bad("the input table is cut short");
      const uint32_t first = rd32(q), count = rd32(q + 4), l = rd32(q + 8);
      if (l > left - 12) return bad("the input table is cut short");
      if ((uint64_t)first + count > n_inputs) return bad("input " + std::to_string(i) + " is out of range");
      p.inputs.push_back({std::string((const char*)q + 12, l), first, count});
      q += 12 + l; left -= 12 + l;
    }
    if (left) return bad("bytes behind the input table");
  }
  // the level index covers the ops: 0 = lv[0] <= lv[1] <= ... <= lv[n_levels] = n_ops
  if (p.levels[0] != 0 || p.levels[n_levels] != n_ops) return bad("the level index does not cover the ops");
  for (uint32_t l = 0; l < n_levels; l++)
    if (p.levels[l] > p.levels[l + 1]) return bad("the level index does not cover the ops");
  // first pass: every op's own fields, and which op defines which wire at which level
  std::vector<uint32_t> wire_level(n_wires, 0xffffffffu);
  wire_level[0] = 0;
  auto define = [&](uint32_t wire, uint32_t level, uint32_t k) -> int {
    if (wire == 0 || wire >= n_wires) return bad("op " + std::to_string(k) + " defines wire " + std::to_string(wire) + ", which is out of range");
    if (wire_level[wire] != 0xffffffffu) return bad("wire " + std::to_string(wire) + " is defined twice");
    wire_level[wire] = level;
    return G16_OK;
  };
  uint32_t level = 0;
  for (uint32_t k = 0; k < n_ops; k++) {
    while (level < n_levels && k >= p.levels[level]) level++;   // op k lies in [lv[level - 1], lv[level])
    const WpOp& op = p.ops[k];
    const std::string at = "op " + std::to_string(k);
    if (op.kind >= WP_KINDS) return bad(at + " has an unknown kind");
    const uint64_t nt = (uint64_t)op.na + op.nb + op.nc;
    if (op.t_off > n_terms || nt > (uint64_t)n_terms - op.t_off) return bad(at + " has terms out of range");
    if (op.kind != WP_QUAD && (op.nb || op.nc)) return bad(at + " has forms its kind does not take");
    if (op.kind == WP_INPUT && (op.na || op.n >= n_inputs)) return bad(at + " reads input word " + std::to_string(op.n) + ", which is out of range");
    if ((op.kind == WP_CHECK || (op.kind == WP_BITS && op.check != kWpNoCheck)) && op.check >= n_checks)
      return bad(at + " names check " + std::to_string(op.check) + ", which is out of range");
    if (op.kind == WP_BITS) {
      if (op.n < 1 || op.n > kWpMaxBits) return bad(at + " takes " + std::to_string(op.n) + " bits (at most " + std::to_string(kWpMaxBits) + ")");
      if (op.dst > n_targets || op.n > n_targets - op.dst) return bad(at + " has targets out of range");
      for (uint32_t i = 0; i < op.n; i++)
        if (const int rc = define(p.targets[op.dst + i], level, k)) return rc;
    } else if (op.kind != WP_CHECK) {
      if (const int rc = define(op.dst, level, k)) return rc;
    }
  }
  for (uint32_t wire = 1; wire < n_wires; wire++)
    if (wire_level[wire] == 0xffffffffu) return bad("wire " + std::to_string(wire) + " is never defined");
  // second pass: every term reads a wire of a strictly lower level
  level = 0;
  for (uint32_t k = 0; k < n_ops; k++) {
    while (level < n_levels && k >= p.levels[level]) level++;
    const WpOp& op = p.ops[k];
    for (uint32_t i = op.t_off; i < op.t_off + op.na + op.nb + op.nc; i++) {
      const uint32_t wire = p.terms[i].wire;
      if (wire >= n_wires) return bad("op " + std::to_string(k) + " reads wire " + std::to_string(wire) + ", which is out of range");
      if (wire_level[wire] >= level)
        return bad("op " + std::to_string(k) + " at level " + std::to_string(level) + " reads wire " + std::to_string(wire) +
                   " of level " + std::to_string(wire_level[wire]));
    }
  }
  for (uint32_t i = 0; i < n_outputs; i++)
    if (p.outputs[i] >= n_wires) return bad("output " + std::to_string(i) + " is out of range");
  // the evaluators' terms: distinct coefficients as Montgomery images
  p.inv_small.assign(kWpInvSmall, fp_zero<FrParams>());
  {  // 1 / k for every small k from ONE inversion: prefix products, then peeled off from the top
    std::vector<FrM> pre(kWpInvSmall, fr_one());
    for (uint32_t k = 1; k < kWpInvSmall; k++) pre[k] = fp_mul(pre[k - 1], fr_u64(k));
    FrM inv = fp_inv(pre[kWpInvSmall - 1]);   // 1 / (K - 1)!
    for (uint32_t k = kWpInvSmall - 1; k >= 1; k--) {
      p.inv_small[k] = fp_from_mont(fp_mul(inv, pre[k - 1]));
      inv = fp_mul(inv, fr_u64(k));
    }
  }
  p.coefs = {fr_one(), fr_neg_one()};
  p.icoefs = {1, -1};
  std::unordered_map<int64_t, uint32_t> idx;
  idx[1] = 0; idx[-1] = 1;
  p.eterms.resize(n_terms);
  for (uint32_t i = 0; i < n_terms; i++) {
    const int64_t cf = (int64_t)((uint64_t)p.terms[i].lo | ((uint64_t)p.terms[i].hi << 32));
    auto it = idx.find(cf);
    if (it == idx.end()) {
      it = idx.emplace(cf, (uint32_t)p.coefs.size()).first;
      const uint64_t mag = cf < 0 ? 0 - (uint64_t)cf : (uint64_t)cf;
      p.coefs.push_back(cf < 0 ? fp_neg(fr_u64(mag)) : fr_u64(mag));
      p.icoefs.push_back(cf);
    }
    p.eterms[i] = {p.terms[i].wire, it->second};
  }
  return G16_OK;
}

// ------------------------------------------------------------------ host route
uint32_t wp_eval_host(const WitnessProgram& p, const uint8_t* inputs, Fr* w) {
  const WpView v = p.view();
  std::vector<Fr> in(p.n_inputs ? p.n_inputs : 1);
  if (p.n_inputs) memcpy((void*)in.data(), inputs, (size_t)p.n_inputs * 32);
  w[0] = wp_small(1);
  uint32_t status = kWpNoCheck;
  for (uint32_t k = 0; k < (uint32_t)p.ops.size(); k++) {   // (level order is an order of evaluation)
    const uint32_t c = wp_eval_op(v, k, in.data(), w);
    if (c < status) status = c;
  }
  return status;
}

}  // namespace g16

// ------------------------------------------------------------------ C ABI
int wcalc_check_inputs(const g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count) {
  if (n_inputs != h->p.n_inputs) {
    set_error("wtns calc: the program takes " + std::to_string(h->p.n_inputs) + " input words, " + std::to_string(n_inputs) + " given");
    return G16_E_ARG;
  }
  for (size_t i = 0; i < count; i++)
    for (size_t j = 0; j < n_inputs; j++) {
      uint32_t v[8];
      memcpy(v, inputs + (i * n_inputs + j) * 32, 32);
      if (fr_below_modulus(v)) continue;
      std::string name = "word " + std::to_string(j);
      for (const WpInput& in : h->p.inputs)
        if (j >= in.first && j - in.first < in.count) name = in.name + "[" + std::to_string(j - in.first) + "]";
      set_error("witness " + std::to_string(i) + ": input " + name + " is not reduced modulo the scalar field");
      return G16_E_FORMAT;
    }
  return G16_OK;
}

int wcalc_match_prover(const g16_wtns_calculator* h, const char* who, int device, uint32_t n_wires, uint32_t n_public) {
  const std::string w(who);
  if (!h->dev) { set_error(w + ": the calculator runs on the host route (create it on the prover's device)"); return G16_E_STATE; }
  if (wcalc_device_id(h->dev) != device) {
    set_error(w + ": the calculator is on device " + std::to_string(wcalc_device_id(h->dev)) + ", the prover on device " +
              std::to_string(device));
    return G16_E_STATE;
  }
  if (h->p.n_wires != n_wires || h->p.n_public != n_public) {
    set_error(w + ": the program has " + std::to_string(h->p.n_wires) + " wires and " + std::to_string(h->p.n_public) +
              " public signals, the key " + std::to_string(n_wires) + " and " + std::to_string(n_public));
    return G16_E_STATE;
  }
  return G16_OK;
}

extern "C" int g16_wtns_calc_create(const uint8_t* prog, size_t len, int device, g16_wtns_calculator** out) {
  if (!out) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  *out = nullptr;
  if (device < -1) { set_error("wtns calc: bad device ordinal"); return G16_E_ARG; }
  return no_bad_alloc("wtns calc", [&]() -> int {
    g16_wtns_calculator* h = new g16_wtns_calculator;
    h->device = device;
    int rc = wp_load(prog, len, h->p);   // (complete, before the device is touched)
    if (!rc && device >= 0) {
      // witnesses per chunk: what 4 GiB hold at 32 bytes per wire, at most 1024 (G16_WTNS_CALC_CHUNK overrides);
      // the buffer itself grows with the batches that arrive
      uint32_t chunk = env_u32("G16_WTNS_CALC_CHUNK");
      if (!chunk) {
        const uint64_t fit = ((uint64_t)4 << 30) / (32 * (uint64_t)h->p.n_wires);
        chunk = (uint32_t)(fit < 1 ? 1 : fit > 1024 ? 1024 : fit);
      }
      rc = wcalc_device_create(device, h->p, chunk, &h->dev);
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return G16_OK;
  });
}

extern "C" void g16_wtns_calc_destroy(g16_wtns_calculator* h) {
  if (!h) return;
  wcalc_device_destroy(h->dev);
  delete h;
}

extern "C" int g16_wtns_calc(g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count, uint8_t* out_bodies,
                             uint32_t* status) {
  if (!h || (count && !status) || (count && n_inputs && !inputs)) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  if (const int rc = wcalc_check_inputs(h, inputs, n_inputs, count)) return rc;
  return no_bad_alloc("wtns calc", [&]() -> int {
    h->ms[0] = h->ms[1] = h->ms[2] = 0.f;
    if (h->dev) return wcalc_device_run(h->dev, inputs, count, out_bodies, status, h->ms);
    const unsigned hw = std::thread::hardware_concurrency();
    parallel_for(count, (int)(hw < 1 ? 1 : hw > 16 ? 16 : hw), [&](size_t lo, size_t hi) {
      std::vector<Fr> w(h->p.n_wires);   // (the caller's buffer need not be aligned for Fr)
      for (size_t i = lo; i < hi; i++) {
        status[i] = wp_eval_host(h->p, inputs + i * n_inputs * 32, w.data());
        if (out_bodies) memcpy(out_bodies + i * (size_t)h->p.n_wires * 32, w.data(), (size_t)h->p.n_wires * 32);
      }
    });
    return G16_OK;
  });
}

extern "C" const char* g16_wtns_calc_check_text(const g16_wtns_calculator* h, uint32_t k) {
  if (!h || k >= h->p.check_text.size()) return nullptr;
  return h->p.texts[h->p.check_text[k]].c_str();
}

extern "C" int g16_wtns_calc_info(const g16_wtns_calculator* h, uint32_t info[6]) {
  if (!h || !info) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  info[0] = h->p.n_wires; info[1] = h->p.n_public; info[2] = h->p.n_inputs;
  info[3] = (uint32_t)h->p.levels.size() - 1; info[4] = (uint32_t)h->p.outputs.size(); info[5] = (uint32_t)h->p.inputs.size();
  return G16_OK;
}
extern "C" int g16_wtns_calc_outputs(const g16_wtns_calculator* h, uint32_t* wires) {
  if (!h || (!wires && !h->p.outputs.empty())) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  for (size_t i = 0; i < h->p.outputs.size(); i++) wires[i] = h->p.outputs[i];
  return G16_OK;
}
extern "C" const char* g16_wtns_calc_input(const g16_wtns_calculator* h, uint32_t i, uint32_t* first, uint32_t* count) {
  if (!h || i >= h->p.inputs.size()) return nullptr;
  if (first) *first = h->p.inputs[i].first;
  if (count) *count = h->p.inputs[i].count;
  return h->p.inputs[i].name.c_str();
}

extern "C" int g16_wtns_calc_wtns(g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, uint32_t* status, uint8_t** wtns,
                                  size_t* len) {
  if (!h || !status || !wtns || !len) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  *wtns = nullptr;
  *len = 0;
  return no_bad_alloc("wtns calc", [&]() -> int {
    // the .wtns image of write_wtns (circuit.cpp): header section, then the words where the calculator puts them
    static const int ids[2] = {1, 2};
    uint64_t sizes[16] = {};
    sizes[1] = 40;
    sizes[2] = (uint64_t)h->p.n_wires * 32;
    Buf z;
    uint8_t* sec[16] = {};
    if (!bin_layout(z, "wtns", 2, ids, 2, sizes, sec)) { set_error("wtns calc: out of memory"); return G16_E_STATE; }
    uint8_t* q = bin_put_field(sec[1], kFrP);
    memcpy(q, &h->p.n_wires, 4);
    const int rc = g16_wtns_calc(h, inputs, n_inputs, 1, sec[2], status);
    if (rc || *status != kWpNoCheck) return rc;   // (a violated check: the verdict, and no image)
    z.give(wtns, len);
    return G16_OK;
  });
}

extern "C" int g16_wtns_calc_timings(const g16_wtns_calculator* h, float ms[3]) {
  if (!h || !ms) { set_error("wtns calc: null argument"); return G16_E_ARG; }
  for (int i = 0; i < 3; i++) ms[i] = h->ms[i];
  return G16_OK;
}

// the input words of NZCPPubIdentity for a ToBeSigned: 8 * max_bytes bits (MSB first per byte, zero beyond the length),
// then the length
extern "C" int g16_nzcp_inputs(const uint8_t* tbs, uint32_t len, uint32_t max_bytes, uint8_t* out_words) {
  if ((!tbs && len) || !out_words || max_bytes == 0 || max_bytes > 503 || len > max_bytes) {
    set_error("nzcp inputs: bad arguments");
    return G16_E_ARG;
  }
  memset(out_words, 0, ((size_t)max_bytes * 8 + 1) * 32);
  for (uint32_t k = 0; k < len * 8; k++) out_words[(size_t)k * 32] = (tbs[k / 8] >> (7 - (k & 7))) & 1;
  memcpy(out_words + (size_t)max_bytes * 8 * 32, &len, 4);
  return G16_OK;
}
