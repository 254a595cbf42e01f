// The real constraint systems built natively and their test-only entry points: SHA-256 chain and message, the NZCP
// public interface on a fixed pass layout, the NZCP circuit library (nzcp_gadgets.h) by template and as a whole.
#include "nzcp_gadgets.h"

// ------------------------------------------------------------------ SHA-256 chain circuit
// A REAL constraint system instead of the shape-matched random one: `blocks` chained SHA-256 compressions,
//   d_0 = the 32-byte private message,  d_{i+1} = SHA-256(d_i)   (one padded 64-byte block each),
// public outputs = the 256 bits of d_blocks, MSB-first per byte -- the bit order of the NZCP circuit's
// sha256 outputs (/root/reference/test/nzcp.js:41-47).  Bit-level R1CS in the style of circomlib's sha256
// gadgets that nzcptpl.circom includes (xor3 / ch / maj as one or two products per bit, modular additions as
// one linear row plus a booleanity row per result and carry bit): ~27 k constraints per block, 155 blocks
// fill a 2^22 domain.  Every wire is a bit, so the witness is bits only.
namespace g16 {
namespace {

// wires: 0 = one, 1..256 = public outputs (digest bits, MSB-first), then the private message bits (MSB-first,
// boolean-constrained), then gates.  chain = true: digest_{i+1} = SHA-256(digest_i), `blocks` times, 32-byte
// message.  chain = false: plain SHA-256 of the `len`-byte message (padding per FIPS 180-4, len is a
// compile-time constant of the circuit, like the fixed-length Sha256 gadgets of circomlib).
void build_sha256(ShaBuilder& sb, bool chain, uint32_t blocks, const uint8_t* msg, uint32_t len) {
  using Word = ShaBuilder::Word;
  for (int i = 0; i < 256; i++) sb.new_wire(0);   // outputs, values filled by the last addition
  std::vector<Bit> mbits((size_t)len * 8);
  for (uint32_t k = 0; k < len * 8; k++) {
    const uint32_t wire = sb.new_wire((msg[k / 8] >> (7 - (k & 7))) & 1);
    sb.boolean(wire);
    mbits[k] = bit_wire(wire);
  }
  Word iv[8];
  for (int j = 0; j < 8; j++) iv[j] = ShaBuilder::word_const(kShaIV[j]);
  if (chain) {
    Word m[8];
    for (int j = 0; j < 8; j++)
      for (int k = 0; k < 32; k++) m[j][31 - k] = mbits[32 * j + k];
    for (uint32_t blk = 0; blk < blocks; blk++) {
      Word W16[16], out[8];
      for (int j = 0; j < 8; j++) W16[j] = m[j];
      W16[8] = ShaBuilder::word_const(0x80000000u);
      for (int j = 9; j < 15; j++) W16[j] = ShaBuilder::word_const(0);
      W16[15] = ShaBuilder::word_const(256);
      sha_compress(sb, iv, W16, out, blk + 1 == blocks ? 1u : 0u);
      for (int j = 0; j < 8; j++) m[j] = out[j];
    }
  } else {
    sha256_bits(sb, mbits, 1);
  }
  sb.c.n = (uint32_t)sb.w.size();
  sb.c.p = 256;
  sb.c.m = (uint32_t)sb.c.rowA.size() - 1;
}

// The NZCP circuit's PUBLIC INTERFACE on a fixed pass layout (/root/reference/circuits/nzcptpl.circom:447-602,
// /root/reference/test/nzcp.js:41-47): public signals [0..255] = SHA-256("given,family,dob") bits,
// [256..511] = SHA-256(ToBeSigned) bits, [512] = exp.  The reference finds the three strings and `exp` by CBOR
// parsing inside the circuit (cbortpl.circom, not restated here); this circuit takes their byte offsets as
// circuit constants instead -- sound for passes of that layout: the credential string is wired to the SAME
// ToBeSigned bit wires at seg_off[k] (no copies), commas are constants, and exp is one linear row over the
// 32 ToBeSigned bits at exp_off.
void build_nzcp_fixed_layout(ShaBuilder& sb, const uint8_t* tbs, uint32_t len, const uint32_t seg_off[3],
                             const uint32_t seg_len[3], uint32_t exp_off) {
  for (int i = 0; i < 512; i++) sb.new_wire(0);   // the two digests
  const uint32_t exp_wire = sb.new_wire(0);
  std::vector<Bit> mbits((size_t)len * 8);
  for (uint32_t k = 0; k < len * 8; k++) {
    const uint32_t wire = sb.new_wire((tbs[k / 8] >> (7 - (k & 7))) & 1);
    sb.boolean(wire);
    mbits[k] = bit_wire(wire);
  }
  std::vector<Bit> subj;
  for (int sgi = 0; sgi < 3; sgi++) {
    if (sgi)
      for (int k = 0; k < 8; k++) subj.push_back(bit_const((',' >> (7 - k)) & 1));
    for (uint32_t k = 0; k < seg_len[sgi] * 8; k++) subj.push_back(mbits[(size_t)seg_off[sgi] * 8 + k]);
  }
  sha256_bits(sb, subj, 1);
  sha256_bits(sb, mbits, 257);
  uint64_t exp = 0;
  Lin a, b, z;
  for (int k = 0; k < 32; k++) {
    const Bit& bt = mbits[(size_t)exp_off * 8 + k];
    exp |= (uint64_t)sb.val(bt) << (31 - k);
    ShaBuilder::add(a, bt, (int64_t)1 << (31 - k));
  }
  sb.w[exp_wire] = exp;
  a.t.push_back({exp_wire, -1});
  b.t.push_back({0u, 1});
  sb.constrain(a, b, z);
  sb.c.n = (uint32_t)sb.w.size();
  sb.c.p = 513;
  sb.c.m = (uint32_t)sb.c.rowA.size() - 1;
}

// every row of the builder's R1CS evaluated on its witness: the index of the first row with <A,w><B,w> != <C,w>,
// or -1
int64_t first_unsatisfied_row(const CBuilder& cb) {
  const Circuit& c = cb.c;
  const uint32_t m = (uint32_t)c.rowA.size() - 1;
  auto dot = [&](const std::vector<Term>& t, uint32_t lo, uint32_t hi) {
    FrM s = fp_zero<FrParams>();
    for (uint32_t k = lo; k < hi; k++) s = fp_add(s, fp_mul(t[k].cf, cb.wire_val(t[k].s)));
    return s;
  };
  for (uint32_t r = 0; r < m; r++) {
    const FrM a = dot(c.tA, c.rowA[r], c.rowA[r + 1]), b = dot(c.tB, c.rowB[r], c.rowB[r + 1]);
    const FrM cc = dot(c.tC, c.rowC[r], c.rowC[r + 1]);
    if (!CBuilder::fr_eq(fp_mul(a, b), cc)) return (int64_t)r;
  }
  return -1;
}

// wtns / r1cs / trapdoor zkey of builder b (ShaBuilder or CBuilder), each on request (the witness vector too)
template <class B>
int emit(const B& b, const char* too_large, uint64_t seed, int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** wtns,
         size_t* wtns_len, uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len) {
  if ((uint64_t)b.c.m + b.c.p + 1 > ((uint64_t)1 << 27)) { set_error(too_large); return G16_E_ARG; }
  if (wtns && wtns_len) {
    std::vector<FrM> w(b.w.size());
    for (size_t i = 0; i < w.size(); i++) w[i] = b.wire_val((uint32_t)i);
    write_wtns(w).give(wtns, wtns_len);
  }
  if (r1cs && r1cs_len) write_r1cs(b.c, b.c.p, 0).give(r1cs, r1cs_len);
  if (zkey && zkey_len) return setup_core(b.c, seed, threads, zkey, zkey_len, vkey, vkey_len);
  return G16_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The NZCP circuit library as native gadgets (nzcp_gadgets.h), one template at a time -- the twins of the
// reference's *_test.circom entry points (/root/reference/circuits/*_test.circom), so that its test vectors
// (/root/reference/test/cbor.js, quinSelector.js, nzcp.js) can be replayed against the natively built rows.
using V = CBuilder::V;

int run_gadget(CBuilder& cb, const std::string& name, const uint32_t* prm, uint32_t nprm, const uint64_t* in, uint32_t nin,
               std::vector<V>& outs) {
  uint32_t pos_in = 0;
  auto P = [&](uint32_t i) -> uint32_t { return i < nprm ? prm[i] : 0u; };
  auto input = [&]() -> V {   // a private input wire
    const uint64_t v = pos_in < nin ? in[pos_in] : 0;
    pos_in++;
    const uint32_t wire = cb.new_wire(v);
    if (cb.rec) cb.rec->input(wire);
    return cb.of_wire(wire);
  };
  auto inputs = [&](uint32_t n) { std::vector<V> r; for (uint32_t i = 0; i < n; i++) r.push_back(input()); return r; };
  if (name == "getType") { outs = {cb.get_type(input())}; }
  else if (name == "getX") { outs = {cb.get_x(input())}; }
  else if (name == "quinSelector") { const std::vector<V> arr = inputs(P(0)); const V idx = input(); outs = {cb.quin_selector(arr, idx)}; }
  else if (name == "getV") { const std::vector<V> b = inputs(P(0)); const V pos = input(); outs = {cb.get_v(b, pos)}; }
  else if (name == "decodeUint23") { outs = {cb.decode_uint23(input())}; }
  else if (name == "decodeUint") {   // inputs: bytes[N], pos, v
    const std::vector<V> b = inputs(P(0)); const V pos = input(); const V v = input();
    const CBuilder::UintOut o = cb.decode_uint(b, pos, v);
    outs = {o.value, o.next_pos};
  } else if (name == "readType") {
    const std::vector<V> b = inputs(P(0)); const V pos = input();
    const CBuilder::TypeOut o = cb.read_type(b, pos);
    outs = {o.next_pos, o.type, o.v};
  } else if (name == "skipValueScalar") { const std::vector<V> b = inputs(P(0)); const V pos = input(); outs = {cb.skip_value_scalar(b, pos)}; }
  else if (name == "skipValue") { const std::vector<V> b = inputs(P(0)); const V pos = input(); outs = {cb.skip_value(b, pos, P(1))}; }
  else if (name == "stringEquals") {   // params: N, constLen, const bytes...; inputs: bytes[N], pos, len
    const uint32_t cl = P(1);
    std::vector<uint8_t> cbts(cl);
    for (uint32_t i = 0; i < cl; i++) cbts[i] = (uint8_t)P(2 + i);
    const std::vector<V> b = inputs(P(0)); const V pos = input(); const V len = input();
    outs = {cb.string_equals(b, pos, len, cbts.data(), cl)};
  } else if (name == "readStringLength") {
    const std::vector<V> b = inputs(P(0)); const V pos = input();
    const CBuilder::LenOut o = cb.read_string_length(b, pos);
    outs = {o.len, o.next_pos};
  } else if (name == "readMapLength") {
    const std::vector<V> b = inputs(P(0)); const V pos = input();
    const CBuilder::LenOut o = cb.read_map_length(b, pos);
    outs = {o.len, o.next_pos};
  } else if (name == "copyString") {
    const std::vector<V> b = inputs(P(0)); const V pos = input();
    const CBuilder::CopyOut o = cb.copy_string(b, pos, P(1));
    outs = o.out; outs.push_back(o.next_pos); outs.push_back(o.len);
  } else if (name == "findVCAndExp" || name == "findCredSubj") {   // params: N, maxArr, maxMap; inputs: bytes[N], pos, mapLen
    static const uint8_t kVC[2] = {118, 99};
    static const uint8_t kCS[17] = {99, 114, 101, 100, 101, 110, 116, 105, 97, 108, 83, 117, 98, 106, 101, 99, 116};
    const std::vector<V> b = inputs(P(0)); const V pos = input(); const V ml = input();
    const bool vc = name == "findVCAndExp";
    const CBuilder::FindOut o = cb.find_in_map(b, pos, ml, P(1), P(2), vc ? kVC : kCS, vc ? 2 : 17, vc);
    outs = {o.needle_pos};
    if (vc) outs.push_back(o.exp_pos);
  } else if (name == "readCredSubj") {   // params: N, maxBufferLen; inputs: bytes[N], pos, mapLen
    const std::vector<V> b = inputs(P(0)); const V pos = input(); const V ml = input();
    const CBuilder::CredSubj o = cb.read_cred_subj(b, pos, ml, P(1));
    outs = o.given; outs.push_back(o.given_len);
    outs.insert(outs.end(), o.family.begin(), o.family.end()); outs.push_back(o.family_len);
    outs.insert(outs.end(), o.dob.begin(), o.dob.end()); outs.push_back(o.dob_len);
  } else if (name == "concatCredSubj") {   // params: maxBufferLen; inputs: given[M], givenLen, family[M], familyLen, dob[M], dobLen
    CBuilder::CredSubj cs;
    cs.given = inputs(P(0)); cs.given_len = input();
    cs.family = inputs(P(0)); cs.family_len = input();
    cs.dob = inputs(P(0)); cs.dob_len = input();
    const CBuilder::Concat o = cb.concat_cred_subj(cs, P(0));
    outs = o.result; outs.push_back(o.result_len);
  } else if (name == "sha256Var") {   // params: blockSpace; inputs: len_bits, then the message BYTES (bits are derived)
    const int bs = (int)P(0);
    const V len = input();
    std::vector<Bit> bits((size_t)512 << bs, bit_const(0));
    const uint32_t out_base = cb.new_wire(0);
    for (int i = 1; i < 256; i++) cb.new_wire(0);
    // (a recorded program takes every bit of the buffer as an input word of its own, whatever this call was given)
    for (uint32_t j = 0; (cb.rec || j + 1 < nin) && j < (64u << bs); j++)
      for (int i = 0; i < 8; i++) {
        const uint32_t wire = cb.new_wire(j + 1 < nin ? (in[1 + j] >> (7 - i)) & 1 : 0);
        if (cb.rec) cb.rec->input(wire);
        cb.boolean(wire);
        bits[(size_t)j * 8 + (size_t)i] = bit_wire(wire);
      }
    cb.sha256_var(bits, len, bs, out_base);
    for (int i = 0; i < 256; i++) outs.push_back(cb.of_wire(out_base + (uint32_t)i));
  } else {
    set_error("unknown gadget: " + name);
    return G16_E_ARG;
  }
  return G16_OK;
}

}  // namespace
}  // namespace g16

using namespace g16;

// Test-only: the SHA-256 circuits above, keyed with a known trapdoor.  Any output pointer may be NULL.
// r1cs: iden3 .r1cs v1 image of the same constraint system (for snarkjs / tools/r1cs_setup.py).
extern "C" int g16_sha256_chain_setup(uint32_t blocks, const uint8_t msg[32], uint64_t seed, int threads,
                                      uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                                      uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len) {
  if (!msg || blocks == 0 || blocks > 4096) { set_error("sha256 chain: bad arguments"); return G16_E_ARG; }
  ShaBuilder sb;
  build_sha256(sb, true, blocks, msg, 32);
  return emit(sb, "sha256 circuit too large", seed, threads, zkey, zkey_len, wtns, wtns_len, vkey, vkey_len, r1cs, r1cs_len);
}

extern "C" int g16_sha256_message_setup(const uint8_t* msg, uint32_t len, uint64_t seed, int threads,
                                        uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                                        uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len) {
  if ((!msg && len) || len > (1u << 20)) { set_error("sha256 message: bad arguments"); return G16_E_ARG; }
  ShaBuilder sb;
  const uint8_t none = 0;
  build_sha256(sb, false, 0, msg ? msg : &none, len);
  return emit(sb, "sha256 circuit too large", seed, threads, zkey, zkey_len, wtns, wtns_len, vkey, vkey_len, r1cs, r1cs_len);
}

extern "C" int g16_nzcp_fixed_layout_setup(const uint8_t* tbs, uint32_t len, const uint32_t seg_off[3],
                                          const uint32_t seg_len[3], uint32_t exp_off, uint64_t seed, int threads,
                                          uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                                          uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len) {
  if (!tbs || !seg_off || !seg_len || len == 0 || len > 4096 || (uint64_t)exp_off + 4 > len) {
    set_error("nzcp fixed layout: bad arguments");
    return G16_E_ARG;
  }
  for (int k = 0; k < 3; k++)
    if ((uint64_t)seg_off[k] + seg_len[k] > len) { set_error("nzcp fixed layout: segment out of range"); return G16_E_ARG; }
  ShaBuilder sb;
  build_nzcp_fixed_layout(sb, tbs, len, seg_off, seg_len, exp_off);
  return emit(sb, "sha256 circuit too large", seed, threads, zkey, zkey_len, wtns, wtns_len, vkey, vkey_len, r1cs, r1cs_len);
}

// Test-only: build ONE template of the NZCP circuit library over the given private inputs, check every emitted
// R1CS row on the computed witness and return the template's outputs.  G16_E_STATE + "constraint not satisfied:
// ..." when the inputs violate one of the template's `===` / Num2Bits range constraints (where circom's witness
// generator throws).  outputs: *nout in = capacity, out = count.
extern "C" int g16_nzcp_gadget(const char* name, const uint32_t* params, uint32_t nparams, const uint64_t* inputs,
                               uint32_t nin, uint64_t* outputs, uint32_t* nout, uint32_t* n_constraints) {
  if (!name || !nout || (nparams && !params) || (nin && !inputs)) { set_error("NULL argument"); return G16_E_ARG; }
  CBuilder cb;
  std::vector<CBuilder::V> outs;
  int rc = run_gadget(cb, name, params, nparams, inputs, nin, outs);
  if (rc) return rc;
  if (n_constraints) *n_constraints = (uint32_t)cb.c.rowA.size() - 1;
  const int64_t bad = first_unsatisfied_row(cb);
  if (!cb.ok) {
    set_error("constraint not satisfied: " + cb.fail);
    return G16_E_STATE;
  }
  if (bad >= 0) { set_error("internal: R1CS row " + std::to_string(bad) + " is not satisfied by the computed witness"); return G16_E_HIP; }
  if (outs.size() > *nout) { set_error("output buffer too small"); return G16_E_ARG; }
  for (size_t i = 0; i < outs.size(); i++) {
    uint64_t v = 0;
    if (!CBuilder::small_of(outs[i].val, v)) { set_error("gadget output is not a small integer"); return G16_E_STATE; }
    if (outputs) outputs[i] = v;
  }
  *nout = (uint32_t)outs.size();
  return G16_OK;
}

// Test-only: the full NZCPPubIdentity(IsLive, MaxToBeSignedBytes, MaxCborArrayLenVC, MaxCborMapLenVC,
// MaxCborArrayLenCredSubj, MaxCborMapLenCredSubj, CredSubjMaxBufferSpace) constraint system
// (/root/reference/circuits/nzcptpl.circom:433; nzcp_exampleTest.circom = (0, 314, 0, 4, 2, 4, 5),
// nzcp_liveTest.circom = (1, 355, 0, 4, 2, 4, 6)) with the CBOR search IN the circuit, its witness for the given
// ToBeSigned bytes, and a trapdoor proving key.  params = the seven template parameters in that order.
extern "C" int g16_nzcp_circuit_setup(const uint32_t params[7], const uint8_t* tbs, uint32_t len, uint64_t seed,
                                      int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                                      uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len,
                                      uint32_t* n_constraints) {
  if (!params || !tbs || params[1] == 0 || params[1] > 503 || params[6] < 2 || params[6] > 6 || len > params[1]) {
    set_error("nzcp circuit: bad arguments");
    return G16_E_ARG;
  }
  CBuilder cb;
  cb.nzcp_pub_identity(params[0] != 0, params[1], params[2], params[3], params[4], params[5], params[6], tbs, len);
  if (n_constraints) *n_constraints = cb.c.m;
  if (!cb.ok) { set_error("constraint not satisfied: " + cb.fail); return G16_E_STATE; }
  const int64_t bad = first_unsatisfied_row(cb);
  if (bad >= 0) { set_error("internal: R1CS row " + std::to_string(bad) + " is not satisfied by the computed witness"); return G16_E_HIP; }
  return emit(cb, "nzcp circuit too large", seed, threads, zkey, zkey_len, wtns, wtns_len, vkey, vkey_len, r1cs, r1cs_len);
}

// ---------------------------------------------------------------------------------------------------------
// Witness programs (witness_program.h): the builders above run once on an all-zero input with a recorder attached;
// what they record does not depend on the input (which wires exist, and what each is a function of, is decided by
// the template parameters alone).  The two builder-internal `violate` texts ("a bit-valued expression is not small",
// "exp is not a small integer") are not checks of the program: with bit-valued toBeSigned words they cannot fire.
extern "C" int g16_nzcp_witness_program(const uint32_t params[7], uint8_t** prog, size_t* len) {
  if (!prog || !len) { set_error("NULL argument"); return G16_E_ARG; }
  if (!params || params[1] == 0 || params[1] > 503 || params[6] < 2 || params[6] > 6) {
    set_error("nzcp circuit: bad arguments");
    return G16_E_ARG;
  }
  return no_bad_alloc("witness program", [&]() -> int {
    WpRecorder rec;
    CBuilder cb;
    cb.rec = &rec;
    const uint8_t none = 0;
    cb.nzcp_pub_identity(params[0] != 0, params[1], params[2], params[3], params[4], params[5], params[6], &none, 0);
    Buf z = rec.finish(cb.c.n, cb.c.p);
    if (!z.p) { set_error("witness program: out of memory"); return G16_E_STATE; }
    z.give(prog, len);
    return G16_OK;
  });
}

// One template of the library as a program: its private inputs are the program's input words, in run_gadget's order
// (sha256Var: the length in bits, then the 512 << blockSpace message BITS, MSB first per byte); every output value is
// settled on a wire of its own, listed in the program's outputs.
extern "C" int g16_nzcp_gadget_program(const char* name, const uint32_t* params, uint32_t nparams, uint8_t** prog, size_t* len) {
  if (!name || !prog || !len || (nparams && !params)) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("witness program", [&]() -> int {
    WpRecorder rec;
    CBuilder cb;
    cb.rec = &rec;
    std::vector<CBuilder::V> outs;
    if (const int rc = run_gadget(cb, name, params, nparams, nullptr, 0, outs)) return rc;
    rec.name_inputs("in", rec.n_inputs);
    for (const CBuilder::V& o : outs) {
      const uint32_t wire = cb.new_wire_fr(o.val);
      rec.quad(wire, {}, {}, o.lin.t);
      rec.outputs.push_back(wire);
    }
    Buf z = rec.finish((uint32_t)cb.w.size(), 0);
    if (!z.p) { set_error("witness program: out of memory"); return G16_E_STATE; }
    z.give(prog, len);
    return G16_OK;
  });
}
