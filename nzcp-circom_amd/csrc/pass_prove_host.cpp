// The holder's side of NZCP passes (include/g16_prover.h, "Proving passes from their URIs"): g16_pass_fullprove_batch,
// g16_plonk_pass_fullprove_batch and the layer operator g16_pass_inputs.  The checks, the outcome of every pass and the
// host-thread route live here; the kernel that forms the input words is pass_prove.hip, the front end pass_verify.hip,
// the proofs the batched fullprove routines of prover.cpp and plonk.hip over a device-side source (witness_program.h).
#include <string.h>
#include <string>
#include <thread>
#include <vector>

#include "fixed_base.h"
#include "internal.h"
#include "pass_prove.h"
#include "witness_program.h"

using namespace g16;

namespace {

constexpr uint32_t kNzcpPublic = 513;   // NZCPPubIdentity: 256 + 256 digest bits, exp

bool well_formed(uint32_t verdict) { return verdict != G16_PASS_MALFORMED && verdict != G16_PASS_TOO_LONG; }

// M of a program whose named inputs are exactly toBeSigned[8 M], toBeSignedLen; 0 otherwise
uint32_t program_max_bytes(const g16_wtns_calculator* h) {
  const std::vector<WpInput>& in = h->p.inputs;
  if (in.size() != 2 || in[0].name != "toBeSigned" || in[1].name != "toBeSignedLen" || in[0].first != 0 || in[1].count != 1 ||
      in[0].count % 8 || in[1].first != in[0].count || h->p.n_inputs != in[0].count + 1)
    return 0;
  const uint32_t m = in[0].count / 8;
  return m <= kPassInputsMaxBytes ? m : 0;
}

bool word_is(const uint8_t* w, uint64_t v) {
  for (int k = 0; k < 32; k++)
    if (w[k] != (k < 8 ? (uint8_t)(v >> (8 * k)) : 0)) return false;
  return true;
}
// the MATCH_PUBLIC relation: the witness's 513 public signals against the front end's record
bool public_matches(const uint8_t* pub, const g16_pass_result& r) {
  if (!(r.flags & G16_PASS_HAS_SUBJECT) || r.exp < 0) return false;
  for (uint32_t k = 0; k < 256; k++) {
    if (!word_is(pub + (size_t)k * 32, (r.cred_subj_sha256[k >> 3] >> (7 - (k & 7))) & 1u)) return false;
    if (!word_is(pub + (size_t)(256 + k) * 32, (r.tbs_sha256[k >> 3] >> (7 - (k & 7))) & 1u)) return false;
  }
  return word_is(pub + (size_t)512 * 32, (uint64_t)r.exp);
}

// What the two provers differ in: the size of a proof and of its blinding, and how the batched fullprove is run.
struct ProverSide {
  std::string who;
  uint32_t n_public;
  size_t proof_bytes, blind_bytes;
  std::function<int(const FullproveSource&, size_t, const uint8_t*, uint8_t*, uint8_t*, uint32_t*)> run;
};

// after the prover is locked and matched against the calculator
int pass_prove(const ProverSide& P, g16_wtns_calculator* h, g16_pass_verifier* V, const uint8_t* text, const uint64_t* offsets,
               size_t count, int64_t now, uint32_t flags, const uint8_t* blind, uint8_t* out, uint8_t* pub, g16_pass_prove_result* res) {
  const std::string& who = P.who;
  const int device = wcalc_device_id(h->dev);   // (the prover's: matched)
  if (!V->dev) { set_error(who + ": the pass verifier runs on the host route (create it on the prover's device)"); return G16_E_STATE; }
  if (pass_device_id(V->dev) != device) {
    set_error(who + ": the pass verifier is on device " + std::to_string(pass_device_id(V->dev)) + ", the prover on device " + std::to_string(device));
    return G16_E_STATE;
  }
  const uint32_t M = program_max_bytes(h);
  if (M == 0) { set_error(who + ": the program's inputs are not toBeSigned[8 M] and toBeSignedLen"); return G16_E_ARG; }
  if (flags & ~(G16_PASS_PROVE_UNSIGNED | G16_PASS_PROVE_MATCH_PUBLIC)) { set_error(who + ": unknown flags"); return G16_E_ARG; }
  const bool match = (flags & G16_PASS_PROVE_MATCH_PUBLIC) != 0, unsigned_too = (flags & G16_PASS_PROVE_UNSIGNED) != 0;
  if (match && P.n_public != kNzcpPublic) {
    set_error(who + ": MATCH_PUBLIC takes the 513 public signals of NZCPPubIdentity, the program has " + std::to_string(P.n_public));
    return G16_E_ARG;
  }
  if (const int rc = pass_check_items(who.c_str(), text, offsets, count)) return rc;
  if (count == 0) return G16_OK;
  if (!out || !res) { set_error("NULL argument"); return G16_E_ARG; }
  std::lock_guard<std::mutex> vlk(V->mu);

  // the front end and the signatures, as g16_pass_verify_batch runs them
  std::vector<g16_pass_result> records(count);
  std::vector<uint8_t> ok(count);
  if (const int rc = pass_device_batch(V->dev, es256_verifier_device(V->es), text, offsets, count, records.data(), ok.data(), V->last_ms))
    return rc;
  const size_t pub_bytes = (size_t)P.n_public * 32;
  std::vector<uint32_t> sel;
  for (size_t i = 0; i < count; i++) {
    g16_pass_result& r = records[i];
    r.verdict = pass_merge(r.verdict, ok[i] != 0, r.nbf, r.exp, now);
    const bool passes = r.verdict == G16_PASS_OK || (unsigned_too && r.verdict >= G16_PASS_KEY && r.verdict <= G16_PASS_EXPIRED);
    res[i].pass = r;
    res[i].check = 0xffffffffu;
    res[i].outcome = !passes ? G16_PROVE_PASS : r.tbs_len > M ? G16_PROVE_TOO_LONG : G16_PROVE_DONE;
    memset(out + i * P.proof_bytes, 0, P.proof_bytes);
    if (pub) memset(pub + i * pub_bytes, 0, pub_bytes);
    if (res[i].outcome == G16_PROVE_DONE) sel.push_back((uint32_t)i);
  }
  const size_t n = sel.size();
  if (n == 0) return G16_OK;

  // the selected passes, side by side: their blinding in, their proofs, public signals and status words out
  const bool want_pub = pub || match;
  std::vector<uint8_t> c_blind(blind ? n * P.blind_bytes : 0), c_out(n * P.proof_bytes), c_pub(want_pub ? n * pub_bytes : 0);
  std::vector<uint32_t> c_status(n, 0xffffffffu);
  if (blind)
    for (size_t j = 0; j < n; j++) memcpy(&c_blind[j * P.blind_bytes], blind + sel[j] * P.blind_bytes, P.blind_bytes);

  const hipError_t e0 = hipSetDevice(device);
  if (e0 != hipSuccess) { set_error(who + ": " + hipGetErrorString(e0)); return G16_E_HIP; }
  DeviceJob job(P.who.c_str());
  DeviceBuf<uint32_t> d_sel, d_bad;   // (freed after the run has drained every stream that reads them, on every path)
  PinnedBuf<uint32_t> h_bad;
  if (job.fail(d_sel.alloc(n)) || job.fail(d_bad.alloc(n)) || job.fail(h_bad.alloc(n)) ||
      job.fail(hipMemcpy(d_sel.p, sel.data(), n * 4, hipMemcpyHostToDevice)))
    return job.rc;
  const uint8_t* d_text = nullptr;
  const uint64_t* d_offsets = nullptr;
  pass_device_uploaded(V->dev, &d_text, &d_offsets);   // (the ES256 stream has passed the batch: nothing writes them now)

  FullproveSource src;
  src.who = P.who.c_str();
  src.fill = [&](Fr* d_in, size_t at, uint32_t cnt, hipStream_t st) -> int {
    if (const int rc = pass_inputs_enqueue(d_text, d_offsets, d_sel.p + at, cnt, M, d_in, d_bad.p + at, st)) return rc;
    G16_HIP(hipMemcpyAsync(h_bad.p + at, d_bad.p + at, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    return G16_OK;
  };
  src.gate = [&](size_t j, const uint8_t* pub_row) -> int {
    if (h_bad.p[j]) {
      set_error(who + ": the device disagrees with the front end on pass " + std::to_string(sel[j]));
      return G16_E_STATE;
    }
    if (match && !(pub_row && public_matches(pub_row, records[sel[j]]))) {
      res[sel[j]].outcome = G16_PROVE_MISMATCH;
      return 1;
    }
    return 0;
  };
  if (const int rc = P.run(src, n, blind ? c_blind.data() : nullptr, c_out.data(), want_pub ? c_pub.data() : nullptr, c_status.data()))
    return rc;
  for (size_t j = 0; j < n; j++) {
    g16_pass_prove_result& r = res[sel[j]];
    if (c_status[j] != 0xffffffffu) {
      r.outcome = G16_PROVE_CHECK;
      r.check = c_status[j];
    }
    if (r.outcome != G16_PROVE_DONE) continue;
    memcpy(out + sel[j] * P.proof_bytes, &c_out[j * P.proof_bytes], P.proof_bytes);
    if (pub) memcpy(pub + sel[j] * pub_bytes, &c_pub[j * pub_bytes], pub_bytes);
  }
  return G16_OK;
}

}  // namespace

extern "C" int g16_pass_fullprove_batch(g16_prover* p, g16_wtns_calculator* h, g16_pass_verifier* v, const uint8_t* text,
                                        const uint64_t* offsets, size_t count, int64_t now, uint32_t flags, const uint8_t* rs,
                                        g16_proof* out, uint8_t* pub, g16_pass_prove_result* res) {
  if (!p || !h || !v) { set_error("NULL argument"); return G16_E_ARG; }
  std::unique_lock<std::mutex> lk;
  if (const int rc = fullprove_enter(p, h, "pass prove", lk)) return rc;
  return no_bad_alloc("pass prove", [&]() -> int {
    ProverSide P{"pass prove", h->p.n_public, sizeof(g16_proof), 64, nullptr};
    P.run = [&](const FullproveSource& src, size_t n, const uint8_t* blind, uint8_t* o, uint8_t* pb, uint32_t* st) {
      return fullprove_run(p, h, src, n, blind, (g16_proof*)o, pb, st);
    };
    return pass_prove(P, h, v, text, offsets, count, now, flags, rs, (uint8_t*)out, pub, res);
  });
}

extern "C" int g16_plonk_pass_fullprove_batch(g16_plonk* p, g16_wtns_calculator* h, g16_pass_verifier* v, const uint8_t* text,
                                              const uint64_t* offsets, size_t count, int64_t now, uint32_t flags,
                                              const uint8_t* blinding, g16_plonk_proof* out, uint8_t* pub, g16_pass_prove_result* res) {
  if (!p || !h || !v) { set_error("NULL argument"); return G16_E_ARG; }
  std::unique_lock<std::mutex> lk;
  if (const int rc = plonk_fullprove_enter(p, h, "plonk pass prove", lk)) return rc;
  return no_bad_alloc("plonk pass prove", [&]() -> int {
    ProverSide P{"plonk pass prove", h->p.n_public, sizeof(g16_plonk_proof), 9 * 32, nullptr};
    P.run = [&](const FullproveSource& src, size_t n, const uint8_t* blind, uint8_t* o, uint8_t* pb, uint32_t* st) {
      return plonk_fullprove_run(p, h, src, n, blind, (g16_plonk_proof*)o, pb, st);
    };
    return pass_prove(P, h, v, text, offsets, count, now, flags, blinding, (uint8_t*)out, pub, res);
  });
}

// The calculator alone over pass URIs, fed by pass_inputs_kernel: no key, no proof, no signature work.
extern "C" int g16_pass_wtns_public(g16_wtns_calculator* h, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* pub,
                                    uint32_t* status) {
  const std::string who = "pass witness";
  if (!h) { set_error("NULL argument"); return G16_E_ARG; }
  if (!h->dev) { set_error(who + ": the calculator runs on the host route"); return G16_E_STATE; }
  const uint32_t M = program_max_bytes(h);
  if (M == 0) { set_error(who + ": the program's inputs are not toBeSigned[8 M] and toBeSignedLen"); return G16_E_ARG; }
  if (const int rc = pass_check_items(who.c_str(), text, offsets, count)) return rc;
  if (count == 0) return G16_OK;
  if (!pub || !status) { set_error("NULL argument"); return G16_E_ARG; }
  return no_bad_alloc("pass witness", [&]() -> int {
    const int device = wcalc_device_id(h->dev);
    const size_t pub_bytes = (size_t)h->p.n_public * 32, text_bytes = (size_t)(offsets[count] - offsets[0]);
    std::vector<g16_pass_result> records(count);
    if (const int rc = pass_device_op(device, kPassOpFront, text, offsets, count, (uint8_t*)records.data())) return rc;
    std::vector<uint32_t> sel;
    memset(pub, 0, count * pub_bytes);
    for (size_t i = 0; i < count; i++) {
      status[i] = G16_PASS_WTNS_NO_ROW;
      if (well_formed(records[i].verdict) && records[i].tbs_len <= M) sel.push_back((uint32_t)i);
    }
    const size_t n = sel.size();
    if (n == 0) return G16_OK;
    const hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess) { set_error(who + ": " + hipGetErrorString(e0)); return G16_E_HIP; }
    DeviceJob job("pass witness");
    DeviceBuf<uint8_t> d_text;   // (the calculator's stream is drained before these go, on every path)
    DeviceBuf<uint64_t> d_offsets;
    DeviceBuf<uint32_t> d_sel, d_bad;
    PinnedBuf<uint32_t> h_bad;
    if (job.fail(d_text.alloc(text_bytes)) || job.fail(d_offsets.alloc(count + 1)) || job.fail(d_sel.alloc(n)) || job.fail(d_bad.alloc(n)) ||
        job.fail(h_bad.alloc(n)) || (text_bytes && job.fail(hipMemcpy(d_text.p, text + offsets[0], text_bytes, hipMemcpyHostToDevice))) ||
        job.fail(hipMemcpy(d_offsets.p, offsets, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice)) ||
        job.fail(hipMemcpy(d_sel.p, sel.data(), n * 4, hipMemcpyHostToDevice)))
      return job.rc;
    const size_t chunk = wcalc_chunk_size(h->dev);
    for (size_t at = 0; at < n; at += chunk) {
      const uint32_t cnt = (uint32_t)(n - at < chunk ? n - at : chunk);
      WcalcChunk c;
      int rc = wcalc_chunk_launch_from(h->dev, 0, [&](Fr* d_in, uint32_t k, hipStream_t st) -> int {
        if (const int e = pass_inputs_enqueue(d_text.p, d_offsets.p, d_sel.p + at, k, M, d_in, d_bad.p + at, st)) return e;
        G16_HIP(hipMemcpyAsync(h_bad.p + at, d_bad.p + at, (size_t)k * 4, hipMemcpyDeviceToHost, st));
        return G16_OK;
      }, cnt, true, &c);
      if (!rc && job.fail(hipEventSynchronize(c.ready))) rc = job.rc;
      if (rc) { wcalc_chunk_drain(h->dev); return rc; }
      for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t i = sel[at + j];
        if (h_bad.p[at + j]) {
          set_error(who + ": the device disagrees with the front end on pass " + std::to_string(i));
          return G16_E_STATE;
        }
        status[i] = c.status[j];
        if (c.status[j] == 0xffffffffu && c.pub) memcpy(pub + i * pub_bytes, c.pub + j * pub_bytes, pub_bytes);
      }
    }
    return G16_OK;
  });
}

extern "C" int g16_pass_inputs(int device, const uint8_t* text, const uint64_t* offsets, size_t count, uint32_t max_bytes,
                               uint8_t* out_words, uint8_t* ok) {
  if (device < -1) { set_error("pass inputs: bad device ordinal"); return G16_E_ARG; }
  if (max_bytes < 1 || max_bytes > kPassInputsMaxBytes) {
    set_error("pass inputs: max_bytes must be 1 to " + std::to_string(kPassInputsMaxBytes));
    return G16_E_ARG;
  }
  if (count && (!out_words || !ok)) { set_error("NULL argument"); return G16_E_ARG; }
  if (const int rc = pass_check_items("pass inputs", text, offsets, count)) return rc;
  if (count == 0) return G16_OK;
  const size_t row_bytes = (size_t)pass_input_count(max_bytes) * 32;
  return no_bad_alloc("pass inputs", [&]() -> int {
    if (device < 0) {
      parallel_for(count, host_threads(count), [&](size_t lo, size_t hi) {
        uint8_t dec[kPassDecodedMax], sig[64];
        uint32_t stack[kPassCborDepth];
        g16_pass_result r;
        for (size_t i = lo; i < hi; i++) {
          const uint8_t* item = text + offsets[i];
          const uint64_t n = offsets[i + 1] - offsets[i];
          uint8_t* row = out_words + i * row_bytes;
          pass_uri_one(item, n, nullptr, 0, dec, stack, &r, sig);   // the whole front end: is the pass well-formed?
          ok[i] = pass_inputs_one(item, n, max_bytes, dec, stack, row) && well_formed(r.verdict);
          if (!ok[i]) memset(row, 0, row_bytes);
        }
      });
      return G16_OK;
    }
    // the device route: the front end decides which passes have a row (pass_verify.hip), pass_inputs_kernel writes them
    std::vector<g16_pass_result> records(count);
    if (const int rc = pass_device_op(device, kPassOpFront, text, offsets, count, (uint8_t*)records.data())) return rc;
    std::vector<uint32_t> sel;
    for (size_t i = 0; i < count; i++) {
      ok[i] = well_formed(records[i].verdict) && records[i].tbs_len <= max_bytes;
      if (ok[i]) sel.push_back((uint32_t)i);
      else memset(out_words + i * row_bytes, 0, row_bytes);
    }
    std::vector<uint32_t> bad(sel.size() + 1);
    if (const int rc = pass_device_inputs(device, text, offsets, count, sel.data(), sel.size(), max_bytes, out_words, bad.data())) return rc;
    for (size_t j = 0; j < sel.size(); j++)
      if (bad[j]) {
        set_error("pass inputs: the device disagrees with the front end on pass " + std::to_string(sel[j]));
        return G16_E_STATE;
      }
    return G16_OK;
  });
}
