// The witness program (g16_wtns_calc): a recorded tape of how every wire of a natively built circuit is computed,
// independent of any particular input.  ShaBuilder / CBuilder append one op per wire they create or assign when a
// recorder is attached (sha_builder.h, nzcp_gadgets.h); the host evaluator (witness_program.cpp) and the device
// evaluator (wtns_calc.hip) walk the same tape.
//
// Ops.  A linear form <a,w> is a list of (wire, int64 coefficient) terms over EARLIER wires (wire 0 = the constant 1).
//   INPUT j     wire = input word j
//   QUAD        wire = <a,w> * <b,w> + <c,w>          (mul, settle, xor2, ch, maj, the padded-bit wires)
//   BITS n      the n listed target wires take the low n bits of <a,w>; a value of 2^n or more raises check k (when the
//               op has one) and the bits are those of 0, as in the builder          (num2bits, add_mod32)
//   INV0        wire = 1 / <a,w>, or 0 when <a,w> = 0
//   ISZ         wire = [<a,w> = 0]
//   CHECK k     <a,w> must be 0                         (assert_eq)
// Checks are numbered in build order; the status of a witness is the lowest violated one, which is the one the builder's
// `violate` keeps.  Every op carries its level = 1 + the highest level it reads (wire 0: level 0); ops are stored sorted
// by level (then by kind), with a level index, so that all ops of a level can run side by side.
//
// File image: the project's container (binfile.h), magic "wprg", version 1, little-endian u32 unless noted:
//   1 header    n_wires, n_public, n_inputs, n_ops, n_levels, n_terms, n_targets, n_checks, n_texts, n_names, n_outputs
//   2 ops       n_ops x {kind, dst, n, check, t_off, na, nb, nc}: the terms of a, b, c lie behind each other from t_off;
//               dst = the wire (INPUT: n = the input word; BITS: dst = the first of n entries of section 5)
//   3 terms     n_terms x {wire, coefficient: i64 as two words}
//   4 levels    n_levels + 1 op offsets: level l (from 1) = ops [lv[l - 1], lv[l])
//   5 targets   n_targets wires
//   6 checks    n_checks text ids, then n_texts x {length, bytes}
//   7 inputs    n_names x {first word, count, name length, bytes}
//   8 outputs   n_outputs wires (the public signals; a gadget program's output values)
#pragma once
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "circuit.h"
#include "wtns_calc_eval.cuh"

namespace g16 {

static constexpr uint32_t kWpMaxBits = 253;

struct WpTerm { uint32_t wire, lo, hi; };   // coefficient = (int64_t)(lo | hi << 32)
struct WpInput { std::string name; uint32_t first, count; };

struct WitnessProgram {
  uint32_t n_wires = 0, n_public = 0, n_inputs = 0;
  std::vector<WpOp> ops;
  std::vector<WpTerm> terms;
  std::vector<uint32_t> levels;     // n_levels + 1
  std::vector<uint32_t> targets;
  std::vector<uint32_t> check_text; // per check: an index into texts
  std::vector<std::string> texts;
  std::vector<WpInput> inputs;
  std::vector<uint32_t> outputs;
  // what the evaluators read instead of the int64 coefficients (filled by wp_load): per term the wire and an index
  // into coefs, the Montgomery images of the distinct coefficients; entries 0 and 1 are +1 and -1, which add and subtract
  std::vector<WpEvalTerm> eterms;
  std::vector<FrM> coefs;
  std::vector<int64_t> icoefs;
  std::vector<Fr> inv_small;   // 1 / k for k < kWpInvSmall, standard form
  WpView view() const { return WpView{ops.data(), eterms.data(), coefs.data(), icoefs.data(), targets.data(), inv_small.data()}; }
};

// ---------------------------------------------------------------- recording (the builders call these)
struct WpRecorder {
  using LinT = std::vector<std::pair<uint32_t, int64_t>>;
  struct Rec { uint32_t kind, dst, n, check, level; size_t t_off; uint32_t na, nb, nc; };
  std::vector<Rec> recs;
  std::vector<std::pair<uint32_t, int64_t>> terms;
  std::vector<uint32_t> targets, wire_level, check_text, outputs;
  std::vector<std::string> texts;
  std::unordered_map<std::string, uint32_t> text_id;
  std::vector<WpInput> inputs;
  uint32_t n_inputs = 0;

  void input(uint32_t wire);                       // the next input word
  void name_inputs(const char* name, uint32_t count);   // the last `count` input words are input `name`
  void quad(uint32_t wire, const LinT& a, const LinT& b, const LinT& c);
  void bits(const uint32_t* wires, uint32_t n, const LinT& a, const char* what);   // what == nullptr: no check
  void inv0(uint32_t wire, const LinT& a);
  void isz(uint32_t wire, const LinT& a);
  void check(const LinT& a, const char* what);
  // the recorded ops sorted by level -> the file image
  Buf finish(uint32_t n_wires, uint32_t n_public) const;

 private:
  uint32_t put(const LinT& l, uint32_t& level);    // merged like ShaBuilder::push; -> the number of terms kept
  uint32_t new_check(const char* what);
  void define(uint32_t wire, uint32_t level);
};

// ---------------------------------------------------------------- loading and evaluating
// Parses AND validates the image completely (every wire defined exactly once, every term reading a wire of a strictly
// lower level, every index, count and the level index in range, BITS n <= 253): G16_E_FORMAT with a text otherwise.
int wp_load(const uint8_t* buf, size_t len, WitnessProgram& out);
// One witness on the host: inputs = n_inputs canonical words; w = n_wires canonical standard-form words out;
// -> the lowest violated check or 0xffffffff
uint32_t wp_eval_host(const WitnessProgram& p, const uint8_t* inputs, Fr* w);

// ---------------------------------------------------------------- device route (wtns_calc.hip)
struct WcalcDevice;
int wcalc_device_create(int device, const WitnessProgram& p, uint32_t chunk, WcalcDevice** out);
void wcalc_device_destroy(WcalcDevice* d);
int wcalc_device_id(const WcalcDevice* d);
// count witnesses in chunks: inputs = count * n_inputs words (host); out_bodies (optional) = count * n_wires words
// (host); status = count words.  ms (optional): upload, kernel, download (device time, all chunks).
int wcalc_device_run(WcalcDevice* d, const uint8_t* inputs, size_t count, uint8_t* out_bodies, uint32_t* status, float ms[3]);
// one witness evaluated on `st` into d_out (n_wires words on d's device); *status once the call returns (it waits)
int wcalc_device_run_into(WcalcDevice* d, const uint8_t* inputs, Fr* d_out, hipStream_t st, uint32_t* status);
// Chunks that stay on the device, for a prover there (g16_fullprove_batch, g16_plonk_fullprove_batch).  The calculator
// keeps two chunk buffers of up to wcalc_chunk_size witnesses each (at most 2 x 4 GiB of device memory, grown on demand).
struct WcalcChunk {
  const Fr* d_w = nullptr;            // cnt * n_wires words on the device, valid for a stream that waited for `ready`
  const uint32_t* status = nullptr;   // cnt words, pinned: valid on the host once `ready` has completed
  const uint8_t* pub = nullptr;       // cnt * n_public words side by side, pinned (nullptr: not asked for, or none)
  hipEvent_t ready = nullptr;
};
uint32_t wcalc_chunk_size(const WcalcDevice* d);
// cnt <= wcalc_chunk_size witnesses into buffer `which` (0 or 1) on the calculator's own stream: enqueues only.
// `inputs` (host, cnt * n_inputs words) is read until `ready`.  The caller releases the buffer first: what still reads
// its previous chunk is named to wcalc_chunk_release, whose events the calculator's stream waits for.
int wcalc_chunk_launch(WcalcDevice* d, int which, const uint8_t* inputs, uint32_t cnt, bool want_pub, WcalcChunk* out);
// ... with the input words formed on the device: `fill` enqueues on the calculator's stream `st` whatever writes all
// cnt * n_inputs words at d_in (standard form, below r); what it reads stays alive until `ready`
using WcalcFill = std::function<int(Fr* d_in, uint32_t cnt, hipStream_t st)>;
int wcalc_chunk_launch_from(WcalcDevice* d, int which, const WcalcFill& fill, uint32_t cnt, bool want_pub, WcalcChunk* out);
int wcalc_chunk_release(WcalcDevice* d, hipEvent_t ev);
void wcalc_chunk_drain(WcalcDevice* d);   // error paths: the calculator's stream, synchronised

}  // namespace g16

// the handle of the C ABI (witness_program.cpp; g16_stage_inputs in prover.cpp reads it)
struct g16_wtns_calculator {
  g16::WitnessProgram p;
  int device = -1;
  g16::WcalcDevice* dev = nullptr;
  float ms[3] = {0.f, 0.f, 0.f};
};
// the input words of `count` witnesses: the right number of them, every one below r (the text names the first that is not)
int wcalc_check_inputs(const g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count);
// what a prover on `device` with a key of n_wires wires and n_public public signals refuses, "<who>: ..." (G16_E_STATE): a
// calculator on the host route or on another device, a program with other counts
int wcalc_match_prover(const g16_wtns_calculator* h, const char* who, int device, uint32_t n_wires, uint32_t n_public);

// ---------------------------------------------------------------- the batched fullprove over a source of input words
// g16_fullprove_batch (prover.cpp) and g16_plonk_fullprove_batch (plonk.hip) are one routine each over a source: the
// caller's host words there, a kernel that forms the words where they are consumed for the pass prover (pass_prove.hip).
struct g16_prover;
struct g16_plonk;
struct g16_plonk_proof;
namespace g16 {
struct FullproveSource {
  const char* who = "fullprove";   // the head of the texts
  // enqueue on the calculator's stream what writes the input words of witnesses [at, at + cnt) of the batch at d_in
  std::function<int(Fr* d_in, size_t at, uint32_t cnt, hipStream_t st)> fill;
  // optional: asked for every witness without a violated check once its chunk's status words and public signals are on
  // the host (pub_row: its public signals when the call asked for them).  0: prove it; 1: leave it out, proof and row
  // zero as for a violated check; negative: the call fails with this code
  std::function<int(size_t i, const uint8_t* pub_row)> gate;
};
// lock the prover (held by lk from here on), then its refusals and wcalc_match_prover's behind `who`
int fullprove_enter(g16_prover* p, const g16_wtns_calculator* h, const char* who, std::unique_lock<std::mutex>& lk);
// count >= 1 witnesses; the lock is held.  On an error exit the contexts and the calculator's stream are drained
int fullprove_run(g16_prover* p, g16_wtns_calculator* h, const FullproveSource& src, size_t count, const uint8_t* rs,
                  g16_proof* out, uint8_t* pub, uint32_t* status);
int plonk_fullprove_enter(g16_plonk* p, const g16_wtns_calculator* h, const char* who, std::unique_lock<std::mutex>& lk);
int plonk_fullprove_run(g16_plonk* p, g16_wtns_calculator* h, const FullproveSource& src, size_t count, const uint8_t* blinding,
                        g16_plonk_proof* out, uint8_t* pub, uint32_t* status);
}  // namespace g16
