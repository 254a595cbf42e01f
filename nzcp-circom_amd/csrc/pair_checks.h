// A batch of pairing-equality checks for the ceremony verifiers: every check e(P1, Q1) = e(P2, Q2) is collected, ONE
// g16_pairing_op call computes all pairings, and the verdict is the reason of the first check that does not hold.  The
// batch owns its words: a point is copied the moment it is added, so the caller's buffers need not outlive the call.
// Host code; no HIP header, no internal.h (tests/native/pair_checks_test.cpp runs it against a host pairing).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/g16_prover.h"
#include "ec.cuh"

namespace g16 {

// one side of a pairing: a file image (affine little-endian Montgomery) or standard-form words (what the MSM operators
// return); G1 = 2 coordinates, G2 = 4.  Never the point at infinity: the routes test that first, with their own texts.
struct PairPoint { const uint8_t* p; bool std_words; };
inline PairPoint pair_image(const uint8_t* lem) { return PairPoint{lem, false}; }
inline PairPoint pair_words(const uint8_t* std_form) { return PairPoint{std_form, true}; }

class PairChecks {
 public:
  // e(p1, q1) = e(p2, q2)
  void equal(PairPoint p1, PairPoint q1, PairPoint p2, PairPoint q2, const char* why) {
    put(p1, 2); put(q1, 4);
    put(p2, 2); put(q2, 4);
    why_.push_back(why);
  }
  // four file images: a and b have the ratio of c and d, e(a, d) = e(b, c)
  void same_ratio(const uint8_t* g1a, const uint8_t* g1b, const uint8_t* g2c, const uint8_t* g2d, const char* why) {
    equal(pair_image(g1a), pair_image(g2d), pair_image(g1b), pair_image(g2c), why);
  }
  uint32_t pairs() const { return (uint32_t)(in_.size() / 192); }
  const std::vector<uint8_t>& words() const { return in_; }   // g16_pairing_op's input: 192 bytes per pair
  // the single device call (none for an empty batch) -> its code
  int run(int device) {
    gt_.assign((size_t)pairs() * 384, 0);
    return pairs() ? g16_pairing_op(device, in_.data(), pairs(), gt_.data()) : G16_OK;
  }
  // after run(): the reason of the lowest-numbered check whose two pairings differ, or nullptr.  (Checks that were
  // never run do not hold.)
  const char* first_failure() const {
    for (size_t c = 0; c < why_.size(); c++)
      if (gt_.size() < (2 * c + 2) * 384 || memcmp(gt_.data() + 2 * c * 384, gt_.data() + (2 * c + 1) * 384, 384) != 0) return why_[c];
    return nullptr;
  }

 private:
  void put(PairPoint v, int coords) {
    const size_t at = in_.size();
    in_.resize(at + 32 * (size_t)coords);
    if (v.std_words) { memcpy(in_.data() + at, v.p, 32 * (size_t)coords); return; }
    for (int i = 0; i < coords; i++) {
      Fq x;
      memcpy(x.v, v.p + 32 * i, 32);
      x = fp_from_mont(x);
      memcpy(in_.data() + at + 32 * i, x.v, 32);
    }
  }
  std::vector<uint8_t> in_, gt_;
  std::vector<const char*> why_;
};

}  // namespace g16
