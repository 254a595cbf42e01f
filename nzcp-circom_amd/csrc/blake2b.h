// Blake2b-512 (RFC 7693, unkeyed): the hash of the ceremony transcripts and of the circuit hash (blake2b.cpp).  Host
// code only: no HIP header, no internal.h, so a plain C++ program can compile the unit (tests/native/pair_checks_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace g16 {

void blake2b512(const uint8_t* data, size_t len, uint8_t out[64]);
// the same over a feed that arrives in parts of any length (empty ones included); final() once
class Blake2b512 {
 public:
  Blake2b512();
  void update(const uint8_t* data, size_t len);
  void final(uint8_t out[64]);

 private:
  uint64_t h_[8], t_ = 0;   // t_: bytes compressed so far
  uint8_t buf_[128];
  size_t have_ = 0;         // bytes held back in buf_, 0 .. 128
};

}  // namespace g16
