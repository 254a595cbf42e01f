// The iden3 "binfile" container every .zkey, .wtns, .r1cs and .ptau arrives in ([EXT]
// @iden3/binfileutils readBinFile): magic[4], u32 version, u32 section count, then {u32 id, u64 size, bytes} records.
// The ONLY place the framing is read (bin_open) or written (bin_layout), and the {n8 = 32, prime} record that opens
// every header section (bin_put_field / bin_is_field).  Host code only: no HIP header, no internal.h, so a plain C++
// program with its own g16::set_error can compile it (tests/native/binfile_test.cpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/g16_prover.h"
#include "bn254_consts.h"

namespace g16 {

void set_error(const std::string& msg);

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

inline bool fr_below_modulus(const uint32_t s[8]) {   // s (8 x 32-bit LE limbs) < r
  for (int i = 7; i >= 0; i--)
    if (s[i] != kFrP[i]) return s[i] < kFrP[i];
  return false;
}

// ------------------------------------------------------------------ reading
struct BinSection { const uint8_t* p = nullptr; uint64_t size = 0; };   // p == nullptr: absent (a present empty section has p != nullptr)
struct BinView { uint32_t version = 0; BinSection sec[16]; };
enum class BinFault { none, magic, version, table, section };   // table: a record header runs past the end; section: its bytes do

// The section table of buf[0, len) -> out (reset first, so a reused view keeps nothing).  The first occurrence of an
// id wins; ids of 16 or more are skipped (no reader looks one up).  A fault sets "<magic>: Invalid File format" -- "Version not supported" for a version above
// max_version -- and returns G16_E_FORMAT; *why tells the caller that words its own texts which check failed.
inline int bin_open(const uint8_t* buf, size_t len, const char magic[4], uint32_t max_version, BinView& out,
                    BinFault* why = nullptr) {
  auto fault = [&](BinFault f) {
    if (why) *why = f;
    set_error(f == BinFault::version ? std::string("Version not supported") : std::string(magic, 4) + ": Invalid File format");
    return G16_E_FORMAT;
  };
  if (why) *why = BinFault::none;
  out = BinView{};
  if (!buf || len < 12 || memcmp(buf, magic, 4) != 0) return fault(BinFault::magic);
  out.version = rd32(buf + 4);
  if (out.version > max_version) return fault(BinFault::version);
  const uint32_t nsec = rd32(buf + 8);
  size_t pos = 12;
  for (uint32_t i = 0; i < nsec; i++) {
    if (pos + 12 > len) return fault(BinFault::table);     // (pos <= len, so no wrap)
    const uint32_t id = rd32(buf + pos);
    const uint64_t size = rd64(buf + pos + 4);
    pos += 12;
    if (size > len - pos) return fault(BinFault::section);
    if (id < 16 && !out.sec[id].p) out.sec[id] = {buf + pos, size};
    pos += size;
  }
  return G16_OK;
}

// {u32 n8 = 32, the 32 bytes of `prime`}: 36 bytes at p, of which `avail` are there
inline bool bin_is_field(const uint8_t* p, uint64_t avail, const uint32_t prime[8]) {
  return avail >= 36 && rd32(p) == 32 && memcmp(p + 4, prime, 32) == 0;
}

// ------------------------------------------------------------------ writing
// A malloc'd image on its way to the caller of the C ABI (g16_free).  It owns the image until give() hands it out: an
// early return or an exception before that frees it.  Move-only.
struct Buf {
  uint8_t* p = nullptr;
  size_t len = 0, cap = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), len(o.len), cap(o.cap) { o.p = nullptr; o.len = o.cap = 0; }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { free(p); }
  bool reserve(size_t c) {   // once, on an empty Buf
    p = (uint8_t*)malloc(c ? c : 1);
    cap = c;
    return p != nullptr;
  }
  void put(const void* src, size_t n) { memcpy(p + len, src, n); len += n; }
  void u32(uint32_t v) { put(&v, 4); }
  void u64(uint64_t v) { put(&v, 8); }
  uint8_t* skip(size_t n) { uint8_t* q = p + len; len += n; return q; }
  void give(uint8_t** out, size_t* out_len) {   // the image is the caller's from here on
    *out = p; *out_len = len;
    p = nullptr; len = cap = 0;
  }
};

// The whole image reserved and framed: header, then for each of ids[0, nids) (each below 16, in file order) its record
// header and sizes[id] bytes left for the caller at sec[id].  false: the reservation failed (the caller words the error).
inline bool bin_layout(Buf& z, const char magic[4], uint32_t version, const int* ids, int nids, const uint64_t sizes[16],
                       uint8_t* sec[16]) {
  size_t total = 12;
  for (int k = 0; k < nids; k++) total += 12 + sizes[ids[k]];
  if (!z.reserve(total)) return false;
  z.put(magic, 4); z.u32(version); z.u32((uint32_t)nids);
  for (int k = 0; k < nids; k++) {
    z.u32((uint32_t)ids[k]); z.u64(sizes[ids[k]]);
    sec[ids[k]] = z.skip(sizes[ids[k]]);
  }
  return true;
}

inline uint8_t* bin_put_field(uint8_t* q, const uint32_t prime[8]) {   // -> q + 36
  const uint32_t n8 = 32;
  memcpy(q, &n8, 4);
  memcpy(q + 4, prime, 32);
  return q + 36;
}

}  // namespace g16
