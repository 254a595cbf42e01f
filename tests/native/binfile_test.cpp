// Stand-alone memory-safety test of csrc/binfile.h, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_binfile_native.py).  A three-section file lives in a heap buffer of EXACTLY its length, so any read
// past what bin_open was given is a heap overflow the sanitizer reports.  bin_open runs on every prefix length, and at
// each length with every section-size field overwritten by {0, 1, len, 2^40, 2^64 - 1}: the answer must be a clean
// error (G16_E_FORMAT, a fault kind, a text) or a view whose sections lie inside the buffer.  Then bin_layout is read
// back by bin_open.
#include <stdio.h>

#include <utility>
#include <vector>

#include "binfile.h"

static std::string g_err;
namespace g16 {
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace g16
using namespace g16;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

// bin_open on a heap copy of exactly `len` bytes (a null pointer for len 0 would hide nothing: malloc(0) is a valid,
// zero-sized block to the sanitizer); -> whether it parsed
static bool open_exact(const uint8_t* img, size_t len, uint32_t max_version) {
  uint8_t* buf = (uint8_t*)malloc(len);
  CHECK(buf != nullptr);
  if (len) memcpy(buf, img, len);
  BinView v;
  BinFault why = BinFault::none;
  g_err.clear();
  const int rc = bin_open(buf, len, "test", max_version, v, &why);
  if (rc == G16_OK) {
    CHECK(why == BinFault::none);
    for (int id = 0; id < 16; id++) {
      const BinSection& s = v.sec[id];
      if (!s.p) { CHECK(s.size == 0); continue; }
      CHECK(s.p >= buf + 24 && s.p <= buf + len && s.size <= (uint64_t)(buf + len - s.p));
      uint64_t sum = 0;
      for (uint64_t i = 0; i < s.size; i++) sum += s.p[i];   // every byte of the section is readable
      CHECK(sum <= 255 * s.size);
    }
  } else {
    CHECK(rc == G16_E_FORMAT && why != BinFault::none);
    CHECK(g_err == (why == BinFault::version ? "Version not supported" : "test: Invalid File format"));
  }
  free(buf);
  return rc == G16_OK;
}

static Buf filled(size_t n) {   // by value, as write_wtns / write_r1cs return theirs
  Buf b;
  CHECK(b.reserve(n));
  for (size_t i = 0; i < n; i++) { const uint8_t v = (uint8_t)i; b.put(&v, 1); }
  return b;
}

int main() {
  // sections 1 (5 bytes), 3 (empty) and 2 (9 bytes), in that order
  static const int ids[3] = {1, 3, 2};
  uint64_t sizes[16] = {};
  sizes[1] = 5; sizes[3] = 0; sizes[2] = 9;
  Buf z;
  uint8_t* sec[16] = {};
  CHECK(bin_layout(z, "test", 2, ids, 3, sizes, sec));
  const size_t total = 12 + 3 * 12 + 5 + 0 + 9;
  CHECK(z.len == total && z.cap == total);
  for (int id = 1; id <= 3; id++) memset(sec[id], 0x10 * id, sizes[id]);
  const size_t size_at[3] = {12 + 4, 12 + 12 + 5 + 4, 12 + 12 + 5 + 12 + 4};   // the three u64 size fields

  {   // round trip: what bin_layout framed, bin_open finds
    BinView v;
    CHECK(bin_open(z.p, z.len, "test", 2, v) == G16_OK && v.version == 2);
    for (int id = 1; id <= 3; id++) CHECK(v.sec[id].p == sec[id] && v.sec[id].size == sizes[id]);
    CHECK(v.sec[3].p != nullptr && v.sec[3].size == 0);   // present and empty
    CHECK(!v.sec[0].p && !v.sec[4].p && !v.sec[15].p);
    BinFault why;
    CHECK(bin_open(z.p, z.len, "tesu", 2, v, &why) == G16_E_FORMAT && why == BinFault::magic && g_err == "tesu: Invalid File format");
    CHECK(bin_open(z.p, z.len, "test", 1, v, &why) == G16_E_FORMAT && why == BinFault::version && g_err == "Version not supported");
    CHECK(bin_open(nullptr, 64, "test", 2, v, &why) == G16_E_FORMAT && why == BinFault::magic);
    CHECK(bin_open(z.p, 11, "test", 2, v, &why) == G16_E_FORMAT && why == BinFault::magic);
    CHECK(bin_open(z.p, 12 + 11, "test", 2, v, &why) == G16_E_FORMAT && why == BinFault::table);
    CHECK(bin_open(z.p, 12 + 12 + 4, "test", 2, v, &why) == G16_E_FORMAT && why == BinFault::section);
  }
  {   // the first occurrence of an id wins; an id of 16 or more is skipped
    std::vector<uint8_t> img(z.p, z.p + z.len);
    const uint32_t one = 1, big = 18;
    memcpy(&img[size_at[2] - 4], &one, 4);       // section 2 renamed to 1
    BinView v;
    CHECK(bin_open(img.data(), img.size(), "test", 2, v) == G16_OK);
    CHECK(v.sec[1].size == 5 && v.sec[1].p == img.data() + 24 && !v.sec[2].p);
    memcpy(&img[size_at[2] - 4], &big, 4);       // ... and to 18: not section 2
    BinView w;
    CHECK(bin_open(z.p, z.len, "test", 2, w) == G16_OK && w.sec[2].p);
    CHECK(bin_open(img.data(), img.size(), "test", 2, w) == G16_OK && !w.sec[2].p && w.sec[1].p && w.sec[3].p);   // a reused view is reset
    CHECK(bin_open(img.data(), 11, "test", 2, w) == G16_E_FORMAT && !w.sec[1].p && !w.sec[3].p);
  }

  // every prefix, plain and with every size field that is inside it overwritten
  const uint64_t evil[5] = {0, 1, 0 /* = len */, (uint64_t)1 << 40, ~(uint64_t)0};
  size_t parsed = 0, runs = 0;
  std::vector<uint8_t> img(total);
  for (size_t len = 0; len <= total; len++) {
    parsed += open_exact(z.p, len, 2);
    runs++;
    for (int f = 0; f < 3; f++) {
      for (int e = 0; e < 5; e++) {
        memcpy(img.data(), z.p, total);
        const uint64_t val = e == 2 ? (uint64_t)len : evil[e];
        memcpy(&img[size_at[f]], &val, 8);      // (beyond the prefix for a short len: the prefix is then unchanged)
        parsed += open_exact(img.data(), len, 2);
        runs++;
      }
    }
  }
  CHECK(open_exact(z.p, total, 2));
  CHECK(!open_exact(z.p, total - 1, 2));
  CHECK(parsed > 0 && parsed < runs);

  // Buf owns its image until give(): the sanitizer's leak checker and its double-free check are the asserts here
  {   // dropped after reserve, as an early return or an exception drops it
    Buf b;
    CHECK(b.reserve(100));
    b.u32(7);
  }
  {   // moved through a return value, then handed out: the caller frees it, exactly once
    Buf b = filled(64);
    CHECK(b.p != nullptr && b.len == 64 && b.cap == 64);
    Buf c(std::move(b));
    CHECK(b.p == nullptr && b.len == 0 && c.p != nullptr && c.len == 64);
    uint8_t* p = nullptr;
    size_t n = 0;
    c.give(&p, &n);
    CHECK(p != nullptr && n == 64 && p[0] == 0 && p[63] == 63);
    CHECK(c.p == nullptr && c.len == 0 && c.cap == 0);   // after give() the Buf holds nothing
    free(p);
  }
  {   // give() on a temporary, as write_wtns(w).give(...) does
    uint8_t* p = nullptr;
    size_t n = 0;
    filled(8).give(&p, &n);
    CHECK(p != nullptr && n == 8 && p[7] == 7);
    free(p);
  }

  {   // the field record
    uint8_t rec[36];
    CHECK(bin_put_field(rec, kFrP) == rec + 36);
    CHECK(rd32(rec) == 32 && memcmp(rec + 4, kFrP, 32) == 0);
    CHECK(bin_is_field(rec, 36, kFrP) && !bin_is_field(rec, 35, kFrP) && !bin_is_field(rec, 36, kFqP));
    rec[0] = 31;
    CHECK(!bin_is_field(rec, 36, kFrP));
    uint32_t s[8];
    memcpy(s, kFrP, 32);
    CHECK(!fr_below_modulus(s));
    s[0]--;
    CHECK(fr_below_modulus(s));
    s[0]++; s[7]++;
    CHECK(!fr_below_modulus(s));
  }
  printf("%zu runs, %zu parsed\n", runs, parsed);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
