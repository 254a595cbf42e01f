// Stand-alone test of the host side of g16_wtns_calc, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_wtns_calc_native.py) from csrc/witness_program.cpp: the recorder's file image, the loader's complete
// validation and the host route (device = -1).  There is no device here: the device entry points are stubs that fail.
// A program recorded here is evaluated against values worked out by hand; then the loader is fed every prefix of the
// image and the image with every 32-bit word of it overwritten by hostile values, from heap buffers of exactly the
// image's length.  Whatever the loader ACCEPTS is evaluated: an accepted program must be safe to run.
#include <stdio.h>

#include "witness_program.h"

static thread_local std::string g_err;
namespace g16 {
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }
int wcalc_device_create(int, const WitnessProgram&, uint32_t, WcalcDevice**) { set_error("no device in this program"); return G16_E_NOGPU; }
void wcalc_device_destroy(WcalcDevice*) {}
int wcalc_device_id(const WcalcDevice*) { return -1; }
int wcalc_device_run(WcalcDevice*, const uint8_t*, size_t, uint8_t*, uint32_t*, float*) { return G16_E_NOGPU; }
int wcalc_device_run_into(WcalcDevice*, const uint8_t*, Fr*, hipStream_t, uint32_t*) { return G16_E_NOGPU; }
}  // namespace g16
extern "C" const char* g16_last_error(void) { return g_err.c_str(); }
extern "C" void g16_free(void* p) { free(p); }
using namespace g16;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

struct Exact {   // a heap copy of exactly `len` bytes
  uint8_t* p;
  size_t len;
  Exact(const uint8_t* src, size_t n) : p((uint8_t*)malloc(n ? n : 1)), len(n) { if (n) memcpy(p, src, n); }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
};

static uint64_t low64(const uint8_t* words, uint32_t wire) {
  uint64_t v;
  memcpy(&v, words + (size_t)wire * 32, 8);
  for (int i = 8; i < 32; i++)
    if (words[(size_t)wire * 32 + i]) return ~0ull;
  return v;
}

// wires: 1, 2 = inputs x, y; 3 = (x + 2)(y - 3) + 5; 4..11 = the 8 bits of wire 3 (check 0); 12 = 1 / (x - y) or 0;
// 13 = [x = y]; check 1: x - y - 1 = 0
static Buf record() {
  WpRecorder rec;
  rec.input(1);
  rec.input(2);
  rec.name_inputs("x", 1);
  rec.quad(3, {{1, 1}, {0, 2}}, {{2, 1}, {0, -3}}, {{0, 5}});
  const uint32_t bits[8] = {4, 5, 6, 7, 8, 9, 10, 11};
  rec.bits(bits, 8, {{3, 1}}, "does not fit a byte");
  rec.inv0(12, {{1, 1}, {2, -1}});
  rec.isz(13, {{1, 1}, {2, -1}});
  rec.check({{1, 1}, {2, -1}, {0, -1}}, "x is not y + 1");
  rec.outputs = {3, 13};
  return rec.finish(14, 0);
}

static void put_word(uint8_t* w, uint64_t v) { memset(w, 0, 32); memcpy(w, &v, 8); }

int main() {
  const Buf img = record();
  CHECK(img.p != nullptr);
  // ---- the recorded program, by hand
  {
    Exact e(img.p, img.len);
    g16_wtns_calculator* h = nullptr;
    CHECK(g16_wtns_calc_create(e.p, e.len, -1, &h) == G16_OK);
    uint32_t info[6];
    CHECK(g16_wtns_calc_info(h, info) == G16_OK && info[0] == 14 && info[2] == 2 && info[3] == 3 && info[4] == 2);
    uint8_t in[3 * 64];
    put_word(in, 5); put_word(in + 32, 4);            // (7)(1) + 5 = 12; x = y + 1
    put_word(in + 64, 9); put_word(in + 96, 9);       // (11)(6) + 5 = 71; x = y: check 1
    put_word(in + 128, 30); put_word(in + 160, 29);   // (32)(26) + 5 = 837: check 0 first
    std::vector<uint8_t> out((size_t)3 * 14 * 32);
    uint32_t st[3];
    CHECK(g16_wtns_calc(h, in, 2, 3, out.data(), st) == G16_OK);
    CHECK(st[0] == 0xffffffffu && st[1] == 1 && st[2] == 0);
    CHECK(low64(out.data(), 0) == 1 && low64(out.data(), 3) == 12 && low64(out.data(), 12) == 1 && low64(out.data(), 13) == 0);
    CHECK(low64(out.data(), 6) == 1 && low64(out.data(), 7) == 1 && low64(out.data(), 4) == 0);
    const uint8_t* w1 = out.data() + 14 * 32;
    CHECK(low64(w1, 3) == 71 && low64(w1, 12) == 0 && low64(w1, 13) == 1);
    const uint8_t* w2 = out.data() + 2 * 14 * 32;
    CHECK(low64(w2, 3) == 837);
    for (uint32_t b = 4; b < 12; b++) CHECK(low64(w2, b) == 0);
    CHECK(std::string(g16_wtns_calc_check_text(h, 1)) == "x is not y + 1" && g16_wtns_calc_check_text(h, 2) == nullptr);
    uint8_t* wt = nullptr;
    size_t wl = 0;
    uint32_t s1 = 0;
    CHECK(g16_wtns_calc_wtns(h, in, 2, &s1, &wt, &wl) == G16_OK && s1 == 0xffffffffu && wl == 12 + 12 + 40 + 12 + 14 * 32);
    free(wt);
    CHECK(g16_wtns_calc_wtns(h, in + 64, 2, &s1, &wt, &wl) == G16_OK && s1 == 1 && wt == nullptr);
    memset(in + 32, 0xff, 32);                        // not below r
    CHECK(g16_wtns_calc(h, in, 2, 1, nullptr, st) == G16_E_FORMAT && g_err.find("input x[0] is not reduced") != std::string::npos);
    g16_wtns_calc_destroy(h);
  }
  // ---- every prefix is refused
  for (size_t cut = 0; cut < img.len; cut++) {
    Exact e(img.p, cut);
    g16_wtns_calculator* h = nullptr;
    CHECK(g16_wtns_calc_create(e.p, e.len, -1, &h) == G16_E_FORMAT && h == nullptr);
  }
  // ---- every 32-bit word overwritten by hostile values: refused, or safe to run
  size_t accepted = 0, refused = 0;
  static const uint32_t hostile[] = {0u, 2u, 14u, 254u, 0x80000000u, 0xffffffffu};
  for (size_t off = 0; off + 4 <= img.len; off += 4)
    for (uint32_t v : hostile) {
      Exact e(img.p, img.len);
      memcpy(e.p + off, &v, 4);
      g16_wtns_calculator* h = nullptr;
      const int rc = g16_wtns_calc_create(e.p, e.len, -1, &h);
      if (rc) { CHECK(rc == G16_E_FORMAT && h == nullptr && !g_err.empty()); refused++; continue; }
      accepted++;
      uint32_t info[6];
      g16_wtns_calc_info(h, info);
      std::vector<uint8_t> in((size_t)info[2] * 32 + 32, 0), out((size_t)info[0] * 32);
      for (uint32_t j = 0; j < info[2]; j++) in[(size_t)j * 32] = (uint8_t)(7 + j);
      uint32_t st = 0;
      CHECK(g16_wtns_calc(h, in.data(), info[2], 1, out.data(), &st) == G16_OK);
      g16_wtns_calc_destroy(h);
    }
  printf("mutations: %zu accepted and evaluated, %zu refused\n", accepted, refused);
  CHECK(refused > accepted);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
