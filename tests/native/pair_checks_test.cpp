// Stand-alone test of csrc/pair_checks.h, meant to be built with -fsanitize=address,undefined together with
// csrc/blake2b.cpp (tests/test_cpu_pair_checks_native.py).  g16_pairing_op is a stub here that computes on the host
// through csrc/pairing.cuh -- the arithmetic the device kernels run --, counts its calls and can be told to fail.  The
// points are small multiples of the generators.  The Blake2b unit rides along to show that it builds without a HIP
// header: RFC 7693's "abc" vector, and the streaming form against the whole-message form over every kind of split.
#include <stdio.h>

#include <string>
#include <vector>

#include "blake2b.h"
#include "pair_checks.h"
#include "pairing.cuh"

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

// ---- the stub: count pairs of six standard-form words in, twelve standard-form words of e(P, Q) out
static int g_calls = 0, g_rc = G16_OK;
static uint32_t g_last_count = 0;
extern "C" int g16_pairing_op(int device, const uint8_t* in, uint32_t count, uint8_t* out) {
  (void)device;
  g_calls++;
  g_last_count = count;
  if (g_rc) return g_rc;
  PairingConsts pc;
  pairing_consts_init(pc);
  for (uint32_t i = 0; i < count; i++) {
    Fq w[6];
    for (int j = 0; j < 6; j++) { memcpy(w[j].v, in + (size_t)i * 192 + 32 * j, 32); w[j] = fp_to_mont(w[j]); }
    const Affine<FqOps> p{w[0], w[1]};
    const Affine<Fq2Ops> q{Fq2{w[2], w[3]}, Fq2{w[4], w[5]}};
    if (!g1_on_curve(p) || !g2_on_curve(q, pc)) return G16_E_ARG;
    const Fq12 f = final_exponentiation(miller_loop(p, q, pc), pc);
    const Fq2* c[6] = {&f.c0.c0, &f.c1.c0, &f.c0.c1, &f.c1.c1, &f.c0.c2, &f.c1.c2};
    for (int j = 0; j < 6; j++) {
      const Fq a = fp_from_mont(c[j]->a), b = fp_from_mont(c[j]->b);
      memcpy(out + (size_t)i * 384 + 64 * j, a.v, 32);
      memcpy(out + (size_t)i * 384 + 64 * j + 32, b.v, 32);
    }
  }
  return G16_OK;
}

// ---- points: [k] of a generator as a file image (Montgomery) and as standard-form words
template <class F, size_t N> struct Pt { uint8_t image[N], words[N]; };
template <class F, size_t N> static Pt<F, N> mul(const Affine<F>& g, uint32_t k) {
  const uint32_t kk[8] = {k, 0, 0, 0, 0, 0, 0, 0};
  XYZZ<F> acc;
  xyzz_mul_scalar(acc, g, kk);
  Affine<F> r;
  xyzz_to_affine(r, acc);
  Pt<F, N> o;
  memcpy(o.image, &r, N);
  for (size_t c = 0; c < N / 32; c++) {
    Fq x;
    memcpy(x.v, o.image + 32 * c, 32);
    x = fp_from_mont(x);
    memcpy(o.words + 32 * c, x.v, 32);
  }
  return o;
}
using P1 = Pt<FqOps, 64>;
using P2 = Pt<Fq2Ops, 128>;

static std::string hex(const uint8_t* p, size_t n) {
  std::string s;
  char b[3];
  for (size_t i = 0; i < n; i++) { snprintf(b, sizeof(b), "%02x", p[i]); s += b; }
  return s;
}

int main() {
  G1Affine g1;   // (1, 2)
  g1.x = fp_one<FqParams>();
  g1.y = fp_add(g1.x, g1.x);
  const G2Affine g2{Fq2{Fq{G16_G2X0}, Fq{G16_G2X1}}, Fq2{Fq{G16_G2Y0}, Fq{G16_G2Y1}}};
  auto m1 = [&](uint32_t k) { return mul<FqOps, 64>(g1, k); };
  auto m2 = [&](uint32_t k) { return mul<Fq2Ops, 128>(g2, k); };
  const P2 G2one = m2(1);
  static const uint32_t ab[3][2] = {{3, 5}, {7, 11}, {2, 9}};
  static const char* const why[3] = {"check one", "check two", "check three"};

  {   // e([a] G1, [b] G2) = e([ab] G1, G2), three times: all hold, in ONE call of six pairs
    PairChecks c;
    for (int i = 0; i < 3; i++) {
      const P1 a = m1(ab[i][0]), prod = m1(ab[i][0] * ab[i][1]);
      const P2 b = m2(ab[i][1]);
      c.same_ratio(a.image, prod.image, G2one.image, b.image, why[i]);   // (the batch copies: the points die here)
    }
    CHECK(c.pairs() == 6 && c.words().size() == 6 * 192);
    CHECK(c.first_failure() == why[0]);   // not run yet: nothing holds
    g_calls = 0;
    CHECK(c.run(0) == G16_OK && g_calls == 1 && g_last_count == 6);
    CHECK(c.first_failure() == nullptr);
  }
  {   // checks two and three broken: the verdict is check two's
    PairChecks c;
    for (int i = 0; i < 3; i++) {
      const P1 a = m1(ab[i][0]), prod = m1(ab[i][0] * ab[i][1] + (i ? 1 : 0));
      const P2 b = m2(ab[i][1]);
      c.same_ratio(a.image, prod.image, G2one.image, b.image, why[i]);
    }
    CHECK(c.run(0) == G16_OK);
    CHECK(c.first_failure() == why[1]);
  }
  {   // no checks: no call, no failure
    PairChecks c;
    g_calls = 0;
    CHECK(c.pairs() == 0 && c.run(0) == G16_OK && g_calls == 0 && c.first_failure() == nullptr);
  }
  {   // the same points as images and as standard-form words, on either side: the same 192-byte pairs
    const P1 a = m1(3), prod = m1(15);
    const P2 b = m2(5);
    PairChecks img, std_g1, std_g2, std_all;
    img.same_ratio(a.image, prod.image, G2one.image, b.image, "x");
    std_g1.equal(pair_words(a.words), pair_image(b.image), pair_words(prod.words), pair_image(G2one.image), "x");
    std_g2.equal(pair_image(a.image), pair_words(b.words), pair_image(prod.image), pair_words(G2one.words), "x");
    std_all.equal(pair_words(a.words), pair_words(b.words), pair_words(prod.words), pair_words(G2one.words), "x");
    CHECK(img.pairs() == 2 && img.words().size() == 2 * 192);
    CHECK(memcmp(img.words().data(), a.words, 64) == 0 && memcmp(img.words().data() + 64, b.words, 128) == 0);
    CHECK(memcmp(img.words().data() + 192, prod.words, 64) == 0 && memcmp(img.words().data() + 256, G2one.words, 128) == 0);
    CHECK(img.words() == std_g1.words() && img.words() == std_g2.words() && img.words() == std_all.words());
    CHECK(std_g1.run(0) == G16_OK && std_g1.first_failure() == nullptr);
  }
  {   // an error of the device call comes back unchanged, and the checks do not count as held
    PairChecks c;
    const P1 a = m1(3), prod = m1(15);
    const P2 b = m2(5);
    c.same_ratio(a.image, prod.image, G2one.image, b.image, why[0]);
    g_rc = G16_E_HIP;
    CHECK(c.run(0) == G16_E_HIP);
    g_rc = G16_E_NOGPU;
    CHECK(c.run(0) == G16_E_NOGPU);
    g_rc = G16_OK;
    CHECK(c.run(0) == G16_OK && c.first_failure() == nullptr);
  }

  {   // Blake2b-512: RFC 7693 appendix A, whole and split
    static const char* const abc =
        "ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d17d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923";
    uint8_t h[64], h2[64];
    blake2b512((const uint8_t*)"abc", 3, h);
    CHECK(hex(h, 64) == abc);
    Blake2b512 s;
    s.update((const uint8_t*)"a", 1);
    s.update(nullptr, 0);
    s.update((const uint8_t*)"bc", 2);
    s.final(h2);
    CHECK(memcmp(h, h2, 64) == 0);
    // every length around the block size, cut at every place where the hold-back rule can go wrong
    std::vector<uint8_t> msg(400);
    for (size_t i = 0; i < msg.size(); i++) msg[i] = (uint8_t)(31 * i + 7);
    static const size_t lens[] = {0, 1, 127, 128, 129, 255, 256, 257, 384, 400};
    static const size_t cuts[] = {0, 1, 64, 127, 128, 129, 200, 256, 383};
    for (const size_t len : lens) {
      blake2b512(msg.data(), len, h);
      for (const size_t c1 : cuts)
        for (const size_t c2 : cuts) {
          if (c1 > c2 || c2 > len) continue;
          Blake2b512 t;
          t.update(msg.data(), c1);
          t.update(msg.data() + c1, c2 - c1);
          t.update(msg.data() + c2, len - c2);
          t.final(h2);
          CHECK(memcmp(h, h2, 64) == 0);
        }
    }
  }
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
