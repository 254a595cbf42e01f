// Host build of fr29.cuh as a vector printer: tests/test_cpu_ntt_lazy.py feeds it the inputs of its Python twin
// (tests/ntt_lazy_ref.py) and compares the integers, not only the residues.
//   g++ -O2 -std=c++17 -DG16_F29_CHECK -I nzcp-circom_amd/csrc tests/native/fr29_vectors.cpp -o fr29_vectors
// stdin:  one case per line, "<op> <hex a> <hex b>" (values as plain hexadecimal integers; b = 0 where unused)
//   op: from_fr (a = canonical Montgomery(2^256) image), mul, weak, sub2, sub3, sub5, to_fr
// stdout: the result's words, least significant first, as hexadecimal: nine 29-bit limbs (the top one holds the
//         rest), or the eight 32-bit words of to_fr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fr29.cuh"

using namespace g16;

// hexadecimal integer -> 320 bits, little-endian words
static void parse_hex(const char* s, uint32_t w[10]) {
  memset(w, 0, 10 * sizeof(uint32_t));
  const size_t n = strlen(s);
  for (size_t i = 0; i < n && i < 80; i++) {
    const char c = s[n - 1 - i];
    const uint32_t d = (c >= '0' && c <= '9') ? (uint32_t)(c - '0') : (uint32_t)((c | 0x20) - 'a' + 10);
    w[i >> 3] |= (d & 15u) << (4 * (i & 7));
  }
}
static F29 to_f29(const uint32_t w[10]) {
  F29 r;
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, k = bit >> 5, o = bit & 31;
    const uint64_t x = (uint64_t)w[k] | ((uint64_t)w[k + 1] << 32);
    r.l[i] = (uint32_t)(x >> o) & (i < 8 ? kM29 : 0xffffffffu);
  }
  r.pad_ = 0;
  return r;
}
static void print_f29(const F29& r) {
  for (int i = 0; i < 9; i++) printf("%x%c", r.l[i], i < 8 ? ' ' : '\n');
}

int main() {
  char op[16];
  static char sa[128], sb[128];
  while (scanf("%15s %127s %127s", op, sa, sb) == 3) {
    uint32_t wa[10], wb[10];
    parse_hex(sa, wa);
    parse_hex(sb, wb);
    const F29 a = to_f29(wa), b = to_f29(wb);
    if (!strcmp(op, "from_fr")) {
      Fr v;
      for (int i = 0; i < 8; i++) v.v[i] = wa[i];
      print_f29(fr29_from_fr(v));
    } else if (!strcmp(op, "mul")) {
      print_f29(fr29_mul(a, b));
    } else if (!strcmp(op, "weak")) {
      print_f29(fr29_weak_reduce(a));
    } else if (!strcmp(op, "sub2")) {
      print_f29(fr29_sub<2>(a, b));
    } else if (!strcmp(op, "sub3")) {
      print_f29(fr29_sub<3>(a, b));
    } else if (!strcmp(op, "sub5")) {
      print_f29(fr29_sub<5>(a, b));
    } else if (!strcmp(op, "to_fr")) {
      const Fr v = fr29_to_fr(a);
      for (int i = 0; i < 8; i++) printf("%x%c", v.v[i], i < 7 ? ' ' : '\n');
    } else {
      fprintf(stderr, "unknown op %s\n", op);
      return 2;
    }
  }
  return 0;
}
