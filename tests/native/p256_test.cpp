// Host driver of the P-256 layer operator's one-item core (csrc/es256.h: p256_op_one) for tests/test_cpu_es256.py, which
// builds it with -DG16_HOST_MUL32 -- the 8 x 32-bit limb forms the device runs, which the library's host route (4 x 64)
// does not -- and with the address and undefined-behaviour sanitizers.
//   p256_test <op> <file a> <file b | -> <file out>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "es256.h"

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int op = atoi(argv[1]);
  size_t sa, sb, so;
  g16::p256_op_strides(op, &sa, &sb, &so);
  const std::vector<uint8_t> a = slurp(argv[2]);
  std::vector<uint8_t> b;
  if (sb) b = slurp(argv[3]);
  const size_t n = a.size() / sa;
  if (a.size() != n * sa || b.size() != n * sb) return 2;
  std::vector<uint8_t> out(n * so);
  for (size_t i = 0; i < n; i++) g16::p256_op_one(op, a.data() + i * sa, b.data() + i * sb, out.data() + i * so);
  FILE* f = fopen(argv[4], "wb");
  if (!f) { perror(argv[4]); return 2; }
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}
