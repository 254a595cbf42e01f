// Host driver of the P-256 layer operator's one-item core (csrc/es256.h: p256_op_one) and of one whole verification
// (csrc/p256.cuh: es256_scalars, es256_slice_sum per lane, es256_tree_sum, p256_x_equals_r over tables built by
// p256_table_row) for tests/test_cpu_es256.py, which builds it with -DG16_HOST_MUL32 -- the 8 x 32-bit limb forms the
// device runs, which the library's host route (4 x 64) does not -- and with the address and undefined-behaviour sanitizers.
//   p256_test <op> <file a> <file b | -> <file out>
//   p256_test verify <keys: 64 bytes each> <digests: 32> <signatures: 64> <key indices: uint32 LE> <file out: a byte each>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static int spill(const char* path, const std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}

static int verify(char** argv) {
  using namespace g16;
  const std::vector<uint8_t> keys = slurp(argv[2]), digests = slurp(argv[3]), sigs = slurp(argv[4]), idx = slurp(argv[5]);
  const size_t n_keys = keys.size() / 64, n = digests.size() / 32;
  if (keys.size() != n_keys * 64 || digests.size() != n * 32 || sigs.size() != n * 64 || idx.size() != n * 4) return 2;
  // the tables of G and of every key, once: tbl[(j * 64 + w) * 15 + d - 1] = d * 16^w * points[j]
  std::vector<P256Affine> points(n_keys + 1);
  const uint32_t gx[8] = G16_P256_GX, gy[8] = G16_P256_GY;
  for (int k = 0; k < 8; k++) { points[0].x.v[k] = gx[k]; points[0].y.v[k] = gy[k]; }
  for (size_t j = 0; j < n_keys; j++) {
    points[j + 1] = p256_load_affine_be(keys.data() + j * 64);
    if (!p256_on_curve(points[j + 1])) return 2;
  }
  std::vector<P256Affine> tbl(points.size() * kP256TblPoint);
  for (size_t t = 0; t < points.size() * kP256Win; t++)
    p256_table_row(points[t / kP256Win], (uint32_t)(t % kP256Win), &tbl[t * kP256Row]);
  std::vector<uint8_t> ok(n, 0);
  for (size_t i = 0; i < n; i++) {
    uint32_t key = 0;
    for (int k = 0; k < 4; k++) key |= (uint32_t)idx[i * 4 + k] << (8 * k);
    if (key >= n_keys) return 2;
    P256Fn u1, u2;
    if (!es256_scalars(digests.data() + i * 32, sigs.data() + i * 64, u1, u2)) continue;
    P256Jac slot[kEs256Lanes];
    for (uint32_t l = 0; l < kEs256Lanes; l++) es256_slice_sum(slot[l], tbl.data(), key, u1.v, u2.v, l, kEs256Lanes);
    es256_tree_sum(slot);
    ok[i] = p256_x_equals_r(slot[0].X, slot[0].Z, pf_load_be<P256FnParams>(sigs.data() + i * 64)) ? 1 : 0;
  }
  return spill(argv[6], ok);
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "verify")) return verify(argv);
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
  return spill(argv[4], out);
}
