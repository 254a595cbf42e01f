// Host driver of the pass front end (csrc/pass_verify.h: the one-pass cores of nzcp_pass.cuh) for tests/test_cpu_pass.py,
// which builds it with the address and undefined-behaviour sanitizers.  Every pass's text, its decoded bytes and the skip
// stack are heap blocks of their exact sizes, so that a read or a write one byte outside any of them is reported.
//   pass_test <corpus> <file out>
// corpus: u32 n_keys, per key (u32 length, iss bytes, u32 length, kid bytes), u32 count, count + 1 u64 offsets, the text;
// out: count records (g16_pass_result), then count x 64 signature bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pass_verify.h"

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

struct Reader {
  const std::vector<uint8_t>& v;
  size_t p = 0;
  const uint8_t* take(size_t n) {
    if (n > v.size() - p) { fprintf(stderr, "corpus: truncated\n"); exit(2); }
    p += n;
    return v.data() + p - n;
  }
  uint32_t u32() { uint32_t x; memcpy(&x, take(4), 4); return x; }
  uint64_t u64() { uint64_t x; memcpy(&x, take(8), 8); return x; }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<uint8_t> file = slurp(argv[1]);
  Reader rd{file};
  const uint32_t n_keys = rd.u32();
  if (n_keys > 16) return 2;
  std::vector<g16::PassKeyName> keys(n_keys);
  for (auto& k : keys) {
    memset(&k, 0, sizeof k);
    k.iss_len = rd.u32();
    if (k.iss_len > g16::kPassNameMax) return 2;
    memcpy(k.iss, rd.take(k.iss_len), k.iss_len);
    k.kid_len = rd.u32();
    if (k.kid_len > g16::kPassNameMax) return 2;
    memcpy(k.kid, rd.take(k.kid_len), k.kid_len);
  }
  const uint32_t count = rd.u32();
  std::vector<uint64_t> offsets(count + 1);
  for (auto& o : offsets) o = rd.u64();
  const uint8_t* text = rd.take(file.size() - rd.p);
  const size_t text_len = file.size() - (size_t)(text - file.data());
  std::vector<g16_pass_result> records(count);
  std::vector<uint8_t> sigs((size_t)count * 64);
  for (uint32_t i = 0; i < count; i++) {
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] > text_len) return 2;
    const size_t n = (size_t)(offsets[i + 1] - offsets[i]);
    uint8_t* item = (uint8_t*)malloc(n);
    if (n) memcpy(item, text + offsets[i], n);
    // the decoded bytes at their exact size: the frame is taken here as pass_uri_one takes it
    uint32_t start = 0, n_chars = 0;
    const size_t bytes = g16::pass_uri_frame(item, n, &start, &n_chars) == G16_PASS_OK ? g16::pass_b32_bytes(n_chars) : 0;
    uint8_t* dec = (uint8_t*)malloc(bytes);
    uint32_t* stack = (uint32_t*)malloc(g16::kPassCborDepth * sizeof(uint32_t));
    g16::pass_uri_one(item, n, keys.data(), n_keys, dec, stack, &records[i], &sigs[(size_t)i * 64]);
    free(stack);
    free(dec);
    free(item);
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(records.data(), sizeof(g16_pass_result), records.size(), f);
  fwrite(sigs.data(), 1, sigs.size(), f);
  fclose(f);
  return 0;
}
