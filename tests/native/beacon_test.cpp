// Stand-alone test of csrc/beacon.h, meant to be built with -fsanitize=address,undefined
// (tests/test_cpu_beacon_native.py).  The params walker runs on every prefix of a valid params block held in a heap
// buffer of EXACTLY that length, so any read past what it was given is a heap overflow the sanitizer reports, and at
// each length with every length byte overwritten by hostile values.  The delay function runs at e = 10 against constants
// computed by the Python twin (tests/beacon_ref.py chain()).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "beacon.h"

using namespace g16;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

// the walker on a heap copy of exactly `len` bytes; what it returns must lie inside the copy
static bool walk_exact(const uint8_t* img, size_t len, BeaconStated& st) {
  uint8_t* buf = (uint8_t*)malloc(len);
  CHECK(buf != nullptr);
  if (len) memcpy(buf, img, len);
  const bool ok = beacon_params_walk(buf, len, st);
  if (ok) {
    CHECK(st.hash >= buf + 4 && st.hash_len >= 1 && st.hash_len <= 255 && st.hash + st.hash_len <= buf + len);
    CHECK(st.exp >= kBeaconExpMin && st.exp <= kBeaconExpMax);
    unsigned sum = 0;
    for (size_t i = 0; i < st.hash_len; i++) sum += st.hash[i];   // every byte of the hash is readable
    CHECK(sum <= 255 * st.hash_len);
    st.hash = img + (st.hash - buf);   // (the copy is freed: point into the caller's image)
  }
  free(buf);
  return ok;
}

static std::string hex(const uint32_t w[8]) {
  char s[65];
  for (int i = 0; i < 8; i++) snprintf(s + 8 * i, 9, "%08x", w[i]);
  return s;
}

int main() {
  uint8_t beacon[255];
  for (int i = 0; i < 255; i++) beacon[i] = (uint8_t)(37 * i + 11);

  // ---- the builder, and the walker on what it built
  const std::string name = std::string("\x01\x04", 2) + "name";
  const std::string blocks[3] = {beacon_params(beacon, 32, 10), name + beacon_params(beacon, 32, 10), name + beacon_params(beacon, 255, 63)};
  CHECK(blocks[0].size() == 4 + 32 && blocks[0][0] == 2 && blocks[0][1] == 10 && blocks[0][2] == 3 && blocks[0][3] == 32);
  CHECK(memcmp(blocks[0].data() + 4, beacon, 32) == 0);
  for (const std::string& b : blocks) {
    BeaconStated st;
    const uint8_t* p = (const uint8_t*)b.data();
    CHECK(walk_exact(p, b.size(), st));
    CHECK(st.exp == (uint8_t)b[b.size() - st.hash_len - 3] && st.hash == p + b.size() - st.hash_len);
    CHECK(memcmp(st.hash, beacon, st.hash_len) == 0);
  }

  // ---- every prefix, plain and with every byte that can be a length (or an id) overwritten
  const uint8_t evil[6] = {0, 1, 2, 3, 4, 255};
  size_t runs = 0, stated = 0;
  for (const std::string& b : blocks) {
    const size_t total = b.size();
    std::vector<uint8_t> img(total);
    for (size_t len = 0; len <= total; len++) {
      BeaconStated st;
      const bool whole = walk_exact((const uint8_t*)b.data(), len, st);
      CHECK(whole == (len == total));   // a cut block never states a beacon
      runs++;
      stated += whole;
      const size_t heads = b[0] == 1 ? 10 : 4;   // the ids, the lengths and e
      for (size_t at = 0; at < heads && at < total; at++)
        for (uint8_t e : evil) {
          memcpy(img.data(), b.data(), total);
          img[at] = e;
          stated += walk_exact(img.data(), len, st);
          runs++;
        }
    }
  }
  CHECK(stated > 0 && stated < runs);

  {   // what does not state a beacon
    BeaconStated st;
    const uint8_t unsorted[] = {3, 1, 9, 2, 10}, twice[] = {2, 10, 2, 10, 3, 1, 9}, e9[] = {2, 9, 3, 1, 9}, e64[] = {2, 64, 3, 1, 9};
    const uint8_t empty[] = {2, 10, 3, 0}, unknown[] = {2, 10, 3, 1, 9, 4, 0}, only2[] = {2, 10}, only3[] = {3, 1, 9}, id0[] = {0, 0, 2, 10, 3, 1, 9};
    const uint8_t good[] = {2, 10, 3, 1, 9};
    CHECK(!walk_exact(unsorted, sizeof(unsorted), st) && !walk_exact(twice, sizeof(twice), st));
    CHECK(!walk_exact(e9, sizeof(e9), st) && !walk_exact(e64, sizeof(e64), st));
    CHECK(!walk_exact(empty, sizeof(empty), st) && !walk_exact(unknown, sizeof(unknown), st));
    CHECK(!walk_exact(only2, sizeof(only2), st) && !walk_exact(only3, sizeof(only3), st) && !walk_exact(id0, sizeof(id0), st));
    CHECK(!walk_exact(good, 0, st) && !beacon_params_walk(nullptr, 0, st));
    CHECK(walk_exact(good, sizeof(good), st) && st.exp == 10 && st.hash_len == 1 && st.hash[0] == 9);
  }

  // ---- SHA-256 and the chain
  {
    uint32_t h[8];
    sha256_words((const uint8_t*)"abc", 3, h);
    CHECK(hex(h) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
    sha256_words(nullptr, 0, h);
    CHECK(hex(h) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
    sha256_words((const uint8_t*)"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", 56, h);   // 55 / 56: one block / two
    CHECK(hex(h) == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");
    // the chain at e = 10 for beacons of 32, 1 and 255 bytes: tests/beacon_ref.py chain()
    beacon_chain(beacon, 32, 10, h);
    CHECK(hex(h) == "4f7c00f7d79b9387c6137abe6ea430ac2bfbc654c08856807c9f3ba77ff71a0c");
    const uint8_t one = 1;
    beacon_chain(&one, 1, 10, h);
    CHECK(hex(h) == "cc5deae2ed8f472226223e3cccbc4e56044541b27764720e502499e81592b99d");
    beacon_chain(beacon, 255, 10, h);
    CHECK(hex(h) == "9be189c455ccc1ffbbddae7a60a5a084ca9d8f9c851a66e4ee6beef887aa9446");
  }
  printf("%zu walks, %zu stated a beacon\n", runs, stated);
  if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
  printf("ALL OK\n");
  return 0;
}
