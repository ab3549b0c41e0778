// lenstream_check.cpp -- the host code of the length stream (scalce_amd/csrc/lenstream.hpp) and the sample rule of a
// variable-length run (scalce_varlen_sample, qualmap.cpp) on their own: a program for AddressSanitizer, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/lenstream_check.cpp \
//       scalce_amd/csrc/qualmap.cpp -o /tmp/lenstream_check && /tmp/lenstream_check
// Every buffer is a heap block of exactly the size the call may touch, so a byte too far is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../include/scalce_hip.h"
#include "../scalce_amd/csrc/lenstream.hpp"

using namespace scalce_host;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static void round_trip(int L, size_t n, unsigned seed) {
  const int width = len_entry_width(L);
  std::unique_ptr<uint16_t[]> pad(new uint16_t[n ? n : 1]);
  uint64_t sum = 0;
  srand(seed);
  for (size_t i = 0; i < n; i++) { pad[i] = (uint16_t)(i == 0 ? L : i == 1 ? 0 : rand() % (L + 1)); sum += pad[i]; }
  std::unique_ptr<uint8_t[]> head(new uint8_t[LEN_HEADER_BYTES]), body(new uint8_t[n * width ? n * width : 1]);
  len_header_write(head.get(), L);
  len_entries_write(pad.get(), n, width, body.get());
  int w = 0, l = 0;
  CHECK(len_header_read(head.get(), LEN_HEADER_BYTES, &w, &l) == nullptr && w == width && l == L);
  CHECK(len_entries_sum(body.get(), n, width, L) == sum);
  for (size_t cut = 0; cut < LEN_HEADER_BYTES; cut++) {  // a header that is cut short, from a block of just that size
    std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
    memcpy(part.get(), head.get(), cut);
    CHECK(len_header_read(part.get(), cut, &w, &l) != nullptr);
  }
  if (n && L < 65535 && width == 2) {  // an entry above L is a verdict
    body[1] = 0xFF;
    CHECK(len_entries_sum(body.get(), n, width, L) == ~0ull);
  }
  head[9] = 7;  // a width that does not fit
  CHECK(len_header_read(head.get(), LEN_HEADER_BYTES, &w, &l) != nullptr);
}

static void sample(void) {
  const int lens[] = {30, 0, 77, 12, 100, 5};
  std::string text;
  for (int i = 0; i < 6; i++) text += "@r" + std::to_string(i) + "\n" + std::string(lens[i], 'A') + "\n+\n" + std::string(lens[i], 'I') + "\n";
  for (size_t cut = 0; cut <= text.size(); cut++) {  // every prefix, from a block of exactly its size
    std::unique_ptr<uint8_t[]> t(new uint8_t[cut ? cut : 1]);
    memcpy(t.get(), text.data(), cut);
    int32_t stat[128] = {0}, L = -1;
    const int64_t got = scalce_varlen_sample(t.get(), cut, 100, 1, 0, 0, stat, &L);
    int want_n = 0, want_L = 0;
    size_t at = 0;
    for (int i = 0; i < 6; i++) {
      at += 3 + std::to_string(i).size() + 2 * (size_t)lens[i] + 4;
      if (at <= cut) { want_n++; if (lens[i] > want_L) want_L = lens[i]; }
    }
    CHECK(got == want_n && L == want_L);
    int64_t chars = 0;
    for (int c = 0; c < 128; c++) chars += stat[c];
    CHECK(chars == stat['I']);
  }
  int32_t L = 0;
  CHECK(scalce_varlen_sample((const uint8_t *)text.data(), text.size(), 2, 1, 0, 150, nullptr, &L) == 2 && L == 150);
  CHECK(scalce_varlen_sample((const uint8_t *)text.data(), text.size(), 3, 2, 1, 0, nullptr, &L) == 3 && L == 12);
  CHECK(scalce_varlen_sample(nullptr, 0, 3, 1, 0, 0, nullptr, &L) == 0 && L == 0);
}

int main() {
  for (int L : {1, 100, 255, 256, 300, 2498})
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000}) round_trip(L, n, (unsigned)(L * 31 + n));
  sample();
  puts("lenstream_check: ok");
  return 0;
}
