// Stand-alone driver of bang_consolidate_group (csrc/bang_consolidate_group.cpp) for a sanitizer build: bitmaps of 0, 1, 31, 32, 33 and 130 nodes
// -- all set, none set, random --, the bitmap heap-allocated to exactly ceil(n / 32) words and the list to exactly n words, the slack bits of
// the last word set (they belong to no node).  Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bang_c.h"

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

// fill: 0 = none set, 1 = all set, 2 = random; slack: the bits at and behind n of the last word are set
static int one(uint32_t n, int fill, bool slack, uint64_t seed) {
  const uint32_t words = (n + 31u) / 32u;
  uint32_t* bitmap = (uint32_t*)malloc((size_t)words * 4 + (words == 0 ? 4 : 0));
  uint32_t* ids = (uint32_t*)malloc((size_t)n * 4 + (n == 0 ? 4 : 0));
  std::vector<uint32_t> want;
  for (uint32_t w = 0; w < words; ++w) bitmap[w] = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const bool on = fill == 1 || (fill == 2 && (rnd(seed) & 3u) == 0u);
    if (on) { bitmap[i >> 5] |= 1u << (i & 31u); want.push_back(i); }
  }
  if (slack && (n & 31u) != 0u) bitmap[words - 1] |= ~((1u << (n & 31u)) - 1u);
  uint32_t got = 0xDEADBEEFu;
  if (bang_consolidate_group(bitmap, n, ids, &got) != BANG_OK) return 1;
  if (got != want.size()) return 2;
  for (uint32_t i = 0; i < got; ++i)
    if (ids[i] != want[i]) return 3;
  if (bang_consolidate_group(nullptr, n, ids, &got) != BANG_ERR_ARG) return 4;
  if (bang_consolidate_group(bitmap, n, nullptr, &got) != BANG_ERR_ARG) return 5;
  if (bang_consolidate_group(bitmap, n, ids, nullptr) != BANG_ERR_ARG) return 6;
  free(bitmap); free(ids);
  return 0;
}

int main() {
  int cases = 0;
  const uint32_t ns[] = {0, 1, 31, 32, 33, 130};
  for (uint32_t n : ns)
    for (int fill = 0; fill < 3; ++fill)
      for (int slack = 0; slack < 2; ++slack) {
        const int rc = one(n, fill, slack != 0, 77u * n + 5u * (uint32_t)fill + (uint32_t)slack);
        if (rc != 0) { printf("FAILED n=%u fill=%d slack=%d rc=%d\n", n, fill, slack, rc); return 1; }
        ++cases;
      }
  printf("ok %d\n", cases);
  return 0;
}
