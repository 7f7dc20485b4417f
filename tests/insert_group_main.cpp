// Stand-alone driver of bang_insert_group (csrc/bang_insert_group.cpp) for a sanitizer build: random rows, every output array heap-allocated to
// exactly the size the contract names, the CSR checked against a plain recount.  Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "bang_c.h"

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static int one(uint32_t n, uint32_t R, uint32_t n_old, uint64_t seed) {
  const uint32_t rs = R + 1, first = n_old;
  uint32_t* rows = (uint32_t*)malloc((size_t)n * rs * 4 + 4);
  uint32_t* targets = (uint32_t*)malloc((size_t)n * R * 4 + 4);
  uint32_t* offs = (uint32_t*)malloc(((size_t)n * R + 1) * 4);
  uint32_t* srcs = (uint32_t*)malloc((size_t)n * R * 4 + 4);
  std::map<uint32_t, std::vector<uint32_t>> want;
  size_t pairs = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t deg = rnd(seed) % (R + 1);
    std::vector<uint32_t> ids;
    while (ids.size() < deg) {
      const uint32_t x = rnd(seed) % n_old;
      if (std::find(ids.begin(), ids.end(), x) == ids.end()) ids.push_back(x);
    }
    rows[(size_t)i * rs] = deg;
    for (uint32_t j = 0; j < R; ++j) rows[(size_t)i * rs + 1 + j] = j < deg ? ids[j] : 0u;
    for (uint32_t x : ids) want[x].push_back(first + i);
    pairs += deg;
  }
  uint32_t nt = 0xDEADBEEFu;
  if (bang_insert_group(rows, n, rs, first, n_old, targets, offs, srcs, &nt) != BANG_OK) return 1;
  if (nt != want.size() || offs[0] != 0 || offs[nt] != pairs) return 2;
  uint32_t t = 0;
  for (const auto& kv : want) {
    if (targets[t] != kv.first || offs[t + 1] - offs[t] != kv.second.size()) return 3;
    for (size_t j = 0; j < kv.second.size(); ++j)
      if (srcs[offs[t] + j] != kv.second[j]) return 4;              // (ascending: the rows were visited in id order)
    ++t;
  }
  // refusals: an id outside the old index, a degree beyond the row, null arguments
  if (n != 0 && R != 0) {
    const uint32_t keep0 = rows[0], keep1 = rows[1];
    rows[0] = 1; rows[1] = n_old;
    if (bang_insert_group(rows, n, rs, first, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 5;
    rows[0] = R + 1; rows[1] = keep1;
    if (bang_insert_group(rows, n, rs, first, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 6;
    rows[0] = keep0;
  }
  if (bang_insert_group(nullptr, n, rs, first, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 7;
  if (bang_insert_group(rows, n, 1, first, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 8;
  free(rows); free(targets); free(offs); free(srcs);
  return 0;
}

int main() {
  int cases = 0;
  const uint32_t ns[] = {0, 1, 2, 17, 96, 1000}, Rs[] = {1, 2, 32, 64}, olds[] = {1, 5, 70, 100000};
  for (uint32_t n : ns)
    for (uint32_t R : Rs)
      for (uint32_t n_old : olds) {
        if (n_old < R) continue;                                    // (a row of R distinct old ids needs R old nodes)
        const int rc = one(n, R, n_old, 1000u * n + 10u * R + n_old);
        if (rc != 0) { printf("FAILED n=%u R=%u n_old=%u rc=%d\n", n, R, n_old, rc); return 1; }
        ++cases;
      }
  printf("ok %d\n", cases);
  return 0;
}
