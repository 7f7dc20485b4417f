// Stand-alone driver of bang_reuse_assign and bang_insert_group_ids (csrc/bang_reuse_group.cpp) for a sanitizer build: random rows whose sources are
// scattered slot ids followed by appended ids, every array heap-allocated to exactly the size the contract names, the CSR checked against a plain
// recount, and the refusals.  Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "bang_c.h"

static uint32_t rnd(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static int one(uint32_t n, uint32_t R, uint32_t n_old, uint32_t n_free, uint64_t seed) {
  const uint32_t rs = R + 1;
  // free slots: n_free distinct ids below n_old, ascending; the rows never list them
  std::vector<uint32_t> pool(n_old);
  for (uint32_t i = 0; i < n_old; ++i) pool[i] = i;
  for (uint32_t i = 0; i < n_free; ++i) std::swap(pool[i], pool[i + rnd(seed) % (n_old - i)]);
  uint32_t* free_ids = (uint32_t*)malloc((size_t)n_free * 4 + 4);
  for (uint32_t i = 0; i < n_free; ++i) free_ids[i] = pool[i];
  std::sort(free_ids, free_ids + n_free);
  std::vector<uint32_t> live(pool.begin() + n_free, pool.end());
  if (live.size() < R) { free(free_ids); return 0; }
  uint32_t* ids = (uint32_t*)malloc((size_t)n * 4 + 4);
  uint32_t appended = 0xDEADBEEFu;
  if (bang_reuse_assign(free_ids, n_free, n, n_old, ids, &appended) != BANG_OK) return 20;
  const uint32_t f = std::min(n, n_free);
  if (appended != n - f) return 21;
  for (uint32_t i = 0; i < n; ++i)
    if (ids[i] != (i < f ? free_ids[i] : n_old + (i - f))) return 22;
  uint32_t* rows = (uint32_t*)malloc((size_t)n * rs * 4 + 4);
  uint32_t* targets = (uint32_t*)malloc((size_t)n * R * 4 + 4);
  uint32_t* offs = (uint32_t*)malloc(((size_t)n * R + 1) * 4);
  uint32_t* srcs = (uint32_t*)malloc((size_t)n * R * 4 + 4);
  std::map<uint32_t, std::vector<uint32_t>> want;
  size_t pairs = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t deg = rnd(seed) % (R + 1);
    std::vector<uint32_t> row;
    while (row.size() < deg) {
      const uint32_t x = live[rnd(seed) % live.size()];
      if (std::find(row.begin(), row.end(), x) == row.end()) row.push_back(x);
    }
    rows[(size_t)i * rs] = deg;
    for (uint32_t j = 0; j < R; ++j) rows[(size_t)i * rs + 1 + j] = j < deg ? row[j] : 0u;
    for (uint32_t x : row) want[x].push_back(ids[i]);
    pairs += deg;
  }
  uint32_t nt = 0xDEADBEEFu;
  if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_OK) return 1;
  if (nt != want.size() || offs[0] != 0 || offs[nt] != pairs) return 2;
  uint32_t t = 0;
  for (const auto& kv : want) {
    if (targets[t] != kv.first || offs[t + 1] - offs[t] != kv.second.size()) return 3;
    for (size_t j = 0; j < kv.second.size(); ++j)
      if (srcs[offs[t] + j] != kv.second[j]) return 4;              // (ascending: the rows were visited in id order)
    ++t;
  }
  // contiguous ids: the CSR of bang_insert_group
  if (n != 0) {
    uint32_t* t2 = (uint32_t*)malloc((size_t)n * R * 4 + 4);
    uint32_t* o2 = (uint32_t*)malloc(((size_t)n * R + 1) * 4);
    uint32_t* s2 = (uint32_t*)malloc((size_t)n * R * 4 + 4);
    uint32_t* seq = (uint32_t*)malloc((size_t)n * 4);
    for (uint32_t i = 0; i < n; ++i) seq[i] = n_old + i;
    uint32_t na = 0, nb = 0;
    if (bang_insert_group_ids(rows, n, rs, seq, n_old, targets, offs, srcs, &na) != BANG_OK) return 9;
    if (bang_insert_group(rows, n, rs, n_old, n_old, t2, o2, s2, &nb) != BANG_OK) return 10;
    if (na != nb || !std::equal(targets, targets + na, t2) || !std::equal(offs, offs + na + 1, o2) || !std::equal(srcs, srcs + o2[nb], s2)) return 11;
    free(t2); free(o2); free(s2); free(seq);
  }
  // refusals: unsorted ids, a row that lists an id of the batch, an id outside the old index, a degree beyond the row, null arguments
  if (n >= 2) {
    std::swap(ids[0], ids[1]);
    if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 12;
    std::swap(ids[0], ids[1]);
    const uint32_t keep = ids[1];
    ids[1] = ids[0];
    if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 13;
    ids[1] = keep;
  }
  if (n != 0 && R != 0) {
    const uint32_t keep0 = rows[0], keep1 = rows[1];
    if (f != 0) {
      rows[0] = 1; rows[1] = ids[f - 1];                              // a re-used slot of the batch
      if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 14;
    }
    rows[0] = 1; rows[1] = n_old;
    if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 5;
    rows[0] = R + 1; rows[1] = keep1;
    if (bang_insert_group_ids(rows, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 6;
    rows[0] = keep0;
  }
  if (bang_insert_group_ids(nullptr, n, rs, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 7;
  if (bang_insert_group_ids(rows, n, rs, nullptr, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 15;
  if (bang_insert_group_ids(rows, n, 1, ids, n_old, targets, offs, srcs, &nt) != BANG_ERR_ARG) return 8;
  if (n_free >= 2 && n >= 2) {
    std::swap(free_ids[0], free_ids[1]);
    if (bang_reuse_assign(free_ids, n_free, n, n_old, ids, &appended) != BANG_ERR_ARG) return 23;
    std::swap(free_ids[0], free_ids[1]);
  }
  if (n_free >= 1 && n >= 1) {
    const uint32_t keep = free_ids[f - 1];
    free_ids[f - 1] = n_old;
    if (bang_reuse_assign(free_ids, n_free, n, n_old, ids, &appended) != BANG_ERR_ARG) return 24;
    free_ids[f - 1] = keep;
  }
  if (bang_reuse_assign(free_ids, n_free, n, n_old, ids, nullptr) != BANG_ERR_ARG) return 25;
  free(free_ids); free(ids); free(rows); free(targets); free(offs); free(srcs);
  return 0;
}

int main() {
  int cases = 0;
  const uint32_t ns[] = {0, 1, 2, 17, 96, 1000}, Rs[] = {1, 2, 32, 64}, olds[] = {70, 100000}, frees[] = {0, 1, 5, 17, 2000};
  for (uint32_t n : ns)
    for (uint32_t R : Rs)
      for (uint32_t n_old : olds)
        for (uint32_t n_free : frees) {
          if (n_free + R > n_old) continue;                         // (a row of R distinct live ids needs R live nodes)
          const int rc = one(n, R, n_old, n_free, 1000u * n + 10u * R + n_old + 7u * n_free);
          if (rc != 0) { printf("FAILED n=%u R=%u n_old=%u n_free=%u rc=%d\n", n, R, n_old, n_free, rc); return 1; }
          ++cases;
        }
  printf("ok %d\n", cases);
  return 0;
}
