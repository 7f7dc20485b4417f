// bang_reuse_group.cpp -- host side of an insert that re-uses the ids of removed nodes (DESIGN.md section 2 CANON 24, section 4.18), without a HIP
// call and without the engine: the assignment of ids to a batch, and bang_insert_group (bang_insert_group.cpp) with explicit source ids.  The
// sources of the keys are made in input order, which is ascending id order because ids is strictly ascending: the stable sort by target alone
// leaves each target's sources ascending, as there.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bang_c.h"

extern "C" int bang_reuse_assign(const uint32_t* free_ids, uint32_t n_free, uint32_t n, uint32_t N, uint32_t* ids_out, uint32_t* appended_out) {
  if ((n_free != 0 && !free_ids) || (n != 0 && !ids_out) || !appended_out) return BANG_ERR_ARG;
  const uint32_t f = std::min(n, n_free);
  for (uint32_t i = 0; i < f; ++i) {
    if (free_ids[i] >= N || (i != 0 && free_ids[i] <= free_ids[i - 1])) return BANG_ERR_ARG;
  }
  if ((uint64_t)N + (n - f) > 0xFFFFFFFFull) return BANG_ERR_ARG;   // (the appended ids stay 32-bit)
  for (uint32_t i = 0; i < f; ++i) ids_out[i] = free_ids[i];
  for (uint32_t i = f; i < n; ++i) ids_out[i] = N + (i - f);
  *appended_out = n - f;
  return BANG_OK;
}

extern "C" int bang_insert_group_ids(const uint32_t* rows, uint32_t n, uint32_t row_stride, const uint32_t* ids, uint32_t n_old, uint32_t* targets,
                                     uint32_t* offs, uint32_t* srcs, uint32_t* n_targets) {
  if (!rows || !ids || !targets || !offs || !srcs || !n_targets || row_stride < 2u) return BANG_ERR_ARG;
  for (uint32_t i = 1; i < n; ++i)
    if (ids[i] <= ids[i - 1]) return BANG_ERR_ARG;
  const uint32_t R = row_stride - 1u;
  std::vector<uint64_t> keys;
  keys.reserve((size_t)n * R);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* row = rows + (size_t)i * row_stride;
    const uint32_t deg = row[0];
    if (deg > R) return BANG_ERR_ARG;
    for (uint32_t j = 0; j < deg; ++j) {
      const uint32_t t = row[1u + j];
      if (t >= n_old) return BANG_ERR_ARG;                           // a new row lists old nodes only (the search ran on the old graph) ...
      if (std::binary_search(ids, ids + n, t)) return BANG_ERR_ARG;  // ... and never a slot of this batch: no walk reaches a free slot
      keys.push_back(((uint64_t)t << 32) | (uint64_t)ids[i]);
    }
  }
  // LSD radix sort over the bytes of the target that n_old uses (bang_insert_group): stable, so each target's sources stay ascending
  {
    std::vector<uint64_t> tmp(keys.size());
    for (uint32_t shift = 32; n_old != 0 && shift < 64 && ((uint64_t)(n_old - 1u) >> (shift - 32)) != 0; shift += 8) {
      size_t count[257] = {0};
      for (uint64_t k : keys) ++count[((k >> shift) & 0xFFu) + 1u];
      for (int b = 0; b < 256; ++b) count[b + 1] += count[b];
      for (uint64_t k : keys) tmp[count[(k >> shift) & 0xFFu]++] = k;
      keys.swap(tmp);
    }
  }
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  uint32_t nt = 0;
  for (size_t i = 0; i < keys.size(); ++i) {
    const uint32_t t = (uint32_t)(keys[i] >> 32);
    if (i == 0 || t != (uint32_t)(keys[i - 1] >> 32)) { targets[nt] = t; offs[nt] = (uint32_t)i; ++nt; }
    srcs[i] = (uint32_t)keys[i];
  }
  offs[nt] = (uint32_t)keys.size();
  *n_targets = nt;
  return BANG_OK;
}
