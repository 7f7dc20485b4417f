// bang_insert_group.cpp -- host side of an insert, without a HIP call and without the engine: the new rows of a batch
// grouped by target.  Every (target, source) pair of the n rows becomes one 64-bit key (target << 32 | source); a stable sort of the keys by
// target puts the targets in ascending order and, within a target, the new ids that list it in ascending order -- the CSR the back-edge kernel
// reads.  n * R keys (at most 16384 x 64 = 1 M, 8 MB), a byte-wise radix sort; tools/insert_sweep.py reports the share of this step.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "bang_c.h"

extern "C" int bang_insert_group(const uint32_t* rows, uint32_t n, uint32_t row_stride, uint32_t first_id, uint32_t n_old, uint32_t* targets,
                                 uint32_t* offs, uint32_t* srcs, uint32_t* n_targets) {
  if (!rows || !targets || !offs || !srcs || !n_targets || row_stride < 2u) return BANG_ERR_ARG;
  const uint32_t R = row_stride - 1u;
  std::vector<uint64_t> keys;
  keys.reserve((size_t)n * R);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* row = rows + (size_t)i * row_stride;
    const uint32_t deg = row[0];
    if (deg > R) return BANG_ERR_ARG;
    for (uint32_t j = 0; j < deg; ++j) {
      if (row[1u + j] >= n_old) return BANG_ERR_ARG;              // a new row lists old nodes only (the search ran on the old graph)
      keys.push_back(((uint64_t)row[1u + j] << 32) | (uint64_t)(first_id + i));
    }
  }
  // The keys were made in ascending source order, so a STABLE sort by target alone leaves each target's sources ascending: an LSD radix sort
  // over the bytes of the target that n_old uses (three passes at 10^6 .. 16 M nodes): linear in the number of keys, no compare of whole keys
  {
    std::vector<uint64_t> tmp(keys.size());
    for (uint32_t shift = 32; shift < 64 && ((uint64_t)(n_old - 1u) >> (shift - 32)) != 0; shift += 8) {
      size_t count[257] = {0};
      for (uint64_t k : keys) ++count[((k >> shift) & 0xFFu) + 1u];
      for (int b = 0; b < 256; ++b) count[b + 1] += count[b];
      for (uint64_t k : keys) tmp[count[(k >> shift) & 0xFFu]++] = k;
      keys.swap(tmp);
    }
  }
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());  // (a row never lists an id twice; kept as the CSR's contract)
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
