// bang_consolidate_group.cpp -- host side of a consolidation, without a HIP call and without the engine: the affected
// bitmap the scan kernel wrote, as the ascending list of node ids the gather kernel takes in chunks.  One pass over ceil(n_nodes / 32) words
// (31 250 at 10^6 nodes); bits of the last word at or behind n_nodes belong to no node and are ignored.
#include <stdint.h>

#include "bang_c.h"

extern "C" int bang_consolidate_group(const uint32_t* bitmap, uint32_t n_nodes, uint32_t* ids, uint32_t* n_ids) {
  if (!bitmap || !ids || !n_ids) return BANG_ERR_ARG;
  const uint32_t words = n_nodes / 32u + ((n_nodes & 31u) != 0u ? 1u : 0u);
  uint32_t n = 0;
  for (uint32_t w = 0; w < words; ++w) {
    uint32_t bits = bitmap[w];
    if (w == words - 1u && (n_nodes & 31u) != 0u) bits &= (1u << (n_nodes & 31u)) - 1u;
    while (bits != 0u) {
      ids[n++] = w * 32u + (uint32_t)__builtin_ctz(bits);
      bits &= bits - 1u;
    }
  }
  *n_ids = n;
  return BANG_OK;
}
