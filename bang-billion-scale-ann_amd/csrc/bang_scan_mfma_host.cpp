// bang_scan_mfma_host.cpp -- the host side of bang_scan_mfma.hip (option scan_mfma): the argument checks of a
// bang_k_scan_f32_mfma launch and its grid.  A round of that kernel is 128 points (four waves of 32), not the 256 of the float chain kernels, so the
// largest number of stripes is this file's own rule; the scratch is bang_scan_scratch_bytes'.
// No HIP call and no engine in this file: the tests build it alone.
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"

namespace {
constexpr uint32_t QUERY_TILE = 32u;     // queries per workgroup: one A tile of v_mfma_f32_32x32x2_f32
constexpr uint32_t ROUND = 128u;         // points a workgroup takes between two cuts of its lists
}  // namespace

extern "C" uint32_t bang_scan_f32_mfma_max_stripes(uint32_t n_nodes, uint32_t k) {
  if (k == 0u || k > BANG_SCAN_MAX_K || n_nodes == 0u) return 0u;
  const uint32_t by_points = (uint32_t)(((uint64_t)n_nodes + ROUND - 1u) / ROUND);
  const uint32_t by_keys = BANG_SCAN_MAX_KEYS / k;
  return by_points < by_keys ? by_points : by_keys;
}

extern "C" int bang_scan_f32_mfma_geometry(uint32_t D, uint32_t nq, uint32_t n_nodes, uint32_t k, uint32_t* tiles, uint32_t* stripes) {
  if (!tiles || !stripes || nq == 0u || n_nodes == 0u || k == 0u || k > BANG_SCAN_MAX_K || nq > BANG_SCAN_MAX_QUERIES) return BANG_ERR_ARG;
  if (D == 0u || D > BANG_SCAN_ANY_MAX_D) return BANG_ERR_UNSUPPORTED;
  const uint32_t t = (nq + QUERY_TILE - 1u) / QUERY_TILE;
  // one workgroup per CU (its lists and query image leave no room for a second) on a 256-CU device, twice over; no stripe shorter than 16 rounds
  const uint32_t want = (512u + t - 1u) / t;
  const uint32_t long_enough = (uint32_t)(((uint64_t)n_nodes + 16ull * ROUND - 1u) / (16ull * ROUND));
  uint32_t s = want < long_enough ? want : long_enough;
  const uint32_t most = bang_scan_f32_mfma_max_stripes(n_nodes, k);
  if (s > most) s = most;
  if (s < 1u) s = 1u;
  // a stripe is ceil(n_nodes / s) points rounded up to whole rounds: fewer stripes until the last one still begins inside the table
  for (; s > 1u; --s) {
    const uint64_t per = (((uint64_t)n_nodes + s - 1u) / s + ROUND - 1u) / ROUND * ROUND;
    if ((uint64_t)(s - 1u) * per < (uint64_t)n_nodes) break;
  }
  *tiles = t;
  *stripes = s;
  return BANG_OK;
}

extern "C" int bang_scan_f32_mfma_check(const bang_scan_params* p, uint32_t qdim) {
  if (!p) { bang_set_error("bang_k_scan_f32_mfma: the parameter block is null"); return BANG_ERR_ARG; }
  if (!p->d_vec_base || (((uintptr_t)p->d_vec_base) & 3u)) { bang_set_error("bang_k_scan_f32_mfma: d_vec_base is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!p->d_queries || (((uintptr_t)p->d_queries) & 3u)) { bang_set_error("bang_k_scan_f32_mfma: d_queries is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (p->n_nodes == 0u) { bang_set_error("bang_k_scan_f32_mfma: n_nodes = 0"); return BANG_ERR_ARG; }
  if (p->nq == 0u || p->nq > BANG_SCAN_MAX_QUERIES) { bang_set_error("bang_k_scan_f32_mfma: nq = %u is outside [1, %u]", p->nq, BANG_SCAN_MAX_QUERIES); return BANG_ERR_ARG; }
  if (p->k == 0u || p->k > BANG_SCAN_MAX_K) { bang_set_error("bang_k_scan_f32_mfma: k = %u is outside [1, %u]", p->k, BANG_SCAN_MAX_K); return BANG_ERR_ARG; }
  if (p->dtype != BANG_F32) { bang_set_error("bang_k_scan_f32_mfma: dtype = %u is not float: 8-bit vectors run on bang_k_scan / bang_k_scan_any", p->dtype); return BANG_ERR_UNSUPPORTED; }
  if (p->D == 0u || p->D > BANG_SCAN_ANY_MAX_D) { bang_set_error("bang_k_scan_f32_mfma: D = %u is outside [1, %u]", p->D, BANG_SCAN_ANY_MAX_D); return BANG_ERR_UNSUPPORTED; }
  if ((p->vec_stride & 3u) != 0 || p->vec_stride < 4ull * p->D) {
    bang_set_error("bang_k_scan_f32_mfma: vec_stride = %llu: a stride divisible by 4 that holds the vector (D = %u)", (unsigned long long)p->vec_stride, p->D);
    return BANG_ERR_UNSUPPORTED;
  }
  if (qdim == 0u || (qdim != p->D && qdim + 1u != p->D)) { bang_set_error("bang_k_scan_f32_mfma: qdim = %u: a query holds D or D - 1 (MIPS) elements, D = %u", qdim, p->D); return BANG_ERR_ARG; }
  if ((p->d_labels == nullptr) != (p->d_filters == nullptr)) { bang_set_error("bang_k_scan_f32_mfma: d_labels and d_filters come together: exactly one of them is null"); return BANG_ERR_ARG; }
  const uint32_t most = bang_scan_f32_mfma_max_stripes(p->n_nodes, p->k);
  if (p->stripes > most) {
    bang_set_error("bang_k_scan_f32_mfma: stripes = %u exceeds %u: stripes * k <= %u and no stripe without a round of %u points", p->stripes, most, BANG_SCAN_MAX_KEYS, ROUND);
    return BANG_ERR_ARG;
  }
  uint32_t tiles = 0, stripes = p->stripes;
  if (stripes == 0u) (void)bang_scan_f32_mfma_geometry(p->D, p->nq, p->n_nodes, p->k, &tiles, &stripes);
  if (!p->d_scratch || (((uintptr_t)p->d_scratch) & 7u)) { bang_set_error("bang_k_scan_f32_mfma: d_scratch is null or not 8-byte aligned"); return BANG_ERR_ARG; }
  const uint64_t need = bang_scan_scratch_bytes(p->nq, p->k, stripes);
  if (p->scratch_bytes < need) {
    bang_set_error("bang_k_scan_f32_mfma: scratch_bytes = %llu, %u stripes of %u queries at k = %u need %llu", (unsigned long long)p->scratch_bytes, stripes, p->nq, p->k,
                   (unsigned long long)need);
    return BANG_ERR_ARG;
  }
  if (!p->d_ids_out) { bang_set_error("bang_k_scan_f32_mfma: d_ids_out is null"); return BANG_ERR_ARG; }
  if (!p->d_dists_out) { bang_set_error("bang_k_scan_f32_mfma: d_dists_out is null"); return BANG_ERR_ARG; }
  if (!p->d_matched) { bang_set_error("bang_k_scan_f32_mfma: d_matched is null"); return BANG_ERR_ARG; }
  return BANG_OK;
}
