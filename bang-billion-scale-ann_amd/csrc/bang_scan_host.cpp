// bang_scan_host.cpp -- the host side of bang_scan.hip (the exact scan, DESIGN.md section 2 CANON 23, section 4.17): the argument checks of a
// bang_k_scan launch, the grid (query tiles x stripes) and the scratch size.  No HIP call and no engine in this file: the tests build it alone.
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"

namespace {

// the layouts of bang_search_can_rerank, with the stride holding the vector
bool scan_layout(int dtype, uint32_t D, uint64_t stride) {
  const uint32_t G = D >> 4;
  if ((stride & 3u) != 0 || D > 256u) return false;
  if (dtype == BANG_F32) return D >= 4u && (D & 3u) == 0u && stride >= 4ull * D;
  return (dtype == BANG_U8 || dtype == BANG_I8) && D >= 16u && (D & 15u) == 0u && (G & (G - 1u)) == 0u && stride >= D;
}
uint32_t query_tile(int dtype) { return dtype == BANG_F32 ? 16u : 32u; }       // queries per workgroup
uint32_t round_points(int dtype) { return dtype == BANG_F32 ? 256u : 128u; }   // points a workgroup takes between two cuts of its lists

}  // namespace

extern "C" uint32_t bang_scan_max_stripes(int dtype, uint32_t n_nodes, uint32_t k) {
  if (k == 0u || k > BANG_SCAN_MAX_K || n_nodes == 0u) return 0u;
  const uint32_t rp = round_points(dtype);
  const uint32_t by_points = (uint32_t)(((uint64_t)n_nodes + rp - 1u) / rp);
  const uint32_t by_keys = BANG_SCAN_MAX_KEYS / k;
  return by_points < by_keys ? by_points : by_keys;
}

extern "C" int bang_scan_geometry(int dtype, uint32_t D, uint32_t nq, uint32_t n_nodes, uint32_t k, uint32_t* tiles, uint32_t* stripes) {
  if (!tiles || !stripes || nq == 0u || n_nodes == 0u || k == 0u || k > BANG_SCAN_MAX_K || nq > BANG_SCAN_MAX_QUERIES) return BANG_ERR_ARG;
  if (!scan_layout(dtype, D, dtype == BANG_F32 ? 4ull * D : (uint64_t)D)) return BANG_ERR_UNSUPPORTED;
  const uint32_t qt = query_tile(dtype);
  const uint32_t t = (nq + qt - 1u) / qt;
  // about four workgroups per CU of a 256-CU device, and no stripe shorter than 16 rounds: a stripe's lists cost a sort however short it is
  const uint32_t want = (1024u + t - 1u) / t;
  const uint32_t rp = round_points(dtype);
  const uint32_t long_enough = (uint32_t)(((uint64_t)n_nodes + 16ull * rp - 1u) / (16ull * rp));
  uint32_t s = want < long_enough ? want : long_enough;
  const uint32_t most = bang_scan_max_stripes(dtype, n_nodes, k);
  if (s > most) s = most;
  if (s < 1u) s = 1u;
  *tiles = t;
  *stripes = s;
  return BANG_OK;
}

extern "C" uint64_t bang_scan_scratch_bytes(uint32_t nq, uint32_t k, uint32_t stripes) {
  // ids u32 [nq][stripes * k] | distance bits u32 [nq][stripes * k] | offered u32 [nq] | count u32 [nq]
  return 8ull * nq * stripes * k + 8ull * nq;
}

extern "C" int bang_scan_check(const bang_scan_params* p) {
  if (!p) { bang_set_error("bang_k_scan: the parameter block is null"); return BANG_ERR_ARG; }
  if (!p->d_vec_base || (((uintptr_t)p->d_vec_base) & 3u)) { bang_set_error("bang_k_scan: d_vec_base is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!p->d_queries || (((uintptr_t)p->d_queries) & 3u)) { bang_set_error("bang_k_scan: d_queries is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (p->n_nodes == 0u) { bang_set_error("bang_k_scan: n_nodes = 0"); return BANG_ERR_ARG; }
  if (p->nq == 0u || p->nq > BANG_SCAN_MAX_QUERIES) { bang_set_error("bang_k_scan: nq = %u is outside [1, %u]", p->nq, BANG_SCAN_MAX_QUERIES); return BANG_ERR_ARG; }
  if (p->k == 0u || p->k > BANG_SCAN_MAX_K) { bang_set_error("bang_k_scan: k = %u is outside [1, %u]", p->k, BANG_SCAN_MAX_K); return BANG_ERR_ARG; }
  if (!scan_layout((int)p->dtype, p->D, p->vec_stride)) {
    bang_set_error("bang_k_scan: the vector layout (dtype %u, D = %u, vec_stride %llu) is outside bang_search_can_rerank: 8-bit vectors need D %% 16 == 0 with "
                   "D / 16 a power of two, float vectors D %% 4 == 0; D <= 256; a stride divisible by 4 that holds the vector", p->dtype, p->D,
                   (unsigned long long)p->vec_stride);
    return BANG_ERR_UNSUPPORTED;
  }
  if ((p->d_labels == nullptr) != (p->d_filters == nullptr)) { bang_set_error("bang_k_scan: d_labels and d_filters come together: exactly one of them is null"); return BANG_ERR_ARG; }
  const uint32_t most = bang_scan_max_stripes((int)p->dtype, p->n_nodes, p->k);
  if (p->stripes > most) {
    bang_set_error("bang_k_scan: stripes = %u exceeds %u: stripes * k <= %u and no stripe without a round of points", p->stripes, most, BANG_SCAN_MAX_KEYS);
    return BANG_ERR_ARG;
  }
  uint32_t tiles = 0, stripes = p->stripes;
  if (stripes == 0u && bang_scan_geometry((int)p->dtype, p->D, p->nq, p->n_nodes, p->k, &tiles, &stripes) != BANG_OK) {
    bang_set_error("bang_k_scan: no geometry for this launch");
    return BANG_ERR_ARG;
  }
  if (!p->d_scratch || (((uintptr_t)p->d_scratch) & 7u)) { bang_set_error("bang_k_scan: d_scratch is null or not 8-byte aligned"); return BANG_ERR_ARG; }
  const uint64_t need = bang_scan_scratch_bytes(p->nq, p->k, stripes);
  if (p->scratch_bytes < need) {
    bang_set_error("bang_k_scan: scratch_bytes = %llu, %u stripes of %u queries at k = %u need %llu", (unsigned long long)p->scratch_bytes, stripes, p->nq, p->k,
                   (unsigned long long)need);
    return BANG_ERR_ARG;
  }
  if (!p->d_ids_out) { bang_set_error("bang_k_scan: d_ids_out is null"); return BANG_ERR_ARG; }
  if (!p->d_dists_out) { bang_set_error("bang_k_scan: d_dists_out is null"); return BANG_ERR_ARG; }
  if (!p->d_matched) { bang_set_error("bang_k_scan: d_matched is null"); return BANG_ERR_ARG; }
  return BANG_OK;
}
