// bang_scan_radix_host.cpp -- the host side of bang_scan_radix.hip (option scan_radix: the exact scan for k up to 4096 by radix select, DESIGN.md
// section 4.21): the argument checks of a bang_k_scan_radix launch, the grid (query tiles x runs) and the scratch size.  No HIP call and no engine
// in this file.
//
// The geometry is the range scan's.  A RUN is a contiguous piece of the points [0, n_nodes) made of whole 32-point tiles and is one wave's share; a
// workgroup is four runs of one tile of queries (32 queries for 8-bit vectors, 16 for float vectors).
//   tiles    = ceil(nq / queries per tile)
//   max_runs = min(ceil(n_nodes / 32), BANG_SCAN_RANGE_MAX_RUNS): never more runs than 32-point tiles
//   runs     = ceil(2048 / tiles) -- eight waves per CU of a 256-CU device --, rounded up to whole workgroups of four, no run shorter than 256
//              points (a run's end costs a partial tile), clamped to [1, max_runs]
// k does not enter the grid: no list is kept per run.  The scratch holds per-query state only, so it does not grow with runs either.
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"

namespace {

bool layout_ok(int dtype, uint32_t D) {
  if (D == 0u || D > BANG_SCAN_ANY_MAX_D) return false;
  if (dtype == BANG_F32) return true;
  return (dtype == BANG_U8 || dtype == BANG_I8) && (D & 3u) == 0u;
}

uint32_t max_runs_of(uint32_t n_nodes) {
  const uint32_t m = (uint32_t)(((uint64_t)n_nodes + 31u) / 32u);
  return m > BANG_SCAN_RANGE_MAX_RUNS ? BANG_SCAN_RANGE_MAX_RUNS : (m < 1u ? 1u : m);
}

void grid(int dtype, uint32_t nq, uint32_t n_nodes, uint32_t* tiles, uint32_t* runs, uint32_t* max_runs) {
  const uint32_t qt = dtype == BANG_F32 ? 16u : 32u;
  const uint32_t t = (nq + qt - 1u) / qt;
  uint32_t r = ((2048u + t - 1u) / t + 3u) & ~3u;
  const uint32_t long_enough = (uint32_t)(((uint64_t)n_nodes + 255u) / 256u);
  if (r > long_enough) r = long_enough;
  const uint32_t most = max_runs_of(n_nodes);
  if (r > most) r = most;
  if (r < 1u) r = 1u;
  *tiles = t;
  *runs = r;
  if (max_runs) *max_runs = most;
}

}  // namespace

extern "C" int bang_scan_radix_geometry(int dtype, uint32_t D, uint32_t nq, uint32_t n_nodes, uint32_t k, uint32_t* tiles, uint32_t* runs,
                                        uint32_t* max_runs) {
  if (!tiles || !runs || nq == 0u || n_nodes == 0u || k == 0u || k > BANG_SCAN_RADIX_MAX_K || nq > BANG_SCAN_MAX_QUERIES) return BANG_ERR_ARG;
  if (!layout_ok(dtype, D)) return BANG_ERR_UNSUPPORTED;
  grid(dtype, nq, n_nodes, tiles, runs, max_runs);
  return BANG_OK;
}

extern "C" uint64_t bang_scan_radix_scratch_bytes(uint32_t nq, uint32_t k, uint32_t runs) {
  (void)runs;                                                              // (no per-run state: the histograms are summed per query)
  // prefix u64 [nq] | bins u32 [nq][256] | rank, fixed bits, flags, emitted, count u32 [nq] each | ids u32 [nq][k] | distance bits u32 [nq][k] |
  // the unresolved word and its padding
  return 8ull * nq + 4ull * BANG_SCAN_RADIX_BINS * nq + 20ull * nq + 8ull * nq * k + 8ull;
}

extern "C" int bang_scan_radix_check(const bang_scan_params* p, uint32_t qdim) {
  if (!p) { bang_set_error("bang_k_scan_radix: the parameter block is null"); return BANG_ERR_ARG; }
  if (!p->d_vec_base || (((uintptr_t)p->d_vec_base) & 3u)) { bang_set_error("bang_k_scan_radix: d_vec_base is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!p->d_queries || (((uintptr_t)p->d_queries) & 3u)) { bang_set_error("bang_k_scan_radix: d_queries is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (p->n_nodes == 0u) { bang_set_error("bang_k_scan_radix: n_nodes = 0"); return BANG_ERR_ARG; }
  if (p->nq == 0u || p->nq > BANG_SCAN_MAX_QUERIES) { bang_set_error("bang_k_scan_radix: nq = %u is outside [1, %u]", p->nq, BANG_SCAN_MAX_QUERIES); return BANG_ERR_ARG; }
  if (p->k == 0u || p->k > BANG_SCAN_RADIX_MAX_K) { bang_set_error("bang_k_scan_radix: k = %u is outside [1, %u]", p->k, BANG_SCAN_RADIX_MAX_K); return BANG_ERR_ARG; }
  if (p->dtype != BANG_F32 && p->dtype != BANG_U8 && p->dtype != BANG_I8) { bang_set_error("bang_k_scan_radix: dtype = %u is none of uint8, int8, float", p->dtype); return BANG_ERR_UNSUPPORTED; }
  if (p->D == 0u || p->D > BANG_SCAN_ANY_MAX_D) { bang_set_error("bang_k_scan_radix: D = %u is outside [1, %u]", p->D, BANG_SCAN_ANY_MAX_D); return BANG_ERR_UNSUPPORTED; }
  if (p->dtype != BANG_F32 && (p->D & 3u) != 0u) { bang_set_error("bang_k_scan_radix: D = %u: 8-bit vectors need D %% 4 == 0 (whole dwords)", p->D); return BANG_ERR_UNSUPPORTED; }
  if ((p->vec_stride & 3u) != 0 || p->vec_stride < (p->dtype == BANG_F32 ? 4ull * p->D : (uint64_t)p->D)) {
    bang_set_error("bang_k_scan_radix: vec_stride = %llu: a stride divisible by 4 that holds the vector (D = %u)", (unsigned long long)p->vec_stride, p->D);
    return BANG_ERR_UNSUPPORTED;
  }
  if (qdim == 0u || (qdim != p->D && qdim + 1u != p->D)) { bang_set_error("bang_k_scan_radix: qdim = %u: a query holds D or D - 1 (MIPS) elements, D = %u", qdim, p->D); return BANG_ERR_ARG; }
  if ((p->d_labels == nullptr) != (p->d_filters == nullptr)) { bang_set_error("bang_k_scan_radix: d_labels and d_filters come together: exactly one of them is null"); return BANG_ERR_ARG; }
  uint32_t tiles = 0, runs = 0, most = 0;
  grid((int)p->dtype, p->nq, p->n_nodes, &tiles, &runs, &most);
  if (p->stripes > most) {
    bang_set_error("bang_k_scan_radix: runs (stripes) = %u exceeds %u: no more runs than 32-point tiles, at most %u", p->stripes, most, BANG_SCAN_RANGE_MAX_RUNS);
    return BANG_ERR_ARG;
  }
  if (p->stripes != 0u) runs = p->stripes;
  if (!p->d_scratch || (((uintptr_t)p->d_scratch) & 7u)) { bang_set_error("bang_k_scan_radix: d_scratch is null or not 8-byte aligned"); return BANG_ERR_ARG; }
  const uint64_t need = bang_scan_radix_scratch_bytes(p->nq, p->k, runs);
  if (p->scratch_bytes < need) {
    bang_set_error("bang_k_scan_radix: scratch_bytes = %llu, %u queries at k = %u need %llu", (unsigned long long)p->scratch_bytes, p->nq, p->k, (unsigned long long)need);
    return BANG_ERR_ARG;
  }
  if (!p->d_ids_out) { bang_set_error("bang_k_scan_radix: d_ids_out is null"); return BANG_ERR_ARG; }
  if (!p->d_dists_out) { bang_set_error("bang_k_scan_radix: d_dists_out is null"); return BANG_ERR_ARG; }
  if (!p->d_matched) { bang_set_error("bang_k_scan_radix: d_matched is null"); return BANG_ERR_ARG; }
  return BANG_OK;
}
