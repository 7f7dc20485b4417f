// bang_wave_host.cpp -- the host side the wave-resident search kernels share, without a HIP call in it: the launch geometry (bang_search_exact.hip,
// bang_search_beam.hip, bang_search_lut.hip), the argument checks of an exact-distance launch, and the entry points that route one to the build of
// bang_search_exact.hip that holds its instance.
#include <stdint.h>

#include "bang_c.h"
#include "bang_internal.h"

// Waves per CU: what the kernel's registers allow (512 per SIMD lane, allocated in granules of 8, four SIMDs, at most 8 waves per SIMD) and what
// 160 KB of LDS hold, at most 32; one workgroup of at most 16 waves, within the instance's launch bound.  A batch of fewer than a workgroup-full
// of queries per CU is spread over all CUs with fewer waves each (a wave's iteration is latency bound, as in bang_search_geometry).
extern "C" int bang_wave_geometry(uint32_t regs, uint32_t max_waves_wg, uint32_t wave_bytes, uint32_t cus, uint32_t Q, uint32_t max_wgs,
                                  uint32_t max_waves, uint32_t* workgroups, uint32_t* waves) {
  if (!workgroups || !waves || Q == 0 || regs == 0 || max_waves_wg == 0 || wave_bytes == 0 || cus == 0) return BANG_ERR_ARG;
  const uint32_t alloc = (regs + 7u) & ~7u;
  uint32_t per_simd = 512u / alloc;
  if (per_simd > 8u) per_simd = 8u;
  uint32_t per_cu = 4u * per_simd;
  const uint32_t by_lds = BANG_WAVE_MAX_LDS / wave_bytes;
  if (by_lds < per_cu) per_cu = by_lds;
  if (per_cu > 32u) per_cu = 32u;
  if (per_cu == 0) return BANG_ERR_UNSUPPORTED;
  uint32_t W = per_cu < 16u ? per_cu : 16u;
  if (W > max_waves_wg) W = max_waves_wg;                         // (the instance's launch bound)
  const uint32_t wgs_per_cu = per_cu / W;
  if (max_waves && max_waves < W) W = max_waves;
  uint32_t grid_n;
  if (Q <= cus * W) {                                             // fewer queries than a wave-full per CU: all CUs, fewer waves each
    grid_n = Q < cus ? Q : cus;
    if (max_wgs && max_wgs < grid_n) grid_n = max_wgs;
    const uint32_t share = (Q + grid_n - 1) / grid_n;
    if (share < W) W = share;
  } else {
    const uint32_t want = (Q + W - 1) / W;
    grid_n = cus * wgs_per_cu;
    if (want < grid_n) grid_n = want;
    if (max_wgs && max_wgs < grid_n) grid_n = max_wgs;
  }
  *workgroups = grid_n;
  *waves = W;
  return BANG_OK;
}

// Vector layouts the kernels evaluate.  8-bit: D % 16 == 0; float: D % 4 == 0; D <= 1024; a 4-byte-aligned entry stride; no MIPS padding.
// Those of the fused re-rank (bang_search_can_rerank: D <= 256, 8-bit D / 16 a power of two) run on the narrow instances, the others on the
// wide ones.
extern "C" int bang_search_exact_supported(int dtype, uint32_t D, uint64_t entry_len) {
  if (D == 0 || D > BANG_EXACT_MAX_D || (entry_len & 3u)) return 0;
  if (dtype == BANG_F32) return D % 4u == 0 && entry_len >= 4ull * D;
  if (dtype == BANG_U8 || dtype == BANG_I8) return D % 16u == 0 && entry_len >= D;
  return 0;
}

extern "C" int bang_exact_check_args(const bang_search_params* p, const char* prefix) {
  if (p->R == 0 || p->R > BANG_MAX_R || p->L == 0 || p->L > BANG_MAX_L) { bang_set_error("%s: bad R/L", prefix); return BANG_ERR_ARG; }
  if (p->row_layout > 1u) { bang_set_error("%s: row_layout = %u: the adjacency lists are graph entries in HBM (0) or 256-byte rows (1)", prefix, p->row_layout); return BANG_ERR_UNSUPPORTED; }
  if (p->row_layout == 0u && !p->d_graph) { bang_set_error("%s: the exact-distance kernel needs the graph entries in HBM (d_graph, row_layout = 0)", prefix); return BANG_ERR_UNSUPPORTED; }
  if (!p->d_seed || !p->d_bloom || !p->d_cand_ids || !p->d_cand_cnt || !p->d_next_query || !p->rr_queries || !p->rr_ids_out || !p->rr_dists_out) {
    bang_set_error("%s: null buffer", prefix); return BANG_ERR_ARG;
  }
  if (p->cap_iter == 0 || p->cap_iter > p->L + BANG_EXTRA_ITERS - 1) { bang_set_error("%s: bad iteration cap", prefix); return BANG_ERR_ARG; }
  if (p->rr_k == 0 || p->rr_k > p->L || p->rr_Q_total < p->rr_q0 + p->Q) { bang_set_error("%s: bad k / result rows", prefix); return BANG_ERR_ARG; }
  if (p->rr_vec_f16 > 1u) { bang_set_error("%s: rr_vec_f16 = %u (0 = float / 8-bit rows, 1 = fp16 rows)", prefix, p->rr_vec_f16); return BANG_ERR_ARG; }
  return BANG_OK;
}

extern "C" int bang_exact_check_layout(const bang_search_params* p, const char* prefix) {
  if (p->row_layout == 1u) {
    // the pulled-rows form: adjacency rows in d_graph (pinned host memory; 4-byte aligned), vectors at rr_vec_base + id * rr_vec_stride
    if (!p->d_graph || (((uintptr_t)p->d_graph) & 3u)) { bang_set_error("%s, row_layout = 1: d_graph (the 256-byte adjacency rows) is null or not 4-byte aligned", prefix); return BANG_ERR_ARG; }
    if (p->R > 64u) { bang_set_error("%s, row_layout = 1: R = %u, a 256-byte row holds 64 ids", prefix, p->R); return BANG_ERR_ARG; }
    if (!p->rr_vec_base || (((uintptr_t)p->rr_vec_base) & 3u)) { bang_set_error("%s, row_layout = 1: rr_vec_base (the vectors) is null or not 4-byte aligned", prefix); return BANG_ERR_ARG; }
    if (p->rr_vec_f16 == 1u && ((p->rr_vec_stride & 3u) || p->rr_vec_stride < 2ull * p->rr_D)) {
      bang_set_error("%s, row_layout = 1, rr_vec_f16 = 1: rr_vec_stride = %llu is not divisible by 4 or does not hold rr_D = %u halves", prefix,
                     (unsigned long long)p->rr_vec_stride, p->rr_D);
      return BANG_ERR_ARG;
    }
    if (p->rr_vec_f16 != 1u && !bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->rr_vec_stride)) {
      bang_set_error("%s, row_layout = 1: rr_vec_stride = %llu does not describe vectors the kernel evaluates (dtype %u, D = %u): 8-bit vectors need "
                     "D %% 16 == 0, float vectors D %% 4 == 0; D <= %u; a stride divisible by 4 that holds the vector", prefix,
                     (unsigned long long)p->rr_vec_stride, p->rr_dtype, p->rr_D, BANG_EXACT_MAX_D);
      return BANG_ERR_ARG;
    }
    if (p->vec_bytes != p->rr_D * (p->rr_dtype == BANG_F32 ? 4u : 1u)) { bang_set_error("%s, row_layout = 1: vec_bytes = %u is not rr_D * the element size", prefix, p->vec_bytes); return BANG_ERR_ARG; }
    if (((uintptr_t)p->rr_queries) & 3u) { bang_set_error("%s, row_layout = 1: rr_queries is not 4-byte aligned", prefix); return BANG_ERR_ARG; }
    if (p->n_slices > 1u && !p->d_row_slices) { bang_set_error("%s, row_layout = 1: n_slices = %u needs the slice table d_row_slices", prefix, p->n_slices); return BANG_ERR_ARG; }
    if (p->n_slices > 1u && p->slice_rows == 0u) { bang_set_error("%s, row_layout = 1: n_slices = %u needs slice_rows != 0", prefix, p->n_slices); return BANG_ERR_ARG; }
    if (p->n_rows_hbm != 0u && !p->d_rows_hbm) { bang_set_error("%s, row_layout = 1: n_rows_hbm = %u needs d_rows_hbm", prefix, p->n_rows_hbm); return BANG_ERR_ARG; }
    return BANG_OK;
  }
  if (!bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->entry_len) || p->vec_bytes != p->rr_D * (p->rr_dtype == BANG_F32 ? 4u : 1u) ||
      (((uintptr_t)p->d_graph) & 3u) || (((uintptr_t)p->rr_queries) & 3u)) {
    bang_set_error("%s: unsupported vector layout (dtype %u, D = %u, entry stride %llu): 8-bit vectors need D %% 16 == 0, float vectors "
                   "D %% 4 == 0; D <= %u; an entry stride divisible by 4", prefix, p->rr_dtype, p->rr_D, (unsigned long long)p->entry_len, BANG_EXACT_MAX_D);
    return BANG_ERR_UNSUPPORTED;
  }
  return BANG_OK;
}

// every check of a bang_k_search_exact launch (bang_k_search_exact_labels and _range make them too)
static int exact_check(const bang_search_params* p) {
  static const char* const prefix = "distance = 1";
  int rc = bang_exact_check_args(p, prefix);
  if (rc != BANG_OK) return rc;
  if (p->rr_vec_f16 == 1u) {
    // fp16 rows in the vector table: the pulled-rows form, float queries, the one layout family that has an instance
    if (p->row_layout != 1u) { bang_set_error("distance = 1: rr_vec_f16 = 1 needs row_layout = 1 (graph entries in HBM hold float vectors)"); return BANG_ERR_ARG; }
    if (p->rr_dtype != BANG_F32) { bang_set_error("distance = 1: rr_vec_f16 = 1 needs rr_dtype = BANG_F32 (rr_dtype = %u)", p->rr_dtype); return BANG_ERR_ARG; }
    if (p->rr_D == 0u || p->rr_D % 8u != 0u || p->rr_D > 256u) { bang_set_error("distance = 1: rr_vec_f16 = 1 needs rr_D %% 8 == 0 and rr_D <= 256 (rr_D = %u)", p->rr_D); return BANG_ERR_ARG; }
  }
  return bang_exact_check_layout(p, prefix);
}

extern "C" int bang_k_search_exact(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (p->Q == 0) return BANG_OK;
  const int rc = exact_check(p);
  if (rc != BANG_OK) return rc;
  if (p->row_layout == 1u) {
    if (p->rr_vec_f16 == 1u) return bang_k_search_exact_pull_f16(p, stream);
    if (bang_search_can_rerank((int)p->rr_dtype, p->rr_D, p->rr_vec_stride, 0)) return bang_k_search_exact_pull(p, stream);
    return bang_k_search_exact_wide_pull(p, stream);
  }
  if (bang_search_can_rerank((int)p->rr_dtype, p->rr_D, p->entry_len, 0)) return bang_k_search_exact_hbm(p, stream);
  return bang_k_search_exact_wide(p, stream);
}

// The walk of bang_k_search_exact with per-query label filters (CANON 18): the narrow layouts only, routed on row_layout to the
// instances of bang_search_exact_labels.o / bang_search_exact_labels_pull.o
extern "C" int bang_k_search_exact_labels(const bang_search_params* p, const bang_label_filter* f, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (!f) { bang_set_error("distance = 1, labels: the filter arguments f (bang_label_filter) are null"); return BANG_ERR_ARG; }
  if (!f->d_labels) { bang_set_error("distance = 1, labels: d_labels (one label word per node) is null"); return BANG_ERR_ARG; }
  if (!f->d_filters) { bang_set_error("distance = 1, labels: d_filters (the queries' {any, all} words) is null"); return BANG_ERR_ARG; }
  if (p->n_nodes == 0u) { bang_set_error("distance = 1, labels: n_nodes = 0: d_labels and d_excluded are indexed by node id and need the number of nodes"); return BANG_ERR_ARG; }
  if (p->Q == 0) return BANG_OK;
  const int rc = exact_check(p);
  if (rc != BANG_OK) return rc;
  if (p->rr_vec_f16 == 1u) { bang_set_error("distance = 1, labels: rr_vec_f16 = 1 (fp16 rows) has no label-filter instance"); return BANG_ERR_UNSUPPORTED; }
  const uint64_t stride = p->row_layout == 1u ? p->rr_vec_stride : p->entry_len;
  if (!bang_search_can_rerank((int)p->rr_dtype, p->rr_D, stride, 0)) {
    bang_set_error("distance = 1, labels: the vector layout (dtype %u, rr_D = %u, stride %llu) runs on the wide instances, which have no label-filter form "
                   "(8-bit vectors need D / 16 a power of two; D <= 256)", p->rr_dtype, p->rr_D, (unsigned long long)stride);
    return BANG_ERR_UNSUPPORTED;
  }
  if (p->row_layout == 1u) return bang_k_search_exact_labels_pull(p, f, stream);
  return bang_k_search_exact_labels_hbm(p, f, stream);
}

// The walk of bang_k_search_exact with a per-query radius (CANON 19): the same results, and beside them every evaluated node
// within the radius in the query's row of the hit log.  The narrow layouts only, routed on row_layout to the instances of
// bang_search_exact_range.o / bang_search_exact_range_pull.o
extern "C" int bang_k_search_exact_range(const bang_search_params* p, const bang_range_out* r, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (!r) { bang_set_error("distance = 1, range: the range arguments r (bang_range_out) are null"); return BANG_ERR_ARG; }
  if (!r->d_radius) { bang_set_error("distance = 1, range: d_radius (one radius per query) is null"); return BANG_ERR_ARG; }
  if (!r->d_hit_ids) { bang_set_error("distance = 1, range: d_hit_ids (the hit log's ids) is null"); return BANG_ERR_ARG; }
  if (!r->d_hit_dists) { bang_set_error("distance = 1, range: d_hit_dists (the hit log's distances) is null"); return BANG_ERR_ARG; }
  if (!r->d_offered) { bang_set_error("distance = 1, range: d_offered (the hit counts) is null"); return BANG_ERR_ARG; }
  if (r->cap == 0u || r->cap > BANG_RANGE_MAX_HITS) { bang_set_error("distance = 1, range: cap = %u is outside [1, %u]", r->cap, BANG_RANGE_MAX_HITS); return BANG_ERR_ARG; }
  if (r->d_excluded && p->n_nodes == 0u) { bang_set_error("distance = 1, range: n_nodes = 0 with d_excluded set: the bitmap is indexed by node id and needs the number of nodes"); return BANG_ERR_ARG; }
  if (p->Q == 0) return BANG_OK;
  const int rc = exact_check(p);
  if (rc != BANG_OK) return rc;
  if (p->rr_vec_f16 == 1u) { bang_set_error("distance = 1, range: rr_vec_f16 = 1 (fp16 rows) has no range instance"); return BANG_ERR_UNSUPPORTED; }
  const uint64_t stride = p->row_layout == 1u ? p->rr_vec_stride : p->entry_len;
  if (!bang_search_can_rerank((int)p->rr_dtype, p->rr_D, stride, 0)) {
    bang_set_error("distance = 1, range: the vector layout (dtype %u, rr_D = %u, stride %llu) runs on the wide instances, which have no range form "
                   "(8-bit vectors need D / 16 a power of two; D <= 256)", p->rr_dtype, p->rr_D, (unsigned long long)stride);
    return BANG_ERR_UNSUPPORTED;
  }
  if (p->row_layout == 1u) return bang_k_search_exact_range_pull(p, r, stream);
  return bang_k_search_exact_range_hbm(p, r, stream);
}
