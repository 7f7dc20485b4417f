// bang_consolidate_host.cpp -- bang_consolidate_e: the exclusion set folded into the graph of a loaded index whose graph is in HBM (DESIGN.md
// section 2 CANON 22, section 4.16; FreshDiskANN Algorithm 4).  The device tables are the only state it changes: the rows of the affected nodes,
// the rows of the removed nodes, the seed list and the exclusion bitmap.  Launches, in stream order:
//   bang_k_consolidate_scan, the affected bitmap down, bang_consolidate_group (no HIP call), the list up
//   per chunk of <= 8192 affected nodes: bang_k_consolidate_gather -> bang_k_range_sort -> bang_k_prune (the insert's back-edge sequence and
//   its scratch sizes)
//   bang_k_consolidate_clear, the seed list, bang_k_bitmap_or (the removed nodes into d_removed), the exclusion bitmap
#include "bang_engine.h"

#include <cmath>

using namespace bang;

namespace {

constexpr uint32_t NODE_CHUNK = 8192;       // affected nodes per launch: 8192 x 512 candidates x 8 B = 32 MB

// device temporaries of one call, freed on every way out
struct Scratch {
  std::vector<void*> ptrs;
  ~Scratch() { for (void* p : ptrs) if (p) (void)hipFree(p); }
  template <typename T> int get(T** p, size_t count) {
    BANG_TRY(dmalloc(p, count));
    ptrs.push_back((void*)*p);
    return BANG_OK;
  }
};

int check_abort(uint32_t* d_abort, const char* where) {
  uint32_t ab = 0;
  HIP_TRY(hipMemcpy(&ab, d_abort, 4, hipMemcpyDeviceToHost));
  if (ab != 0) { bang_set_error("bang_consolidate: %s met a node id outside the index (abort code %u): corrupt adjacency row", where, ab); return BANG_ERR_IO; }
  return BANG_OK;
}

int consolidate(bang_engine* e, float alpha2, uint64_t st[4]) {
  const uint32_t N = e->N, R = e->R, D = e->D, med = (uint32_t)e->medoid;
  const size_t vb = vec_bytes(e);
  const uint64_t el = e->entry_len;
  hipStream_t s = nullptr;
  Scratch sc;
  double* ms = e->consolidate_ms;
  const Clock::time_point t_call = Clock::now();
  // is the medoid in X?  It stays a routing node and stays excluded
  uint32_t med_word = 0;
  HIP_TRY(hipMemcpy(&med_word, e->d_excl + (med >> 5), 4, hipMemcpyDeviceToHost));
  const bool med_excluded = ((med_word >> (med & 31u)) & 1u) != 0u;
  const uint64_t removed = e->n_excl - (med_excluded ? 1u : 0u);
  st[3] = med_excluded ? 1u : 0u;
  if (removed == 0) { ms[3] = ms_since(t_call); return BANG_OK; }   // X = {med}: nothing to fold, nothing is written
  const uint32_t chunk = (uint32_t)std::min((long)NODE_CHUNK, std::max(1L, env_long("BANG_CONSOLIDATE_CHUNK", NODE_CHUNK)));   // test hook, clamped
  const size_t words = ((size_t)N + 31) / 32;
  uint32_t *d_aff = nullptr, *d_ctl = nullptr;
  BANG_TRY(sc.get(&d_aff, words + 1));
  BANG_TRY(sc.get(&d_ctl, 8));                                      // [0] abort word, [1] candidates dropped by the cut
  HIP_TRY(hipMemsetAsync(d_aff, 0, (words + 1) * 4, s));
  HIP_TRY(hipMemsetAsync(d_ctl, 0, 32, s));
  // step 1: the affected nodes
  bang_consolidate_scan_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.d_graph = e->d_graph; sp.entry_len = el; sp.dtype = (uint32_t)e->dtype; sp.D = D; sp.R = R; sp.n_nodes = N; sp.medoid = med;
  sp.d_excluded = e->d_excl; sp.d_affected = d_aff; sp.d_abort = d_ctl;
  BANG_TRY(bang_k_consolidate_scan(&sp, s));
  HIP_TRY(hipStreamSynchronize(s));
  BANG_TRY(check_abort(d_ctl, "the scan of the rows"));
  std::vector<uint32_t> aff(words), nodes(N);
  HIP_TRY(hipMemcpy(aff.data(), d_aff, words * 4, hipMemcpyDeviceToHost));
  uint32_t na = 0;
  if (bang_consolidate_group(aff.data(), N, nodes.data(), &na) != BANG_OK) { bang_set_error("bang_consolidate: the affected bitmap could not be listed"); return BANG_ERR_ARG; }
  ms[0] = ms_since(t_call);
  // steps 2 - 5: candidates, distances, sort, prune.  Every list is made of the node's own old row, rows of removed nodes and vectors, none of
  // which changes before step 6: the chunks may run in any order
  const Clock::time_point t_rows = Clock::now();
  if (na != 0) {
    const uint32_t TC = std::min(na, chunk);
    uint32_t *d_nodes = nullptr, *d_cids = nullptr, *d_offered = nullptr, *d_count = nullptr, *d_own_out = nullptr;
    float* d_cdists = nullptr;
    BANG_TRY(sc.get(&d_nodes, na));
    BANG_TRY(sc.get(&d_cids, (size_t)TC * BANG_PRUNE_MAX_LIST));
    BANG_TRY(sc.get(&d_cdists, (size_t)TC * BANG_PRUNE_MAX_LIST));
    BANG_TRY(sc.get(&d_offered, TC));
    BANG_TRY(sc.get(&d_count, TC));
    BANG_TRY(sc.get(&d_own_out, TC));
    HIP_TRY(hipMemcpy(d_nodes, nodes.data(), (size_t)na * 4, hipMemcpyHostToDevice));
    for (uint32_t t0 = 0; t0 < na; t0 += TC) {
      const uint32_t tn = std::min(TC, na - t0);
      bang_consolidate_gather_params gp;
      memset(&gp, 0, sizeof(gp));
      gp.d_graph = e->d_graph; gp.entry_len = el; gp.dtype = (uint32_t)e->dtype; gp.D = D; gp.R = R; gp.n_nodes = N; gp.medoid = med; gp.n_lists = tn;
      gp.d_excluded = e->d_excl; gp.d_nodes = d_nodes + t0; gp.d_cand_ids = d_cids; gp.d_cand_dists = d_cdists; gp.d_offered = d_offered;
      gp.d_own_out = d_own_out; gp.d_stats = d_ctl + 1; gp.d_abort = d_ctl;
      BANG_TRY(bang_k_consolidate_gather(&gp, s));
      BANG_TRY(bang_k_range_sort(d_cids, d_cdists, d_offered, BANG_PRUNE_MAX_LIST, 0, tn, tn, d_count, s));
      bang_prune_params pp;
      memset(&pp, 0, sizeof(pp));
      pp.d_graph = e->d_graph; pp.entry_len = el; pp.dtype = (uint32_t)e->dtype; pp.D = D; pp.n_nodes = N; pp.R = R; pp.alpha2 = alpha2;
      pp.n_lists = tn; pp.list_stride = BANG_PRUNE_MAX_LIST; pp.d_list_ids = d_cids; pp.d_list_dists = d_cdists; pp.d_list_cnt = d_count;
      pp.d_own = d_own_out; pp.d_out = e->d_graph + vb; pp.out_stride = el; pp.out_by_own = 1; pp.d_abort = d_ctl;
      BANG_TRY(bang_k_prune(&pp, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    BANG_TRY(check_abort(d_ctl, "the gather of the candidates"));
  }
  ms[1] = ms_since(t_rows);
  // step 6: the rows of the removed nodes.  Up to here a failure left a graph every walk may run on -- rewritten rows list live nodes only, the
  // others nodes that still exist -- and the exclusion set untouched, so answers stayed correct: no latch like insert_broken is needed.  From
  // here on nothing but a HIP error can fail
  const Clock::time_point t_clear = Clock::now();
  bang_consolidate_clear_params cp;
  memset(&cp, 0, sizeof(cp));
  cp.d_graph = e->d_graph; cp.entry_len = el; cp.dtype = (uint32_t)e->dtype; cp.D = D; cp.R = R; cp.n_nodes = N; cp.medoid = med; cp.d_excluded = e->d_excl;
  BANG_TRY(bang_k_consolidate_clear(&cp, s));
  HIP_TRY(hipStreamSynchronize(s));
  // step 7: the seed list (from the medoid's row as it stands), the exclusion set X & {med}, the counters
  BANG_TRY(rebuild_seed(e));
  uint32_t dropped = 0;
  HIP_TRY(hipMemcpy(&dropped, d_ctl + 1, 4, hipMemcpyDeviceToHost));
  const size_t nodes_cap = std::max<size_t>(N, e->capacity > 0 ? (size_t)e->capacity : 0);
  const size_t excl_words = (nodes_cap + 31) / 32 + 1;
  // the removed set D = X \ {med} joins d_removed (what an exact scan leaves out: the removed nodes keep their vectors) before X is reduced
  if (!e->d_removed) {
    BANG_TRY(dmalloc(&e->d_removed, excl_words));
    HIP_TRY(hipMemset(e->d_removed, 0, excl_words * 4));
  }
  BANG_TRY(bang_k_bitmap_or(e->d_removed, e->d_excl, excl_words, med >> 5, 1u << (med & 31u), s));
  HIP_TRY(hipStreamSynchronize(s));
  if (med_excluded) {
    const uint32_t bit = 1u << (med & 31u);
    HIP_TRY(hipMemset(e->d_excl, 0, ((nodes_cap + 31) / 32 + 1) * 4));
    HIP_TRY(hipMemcpy(e->d_excl + (med >> 5), &bit, 4, hipMemcpyHostToDevice));
    e->n_excl = 1;
  } else {
    dfree(e->d_excl);
    e->n_excl = 0;
  }
  st[0] = na; st[1] = removed; st[2] = dropped;
  e->stat_cons_rows += na; e->stat_cons_removed += removed; e->stat_cons_dropped += dropped;
  ms[2] = ms_since(t_clear);
  ms[3] = ms_since(t_call);
  return BANG_OK;
}

}  // namespace

extern "C" int bang_consolidate_e(bang_engine_t* e, float alpha, uint64_t* out_stats4) {
  if (!e) { bang_set_error("bang_consolidate: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("bang_consolidate: no index is loaded"); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("bang_consolidate: an allocation is live (call bang_free first): a batch may be reading the tables"); return BANG_ERR_ARG; }
  if (e->insert_broken) { bang_set_error("bang_consolidate: an earlier insert failed half-way and old rows may list ids beyond N: unload this engine (bang_unload) and load the index again"); return BANG_ERR_ARG; }
  if (e->capacity <= 0 || !e->d_graph) { bang_set_error("bang_consolidate: the index was loaded without option capacity: only an engine whose tables may change (graph = device, capacity >= N) consolidates"); return BANG_ERR_ARG; }
  if (!std::isfinite(alpha) || alpha < 1.0f || alpha > 8.0f) { bang_set_error("bang_consolidate: alpha = %g is not finite or outside [1, 8]", (double)alpha); return BANG_ERR_ARG; }
  if (e->params_set && e->distfn == BANG_DIST_MIPS) { bang_set_error("bang_consolidate: MIPS search parameters are set: the prune runs on L2 distances only"); return BANG_ERR_UNSUPPORTED; }
  if (!bang_search_can_rerank(e->dtype, e->D, e->entry_len, 0)) {
    bang_set_error("bang_consolidate: the vector layout (dtype %d, D = %u, entry stride %llu) is outside bang_search_can_rerank: 8-bit vectors need D %% 16 == 0 "
                   "with D / 16 a power of two, float vectors D %% 4 == 0; D <= 256", e->dtype, e->D, (unsigned long long)e->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  uint64_t st[4] = {0, 0, 0, 0};
  for (double& x : e->consolidate_ms) x = 0;
  if (e->n_excl != 0 && e->d_excl) {
    BANG_TRY(ensure_device(e));
    const float a32 = alpha;
    const float alpha2 = a32 * a32;
    const int rc = consolidate(e, alpha2, st);
    if (rc != BANG_OK) { (void)hipDeviceSynchronize(); return rc; }
  }
  if (out_stats4) memcpy(out_stats4, st, sizeof(st));
  return BANG_OK;
}

extern "C" int bang_get_stats_ext6(bang_engine_t* e, bang_stats_ext6* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats_ext5(e, &out->ext5));
  out->consolidated_rows = e->stat_cons_rows;
  out->removed = e->stat_cons_removed;
  out->consolidate_dropped = e->stat_cons_dropped;
  return BANG_OK;
}

extern "C" int bang_get_consolidate_times(bang_engine_t* e, double* ms4) {
  if (!e || !ms4) return BANG_ERR_ARG;
  memcpy(ms4, e->consolidate_ms, sizeof(e->consolidate_ms));
  return BANG_OK;
}
