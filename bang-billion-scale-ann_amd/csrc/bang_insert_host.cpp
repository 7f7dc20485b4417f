// bang_insert_host.cpp -- bang_insert_e: new points into a loaded index whose graph is in HBM (DESIGN.md section 2 CANON 21, section 4.15), and the
// downloads that let a caller persist the result (bang_get_entries_e / bang_get_codes_e).  With the graph in HBM the host copy is read only during
// bang_load, so the device tables are the only state an insert changes: graph entries N .. N + n - 1 (vector + pruned row), the rows of the old
// nodes the new rows list (back-edges), the code rows N .. N + n - 1 and the seed list.  Launches, in stream order:
//   per chunk of <= 1024 points: bang_k_search_exact (rr_k = L) -> bang_k_worklist_lists -> bang_k_prune (rows into the new entries)
//   the new rows back to the host, bang_insert_group (no HIP call), the CSR up
//   per chunk of <= 8192 targets: bang_k_backedge -> bang_k_range_sort -> bang_k_prune (rows of the overflowing targets)
//   bang_k_pq_encode in chunks of 256 points
#include "bang_engine.h"

#include <cmath>

using namespace bang;

namespace {

constexpr uint32_t SEARCH_CHUNK = 1024;     // points per search launch: 1024 visited filters of 50 KB
constexpr uint32_t TARGET_CHUNK = 8192;     // back-edge targets per launch: 8192 x 512 candidates x 8 B = 32 MB
constexpr uint32_t ENCODE_CHUNK = 256;      // points per K1 launch: 256 x m x 1 KB of tables

// test hooks: a chunk size from the environment is clamped to [1, the size above]; unset = the size above
uint32_t chunk_of(long asked, uint32_t dflt) { return (uint32_t)std::min((long)dflt, std::max(1L, asked)); }

// device temporaries of one call, freed on every way out
struct Scratch {
  std::vector<void*> ptrs;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // phase stamps on the stream (bang_get_insert_times)
  ~Scratch() {
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  }
  int elapsed(int a, int b, double* ms) {                        // += the stream time between two recorded stamps (both complete)
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, ev[a], ev[b]));
    *ms += t;
    return BANG_OK;
  }
  template <typename T> int get(T** p, size_t count) {
    BANG_TRY(dmalloc(p, count));
    ptrs.push_back((void*)*p);
    return BANG_OK;
  }
};

int check_abort(uint32_t* d_abort, const char* where) {
  uint32_t ab = 0;
  HIP_TRY(hipMemcpy(&ab, d_abort, 4, hipMemcpyDeviceToHost));
  if (ab != 0) { bang_set_error("bang_insert: %s met a node id outside the index (abort code %u): corrupt adjacency row", where, ab); return BANG_ERR_IO; }
  return BANG_OK;
}

int insert_batch(bang_engine* e, const uint8_t* h_vectors, uint32_t n, uint32_t L, float alpha2) {
  const uint32_t N = e->N, R = e->R, D = e->D;
  const size_t vb = vec_bytes(e);
  const uint64_t el = e->entry_len;
  hipStream_t s = nullptr;
  Scratch sc;
  const uint32_t search_chunk = chunk_of(env_long("BANG_INSERT_SEARCH_CHUNK", SEARCH_CHUNK), SEARCH_CHUNK);
  const uint32_t target_chunk = chunk_of(env_long("BANG_INSERT_TARGET_CHUNK", TARGET_CHUNK), TARGET_CHUNK);
  const uint32_t encode_chunk = chunk_of(env_long("BANG_INSERT_ENCODE_CHUNK", ENCODE_CHUNK), ENCODE_CHUNK);
  const uint32_t QC = std::min(n, search_chunk);
  uint8_t* d_vecs = nullptr;
  uint32_t *d_bloom = nullptr, *d_cand_ids = nullptr, *d_cand_cnt = nullptr, *d_ctl = nullptr, *d_list_ids = nullptr, *d_list_cnt = nullptr, *d_own = nullptr;
  uint64_t* d_wl_ids = nullptr;
  float *d_wl_dists = nullptr, *d_list_dists = nullptr;
  BANG_TRY(sc.get(&d_vecs, (size_t)n * vb + 256));
  BANG_TRY(sc.get(&d_bloom, (size_t)QC * BANG_BF_WORDS));
  BANG_TRY(sc.get(&d_cand_ids, (size_t)QC * (L + BANG_EXTRA_ITERS)));
  BANG_TRY(sc.get(&d_cand_cnt, QC));
  BANG_TRY(sc.get(&d_ctl, 8));                                    // [0] hand-out counter, [1] abort word, [2..4] back-edge statistics
  BANG_TRY(sc.get(&d_wl_ids, (size_t)QC * L));
  BANG_TRY(sc.get(&d_wl_dists, (size_t)QC * L));
  BANG_TRY(sc.get(&d_list_ids, (size_t)QC * L));
  BANG_TRY(sc.get(&d_list_dists, (size_t)QC * L));
  BANG_TRY(sc.get(&d_list_cnt, QC));
  BANG_TRY(sc.get(&d_own, n));
  for (hipEvent_t& x : sc.ev) HIP_TRY(hipEventCreate(&x));
  double* ms = e->insert_ms;                                      // {search, prune, host grouping, back-edges, encode, whole call}
  for (int i = 0; i < 6; ++i) ms[i] = 0;
  const Clock::time_point t_call = Clock::now();
  HIP_TRY(hipMemcpy(d_vecs, h_vectors, (size_t)n * vb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_ctl, 0, 32));
  // step 3, first half: the new entries with their vectors and empty rows (unused slots 0); the search below never reaches them (n_nodes = N)
  {
    std::vector<uint8_t> ent((size_t)n * el, 0);
    for (uint32_t i = 0; i < n; ++i) memcpy(ent.data() + (size_t)i * el, h_vectors + (size_t)i * vb, vb);
    HIP_TRY(hipMemcpy(e->d_graph + (uint64_t)N * el, ent.data(), ent.size(), hipMemcpyHostToDevice));
    std::vector<uint32_t> own(n);
    for (uint32_t i = 0; i < n; ++i) own[i] = N + i;
    HIP_TRY(hipMemcpy(d_own, own.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  // steps 1 + 2: candidates and rows
  for (uint32_t q0 = 0; q0 < n; q0 += QC) {
    const uint32_t nq = std::min(QC, n - q0);
    HIP_TRY(hipMemsetAsync(d_bloom, 0, (size_t)nq * BANG_BF_WORDS * 4, s));
    HIP_TRY(hipMemsetAsync(d_ctl, 0, 4, s));
    bang_search_params sp;
    memset(&sp, 0, sizeof(sp));
    sp.Q = nq; sp.R = R; sp.m = e->m; sp.L = L; sp.medoid = (uint32_t)e->medoid; sp.cap_iter = L + BANG_EXTRA_ITERS - 1;
    sp.d_seed = e->d_seed; sp.d_graph = e->d_graph; sp.entry_len = el; sp.vec_bytes = (uint32_t)vb; sp.row_layout = 0;
    sp.d_bloom = d_bloom; sp.d_cand_ids = d_cand_ids; sp.d_cand_cnt = d_cand_cnt; sp.d_next_query = d_ctl; sp.d_abort = d_ctl + 1;
    sp.n_nodes = N;
    sp.rr_queries = d_vecs + (size_t)q0 * vb; sp.rr_dtype = (uint32_t)e->dtype; sp.rr_D = D; sp.rr_k = L; sp.rr_q0 = 0; sp.rr_Q_total = nq;
    sp.rr_ids_out = d_wl_ids; sp.rr_dists_out = d_wl_dists;
    HIP_TRY(hipEventRecord(sc.ev[0], s));
    BANG_TRY(bang_k_search_exact(&sp, s));
    HIP_TRY(hipEventRecord(sc.ev[1], s));
    BANG_TRY(bang_k_worklist_lists(d_wl_ids, d_wl_dists, L, 0, nq, nq, d_list_ids, d_list_dists, L, d_list_cnt, s));
    bang_prune_params pp;
    memset(&pp, 0, sizeof(pp));
    pp.d_graph = e->d_graph; pp.entry_len = el; pp.dtype = (uint32_t)e->dtype; pp.D = D; pp.R = R; pp.alpha2 = alpha2;
    pp.n_lists = nq; pp.list_stride = L; pp.d_list_ids = d_list_ids; pp.d_list_dists = d_list_dists; pp.d_list_cnt = d_list_cnt;
    pp.d_own = d_own + q0; pp.d_out = e->d_graph + vb; pp.out_stride = el; pp.out_by_own = 1; pp.d_abort = d_ctl + 1;
    pp.n_nodes = N + n;                                            // (own ids N .. N + n - 1 name rows inside the table; list ids are < N)
    BANG_TRY(bang_k_prune(&pp, s));
    HIP_TRY(hipEventRecord(sc.ev[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    BANG_TRY(sc.elapsed(0, 1, &ms[0]));
    BANG_TRY(sc.elapsed(1, 2, &ms[1]));
    BANG_TRY(check_abort(d_ctl + 1, "the candidate search"));
  }
  // step 4: back-edges.  The new rows come back once, are grouped on the host, and the CSR goes up
  const Clock::time_point t_group = Clock::now();
  const uint32_t rs = R + 1;
  std::vector<uint32_t> rows((size_t)n * rs);
  HIP_TRY(hipMemcpy2D(rows.data(), (size_t)rs * 4, e->d_graph + (uint64_t)N * el + vb, el, (size_t)rs * 4, n, hipMemcpyDeviceToHost));
  std::vector<uint32_t> targets((size_t)n * R), offs((size_t)n * R + 1), srcs((size_t)n * R);
  uint32_t nt = 0;
  if (bang_insert_group(rows.data(), n, rs, N, N, targets.data(), offs.data(), srcs.data(), &nt) != BANG_OK) {
    bang_set_error("bang_insert: a new row lists an id outside the old index");
    return BANG_ERR_IO;
  }
  ms[2] = ms_since(t_group);
  HIP_TRY(hipEventRecord(sc.ev[0], s));
  if (nt != 0) {
    const uint32_t TC = std::min(nt, target_chunk);
    uint32_t *d_targets = nullptr, *d_offs = nullptr, *d_srcs = nullptr, *d_cids = nullptr, *d_offered = nullptr, *d_count = nullptr, *d_own_out = nullptr;
    float* d_cdists = nullptr;
    BANG_TRY(sc.get(&d_targets, nt));
    BANG_TRY(sc.get(&d_offs, (size_t)nt + 1));
    BANG_TRY(sc.get(&d_srcs, offs[nt]));
    BANG_TRY(sc.get(&d_cids, (size_t)TC * BANG_PRUNE_MAX_LIST));
    BANG_TRY(sc.get(&d_cdists, (size_t)TC * BANG_PRUNE_MAX_LIST));
    BANG_TRY(sc.get(&d_offered, TC));
    BANG_TRY(sc.get(&d_count, TC));
    BANG_TRY(sc.get(&d_own_out, TC));
    HIP_TRY(hipMemcpy(d_targets, targets.data(), (size_t)nt * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offs, offs.data(), ((size_t)nt + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_srcs, srcs.data(), (size_t)offs[nt] * 4, hipMemcpyHostToDevice));
    // from here on old rows change: a failure before the end leaves rows that list ids >= N, and the engine says so until it is unloaded
    // (everything written so far lies behind N, where no kernel looks)
    e->insert_broken = true;
    for (uint32_t t0 = 0; t0 < nt; t0 += TC) {
      const uint32_t tn = std::min(TC, nt - t0);
      bang_backedge_params bp;
      memset(&bp, 0, sizeof(bp));
      bp.d_graph = e->d_graph; bp.entry_len = el; bp.dtype = (uint32_t)e->dtype; bp.D = D; bp.R = R; bp.n_nodes = N + n; bp.n_old = N; bp.n_targets = tn;
      bp.d_targets = d_targets + t0; bp.d_offs = d_offs + t0; bp.d_srcs = d_srcs;     // (the offsets stay absolute: d_srcs is the whole array)
      bp.d_cand_ids = d_cids; bp.d_cand_dists = d_cdists; bp.d_offered = d_offered; bp.d_own_out = d_own_out; bp.d_stats = d_ctl + 2; bp.d_abort = d_ctl + 1;
      BANG_TRY(bang_k_backedge(&bp, s));
      BANG_TRY(bang_k_range_sort(d_cids, d_cdists, d_offered, BANG_PRUNE_MAX_LIST, 0, tn, tn, d_count, s));
      bang_prune_params pp;
      memset(&pp, 0, sizeof(pp));
      pp.d_graph = e->d_graph; pp.entry_len = el; pp.dtype = (uint32_t)e->dtype; pp.D = D; pp.n_nodes = N + n; pp.R = R; pp.alpha2 = alpha2;
      pp.n_lists = tn; pp.list_stride = BANG_PRUNE_MAX_LIST; pp.d_list_ids = d_cids; pp.d_list_dists = d_cdists; pp.d_list_cnt = d_count;
      pp.d_own = d_own_out; pp.d_out = e->d_graph + vb; pp.out_stride = el; pp.out_by_own = 1; pp.d_abort = d_ctl + 1;
      BANG_TRY(bang_k_prune(&pp, s));
    }
  }
  HIP_TRY(hipEventRecord(sc.ev[1], s));
  // step 5: PQ codes at the engine's stride
  {
    float* d_lut = nullptr;
    const uint32_t EC = std::min(n, encode_chunk);
    BANG_TRY(sc.get(&d_lut, (size_t)EC * e->m * 256));
    BANG_TRY(bang_k_pq_encode(e->d_pivots_T, d_vecs, e->dtype, e->d_centroid, e->d_chunk_off, d_lut, EC, n, D, e->m,
                              e->d_codes + (uint64_t)N * e->code_stride, e->code_stride, s));
  }
  HIP_TRY(hipEventRecord(sc.ev[2], s));
  HIP_TRY(hipStreamSynchronize(s));
  BANG_TRY(sc.elapsed(0, 1, &ms[3]));                              // (the CSR upload is counted with the back-edges)
  BANG_TRY(sc.elapsed(1, 2, &ms[4]));
  BANG_TRY(check_abort(d_ctl + 1, "the back-edge step"));
  // step 6: the seed list (rebuilt from the medoid's row as it stands: the same words where the row did not change), the counters, N
  BANG_TRY(rebuild_seed(e));
  uint32_t st[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(st, d_ctl + 2, 12, hipMemcpyDeviceToHost));
  e->stat_inserted += n; e->stat_be_appended += st[0]; e->stat_be_pruned += st[1]; e->stat_be_dropped += st[2];
  e->N = N + n;
  e->insert_broken = false;
  ms[5] = ms_since(t_call);
  return BANG_OK;
}

}  // namespace

int bang::rebuild_seed(bang_engine* e) {
  const size_t vb = vec_bytes(e);
  std::vector<uint32_t> row(1 + e->R), seed(2 + BANG_MAX_R + 1, 0);
  HIP_TRY(hipMemcpy(row.data(), e->d_graph + e->medoid * e->entry_len + vb, row.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t deg = std::min(row[0], e->R);
  seed[0] = deg + 1;
  seed[1] = (uint32_t)e->medoid;
  memcpy(&seed[2], row.data() + 1, (size_t)deg * 4);
  HIP_TRY(hipMemcpy(e->d_seed, seed.data(), seed.size() * 4, hipMemcpyHostToDevice));
  return BANG_OK;
}

extern "C" int bang_insert_e(bang_engine_t* e, const void* h_vectors, uint32_t n, uint32_t L_build, float alpha, uint64_t* first_id) {
  if (!e) { bang_set_error("bang_insert: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("bang_insert: no index is loaded"); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("bang_insert: an allocation is live (call bang_free first): a batch may be reading the tables"); return BANG_ERR_ARG; }
  if (e->insert_broken) { bang_set_error("bang_insert: an earlier insert failed half-way and old rows may list ids beyond N: unload this engine (bang_unload) and load the index again"); return BANG_ERR_ARG; }
  if (e->capacity <= 0 || !e->d_graph) { bang_set_error("bang_insert: the index was loaded without option capacity: its tables hold no further node"); return BANG_ERR_ARG; }
  if (n == 0 || n > BANG_INSERT_MAX_BATCH) { bang_set_error("bang_insert: n = %u is outside [1, %u]", n, BANG_INSERT_MAX_BATCH); return BANG_ERR_ARG; }
  if ((uint64_t)e->N + n > (uint64_t)e->capacity) {
    bang_set_error("bang_insert: N + n = %llu exceeds capacity = %d", (unsigned long long)e->N + n, e->capacity);
    return BANG_ERR_ARG;
  }
  if (!h_vectors) { bang_set_error("bang_insert: h_vectors is null"); return BANG_ERR_ARG; }
  if (L_build < 1 || L_build > BANG_MAX_L) { bang_set_error("bang_insert: L_build = %u is outside [1, %d]", L_build, BANG_MAX_L); return BANG_ERR_ARG; }
  if (!std::isfinite(alpha) || alpha < 1.0f || alpha > 8.0f) { bang_set_error("bang_insert: alpha = %g is not finite or outside [1, 8]", (double)alpha); return BANG_ERR_ARG; }
  if (e->params_set && e->distfn == BANG_DIST_MIPS) { bang_set_error("bang_insert: MIPS search parameters are set: inserts run on L2 distances only"); return BANG_ERR_UNSUPPORTED; }
  if (!bang_search_can_rerank(e->dtype, e->D, e->entry_len, 0)) {
    bang_set_error("bang_insert: the vector layout (dtype %d, D = %u, entry stride %llu) is outside bang_search_can_rerank: 8-bit vectors need D %% 16 == 0 "
                   "with D / 16 a power of two, float vectors D %% 4 == 0; D <= 256", e->dtype, e->D, (unsigned long long)e->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->d_labels) { bang_set_error("bang_insert: a label table is set (labels cover exactly N nodes): clear it, insert, then set one for the new N"); return BANG_ERR_ARG; }
  if (e->dtype == BANG_F32) {
    uint64_t bad = 0;
    if (bang_check_floats((const float*)h_vectors, (uint64_t)n * e->D, &bad) != BANG_OK) {
      bang_set_error("bang_insert: vector %llu, dimension %llu holds %g: float vectors must be finite with |x| <= 2^56", (unsigned long long)(bad / e->D),
                     (unsigned long long)(bad % e->D), (double)((const float*)h_vectors)[bad]);
      return BANG_ERR_ARG;
    }
  }
  BANG_TRY(ensure_device(e));
  const float a32 = alpha;
  const float alpha2 = a32 * a32;
  const uint64_t first = e->N;
  const int rc = insert_batch(e, (const uint8_t*)h_vectors, n, L_build, alpha2);
  if (rc != BANG_OK) { (void)hipDeviceSynchronize(); return rc; }
  if (first_id) *first_id = first;
  return BANG_OK;
}

extern "C" int bang_get_entries_e(bang_engine_t* e, uint64_t first, uint64_t n, void* out) {
  if (!e) { bang_set_error("bang_get_entries: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded || !e->d_graph) { bang_set_error("bang_get_entries: no index with its graph in HBM is loaded"); return BANG_ERR_ARG; }
  if (first + n > (uint64_t)e->N || first + n < first) { bang_set_error("bang_get_entries: [%llu, %llu) leaves the index (N = %u)", (unsigned long long)first, (unsigned long long)(first + n), e->N); return BANG_ERR_ARG; }
  if (n == 0) return BANG_OK;
  if (!out) { bang_set_error("bang_get_entries: out is null"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  HIP_TRY(hipMemcpy(out, e->d_graph + first * e->entry_len, (size_t)(n * e->entry_len), hipMemcpyDeviceToHost));
  return BANG_OK;
}

extern "C" int bang_get_codes_e(bang_engine_t* e, uint64_t first, uint64_t n, void* out) {
  if (!e) { bang_set_error("bang_get_codes: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded || !e->d_codes) { bang_set_error("bang_get_codes: no index is loaded"); return BANG_ERR_ARG; }
  if (first + n > (uint64_t)e->N || first + n < first) { bang_set_error("bang_get_codes: [%llu, %llu) leaves the index (N = %u)", (unsigned long long)first, (unsigned long long)(first + n), e->N); return BANG_ERR_ARG; }
  if (n == 0) return BANG_OK;
  if (!out) { bang_set_error("bang_get_codes: out is null"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  HIP_TRY(hipMemcpy2D(out, e->m, e->d_codes + first * e->code_stride, e->code_stride, e->m, (size_t)n, hipMemcpyDeviceToHost));
  return BANG_OK;
}

extern "C" int bang_get_stats_ext5(bang_engine_t* e, bang_stats_ext5* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats_ext4(e, &out->ext4));
  out->capacity = e->capacity > 0 ? (uint64_t)e->capacity : 0;
  out->inserted = e->stat_inserted;
  out->backedge_appended = e->stat_be_appended;
  out->backedge_pruned = e->stat_be_pruned;
  out->backedge_dropped = e->stat_be_dropped;
  return BANG_OK;
}

extern "C" int bang_get_insert_times(bang_engine_t* e, double* ms6) {
  if (!e || !ms6) return BANG_ERR_ARG;
  memcpy(ms6, e->insert_ms, sizeof(e->insert_ms));
  return BANG_OK;
}
