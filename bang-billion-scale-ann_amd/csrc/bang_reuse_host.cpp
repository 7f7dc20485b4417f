// bang_reuse_host.cpp -- bang_insert_reuse_e: an insert whose points take the ids of removed nodes first (DESIGN.md section 2 CANON 24, section
// 4.18), and the calls that hand the free set out and take it back (bang_get_free_slots_e, bang_get_removed_e, bang_set_removed_e).  A sibling
// of insert_batch (bang_insert_host.cpp), which keeps its own code path: the same launches with d_own = ids, and a row copy by id wherever that one
// relies on the new slots lying side by side.  Launches, in stream order:
//   bang_k_bitmap_select (E = removed & ~excluded, the lowest n), bang_reuse_assign (no HIP call), the entries up, bang_k_copy_rows_by_id (to the slots)
//   per chunk of <= 1024 points: bang_k_search_exact (rr_k = L, n_nodes = N) -> bang_k_worklist_lists -> bang_k_prune (rows into the slots)
//   bang_k_copy_rows_by_id (the new rows, packed), down, bang_insert_group_ids (no HIP call), the CSR up
//   per chunk of <= 8192 targets: bang_k_backedge -> bang_k_range_sort -> bang_k_prune
//   bang_k_pq_encode into a staging table at the engine's code stride, bang_k_copy_rows_by_id (to the slots)
//   the seed list, bang_k_bitmap_clear_ids (the re-used slots leave the removed bitmap), N
#include "bang_engine.h"

#include <cmath>

using namespace bang;

namespace {

constexpr uint32_t SEARCH_CHUNK = 1024;     // the chunk sizes and test hooks of bang_insert_e
constexpr uint32_t TARGET_CHUNK = 8192;
constexpr uint32_t ENCODE_CHUNK = 256;

uint32_t chunk_of(long asked, uint32_t dflt) { return (uint32_t)std::min((long)dflt, std::max(1L, asked)); }

// device temporaries of one call, freed on every way out
struct Scratch {
  std::vector<void*> ptrs;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Scratch() {
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  }
  int elapsed(int a, int b, double* ms) {
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
  if (ab != 0) { bang_set_error("bang_insert_reuse: %s met a node id outside the index (abort code %u): corrupt adjacency row", where, ab); return BANG_ERR_IO; }
  return BANG_OK;
}

size_t bitmap_nodes(const bang_engine* e) { return std::max<size_t>(e->N, e->capacity > 0 ? (size_t)e->capacity : 0); }
const uint32_t* excl_of(const bang_engine* e) { return (e->n_excl != 0 && e->d_excl) ? e->d_excl : nullptr; }

// the lowest `want` ids of d_a & ~d_not below N into h_ids (want may be 0), their number in all into *total
int select_ids(bang_engine* e, const uint32_t* d_a, const uint32_t* d_not, uint32_t want, std::vector<uint32_t>* h_ids, uint32_t* total) {
  *total = 0;
  if (h_ids) h_ids->clear();
  if (!d_a) return BANG_OK;
  Scratch sc;
  uint32_t *d_ids = nullptr, *d_total = nullptr, *d_scr = nullptr;
  BANG_TRY(sc.get(&d_ids, std::max<size_t>(want, 1)));
  BANG_TRY(sc.get(&d_total, 1));
  BANG_TRY(sc.get(&d_scr, (size_t)bang_bitmap_select_scratch_words(e->N)));
  BANG_TRY(bang_k_bitmap_select(d_a, d_not, e->N, want, d_ids, d_total, d_scr, nullptr));
  HIP_TRY(hipMemcpy(total, d_total, 4, hipMemcpyDeviceToHost));
  const uint32_t k = std::min(want, *total);
  if (h_ids && k != 0) {
    h_ids->resize(k);
    HIP_TRY(hipMemcpy(h_ids->data(), d_ids, (size_t)k * 4, hipMemcpyDeviceToHost));
  }
  return BANG_OK;
}

int reuse_batch(bang_engine* e, const uint8_t* h_vectors, uint32_t n, uint32_t L, float alpha2, uint64_t* ids_out) {
  const uint32_t N = e->N, R = e->R, D = e->D;
  const size_t vb = vec_bytes(e);
  const uint64_t el = e->entry_len;
  hipStream_t s = nullptr;
  Scratch sc;
  const Clock::time_point t_call = Clock::now();
  // E and the ids of the batch; the one refusal that needs the bitmaps
  std::vector<uint32_t> free_ids, own(n);
  uint32_t n_eligible = 0, appended = 0;
  BANG_TRY(select_ids(e, e->d_removed, excl_of(e), n, &free_ids, &n_eligible));
  if (bang_reuse_assign(free_ids.data(), (uint32_t)free_ids.size(), n, N, own.data(), &appended) != BANG_OK) {
    bang_set_error("bang_insert_reuse: the free slots came back unordered or outside the index");
    return BANG_ERR_IO;
  }
  const uint32_t f = n - appended, N2 = N + appended;
  if ((uint64_t)N + appended > (uint64_t)e->capacity) {
    bang_set_error("bang_insert_reuse: N + (n - f) = %llu exceeds capacity = %d (f = %u free slots are eligible)", (unsigned long long)N + appended, e->capacity, f);
    return BANG_ERR_ARG;
  }
  const uint32_t search_chunk = chunk_of(env_long("BANG_INSERT_SEARCH_CHUNK", SEARCH_CHUNK), SEARCH_CHUNK);
  const uint32_t target_chunk = chunk_of(env_long("BANG_INSERT_TARGET_CHUNK", TARGET_CHUNK), TARGET_CHUNK);
  const uint32_t encode_chunk = chunk_of(env_long("BANG_INSERT_ENCODE_CHUNK", ENCODE_CHUNK), ENCODE_CHUNK);
  const uint32_t QC = std::min(n, search_chunk);
  const uint32_t rs = R + 1;
  uint8_t *d_vecs = nullptr, *d_ent = nullptr;
  uint32_t *d_bloom = nullptr, *d_cand_ids = nullptr, *d_cand_cnt = nullptr, *d_ctl = nullptr, *d_list_ids = nullptr, *d_list_cnt = nullptr, *d_own = nullptr, *d_rows = nullptr;
  uint64_t* d_wl_ids = nullptr;
  float *d_wl_dists = nullptr, *d_list_dists = nullptr;
  BANG_TRY(sc.get(&d_vecs, (size_t)n * vb + 256));
  BANG_TRY(sc.get(&d_ent, (size_t)n * el));
  BANG_TRY(sc.get(&d_rows, (size_t)n * rs));
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
  double* ms = e->insert_ms;                                      // {search, prune, select + entries + rows down + host grouping, back-edges, encode + code rows, whole call}
  for (int i = 0; i < 6; ++i) ms[i] = 0;
  HIP_TRY(hipMemcpy(d_vecs, h_vectors, (size_t)n * vb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_ctl, 0, 32));
  HIP_TRY(hipMemcpy(d_own, own.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  // step 3, first half: the new entries with their vectors and empty rows at their slots.  A re-used slot is a node of F: no row of a live node
  // lists it and the search below (n_nodes = N) starts at the medoid, which is never in F -- nothing reads the slot before the call ends
  {
    std::vector<uint8_t> ent((size_t)n * el, 0);
    for (uint32_t i = 0; i < n; ++i) memcpy(ent.data() + (size_t)i * el, h_vectors + (size_t)i * vb, vb);
    HIP_TRY(hipMemcpy(d_ent, ent.data(), ent.size(), hipMemcpyHostToDevice));
    BANG_TRY(bang_k_copy_rows_by_id(e->d_graph, el, 0, d_own, n, N2, d_ent, el, (uint32_t)el, 1, d_ctl + 1, s));
    HIP_TRY(hipStreamSynchronize(s));
    BANG_TRY(check_abort(d_ctl + 1, "the upload of the entries"));
  }
  ms[2] = ms_since(t_call);
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
    pp.n_nodes = N2;                                               // (own ids name rows inside the table; list ids are < N)
    BANG_TRY(bang_k_prune(&pp, s));
    HIP_TRY(hipEventRecord(sc.ev[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    BANG_TRY(sc.elapsed(0, 1, &ms[0]));
    BANG_TRY(sc.elapsed(1, 2, &ms[1]));
    BANG_TRY(check_abort(d_ctl + 1, "the candidate search"));
  }
  // step 4: back-edges.  The new rows are gathered from their slots, come back once, are grouped on the host, and the CSR goes up
  const Clock::time_point t_group = Clock::now();
  std::vector<uint32_t> rows((size_t)n * rs);
  BANG_TRY(bang_k_copy_rows_by_id(e->d_graph, el, vb, d_own, n, N2, d_rows, (uint64_t)rs * 4, rs * 4, 0, d_ctl + 1, s));
  HIP_TRY(hipMemcpy(rows.data(), d_rows, rows.size() * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> targets((size_t)n * R), offs((size_t)n * R + 1), srcs((size_t)n * R);
  uint32_t nt = 0;
  if (bang_insert_group_ids(rows.data(), n, rs, own.data(), N, targets.data(), offs.data(), srcs.data(), &nt) != BANG_OK) {
    bang_set_error("bang_insert_reuse: a new row lists an id outside the old index or a slot of this batch: a free slot was reachable");
    return BANG_ERR_IO;
  }
  ms[2] += ms_since(t_group);
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
    // from here on old rows change: a failure before the end leaves rows that list slots still marked free or ids >= N (bang_insert_e's latch)
    e->insert_broken = true;
    for (uint32_t t0 = 0; t0 < nt; t0 += TC) {
      const uint32_t tn = std::min(TC, nt - t0);
      bang_backedge_params bp;
      memset(&bp, 0, sizeof(bp));
      bp.d_graph = e->d_graph; bp.entry_len = el; bp.dtype = (uint32_t)e->dtype; bp.D = D; bp.R = R; bp.n_nodes = N2; bp.n_old = N; bp.n_targets = tn;
      bp.d_targets = d_targets + t0; bp.d_offs = d_offs + t0; bp.d_srcs = d_srcs;
      bp.d_cand_ids = d_cids; bp.d_cand_dists = d_cdists; bp.d_offered = d_offered; bp.d_own_out = d_own_out; bp.d_stats = d_ctl + 2; bp.d_abort = d_ctl + 1;
      BANG_TRY(bang_k_backedge(&bp, s));
      BANG_TRY(bang_k_range_sort(d_cids, d_cdists, d_offered, BANG_PRUNE_MAX_LIST, 0, tn, tn, d_count, s));
      bang_prune_params pp;
      memset(&pp, 0, sizeof(pp));
      pp.d_graph = e->d_graph; pp.entry_len = el; pp.dtype = (uint32_t)e->dtype; pp.D = D; pp.n_nodes = N2; pp.R = R; pp.alpha2 = alpha2;
      pp.n_lists = tn; pp.list_stride = BANG_PRUNE_MAX_LIST; pp.d_list_ids = d_cids; pp.d_list_dists = d_cdists; pp.d_list_cnt = d_count;
      pp.d_own = d_own_out; pp.d_out = e->d_graph + vb; pp.out_stride = el; pp.out_by_own = 1; pp.d_abort = d_ctl + 1;
      BANG_TRY(bang_k_prune(&pp, s));
    }
  }
  HIP_TRY(hipEventRecord(sc.ev[1], s));
  // step 5: PQ codes, encoded side by side at the engine's stride (bytes behind m zero, as bang_insert_e leaves them) and copied to their slots
  {
    float* d_lut = nullptr;
    uint8_t* d_stage = nullptr;
    const uint32_t EC = std::min(n, encode_chunk);
    BANG_TRY(sc.get(&d_lut, (size_t)EC * e->m * 256));
    BANG_TRY(sc.get(&d_stage, (size_t)n * e->code_stride + 16));
    BANG_TRY(bang_k_pq_encode(e->d_pivots_T, d_vecs, e->dtype, e->d_centroid, e->d_chunk_off, d_lut, EC, n, D, e->m, d_stage, e->code_stride, s));
    BANG_TRY(bang_k_copy_rows_by_id(e->d_codes, e->code_stride, 0, d_own, n, N2, d_stage, e->code_stride, e->code_stride, 1, d_ctl + 1, s));
  }
  HIP_TRY(hipEventRecord(sc.ev[2], s));
  HIP_TRY(hipStreamSynchronize(s));
  BANG_TRY(sc.elapsed(0, 1, &ms[3]));
  BANG_TRY(sc.elapsed(1, 2, &ms[4]));
  BANG_TRY(check_abort(d_ctl + 1, "the back-edge step"));
  // step 6: the seed list, the removed bits of the re-used slots, the counters, N
  BANG_TRY(rebuild_seed(e));
  if (f != 0) {
    BANG_TRY(bang_k_bitmap_clear_ids(e->d_removed, N, d_own, f, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  uint32_t st[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(st, d_ctl + 2, 12, hipMemcpyDeviceToHost));
  e->stat_inserted += n; e->stat_be_appended += st[0]; e->stat_be_pruned += st[1]; e->stat_be_dropped += st[2];
  e->stat_reused += f;
  e->N = N2;
  e->insert_broken = false;
  for (uint32_t i = 0; i < n; ++i) ids_out[i] = own[i];
  ms[5] = ms_since(t_call);
  return BANG_OK;
}

// what bang_get_removed_e / bang_set_removed_e / bang_get_free_slots_e ask of the engine
int mutable_engine(bang_engine* e, const char* what, bool need_free) {
  if (!e) { bang_set_error("%s: the engine is null", what); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("%s: no index is loaded", what); return BANG_ERR_ARG; }
  if (need_free && e->allocated) { bang_set_error("%s: an allocation is live (call bang_free first): a batch may be reading the tables", what); return BANG_ERR_ARG; }
  if (!e->d_graph) { bang_set_error("%s: the graph is not in HBM (graph = device)", what); return BANG_ERR_ARG; }
  return BANG_OK;
}

}  // namespace

extern "C" int bang_insert_reuse_e(bang_engine_t* e, const void* h_vectors, uint32_t n, uint32_t L_build, float alpha, uint64_t* ids_out) {
  if (!e) { bang_set_error("bang_insert_reuse: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("bang_insert_reuse: no index is loaded"); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("bang_insert_reuse: an allocation is live (call bang_free first): a batch may be reading the tables"); return BANG_ERR_ARG; }
  if (e->insert_broken) { bang_set_error("bang_insert_reuse: an earlier insert failed half-way and old rows may list ids beyond N or free slots: unload this engine (bang_unload) and load the index again"); return BANG_ERR_ARG; }
  if (e->capacity <= 0 || !e->d_graph) { bang_set_error("bang_insert_reuse: the index was loaded without option capacity: only an engine whose tables may change (graph = device, capacity >= N) inserts"); return BANG_ERR_ARG; }
  if (n == 0 || n > BANG_INSERT_MAX_BATCH) { bang_set_error("bang_insert_reuse: n = %u is outside [1, %u]", n, BANG_INSERT_MAX_BATCH); return BANG_ERR_ARG; }
  if (!h_vectors) { bang_set_error("bang_insert_reuse: h_vectors is null"); return BANG_ERR_ARG; }
  if (!ids_out) { bang_set_error("bang_insert_reuse: ids_out is null"); return BANG_ERR_ARG; }
  if (L_build < 1 || L_build > BANG_MAX_L) { bang_set_error("bang_insert_reuse: L_build = %u is outside [1, %d]", L_build, BANG_MAX_L); return BANG_ERR_ARG; }
  if (!std::isfinite(alpha) || alpha < 1.0f || alpha > 8.0f) { bang_set_error("bang_insert_reuse: alpha = %g is not finite or outside [1, 8]", (double)alpha); return BANG_ERR_ARG; }
  if (e->params_set && e->distfn == BANG_DIST_MIPS) { bang_set_error("bang_insert_reuse: MIPS search parameters are set: inserts run on L2 distances only"); return BANG_ERR_UNSUPPORTED; }
  if (!bang_search_can_rerank(e->dtype, e->D, e->entry_len, 0)) {
    bang_set_error("bang_insert_reuse: the vector layout (dtype %d, D = %u, entry stride %llu) is outside bang_search_can_rerank: 8-bit vectors need D %% 16 == 0 "
                   "with D / 16 a power of two, float vectors D %% 4 == 0; D <= 256", e->dtype, e->D, (unsigned long long)e->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->d_labels) { bang_set_error("bang_insert_reuse: a label table is set (labels cover exactly N nodes and name the removed ones): clear it, insert, then set one for the new index"); return BANG_ERR_ARG; }
  if (e->dtype == BANG_F32) {
    uint64_t bad = 0;
    if (bang_check_floats((const float*)h_vectors, (uint64_t)n * e->D, &bad) != BANG_OK) {
      bang_set_error("bang_insert_reuse: vector %llu, dimension %llu holds %g: float vectors must be finite with |x| <= 2^56", (unsigned long long)(bad / e->D),
                     (unsigned long long)(bad % e->D), (double)((const float*)h_vectors)[bad]);
      return BANG_ERR_ARG;
    }
  }
  BANG_TRY(ensure_device(e));
  const float a32 = alpha;
  const float alpha2 = a32 * a32;
  const int rc = reuse_batch(e, (const uint8_t*)h_vectors, n, L_build, alpha2, ids_out);
  if (rc != BANG_OK) { (void)hipDeviceSynchronize(); return rc; }
  return BANG_OK;
}

extern "C" int bang_get_free_slots_e(bang_engine_t* e, uint64_t* out3) {
  BANG_TRY(mutable_engine(e, "bang_get_free_slots", false));
  if (!out3) { bang_set_error("bang_get_free_slots: out3 is null"); return BANG_ERR_ARG; }
  out3[0] = out3[1] = 0;
  out3[2] = e->stat_reused;
  if (!e->d_removed) return BANG_OK;
  BANG_TRY(ensure_device(e));
  uint32_t all = 0, eligible = 0;
  BANG_TRY(select_ids(e, e->d_removed, nullptr, 0, nullptr, &all));
  BANG_TRY(select_ids(e, e->d_removed, excl_of(e), 0, nullptr, &eligible));
  out3[0] = all; out3[1] = eligible;
  return BANG_OK;
}

extern "C" int bang_get_removed_e(bang_engine_t* e, uint32_t* ids_out, uint64_t cap, uint64_t* count) {
  BANG_TRY(mutable_engine(e, "bang_get_removed", false));
  if (!count) { bang_set_error("bang_get_removed: count is null"); return BANG_ERR_ARG; }
  *count = 0;
  if (!e->d_removed) return BANG_OK;
  BANG_TRY(ensure_device(e));
  uint32_t total = 0;
  BANG_TRY(select_ids(e, e->d_removed, nullptr, 0, nullptr, &total));
  *count = total;
  if (!ids_out || total == 0) return BANG_OK;
  if (cap < total) { bang_set_error("bang_get_removed: ids_out holds %llu ids, %u are removed", (unsigned long long)cap, total); return BANG_ERR_ARG; }
  std::vector<uint32_t> ids;
  BANG_TRY(select_ids(e, e->d_removed, nullptr, total, &ids, &total));
  memcpy(ids_out, ids.data(), ids.size() * 4);
  return BANG_OK;
}

extern "C" int bang_set_removed_e(bang_engine_t* e, const uint32_t* ids, uint64_t n) {
  BANG_TRY(mutable_engine(e, "bang_set_removed", true));
  if (e->insert_broken) { bang_set_error("bang_set_removed: an earlier insert failed half-way: unload this engine (bang_unload) and load the index again"); return BANG_ERR_ARG; }
  if (n != 0 && !ids) { bang_set_error("bang_set_removed: ids is null"); return BANG_ERR_ARG; }
  if (n >= 0xFFFFFFFFull) { bang_set_error("bang_set_removed: n = %llu ids: more than node ids exist", (unsigned long long)n); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  if (n == 0) { dfree(e->d_removed); return BANG_OK; }
  if (!bang_search_can_rerank(e->dtype, e->D, e->entry_len, 0) || e->R > BANG_MAX_R) {
    bang_set_error("bang_set_removed: the vector layout (dtype %d, D = %u, entry stride %llu) is outside bang_search_can_rerank: the rows cannot be scanned", e->dtype, e->D, (unsigned long long)e->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  const uint32_t N = e->N, med = (uint32_t)e->medoid;
  const size_t vb = vec_bytes(e);
  const size_t words = (bitmap_nodes(e) + 31) / 32 + 1;              // the shape of the exclusion bitmap
  Scratch sc;
  hipStream_t s = nullptr;
  uint32_t *d_ids = nullptr, *d_ctl = nullptr, *d_aff = nullptr, *d_scr = nullptr, *d_new = nullptr;
  BANG_TRY(sc.get(&d_ids, (size_t)n));
  BANG_TRY(sc.get(&d_ctl, 8));                                      // [0] first offending list position, [1] abort word, [2] offenders of the scan, [3] the first of them
  BANG_TRY(sc.get(&d_aff, words));
  BANG_TRY(sc.get(&d_scr, (size_t)bang_bitmap_select_scratch_words(N)));
  BANG_TRY(dmalloc(&d_new, words));                                 // becomes the engine's bitmap, or is freed below
  struct Guard { uint32_t*& p; ~Guard() { dfree(p); } } guard{d_new};
  const uint32_t init[4] = {0xFFFFFFFFu, 0u, 0u, 0u};
  HIP_TRY(hipMemcpy(d_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ctl, init, 16, hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(d_aff, 0, words * 4, s));
  HIP_TRY(hipMemsetAsync(d_new, 0, words * 4, s));
  // every id a node, not the medoid, its row empty
  BANG_TRY(bang_k_rows_check(e->d_graph, e->entry_len, vb, d_ids, n, N, med, d_ctl, s));
  uint32_t first = 0;
  HIP_TRY(hipMemcpy(&first, d_ctl, 4, hipMemcpyDeviceToHost));
  if (first != 0xFFFFFFFFu) {
    const uint32_t id = ids[first];
    if (id >= N) bang_set_error("bang_set_removed: id %u (entry %u of the list) is out of range: the index has N = %u nodes", id, first, N);
    else if (id == med) bang_set_error("bang_set_removed: id %u (entry %u of the list) is the medoid, which is never removed", id, first);
    else bang_set_error("bang_set_removed: id %u (entry %u of the list) has a row that is not empty: it was not removed by a consolidation", id, first);
    return BANG_ERR_ARG;
  }
  // no row of a node outside the list names a listed id: the consolidation's scan with the candidates as its set never flags a listed node, so
  // every bit of its affected bitmap is an offender
  BANG_TRY(bang_k_bitmap_set_ids(d_new, N, d_ids, n, s));
  bang_consolidate_scan_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.d_graph = e->d_graph; sp.entry_len = e->entry_len; sp.dtype = (uint32_t)e->dtype; sp.D = e->D; sp.R = e->R; sp.n_nodes = N; sp.medoid = med;
  sp.d_excluded = d_new; sp.d_affected = d_aff; sp.d_abort = d_ctl + 1;
  BANG_TRY(bang_k_consolidate_scan(&sp, s));
  BANG_TRY(bang_k_bitmap_select(d_aff, nullptr, N, 1, d_ctl + 3, d_ctl + 2, d_scr, s));
  uint32_t res[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(res, d_ctl, 16, hipMemcpyDeviceToHost));
  if (res[1] != 0) { bang_set_error("bang_set_removed: the scan of the rows met a node id outside the index (abort code %u): corrupt adjacency row", res[1]); return BANG_ERR_IO; }
  if (res[2] != 0) {
    bang_set_error("bang_set_removed: the row of node %u, which is not in the list, names a listed id (%u such rows): the listed nodes are not all removed", res[3], res[2]);
    return BANG_ERR_ARG;
  }
  std::swap(e->d_removed, d_new);                                    // (the guard frees the old bitmap)
  return BANG_OK;
}
