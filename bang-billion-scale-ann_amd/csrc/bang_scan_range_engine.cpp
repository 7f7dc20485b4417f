// bang_scan_range_engine.cpp -- bang_scan_range_e: the exact range scan of a loaded index (DESIGN.md section 2 CANON 26, section 4.20).  As
// bang_scan_e it reads the engine's tables -- the graph entries in HBM or the packed vector table, the exclusion bitmap, the removed bitmap, the
// label table -- and writes none of them; its device temporaries live for the call.  Per chunk of <= 4096 queries, in stream order: the queries,
// radii (and filters) up, bang_k_scan_range (count, prefix, emit, sort), the hit rows and counts down; the rows are widened and padded on the host.
#include "bang_engine.h"

using namespace bang;

namespace {

constexpr uint32_t QUERY_CHUNK = 4096;      // queries per launch: 4096 x 4096 hits x 8 B = 128 MB of rows at the most

struct Scratch {                            // device temporaries of one call, freed on every way out
  std::vector<void*> ptrs;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Scratch() {
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  }
  template <typename T> int get(T** p, size_t count) {
    BANG_TRY(dmalloc(p, count));
    ptrs.push_back((void*)*p);
    return BANG_OK;
  }
};

int scan_range(bang_engine* e, const uint8_t* vec_base, uint64_t vec_stride, const void* h_queries, uint32_t nq, const float* h_radii, uint32_t H,
               const uint32_t* any, const uint32_t* all, uint64_t* ids_out, float* dists_out, uint32_t* count_out, uint32_t* offered_out,
               uint32_t* matched_out) {
  const Clock::time_point t_call = Clock::now();
  const size_t qbytes = vec_bytes(e);
  hipStream_t s = nullptr;
  Scratch sc;
  const uint32_t chunk = (uint32_t)std::min((long)QUERY_CHUNK, std::max(1L, env_long("BANG_SCAN_QUERY_CHUNK", QUERY_CHUNK)));   // test hook, clamped
  const uint32_t QC = std::min(nq, chunk);
  uint32_t tiles = 0, runs = 0, most = 0;
  if (bang_scan_range_geometry(e->dtype, e->D, QC, e->N, &tiles, &runs, &most) != BANG_OK) { bang_set_error("bang_scan_range: no launch geometry"); return BANG_ERR_ARG; }
  const long want = env_long("BANG_SCAN_RANGE_RUNS", 0);                   // test hook, clamped
  if (want > 0) runs = (uint32_t)std::min<long>(want, most);
  const uint64_t scratch_bytes = bang_scan_range_scratch_bytes(QC, runs);
  uint8_t *d_q = nullptr, *d_scratch = nullptr;
  float *d_rad = nullptr, *d_dists = nullptr;
  uint32_t *d_flt = nullptr, *d_ids = nullptr, *d_words = nullptr;         // d_words: offered | count | matched, [3][QC]
  BANG_TRY(sc.get(&d_q, (size_t)QC * qbytes));
  BANG_TRY(sc.get(&d_rad, QC));
  BANG_TRY(sc.get(&d_scratch, (size_t)scratch_bytes));
  BANG_TRY(sc.get(&d_ids, (size_t)QC * H));
  BANG_TRY(sc.get(&d_dists, (size_t)QC * H));
  BANG_TRY(sc.get(&d_words, (size_t)QC * 3));
  if (any) BANG_TRY(sc.get(&d_flt, (size_t)QC * 2));
  for (hipEvent_t& x : sc.ev) HIP_TRY(hipEventCreate(&x));
  std::vector<uint32_t> flt, h_ids((size_t)QC * H), h_words((size_t)QC * 3);
  double ms[3] = {0, 0, 0};
  for (uint32_t q0 = 0; q0 < nq; q0 += QC) {
    const uint32_t n = std::min(QC, nq - q0);
    HIP_TRY(hipMemcpyAsync(d_q, (const uint8_t*)h_queries + (size_t)q0 * qbytes, (size_t)n * qbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rad, h_radii + q0, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (any) {
      flt.resize((size_t)n * 2);
      for (uint32_t i = 0; i < n; ++i) { flt[2 * (size_t)i] = any[q0 + i]; flt[2 * (size_t)i + 1] = all[q0 + i]; }
      HIP_TRY(hipMemcpyAsync(d_flt, flt.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    bang_scan_range_params p;
    memset(&p, 0, sizeof(p));
    p.d_vec_base = vec_base; p.vec_stride = vec_stride; p.dtype = (uint32_t)e->dtype; p.D = e->D; p.n_nodes = e->N;
    p.d_queries = d_q; p.nq = n; p.d_radius = d_rad;
    p.d_excluded = (e->n_excl != 0 && e->d_excl) ? e->d_excl : nullptr;
    p.d_removed = e->d_removed;
    p.d_labels = any ? e->d_labels : nullptr; p.d_filters = any ? d_flt : nullptr;
    p.max_hits = H; p.runs = runs; p.d_scratch = d_scratch; p.scratch_bytes = scratch_bytes;
    p.d_hit_ids = d_ids; p.d_hit_dists = d_dists; p.d_offered = d_words; p.d_count = d_words + QC; p.d_matched = d_words + 2 * (size_t)QC;
    HIP_TRY(hipEventRecord(sc.ev[0], s));
    BANG_TRY(bang_k_scan_range_marked(&p, s, sc.ev[1], sc.ev[2]));
    HIP_TRY(hipEventRecord(sc.ev[3], s));
    // the rows of this chunk: the distances are the caller's rows as they are, the ids are widened below
    HIP_TRY(hipMemcpyAsync(h_words.data(), d_words, (size_t)QC * 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_ids.data(), d_ids, (size_t)n * H * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(dists_out + (size_t)q0 * H, d_dists, (size_t)n * H * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t c = h_words[(size_t)QC + i];
      uint64_t* ids = ids_out + (size_t)(q0 + i) * H;
      float* dists = dists_out + (size_t)(q0 + i) * H;
      const uint32_t* src = h_ids.data() + (size_t)i * H;
      for (uint32_t j = 0; j < c; ++j) ids[j] = src[j];
      for (uint32_t j = c; j < H; ++j) { ids[j] = UINT64_MAX; dists[j] = 3.402823E+38f; }
      offered_out[q0 + i] = h_words[i];
      count_out[q0 + i] = c;
      if (matched_out) matched_out[q0 + i] = h_words[2 * (size_t)QC + i];
    }
    for (int k = 0; k < 3; ++k) {
      float x = 0;
      HIP_TRY(hipEventElapsedTime(&x, sc.ev[k], sc.ev[k + 1]));
      ms[k] += x;
    }
  }
  e->scan_range_ms[0] = ms[0]; e->scan_range_ms[1] = ms[1];
  e->scan_ms[0] = ms[0] + ms[1]; e->scan_ms[1] = ms[2]; e->scan_ms[2] = ms_since(t_call);
  return BANG_OK;
}

}  // namespace

extern "C" int bang_scan_range_e(bang_engine_t* e, const void* h_queries, uint32_t nq, const float* h_radii, uint32_t max_hits, const uint32_t* any,
                                 const uint32_t* all, uint64_t* ids_out, float* dists_out, uint32_t* count_out, uint32_t* offered_out,
                                 uint32_t* matched_out) {
  if (!e) { bang_set_error("bang_scan_range: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("bang_scan_range: no index is loaded"); return BANG_ERR_ARG; }
  if (!h_queries) { bang_set_error("bang_scan_range: the queries are null"); return BANG_ERR_ARG; }
  if (!h_radii) { bang_set_error("bang_scan_range: the radii are null"); return BANG_ERR_ARG; }
  if (!ids_out || !dists_out || !count_out || !offered_out) { bang_set_error("bang_scan_range: an output buffer (ids, dists, count, offered) is null"); return BANG_ERR_ARG; }
  if (nq == 0 || nq > BANG_SCAN_MAX_QUERIES) { bang_set_error("bang_scan_range: nq = %u is outside [1, %u]", nq, BANG_SCAN_MAX_QUERIES); return BANG_ERR_ARG; }
  if (max_hits == 0 || max_hits > BANG_RANGE_MAX_HITS) { bang_set_error("bang_scan_range: max_hits = %u is outside [1, %u]", max_hits, BANG_RANGE_MAX_HITS); return BANG_ERR_ARG; }
  if ((uint64_t)nq * max_hits > BANG_SCAN_RANGE_MAX_OUT) {
    bang_set_error("bang_scan_range: nq x max_hits = %llu exceeds %u result slots per call", (unsigned long long)nq * max_hits, BANG_SCAN_RANGE_MAX_OUT);
    return BANG_ERR_ARG;
  }
  if ((any == nullptr) != (all == nullptr)) { bang_set_error("bang_scan_range: exactly one of any / all is given: a filter batch is both arrays, or neither"); return BANG_ERR_ARG; }
  if (any && !e->d_labels) { bang_set_error("bang_scan_range: filters without labels: the index has no label table (bang_set_labels_e)"); return BANG_ERR_ARG; }
  if (e->params_set && e->distfn != BANG_DIST_L2) {
    bang_set_error("bang_scan_range: %s search parameters are set: the range scan runs on L2 distances only", e->distfn == BANG_DIST_MIPS ? "MIPS" : "non-L2");
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->vecs_f16) { bang_set_error("bang_scan_range: the vector table holds fp16 rows (option vectors_fp16): their distances are not the exact ones"); return BANG_ERR_UNSUPPORTED; }
  const uint8_t* vec_base = e->d_graph ? e->d_graph : e->d_vecs;
  const uint64_t vec_stride = e->d_graph ? e->entry_len : (uint64_t)vec_bytes(e);
  if (!vec_base) { bang_set_error("bang_scan_range: no resident vectors: the graph is in host RAM and the vectors were left there (option vectors = 0)"); return BANG_ERR_UNSUPPORTED; }
  if (e->D == 0u || e->D > BANG_SCAN_ANY_MAX_D) { bang_set_error("bang_scan_range: D = %u exceeds %u, the widest vector the range scan serves", e->D, BANG_SCAN_ANY_MAX_D); return BANG_ERR_UNSUPPORTED; }
  if (e->dtype != BANG_F32 && (e->D & 3u) != 0u) { bang_set_error("bang_scan_range: D = %u: 8-bit vectors need D %% 4 == 0", e->D); return BANG_ERR_UNSUPPORTED; }
  if ((vec_stride & 3u) != 0 || vec_stride < (uint64_t)vec_bytes(e)) {
    bang_set_error("bang_scan_range: the vector stride %llu is not a multiple of 4 that holds the vector (dtype %d, D = %u)", (unsigned long long)vec_stride, e->dtype, e->D);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->dtype == BANG_F32) {
    uint64_t bad = 0;
    if (bang_check_floats((const float*)h_queries, (uint64_t)nq * e->D, &bad) != BANG_OK) {
      bang_set_error("bang_scan_range: query %llu, dimension %llu holds %g: float queries must be finite with |x| <= 2^56 (nothing was launched)",
                     (unsigned long long)(bad / e->D), (unsigned long long)(bad % e->D), (double)((const float*)h_queries)[bad]);
      return BANG_ERR_ARG;
    }
  }
  BANG_TRY(ensure_device(e));
  for (double& x : e->scan_ms) x = 0;
  for (double& x : e->scan_range_ms) x = 0;
  const int rc = scan_range(e, vec_base, vec_stride, h_queries, nq, h_radii, max_hits, any, all, ids_out, dists_out, count_out, offered_out, matched_out);
  if (rc != BANG_OK) (void)hipDeviceSynchronize();
  return rc;
}

extern "C" int bang_get_scan_range_times(bang_engine_t* e, double* ms2) {
  if (!e || !ms2) return BANG_ERR_ARG;
  memcpy(ms2, e->scan_range_ms, sizeof(e->scan_range_ms));
  return BANG_OK;
}
