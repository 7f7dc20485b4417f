// bang_scan_engine.cpp -- bang_scan_e: the exact scan of a loaded index (DESIGN.md section 2 CANON 23, section 4.17).  It reads the engine's tables
// -- the graph entries in HBM or the packed vector table, the exclusion bitmap, the removed bitmap, the label table -- and writes none of them; its
// device temporaries live for the call.  Per chunk of <= 4096 queries, in stream order: the queries (and filters) up, bang_k_scan (the scan launch,
// bang_k_range_sort over the stripes' lists, the output kernel), the results down.
#include "bang_engine.h"

using namespace bang;

namespace {

constexpr uint32_t QUERY_CHUNK = 4096;      // queries per launch: 4096 x 4096 keys x 8 B = 128 MB of lists at the most

struct Scratch {                            // device temporaries of one call, freed on every way out
  std::vector<void*> ptrs;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
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

int scan(bang_engine* e, const uint8_t* vec_base, uint64_t vec_stride, const void* h_queries, uint32_t nq, uint32_t k, const uint32_t* any,
         const uint32_t* all, uint64_t* ids_out, float* dists_out, uint32_t* matched_out) {
  const Clock::time_point t_call = Clock::now();
  const size_t qbytes = vec_bytes(e);
  hipStream_t s = nullptr;
  Scratch sc;
  const uint32_t chunk = (uint32_t)std::min((long)QUERY_CHUNK, std::max(1L, env_long("BANG_SCAN_QUERY_CHUNK", QUERY_CHUNK)));   // test hook, clamped
  const uint32_t QC = std::min(nq, chunk);
  uint32_t tiles = 0, stripes = 0;
  if (bang_scan_geometry(e->dtype, e->D, QC, e->N, k, &tiles, &stripes) != BANG_OK) { bang_set_error("bang_scan: no launch geometry"); return BANG_ERR_ARG; }
  const long want = env_long("BANG_SCAN_STRIPES", 0);                      // test hook, clamped
  if (want > 0) stripes = (uint32_t)std::min<long>(want, std::max<uint32_t>(1u, bang_scan_max_stripes(e->dtype, e->N, k)));
  const uint64_t scratch_bytes = bang_scan_scratch_bytes(QC, k, stripes);
  uint8_t *d_q = nullptr, *d_scratch = nullptr;
  uint32_t *d_flt = nullptr, *d_matched = nullptr;
  uint64_t* d_ids = nullptr;
  float* d_dists = nullptr;
  BANG_TRY(sc.get(&d_q, (size_t)QC * qbytes));
  BANG_TRY(sc.get(&d_scratch, (size_t)scratch_bytes));
  BANG_TRY(sc.get(&d_ids, (size_t)QC * k));
  BANG_TRY(sc.get(&d_dists, (size_t)QC * k));
  BANG_TRY(sc.get(&d_matched, QC));
  if (any) BANG_TRY(sc.get(&d_flt, (size_t)QC * 2));
  for (hipEvent_t& x : sc.ev) HIP_TRY(hipEventCreate(&x));
  std::vector<uint32_t> flt;
  double ms_scan = 0, ms_merge = 0;
  for (uint32_t q0 = 0; q0 < nq; q0 += QC) {
    const uint32_t n = std::min(QC, nq - q0);
    HIP_TRY(hipMemcpyAsync(d_q, (const uint8_t*)h_queries + (size_t)q0 * qbytes, (size_t)n * qbytes, hipMemcpyHostToDevice, s));
    if (any) {
      flt.resize((size_t)n * 2);
      for (uint32_t i = 0; i < n; ++i) { flt[2 * (size_t)i] = any[q0 + i]; flt[2 * (size_t)i + 1] = all[q0 + i]; }
      HIP_TRY(hipMemcpyAsync(d_flt, flt.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    bang_scan_params p;
    memset(&p, 0, sizeof(p));
    p.d_vec_base = vec_base; p.vec_stride = vec_stride; p.dtype = (uint32_t)e->dtype; p.D = e->D; p.n_nodes = e->N;
    p.d_queries = d_q; p.nq = n; p.k = k;
    p.d_excluded = (e->n_excl != 0 && e->d_excl) ? e->d_excl : nullptr;
    p.d_removed = e->d_removed;
    p.d_labels = any ? e->d_labels : nullptr; p.d_filters = any ? d_flt : nullptr;
    p.stripes = stripes; p.d_scratch = d_scratch; p.scratch_bytes = scratch_bytes;
    p.d_ids_out = d_ids; p.d_dists_out = d_dists; p.d_matched = d_matched;
    HIP_TRY(hipEventRecord(sc.ev[0], s));
    BANG_TRY(bang_k_scan_marked(&p, s, sc.ev[1]));
    HIP_TRY(hipEventRecord(sc.ev[2], s));
    // the results of this chunk: ids [n][k] are a contiguous piece of the caller's rows, distances [k][n] one piece per rank
    HIP_TRY(hipMemcpyAsync(ids_out + (size_t)q0 * k, d_ids, (size_t)n * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpy2DAsync(dists_out + q0, (size_t)nq * 4, d_dists, (size_t)n * 4, (size_t)n * 4, k, hipMemcpyDeviceToHost, s));
    if (matched_out) HIP_TRY(hipMemcpyAsync(matched_out + q0, d_matched, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, sc.ev[0], sc.ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, sc.ev[1], sc.ev[2]));
    ms_scan += a; ms_merge += b;
  }
  e->scan_ms[0] = ms_scan; e->scan_ms[1] = ms_merge; e->scan_ms[2] = ms_since(t_call);
  return BANG_OK;
}

}  // namespace

extern "C" int bang_scan_e(bang_engine_t* e, const void* h_queries, uint32_t nq, uint32_t k, const uint32_t* any, const uint32_t* all, uint64_t* ids_out,
                           float* dists_out, uint32_t* matched_out) {
  if (!e) { bang_set_error("bang_scan: the engine is null"); return BANG_ERR_ARG; }
  if (!e->loaded) { bang_set_error("bang_scan: no index is loaded"); return BANG_ERR_ARG; }
  if (!h_queries) { bang_set_error("bang_scan: the queries are null"); return BANG_ERR_ARG; }
  if (!ids_out || !dists_out) { bang_set_error("bang_scan: an output buffer (ids, dists) is null"); return BANG_ERR_ARG; }
  if (nq == 0 || nq > BANG_SCAN_MAX_QUERIES) { bang_set_error("bang_scan: nq = %u is outside [1, %u]", nq, BANG_SCAN_MAX_QUERIES); return BANG_ERR_ARG; }
  if (k == 0 || k > BANG_SCAN_MAX_K) { bang_set_error("bang_scan: k = %u is outside [1, %u]", k, BANG_SCAN_MAX_K); return BANG_ERR_ARG; }
  if ((any == nullptr) != (all == nullptr)) { bang_set_error("bang_scan: exactly one of any / all is given: a filter batch is both arrays, or neither"); return BANG_ERR_ARG; }
  if (any && !e->d_labels) { bang_set_error("bang_scan: filters without labels: the index has no label table (bang_set_labels_e)"); return BANG_ERR_ARG; }
  if (e->params_set && e->distfn == BANG_DIST_MIPS) { bang_set_error("bang_scan: MIPS search parameters are set: the scan runs on L2 distances only"); return BANG_ERR_UNSUPPORTED; }
  if (e->vecs_f16) { bang_set_error("bang_scan: the vector table holds fp16 rows (option vectors_fp16): their distances are not the exact ones"); return BANG_ERR_UNSUPPORTED; }
  const uint8_t* vec_base = e->d_graph ? e->d_graph : e->d_vecs;
  const uint64_t vec_stride = e->d_graph ? e->entry_len : (uint64_t)vec_bytes(e);
  if (!vec_base) { bang_set_error("bang_scan: no resident vectors: the graph is in host RAM and the vectors were left there (option vectors = 0)"); return BANG_ERR_UNSUPPORTED; }
  if (!bang_search_can_rerank(e->dtype, e->D, vec_stride, 0)) {
    bang_set_error("bang_scan: the vector layout (dtype %d, D = %u, stride %llu) is outside bang_search_can_rerank: 8-bit vectors need D %% 16 == 0 with D / 16 a "
                   "power of two, float vectors D %% 4 == 0; D <= 256", e->dtype, e->D, (unsigned long long)vec_stride);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->dtype == BANG_F32) {
    uint64_t bad = 0;
    if (bang_check_floats((const float*)h_queries, (uint64_t)nq * e->D, &bad) != BANG_OK) {
      bang_set_error("bang_scan: query %llu, dimension %llu holds %g: float queries must be finite with |x| <= 2^56 (nothing was launched)",
                     (unsigned long long)(bad / e->D), (unsigned long long)(bad % e->D), (double)((const float*)h_queries)[bad]);
      return BANG_ERR_ARG;
    }
  }
  BANG_TRY(ensure_device(e));
  for (double& x : e->scan_ms) x = 0;
  const int rc = scan(e, vec_base, vec_stride, h_queries, nq, k, any, all, ids_out, dists_out, matched_out);
  if (rc != BANG_OK) (void)hipDeviceSynchronize();
  return rc;
}

extern "C" int bang_get_scan_times(bang_engine_t* e, double* ms3) {
  if (!e || !ms3) return BANG_ERR_ARG;
  memcpy(ms3, e->scan_ms, sizeof(e->scan_ms));
  return BANG_OK;
}
