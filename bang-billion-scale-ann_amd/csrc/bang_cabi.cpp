// bang_cabi.cpp -- the engine-level C-ABI of include/bang_c.h: thin entry points over the engine (bang.h:36-87 / :89-101).
#include "bang_engine.h"

#include <cerrno>

using namespace bang;

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
extern "C" void bang_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* bang_last_error(void) { return g_err; }

extern "C" int bang_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ------------------------------------------------------------------ device helpers
extern "C" int bang_dev_malloc(void** d_ptr, size_t bytes) {
  if (!d_ptr) return BANG_ERR_ARG;
  if (bang_device_count() == 0) { bang_set_error("no HIP device"); return BANG_ERR_NOGPU; }
  HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 4));
  return BANG_OK;
}
extern "C" int bang_dev_free(void* d_ptr) { if (d_ptr) HIP_TRY(hipFree(d_ptr)); return BANG_OK; }
extern "C" int bang_dev_memset(void* d_ptr, int value, size_t bytes) { HIP_TRY(hipMemset(d_ptr, value, bytes)); return BANG_OK; }
extern "C" int bang_dev_h2d(void* d_dst, const void* h_src, size_t bytes) {
  HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return BANG_OK;
}
extern "C" int bang_dev_d2h(void* h_dst, const void* d_src, size_t bytes) {
  HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return BANG_OK;
}
extern "C" int bang_dev_sync(void) { HIP_TRY(hipDeviceSynchronize()); return BANG_OK; }

// ------------------------------------------------------------------ excluded ids (lazy deletes)
static void drop_excluded(bang_engine* e) {
  dfree(e->d_excl);
  e->n_excl = 0;
}

// the set as a bitmap, built on the host and copied to the device; nothing is touched before every id has been checked
static int set_excluded(bang_engine* e, const uint32_t* ids, uint64_t n, const char* what) {
  if (!e->loaded) { bang_set_error("%s: no index is loaded", what); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("%s: the excluded ids must be set before bang_alloc (an allocation is live: call bang_free first)", what); return BANG_ERR_ARG; }
  if (n != 0 && !ids) { bang_set_error("%s: ids is null", what); return BANG_ERR_ARG; }
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= e->N) {
      bang_set_error("%s: id %u (entry %llu of the list) is out of range: the index has N = %u nodes", what, ids[i], (unsigned long long)i, e->N);
      return BANG_ERR_ARG;
    }
  if (n == 0) { (void)hipSetDevice(e->device); drop_excluded(e); return BANG_OK; }
  const size_t nodes = std::max<size_t>(e->N, e->capacity > 0 ? (size_t)e->capacity : 0);   // option capacity: the bitmap covers the nodes to come
  const size_t words = (nodes + 31) / 32 + 1;                      // + a word of slack
  std::vector<uint32_t> bits(words, 0u);
  for (uint64_t i = 0; i < n; ++i) bits[ids[i] >> 5] |= 1u << (ids[i] & 31u);
  uint64_t distinct = 0;
  for (uint32_t w : bits) distinct += (uint64_t)__builtin_popcount(w);
  BANG_TRY(ensure_device(e));
  if (!e->d_excl) BANG_TRY(dmalloc(&e->d_excl, words));
  const hipError_t err = hipMemcpy(e->d_excl, bits.data(), words * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) { drop_excluded(e); HIP_TRY(err); }
  e->n_excl = distinct;
  return BANG_OK;
}

extern "C" int bang_set_excluded_e(bang_engine_t* e, const uint32_t* ids, uint64_t n) {
  if (!e) return BANG_ERR_ARG;
  return set_excluded(e, ids, n, "bang_set_excluded");
}

extern "C" int bang_clear_excluded_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  return set_excluded(e, nullptr, 0, "bang_clear_excluded");
}

// a .bin file of u32 words with `cols` columns (i32 rows, i32 cols, rows x cols u32) -> words.  The header's row count must be what the file's size
// says before anything is allocated for it: a corrupt header is a refused file, not an allocation of up to 2^31 rows
static int read_u32_bin(const char* var, const char* path, int32_t cols, const char* layout, std::vector<uint32_t>& words) {
  FILE* f = fopen(path, "rb");
  if (!f) { bang_set_error("%s %s: cannot be opened: %s", var, path, strerror(errno)); return BANG_ERR_IO; }
  int32_t hdr[2] = {0, 0};
  bool ok = fread(hdr, 4, 2, f) == 2 && hdr[0] >= 0 && hdr[1] == cols;
  if (ok) {
    const long long want = 8ll + 4ll * (long long)hdr[0] * (long long)cols;
    ok = fseek(f, 0, SEEK_END) == 0 && (long long)ftell(f) == want && fseek(f, 8, SEEK_SET) == 0;
  }
  if (ok) {
    words.resize((size_t)hdr[0] * (size_t)cols);
    ok = fread(words.data(), 4, words.size(), f) == words.size();
  }
  fclose(f);
  if (!ok) { bang_set_error("%s %s: not a .bin file of %s", var, path, layout); return BANG_ERR_IO; }
  return BANG_OK;
}

// BANG_EXCLUDE_FILE: the last step of every load.  The file has the .bin layout (i32 count, i32 1, count u32 ids)
static int load_exclude_file(bang_engine* e) {
  const char* path = env_str("BANG_EXCLUDE_FILE");
  if (!path) return BANG_OK;
  std::vector<uint32_t> ids;
  BANG_TRY(read_u32_bin("BANG_EXCLUDE_FILE", path, 1, "ids (i32 count, i32 1, count u32 ids)", ids));
  const int rc = set_excluded(e, ids.data(), ids.size(), "BANG_EXCLUDE_FILE");
  if (rc != BANG_OK) {
    const std::string why = bang_last_error();
    bang_set_error("BANG_EXCLUDE_FILE %s: %s", path, why.c_str());
  }
  return rc;
}
// ------------------------------------------------------------------ labels and per-query filters
static void drop_labels(bang_engine* e) { dfree(e->d_labels); }

static int set_labels(bang_engine* e, const uint32_t* labels, uint64_t n, const char* what) {
  if (!e->loaded) { bang_set_error("%s: no index is loaded", what); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("%s: the labels must be set before bang_alloc (an allocation is live: call bang_free first)", what); return BANG_ERR_ARG; }
  if (n == 0) { (void)hipSetDevice(e->device); drop_labels(e); return BANG_OK; }
  if (n != e->N) { bang_set_error("%s: %llu labels for an index of N = %u nodes: every node carries one label word", what, (unsigned long long)n, e->N); return BANG_ERR_ARG; }
  if (!labels) { bang_set_error("%s: labels is null", what); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  if (!e->d_labels) BANG_TRY(dmalloc(&e->d_labels, (size_t)e->N));
  const hipError_t err = hipMemcpy(e->d_labels, labels, (size_t)e->N * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) { drop_labels(e); HIP_TRY(err); }
  return BANG_OK;
}

extern "C" int bang_set_labels_e(bang_engine_t* e, const uint32_t* labels, uint64_t n) {
  if (!e) return BANG_ERR_ARG;
  return set_labels(e, labels, n, "bang_set_labels");
}

extern "C" int bang_clear_labels_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  return set_labels(e, nullptr, 0, "bang_clear_labels");
}

// BANG_LABEL_FILE: read behind BANG_EXCLUDE_FILE as the last step of every load.  The file has the .bin layout (i32 N, i32 1, N u32 label words)
static int load_label_file(bang_engine* e) {
  const char* path = env_str("BANG_LABEL_FILE");
  if (!path) return BANG_OK;
  std::vector<uint32_t> words;
  BANG_TRY(read_u32_bin("BANG_LABEL_FILE", path, 1, "labels (i32 N, i32 1, N u32 label words)", words));
  if (words.empty()) { bang_set_error("BANG_LABEL_FILE %s: the file holds 0 labels for an index of N = %u nodes", path, e->N); return BANG_ERR_ARG; }
  const int rc = set_labels(e, words.data(), words.size(), "BANG_LABEL_FILE");
  if (rc != BANG_OK) {
    const std::string why = bang_last_error();
    bang_set_error("BANG_LABEL_FILE %s: %s", path, why.c_str());
  }
  return rc;
}

static void drop_query_filters(bang_engine* e) {
  dfree(e->d_qfilters); dfree(e->d_matched);
  e->n_qfilters = 0; e->n_filtered = 0; e->qfilters_from_file = false;
}

extern "C" int bang_set_query_filters_e(bang_engine_t* e, const uint32_t* any, const uint32_t* all, int nq) {
  if (!e) return BANG_ERR_ARG;
  const char* what = "bang_set_query_filters";
  if (!e->allocated) { bang_set_error("%s: the filters of a batch live in its allocation: call bang_alloc first", what); return BANG_ERR_ARG; }
  if (nq < 0 || nq > e->Qcap) { bang_set_error("%s: %d filters exceed the allocation of %d queries", what, nq, e->Qcap); return BANG_ERR_ARG; }
  if (nq == 0) { (void)hipSetDevice(e->device); drop_query_filters(e); return BANG_OK; }
  if (!any || !all) { bang_set_error("%s: any / all is null", what); return BANG_ERR_ARG; }
  if (!e->d_labels) { bang_set_error("%s: no labels are set (bang_set_labels_e or BANG_LABEL_FILE, before bang_alloc)", what); return BANG_ERR_UNSUPPORTED; }
  if (e->n_radii != 0) { bang_set_error("%s: filters on labels and radii (bang_set_query_radii_e) do not combine: clear the radii first (bang_clear_query_radii_e)", what); return BANG_ERR_UNSUPPORTED; }
  // the forms without a label-filter kernel are refused: there is no unfiltered fallback
  const bool dev_graph = (e->graph_mode == BANG_GRAPH_DEVICE);
  if (e->form != LoopForm::Exact) {
    bang_set_error("%s: filters on labels need option distance = 1 (exact): the PQ walks have no exact distance when a node is evaluated", what);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->beam > 1) { bang_set_error("%s: filters on labels are not available with option beam = %d: the beam kernel keeps no result list", what, e->beam); return BANG_ERR_UNSUPPORTED; }
  if (e->vecs_f16 && !dev_graph) { bang_set_error("%s: filters on labels are not available with vectors_fp16 = 1: the label-filter kernel reads float / 8-bit rows", what); return BANG_ERR_UNSUPPORTED; }
  if (!bang_search_can_rerank(e->dtype, e->D, dev_graph ? e->entry_len : (uint64_t)vec_table_stride(e), 0)) {
    bang_set_error("%s: filters on labels are not available on the wide vector layouts (dtype %d, D = %u): 8-bit vectors need D / 16 a power of two, D <= 256",
                   what, e->dtype, e->D);
    return BANG_ERR_UNSUPPORTED;
  }
  BANG_TRY(ensure_device(e));
  std::vector<uint32_t> rows((size_t)nq * 2);
  uint64_t filtered = 0;
  for (int i = 0; i < nq; ++i) { rows[2 * (size_t)i] = any[i]; rows[2 * (size_t)i + 1] = all[i]; filtered += (any[i] | all[i]) != 0u; }
  if (!e->d_qfilters) BANG_TRY(dmalloc(&e->d_qfilters, (size_t)e->Qcap * 2));
  if (!e->d_matched) BANG_TRY(dmalloc(&e->d_matched, (size_t)e->Qcap));
  const hipError_t err = hipMemcpy(e->d_qfilters, rows.data(), rows.size() * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) { drop_query_filters(e); HIP_TRY(err); }
  e->n_qfilters = (uint32_t)nq;
  e->n_filtered = filtered;
  e->qfilters_from_file = false;
  return BANG_OK;
}

extern "C" int bang_clear_query_filters_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  if (e->allocated) (void)hipSetDevice(e->device);
  drop_query_filters(e);
  return BANG_OK;
}

// BANG_QUERY_FILTER_FILE, for the bang.h class and the CLI (bang_internal.h; called by BANGSearch<T>::bang_query): row i of the file is the filter of
// query i of the batch about to run.  The file is read once per allocation (bang_free forgets it) and its rows go to HBM when the first batch
// runs or a batch of another size follows; a batch of the size the filters already have costs nothing here
extern "C" int bang_apply_query_filter_file_e(bang_engine_t* e, int nq) {
  if (!e) return BANG_ERR_ARG;
  const char* path = env_str("BANG_QUERY_FILTER_FILE");
  if (!path) return BANG_OK;
  if (e->qfilters_from_file && nq > 0 && e->n_qfilters == (uint32_t)nq) return BANG_OK;
  if (e->qfilter_file_rows.empty()) BANG_TRY(read_u32_bin("BANG_QUERY_FILTER_FILE", path, 2, "filters (i32 Q, i32 2, Q x {any, all} u32)", e->qfilter_file_rows));
  const std::vector<uint32_t>& words = e->qfilter_file_rows;
  if (nq <= 0 || words.size() / 2 < (size_t)nq) {
    bang_set_error("BANG_QUERY_FILTER_FILE %s: the file holds %zu filters, the batch has %d queries", path, words.size() / 2, nq);
    return BANG_ERR_ARG;
  }
  std::vector<uint32_t> any((size_t)nq), all((size_t)nq);
  for (int i = 0; i < nq; ++i) { any[(size_t)i] = words[2 * (size_t)i]; all[(size_t)i] = words[2 * (size_t)i + 1]; }
  const int rc = bang_set_query_filters_e(e, any.data(), all.data(), nq);
  if (rc != BANG_OK) {
    const std::string why = bang_last_error();
    bang_set_error("BANG_QUERY_FILTER_FILE %s: %s", path, why.c_str());
  } else e->qfilters_from_file = true;
  return rc;
}

extern "C" int bang_get_matched_counts(bang_engine_t* e, uint32_t* out, uint32_t num_queries) {
  if (!e || !out) return BANG_ERR_ARG;
  if (!e->allocated || e->Qcur <= 0 || e->stat_label_launches == 0 || !e->d_matched) {
    bang_set_error("bang_get_matched_counts: the last query on this allocation did not run with filters on labels");
    return BANG_ERR_ARG;
  }
  if (num_queries > (uint32_t)e->Qcur) { bang_set_error("bang_get_matched_counts: %u counts asked for, the last batch had %d queries", num_queries, e->Qcur); return BANG_ERR_ARG; }
  HIP_TRY(hipMemcpy(out, e->d_matched, (size_t)num_queries * 4, hipMemcpyDeviceToHost));
  return BANG_OK;
}

// ------------------------------------------------------------------ range search: per-query radii and the batch's hits
extern "C" int bang_set_query_radii_e(bang_engine_t* e, const float* radii, int nq) {
  if (!e) return BANG_ERR_ARG;
  const char* what = "bang_set_query_radii";
  if (!e->allocated) { bang_set_error("%s: the radii of a batch live in its allocation: call bang_alloc first", what); return BANG_ERR_ARG; }
  if (e->range_hits <= 0 || !e->d_radius) { bang_set_error("%s: range search is off: option range_hits = 0 (set it before bang_alloc)", what); return BANG_ERR_UNSUPPORTED; }
  if (nq < 0 || nq > e->Qcap) { bang_set_error("%s: %d radii exceed the allocation of %d queries", what, nq, e->Qcap); return BANG_ERR_ARG; }
  if (nq == 0) { e->n_radii = 0; return BANG_OK; }
  if (!radii) { bang_set_error("%s: radii is null", what); return BANG_ERR_ARG; }
  if (e->n_qfilters != 0) { bang_set_error("%s: radii and filters on labels (bang_set_query_filters_e) do not combine: clear the filters first (bang_clear_query_filters_e)", what); return BANG_ERR_UNSUPPORTED; }
  BANG_TRY(ensure_device(e));
  const hipError_t err = hipMemcpy(e->d_radius, radii, (size_t)nq * 4, hipMemcpyHostToDevice);
  if (err != hipSuccess) { e->n_radii = 0; HIP_TRY(err); }
  e->n_radii = (uint32_t)nq;
  return BANG_OK;
}

extern "C" int bang_clear_query_radii_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  e->n_radii = 0;
  return BANG_OK;
}

// the counts of the last range batch, fetched once per batch: count and offered of its Qcur queries
static int range_counts(bang_engine* e, const char* what) {
  if (!e->allocated || e->Qcur <= 0 || e->stat_range_launches == 0 || !e->d_range_count) {
    bang_set_error("%s: the last query on this allocation did not run with radii (bang_set_query_radii_e)", what);
    return BANG_ERR_ARG;
  }
  if (e->range_counts_valid) return BANG_OK;
  const size_t nq = (size_t)e->Qcur;
  e->h_range_count.resize(nq); e->h_range_offered.resize(nq);
  (void)hipSetDevice(e->device);
  HIP_TRY(hipMemcpy(e->h_range_count.data(), e->d_range_count, nq * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(e->h_range_offered.data(), e->d_offered, nq * 4, hipMemcpyDeviceToHost));
  uint64_t trunc = 0;
  for (size_t i = 0; i < nq; ++i) trunc += e->h_range_offered[i] > (uint32_t)e->range_hits;
  e->stat_range_truncated = trunc;
  e->range_counts_valid = true;
  return BANG_OK;
}

extern "C" int bang_get_range_counts(bang_engine_t* e, uint32_t* counts, uint32_t* offered, uint32_t num_queries) {
  if (!e) return BANG_ERR_ARG;
  BANG_TRY(range_counts(e, "bang_get_range_counts"));
  if (num_queries > (uint32_t)e->Qcur) { bang_set_error("bang_get_range_counts: %u counts asked for, the last batch had %d queries", num_queries, e->Qcur); return BANG_ERR_ARG; }
  if (counts) memcpy(counts, e->h_range_count.data(), (size_t)num_queries * 4);
  if (offered) memcpy(offered, e->h_range_offered.data(), (size_t)num_queries * 4);
  return BANG_OK;
}

extern "C" int bang_get_range_results(bang_engine_t* e, uint64_t* lims, uint64_t* ids, float* dists, uint64_t capacity) {
  if (!e || !lims) return BANG_ERR_ARG;
  BANG_TRY(range_counts(e, "bang_get_range_results"));
  const size_t nq = (size_t)e->Qcur;
  uint64_t total = 0;
  uint32_t width = 0;
  for (size_t i = 0; i < nq; ++i) { total += e->h_range_count[i]; width = std::max(width, e->h_range_count[i]); }
  if (capacity < total) { bang_set_error("bang_get_range_results: capacity = %llu, the last batch has %llu hits", (unsigned long long)capacity, (unsigned long long)total); return BANG_ERR_ARG; }
  if (total != 0 && (!ids || !dists)) { bang_set_error("bang_get_range_results: ids / dists is null"); return BANG_ERR_ARG; }
  if (width != 0) {
    // ONE strided copy per array: the first `width` columns -- the largest count -- of the batch's rows, then packed on the host
    const size_t pitch = (size_t)e->range_hits * 4;
    std::vector<uint32_t> hid(nq * width), hd(nq * width);
    HIP_TRY(hipMemcpy2D(hid.data(), (size_t)width * 4, e->d_hit_ids, pitch, (size_t)width * 4, nq, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(hd.data(), (size_t)width * 4, e->d_hit_dists, pitch, (size_t)width * 4, nq, hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (size_t i = 0; i < nq; ++i) {
      const uint32_t c = e->h_range_count[i];
      for (uint32_t j = 0; j < c; ++j) ids[at + j] = (uint64_t)hid[i * width + j];
      memcpy(dists + at, hd.data() + i * width, (size_t)c * 4);
      at += c;
    }
  }
  lims[0] = 0;
  for (size_t i = 0; i < nq; ++i) lims[i + 1] = lims[i] + e->h_range_count[i];
  return BANG_OK;
}

static int finish_load(bang_engine* e, int rc) {
  if (rc == BANG_OK) rc = load_exclude_file(e);
  if (rc == BANG_OK) rc = load_label_file(e);
  if (rc != BANG_OK) { drop_excluded(e); drop_labels(e); unload_index(e); }
  return rc;
}

// ------------------------------------------------------------------ C-ABI, engine level
extern "C" int bang_create(int dtype, bang_engine_t** out) {
  if (!out || dtype < BANG_U8 || dtype > BANG_F32) { bang_set_error("bad dtype"); return BANG_ERR_ARG; }
  bang_engine* e = new (std::nothrow) bang_engine();
  if (!e) return BANG_ERR_NOMEM;
  e->dtype = dtype;
  e->tsize = (dtype == BANG_F32) ? 4 : 1;
  // presets from the environment, so that callers of the bang.h class API (no option methods, e.g. the bang_search CLI) can still
  // choose placement and loop form (bang_options.cpp: BANG_GRAPH=host|device|auto, BANG_PULL, BANG_THREADS, ...)
  apply_env_defaults(e);
  *out = e;
  return BANG_OK;
}

extern "C" int bang_destroy(bang_engine_t* e) {
  if (!e) return BANG_OK;
  if (e->allocated) free_batch(e);
  drop_excluded(e);
  drop_labels(e);
  dfree(e->d_removed);
  if (e->loaded) unload_index(e);
  delete e;
  return BANG_OK;
}

extern "C" int bang_load_e(bang_engine_t* e, const char* prefix) {
  if (!e || !prefix) return BANG_ERR_ARG;
  if (e->loaded) { bang_set_error("index already loaded"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  const int rc = load_files(e, prefix);
  if (rc != BANG_OK) return rc;
  return finish_load(e, rc);
}

extern "C" int bang_load_mem_e(bang_engine_t* e, const bang_index_desc* d) {
  if (!e || !d || !d->graph || !d->pivots || !d->centroid || !d->chunk_off || (!d->codes && !d->d_codes)) {
    bang_set_error("bad index descriptor");
    return BANG_ERR_ARG;
  }
  if (e->loaded) { bang_set_error("index already loaded"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  e->medoid = d->medoid; e->entry_len = d->entry_len; e->D = d->D; e->R = d->R; e->N = d->N; e->m = d->m;
  e->graph = d->graph;
  e->graph_owned = nullptr;
  e->graph_path.clear();
  const int rc = upload_index(e, d->codes, d->d_codes, d->pivots, d->centroid, d->chunk_off, d->d_codes ? d->code_stride : 0);
  return finish_load(e, rc);
}

extern "C" int bang_load_stream_e(bang_engine_t* e, const bang_index_desc* d, bang_entry_source src, void* ctx) {
  if (!e || !d || !src || d->graph || !d->pivots || !d->centroid || !d->chunk_off || (!d->codes && !d->d_codes)) {
    bang_set_error("bad index descriptor (a streamed load takes an entry source and no graph pointer)");
    return BANG_ERR_ARG;
  }
  if (e->loaded) { bang_set_error("index already loaded"); return BANG_ERR_ARG; }
  if (e->capacity > 0) { bang_set_error("option capacity = %d does not apply: a streamed load keeps the adjacency lists on the host (and the vectors, where given, in the caller's buffer)", e->capacity); return BANG_ERR_UNSUPPORTED; }
  BANG_TRY(ensure_device(e));
  e->medoid = d->medoid; e->entry_len = d->entry_len; e->D = d->D; e->R = d->R; e->N = d->N; e->m = d->m;
  e->graph = nullptr;
  e->graph_owned = nullptr;
  e->graph_path.clear();
  if (e->graph_mode == BANG_GRAPH_DEVICE) { bang_set_error("a streamed load keeps the adjacency lists on the host (pull mode): option graph = device does not apply"); return BANG_ERR_UNSUPPORTED; }
  e->graph_mode = BANG_GRAPH_HOST;                       // (auto included: there is no graph image to put into HBM)
  if (e->entry_len != (uint64_t)e->D * e->tsize + 4 + 4ull * e->R) {
    bang_set_error("index entry length %llu does not match D=%u x %zu B + 4 + 4 x R=%u", (unsigned long long)e->entry_len, e->D, e->tsize, e->R);
    return BANG_ERR_ARG;
  }
  e->entry_fn = src; e->entry_ctx = ctx;
  e->ext_vecs = (uint8_t*)d->d_vectors; e->ext_vecs_ready = false;
  const int rc = upload_index(e, d->codes, d->d_codes, d->pivots, d->centroid, d->chunk_off, d->d_codes ? d->code_stride : 0);
  e->entry_fn = nullptr; e->entry_ctx = nullptr; e->ext_vecs = nullptr;
  return finish_load(e, rc);
}

extern "C" int bang_load_shared_e(bang_engine_t* e, const bang_index_desc* d) {
  if (!e || !d || d->graph || !d->pivots || !d->centroid || !d->chunk_off || (!d->codes && !d->d_codes) || !d->d_vectors || !d->vectors_ready) {
    bang_set_error("bad index descriptor (a shared load takes the filled vector buffer of the node's loading rank and no graph)");
    return BANG_ERR_ARG;
  }
  if (e->loaded) { bang_set_error("index already loaded"); return BANG_ERR_ARG; }
  if (e->capacity > 0) { bang_set_error("option capacity = %d does not apply: a shared load runs on the host placement, its vectors in the caller's buffer", e->capacity); return BANG_ERR_UNSUPPORTED; }
  BANG_TRY(ensure_device(e));
  e->medoid = d->medoid; e->entry_len = d->entry_len; e->D = d->D; e->R = d->R; e->N = d->N; e->m = d->m;
  e->graph = nullptr; e->graph_owned = nullptr; e->graph_path.clear();
  if (e->graph_mode == BANG_GRAPH_DEVICE || e->pull_opt == 0 || e->vectors_opt == 0 || e->persistent == 0 || e->search_opt == 0) {
    bang_set_error("a shared load runs in pull mode on the host placement only");
    return BANG_ERR_UNSUPPORTED;
  }
  e->graph_mode = BANG_GRAPH_HOST;
  if (e->entry_len != (uint64_t)e->D * e->tsize + 4 + 4ull * e->R) { bang_set_error("index entry length does not match D / R"); return BANG_ERR_ARG; }
  e->entry_fn = nullptr; e->entry_ctx = nullptr;
  e->ext_vecs = (uint8_t*)d->d_vectors; e->ext_vecs_ready = true; e->rows_hash = d->rows_hash;
  const int rc = upload_index(e, d->codes, d->d_codes, d->pivots, d->centroid, d->chunk_off, d->d_codes ? d->code_stride : 0);
  e->ext_vecs = nullptr; e->ext_vecs_ready = false;
  return finish_load(e, rc);
}

extern "C" int bang_get_rows_hash(bang_engine_t* e, uint64_t* out) {
  if (!e || !out) return BANG_ERR_ARG;
  if (!e->loaded || !e->pull) { bang_set_error("bang_get_rows_hash: no index in pull mode is loaded"); return BANG_ERR_ARG; }
  *out = e->rows_hash;
  return BANG_OK;
}

extern "C" int bang_set_searchparams_e(bang_engine_t* e, int recall, int worklist_length, int distfn) {
  if (!e) return BANG_ERR_ARG;
  if (recall <= 0 || worklist_length < recall || worklist_length > BANG_MAX_L ||            // assert(2L <= 1024) :439
      (distfn != BANG_DIST_L2 && distfn != BANG_DIST_MIPS)) {
    bang_set_error("bad search params: recall=%d L=%d distfn=%d", recall, worklist_length, distfn);
    return BANG_ERR_ARG;
  }
  if (e->allocated && (recall != e->k || worklist_length != e->L)) {
    bang_set_error("bang_free must be called before changing recall / worklist length");   // sizes depend on them :370-384
    return BANG_ERR_ARG;
  }
  e->k = recall; e->L = worklist_length; e->distfn = distfn;
  e->params_set = true;
  return BANG_OK;
}

extern "C" int bang_alloc_e(bang_engine_t* e, int Q) {
  if (!e || Q <= 0) return BANG_ERR_ARG;
  if (!e->loaded || !e->params_set) { bang_set_error("bang_alloc: load an index and set search params first"); return BANG_ERR_ARG; }
  if (e->allocated) { bang_set_error("bang_alloc: already allocated (call bang_free)"); return BANG_ERR_ARG; }
  if (e->insert_broken) { bang_set_error("bang_alloc: an insert failed half-way and old rows may list ids beyond N: unload this engine (bang_unload) and load the index again"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  e->Qcap = Q;
  e->Qcur = 0;
  e->cand_stride = (uint32_t)e->L + (e->semantics == 1 ? BANG_INMEM_EXTRA_ITERS : BANG_EXTRA_ITERS);     // (semantics = 1: L + 120)
  BANG_TRY(validate_pull_rows(e));       // a truncated / overwritten rows file is reported as such -- and never costs the HBM row cache below
  if (e->n_slices > 1) {                 // peer rows: the slice table (biased base addresses: own HBM, peers' HBM) goes to the device
    if (!e->d_slice_tab) BANG_TRY(dmalloc(&e->d_slice_tab, (size_t)BANG_MAX_ROW_SLICES));
    HIP_TRY(hipMemcpy(e->d_slice_tab, e->slice_base, sizeof(e->slice_base), hipMemcpyHostToDevice));
  }
  int rc = alloc_buffers(e, Q);
  if (rc == BANG_ERR_NOMEM && e->d_rows_hbm && !e->rows_exported && e->n_slices == 0) {
    // the copy of the first adjacency rows took the HBM a batch of this size needs: the rows are in host memory anyway
    free_batch(e);
    dfree(e->d_rows_hbm);
    e->n_rows_hbm = 0; e->rows_first = e->n_rows_pad;      // (the padded rows cost no memory: they stay)
    (void)hipGetLastError();
    rc = alloc_buffers(e, Q);
  }
  if (rc != BANG_OK) { free_batch(e); return rc; }
  e->allocated = true;
  e->inited = false;
  return BANG_OK;
}

extern "C" int bang_init_e(bang_engine_t* e, int Q) {
  if (!e || !e->allocated || Q <= 0 || Q > e->Qcap) { bang_set_error("bang_init: bad state / numQueries"); return BANG_ERR_ARG; }
  BANG_TRY(ensure_device(e));
  const size_t nq = (size_t)Q;
  // ONE launch (filters :443, state :440-464, counters) on the stream the first lane's bang_query starts on; the call returns when
  // it is done -- bang_init stays outside the harness's timed region (test_driver.cpp:432-439) -- without a device-wide synchronisation
  bang_init_params ia;
  memset(&ia, 0, sizeof(ia));
  ia.Q = (uint32_t)Q; ia.medoid = (uint32_t)e->medoid; ia.cand_stride = e->cand_stride;
  ia.d_bloom = e->d_bloom; ia.d_cand_ids = e->d_cand_ids; ia.d_cand_row = e->d_cand_row; ia.d_cand_cnt = e->d_cand_cnt;
  ia.d_wl_cnt = e->d_wl_cnt; ia.d_mark = e->d_mark; ia.d_parents = e->d_parents_dev; ia.d_cnt = e->d_cnt;
  ia.d_qstats = e->d_qstats; ia.d_qskip = e->d_qskip;
  ia.d_active = e->d_active; ia.n_active = e->d_active ? e->cand_stride + 2 : 0;
  hipStream_t st = e->lanes.empty() ? nullptr : e->lanes[0]->s_main;
  BANG_TRY(bang_k_init_all(&ia, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (e->h_parents && e->form != LoopForm::SelfPaced && e->form != LoopForm::Exact) for (size_t i = 0; i < nq; ++i) e->h_parents[i] = BANG_NO_PARENT;   // (the walker forms read it)
  e->inited = true;
  return BANG_OK;
}

static int query_impl(bang_engine_t* e, const void* h_queries, int Q, uint64_t* h_ids, float* h_dists, uint64_t* d_ids_user, float* d_dists_user);

extern "C" int bang_query_e(bang_engine_t* e, const void* h_queries, int Q, uint64_t* h_ids, float* h_dists) {
  if (!e || !h_queries || !h_ids || !h_dists) return BANG_ERR_ARG;
  return query_impl(e, h_queries, Q, h_ids, h_dists, nullptr, nullptr);
}

extern "C" int bang_query_dev_e(bang_engine_t* e, const void* h_queries, int Q, uint64_t* d_ids, float* d_dists) {
  if (!e || !h_queries || !d_ids) return BANG_ERR_ARG;
  return query_impl(e, h_queries, Q, nullptr, nullptr, d_ids, d_dists);
}

static int query_impl(bang_engine_t* e, const void* h_queries, int Q, uint64_t* h_ids, float* h_dists, uint64_t* d_ids_user, float* d_dists_user) {
  if (!e->allocated || !e->inited) { bang_set_error("bang_query: bang_alloc + bang_init must precede every query"); return BANG_ERR_ARG; }
  if (Q <= 0 || Q > e->Qcap) { bang_set_error("bang_query: numQueries %d exceeds allocation %d", Q, e->Qcap); return BANG_ERR_ARG; }
  if (e->n_radii != 0 && (uint32_t)Q != e->n_radii) {
    bang_set_error("bang_query: a batch of %d queries, but the radii were set for %u (bang_set_query_radii_e; bang_clear_query_radii_e drops them)", Q, e->n_radii);
    return BANG_ERR_ARG;
  }
  if (e->n_qfilters != 0 && (uint32_t)Q != e->n_qfilters) {
    bang_set_error("bang_query: a batch of %d queries, but the filters were set for %u (bang_set_query_filters_e; bang_clear_query_filters_e drops them)", Q, e->n_qfilters);
    return BANG_ERR_ARG;
  }
  if (e->dtype == BANG_F32) {                          // CANON 20: finite, |x| <= 2^56 -- before a lane is started or a copy issued
    const uint64_t qdim = e->D - (e->distfn == BANG_DIST_MIPS ? 1u : 0u);    // MIPS: the queries come without the padding dimension (bang_lane.cpp)
    uint64_t bad = 0;
    if (bang_check_floats((const float*)h_queries, (uint64_t)Q * qdim, &bad) != BANG_OK) {
      const float v = ((const float*)h_queries)[bad];
      bang_set_error("bang_query: query %llu, dimension %llu holds %g: float queries must be finite with |x| <= 2^56 (nothing was launched)",
                     (unsigned long long)(bad / qdim), (unsigned long long)(bad % qdim), (double)v);
      return BANG_ERR_ARG;
    }
  }
  e->inited = false;   // state is consumed
  e->Qcur = Q;
  // the calling thread is lane 0's walker: it joins the GPU's NUMA node for the duration of the query
  cpu_set_t caller_cpus;
  const bool repin = e->numa_on && sched_getaffinity(0, sizeof(caller_cpus), &caller_cpus) == 0;
  if (repin) pin_walker_thread(e, 0);
  const auto t0 = Clock::now();
  const int nl = (int)e->lanes.size();
  for (int i = 0; i < nl; ++i) {                       // lanes were laid out for Qcap; re-slice for this Q
    Lane& ln = *e->lanes[(size_t)i];
    ln.q0 = (uint32_t)((size_t)Q * i / nl);
    ln.nq = (uint32_t)((size_t)Q * (i + 1) / nl) - ln.q0;
  }
  std::atomic<bool> wd_stop{false};
  std::thread wd;
  if (const char* wd_path = env_str("BANG_WATCHDOG")) {
    wd = std::thread([&, wd_path] {
      FILE* wf = fopen(wd_path, "a");
      if (!wf) wf = stderr;
      int ticks = 0;
      while (!wd_stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        if (++ticks % 50 == 0) {
          for (auto& lp : e->lanes)
            fprintf(wf, "[watchdog] lane %d phase %d iter %u pending %u epoch %u flag %u active %d\n", lp->index, lp->phase.load(),
                    lp->phase_iter.load(), lp->pending.load(), lp->epoch.load(), e->h_done ? e->h_done[(size_t)lp->index * 16] : 0u,
                    (int)lp->team_active.load());
          fflush(wf);
        }
      }
      if (wf != stderr) fclose(wf);
    });
  }
  Pool& pool = e->pool;
  {
    std::lock_guard<std::mutex> lk(pool.m);
    pool.h_queries = h_queries; pool.h_ids = h_ids; pool.h_dists = h_dists; pool.Q = Q;
    pool.d_ids_user = d_ids_user; pool.d_dists_user = d_dists_user;
    pool.lanes_done = 0;
    ++pool.query_seq;
  }
  pool.cv_start.notify_all();
  lane_job(e, *e->lanes[0]);                           // lane 0 on the calling thread
  if (nl > 1) {
    std::unique_lock<std::mutex> lk(pool.m);
    pool.cv_done.wait(lk, [&] { return pool.lanes_done == nl - 1; });
  }
  if (wd.joinable()) { wd_stop.store(true); wd.join(); }
  if (repin) (void)sched_setaffinity(0, sizeof(caller_cpus), &caller_cpus);
  int rc = BANG_OK;
  for (auto& lp : e->lanes)
    if (lp->rc != BANG_OK) { rc = lp->rc; bang_set_error("%s", lp->err.c_str()); break; }
  bang_stats& s = e->stats;
  memset(&s, 0, sizeof(s));
  s.wall_ms = ms_since(t0);
  for (auto& lp : e->lanes) {
    Lane& ln = *lp;
    s.iterations = std::max<uint64_t>(s.iterations, ln.iterations);
    s.front_launches += ln.front_launches;
    s.front_ms += ln.front_ms; s.back_ms += ln.back_ms; s.rerank_ms += ln.rerank_ms; s.walker_ms += ln.walker_ms;
    s.sync_ms += ln.sync_ms; s.enqueue_ms += ln.enqueue_ms;
    s.h2d_bytes += ln.h2d_bytes.load();
  }
  e->stat_exclude_launches = 0;
  for (auto& lp : e->lanes) e->stat_exclude_launches += lp->exclude_launches;
  e->stat_label_launches = 0;
  for (auto& lp : e->lanes) e->stat_label_launches += lp->label_launches;
  e->stat_filtered_queries = e->stat_label_launches != 0 ? e->n_filtered : 0;
  e->stat_range_launches = 0;
  for (auto& lp : e->lanes) e->stat_range_launches += lp->range_launches;
  e->stat_range_queries = e->stat_range_launches != 0 ? (uint64_t)Q : 0;
  e->stat_range_truncated = 0; e->range_counts_valid = false;       // (counted when the batch's counts are fetched: bang_get_stats_ext4)
  const bool host_paced = e->form == LoopForm::HostPaced;
  const bool self_walk = e->form == LoopForm::SelfPaced || e->form == LoopForm::Exact;      // the kernel finds its adjacency rows itself: nothing walks
  s.persistent = one_launch(e) ? 1 : 0;
  s.vectors_on_device = e->vec_on_device ? 1 : 0;
  s.graph_mode = (uint64_t)e->graph_mode;
  s.lanes = (uint64_t)nl;
  s.walker_threads = (e->graph_mode == BANG_GRAPH_DEVICE || self_walk) ? 0 : (uint64_t)e->threads_eff;   // (pull mode: nothing walks)
  s.wg_queries = host_paced ? e->sv_W * e->sv_C : 0;
  s.pacing_groups = host_paced ? e->sv_NG : 0;
  s.graph_pull = (e->pull && self_walk && e->graph_mode != BANG_GRAPH_DEVICE) ? 1 : 0;
  s.workgroups = host_paced ? (uint64_t)e->sv_G : one_launch(e) ? (uint64_t)std::min(Q, bang_num_cus()) : 0;
  s.search_kernel = one_launch(e) ? 1 : 0;
  s.rerank_fused = e->rerank_fused ? 1 : 0;
  s.vectors_fp16 = e->vecs_f16 ? 1 : 0;
  s.vector_table_bytes = (e->vec_on_device && e->d_vecs) ? (uint64_t)e->N * vec_table_stride(e) + 256 : 0;
  s.walker_rows = (host_paced && e->walker_rows) ? 1 : 0;
  e->stat_filter_layout = e->search_wordfilter ? 1 : 0;          // (reported behind bang_stats: bang_get_stats_ext)
  s.code_stride = e->code_stride;
  // what the kernel was GIVEN (bang_lane.cpp): without a slice table a slice moved off row 0 (bang_rows_slice_e(first > 0)) is not reachable
  // (padded rows, option rows_pad: the nodes [0, n_rows_pad) in front of the copy count too)
  s.rows_in_hbm = (s.graph_pull ? (e->n_slices > 1 ? e->n_rows_hbm : (uint64_t)e->n_rows_pad + rows_direct(e)) : 0);
  return rc;
}

// reduce the in-kernel stamps of a lane: per launch max(end) - min(start) over the workgroups that ran
static int reduce_ktimes(Lane& ln, std::vector<std::pair<unsigned long long, unsigned long long>>& intervals) {
  if (!ln.d_ktime || ln.kt_used == 0) return BANG_OK;
  std::vector<unsigned long long> kt(ln.kt_used * KT_WGS * 2);
  HIP_TRY(hipMemcpy(kt.data(), ln.d_ktime, kt.size() * 8, hipMemcpyDeviceToHost));
  ln.front_ms = 0;
  for (size_t l = 0; l < ln.kt_used; ++l) {
    unsigned long long lo = ~0ull, hi = 0;
    for (size_t w = 0; w < KT_WGS; ++w) {
      const unsigned long long a = kt[(l * KT_WGS + w) * 2], b = kt[(l * KT_WGS + w) * 2 + 1];
      if (a == 0 || b == 0) continue;                  // workgroup slot not used by this launch
      lo = std::min(lo, a);
      hi = std::max(hi, b);
    }
    if (hi > lo) { ln.front_ms += (double)(hi - lo) * 1e-5; intervals.emplace_back(lo, hi); }   // 100 MHz ticks -> ms
  }
  if (const char* path = env_str("BANG_KT_TRACE")) {            // raw stamps of lane 0 for offline analysis
    if (ln.index == 0) if (FILE* f = fopen(path, "wb")) {
      const uint64_t hdr[2] = {(uint64_t)ln.kt_used, (uint64_t)KT_WGS};
      fwrite(hdr, 8, 2, f);
      fwrite(kt.data(), 8, kt.size(), f);
      fclose(f);
    }
  }
  HIP_TRY(hipMemset(ln.d_ktime, 0, ln.kt_used * KT_WGS * 16));
  ln.kt_used = 0;
  return BANG_OK;
}

extern "C" int bang_get_stats(bang_engine_t* e, bang_stats* out) {
  if (!e || !out) return BANG_ERR_ARG;
  bang_stats& s = e->stats;
  if (e->allocated && e->timing && s.front_ms == 0) {
    std::vector<std::pair<unsigned long long, unsigned long long>> iv;
    for (auto& lp : e->lanes) { BANG_TRY(reduce_ktimes(*lp, iv)); s.front_ms += lp->front_ms; }
    std::sort(iv.begin(), iv.end());                   // the stamps of all lanes share one 100 MHz clock: merge the intervals
    unsigned long long cur_lo = 0, cur_hi = 0, busy = 0;
    for (auto& p : iv) {
      if (p.first > cur_hi) { busy += cur_hi - cur_lo; cur_lo = p.first; cur_hi = p.second; }
      else cur_hi = std::max(cur_hi, p.second);
    }
    busy += cur_hi - cur_lo;
    s.front_busy_ms = (double)busy * 1e-5;
  }
  if (e->allocated && e->Qcur > 0 && s.candidates == 0) {   // device-side counters are fetched lazily
    std::vector<uint32_t> qs((size_t)e->Qcur * 2);
    HIP_TRY(hipMemcpy(qs.data(), e->d_qstats, qs.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < qs.size(); i += 2) { s.dist_evals += qs[i]; s.fetched += qs[i + 1]; }
    if (e->form == LoopForm::SelfPaced) {
      std::vector<uint32_t> sk((size_t)e->Qcur);
      HIP_TRY(hipMemcpy(sk.data(), e->d_qskip, sk.size() * 4, hipMemcpyDeviceToHost));
      for (uint32_t v : sk) s.filter_loads_skipped += v;
    }
    std::vector<uint32_t> cc((size_t)e->Qcur);
    HIP_TRY(hipMemcpy(cc.data(), e->d_cand_cnt, cc.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t c : cc) s.candidates += c;
    std::sort(cc.begin(), cc.end());
    s.hops_p50 = cc[cc.size() / 2];
    s.hops_p99 = cc[std::min(cc.size() - 1, (cc.size() * 99) / 100)];
    s.hops_max = cc.back();
    if (s.graph_pull || e->walker_self) {                // one row per expansion (the seed list is on the device) ...
      uint64_t pulled = s.candidates - (uint64_t)e->Qcur;
      if (e->n_rows_hbm || e->n_rows_pad || e->n_slices > 1) {            // ... unless the expanded node's row sits in HBM (this GPU's or a peer's): count the candidate log
        std::vector<uint32_t> ids((size_t)e->Qcur * e->cand_stride);
        HIP_TRY(hipMemcpy(ids.data(), e->d_cand_ids, ids.size() * 4, hipMemcpyDeviceToHost));
        pulled = 0;
        std::vector<uint32_t> cnt((size_t)e->Qcur);
        HIP_TRY(hipMemcpy(cnt.data(), e->d_cand_cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
        for (size_t q = 0; q < (size_t)e->Qcur; ++q)
          for (uint32_t i = 1; i < cnt[q] && i < e->cand_stride; ++i) {
            const uint32_t id = ids[q * e->cand_stride + i];
            if (e->n_slices > 1 && s.graph_pull) {
              const uint32_t sl = id / e->slice_rows;
              if (sl < e->n_slices && e->slice_base[sl]) { if (sl == e->own_slot) ++s.rows_from_own_hbm; else ++s.rows_from_peer; }
              else ++pulled;
            } else if (id < e->n_rows_pad || id - e->n_rows_pad < rows_direct(e)) ++s.rows_from_own_hbm;      // (padded rows, then the copy behind them)
            else ++pulled;
          }
      }
      if (s.graph_pull) s.pulled_bytes = pulled * 256;   // (walker form: the threads' bytes are counted where they copy)
    }
  }
  *out = s;
  return BANG_OK;
}

extern "C" int bang_get_stats_ext(bang_engine_t* e, bang_stats_ext* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats(e, &out->base));
  out->filter_layout = e->stat_filter_layout;
  return BANG_OK;
}

extern "C" int bang_get_stats_ext2(bang_engine_t* e, bang_stats_ext2* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats_ext(e, &out->ext));
  out->excluded = e->n_excl;
  out->exclude_launches = e->stat_exclude_launches;
  return BANG_OK;
}

extern "C" int bang_get_stats_ext3(bang_engine_t* e, bang_stats_ext3* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats_ext2(e, &out->ext2));
  out->labelled = e->d_labels ? (uint64_t)e->N : 0;
  out->filtered_queries = e->stat_filtered_queries;
  out->label_launches = e->stat_label_launches;
  return BANG_OK;
}

extern "C" int bang_get_stats_ext4(bang_engine_t* e, bang_stats_ext4* out) {
  if (!e || !out) return BANG_ERR_ARG;
  BANG_TRY(bang_get_stats_ext3(e, &out->ext3));
  if (e->allocated && e->stat_range_launches != 0) BANG_TRY(range_counts(e, "bang_get_stats_ext4"));     // (range_truncated needs the batch's counts)
  out->range_hits = e->range_hits > 0 ? (uint64_t)e->range_hits : 0;
  out->range_queries = e->stat_range_queries;
  out->range_launches = e->stat_range_launches;
  out->range_truncated = e->stat_range_launches != 0 ? e->stat_range_truncated : 0;
  return BANG_OK;
}

extern "C" int bang_get_query_counters(bang_engine_t* e, uint32_t* dist_evals, uint32_t* fetched, uint32_t* candidates, uint32_t* iterations) {
  if (!e) return BANG_ERR_ARG;
  if (!e->allocated || e->Qcur <= 0) { bang_set_error("bang_get_query_counters: no query has run on this allocation"); return BANG_ERR_ARG; }
  const size_t Q = (size_t)e->Qcur;
  if (dist_evals || fetched) {
    std::vector<uint32_t> qs(Q * 2);
    HIP_TRY(hipMemcpy(qs.data(), e->d_qstats, qs.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < Q; ++i) { if (dist_evals) dist_evals[i] = qs[2 * i]; if (fetched) fetched[i] = qs[2 * i + 1]; }
  }
  if (candidates) HIP_TRY(hipMemcpy(candidates, e->d_cand_cnt, Q * 4, hipMemcpyDeviceToHost));
  if (iterations) {
    if (one_launch(e) && e->h_qiters.size() >= Q) memcpy(iterations, e->h_qiters.data(), Q * 4);
    else memset(iterations, 0, Q * 4);
  }
  return BANG_OK;
}

extern "C" int bang_get_candidate_log(bang_engine_t* e, uint32_t* ids, uint32_t stride, uint32_t* counts, uint32_t num_queries) {
  if (!e || !ids || !counts) return BANG_ERR_ARG;
  if (!e->allocated || e->Qcur <= 0) { bang_set_error("bang_get_candidate_log: no query has run on this allocation"); return BANG_ERR_ARG; }
  if (stride < e->cand_stride) {
    bang_set_error("bang_get_candidate_log: stride %u < %u (L + %d)", stride, e->cand_stride, e->search_inmem ? BANG_INMEM_EXTRA_ITERS : BANG_EXTRA_ITERS);
    return BANG_ERR_ARG;
  }
  if (num_queries < (uint32_t)e->Qcur) { bang_set_error("bang_get_candidate_log: buffers hold %u queries, the last batch had %d", num_queries, e->Qcur); return BANG_ERR_ARG; }
  const size_t Q = (size_t)e->Qcur;
  HIP_TRY(hipMemcpy(counts, e->d_cand_cnt, Q * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(ids, (size_t)stride * 4, e->d_cand_ids, (size_t)e->cand_stride * 4, (size_t)e->cand_stride * 4, Q, hipMemcpyDeviceToHost));
  return BANG_OK;
}

extern "C" int bang_free_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  if (e->allocated) { (void)hipSetDevice(e->device); free_batch(e); }
  return BANG_OK;
}

extern "C" int bang_unload_e(bang_engine_t* e) {
  if (!e) return BANG_ERR_ARG;
  if (e->allocated) free_batch(e);
  if (e->loaded) { (void)hipSetDevice(e->device); drop_excluded(e); drop_labels(e); dfree(e->d_removed); unload_index(e); }
  return BANG_OK;
}

