// bang_lane.cpp -- bang_query of ONE lane (bang_search.cu:569-1068).  lane_run, at the end of the file, is the sequence of its steps:
//   reset the lane's counters -> the facts of this run (RunFacts: refusals come before anything is enqueued) -> queries H2D + K1 ->
//   the search loop in the allocation's form (e->form, chosen by bang_alloc.cpp resolve_form), one function per form:
//       run_exact / run_lut / run_self_paced / run_host_paced   ONE launch per batch: a bang_search_params built from the shared parts
//                                                               (walk_params, pulled_rows, result_sinks) plus what is the form's own
//       run_per_iteration                                       a front + back launch per iteration (bang_iter_params, fill_params)
//   -> the re-rank launch where the search launch did not write the results (rerank_launch) -> the results' way back (results_back) ->
//   the kernel's abort word and the per-query iteration counts.
// Reference line numbers: /root/reference/BANG_Base/bang_search.cu.
#include "bang_engine.h"

namespace bang {

// ------------------------------------------------------------------ the search loop of one lane
void fill_params(bang_engine* e, const Lane& ln, bang_iter_params& p) {
  const size_t q0 = ln.q0;
  memset(&p, 0, sizeof(p));
  p.Q = ln.nq; p.R = e->R; p.m = e->m; p.L = (uint32_t)e->L; p.medoid = (uint32_t)e->medoid;
  p.psz = e->psz; p.mp = e->mp; p.pq_nhi = e->pq_nhi;
  p.max_wgs = e->front_wgs;
  p.d_stage = (e->stage_mode_eff == 1) ? (e->h_stage_dev ? e->h_stage_dev + q0 * BANG_STAGE_STRIDE : nullptr)
                                        : (e->d_stage ? e->d_stage + q0 * BANG_STAGE_STRIDE : nullptr);
  p.d_seed = e->d_seed;
  p.d_codes = e->d_codes;
  p.code_stride = e->code_stride;
  p.d_pivots_packed = e->pq_nhi ? e->d_pivots_ragged : e->d_pivots_packed;
  p.d_qc = e->d_qc ? e->d_qc + q0 * e->mp * e->psz : nullptr;
  p.d_lut = e->d_lut ? e->d_lut + q0 * e->m * 256 : nullptr;
  p.d_graph = (e->graph_mode == BANG_GRAPH_DEVICE) ? e->d_graph : nullptr;
  p.entry_len = e->entry_len;
  p.vec_bytes = (uint32_t)vec_bytes(e);
  p.d_bloom = e->d_bloom + q0 * BANG_BF_WORDS;
  p.d_nbrs = e->d_nbrs + q0 * BANG_NBR_STRIDE;
  p.d_dist = e->d_dist + q0 * BANG_NBR_STRIDE;
  p.d_cnt = e->d_cnt + q0;
  p.d_wl_ids = e->d_wl_ids + q0 * e->L;
  p.d_wl_dist = e->d_wl_dist + q0 * e->L;
  p.d_wl_vis = e->d_wl_vis + q0 * e->L;
  p.d_wl_cnt = e->d_wl_cnt + q0;
  p.d_mark = e->d_mark + q0;
  p.d_parents = e->d_parents_dev + q0;
  p.d_cand_ids = e->d_cand_ids + q0 * e->cand_stride;
  p.d_cand_row = e->d_cand_row ? e->d_cand_row + q0 * e->cand_stride : nullptr;
  p.d_cand_cnt = e->d_cand_cnt + q0;
  p.d_active = nullptr;
  p.d_qstats = e->d_qstats + q0 * 2;
  if (e->graph_mode != BANG_GRAPH_DEVICE && e->use_flag) {
    p.d_done_count = e->d_done_count + (size_t)ln.index * 16;
    p.h_done_flag = e->h_done_dev + (size_t)ln.index * 16;
    p.h_parents = e->d_parents_map + q0;
  }
}

// slot for the in-kernel {start,end} stamps of the next front launch ("timing"=1), or NULL
unsigned long long* ktime_slot(bang_engine* e, Lane& ln) {
  if (!e->timing || !ln.d_ktime || ln.kt_used >= ln.kt_launches) return nullptr;
  return ln.d_ktime + (ln.kt_used++) * KT_WGS * 2;
}

static int g_dbg = -1;
#define DBG(...) do { if (g_dbg < 0) g_dbg = env_flag("BANG_DEBUG") ? 1 : 0; if (g_dbg) { fprintf(stderr, __VA_ARGS__); fflush(stderr); } } while (0)

// host time spent enqueueing (bang_stats.enqueue_ms): a function that brackets its launches declares ENQ_CLOCK() first
#define ENQ_CLOCK() auto t_enq = Clock::now()
#define ENQ_BEGIN() (t_enq = Clock::now())
#define ENQ_END() (ln.enqueue_ms += ms_since(t_enq))

// diagnostic (BANG_TIMELINE=1): host time of every stage of one bang_query, with a stream sync behind each (stderr)
struct Timeline {
  const bool on = env_flag("BANG_TIMELINE");
  Clock::time_point t = Clock::now();
  void stage(const Lane& ln, const char* what) {
    if (!on) return;
    (void)hipStreamSynchronize(ln.s_main);
    fprintf(stderr, "[timeline lane %d] %-28s %8.1f us\n", ln.index, what, ms_since(t) * 1000.0);
    t = Clock::now();
  }
};

// ------------------------------------------------------------------ the facts of one run, derived once and handed to the steps
struct RunFacts {
  int Q;                       // queries of the whole bang_query; this lane runs [ln.q0, ln.q0 + ln.nq)
  bool dev_graph;
  uint32_t dim_adjust;         // MIPS: the queries come without the padding dimension (:631)
  size_t vb;                   // bytes of a full-precision vector
  uint32_t cap_iter;           // the walk's iteration cap (:950; semantics = 1: L + 119)
  bool masked;                 // ids are excluded (bang_set_excluded_e)
  bool fused_rerank;           // K6 + K7 inside the self-paced search launch: no launch behind it
  bool results_in_launch;      // ... or the exact-distance kernel: the search launch writes the results itself
  bool whole;                  // this lane runs the whole batch
  bool to_device;              // bang_query_dev_e: no result leaves the device
  bool mailbox;                // the results return through the pinned mirror, in one copy
  bool results_direct;         // ... or without one: the search launch writes them into the mirror itself
};

static int derive_facts(bang_engine* e, const Lane& ln, int Q, RunFacts& r) {
  r.Q = Q;
  r.dev_graph = (e->graph_mode == BANG_GRAPH_DEVICE);
  r.dim_adjust = (e->distfn == BANG_DIST_MIPS) ? 1u : 0u;
  r.vb = vec_bytes(e);
  r.cap_iter = (uint32_t)e->L + (e->search_inmem ? BANG_INMEM_EXTRA_ITERS : BANG_EXTRA_ITERS) - 1;
  // K6 + K7 inside the search launch (8-bit vectors, self-paced form): no launch behind it
  // (an fp16 vector table, option vectors_fp16, is read by the re-rank launch only)
  // excluded ids (bang_set_excluded_e): the walk runs as ever; the re-rank is a launch of its own on the log without its excluded
  // entries (PQ walks), the exact-distance kernel hands over its whole worklist (rr_k = L) and bang_k_worklist_pick takes the first k live entries
  r.masked = e->n_excl != 0 && e->d_excl != nullptr;
  r.fused_rerank = !r.masked && e->form == LoopForm::SelfPaced && e->fuse_rerank != 0 && (r.dev_graph || e->vec_on_device) && !e->vecs_f16 &&
                   bang_search_can_rerank(e->dtype, e->D, r.dev_graph ? e->entry_len : r.vb, r.dim_adjust) != 0;
  // distance = 1: the exact-distance kernel writes the results itself, as the fused re-rank does (no launch behind it)
  r.results_in_launch = r.fused_rerank || e->form == LoopForm::Exact;
  // semantics = 1: the separate re-rank launch holds at most BANG_MAX_L + 50 candidates per query, and the log may hold L + 120
  if (e->search_inmem && !r.fused_rerank && e->cand_stride > BANG_MAX_L + BANG_EXTRA_ITERS) {
    bang_set_error("option semantics = 1 (inmemory) at L = %d needs the fused re-rank (fuse_rerank != 0 and a vector layout it evaluates): the separate "
                   "re-rank holds %d candidates per query", e->L, BANG_MAX_L + BANG_EXTRA_ITERS);
    return BANG_ERR_UNSUPPORTED;
  }
  if (e->form == LoopForm::Exact && r.dim_adjust != 0) { bang_set_error("option distance = 1 (exact) supports L2 distance only (no MIPS)"); return BANG_ERR_UNSUPPORTED; }
  r.whole = ln.q0 == 0 && (int)ln.nq == Q && (int)ln.nq == e->Qcur;
  const size_t mailbox_max = (size_t)env_long("BANG_MAILBOX_BYTES", BANG_RESULT_MAILBOX_BYTES);
  r.to_device = e->pool.d_ids_user != nullptr;
  r.mailbox = !r.to_device && r.whole && e->res_off_iters <= mailbox_max;
  // ... and with the re-rank fused into the search launch the kernel writes ids, distances, iteration counts and its abort word straight
  // into that pinned mirror (posted PCIe writes, a query at a time as the queries finish): nothing is copied behind the launch
  r.results_direct = !r.masked && r.mailbox && r.results_in_launch && e->h_results_dev != nullptr && env_long("BANG_RESULTS_DIRECT", 1) != 0;
  return BANG_OK;
}

// the lane's word for the search kernel's abort code, behind the results in the pinned mirror (one word per lane)
static uint32_t* abort_word(uint8_t* results, const bang_engine* e, const Lane& ln) {
  return (uint32_t*)(results + e->res_bytes - BANG_MAX_LANES * 4) + ln.index;
}

// ------------------------------------------------------------------ the shared parts of a one-launch form's bang_search_params
// the walk: what every one-launch form hands its kernel -- the lane's queue and abort words zeroed, its slices of the per-query state, the
// timing slot and the experiment / test knobs of the launch shape
static int walk_params(bang_engine* e, Lane& ln, const RunFacts& r, const bang_iter_params& p, bang_search_params& sp) {
  LANE_HIP(hipMemsetAsync(ln.d_pcnt, 0, 64, ln.s_main));
  memset(&sp, 0, sizeof(sp));
  sp.Q = ln.nq; sp.R = e->R; sp.m = e->m; sp.L = (uint32_t)e->L; sp.medoid = (uint32_t)e->medoid; sp.cap_iter = r.cap_iter;
  sp.d_seed = e->d_seed;
  sp.d_bloom = p.d_bloom; sp.d_cand_ids = p.d_cand_ids; sp.d_cand_cnt = p.d_cand_cnt; sp.d_qstats = p.d_qstats;
  sp.d_qiters = e->d_qiters + ln.q0; sp.d_next_query = ln.d_pcnt; sp.d_abort = ln.d_pcnt + 1;
  sp.d_ktime = ktime_slot(e, ln);
  sp.max_wgs = (uint32_t)std::max(0L, env_long("BANG_SEARCH_MAX_WGS", 0));
  sp.max_waves = (uint32_t)std::max(0L, env_long("BANG_SEARCH_MAX_WAVES", 0));
  return BANG_OK;
}

// graph in host RAM, adjacency rows pulled by the kernel (bang_alloc: pull = 1, vectors resident): the 256-byte rows in mapped host memory, the
// HBM copy of the first rows and the node's slice table
static void pulled_rows(const bang_engine* e, bang_search_params& sp) {
  sp.d_graph = (const uint8_t*)e->d_adj; sp.entry_len = 256; sp.row_layout = 1;
  sp.d_rows_hbm = e->d_rows_hbm; sp.n_rows_hbm = rows_direct(e);      // (a moved slice is only reachable through the table)
  sp.n_rows_pad = e->n_rows_pad;                                      // (padded rows: the self-paced PQ form alone -- bang_alloc gave them up or refused for every other)
  if (e->n_slices > 1 && e->d_slice_tab) { sp.d_row_slices = e->d_slice_tab; sp.n_slices = e->n_slices; sp.slice_rows = e->slice_rows; }
}

// where a launch that writes the results itself puts them: the engine's result block, the caller's device buffers (bang_query_dev_e), or --
// results_direct -- the pinned mirror, iteration counts and abort word included
static void result_sinks(bang_engine* e, const Lane& ln, const RunFacts& r, bang_search_params& sp) {
  sp.rr_queries = e->d_queries;
  sp.rr_dtype = (uint32_t)e->dtype; sp.rr_D = e->D; sp.rr_k = (uint32_t)e->k; sp.rr_q0 = ln.q0; sp.rr_Q_total = (uint32_t)r.Q;
  sp.rr_ids_out = e->d_ids_out; sp.rr_dists_out = e->d_dists_out;
  if (r.to_device && r.whole) {
    sp.rr_ids_out = e->pool.d_ids_user;
    if (e->pool.d_dists_user) sp.rr_dists_out = e->pool.d_dists_user;
  }
  if (r.results_direct) {
    sp.rr_ids_out = (uint64_t*)e->h_results_dev; sp.rr_dists_out = (float*)(e->h_results_dev + e->res_off_dists);
    sp.d_qiters = (uint32_t*)(e->h_results_dev + e->res_off_iters) + ln.q0;
    sp.d_abort = abort_word(e->h_results_dev, e, ln);
  }
}

// ------------------------------------------------------------------ diagnostic (BANG_SEARCH_PROF=1): a 128-byte record per workgroup of the PQ search kernel
static int prof_begin(Lane& ln, uint32_t G, bang_search_params& sp) {
  if (!env_flag("BANG_SEARCH_PROF")) return BANG_OK;
  unsigned long long* d_prof = nullptr;
  LANE_HIP(hipMalloc((void**)&d_prof, (size_t)G * 128));
  LANE_HIP(hipMemsetAsync(d_prof, 0, (size_t)G * 128, ln.s_main));
  sp.d_prof = d_prof;
  return BANG_OK;
}

// the records of the finished launch, [G][16] (empty: not asked for), behind the line of a diagnostic build (-DBANG_SEARCH_PHASE_PROF): per-iteration
// phase times of wave 0 of every workgroup, slots [8..15] of its record
static std::vector<unsigned long long> prof_end(const Lane& ln, uint32_t G, const bang_search_params& sp) {
  std::vector<unsigned long long> pr;
  if (!sp.d_prof) return pr;
  pr.resize((size_t)G * 16);
  (void)hipStreamSynchronize(ln.s_main);
  (void)hipMemcpy(pr.data(), sp.d_prof, pr.size() * 8, hipMemcpyDeviceToHost);
  (void)hipFree(sp.d_prof);
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t w = 0; w < G; ++w) for (int k = 0; k < 8; ++k) a[k] += (double)pr[(size_t)w * 16 + 8 + k];
  if (a[7] <= 0) return pr;
  const double n = a[7];
  double x[3] = {0, 0, 0};                     // self-paced form: [0] hand-over (row request), [1] worklist head, [2] summary marks -- split off phases 6 / 0
  for (uint32_t w = 0; w < G; ++w) for (int k = 0; k < 3; ++k) x[k] += (double)pr[(size_t)w * 16 + k];
  fprintf(stderr, "[search] phases of an iteration (wave 0 of %u workgroups, %.0f iterations each): row arrival + loop %.2f us, hashes + probes %.2f, "
                  "compaction %.2f, filter update %.2f, code rows + distances %.2f, parent %.2f, publish + sort/merge %.2f (self-paced, split off: hand-over %.2f, "
                  "worklist head %.2f, summary marks %.2f)\n", G, n / G,
          a[0] * 0.01 / n, a[1] * 0.01 / n, a[2] * 0.01 / n, a[3] * 0.01 / n, a[4] * 0.01 / n, a[5] * 0.01 / n, a[6] * 0.01 / n, x[0] * 0.01 / n, x[1] * 0.01 / n,
          x[2] * 0.01 / n);
  return pr;
}

// ------------------------------------------------------------------ the forms of the search loop
// distance = 1: ONE launch of the exact-distance search kernel; it writes the results itself
static int run_exact(bang_engine* e, Lane& ln, const RunFacts& r, const bang_iter_params& p) {
  ENQ_CLOCK();
  bang_search_params sp;
  BANG_TRY(walk_params(e, ln, r, p, sp));
  sp.n_nodes = e->N;
  sp.d_graph = e->d_graph; sp.entry_len = e->entry_len; sp.vec_bytes = (uint32_t)r.vb;
  if (!r.dev_graph) {                                                 // (vec_bytes stays: the vectors come from the packed table in HBM)
    pulled_rows(e, sp);
    sp.rr_vec_base = e->d_vecs; sp.rr_vec_stride = vec_table_stride(e); sp.rr_vec_f16 = e->vecs_f16 ? 1u : 0u;
  }
  result_sinks(e, ln, r, sp);
  // per-query label filters (bang_set_query_filters_e): the kernel collects the results itself, from every node the walk evaluates,
  // and tests the exclusion bitmap on the way -- no pick behind it
  const bool filtered = e->n_qfilters != 0;
  // excluded ids otherwise: the launch hands over the whole final worklist, [Q][L] / [L][Q], and the pick that follows writes the first k live
  // entries where the launch would have (never the pinned mirror: results_direct is off whenever ids are excluded)
  const bool picked = r.masked && !filtered;
  uint64_t* pick_ids = sp.rr_ids_out;
  float* pick_dists = sp.rr_dists_out;
  if (picked) { sp.rr_k = (uint32_t)e->L; sp.rr_ids_out = e->d_wl_ids_full; sp.rr_dists_out = e->d_wl_dists_full; }
  e->rerank_fused = false;
  ENQ_BEGIN();
  // per-query radii (bang_set_query_radii_e): the same walk and the same results -- the pick behind the launch included -- and the
  // hit log beside them, sorted and de-duplicated behind the launch
  const bool ranged = e->n_radii != 0;
  if (ranged) {
    bang_range_out ro;
    ro.d_radius = e->d_radius; ro.d_excluded = r.masked ? e->d_excl : nullptr; ro.d_hit_ids = e->d_hit_ids; ro.d_hit_dists = e->d_hit_dists;
    ro.d_offered = e->d_offered; ro.cap = (uint32_t)e->range_hits;
    BANG_TRY(bang_k_search_exact_range(&sp, &ro, ln.s_main));
    ++ln.range_launches;
  } else if (filtered) {
    bang_label_filter lf;
    lf.d_labels = e->d_labels; lf.d_filters = e->d_qfilters; lf.d_excluded = r.masked ? e->d_excl : nullptr; lf.d_matched = e->d_matched;
    BANG_TRY(bang_k_search_exact_labels(&sp, &lf, ln.s_main));
    ++ln.label_launches;
  } else if (e->beam > 1) BANG_TRY(bang_k_search_exact_beam(&sp, (uint32_t)e->beam, ln.s_main));   // up to beam parents per iteration (bang_search_beam.hip)
  else BANG_TRY(bang_k_search_exact(&sp, ln.s_main));
  if (picked) {
    BANG_TRY(bang_k_worklist_pick(e->d_wl_ids_full, e->d_wl_dists_full, (uint32_t)e->L, ln.q0, ln.nq, (uint32_t)r.Q, e->d_excl, e->N, (uint32_t)e->k,
                                  pick_ids, pick_dists, ln.s_main));
    ++ln.exclude_launches;
  }
  if (ranged) BANG_TRY(bang_k_range_sort(e->d_hit_ids, e->d_hit_dists, e->d_offered, (uint32_t)e->range_hits, ln.q0, ln.nq, (uint32_t)r.Q, e->d_range_count, ln.s_main));
  ENQ_END();
  ++ln.front_launches;
  return BANG_OK;
}

// LUT path, graph in HBM: ONE launch of the LUT-path search kernel behind K1; its candidate log feeds the re-rank launch (no rr_* field is set)
static int run_lut(bang_engine* e, Lane& ln, const RunFacts& r, const bang_iter_params& p) {
  ENQ_CLOCK();
  bang_search_params sp;
  BANG_TRY(walk_params(e, ln, r, p, sp));
  sp.n_nodes = e->N;
  sp.d_codes = e->d_codes; sp.code_stride = e->code_stride; sp.d_lut = p.d_lut;
  sp.d_graph = e->d_graph; sp.entry_len = e->entry_len; sp.vec_bytes = (uint32_t)r.vb;
  e->rerank_fused = false;
  ENQ_BEGIN();
  BANG_TRY(bang_k_search_lut(&sp, ln.s_main));
  ENQ_END();
  ++ln.front_launches;
  return BANG_OK;
}

// graph in HBM, or its adjacency rows pulled by the kernel: ONE launch of the query-resident PQ search kernel; no host involvement until the re-rank
static int run_self_paced(bang_engine* e, Lane& ln, const RunFacts& r, const bang_iter_params& p) {
  ENQ_CLOCK();
  bang_search_params sp;
  BANG_TRY(walk_params(e, ln, r, p, sp));
  sp.n_nodes = e->N;
  sp.psz = e->psz; sp.mp = e->mp; sp.pq_nhi = e->pq_nhi;
  sp.d_codes = e->d_codes; sp.code_stride = e->code_stride; sp.d_pivots_packed = p.d_pivots_packed; sp.d_qc = p.d_qc;
  sp.d_graph = e->d_graph; sp.entry_len = e->entry_len; sp.vec_bytes = (uint32_t)r.vb;
  if (!r.dev_graph) { pulled_rows(e, sp); sp.vec_bytes = 0; }        // (the walk reads no vector: only the fused re-rank does, from d_vecs)
  sp.d_qskip = e->d_qskip + ln.q0;
  sp.spec_rows = (uint32_t)std::min(2L, std::max(0L, env_long("BANG_SPEC_ROWS", 0)));
  e->rerank_fused = r.fused_rerank;
  if (r.fused_rerank) {                                               // K6 + K7 by the wave that finishes the query: no launch behind this one
    result_sinks(e, ln, r, sp);
    sp.rr_vec_base = r.dev_graph ? e->d_graph : e->d_vecs; sp.rr_vec_stride = r.dev_graph ? e->entry_len : r.vb;
  }
  { const long si = env_long("BANG_SUMM_ITERS", 0); sp.summ_iters = si < 0 ? 0xFFFFFFFFu : (uint32_t)si; }     // 0 = auto, -1 = always
  const uint32_t G = (uint32_t)std::min<int>((int)ln.nq, bang_num_cus());
  BANG_TRY(prof_begin(ln, G, sp));                                    // (phase times: diagnostic build only)
  ENQ_BEGIN();
  BANG_TRY(e->search_inmem ? bang_k_search_inmem(&sp, ln.s_main) : e->search_wordfilter ? bang_k_search_wf(&sp, ln.s_main) : bang_k_search(&sp, ln.s_main));
  ENQ_END();
  ++ln.front_launches;
  (void)prof_end(ln, G, sp);
  return BANG_OK;
}

// graph in host RAM: ONE launch of the host-paced form of that kernel; its workgroups are served round by round by the walker team.  The launch
// shape is fixed HERE (the pacing state is laid out for it) and handed to the kernel as max_wgs / max_waves; no graph, node count or filter
// summary goes in, and the launch is not counted into enqueue_ms
static int run_host_paced(bang_engine* e, Lane& ln, const RunFacts& r, const bang_iter_params& p) {
  bang_search_params sp;
  BANG_TRY(walk_params(e, ln, r, p, sp));
  uint32_t G = 0, W = 0;
  uint32_t C = (uint32_t)std::max(0L, env_long("BANG_SEARCH_CTX", 0)), GS = (uint32_t)std::max(0L, env_long("BANG_SEARCH_GS", 0));
  BANG_TRY(bang_search_geometry(e->psz, e->mp, e->pq_nhi, (uint32_t)e->L, ln.nq, sp.max_wgs, sp.max_waves, 1, &G, &W, &C, &GS));   // (the knobs bound the geometry)
  e->sv_C = C; e->sv_GS = GS;
  e->sv_NG = G * ((W + GS - 1) / GS) * C;
  if (e->sv_NG > 8 * KT_WGS) { bang_set_error("search kernel: %u pacing groups exceed the pacing buffers", e->sv_NG); return BANG_ERR_ARG; }
  e->sv_G = G; e->sv_W = W;
  const uint32_t NG = e->sv_NG;                                              // pacing groups
  for (size_t i = 0; i < (size_t)NG * 16; ++i) e->h_parents[i] = BANG_NO_PARENT;
  ln.pw_groups = NG;
  ln.pw_error.store(0);
  for (uint32_t w = 0; w < NG; ++w) ln.pw_expect[w].store(1u, std::memory_order_relaxed);
  ln.pw_remaining.store(NG, std::memory_order_release);
  for (uint32_t w = 0; w < NG; ++w) { e->h_done[(size_t)w * 16] = 0; e->d_sctl[(size_t)w * 16] = 0; }
  _mm_sfence();
  sp.psz = e->psz; sp.mp = e->mp; sp.pq_nhi = e->pq_nhi;
  sp.max_wgs = G; sp.max_waves = W; sp.nctx = e->sv_C; sp.group_waves = e->sv_GS;
  sp.d_codes = e->d_codes; sp.code_stride = e->code_stride; sp.d_pivots_packed = p.d_pivots_packed; sp.d_qc = p.d_qc;
  sp.d_graph = nullptr; sp.entry_len = e->entry_len; sp.vec_bytes = (uint32_t)r.vb;
  // walker-from-rows: parents whose row sits in this GPU's HBM copy of the first rows are served by the kernel itself
  e->walker_self = e->walker_rows && e->d_rows_hbm && e->rows_first == 0 && e->n_rows_pad == 0 && env_long("BANG_WALKER_SELF_ROWS", 1) != 0;
  if (e->walker_self) { sp.d_rows_hbm = e->d_rows_hbm; sp.n_rows_hbm = e->n_rows_hbm; }
  sp.d_rows = e->d_srows; sp.d_ctl = e->d_sctl; sp.h_done = e->h_done_dev; sp.h_parents = e->d_parents_map;
  sp.h_pub_q = e->d_pub_q; sp.h_pub_c = e->d_pub_c; sp.ship_vectors = e->vec_on_device ? 0u : 1u;
  sp.go_timeout_ticks = (unsigned long long)e->kernel_go_timeout_ms * 100000ull;
  BANG_TRY(prof_begin(ln, G, sp));                                           // (phase times of the half-rounds)
  BANG_TRY(bang_k_search(&sp, ln.s_main));
  ++ln.front_launches;
  const auto t0 = Clock::now();
  const int T = 1 + (int)ln.helpers.size();
  if (e->walker_stall_ms > 0) {                // test hook: nobody serves the kernel for a while (one shot)
    std::this_thread::sleep_for(std::chrono::milliseconds(e->walker_stall_ms));
    e->walker_stall_ms = 0;
  }
  ln.job_kind = 2;
  if (T > 1) {
    ln.pending.store((uint32_t)(T - 1), std::memory_order_relaxed);
    ln.epoch.fetch_add(1, std::memory_order_release);
  }
  swalk(e, ln, 0, T);
  if (T > 1) while (ln.pending.load(std::memory_order_acquire) != 0) _mm_pause();
  ln.walker_ms += ms_since(t0);
  if (ln.pw_error.load()) {
    // one side of the hand-shake gave up: the kernel has been stopped through its control lines (or has left by itself)
    (void)hipStreamSynchronize(ln.s_main);
    uint32_t gave_up = 0;
    (void)hipMemcpy(&gave_up, ln.d_pcnt + 1, 4, hipMemcpyDeviceToHost);
    if (gave_up) bang_set_error("the search kernel gave up waiting for the host walker (kernel_go_timeout_ms = %d)", e->kernel_go_timeout_ms);
    else bang_set_error("the walker gave up waiting for the search kernel (host_walk_timeout_ms = %d)", e->host_walk_timeout_ms);
    return BANG_ERR_HIP;
  }
  const std::vector<unsigned long long> pr = prof_end(ln, G, sp);
  if (!pr.empty()) {
    double a[5] = {0, 0, 0, 0, 0};
    for (uint32_t w = 0; w < G; ++w) for (int k = 0; k < 5; ++k) a[k] += (double)pr[(size_t)w * 16 + k];
    const double n = a[4] > 0 ? a[4] : 1;
    fprintf(stderr, "[search] %u workgroups x %u waves x %u contexts, %u waves per pacing group: %.0f half-rounds per group; per half-round: wait for rows %.2f us, "
                    "front (to the publish barrier) %.2f us, publish %.2f us, sort/merge %.2f us\n", G, W, e->sv_C, e->sv_GS, a[4] / G,
            a[0] * 0.01 / n, a[1] * 0.01 / n, a[2] * 0.01 / n, a[3] * 0.01 / n);
  }
  if (!e->fp_direct && !e->vec_on_device)     // vectors staged in pinned memory: one copy of this lane's part of the log
    LANE_HIP(hipMemcpyAsync(e->d_fp + (size_t)ln.q0 * e->cand_stride * r.vb, e->h_fp + (size_t)ln.q0 * e->cand_stride * r.vb,
                            (size_t)ln.nq * e->cand_stride * r.vb, hipMemcpyHostToDevice, ln.s_main));
  return BANG_OK;
}

// a front + back launch per iteration (graph in HBM, or walked by the C++ walker between the two).  *iters: the iterations run; *fp_copied: rows
// of the vector log went to the device on the lane's second stream, which the re-rank has to wait for
static int run_per_iteration(bang_engine* e, Lane& ln, const RunFacts& r, bang_iter_params& p, uint32_t* iters, bool* fp_copied) {
  ENQ_CLOCK();
  const bool dev_graph = r.dev_graph;
  const uint32_t cap_iter = r.cap_iter;
  uint32_t iter = 1;                                                         // :596
  // Straggler compaction: most queries finish after ~L+5 iterations but the batch runs until its last query does (up to
  // L+49).  Once at most half of a lane's queries are active the kernels iterate over a slot -> query map of the active
  // ones only; finished queries never change state again, so skipping them cannot change any result.
  auto set_qmap = [&](const uint32_t* parents, uint32_t active, uint32_t buf) {
    if (!e->compact || active == 0 || active * 2 > ln.nq) { p.d_qmap = nullptr; p.Q = ln.nq; return; }
    uint32_t* dst = ln.qmap_host[buf];
    uint32_t n = 0;
    for (uint32_t i = 0; i < ln.nq; ++i)
      if (parents[i] != BANG_NO_PARENT) dst[n++] = i;
    if (ln.qmap_is_device) _mm_sfence();
    p.d_qmap = ln.qmap_dev[buf];
    p.Q = n;
  };
  // vector-log rows [fp_lo, fp_hi] are staged in pinned memory but not yet copied to the device
  uint32_t fp_lo = 0, fp_hi = 0;
  bool fp_pending = false;
  auto note_fp = [&](uint32_t n_par) {                                       // the walker staged the vectors of this iteration's parents
    if (!n_par || e->vec_on_device) return;
    if (!fp_pending) { fp_lo = iter; fp_pending = true; }
    fp_hi = iter;
  };
  auto flush_fp = [&]() -> int {                                             // :836-838, batched
    if (!fp_pending) return BANG_OK;
    const size_t off = ((size_t)fp_lo * e->Qcur + ln.q0) * r.vb;
    LANE_HIP(hipMemcpy2DAsync(e->d_fp + off, (size_t)e->Qcur * r.vb, e->h_fp + off, (size_t)e->Qcur * r.vb,
                              (size_t)ln.nq * r.vb, (size_t)(fp_hi - fp_lo + 1), hipMemcpyHostToDevice, ln.s_fp));
    fp_pending = false;
    *fp_copied = true;
    return BANG_OK;
  };

  p.first = 1; p.iter = iter; p.done_value = iter;
  if (dev_graph) p.d_active = e->d_active + iter;
  p.d_ktime = ktime_slot(e, ln);
  BANG_TRY(bang_k_front(&p, ln.s_main));                                     // K5+K2+K4a :650-678
  ++ln.front_launches;

  for (;;) {
    p.first = 0; p.iter = iter;
    ENQ_BEGIN();
    BANG_TRY(bang_k_back(&p, ln.s_main));                                    // K3a+K3b :726-738 (overlaps the walker)
    ENQ_END();
    if (!dev_graph) {
      DBG("[lane %d] wait flag %u\n", ln.index, iter);
      BANG_TRY(wait_flag(e, ln, iter));                                      // parents of this iteration are in h_parents :709,763
      DBG("[lane %d] got flag %u\n", ln.index, iter);
      const auto t0 = Clock::now();
      uint32_t n_par = 0;
      const uint32_t active = walk(e, ln, iter, true, &n_par);               // CPU walker :771-813
      ln.walker_ms += ms_since(t0);
      note_fp(n_par);
      if (active == 0) break;                                                // :958
      set_qmap(e->h_parents + ln.q0, active, (iter + 1) & 1u);
      ENQ_BEGIN();
      if (e->stage_mode_eff == 0)
        LANE_HIP(hipMemcpyAsync((void*)(e->d_stage + (size_t)ln.q0 * BANG_STAGE_STRIDE), e->h_stage + (size_t)ln.q0 * BANG_STAGE_STRIDE,
                                (size_t)ln.nq * BANG_STAGE_STRIDE * 4, hipMemcpyHostToDevice, ln.s_main));   // :827-833
      ENQ_END();
      if (fp_pending && fp_hi - fp_lo + 1 >= (uint32_t)e->fp_batch) { ENQ_BEGIN(); BANG_TRY(flush_fp()); ENQ_END(); }
    }
    ++iter;                                                                  // :879
    p.iter = iter; p.done_value = iter;
    if (dev_graph) p.d_active = e->d_active + iter;
    ENQ_BEGIN();
    p.d_ktime = ktime_slot(e, ln);
    BANG_TRY(bang_k_front(&p, ln.s_main));                                   // K5+K2+K4b :855-917
    ++ln.front_launches;
    ENQ_END();
    if (!dev_graph) {
      if (iter == cap_iter) {                                                // :950-956
        // CANON: the vectors of the parents chosen at the cap are still fetched for the re-rank
        BANG_TRY(wait_flag(e, ln, iter));
        uint32_t n_par = 0;
        (void)walk(e, ln, iter, false, &n_par);
        note_fp(n_par);
        break;
      }
    } else {
      if (iter == cap_iter) break;
      if ((iter % (uint32_t)e->check_every) == 0) {                          // :942-943 (amortised)
        uint32_t act = 0;
        LANE_HIP(hipMemcpyAsync(&act, e->d_active + iter, 4, hipMemcpyDeviceToHost, ln.s_main));
        LANE_HIP(hipStreamSynchronize(ln.s_main));
        if (act == 0) break;
        if (e->compact) {                                                    // refresh the slot -> query map from the parents
          if (ln.parents_tmp.size() < ln.nq) ln.parents_tmp.resize(ln.nq);
          LANE_HIP(hipMemcpy(ln.parents_tmp.data(), e->d_parents_dev + ln.q0, (size_t)ln.nq * 4, hipMemcpyDeviceToHost));
          uint32_t n_act = 0;
          for (uint32_t i = 0; i < ln.nq; ++i) n_act += ln.parents_tmp[i] != BANG_NO_PARENT;
          set_qmap(ln.parents_tmp.data(), n_act, 0);
        }
      }
    }
  }
  *iters = iter;
  return flush_fp();
}

// ------------------------------------------------------------------ behind the search loop
// re-rank K6+K7 (:967-987) as a launch of its own, from the candidate log -- with ids excluded, from the log without its excluded entries, in log
// order (the log itself stays the walk's; bang_alloc refuses excluded ids where the vectors travel in a log)
static int rerank_launch(bang_engine* e, Lane& ln, const RunFacts& r) {
  const int Q = r.Q;
  const uint32_t dim_adjust = r.dim_adjust;
  const uint32_t* rr_ids = e->d_cand_ids;
  const uint32_t* rr_cnt = e->d_cand_cnt;
  if (r.masked) {
    BANG_TRY(bang_k_cand_live(e->d_cand_ids, e->d_cand_cnt, e->cand_stride, ln.q0, ln.nq, e->d_excl, e->N, e->d_live_ids, e->d_live_cnt, ln.s_main));
    ++ln.exclude_launches;
    rr_ids = e->d_live_ids; rr_cnt = e->d_live_cnt;
  }
  if (r.dev_graph)
    BANG_TRY(bang_k_rerank_range(e->d_graph, e->entry_len, e->d_medoid_vec, e->d_queries, e->dtype, rr_ids,
                                 nullptr, rr_cnt, e->cand_stride, ln.q0, ln.nq, (uint32_t)Q, e->D,
                                 (uint32_t)e->k, dim_adjust, e->d_ids_out, e->d_dists_out, ln.s_main));
  else if (e->vec_on_device && e->vecs_f16)
    BANG_TRY(bang_k_rerank_f16_range(e->d_vecs, vec_table_stride(e), e->d_queries, rr_ids, rr_cnt, e->cand_stride, ln.q0, ln.nq,
                                     (uint32_t)Q, e->D, (uint32_t)e->k, dim_adjust, e->d_ids_out, e->d_dists_out, ln.s_main));
  else if (e->vec_on_device)
    BANG_TRY(bang_k_rerank_range(e->d_vecs, r.vb, e->d_medoid_vec, e->d_queries, e->dtype, rr_ids, nullptr, rr_cnt,
                                 e->cand_stride, ln.q0, ln.nq, (uint32_t)Q, e->D, (uint32_t)e->k, dim_adjust, e->d_ids_out,
                                 e->d_dists_out, ln.s_main));
  else if (e->form == LoopForm::HostPaced)                   // the vector log by query ...
    BANG_TRY(bang_k_rerank_byquery(e->d_fp, r.vb, e->d_medoid_vec, e->d_queries, e->dtype, e->d_cand_ids, e->d_cand_cnt,
                                   e->cand_stride, ln.q0, ln.nq, (uint32_t)Q, e->D, (uint32_t)e->k, dim_adjust, e->d_ids_out,
                                   e->d_dists_out, ln.s_main));
  else                                                       // ... or by iteration
    BANG_TRY(bang_k_rerank_range(e->d_fp, r.vb, e->d_medoid_vec, e->d_queries, e->dtype, e->d_cand_ids, e->d_cand_row,
                                 e->d_cand_cnt, e->cand_stride, ln.q0, ln.nq, (uint32_t)Q, e->D, (uint32_t)e->k,
                                 dim_adjust, e->d_ids_out, e->d_dists_out, ln.s_main));
  return BANG_OK;
}

// results D2H (:997-999): ids [Q][k]; dists [k][Q] (rank-major); a one-launch form's abort word and per-query iteration counts with them.
// A copy into the caller's pageable arrays is staged by the runtime and costs ~20 us before the first byte moves, per copy.  The
// results come back whole in ONE asynchronous copy into the pinned mirror and are handed out with memcpy (measured: 70 -> 17 us for
// a 1 250-query shard, 92-107 -> 73-82 us for the 10 K batch); only a very large batch keeps the direct, runtime-pipelined copies.
// Four ways: left in the caller's device buffers, already in the mirror (results_direct), that one copy, or the pipelined copies.
static int results_back(bang_engine* e, Lane& ln, const RunFacts& r, uint64_t* h_ids, float* h_dists) {
  const int Q = r.Q;
  const bool iters = one_launch(e);
  uint64_t* d_ids_user = e->pool.d_ids_user;
  float* d_dists_user = e->pool.d_dists_user;
  uint8_t* h_iters = e->h_results + e->res_off_iters + (size_t)ln.q0 * 4;
  if (iters && !r.results_direct) LANE_HIP(hipMemcpyAsync(abort_word(e->h_results, e, ln), ln.d_pcnt + 1, 4, hipMemcpyDeviceToHost, ln.s_main));
  if (r.to_device) {
    const bool in_place = r.results_in_launch && r.whole;       // (the fused re-rank / the exact kernel wrote into the caller's buffers)
    if (!in_place)
      LANE_HIP(hipMemcpyAsync(d_ids_user + (size_t)ln.q0 * e->k, e->d_ids_out + (size_t)ln.q0 * e->k, (size_t)ln.nq * e->k * sizeof(uint64_t),
                              hipMemcpyDeviceToDevice, ln.s_main));
    if (d_dists_user && !in_place)
      LANE_HIP(hipMemcpy2DAsync(d_dists_user + ln.q0, (size_t)Q * 4, e->d_dists_out + ln.q0, (size_t)Q * 4, (size_t)ln.nq * 4, (size_t)e->k,
                                hipMemcpyDeviceToDevice, ln.s_main));
    if (iters) LANE_HIP(hipMemcpyAsync(h_iters, e->d_qiters + ln.q0, (size_t)ln.nq * 4, hipMemcpyDeviceToHost, ln.s_main));
  } else if (r.results_direct) {                                // (already there)
  } else if (r.mailbox) {
    LANE_HIP(hipMemcpyAsync(e->h_results, e->d_results, iters ? e->res_off_iters + (size_t)ln.nq * 4 : e->res_off_iters,
                            hipMemcpyDeviceToHost, ln.s_main));
  } else {
    LANE_HIP(hipMemcpyAsync(h_ids + (size_t)ln.q0 * e->k, e->d_ids_out + (size_t)ln.q0 * e->k,
                            (size_t)ln.nq * e->k * sizeof(uint64_t), hipMemcpyDeviceToHost, ln.s_main));
    LANE_HIP(hipMemcpy2DAsync(h_dists + ln.q0, (size_t)Q * 4, e->d_dists_out + ln.q0, (size_t)Q * 4, (size_t)ln.nq * 4,
                              (size_t)e->k, hipMemcpyDeviceToHost, ln.s_main));
    if (iters) LANE_HIP(hipMemcpyAsync(h_iters, e->d_qiters + ln.q0, (size_t)ln.nq * 4, hipMemcpyDeviceToHost, ln.s_main));
  }
  ln.phase.store(6);
  LANE_HIP(hipStreamSynchronize(ln.s_main));
  ln.phase.store(7);
  if (r.mailbox) {
    memcpy(h_ids, e->h_results, (size_t)ln.nq * e->k * sizeof(uint64_t));
    memcpy(h_dists, e->h_results + e->res_off_dists, (size_t)ln.nq * e->k * 4);
  }
  return BANG_OK;
}

// ------------------------------------------------------------------ bang_query of one lane
int lane_run(bang_engine* e, Lane& ln, const void* h_queries, uint64_t* h_ids, float* h_dists, int Q) {
  DBG("[lane %d] start q0=%u nq=%u\n", ln.index, ln.q0, ln.nq);
  LANE_HIP(hipSetDevice(e->device));
  // the lane's counters of the last run
  if (ln.kt_used) { (void)hipMemset(ln.d_ktime, 0, ln.kt_used * KT_WGS * 16); ln.kt_used = 0; }   // stats not collected
  if (e->h_fin.size() >= (size_t)ln.q0 + ln.nq) memset(e->h_fin.data() + ln.q0, 0, ln.nq);
  ln.h2d_bytes.store(0); ln.iterations = 0; ln.front_launches = 0; ln.exclude_launches = 0; ln.label_launches = 0; ln.range_launches = 0; ln.walker_ms = 0; ln.sync_ms = 0; ln.enqueue_ms = 0;
  RunFacts r;
  BANG_TRY(derive_facts(e, ln, Q, r));                                       // (a refusal: nothing is enqueued yet)
  bang_iter_params p;
  fill_params(e, ln, p);
  if (!r.dev_graph) e->h_done[(size_t)ln.index * 16] = 0;
  p.n_all = ln.nq;
  if (!r.dev_graph && e->stagger_us > 0 && ln.index > 0) {
    const auto ts = Clock::now();
    while (ms_since(ts) * 1000.0 < (double)(e->stagger_us * ln.index)) _mm_pause();
  }
  Timeline tl;
  // queries H2D (:612) + K1 (:623)
  const size_t qbytes = (e->D - r.dim_adjust) * e->tsize;
  uint8_t* dq = (uint8_t*)e->d_queries + (size_t)ln.q0 * qbytes;
  LANE_HIP(hipMemcpyAsync(dq, (const uint8_t*)h_queries + (size_t)ln.q0 * qbytes, (size_t)ln.nq * qbytes,
                          hipMemcpyHostToDevice, ln.s_main));
  if (e->form == LoopForm::Exact) {
    // (exact distances: the raw queries are all the kernel needs -- no centring, no K1)
  } else if (e->psz)
    BANG_TRY(bang_k_center_queries(dq, e->dtype, e->d_centroid, e->d_chunk_off, (float*)p.d_qc, ln.nq, e->D, e->m,
                                   e->mp, e->psz, r.dim_adjust, ln.s_main));
  else
    BANG_TRY(bang_k_lut_build(e->d_pivots_T, dq, e->dtype, e->d_centroid, e->d_chunk_off, (float*)p.d_lut, ln.nq,
                              e->D, e->m, r.dim_adjust, ln.s_main));
  tl.stage(ln, "queries H2D + K1");

  // the search loop
  uint32_t* h_abort = abort_word(e->h_results, e, ln);
  *h_abort = 0;
  uint32_t iter = r.cap_iter;                                                // (a one-launch form: refined from the per-query counts below)
  bool fp_copied = false;
  switch (e->form) {
    case LoopForm::Exact: BANG_TRY(run_exact(e, ln, r, p)); break;
    case LoopForm::Lut: BANG_TRY(run_lut(e, ln, r, p)); break;
    case LoopForm::SelfPaced: BANG_TRY(run_self_paced(e, ln, r, p)); break;
    case LoopForm::HostPaced: BANG_TRY(run_host_paced(e, ln, r, p)); break;
    case LoopForm::PerIteration: BANG_TRY(run_per_iteration(e, ln, r, p, &iter, &fp_copied)); break;
  }
  ln.iterations = iter;
  ln.phase.store(5);
  DBG("[lane %d] loop done iter=%u\n", ln.index, iter);
  tl.stage(ln, "search");

  if (fp_copied) {                                                           // the re-rank reads the vector log
    LANE_HIP(hipEventRecord(ln.ev_fp, ln.s_fp));
    LANE_HIP(hipStreamWaitEvent(ln.s_main, ln.ev_fp, 0));
  }
  if (!r.results_in_launch) BANG_TRY(rerank_launch(e, ln, r));
  tl.stage(ln, "re-rank");
  BANG_TRY(results_back(e, ln, r, h_ids, h_dists));
  tl.stage(ln, "results D2H");

  const uint32_t aborted = *h_abort;
  if (aborted == 2u) {
    bang_set_error("search kernel: an adjacency row named a node id out of range (N = %u): the rows were overwritten since bang_load%s%s", e->N,
                   e->rows_path.empty() ? "" : " -- ", e->rows_path.c_str());
    return BANG_ERR_HIP;
  }
  if (aborted) { bang_set_error("search kernel gave up waiting for the host walker"); return BANG_ERR_HIP; }
  if (one_launch(e)) {
    const uint32_t* hq = (const uint32_t*)(e->h_results + e->res_off_iters) + ln.q0;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < ln.nq; ++i) { e->h_qiters[ln.q0 + i] = hq[i]; mx = std::max(mx, hq[i]); }
    ln.iterations = mx;
  }
  DBG("[lane %d] synced\n", ln.index);
  ln.front_ms = ln.back_ms = ln.rerank_ms = 0;   // the in-kernel stamps are reduced lazily in bang_get_stats
  return BANG_OK;
}

}  // namespace bang
