// bang_search_host.cpp -- the host side of the query-resident search kernel (bang_search.hip) and of the PQ layouts its instances are compiled for,
// without a HIP call in it: which layout an index gets and how its pivot table is packed, the argument checks of a launch (search_setup), the grid
// arithmetic (bang_search_geometry), the three measured launch policies (filter summary, wave priority, speculative row request), and the entry
// points bang_k_search / _inmem / _wf, each of which ends in the instance dispatch of its variant's first translation unit (bang_search_args.h).
#include <stdint.h>
#include <string.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_search_args.h"
#include "bang_pad_rows.h"

static const uint32_t kWaveLanes = 64;
namespace bang { const char* env_str(const char* name); }      // bang_options.cpp: environment switches are read when they are used

// ---------------------------------------------------------------------------------------------------------------------
// the PQ layouts (BANG_PQ_LAYOUTS) and their pivot tables
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int bang_pq_layout(const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t* psz_out, uint32_t* mp_out) {
  if (!chunk_off || m == 0 || !psz_out || !mp_out) return BANG_ERR_ARG;
  *psz_out = 0;
  *mp_out = m;
  uint32_t mx = 0;
  for (uint32_t c = 0; c < m; ++c) {
    if (chunk_off[c + 1] < chunk_off[c] || chunk_off[c + 1] > D) { bang_set_error("bad chunk offsets"); return BANG_ERR_ARG; }
    const uint32_t sz = chunk_off[c + 1] - chunk_off[c];
    if (sz > mx) mx = sz;
  }
  const uint32_t psz = mx <= 1 ? 1 : mx <= 2 ? 2 : mx <= 4 ? 4 : mx <= 8 ? 8 : 0;
  if (psz == 0) return BANG_OK;                       // LUT path
  const uint32_t need = (m + 3) / 4;
  uint32_t ndw = 0;                                   // the smallest listed row that holds the chunks
#define PQ_FIT(PSZ, NDW) if (psz == PSZ && NDW >= need && (ndw == 0 || NDW < ndw)) ndw = NDW;
  BANG_PQ_LAYOUTS(PQ_FIT)
#undef PQ_FIT
  if (ndw == 0) return BANG_OK;                       // too many chunks for LDS: LUT path
  *psz_out = psz;
  *mp_out = ndw * 4;
  return BANG_OK;
}

extern "C" int bang_pack_pivots_ragged(const float* pivots, const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t mp,
                                       uint32_t* nhi_out, float* out, uint64_t* floats_out) {
  if (!chunk_off || !nhi_out || m == 0 || mp < m) return BANG_ERR_ARG;
  *nhi_out = 0;
  if (floats_out) *floats_out = 0;
  uint32_t nhi = 0;
  while (nhi < m && chunk_off[nhi + 1] - chunk_off[nhi] == 2) ++nhi;
  if (nhi == 0 || nhi == m) return BANG_OK;                          // no 2-dim prefix, or nothing to save
  for (uint32_t c = nhi; c < m; ++c)
    if (chunk_off[c + 1] - chunk_off[c] > 1) return BANG_OK;       // not of the form 2,..,2,1,..,1
  const uint32_t total = pivot_table_floats(2, mp, nhi);
  *nhi_out = nhi;
  if (floats_out) *floats_out = total;
  if (!out) return BANG_OK;
  if (!pivots) return BANG_ERR_ARG;
  for (uint32_t i = 0; i < total; ++i) out[i] = 0.0f;
  for (uint32_t c = 0; c < m; ++c) {
    const uint32_t sz = chunk_off[c + 1] - chunk_off[c];
    const size_t base = c < nhi ? (size_t)c * 512 : (size_t)nhi * 256 + (size_t)c * 256;
    for (uint32_t code = 0; code < 256; ++code)
      for (uint32_t i = 0; i < sz; ++i) {
        const uint32_t j = chunk_off[c] + i;
        if (j < D) out[base + (size_t)code * (c < nhi ? 2 : 1) + i] = pivots[(size_t)code * D + j];
      }
  }
  return BANG_OK;
}

extern "C" int bang_pack_pivots(const float* pivots, const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t psz,
                                uint32_t mp, float* out) {
  if (!pivots || !chunk_off || !out || psz == 0 || mp < m) return BANG_ERR_ARG;
  for (uint32_t c = 0; c < mp; ++c)
    for (uint32_t code = 0; code < 256; ++code)
      for (uint32_t i = 0; i < psz; ++i) {
        float v = 0.0f;
        if (c < m) {
          const uint32_t j = chunk_off[c] + i;
          if (j < chunk_off[c + 1]) v = pivots[(size_t)code * D + j];
        }
        out[((size_t)c * 256 + code) * psz + i] = v;
      }
  return BANG_OK;
}

// Is there a kernel instance for the exact-size pivot table of this layout (bang_layout_nhi; rows of 70 / 74 chunks, never a multiple of 4)?
extern "C" int bang_ragged_supported(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t m) {
  return (nhi != 0 && (mp & 3u) == 0 && (m & 3u) != 0 && (uint32_t)bang_layout_nhi((int)psz, (int)(mp / 4u)) == nhi) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// which instances exist
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int bang_search_can_rerank(int dtype, uint32_t D, uint64_t vec_stride, uint32_t dim_adjust) {
  const uint32_t G = D >> 4;
  if (dim_adjust != 0 || (vec_stride & 3u) != 0 || D > 256) return 0;
  if (dtype == BANG_F32) return D >= 4 && (D & 3u) == 0;                       // (one lane per candidate: wave_rerank_f32)
  return (dtype == BANG_U8 || dtype == BANG_I8) && D >= 16 && (D & 15u) == 0 && (G & (G - 1u)) == 0;
}

// engine-internal (bang_engine.h): does a semantics = 1 instance exist for this pivot layout and code-row stride?  (launch_al: not for 128-chunk
// rows that are not dword-aligned)
extern "C" int bang_search_inmem_has_instance(uint32_t psz, uint32_t mp, uint32_t code_stride) {
  return (psz != 0 && mp / 4u >= 32u && (code_stride % 4u) != 0u) ? 0 : 1;
}

// does a search_wf_kernel instance exist for this pivot layout and code-row stride?  (every layout of search_dispatch, in both row alignments)
extern "C" int bang_search_wf_has_instance(uint32_t psz, uint32_t mp, uint32_t code_stride) {
  (void)code_stride;
  if (psz == 0 || (mp & 3u)) return 0;
#define WF_HAS(PSZ, NDW) if (psz == PSZ && mp / 4u == NDW) return 1;
  BANG_SEARCH_LAYOUTS(WF_HAS)
#undef WF_HAS
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the grid
// ---------------------------------------------------------------------------------------------------------------------
// waves per workgroup that fit beside the pivot table with nctx query contexts each (0: not even one); the host-paced form also
// keeps its pacing groups' shared words there
static uint32_t waves_that_fit(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t nctx, bool host_paced) {
  const size_t piv_bytes = (size_t)pivot_table_floats(psz, mp, nhi) * 4u;
  const size_t per_wave = (size_t)search_wave_words(L, nctx, (int)(mp / 4u), host_paced) * 4u;
  const size_t cap = (size_t)160 * 1024 - (host_paced ? SRCH_WG_SHARED_BYTES : 0u);
  if (piv_bytes + per_wave > cap) return 0;
  const size_t w = (cap - piv_bytes) / per_wave;
  const size_t most = (size_t)search_maxt((int)(mp / 4u), host_paced) / kWaveLanes;      // what the instance is compiled for
  return (uint32_t)(w > most ? most : w);
}

extern "C" int bang_search_supported(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L) {
  if (psz == 0 || L == 0 || L > BANG_MAX_L) return 0;
  return (int)waves_that_fit(psz, mp, nhi, L, 1, false);            // (the self-paced form; the host-paced one may hold one wave less)
}

// One workgroup per CU at most (the pivot table takes most of the LDS).  A batch smaller than CUs x waves is spread over all
// CUs with fewer waves each: a wave's iteration is latency bound, and fewer waves per CU contend less for LDS and L1.
// Host-paced form: *nctx_io = query contexts per wave (0 = auto = 1), *group_waves_io = waves per pacing group (0 = auto = 8).
extern "C" int bang_search_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs,
                                    uint32_t max_waves, int host_paced, uint32_t* workgroups, uint32_t* waves_out, uint32_t* nctx_io,
                                    uint32_t* group_waves_io) {
  if (!workgroups || !waves_out || !nctx_io || !group_waves_io || Q == 0) return BANG_ERR_ARG;
  if (psz == 0 || L == 0 || L > BANG_MAX_L) { bang_set_error("bad pq layout / L"); return BANG_ERR_ARG; }
  uint32_t nctx = *nctx_io;
  if (!host_paced) nctx = 1;
  else if (nctx == 0) nctx = 1;     // two contexts per wave measured slower (more, emptier half-rounds): kept as an experiment knob
  else if (nctx > 2) nctx = 2;
  if (host_paced && search_maxt((int)(mp / 4u), true) < 1024) nctx = 1;       // (the filter summary lives in registers: one query per wave)
  uint32_t waves = waves_that_fit(psz, mp, nhi, L, nctx, host_paced != 0);
  if (waves == 0) { bang_set_error("pivot table + one wave's worklist do not fit LDS at L=%u", L); return BANG_ERR_UNSUPPORTED; }
  if (max_waves && max_waves < waves) waves = max_waves;
  const uint32_t cus = (uint32_t)bang_num_cus();
  uint32_t grid_n = Q < cus ? Q : cus;
  if (max_wgs && max_wgs < grid_n) grid_n = max_wgs;
  const uint32_t per_wg = ((Q + grid_n - 1) / grid_n + nctx - 1) / nctx;       // waves a workgroup needs to hold its share at once
  if (per_wg < waves) waves = per_wg;
  // A batch of one to two wave-fulls per CU runs as two EQUAL rounds (a full one followed by a nearly empty one keeps the chip a query
  // lifetime longer for a few queries: 4 000 queries 3.75 -> 3.50 ms with 8 waves, 5 000: 4.39 -> 4.28 with 10; three rounds and more: nothing)
  else if (!host_paced && per_wg > waves && per_wg <= 2 * waves) waves = (per_wg + 1) / 2;
  // pacing groups: 8 waves by default, at least 4 (the group-shared LDS area holds 4 groups), the whole workgroup if it is small
  uint32_t gs = *group_waves_io ? *group_waves_io : SRCH_DEFAULT_GROUP_WAVES;
  if (gs > 16) gs = 16;
  if (gs < 4) gs = 4;
  if (gs > waves) gs = waves;
  *workgroups = grid_n;
  *waves_out = waves;
  *nctx_io = nctx;
  *group_waves_io = host_paced ? gs : waves;
  return BANG_OK;
}

// semantics = 1 and filter_layout = 1: the grid is that of the self-paced form of bang_k_search (the same LDS per wave: the candidate log and the
// filter memory are in HBM)
extern "C" int bang_search_inmem_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                                          uint32_t* workgroups, uint32_t* waves) {
  uint32_t nctx = 1, gs = 0;
  return bang_search_geometry(psz, mp, nhi, L, Q, max_wgs, max_waves, 0, workgroups, waves, &nctx, &gs);
}
extern "C" int bang_search_wf_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                                       uint32_t* workgroups, uint32_t* waves) {
  return bang_search_inmem_geometry(psz, mp, nhi, L, Q, max_wgs, max_waves, workgroups, waves);
}

// ---------------------------------------------------------------------------------------------------------------------
// a launch
// ---------------------------------------------------------------------------------------------------------------------
// Argument checks, IterArgs, grid and launch policies of a search-kernel launch -- ONE copy for bang_k_search, bang_k_search_wf and
// bang_k_search_inmem (inmem: semantics = 1 -- self-paced only, cap up to L + 119, no speculative row request)
static int search_setup(const bang_search_params* p, bool inmem, SearchArgs* out, uint32_t* grid, uint32_t* block, size_t* lds) {
  if (p->R == 0 || p->R > BANG_MAX_R || p->L == 0 || p->L > BANG_MAX_L || p->m == 0) { bang_set_error("bad R/L/m"); return BANG_ERR_ARG; }
  if (p->psz == 0 || p->mp < p->m || (p->mp & 3u)) { bang_set_error("the search kernel needs the LDS-resident pivot layout"); return BANG_ERR_UNSUPPORTED; }
  if (!p->d_codes || !p->d_pivots_packed || !p->d_qc || !p->d_seed || !p->d_bloom || !p->d_cand_ids || !p->d_cand_cnt ||
      !p->d_next_query) { bang_set_error("null buffer"); return BANG_ERR_ARG; }
  if (!p->d_graph && (!p->d_rows || !p->d_ctl || !p->h_done || !p->h_parents || (p->ship_vectors && (!p->h_pub_q || !p->h_pub_c)))) {
    bang_set_error("host-paced search kernel: null pacing buffer"); return BANG_ERR_ARG;
  }
  if (inmem && (!p->d_graph || p->row_layout != 0u)) { bang_set_error("semantics = 1: the graph entries must be in HBM (d_graph, row_layout 0)"); return BANG_ERR_UNSUPPORTED; }
  if (p->pq_nhi && (p->psz != 2 || p->pq_nhi > p->mp)) { bang_set_error("bad pq_nhi"); return BANG_ERR_ARG; }
  if (p->cap_iter == 0 || p->cap_iter > p->L + (inmem ? BANG_INMEM_EXTRA_ITERS : BANG_EXTRA_ITERS) - 1) { bang_set_error("bad iteration cap"); return BANG_ERR_ARG; }
  if (p->rr_queries) {
    if (!p->d_graph) { bang_set_error("the fused re-rank belongs to the self-paced form"); return BANG_ERR_ARG; }
    if (!p->rr_vec_base || !p->rr_ids_out || !p->rr_dists_out || p->rr_k == 0 || p->rr_Q_total < p->rr_q0 + p->Q ||
        !bang_search_can_rerank((int)p->rr_dtype, p->rr_D, p->rr_vec_stride, 0) || (((uintptr_t)p->rr_vec_base) & 3u) || (((uintptr_t)p->rr_queries) & 3u)) {
      bang_set_error("fused re-rank: bad arguments / unsupported vector layout"); return BANG_ERR_ARG;
    }
  }
  if (p->n_rows_pad != 0u) {
    // padded rows: only the instances of search_has_pad_rows read them, at the layout their hand-over is compiled for; the last padded row ends inside the table
    const BangPadRowsLayout pl = bang_pad_rows_layout(p->code_stride, p->mp);
    const char* no = inmem ? "semantics = 1" : !p->d_graph ? "the host-paced form" : p->row_layout != 1u ? "row_layout != 1" : p->n_slices > 1u ? "peer rows (n_slices > 1)"
                   : !search_has_pad_rows((int)(p->mp / 4u), false) ? "this PQ layout (rows read as 72 chunks -- 65 to 72 of at most 2 dims -- only)"
                   : (p->code_stride != 128u || !pl.usable || pl.pad_off != p->mp) ? "this code_stride (128 only)" : nullptr;
    if (no) { bang_set_error("n_rows_pad = %u (option rows_pad): padded rows cannot be read with %s", p->n_rows_pad, no); return BANG_ERR_ARG; }
    if (p->n_rows_pad > bang_pad_rows_count(pl, p->n_nodes)) {
      bang_set_error("n_rows_pad = %u (option rows_pad) exceeds the %u rows the padding of n_nodes = %u code lines holds", p->n_rows_pad, bang_pad_rows_count(pl, p->n_nodes), p->n_nodes);
      return BANG_ERR_ARG;
    }
  }
  SearchArgs& a = *out;
  a.p = *p;
  a.lds_piv_floats = pivot_table_floats(p->psz, p->mp, p->pq_nhi);
  memset(&a.iter, 0, sizeof(a.iter));
  a.iter.d_codes = p->d_codes; a.iter.n_nodes = p->n_nodes; a.iter.d_cand_ids = p->d_cand_ids; a.iter.d_graph = p->d_graph; a.iter.entry_len = p->entry_len;
  a.iter.vec_bytes = p->vec_bytes; a.iter.row_layout = p->row_layout; a.iter.n_rows_hbm = p->n_rows_hbm; a.iter.n_slices = p->n_slices;
  a.iter.d_rows_hbm = p->d_rows_hbm; a.iter.d_row_slices = p->d_row_slices; a.iter.slice_rows = p->slice_rows;
  a.iter.d_bloom = p->d_bloom; a.iter.cap_iter = p->cap_iter; a.iter.n_pad = p->n_rows_pad;      // (summ_iters: below, once the policy is resolved)
  uint32_t grid_n = 0, waves = 0, nctx = p->nctx, gs = p->group_waves;
  const int rc = bang_search_geometry(p->psz, p->mp, p->pq_nhi, p->L, p->Q, p->max_wgs, p->max_waves, p->d_graph ? 0 : 1, &grid_n, &waves, &nctx, &gs);
  if (rc != BANG_OK) return rc;
  a.nctx = nctx;
  a.gs = gs;
  // The filter summary trades LDS-crossbar work on the chain of every iteration (12 ds_bpermute + two transposition passes) for
  // memory requests.  A full chip is short of requests-in-flight: with it the 10 K SIFT1B-shape batch takes 8.36 instead of 9.09 ms, 5 000 /
  // 2 500 queries 4.68 / 2.37 instead of 4.99 / 2.71.  A lightly loaded one is short of nothing but the chain: 1 250 queries (5 waves per CU)
  // 1.70 ms without it against 1.77, 625 queries 1.43 against 1.53 (profiles/r04_summary_cutoff.md).  auto then: off up to 6 queries per CU.
  // (with spec_rows on, re-measured: 1 250 queries 1.69 with / 1.63 without, 1 400: 1.73 / 1.72, 1 536 = 6 per CU: 1.74-1.78 / 1.73-1.74, 1 900: 1.94 / 1.99)
  // (round 6, final kernel: 1 536 queries = 6 per CU 1.555 with / 1.585 without, 1 250 = 5 per CU 1.493 / 1.453: the cut-off is 5)
  const bool light = (p->Q + grid_n - 1) / grid_n <= 5u;
  if (a.p.summ_iters == 0u) a.p.summ_iters = light ? 1u : 0xFFFFFFFFu;
  a.iter.summ_iters = a.p.summ_iters;
  // wave priority around the request-issuing stretches of an iteration: on where wave slots are free (<= 10 queries per CU); BANG_SEARCH_PRIO = 0 / 1 forces it
  { const char* e = bang::env_str("BANG_SEARCH_PRIO"); a.iter.prio = (e && e[0] >= '0' && e[0] <= '3') ? (e[0] == '1' ? 3u : e[0] == '3' ? 1u : (uint32_t)(e[0] - '0')) : (((p->Q + grid_n - 1) / grid_n <= 10u) ? 3u : 0u); }   // (1 = both stretches, 2 = the hand-over's only, 3 = the top's only)
  // spec_rows: one memory latency less on the chain of every iteration, the rows of the ids the filter drops fetched in vain.  Without / with,
  // ms per batch (profiles/r05_spec_rows.md) -- rows pulled, N = 1e9 random graph: 10 000 queries 8.75 / 8.38, 5 000 4.72 / 4.61, 2 500 2.33 / 2.29, 1 250 1.74 / 1.63; N = 1e8 Vamana-style graph, pulled:
  // 6.48 / 6.38, 1.77 / 1.77, 1.29 / 1.23; the same graph in HBM: 4.68 / 4.79, 1.44 / 1.41, 1.13 / 1.07.
  // auto: on where the rows are pulled, and up to 8 queries per CU where the graph is in HBM
  // (round 6, final kernel, structured 1e8-point graph in HBM, without / with: 10 000 queries 4.40 / 4.62 ms, 2 500: 1.32 / 1.345, 2 000: 1.18 / 1.13, 1 250: 1.05 / 1.02, 625: 0.94 / 0.91;
  //  the shape-only DEEP100M index -- its filter drops next to nothing -- 7.16 / 7.05 at 10 000: the policy follows the structured graph, up to 8 queries per CU)
  const bool spec_auto = p->row_layout != 0u || (p->Q + grid_n - 1) / grid_n <= 8u;
  a.p.spec_rows = (!inmem && search_has_spec((int)(p->mp / 4u)) && p->d_graph && (p->spec_rows == 1u || (p->spec_rows == 0u && spec_auto))) ? 1u : 2u;
  // (semantics = 1: no instances with the speculative row request -- off)
  a.wl_words = search_wl_words(p->L);
  a.wave_words = search_wave_words(p->L, nctx, (int)(p->mp / 4u), p->d_graph == nullptr);
  *lds = (size_t)a.lds_piv_floats * 4 + (size_t)waves * a.wave_words * 4 + (p->d_graph ? 0u : SRCH_WG_SHARED_BYTES);
  *grid = grid_n;
  *block = waves * kWaveLanes;
  return BANG_OK;
}

extern "C" int bang_k_search(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (p->Q == 0) return BANG_OK;
  SearchArgs a;
  uint32_t grid = 0, block = 0;
  size_t lds = 0;
  const int rc = search_setup(p, false, &a, &grid, &block, &lds);
  if (rc != BANG_OK) return rc;
  return bang_search_launch_part0(&a, grid, block, lds, stream);
}

extern "C" int bang_k_search_inmem(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (p->Q == 0) return BANG_OK;
  SearchArgs a;
  uint32_t grid = 0, block = 0;
  size_t lds = 0;
  const int rc = search_setup(p, true, &a, &grid, &block, &lds);
  if (rc != BANG_OK) return rc;
  // the fused re-rank works in the wave's LDS region: its n <= L + 120 candidate words fit (2L + L/4 + 144 words)
  static_assert(BANG_INMEM_EXTRA_ITERS <= 144, "the fused re-rank's candidates fit the wave's LDS region");
  return bang_search_launch_part2(&a, grid, block, lds, stream);
}

extern "C" int bang_k_search_wf(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (p->Q == 0) return BANG_OK;
  if (!p->d_graph) { bang_set_error("filter_layout = 1: the word-local filter belongs to the self-paced form (d_graph: graph entries or pulled rows)"); return BANG_ERR_UNSUPPORTED; }
  SearchArgs a;
  uint32_t grid = 0, block = 0;
  size_t lds = 0;
  const int rc = search_setup(p, false, &a, &grid, &block, &lds);
  if (rc != BANG_OK) return rc;
  return bang_search_launch_part4(&a, grid, block, lds, stream);
}
