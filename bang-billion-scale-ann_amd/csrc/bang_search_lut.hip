// bang_search_lut.hip -- the query-resident search kernel for indexes on the LUT path (psz == 0: chunks wider than 8 dimensions, a pivot table
// that does not fit LDS, or option pq = 1): the BANG_Base search loop as bang_search_exact.hip runs it, with every neighbour's distance the PQ
// estimate gathered from the query's look-up table (K2, compute_neighborDist_par bang_search.cu:1201-1241) and the candidate log as its result
// (the re-rank launch bang_k_rerank follows, as behind bang_k_search without the fused re-rank).
//
//  * Query-resident, self-paced, graph entries resident in HBM (d_graph, row_layout 0).  Everything but the distance stage is the walk of
//    search_exact_kernel, called from the same functions: bang_wave_walk.h (hand-out, filter, eager parent, row fetch, the guard against
//    adjacency ids >= n_nodes, counters) and bang_worklist.h (sort, merge, worklist head); per-query activity and the L + 49 cap as there.
//  * Distances: one lane per survivor.  The lane walks its code row 16 chunks at a time -- a 16-byte window read from the row's 4-byte-aligned
//    base with the non-temporal hint (a row is read once), the next window in flight meanwhile; rows that are not dword-aligned (m = 65, m = 5)
//    are shifted into place with v_alignbyte -- and gathers the 16 table entries lut[c][code_c] together with ordinary cached loads (the query
//    re-reads its table every iteration).  The sum is pq_distance_lut's, bit for bit: eight partial sums s[c % 8] in ascending c, the tail
//    c + l < m added the same way, then ((s0+s1)+(s2+s3)) + ((s4+s5)+(s6+s7)).  Any m, any code stride; one instance, no dtype.
//    The table d_lut + q * m * 256 (K1, bang_k_lut_build) is read-only for the launch.  A row is over-read by at most 18 bytes (d_codes has
//    256 bytes of slack).
//  * LDS per wave: 2L + L/4 + 144 words, as the exact kernel; the launch is bound by VGPRs and bang_search_lut_geometry reads the instance's
//    register count.
//
// Reference line numbers: the reference's BANG_Base/bang_search.cu.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_worklist.h"
#include "bang_exact_dist.h"
#include "bang_wave_walk.h"

struct LutArgs {
  bang_search_params p;
  uint32_t wave_words;               // LDS words per wave: worklist + scratch
  uint32_t wl_words;                 // LDS words of the worklist (2L + ceil(L/4), rounded to 4)
};

static inline uint32_t lut_wave_bytes(uint32_t L) { return (wave_wl_words(L) + WAVE_SCRATCH_WORDS) * 4u; }

__device__ __forceinline__ uint32_t code_byte(const uint32_t (&b)[4], int l) { return (b[l >> 2] >> (8 * (l & 3))) & 255u; }

// PQ distances of the n survivors (ids in LDS: sid[0, n)) -> dist[0, n) in LDS; lane i evaluates survivor i0 + i.  Every lane of the wave
// executes: a lane without a survivor evaluates sid[0] again and stores nothing.
__device__ __forceinline__ void lut_dist(const uint8_t GAS* codes, uint32_t stride, uint32_t m, const float GAS* lut, const uint32_t* sid,
                                         uint32_t n, float* dist, int lane) {
  const uint32_t nwin = (m + 3u + 15u) >> 4;                       // 16-byte windows a row can touch from its aligned base
  for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {                      // (uniform; a second pass for the 65th id of the seed list only)
    const uint32_t i = i0 + (uint32_t)lane;
    const uint32_t id = sid[i < n ? i : 0u];
    const uint64_t a = (uint64_t)id * stride;                      // 64-bit row offset :1232
    const uint32_t sh = (uint32_t)a & 3u;
    const u32x4a GAS* row = (const u32x4a GAS*)(codes + (a & ~3ull));
    u32x4a cur = __builtin_nontemporal_load(row);
    float s[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) s[l] = 0.0f;
    uint32_t c = 0, w = 0;
    for (; c + 16u <= m; c += 16u, ++w) {                          // (uniform) two groups of eight chunks
      const u32x4a nxt = __builtin_nontemporal_load(row + (w + 1u < nwin ? w + 1u : w));
      const uint32_t b[4] = {__builtin_amdgcn_alignbyte(cur.y, cur.x, sh), __builtin_amdgcn_alignbyte(cur.z, cur.y, sh),
                             __builtin_amdgcn_alignbyte(cur.w, cur.z, sh), __builtin_amdgcn_alignbyte(nxt.x, cur.w, sh)};
      const float GAS* lc = lut + (size_t)c * 256u;
      float t[16];
#pragma unroll
      for (int l = 0; l < 16; ++l) t[l] = lc[(uint32_t)l * 256u + code_byte(b, l)];
#pragma unroll
      for (int l = 0; l < 8; ++l) s[l] = s[l] + t[l];
#pragma unroll
      for (int l = 0; l < 8; ++l) s[l] = s[l] + t[8 + l];
      cur = nxt;
    }
    const uint32_t r = m - c;                                      // 0..15 chunks left: a group of eight if r >= 8, then the tail
    if (r != 0u) {                                                 // (uniform)
      const u32x4a nxt = __builtin_nontemporal_load(row + (w + 1u < nwin ? w + 1u : w));
      const uint32_t b[4] = {__builtin_amdgcn_alignbyte(cur.y, cur.x, sh), __builtin_amdgcn_alignbyte(cur.z, cur.y, sh),
                             __builtin_amdgcn_alignbyte(cur.w, cur.z, sh), __builtin_amdgcn_alignbyte(nxt.x, cur.w, sh)};
      const float GAS* lc = lut + (size_t)c * 256u;
      float t[16];
#pragma unroll
      for (int l = 0; l < 16; ++l) {                               // (a chunk behind the row's end: chunk c again, never added)
        const bool in = (uint32_t)l < r;
        t[l] = lc[in ? (uint32_t)l * 256u + code_byte(b, l) : code_byte(b, 0)];
      }
#pragma unroll
      for (int l = 0; l < 8; ++l) s[l] = (uint32_t)l < r ? s[l] + t[l] : s[l];
#pragma unroll
      for (int l = 0; l < 8; ++l) s[l] = (uint32_t)(8 + l) < r ? s[l] + t[8 + l] : s[l];
    }
    const float x = (s[0] + s[1]) + (s[2] + s[3]);
    const float y = (s[4] + s[5]) + (s[6] + s[7]);
    if (i < n) dist[i] = x + y;
  }
}

__global__ __launch_bounds__(1024) void search_lut_kernel(const LutArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t llds[];
  const bang_search_params& p = a.p;
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t nwaves = blockDim.x >> 6;
  const uint32_t L = p.L, medoid = p.medoid, cap_iter = p.cap_iter, R = p.R, n_nodes = p.n_nodes, m = p.m;
  const uint32_t cstride = p.code_stride ? p.code_stride : m;
  const uint32_t cand_stride = L + BANG_EXTRA_ITERS;
  const uint8_t GAS* graph = (const uint8_t GAS*)p.d_graph;
  const uint8_t GAS* codes = (const uint8_t GAS*)p.d_codes;
  const uint64_t entry_len = p.entry_len;
  const WalkLds w = walk_lds(llds + (size_t)wave * a.wave_words, L, a.wl_words);
  const WaveLds& s = w.s;
  float* sdist = w.sdist;
  uint32_t* sc = w.sc;
  walk_stamp_start(p.d_ktime);
  const uint32_t total_waves = gridDim.x * nwaves;
  const uint32_t gw = blockIdx.x * nwaves + wave;

  for (bool first_q = true;; first_q = false) {
    const uint32_t q = walk_next_query(first_q, gw, total_waves, p.d_next_query, lane);
    if (q >= p.Q) break;
    uint32_t GAS* bloom = (uint32_t GAS*)p.d_bloom + (size_t)q * BANG_BF_WORDS;
    const float GAS* lut = (const float GAS*)p.d_lut + (size_t)q * m * 256u;      // K1's table of this query :1236

    uint32_t iter = 1, w_n = 0, cc = 1, mark = 0x01010101u, evals = 0, fetched = 0;
    WlHead head = walk_empty_head();
    const WalkSeed seed = walk_begin_query(p.d_cand_ids, p.d_seed, q, cand_stride, medoid, lane);
    uint32_t cnt_in = seed.cnt, x0 = seed.x0;
    const uint32_t x1 = seed.x1;
    bool have_row = true;

    for (;;) {
      const bool first = (iter == 1);
      // ---------------- K5: filter
      const uint32_t ci = walk_row_len_entry(have_row, cnt_in, first, R, n_nodes, x0, x1, p.d_abort, lane);
      fetched += ci;
      const WalkSurvivors sv = walk_filter(bloom, ci, x0, x1, sc, lane);
      const uint32_t n = sv.n, sid0 = sv.sid0, sid1 = sv.sid1;
      evals += n;

      // ---------------- K2: PQ distances from the query's table (compute_neighborDist_par :1201-1241) ----------------
      if (n > 0) lut_dist(codes, cstride, m, lut, sc, n, sdist, lane);
      wave_sync();
      const float d0 = ((uint32_t)lane < n) ? sdist[lane] : BIG_DIST;
      const float d1 = (lane == 0 && n > 64) ? sdist[64] : BIG_DIST;
      wave_sync();

      // ---------------- K4: parent
      uint32_t parent = 0;
      bool found = false;
      walk_parent(s, head, n, sid0, sid1, d0, d1, first, w_n, medoid, mark, cc, parent, found, lane);

      // ---------------- hand the parent over: its adjacency row is requested now and travels during the sort/merge
      if (found && iter < cap_iter) {
        const WalkEntryRow row = walk_fetch_entry_row(graph, entry_len, p.vec_bytes, R, parent, lane);
        cnt_in = row.cnt; x0 = row.x;
      }
      if (found && lane == 0) p.d_cand_ids[(size_t)q * cand_stride + cc - 1u] = parent;      // :1451-1458

      // ---------------- K3a + K3b: sort the survivors, merge them into the worklist (not at the cap: CANON 6) ----------------
      if (n > 0 && iter < cap_iter) w_n = sort_and_merge(s, n, d0, sid0, d1, sid1, iter, w_n, L, medoid, mark, head.tail, lane);

      // a query is active while it has a parent or unmerged survivors (CANON 4); the loop ends at the cap (:950-956)
      if ((!found && n == 0) || iter == cap_iter) break;
      ++iter;
      have_row = found;
      head = worklist_head(s, w_n, lane);
    }

    // ---------------- the query is finished: its candidate log feeds the re-rank launch (K6 + K7)
    walk_finish_query(p.d_cand_cnt, p.d_qstats, p.d_qiters, q, cc, evals, fetched, iter, lane);
    wave_sync();
  }
  walk_stamp_end(p.d_ktime);
}

// ---------------------------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------------------------
// 1 if one wave's state (2L + L/4 + 144 words) fits LDS; the table stays in HBM / the caches, so m only has to be a chunk count
extern "C" int bang_search_lut_supported(uint32_t m, uint32_t L) {
  if (m == 0 || L == 0 || L > BANG_MAX_L) return 0;
  return lut_wave_bytes(L) <= WAVE_MAX_LDS ? 1 : 0;
}

static WaveKernelAttr lut_attr;                                    // the instance's figures, per device

// The grid of a launch (bang_wave_geometry on the instance's own figures), as bang_search_exact_geometry
extern "C" int bang_search_lut_geometry(uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves) {
  if (!workgroups || !waves || Q == 0) return BANG_ERR_ARG;
  if (L == 0 || L > BANG_MAX_L) { bang_set_error("LUT search kernel: bad L"); return BANG_ERR_ARG; }
  const int rc = wave_kernel_geometry((const void*)search_lut_kernel, lut_attr, lut_wave_bytes(L), Q, max_wgs, max_waves, workgroups, waves);
  if (rc == BANG_ERR_UNSUPPORTED) bang_set_error("LUT search kernel: one wave's worklist does not fit LDS at L=%u", L);
  return rc;
}

extern "C" int bang_k_search_lut(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (p->Q == 0) return BANG_OK;
  if (p->R == 0 || p->R > BANG_MAX_R || p->L == 0 || p->L > BANG_MAX_L) { bang_set_error("LUT search kernel: bad R/L"); return BANG_ERR_ARG; }
  if (p->psz != 0) { bang_set_error("LUT search kernel: psz = %u (an index with an LDS pivot table runs on bang_k_search)", p->psz); return BANG_ERR_UNSUPPORTED; }
  if (!p->d_graph || p->row_layout != 0) { bang_set_error("LUT search kernel: needs the graph entries in HBM (d_graph, row_layout = 0)"); return BANG_ERR_UNSUPPORTED; }
  if (p->m == 0 || (p->code_stride != 0 && p->code_stride < p->m)) { bang_set_error("LUT search kernel: bad m / code stride"); return BANG_ERR_ARG; }
  if (!p->d_lut || !p->d_codes || !p->d_seed || !p->d_bloom || !p->d_cand_ids || !p->d_cand_cnt || !p->d_next_query) {
    bang_set_error("LUT search kernel: null buffer (d_lut, d_codes, d_seed, d_bloom, d_cand_ids, d_cand_cnt, d_next_query)"); return BANG_ERR_ARG;
  }
  if (p->cap_iter == 0 || p->cap_iter > p->L + BANG_EXTRA_ITERS - 1) { bang_set_error("LUT search kernel: bad iteration cap"); return BANG_ERR_ARG; }
  if (p->entry_len < (uint64_t)p->vec_bytes + 4u * (1u + p->R)) {
    bang_set_error("LUT search kernel: a graph entry of %llu bytes does not hold %u vector bytes, the degree and R = %u ids", (unsigned long long)p->entry_len, p->vec_bytes, p->R);
    return BANG_ERR_ARG;
  }
  if ((((uintptr_t)p->d_codes) & 3u) || (((uintptr_t)p->d_lut) & 3u)) { bang_set_error("LUT search kernel: code table and LUT must be 4-byte aligned"); return BANG_ERR_ARG; }
  if (!bang_search_lut_supported(p->m, p->L)) { bang_set_error("LUT search kernel: one wave's worklist does not fit LDS at L=%u", p->L); return BANG_ERR_UNSUPPORTED; }
  uint32_t grid_n = 0, waves = 0;
  const int rc = bang_search_lut_geometry(p->L, p->Q, p->max_wgs, p->max_waves, &grid_n, &waves);
  if (rc != BANG_OK) return rc;
  LutArgs a;
  a.p = *p;
  a.wl_words = wave_wl_words(p->L);
  a.wave_words = a.wl_words + WAVE_SCRATCH_WORDS;
  return wave_kernel_launch((const void*)search_lut_kernel, lut_attr, grid_n, waves, a.wave_words * 4u, stream, a);
}
