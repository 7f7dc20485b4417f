// bang_search_beam.hip -- the BEAM form of the exact-distance search kernel (engine options distance = 1, beam = W in 2..4; DESIGN.md
// section 4.10): the walk of bang_search_exact.hip with up to W parents expanded per iteration, the way DiskANN's beam search expands the W
// closest unvisited worklist entries together -- their adjacency rows, filter probes and vectors share one round trip each, and a query
// lives for about 1 / W of the iterations.  The walk is the post-merge-parent one (CANON 14 and 15):
//
//   1. the ids of the <= W rows of an iteration are ALL tested against the filter state at entry (CANON 3), then the bits of those that
//      passed are set;
//   2. a survivor of row j whose id also survived in a row i < j is dropped (exact on ids; duplicates inside one row stay);
//   3. ONE distance call covers every kept survivor (<= 256, the seed list 65) -- the routines of bang_search_exact.hip (bang_exact_dist.h);
//   4. the rows are sorted and merged into the worklist one after the other (sort_and_merge of bang_worklist.h, unchanged, mark = none):
//      among equal distances a later row's entry stands in front of an earlier row's;
//   5. the first P = min(W, room in the candidate log, unvisited entries) unvisited worklist entries are marked and logged; P == 0 ends
//      the query;
//   6. at the iteration cap the query ends with those parents logged, never expanded;
//   7. the P rows are requested together, one dword per lane each, before the first is waited for.
//
// Results: the first min(k, w_n) worklist entries (CANON 11).  W = 1 is accepted at this level (the post-merge walk with exact distances);
// the engine never asks for it -- option beam = 1 keeps the kernels of bang_search_exact.hip.
//
// Narrow layouts only (those of bang_search_can_rerank: 8-bit D % 16 == 0 with D / 16 a power of two, float D % 4 == 0, D <= 256), float /
// 8-bit rows (no fp16 table).  Built twice: bang_search_beam.o (search_exact_beam_kernel: graph entries in HBM) and, with
// -DBANG_EXACT_PULL=1, bang_search_beam_pull.o (search_exact_beam_pull_kernel: row_layout 1, the packed vector table, every parent's row from
// the slice table, the HBM row copy or pinned host memory: walk_fetch_pulled_row).  Around steps 1-5 the kernel calls the stages of
// bang_wave_walk.h that bang_search_exact.hip calls (hand-out, LDS carve, query load, seed list, row fetches, counters, stamps); its
// four-row filter -- branch-free probes, cross-row duplicates -- is its own.
//
// LDS per wave: the worklist (2L + L/4 words) + 144 words of sort scratch + two arrays of 64 W + 4 words (the kept survivors' ids and
// distances, row after row).  No scratch memory, no flat_ instruction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_worklist.h"
#include "bang_exact_dist.h"
#include "bang_wave_walk.h"

#define BEAM_MAX 4                   // rows per iteration the kernel is compiled for
#define BEAM_NO_MARK 0xFFFFFFFFu     // the merge marks nothing: parents are taken behind it

struct BeamArgs {
  bang_search_params p;
  uint32_t wave_words;               // LDS words per wave: worklist + scratch + the two survivor arrays
  uint32_t wl_words;                 // LDS words of the worklist (2L + ceil(L/4), rounded to 4)
  uint32_t row_words;                // words of one survivor array: 64 beam + 4
  uint32_t beam;
};

static __host__ __device__ inline uint32_t beam_row_words(uint32_t beam) { return 64u * beam + 4u; }

typedef uint32_t u32x4b __attribute__((ext_vector_type(4)));     // 16-byte aligned: ds_read_b128

#ifdef BANG_EXACT_PULL
#define BEAM_PULL 1
#define BEAM_KERNEL search_exact_beam_pull_kernel
#define BEAM_GEOMETRY bang_search_exact_beam_pull_geometry
#else
#define BEAM_PULL 0
#define BEAM_KERNEL search_exact_beam_kernel
#define BEAM_GEOMETRY bang_search_exact_beam_geometry
#endif

template <int DT>
__global__ __launch_bounds__(1024) void BEAM_KERNEL(const BeamArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t xlds[];
  const bang_search_params& p = a.p;
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t nwaves = blockDim.x >> 6;
  const uint32_t L = p.L, medoid = p.medoid, cap_iter = p.cap_iter, R = p.R, n_nodes = p.n_nodes, beam = a.beam;
  const uint32_t cand_stride = L + BANG_EXTRA_ITERS;
#if BEAM_PULL
  const uint8_t GAS* graph = (const uint8_t GAS*)p.rr_vec_base;   // the vectors: node x's at graph + x * entry_len
  const uint64_t entry_len = p.rr_vec_stride;
  const uint32_t lim = n_nodes != 0u ? n_nodes : BANG_ADJ_PAD;    // (a pad value in front of an id is an id out of range whether or not n_nodes was given)
#else
  const uint8_t GAS* graph = (const uint8_t GAS*)p.d_graph;
  const uint64_t entry_len = p.entry_len;
  const uint32_t lim = n_nodes;                                   // 0: ids are not checked
#endif
  const WalkLds w = walk_lds(xlds + (size_t)wave * a.wave_words, L, a.wl_words);
  const WaveLds& s = w.s;
  uint32_t* bid = w.scratch + WAVE_SCRATCH_WORDS; // the kept survivors' ids, row after row, input order (16-byte aligned)
  float* bdist = (float*)(bid + a.row_words);     // ... and their distances
  uint32_t* psel = w.scratch;                     // the parents picked by the selection (the sort scratch is dead there)
  walk_stamp_start(p.d_ktime);
  const uint32_t total_waves = gridDim.x * nwaves;
  const uint32_t gw = blockIdx.x * nwaves + wave;

  for (bool first_q = true;; first_q = false) {
    const uint32_t q = walk_next_query(first_q, gw, total_waves, p.d_next_query, lane);
    if (q >= p.Q) break;
    const size_t qabs = (size_t)p.rr_q0 + q;
    uint32_t GAS* bloom = (uint32_t GAS*)p.d_bloom + (size_t)q * BANG_BF_WORDS;

    // the raw query, in registers
    const uint32_t D = p.rr_D;
    const NarrowQuery nq = walk_load_query_narrow<DT>(p.rr_queries, qabs, D, lane);

    // ---------------- per-query state: the walk's, with one row -- the seed list -- of up to BEAM_MAX
    uint32_t iter = 1, w_n = 0, cc = 1, evals = 0, fetched = 0, nrows = 1;
    const WalkSeed seed = walk_begin_query(p.d_cand_ids, p.d_seed, q, cand_stride, medoid, lane);
    uint32_t x[BEAM_MAX], cnt[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) { x[j] = 0u; cnt[j] = 0u; }
    cnt[0] = seed.cnt; x[0] = seed.x0;
    const uint32_t x1 = seed.x1;

    for (;;) {
      const bool first = (iter == 1);
      // ---------------- step 1: the rows' lengths; an id out of range empties every row of the iteration
      uint32_t ci[BEAM_MAX];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        uint32_t c = (uint32_t)j < nrows ? uni(cnt[j]) : 0u;
#if BEAM_PULL
        if (!first && (uint32_t)j < nrows) c = (uint32_t)__popcll(__ballot(x[j] != BANG_ADJ_PAD));   // a 256-byte row: ids first, padding behind them
#endif
        const uint32_t cap = R + ((first && j == 0) ? 1u : 0u);
        if (c > cap) c = cap;
        ci[j] = c;
        if (lim != 0u && __ballot((uint32_t)lane < c && x[j] >= lim) != 0ull) bad = true;
      }
      if (lim != 0u && ci[0] > 64u && uni(x1) >= lim) bad = true;
      if (bad) {
        if (lane == 0 && p.d_abort) *p.d_abort = 2u;
#pragma unroll
        for (int j = 0; j < BEAM_MAX; ++j) ci[j] = 0u;
      }
      fetched += ci[0] + ci[1] + ci[2] + ci[3];
      const bool v1 = ci[0] > 64u;                                // the 65th id exists in the seed list only (uniform)

      // ---------------- K5: every id of every row against the filter state at entry -- the probes of all rows in ONE round trip
      uint32_t ha[BEAM_MAX], hb[BEAM_MAX], wa[BEAM_MAX], wb[BEAM_MAX];
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) { ha[j] = hash1(x[j]); hb[j] = hash2(x[j]); }
      // CANON 3: the previous iteration's atomic ORs have completed (and the rows have arrived)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        // (a lane without an id reads word 0 instead of sitting the load out: eight loads in flight, no branch between them)
        const bool v = (uint32_t)lane < ci[j];
        wa[j] = ld_bypass_l1(&bloom[v ? ha[j] >> 5 : 0u]);
        wb[j] = ld_bypass_l1(&bloom[v ? hb[j] >> 5 : 0u]);
      }
      uint32_t h1a = 0, h1b = 0, w1a = 0, w1b = 0;
      if (v1) {
        h1a = hash1(x1); h1b = hash2(x1);
        if (lane == 0) { w1a = ld_bypass_l1(&bloom[h1a >> 5]); w1b = ld_bypass_l1(&bloom[h1b >> 5]); }
      }
      bool pass[BEAM_MAX];
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j)
        pass[j] = (uint32_t)lane < ci[j] && !(((wa[j] >> (ha[j] & 31)) & 1u) && ((wb[j] >> (hb[j] & 31)) & 1u));
      const bool pass1 = v1 && (lane == 0) && !(((w1a >> (h1a & 31)) & 1u) && ((w1b >> (h1b & 31)) & 1u));
      // ... then every survivor's two bits are set
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        if (pass[j]) {
          (void)__hip_atomic_fetch_or(&bloom[ha[j] >> 5], 1u << (ha[j] & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_or(&bloom[hb[j] >> 5], 1u << (hb[j] & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (pass1) {
        (void)__hip_atomic_fetch_or(&bloom[h1a >> 5], 1u << (h1a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_or(&bloom[h1b >> 5], 1u << (h1b & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }

      // ---------------- step 2: cross-row duplicates dropped (exact on ids), the kept survivors compacted row after row, input order
      uint32_t off[BEAM_MAX], nk[BEAM_MAX], tot = 0;
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        bool keep = pass[j];
        if (j > 0 && tot > 0u && __ballot(pass[j]) != 0ull) {     // (uniform) against the <= 64 j kept survivors of the earlier rows
          bool dup = false;
          for (uint32_t t = 0; t < tot; t += 4u) {                // broadcast ds_read_b128; the words behind tot are not ids
            const u32x4b e = *(const u32x4b*)(bid + t);
            dup |= (e.x == x[j]) | ((t + 1u < tot) & (e.y == x[j])) | ((t + 2u < tot) & (e.z == x[j])) | ((t + 3u < tot) & (e.w == x[j]));
          }
          keep = keep && !dup;
        }
        const uint64_t mk = __ballot(keep);
        if (keep) bid[tot + lanes_below(mk)] = x[j];
        off[j] = tot;
        nk[j] = (uint32_t)__popcll(mk);
        tot += nk[j];
        if (j == 0) {                                             // the seed list's 65th id, behind the 64 of the lanes
          if (pass1) bid[tot] = x1;
          if (__ballot(pass1) != 0ull) { ++nk[0]; ++tot; }
        }
        wave_sync();
      }
      evals += tot;

      // ---------------- step 3: exact distances (bang_exact_dist.h), one call over every kept survivor
      if (tot > 0u) {
        if (DT == BANG_F32) exact_dist_f32(graph, entry_len, D, bid, tot, bdist, nq.qr, lane);
        else exact_dist8<DT == BANG_I8>(graph, entry_len, nq.G, bid, tot, bdist, nq.qw, nq.qq, lane);
      }
      wave_sync();

      // ---------------- step 4: K3a + K3b per row (the seed list as iteration 1, every later row as iteration 2)
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        const uint32_t n = nk[j], o = off[j];
        if (n > 0u) {                                             // (uniform)
          const float d0 = ((uint32_t)lane < n) ? bdist[o + (uint32_t)lane] : BIG_DIST;
          const uint32_t id0 = ((uint32_t)lane < n) ? bid[o + (uint32_t)lane] : 0u;
          const float d1 = (lane == 0 && n > 64u) ? bdist[o + 64u] : BIG_DIST;
          const uint32_t id1 = (lane == 0 && n > 64u) ? bid[o + 64u] : 0u;
          float worst = 0.0f;
          if (w_n > 0u) worst = __uint_as_float(uni(__float_as_uint(s.wd[w_n - 1u])));
          wave_sync();
          w_n = sort_and_merge(s, n, d0, id0, d1, id1, first ? 1u : 2u, w_n, L, medoid, BEAM_NO_MARK, worst, lane);
        }
      }

      // ---------------- step 5: the first P unvisited worklist entries are marked visited and logged
      uint32_t want = cand_stride - cc;
      if (want > beam) want = beam;
      uint32_t got = 0;
      for (uint32_t base = 0; base < w_n && got < want; base += WAVE) {        // (uniform)
        const uint32_t i = base + (uint32_t)lane;
        const bool unv = i < w_n && s.wv[i < w_n ? i : 0u] == 0;
        const uint64_t mk = __ballot(unv);
        const uint32_t r = lanes_below(mk), left = want - got;
        if (unv && r < left) {
          const uint32_t id = s.wi[i];
          s.wv[i] = 1;
          psel[got + r] = id;
          p.d_cand_ids[(size_t)q * cand_stride + cc + got + r] = id;
        }
        const uint32_t c = (uint32_t)__popcll(mk);
        got += c < left ? c : left;
      }
      wave_sync();
      cc += got;
      // P == 0: the query ends; step 6: at the cap these parents are logged, never expanded
      if (got == 0u || iter == cap_iter) break;

      // ---------------- step 7: the P rows are requested together; they travel until the next iteration's probes need them
      nrows = got;
#pragma unroll
      for (int j = 0; j < BEAM_MAX; ++j) {
        if ((uint32_t)j < got) {                                  // (uniform)
          const uint32_t parent = uni(psel[j]);
#if BEAM_PULL
          x[j] = walk_fetch_pulled_row(p.n_slices, p.slice_rows, p.d_row_slices, p.n_rows_hbm, p.d_rows_hbm, p.d_graph, parent, lane);
          cnt[j] = 64u;                                           // counted when the row is consumed
#else
          const WalkEntryRow row = walk_fetch_entry_row(graph, entry_len, p.vec_bytes, R, parent, lane);
          cnt[j] = row.cnt; x[j] = row.x;
#endif
        }
      }
      wave_sync();                                                // (psel is read before the next iteration's sort overwrites it)
      ++iter;
    }

    // ---------------- the query is finished: counters, then the results straight from the worklist (CANON 11)
    walk_finish_query(p.d_cand_cnt, p.d_qstats, p.d_qiters, q, cc, evals, fetched, iter, lane);
    // walk_write_results(s, w_n, ...), written out as in bang_search_exact.hip: inlined from the header the loop costs the u8 / i8 instances twice
    // the SGPR spills (87 -> 178) and the small batches 2-3 % (profiles/wave_walk_device_code.md, profiles/wave_walk_bench.md)
    const uint32_t k = p.rr_k, Qt = p.rr_Q_total;
    uint64_t GAS* ids_out = (uint64_t GAS*)p.rr_ids_out;
    float GAS* dists_out = (float GAS*)p.rr_dists_out;
    for (uint32_t r = (uint32_t)lane; r < k; r += WAVE) {
      const bool have = r < w_n;                                  // a short worklist is padded (CANON 8)
      ids_out[qabs * k + r] = have ? (uint64_t)s.wi[r] : ~0ull;                     // [Q][k] u64
      dists_out[(size_t)r * Qt + qabs] = have ? s.wd[r] : BIG_DIST;                 // [rank][Q]
    }
    wave_sync();                                                  // (the worklist is read before the next query overwrites it)
  }
  walk_stamp_end(p.d_ktime);
}

// ---------------------------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------------------------
static const void* beam_instance(int dtype) {
  if (dtype == BANG_U8) return (const void*)BEAM_KERNEL<BANG_U8>;
  if (dtype == BANG_I8) return (const void*)BEAM_KERNEL<BANG_I8>;
  if (dtype == BANG_F32) return (const void*)BEAM_KERNEL<BANG_F32>;
  return nullptr;
}
static WaveKernelAttr beam_attr[3];                                // per instance: its figures, per device

static uint32_t beam_wave_words(uint32_t L, uint32_t beam) { return wave_wl_words(L) + WAVE_SCRATCH_WORDS + 2u * beam_row_words(beam); }

// The grid of a launch (bang_wave_geometry on the instance's own figures); LDS per wave: 2L + L/4 + 144 + 2 (64 beam + 4) words
extern "C" int BEAM_GEOMETRY(int dtype, uint32_t L, uint32_t beam, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves) {
  if (!workgroups || !waves || Q == 0) return BANG_ERR_ARG;
  if (beam == 0 || beam > BEAM_MAX) { bang_set_error("distance = 1: beam = %u is outside [1, %d]", beam, BEAM_MAX); return BANG_ERR_ARG; }
  const void* k = beam_instance(dtype);
  if (!k || L == 0 || L > BANG_MAX_L) { bang_set_error("distance = 1, beam = %u: bad dtype / L", beam); return BANG_ERR_ARG; }
  const int rc = wave_kernel_geometry(k, beam_attr[dtype], beam_wave_words(L, beam) * 4u, Q, max_wgs, max_waves, workgroups, waves);
  if (rc == BANG_ERR_UNSUPPORTED) bang_set_error("distance = 1, beam = %u: one wave's worklist does not fit LDS at L=%u", beam, L);
  return rc;
}

// one launch of this translation unit's instances (the arguments are checked: bang_k_search_exact_beam)
static int beam_launch(const bang_search_params* p, uint32_t beam, void* stream) {
  uint32_t grid_n = 0, waves = 0;
  const int rc = BEAM_GEOMETRY((int)p->rr_dtype, p->L, beam, p->Q, p->max_wgs, p->max_waves, &grid_n, &waves);
  if (rc != BANG_OK) return rc;
  BeamArgs a;
  a.p = *p;
  a.beam = beam;
  a.wl_words = wave_wl_words(p->L);
  a.row_words = beam_row_words(beam);
  a.wave_words = beam_wave_words(p->L, beam);
  return wave_kernel_launch(beam_instance((int)p->rr_dtype), beam_attr[p->rr_dtype], grid_n, waves, a.wave_words * 4u, stream, a);
}

#if BEAM_PULL
// the pulled-rows instances (row_layout 1), called by bang_k_search_exact_beam with its arguments checked
extern "C" int bang_k_search_exact_beam_pull(const bang_search_params* p, uint32_t beam, void* stream) {
  if (!p || p->row_layout != 1u || p->rr_vec_f16 != 0u || beam == 0 || beam > BEAM_MAX ||
      !bang_search_exact_beam_supported((int)p->rr_dtype, p->rr_D, p->rr_vec_stride)) return BANG_ERR_ARG;
  return beam_launch(p, beam, stream);
}
#else
// Vector layouts the beam instances evaluate: those of the narrow exact-distance instances (bang_search_exact_supported and
// bang_search_can_rerank: 8-bit D % 16 == 0 with D / 16 a power of two, float D % 4 == 0, D <= 256, a stride divisible by 4, no MIPS padding)
extern "C" int bang_search_exact_beam_supported(int dtype, uint32_t D, uint64_t stride) {
  return bang_search_exact_supported(dtype, D, stride) != 0 && bang_search_can_rerank(dtype, D, stride, 0) != 0 ? 1 : 0;
}

// the checks of bang_k_search_exact (bang_exact_check_args / _layout), in its order and with its texts behind "distance = 1, beam = W"; what has no
// beam instance -- an fp16 vector table, the wide layouts -- is refused where bang_k_search_exact looks at it
extern "C" int bang_k_search_exact_beam(const bang_search_params* p, uint32_t beam, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (beam == 0 || beam > BEAM_MAX) { bang_set_error("distance = 1: beam = %u is outside [1, %d]", beam, BEAM_MAX); return BANG_ERR_ARG; }
  if (p->Q == 0) return BANG_OK;
  char prefix[32];
  snprintf(prefix, sizeof prefix, "distance = 1, beam = %u", beam);
  int rc = bang_exact_check_args(p, prefix);
  if (rc != BANG_OK) return rc;
  if (p->rr_vec_f16 == 1u) { bang_set_error("%s: rr_vec_f16 = 1 (an fp16 vector table) has no beam instance", prefix); return BANG_ERR_UNSUPPORTED; }
  rc = bang_exact_check_layout(p, prefix);
  if (rc != BANG_OK) return rc;
  if (!bang_search_exact_beam_supported((int)p->rr_dtype, p->rr_D, p->row_layout == 1u ? p->rr_vec_stride : p->entry_len)) {
    bang_set_error("%s: the wide vector layouts (dtype %u, D = %u) have no beam instance: 8-bit D / 16 a power of two, D <= 256", prefix, p->rr_dtype, p->rr_D);
    return BANG_ERR_UNSUPPORTED;
  }
  if (p->row_layout == 1u) return bang_k_search_exact_beam_pull(p, beam, stream);
  return beam_launch(p, beam, stream);
}
#endif
