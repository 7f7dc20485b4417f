// bang_search_beam.hip -- the BEAM form of the exact-distance search kernel (engine options distance = 1, beam = W in 2..4; DESIGN.md
// section 4.10): the walk of bang_search_exact.hip with up to W parents expanded per iteration, the way DiskANN's beam search expands the W
// closest unvisited worklist entries together -- their adjacency rows, filter probes and vectors share one round trip each, and a query
// lives for about 1 / W of the iterations.  The walk is the post-merge-parent one (CANON 14 and 15):
//
//   1. the ids of the <= W rows of an iteration are ALL tested against the filter state at entry (CANON 3), then the bits of those that
//      passed are set;
//   2. a survivor of row j whose id also survived in a row i < j is dropped (exact on ids; duplicates inside one row stay);
//   3. ONE distance call covers every kept survivor (<= 256, the seed list 65) -- the arithmetic of bang_search_exact.hip;
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
// the slice table, the HBM row copy or pinned host memory, as bang_search_exact.hip selects it).
//
// LDS per wave: the worklist (2L + L/4 words) + 144 words of sort scratch + two arrays of 64 W + 4 words (the kept survivors' ids and
// distances, row after row).  No scratch memory, no flat_ instruction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_worklist.h"

#define BEAM_SCRATCH_WORDS 144u      // sd/ti [72] + td [72]: the sort of one row
#define BEAM_MAX_LDS (160u * 1024u)
#define BEAM_MAX 4                   // rows per iteration the kernel is compiled for
#define BEAM_NO_MARK 0xFFFFFFFFu     // the merge marks nothing: parents are taken behind it

struct BeamArgs {
  bang_search_params p;
  uint32_t wave_words;               // LDS words per wave: worklist + scratch + the two survivor arrays
  uint32_t wl_words;                 // LDS words of the worklist (2L + ceil(L/4), rounded to 4)
  uint32_t row_words;                // words of one survivor array: 64 beam + 4
  uint32_t beam;
};

static __host__ __device__ inline uint32_t beam_wl_words(uint32_t L) { return (2u * L + (L + 3u) / 4u + 3u) & ~3u; }
static __host__ __device__ inline uint32_t beam_row_words(uint32_t beam) { return 64u * beam + 4u; }

typedef uint32_t u32x4b __attribute__((ext_vector_type(4)));     // 16-byte aligned: ds_read_b128

template <bool SIGNED>
__device__ __forceinline__ int xdot4(uint32_t a, uint32_t b, int c) {
  if (SIGNED) return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
  return (int)__builtin_amdgcn_udot4(a, b, (uint32_t)c, false);
}

// exact distances of the n survivors (ids in LDS: sid[0, n)) -> dist[0, n) in LDS, 8-bit vectors (exact_dist8 of bang_search_exact.hip).
// qw: this lane's 16-byte piece of the query (piece lane % G), qq: the sum of its squares.  Every lane of the wave executes.
template <bool SIGNED>
__device__ __forceinline__ void beam_dist8(const uint8_t GAS* graph, uint64_t entry_len, uint32_t G, const uint32_t* sid, uint32_t n,
                                           float* dist, u32x4a qw, int qq, int lane) {
  constexpr int U = 4;                                            // vector fetches in flight per lane
  const uint32_t per = 64u / G;                                   // survivors per wave instruction
  const uint32_t sub = (uint32_t)lane & (G - 1u), slot = (uint32_t)lane / G;
  for (uint32_t i0 = 0; i0 < n; i0 += per * U) {                  // (uniform)
    u32x4a v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = i0 + (uint32_t)u * per + slot;
      const uint32_t id = sid[i < n ? i : 0u];
      v[u] = *(const u32x4a GAS*)(graph + (uint64_t)id * entry_len + 16u * sub);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = i0 + (uint32_t)u * per + slot;
      int vv = xdot4<SIGNED>(v[u].x, v[u].x, xdot4<SIGNED>(v[u].y, v[u].y, xdot4<SIGNED>(v[u].z, v[u].z, xdot4<SIGNED>(v[u].w, v[u].w, qq))));
      const int vq = xdot4<SIGNED>(v[u].x, qw.x, xdot4<SIGNED>(v[u].y, qw.y, xdot4<SIGNED>(v[u].z, qw.z, xdot4<SIGNED>(v[u].w, qw.w, 0))));
      vv -= 2 * vq;
      for (uint32_t off = 1; off < G; off <<= 1) vv += __shfl_xor(vv, (int)off);
      if (i < n && sub == 0u) dist[i] = (float)vv;
    }
  }
}

// the same for float vectors (exact_dist_f32 of bang_search_exact.hip): lane i evaluates survivor i0 + i, the ascending fmaf chain over the
// D dimensions (D % 4 == 0, <= 256), four 16-byte loads in flight; qr[t]: lane l holds query element 64 t + l
__device__ __forceinline__ void beam_dist_f32(const uint8_t GAS* graph, uint64_t entry_len, uint32_t D, const uint32_t* sid, uint32_t n,
                                              float* dist, const float (&qr)[4], int lane) {
  constexpr int RF = 4;                                           // 16-byte loads in flight per lane
  for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {                     // (uniform)
    const uint32_t i = i0 + (uint32_t)lane;
    const uint32_t id = sid[i < n ? i : 0u];
    const uint8_t GAS* v = graph + (uint64_t)id * entry_len;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t jt = (uint32_t)t * 64u;
      if (jt >= D) break;                                         // (uniform)
      const uint32_t dt = D - jt < 64u ? D - jt : 64u;
      for (uint32_t jl = 0; jl < dt; jl += 4u * RF) {             // (uniform)
        u32x4a w[RF];
#pragma unroll
        for (int u = 0; u < RF; ++u) {
          const uint32_t j = jl + 4u * (uint32_t)u;
          w[u] = *(const u32x4a GAS*)(v + 4u * (jt + (j < dt ? j : 0u)));
        }
#pragma unroll
        for (int u = 0; u < RF; ++u) {
          const uint32_t j = jl + 4u * (uint32_t)u;
          if (j < dt) {                                           // (uniform)
            const uint32_t ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const float qv = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(qr[t]), (int)(j + (uint32_t)d)));
              const float diff = __uint_as_float(ww[d]) - qv;     // orc_exact_dist: vector - query
              acc = __builtin_fmaf(diff, diff, acc);              // ascending dimension
            }
          }
        }
      }
    }
    if (i < n) dist[i] = acc;
  }
}

#ifdef BANG_EXACT_PULL
#define BEAM_PULL 1
#define BEAM_KERNEL search_exact_beam_pull_kernel
#define BEAM_GEOMETRY bang_search_exact_beam_pull_geometry
// the slice table's entry idx (biased base addresses, 0 = that slice is not there), through the scalar cache
__device__ __forceinline__ uint64_t slice_base(const uint64_t* tab, uint32_t idx) {
  uint64_t v;
  const uint64_t a = (uint64_t)(uintptr_t)tab + 8ull * idx;     // (uniform, but not provably so: made so)
  const uint64_t at = ((uint64_t)uni((uint32_t)(a >> 32)) << 32) | uni((uint32_t)a);
  asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(at) : "memory");
  return v;
}
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
  uint32_t* wbase = xlds + (size_t)wave * a.wave_words;
  uint32_t* scratch = wbase + a.wl_words;
  WaveLds s;
  s.wd = (float*)wbase; s.wi = wbase + L; s.wv = (uint8_t*)(wbase + 2 * L);
  s.sd = (float*)scratch; s.ti = scratch; s.td = (float*)(scratch + 72);
  uint32_t* bid = scratch + BEAM_SCRATCH_WORDS;   // the kept survivors' ids, row after row, input order (16-byte aligned)
  float* bdist = (float*)(bid + a.row_words);     // ... and their distances
  uint32_t* psel = scratch;                       // the parents picked by the selection (the sort scratch is dead there)
  if (p.d_ktime && threadIdx.x == 0) p.d_ktime[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
  const uint32_t total_waves = gridDim.x * nwaves;
  const uint32_t gw = blockIdx.x * nwaves + wave;

  for (bool first_q = true;; first_q = false) {
    // ---------------- the next query: the first one by position, then from the hand-out counter
    uint32_t q;
    if (first_q) q = gw;
    else {
      uint32_t t = 0;
      if (lane == 0) t = __hip_atomic_fetch_add(p.d_next_query, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      q = total_waves + uni(t);
    }
    if (q >= p.Q) break;
    const size_t qabs = (size_t)p.rr_q0 + q;
    uint32_t GAS* bloom = (uint32_t GAS*)p.d_bloom + (size_t)q * BANG_BF_WORDS;

    // the raw query, in registers
    const uint32_t D = p.rr_D;
    u32x4a qw = {0u, 0u, 0u, 0u};
    int qq = 0;
    uint32_t G = 1;
    float qr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (DT == BANG_F32) {
      const float GAS* qsrc = (const float GAS*)p.rr_queries + qabs * D;
#pragma unroll
      for (int t = 0; t < 4; ++t) { const uint32_t j = (uint32_t)t * 64u + (uint32_t)lane; qr[t] = qsrc[j < D ? j : 0u]; }
    } else {
      G = D >> 4;
      qw = *(const u32x4a GAS*)((const uint8_t GAS*)p.rr_queries + qabs * D + 16u * ((uint32_t)lane & (G - 1u)));
      qq = xdot4<DT == BANG_I8>(qw.x, qw.x, xdot4<DT == BANG_I8>(qw.y, qw.y, xdot4<DT == BANG_I8>(qw.z, qw.z, xdot4<DT == BANG_I8>(qw.w, qw.w, 0))));
    }

    // ---------------- per-query state: candidate log = [MEDOID], one row: the seed list [MEDOID, adj(MEDOID)...]
    uint32_t iter = 1, w_n = 0, cc = 1, evals = 0, fetched = 0, nrows = 1;
    if (lane == 0) p.d_cand_ids[(size_t)q * cand_stride] = medoid;
    uint32_t x[BEAM_MAX], cnt[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) { x[j] = 0u; cnt[j] = 0u; }
    cnt[0] = p.d_seed[0]; x[0] = p.d_seed[1 + lane];
    uint32_t x1 = p.d_seed[65];

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

      // ---------------- step 3: exact distances, one call over every kept survivor
      if (tot > 0u) {
        if (DT == BANG_F32) beam_dist_f32(graph, entry_len, D, bid, tot, bdist, qr, lane);
        else beam_dist8<DT == BANG_I8>(graph, entry_len, G, bid, tot, bdist, qw, qq, lane);
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
          // all 64 lanes load one dword of the row.  Slice parent / slice_rows of the node's HBM-resident rows (this GPU's HBM or a peer's over
          // xGMI; 0: that slice is not there), else the HBM copy of the first n_rows_hbm rows, else pinned host memory over PCIe
          const uint32_t GAS* hb_rows = nullptr;
          if (p.n_slices > 1u) {
            const uint32_t sl = parent / p.slice_rows;            // (uniform: scalar)
            if (sl < p.n_slices) hb_rows = (const uint32_t GAS*)slice_base(p.d_row_slices, sl);
          } else if (parent < p.n_rows_hbm) hb_rows = (const uint32_t GAS*)p.d_rows_hbm;
          if (hb_rows) x[j] = hb_rows[(uint64_t)parent * 64u + (uint32_t)lane];
          else {
            x[j] = __builtin_nontemporal_load((const uint32_t GAS*)p.d_graph + (uint64_t)parent * 64u + (uint32_t)lane);
            asm volatile("; row from host memory");               // (keeps this load apart from the plain one: merged, the two lose the hint)
          }
          cnt[j] = 64u;                                           // counted when the row is consumed
#else
          const uint32_t GAS* nrow = (const uint32_t GAS*)(graph + (uint64_t)parent * entry_len + p.vec_bytes);
          cnt[j] = nrow[0];
          x[j] = nrow[1 + ((uint32_t)lane < R ? (uint32_t)lane : 0u)];
#endif
        }
      }
      wave_sync();                                                // (psel is read before the next iteration's sort overwrites it)
      ++iter;
    }

    // ---------------- the query is finished: counters, then the results straight from the worklist (CANON 11)
    if (lane == 0) {
      p.d_cand_cnt[q] = cc;
      if (p.d_qstats) { p.d_qstats[(size_t)q * 2] = evals; p.d_qstats[(size_t)q * 2 + 1] = fetched; }
      if (p.d_qiters) p.d_qiters[q] = iter;
    }
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
  if (p.d_ktime) {
    __syncthreads();
    if (threadIdx.x == 0) p.d_ktime[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
  }
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

static uint32_t beam_wave_bytes(uint32_t L, uint32_t beam) { return (beam_wl_words(L) + BEAM_SCRATCH_WORDS + 2u * beam_row_words(beam)) * 4u; }

// Waves per CU as bang_search_exact_geometry: what the instance's registers allow (512 per SIMD lane, allocated in granules of 8, four SIMDs,
// at most 8 waves per SIMD) and what 160 KB of LDS hold -- 2L + L/4 + 144 + 2 (64 beam + 4) words per wave --, at most 32; one workgroup of at
// most 16 waves; a batch of fewer than a workgroup-full of queries per CU is spread over all CUs with fewer waves each.
extern "C" int BEAM_GEOMETRY(int dtype, uint32_t L, uint32_t beam, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves) {
  if (!workgroups || !waves || Q == 0) return BANG_ERR_ARG;
  if (beam == 0 || beam > BEAM_MAX) { bang_set_error("distance = 1: beam = %u is outside [1, %d]", beam, BEAM_MAX); return BANG_ERR_ARG; }
  const void* k = beam_instance(dtype);
  if (!k || L == 0 || L > BANG_MAX_L) { bang_set_error("distance = 1, beam = %u: bad dtype / L", beam); return BANG_ERR_ARG; }
  static int regs[3][BANG_MAX_DEVICES] = {}, max_waves_wg[3][BANG_MAX_DEVICES] = {};   // per instance and device, read once
  const int dev = current_device();
  if (regs[dtype][dev] == 0) {
    hipFuncAttributes at;
    HIP_TRY(hipFuncGetAttributes(&at, k));
    max_waves_wg[dtype][dev] = at.maxThreadsPerBlock >= WAVE ? at.maxThreadsPerBlock / WAVE : 16;
    regs[dtype][dev] = at.numRegs > 0 ? at.numRegs : 128;
  }
  const uint32_t vg = (uint32_t)regs[dtype][dev];
  const uint32_t alloc = (vg + 7u) & ~7u;
  uint32_t per_simd = 512u / alloc;
  if (per_simd > 8u) per_simd = 8u;
  uint32_t per_cu = 4u * per_simd;
  const uint32_t by_lds = BEAM_MAX_LDS / beam_wave_bytes(L, beam);
  if (by_lds < per_cu) per_cu = by_lds;
  if (per_cu > 32u) per_cu = 32u;
  if (per_cu == 0) { bang_set_error("distance = 1, beam = %u: one wave's worklist does not fit LDS at L=%u", beam, L); return BANG_ERR_UNSUPPORTED; }
  uint32_t W = per_cu < 16u ? per_cu : 16u;
  if (W > (uint32_t)max_waves_wg[dtype][dev]) W = (uint32_t)max_waves_wg[dtype][dev];     // (the instance's launch bound)
  const uint32_t wgs_per_cu = per_cu / W;
  if (max_waves && max_waves < W) W = max_waves;
  const uint32_t cus = (uint32_t)num_cus();
  uint32_t grid_n;
  if (Q <= cus * W) {                                             // fewer queries than a wave-full per CU: all CUs, fewer waves each
    grid_n = Q < cus ? Q : cus;
    if (max_wgs && max_wgs < grid_n) grid_n = max_wgs;
    const uint32_t share = (Q + grid_n - 1) / grid_n;
    if (share < W) W = share;
  } else {
    const uint32_t want = (Q + W - 1) / W;
    grid_n = cus * wgs_per_cu;
    if (want < grid_n) grid_n = want;
    if (max_wgs && max_wgs < grid_n) grid_n = max_wgs;
  }
  *workgroups = grid_n;
  *waves = W;
  return BANG_OK;
}

// one launch of this translation unit's instances (the arguments are checked: bang_k_search_exact_beam)
static int beam_launch(const bang_search_params* p, uint32_t beam, void* stream) {
  uint32_t grid_n = 0, waves = 0;
  const int rc = BEAM_GEOMETRY((int)p->rr_dtype, p->L, beam, p->Q, p->max_wgs, p->max_waves, &grid_n, &waves);
  if (rc != BANG_OK) return rc;
  BeamArgs a;
  a.p = *p;
  a.beam = beam;
  a.wl_words = beam_wl_words(p->L);
  a.row_words = beam_row_words(beam);
  a.wave_words = a.wl_words + BEAM_SCRATCH_WORDS + 2u * a.row_words;
  const size_t lds = (size_t)waves * a.wave_words * 4u;
  const void* k = beam_instance((int)p->rr_dtype);
  static bool attr_done[3][BANG_MAX_DEVICES] = {};
  const int dev = current_device();
  if (!attr_done[p->rr_dtype][dev]) {
    HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BEAM_MAX_LDS));
    attr_done[p->rr_dtype][dev] = true;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_n), block(waves * WAVE);
  if (p->rr_dtype == BANG_F32) hipLaunchKernelGGL(BEAM_KERNEL<BANG_F32>, grid, block, lds, st, a);
  else if (p->rr_dtype == BANG_I8) hipLaunchKernelGGL(BEAM_KERNEL<BANG_I8>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(BEAM_KERNEL<BANG_U8>, grid, block, lds, st, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
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

extern "C" int bang_k_search_exact_beam(const bang_search_params* p, uint32_t beam, void* stream) {
  if (!p) return BANG_ERR_ARG;
  if (beam == 0 || beam > BEAM_MAX) { bang_set_error("distance = 1: beam = %u is outside [1, %d]", beam, BEAM_MAX); return BANG_ERR_ARG; }
  if (p->Q == 0) return BANG_OK;
  if (p->R == 0 || p->R > BANG_MAX_R || p->L == 0 || p->L > BANG_MAX_L) { bang_set_error("distance = 1, beam = %u: bad R/L", beam); return BANG_ERR_ARG; }
  if (p->row_layout > 1u) { bang_set_error("distance = 1, beam = %u: row_layout = %u: the adjacency lists are graph entries in HBM (0) or 256-byte rows (1)", beam, p->row_layout); return BANG_ERR_UNSUPPORTED; }
  if (p->row_layout == 0u && !p->d_graph) { bang_set_error("distance = 1, beam = %u: the kernel needs the graph entries in HBM (d_graph, row_layout = 0)", beam); return BANG_ERR_UNSUPPORTED; }
  if (!p->d_seed || !p->d_bloom || !p->d_cand_ids || !p->d_cand_cnt || !p->d_next_query || !p->rr_queries || !p->rr_ids_out || !p->rr_dists_out) {
    bang_set_error("distance = 1, beam = %u: null buffer", beam); return BANG_ERR_ARG;
  }
  if (p->cap_iter == 0 || p->cap_iter > p->L + BANG_EXTRA_ITERS - 1) { bang_set_error("distance = 1, beam = %u: bad iteration cap", beam); return BANG_ERR_ARG; }
  if (p->rr_k == 0 || p->rr_k > p->L || p->rr_Q_total < p->rr_q0 + p->Q) { bang_set_error("distance = 1, beam = %u: bad k / result rows", beam); return BANG_ERR_ARG; }
  if (p->rr_vec_f16 > 1u) { bang_set_error("distance = 1, beam = %u: rr_vec_f16 = %u (0 = float / 8-bit rows, 1 = fp16 rows)", beam, p->rr_vec_f16); return BANG_ERR_ARG; }
  if (p->rr_vec_f16 == 1u) { bang_set_error("distance = 1, beam = %u: rr_vec_f16 = 1 (an fp16 vector table) has no beam instance", beam); return BANG_ERR_UNSUPPORTED; }
  if (p->row_layout == 1u) {
    // the pulled-rows form: adjacency rows in d_graph (pinned host memory; 4-byte aligned), vectors at rr_vec_base + id * rr_vec_stride
    if (!p->d_graph || (((uintptr_t)p->d_graph) & 3u)) { bang_set_error("distance = 1, beam = %u, row_layout = 1: d_graph (the 256-byte adjacency rows) is null or not 4-byte aligned", beam); return BANG_ERR_ARG; }
    if (p->R > 64u) { bang_set_error("distance = 1, beam = %u, row_layout = 1: R = %u, a 256-byte row holds 64 ids", beam, p->R); return BANG_ERR_ARG; }
    if (!p->rr_vec_base || (((uintptr_t)p->rr_vec_base) & 3u)) { bang_set_error("distance = 1, beam = %u, row_layout = 1: rr_vec_base (the vectors) is null or not 4-byte aligned", beam); return BANG_ERR_ARG; }
    if (!bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->rr_vec_stride)) {
      bang_set_error("distance = 1, beam = %u, row_layout = 1: rr_vec_stride = %llu does not describe vectors the kernel evaluates (dtype %u, D = %u): 8-bit vectors "
                     "need D %% 16 == 0, float vectors D %% 4 == 0; a stride divisible by 4 that holds the vector", beam, (unsigned long long)p->rr_vec_stride,
                     p->rr_dtype, p->rr_D);
      return BANG_ERR_ARG;
    }
    if (p->vec_bytes != p->rr_D * (p->rr_dtype == BANG_F32 ? 4u : 1u)) { bang_set_error("distance = 1, beam = %u, row_layout = 1: vec_bytes = %u is not rr_D * the element size", beam, p->vec_bytes); return BANG_ERR_ARG; }
    if (((uintptr_t)p->rr_queries) & 3u) { bang_set_error("distance = 1, beam = %u, row_layout = 1: rr_queries is not 4-byte aligned", beam); return BANG_ERR_ARG; }
    if (p->n_slices > 1u && !p->d_row_slices) { bang_set_error("distance = 1, beam = %u, row_layout = 1: n_slices = %u needs the slice table d_row_slices", beam, p->n_slices); return BANG_ERR_ARG; }
    if (p->n_slices > 1u && p->slice_rows == 0u) { bang_set_error("distance = 1, beam = %u, row_layout = 1: n_slices = %u needs slice_rows != 0", beam, p->n_slices); return BANG_ERR_ARG; }
    if (p->n_rows_hbm != 0u && !p->d_rows_hbm) { bang_set_error("distance = 1, beam = %u, row_layout = 1: n_rows_hbm = %u needs d_rows_hbm", beam, p->n_rows_hbm); return BANG_ERR_ARG; }
    if (!bang_search_exact_beam_supported((int)p->rr_dtype, p->rr_D, p->rr_vec_stride)) {
      bang_set_error("distance = 1, beam = %u: the wide vector layouts (dtype %u, D = %u) have no beam instance: 8-bit D / 16 a power of two, D <= 256", beam, p->rr_dtype, p->rr_D);
      return BANG_ERR_UNSUPPORTED;
    }
    return bang_k_search_exact_beam_pull(p, beam, stream);
  }
  if (!bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->entry_len) || p->vec_bytes != p->rr_D * (p->rr_dtype == BANG_F32 ? 4u : 1u) ||
      (((uintptr_t)p->d_graph) & 3u) || (((uintptr_t)p->rr_queries) & 3u)) {
    bang_set_error("distance = 1, beam = %u: unsupported vector layout (dtype %u, D = %u, entry stride %llu): 8-bit vectors need D %% 16 == 0, float vectors "
                   "D %% 4 == 0; an entry stride divisible by 4", beam, p->rr_dtype, p->rr_D, (unsigned long long)p->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  if (!bang_search_exact_beam_supported((int)p->rr_dtype, p->rr_D, p->entry_len)) {
    bang_set_error("distance = 1, beam = %u: the wide vector layouts (dtype %u, D = %u) have no beam instance: 8-bit D / 16 a power of two, D <= 256", beam, p->rr_dtype, p->rr_D);
    return BANG_ERR_UNSUPPORTED;
  }
  return beam_launch(p, beam, stream);
}
#endif
