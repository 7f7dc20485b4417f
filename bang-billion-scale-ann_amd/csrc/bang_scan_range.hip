// bang_scan_range.hip -- the exact range scan (DESIGN.md section 2 CANON 26, section 4.20): every candidate within a per-query radius, by brute
// force, up to BANG_RANGE_MAX_HITS per query.  An answer's size is known only after the distances are, so nothing is selected while the products
// run (no lists, no thresholds): the launch sequence is COUNT, PREFIX, EMIT, SORT.
//
//  * The points [0, n_nodes) are cut into `runs` contiguous runs of whole 32-point tiles.  A run is ONE WAVE's share and is walked in ascending
//    id order; a workgroup is four runs of one tile of queries, which it stages once into LDS.
//  * count: counts[q][run] = the hits of query q in the run.  prefix (one wave per query): the exclusive scan of counts[q][.] in place and
//    offered[q].  emit: the same grid and the same arithmetic; a hit's position is counts[q][run] + its rank among the run's hits in id order --
//    a ballot, mbcnt and a running count per query row carried from tile to tile in registers -- and positions < max_hits are written with plain
//    vector stores.  No atomic decides a position: the rows hold the first min(offered, max_hits) hits in id order whatever the grid.  sort:
//    bang_k_range_sort (bang_range.hip) on those rows as they are.  The products are paid twice; one pass with an atomic append would keep a
//    different subset whenever a row truncates, and a one-pass variant that holds distances back needs nq x n_nodes words.
//  * scan_range8_kernel<IS_U8, EMIT>: 32 queries x 32 points per v_mfma_i32_32x32x32_i8 with a runtime number of k-steps, |a|^2 - 2 a.b + |b|^2 in
//    i32 with uint8 read as int8 after ^ 0x80, norms by v_dot4; the query image is piece-major (the 16-byte piece lane (r, h) feeds k-step s at
//    16 (64 s + lane): one conflict-free ds_read_b128 per k-step), the points stream in 16-byte loads four k-steps ahead, the last k-step is
//    loaded SHORT (no byte behind a row is read).  THE HIT TEST RUNS ON THE ACCUMULATOR REGISTERS: register i of lane (r, h) is query row
//    (i & 3) + 8 (i >> 2) + 4 h, point column r, so a ballot of register i holds one query row per half-wave in id order -- a popcount per half
//    is the row's count, mbcnt below the lane the rank.  Sums beyond 2^24: with a radius below 2^24 no hit (the chain's value is >= 2^24 exactly
//    when the integer is), else the lane re-evaluates the canonical chain, as scan8_any_kernel does, before the ballots.
//  * scan_range_f32_kernel<EMIT>: one lane per point, 16 queries per tile, query elements broadcast from LDS, the canonical ascending fmaf chain
//    over 16-byte pieces and a dword tail; a ballot per query is already in id order.
//  * Typed global pointers (GAS), 64-bit row and output offsets, vector stores only, no private segment.
#include "bang_scan_select.h"

#define RANGE_WAVES 4u                                                      // runs per workgroup
#define RANGE8_QT 32
#define RANGEF_QT 16
#define RANGE8_U 4                                                          // k-steps of point bytes in flight per lane

struct RangeArgs {
  const uint8_t* vec_base; uint64_t vec_stride;
  const void* queries; const float* radius;
  const uint32_t* excl; const uint32_t* removed; const uint32_t* labels; const uint32_t* filters;
  uint32_t* counts;                                      // [nq][runs]: hits per run, then (prefix) the run's first position
  uint32_t* hit_ids; uint32_t* hit_dists; uint32_t* offered; uint32_t* matched;
  uint64_t per;                                          // points of a run, a multiple of 32
  uint32_t D, n_nodes, nq, max_hits, runs;
};

template <int QT>
struct RangeLds {
  float rad[QT];                                         // NaN behind nq: such a row has no hit
  uint32_t flt[QT][2];
  uint32_t mcnt[QT];
  int qnorm[QT];
  uint32_t mall;
};
#define RANGE_IMG(QT) ((sizeof(RangeLds<QT>) + 15u) & ~(size_t)15u)       // offset of the query image in the workgroup's LDS

template <int QT>
__device__ __forceinline__ void range_lds_init(RangeLds<QT>& s, const RangeArgs& a, uint32_t q0) {
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)QT) {
    const uint32_t q = q0 + t;
    const bool in = q < a.nq, f = a.filters != nullptr && in;
    s.rad[t] = in ? ((const float GAS*)a.radius)[q] : __uint_as_float(0x7FC00000u);
    s.flt[t][0] = f ? ((const uint32_t GAS*)a.filters)[2ull * q] : 0u;
    s.flt[t][1] = f ? ((const uint32_t GAS*)a.filters)[2ull * q + 1u] : 0u;
    s.mcnt[t] = 0u; s.qnorm[t] = 0;
  }
  if (t == 0u) s.mall = 0u;
}

// the end of the count pass: the candidates of this workgroup's runs to matched[q] -- one atomic add per query, a sum is order-free
template <int QT>
__device__ __forceinline__ void range_matched_out(RangeLds<QT>& s, const RangeArgs& a, uint32_t q0) {
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)QT && q0 + t < a.nq) {
    const uint32_t m = s.mcnt[t] + s.mall;
    if (m != 0u) (void)__hip_atomic_fetch_add((uint32_t GAS*)a.matched + q0 + t, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ int range8_norm(i32x4 f, int norm) {
  norm = __builtin_amdgcn_sdot4(f.x, f.x, norm, false);
  norm = __builtin_amdgcn_sdot4(f.y, f.y, norm, false);
  norm = __builtin_amdgcn_sdot4(f.z, f.z, norm, false);
  return __builtin_amdgcn_sdot4(f.w, f.w, norm, false);
}

// the canonical chain of one (query row, point) pair: ascending, (float)(v - q), fmaf.  D % 4 == 0; the image holds the shifted query
template <bool IS_U8>
__device__ __forceinline__ float range8_chain(const uint32_t* img, uint32_t qrow, const uint8_t GAS* v, uint32_t D) {
  float acc = 0.0f;
  for (uint32_t j = 0; j < D; j += 4u) {
    const uint32_t pw = *(const uint32_t GAS*)(v + j);
    uint32_t qw = img[(64u * (j >> 5) + 32u * ((j >> 4) & 1u) + qrow) * 4u + ((j & 15u) >> 2)];
    if (IS_U8) qw ^= 0x80808080u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int pv = IS_U8 ? (int)((pw >> (8 * e)) & 0xffu) : (int)(int8_t)(pw >> (8 * e));
      const int qv = IS_U8 ? (int)((qw >> (8 * e)) & 0xffu) : (int)(int8_t)(qw >> (8 * e));
      const float diff = (float)(pv - qv);                                 // vector - query, as orc_exact_dist
      acc = __builtin_fmaf(diff, diff, acc);
    }
  }
  return acc;
}

template <bool IS_U8, bool EMIT>
__global__ __launch_bounds__(256) void scan_range8_kernel(const RangeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t range_smem[];
  RangeLds<RANGE8_QT>& s = *(RangeLds<RANGE8_QT>*)range_smem;
  i32x4* qimg = (i32x4*)(range_smem + RANGE_IMG(RANGE8_QT));               // [KS][64]: piece 64 s + lane
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t r = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
  const uint32_t q0 = blockIdx.x * RANGE8_QT, run = blockIdx.y * RANGE_WAVES + wave;
  const uint32_t D = a.D;
  const uint32_t KSF = D >> 5, KS = (D + 31u) >> 5;                        // (uniform) whole k-steps, all k-steps
  range_lds_init(s, a, q0);
  __syncthreads();
  // the tile's queries, once per workgroup: shifted, int8 0 behind D; a row behind nq repeats the last query (its radius is NaN)
  for (uint32_t idx = threadIdx.x; idx < KS * 64u; idx += 256u) {
    const uint32_t rr = idx & 31u, b = 32u * (idx >> 6) + 16u * ((idx >> 5) & 1u);
    const uint32_t q = q0 + rr < a.nq ? q0 + rr : a.nq - 1u;
    const uint8_t GAS* src = (const uint8_t GAS*)a.queries + (uint64_t)q * D;        // (D % 4 == 0: rows are dword-aligned)
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t j = b + 4u * (uint32_t)i;
      w[i] = 0u;
      if (j < D) { w[i] = *(const uint32_t GAS*)(src + j); if (IS_U8) w[i] ^= 0x80808080u; }
    }
    const i32x4 f = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    qimg[idx] = f;
    const int part = range8_norm(f, 0);
    if (part != 0) (void)__hip_atomic_fetch_add(&s.qnorm[rr], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const bool mine_run = run < a.runs;                                      // (uniform per wave: the last workgroup of a column may hold idle waves)
  const uint64_t p_begin = (uint64_t)run * a.per;
  uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  if (!mine_run) p_stop = 0ull;
  // register i of lane (r, h): query row (i & 3) + 8 (i >> 2) + 4 h.  cnt of lane (i, h), i < 16: the hits of that row so far (emit: from the
  // run's first position) -- the 32 running counts of a wave in one register
  const uint32_t cq = q0 + ((r & 3u) + 8u * ((r >> 2) & 3u)) + 4u * h;     // the query whose count this lane keeps (r < 16)
  uint32_t cnt = 0u;
  if (EMIT && mine_run && r < 16u && cq < a.nq) cnt = ((const uint32_t GAS*)a.counts)[(uint64_t)cq * a.runs + run];
  // the short k-step: dwords of this lane's piece inside the row
  const uint32_t tail_at = 32u * KSF + 16u * h;
  const uint32_t tail_dw = D > tail_at ? ((D - tail_at) >> 2 < 4u ? (D - tail_at) >> 2 : 4u) : 0u;
  uint32_t unfiltered = 0u;                                                // (uniform) valid points of this wave's tiles
  for (uint64_t base = p_begin; base < p_stop; base += 32u) {              // (uniform over the wave) one 32-point tile per trip, ascending
    const uint64_t pt64 = base + r;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;        // (p_begin < n_nodes here)
    const uint8_t GAS* row = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;
    const uint8_t GAS* mine = row + 16u * h;
    u32x4a cur[RANGE8_U], nxt[RANGE8_U];
#pragma unroll
    for (int u = 0; u < RANGE8_U; ++u) {
      cur[u] = (u32x4a){0u, 0u, 0u, 0u};
      if ((uint32_t)u < KSF) cur[u] = *(const u32x4a GAS*)(mine + 32u * (uint32_t)u);          // (uniform)
    }
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int pn = 0;
    for (uint32_t s0 = 0; s0 < KSF; s0 += RANGE8_U) {                      // (uniform)
#pragma unroll
      for (int u = 0; u < RANGE8_U; ++u) {
        nxt[u] = (u32x4a){0u, 0u, 0u, 0u};
        const uint32_t ks = s0 + RANGE8_U + (uint32_t)u;
        if (ks < KSF) nxt[u] = *(const u32x4a GAS*)(mine + 32u * ks);      // (uniform)
      }
#pragma unroll
      for (int u = 0; u < RANGE8_U; ++u) {
        const uint32_t ks = s0 + (uint32_t)u;
        if (ks < KSF) {                                                    // (uniform)
          u32x4a w = cur[u];
          if (IS_U8) { w.x ^= 0x80808080u; w.y ^= 0x80808080u; w.z ^= 0x80808080u; w.w ^= 0x80808080u; }
          const i32x4 bf = {(int)w.x, (int)w.y, (int)w.z, (int)w.w};
          pn = range8_norm(bf, pn);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * ks + (uint32_t)lane], bf, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < RANGE8_U; ++u) cur[u] = nxt[u];
    }
    if (KS != KSF) {                                                       // (uniform) the short k-step: only the dwords that exist
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      const uint8_t GAS* t = row + tail_at;
      if (tail_dw == 4u) {
        const u32x4a x = *(const u32x4a GAS*)t;
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
      } else {
        if (tail_dw > 0u) w[0] = *(const uint32_t GAS*)t;
        if (tail_dw > 1u) w[1] = *(const uint32_t GAS*)(t + 4);
        if (tail_dw > 2u) w[2] = *(const uint32_t GAS*)(t + 8);
      }
      if (IS_U8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if ((uint32_t)i < tail_dw) w[i] ^= 0x80808080u;
      }
      const i32x4 bf = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
      pn = range8_norm(bf, pn);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * KSF + (uint32_t)lane], bf, acc, 0, 0, 0);
    }
    pn += __shfl_xor(pn, 32);                                              // both halves of the column
    if (!EMIT && !filtered) unfiltered += (uint32_t)__popc((uint32_t)__ballot(valid));        // (the low half: each point once)
    // the hit test on the accumulator registers; acc[i] becomes the distance bits
    uint32_t hits = 0u, slow = 0u;                                         // bit i: register i is a hit / a sum beyond 2^24 under a radius that reaches it
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qrow = (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
      const int d = s.qnorm[qrow] + pn - 2 * acc[i];
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[qrow][0], s.flt[qrow][1]);
        if (!EMIT) {
          const uint64_t mb = __ballot(m);
          const uint32_t hm = h ? (uint32_t)(mb >> 32) : (uint32_t)mb;
          if (r == 0u && hm != 0u) (void)__hip_atomic_fetch_add(&s.mcnt[qrow], (uint32_t)__popc(hm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      const float rad = s.rad[qrow], fd = (float)d;
      const bool big = d > (1 << 24);
      if (m && !big && fd <= rad) hits |= 1u << i;
      if (m && big && rad >= 16777216.0f) slow |= 1u << i;
      acc[i] = (int)__float_as_uint(fd);
    }
    if (__ballot(slow != 0u) != 0ull) {                                    // (uniform) only where sums pass 2^24 under such a radius
#pragma unroll 1
      for (uint32_t i = 0; i < 16u; ++i) {
        const bool again = ((slow >> i) & 1u) != 0u;
        if (__ballot(again) == 0ull) continue;                             // (uniform)
        const uint32_t qrow = (i & 3u) + 8u * (i >> 2) + 4u * h;
        float c = 0.0f;
        if (again) c = range8_chain<IS_U8>((const uint32_t*)qimg, qrow, row, D);
        if (again && c <= s.rad[qrow]) hits |= 1u << i;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (again && (uint32_t)k == i) acc[k] = (int)__float_as_uint(c);      // (register k by a constant index)
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool hit = ((hits >> i) & 1u) != 0u;
      const uint64_t hb = __ballot(hit);
      const uint32_t hm = h ? (uint32_t)(hb >> 32) : (uint32_t)hb;         // this half's query row, bit = point column: id order
      if (EMIT) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)cnt, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)cnt, 32 + i);
        const uint32_t pos = (h ? hi : lo) + (uint32_t)__popc(hm & ((1u << r) - 1u));
        if (hit && pos < a.max_hits) {
          const uint64_t at = (uint64_t)(q0 + (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h) * a.max_hits + pos;
          ((uint32_t GAS*)a.hit_ids)[at] = pt;
          ((uint32_t GAS*)a.hit_dists)[at] = (uint32_t)acc[i];
        }
      }
      if (r == (uint32_t)i) cnt += (uint32_t)__popc(hm);
      __builtin_amdgcn_sched_barrier(0);                                   // (one row's ballot at a time: sixteen live ballots cost scalar registers)
    }
  }
  if (!EMIT) {
    if (mine_run && r < 16u && cq < a.nq) ((uint32_t GAS*)a.counts)[(uint64_t)cq * a.runs + run] = cnt;
    if (!filtered && lane == 0 && unfiltered != 0u) (void)__hip_atomic_fetch_add(&s.mall, unfiltered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    range_matched_out(s, a, q0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// float vectors
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rangef_step(float (&acc)[RANGEF_QT], float x, const float* qd) {
#pragma unroll
  for (int j = 0; j < RANGEF_QT; ++j) {
    const float diff = x - qd[j];                                          // vector - query, as orc_exact_dist
    acc[j] = __builtin_fmaf(diff, diff, acc[j]);                           // ascending dimension
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void scan_range_f32_kernel(const RangeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t range_smem[];
  RangeLds<RANGEF_QT>& s = *(RangeLds<RANGEF_QT>*)range_smem;
  float* qv = (float*)(range_smem + RANGE_IMG(RANGEF_QT));                 // [D][16]: element d of the tile's queries
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t q0 = blockIdx.x * RANGEF_QT, run = blockIdx.y * RANGE_WAVES + wave;
  const uint32_t D = a.D, D4 = a.D & ~3u;
  range_lds_init(s, a, q0);
  for (uint32_t i = threadIdx.x; i < D * RANGEF_QT; i += 256u) {
    const uint32_t d = i / RANGEF_QT, j = i % RANGEF_QT;
    const uint32_t q = q0 + j < a.nq ? q0 + j : a.nq - 1u;
    qv[i] = ((const float GAS*)a.queries)[(uint64_t)q * D + d];
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const bool mine_run = run < a.runs;                                      // (uniform per wave)
  const uint64_t p_begin = (uint64_t)run * a.per;
  uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  if (!mine_run) p_stop = 0ull;
  const uint32_t cq = q0 + (uint32_t)lane;                                 // lane j < 16 keeps the hits of query j so far (emit: from the run's first position)
  uint32_t cnt = 0u;
  if (EMIT && mine_run && lane < RANGEF_QT && cq < a.nq) cnt = ((const uint32_t GAS*)a.counts)[(uint64_t)cq * a.runs + run];
  uint32_t unfiltered = 0u;
  for (uint64_t base = p_begin; base < p_stop; base += WAVE) {             // (uniform over the wave) 64 points per trip, ascending
    const uint64_t pt64 = base + (uint32_t)lane;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;
    const uint8_t GAS* v = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;     // (dword-aligned only: u32x4a is typed so)
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    float acc[RANGEF_QT];
#pragma unroll
    for (int j = 0; j < RANGEF_QT; ++j) acc[j] = 0.0f;
    for (uint32_t d = 0; d < D4; d += 4u) {                                // (uniform) the whole 16-byte pieces
      const u32x4a w = *(const u32x4a GAS*)(v + 4u * d);
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) rangef_step(acc, __uint_as_float(ww[e]), qv + (d + (uint32_t)e) * RANGEF_QT);
    }
    for (uint32_t d = D4; d < D; ++d)                                      // (uniform) the last D % 4 elements, one dword each
      rangef_step(acc, __uint_as_float(*(const uint32_t GAS*)(v + 4u * d)), qv + d * RANGEF_QT);
    if (!EMIT && !filtered) unfiltered += (uint32_t)__popcll(__ballot(valid));
#pragma unroll
    for (int j = 0; j < RANGEF_QT; ++j) {
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[j][0], s.flt[j][1]);
        if (!EMIT) {
          const uint64_t mb = __ballot(m);
          if (lane == 0 && mb != 0ull) (void)__hip_atomic_fetch_add(&s.mcnt[j], (uint32_t)__popcll(mb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      const bool hit = m && acc[j] <= s.rad[j];
      const uint64_t hb = __ballot(hit);                                   // bit = lane = point: id order
      if (EMIT) {
        const uint32_t pos = (uint32_t)__builtin_amdgcn_readlane((int)cnt, j) + lanes_below(hb);
        if (hit && pos < a.max_hits) {
          const uint64_t at = (uint64_t)(q0 + (uint32_t)j) * a.max_hits + pos;
          ((uint32_t GAS*)a.hit_ids)[at] = pt;
          ((uint32_t GAS*)a.hit_dists)[at] = __float_as_uint(acc[j]);
        }
      }
      if (lane == j) cnt += (uint32_t)__popcll(hb);
      __builtin_amdgcn_sched_barrier(0);                                   // (one query's ballot at a time)
    }
  }
  if (!EMIT) {
    if (mine_run && lane < RANGEF_QT && cq < a.nq) ((uint32_t GAS*)a.counts)[(uint64_t)cq * a.runs + run] = cnt;
    if (!filtered && lane == 0 && unfiltered != 0u) (void)__hip_atomic_fetch_add(&s.mall, unfiltered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    range_matched_out(s, a, q0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// prefix: one wave per query, the exclusive scan of its runs' counts in place; offered[q] = the total
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_range_prefix_kernel(const RangeArgs a) {
  const int lane = lane_id();
  const uint32_t q = blockIdx.x * RANGE_WAVES + uni(threadIdx.x >> 6);
  if (q >= a.nq) return;                                                   // (uniform per wave; the kernel has no workgroup barrier)
  uint32_t GAS* row = (uint32_t GAS*)a.counts + (uint64_t)q * a.runs;
  uint32_t carry = 0u;
  for (uint32_t i0 = 0; i0 < a.runs; i0 += WAVE) {                         // (uniform)
    const uint32_t i = i0 + (uint32_t)lane;
    const uint32_t v = i < a.runs ? row[i] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= off) incl += t;
    }
    if (i < a.runs) row[i] = carry + incl - v;
    carry += (uint32_t)__shfl((int)incl, WAVE - 1);
  }
  if (lane == 0) ((uint32_t GAS*)a.offered)[q] = carry;
}

// ---------------------------------------------------------------------------------------------------------------------
// the entry: checks, then count, prefix, emit, sort in stream order
// ---------------------------------------------------------------------------------------------------------------------
// One launch of instance KERNEL.  The float image of D = 1024 takes more than the 64 KB of dynamic LDS a kernel may ask for unprompted: the
// instance's limit is raised once per device to lds_most, the most a launch of it ever asks for
template <auto KERNEL>
static int range_launch(const RangeArgs& a, dim3 grid, size_t lds, size_t lds_most, void* stream) {
  static bool raised[BANG_MAX_DEVICES] = {false};
  const int dev = current_device();
  if (!raised[dev]) {
    HIP_TRY(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_most));
    raised[dev] = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

template <bool EMIT>
static int range_pass(const RangeArgs& a, uint32_t dtype, dim3 grid, void* stream) {
  if (dtype == BANG_F32)
    return range_launch<scan_range_f32_kernel<EMIT>>(a, grid, RANGE_IMG(RANGEF_QT) + (size_t)a.D * RANGEF_QT * 4,
                                                     RANGE_IMG(RANGEF_QT) + (size_t)BANG_SCAN_ANY_MAX_D * RANGEF_QT * 4, stream);
  const size_t lds = RANGE_IMG(RANGE8_QT) + (size_t)((a.D + 31u) / 32u) * 1024u, most = RANGE_IMG(RANGE8_QT) + (size_t)BANG_SCAN_ANY_MAX_D * 32u;
  if (dtype == BANG_U8) return range_launch<scan_range8_kernel<true, EMIT>>(a, grid, lds, most, stream);
  return range_launch<scan_range8_kernel<false, EMIT>>(a, grid, lds, most, stream);
}

extern "C" int bang_k_scan_range(const bang_scan_range_params* p, void* stream) { return bang_k_scan_range_marked(p, stream, nullptr, nullptr); }

extern "C" int bang_k_scan_range_marked(const bang_scan_range_params* p, void* stream, void* ev_emit, void* ev_sort) {
  {
    const int rc = bang_scan_range_check(p);
    if (rc != BANG_OK) return rc;
  }
  uint32_t tiles = 0, runs = 0;
  {
    const int rc = bang_scan_range_geometry((int)p->dtype, p->D, p->nq, p->n_nodes, &tiles, &runs, nullptr);
    if (rc != BANG_OK) { bang_set_error("bang_k_scan_range: no geometry for this launch"); return rc; }
  }
  if (p->runs != 0u) runs = p->runs;
  RangeArgs a;
  a.vec_base = p->d_vec_base; a.vec_stride = p->vec_stride; a.queries = p->d_queries; a.radius = p->d_radius;
  a.excl = p->d_excluded; a.removed = p->d_removed; a.labels = p->d_labels; a.filters = p->d_filters;
  a.counts = (uint32_t*)p->d_scratch; a.hit_ids = p->d_hit_ids; a.hit_dists = (uint32_t*)p->d_hit_dists; a.offered = p->d_offered;
  a.matched = p->d_matched;
  a.D = p->D; a.n_nodes = p->n_nodes; a.nq = p->nq; a.max_hits = p->max_hits; a.runs = runs;
  const uint64_t tiles32 = ((uint64_t)p->n_nodes + 31u) / 32u;
  a.per = (tiles32 + runs - 1u) / runs * 32u;                              // (runs behind the last point are empty: they count 0)
  const dim3 grid(tiles, (runs + RANGE_WAVES - 1u) / RANGE_WAVES);
  HIP_TRY(hipMemsetAsync(p->d_matched, 0, (size_t)p->nq * 4, (hipStream_t)stream));
  BANG_TRY(range_pass<false>(a, p->dtype, grid, stream));
  hipLaunchKernelGGL(scan_range_prefix_kernel, dim3((p->nq + RANGE_WAVES - 1u) / RANGE_WAVES), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  if (ev_emit) HIP_TRY(hipEventRecord((hipEvent_t)ev_emit, (hipStream_t)stream));
  BANG_TRY(range_pass<true>(a, p->dtype, grid, stream));
  if (ev_sort) HIP_TRY(hipEventRecord((hipEvent_t)ev_sort, (hipStream_t)stream));
  return bang_k_range_sort(p->d_hit_ids, p->d_hit_dists, p->d_offered, p->max_hits, 0, p->nq, p->nq, p->d_count, stream);
}
