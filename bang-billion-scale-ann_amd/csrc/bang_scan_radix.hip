// bang_scan_radix.hip -- the exact scan for k up to 4096 (option scan_radix; DESIGN.md section 2 CANON 23, section 4.21): the k smallest keys
// (distance bits << 32) | id of every query by RADIX SELECT over the keys.  No list is kept: per query the device holds a 64-bit prefix, the number
// of its high bits that are fixed, the remaining rank r and a RESOLVED flag, and the launch sequence is
//     init, { HISTOGRAM, PICK } per digit, EMIT, SORT, OUT.
//
//  * Split (the range scan's): the points [0, n_nodes) are cut into `runs` contiguous runs of whole 32-point tiles; a run is ONE WAVE's share and is
//    walked in ascending id order; a workgroup is four runs of one tile of queries, which it stages once into LDS.
//  * Digits are 8 bits wide: four over the distance bits, then the id digits that n_nodes - 1 reaches -- four more at the most.  256 bins per query:
//    the workgroup's histograms take 32 KB (32 queries) / 16 KB (16 queries) of LDS beside the query image.
//  * histogram pass: the products again; a candidate pair whose key lies in [lo, hi] of its query -- lo = the prefix, hi = the prefix with every
//    bit below the fixed ones set -- counts the digit (key >> shift) & 255 in the workgroup's LDS histogram.  The lanes of one ballot that share the
//    FIRST lane's digit add once (the first pass: almost all of them; a later pass: few lanes are left at all), the others one by one.  Non-zero
//    bins go to bins[q][256] in HBM with integer vector atomic adds: a sum is order-free.  A pass with no unresolved query in the batch, and a
//    workgroup with none in its tile, exit at once.
//  * pick pass, one wave per query: four bins per lane, a wave scan, the digit in which the cumulative count crosses r; prefix |= digit << shift,
//    r -= the count below it, the bins zeroed.  The query is RESOLVED when the chosen bin is needed whole (r == its count): the inclusive bound
//    U = prefix | (1 << shift) - 1 then has exactly k keys at or below it.  The first pass also writes matched[q] = the sum of the bins, and a query
//    with fewer than k candidates is resolved with U = ~0.  At shift 0 a bin holds at most one key, so the last pass resolves what is left.
//  * emit pass: the products once more; a candidate with key <= U[q] is appended to row q of ids / distance bits [nq][k] at a position from the
//    query's counter (one vector atomic per ballot).  The SET is fixed by U, so the order does not matter; bang_k_range_sort orders the row and
//    scan_radix_out_kernel widens, transposes and pads.  No position at or beyond k is written.
//  * scan_radix8_kernel<IS_U8, EMIT>: the i8 MFMA tile of scan_range8_kernel (32 queries x 32 points, piece-major query image, 16-byte point loads
//    four k-steps ahead, the last k-step loaded short), the query image staged as scan8_any_kernel does (qdim = D - 1: real 0 in the last byte).
//    The test runs on the accumulator registers; a sum beyond 2^24 whose query's [lo, hi] reaches 2^24 is re-evaluated with the canonical chain
//    before its key is formed.  scan_radix_f32_kernel<EMIT>: one lane per point, 16 queries, the ascending fmaf chain.
//  * Typed global pointers (GAS), 64-bit row and output offsets, vector stores and vector atomics only, no private segment.
#include "bang_scan_select.h"

#define RADIX_WAVES 4u                                                      // runs per workgroup
#define RADIX8_QT 32
#define RADIXF_QT 16
#define RADIX8_U 4                                                          // k-steps of point bytes in flight per lane
#define RADIX_BINS BANG_SCAN_RADIX_BINS
#define RADIX_KEY_2P24 ((uint64_t)0x4B800000u << 32)                        // (bits of 16777216.0f) << 32: no key of a sum beyond 2^24 is below it
#define RADIX_RESOLVED 1u

struct RadixArgs {
  const uint8_t* vec_base; uint64_t vec_stride;
  const void* queries;
  const uint32_t* excl; const uint32_t* removed; const uint32_t* labels; const uint32_t* filters;
  uint64_t* prefix;                                      // [nq]: the fixed high bits of the rank-k key; resolved: the inclusive bound U
  uint32_t* bins;                                        // [nq][256]
  uint32_t* rank;                                        // [nq]: the rank still looked for among the keys under the prefix (1-based)
  uint32_t* fixed;                                       // [nq]: high bits of the prefix that are fixed
  uint32_t* flags;                                       // [nq]: RADIX_RESOLVED
  uint32_t* emitted;                                     // [nq]: keys appended to the row
  uint32_t* count;                                       // [nq]: bang_k_range_sort's count
  uint32_t* row_ids; uint32_t* row_dists;                // [nq][k]
  uint32_t* unresolved;                                  // one word: queries without a bound
  uint32_t* matched;
  uint64_t* ids_out; float* dists_out;
  uint64_t per;                                          // points of a run, a multiple of 32
  uint32_t D, qdim, n_nodes, nq, k, runs, shift;
};

template <int QT>
struct RadixLds {
  uint64_t lo[QT], hi[QT];                               // the keys that count / are emitted; lo > hi: none (a row behind nq, a resolved query)
  uint32_t flt[QT][2];
  int qnorm[QT];
  uint32_t hist[QT][RADIX_BINS];
};
#define RADIX_IMG(QT) ((sizeof(RadixLds<QT>) + 15u) & ~(size_t)15u)       // offset of the query image in the workgroup's LDS

// -> whether the tile has a query this pass works for (uniform over the workgroup; a barrier inside)
template <int QT, bool EMIT>
__device__ __forceinline__ bool radix_lds_init(RadixLds<QT>& s, const RadixArgs& a, uint32_t q0) {
  const uint32_t t = threadIdx.x;
  bool act = false;
  if (t < (uint32_t)QT) {
    const uint32_t q = q0 + t;
    const bool in = q < a.nq, f = a.filters != nullptr && in;
    uint64_t lo = ~0ull, hi = 0ull;
    if (in) {
      const uint64_t pre = ((const uint64_t GAS*)a.prefix)[q];
      const bool resolved = (((const uint32_t GAS*)a.flags)[q] & RADIX_RESOLVED) != 0u;
      if (EMIT ? resolved : !resolved) {
        act = true;
        if (EMIT) { lo = 0ull; hi = pre; }                                 // everything up to the bound U
        else { lo = pre; hi = a.shift + 8u >= 64u ? ~0ull : (pre | ((1ull << (a.shift + 8u)) - 1ull)); }     // the keys under the prefix
      }
    }
    s.lo[t] = lo; s.hi[t] = hi;
    s.flt[t][0] = f ? ((const uint32_t GAS*)a.filters)[2ull * q] : 0u;
    s.flt[t][1] = f ? ((const uint32_t GAS*)a.filters)[2ull * q + 1u] : 0u;
    s.qnorm[t] = 0;
  }
  if (!EMIT)
    for (uint32_t i = t; i < (uint32_t)QT * RADIX_BINS; i += 256u) (&s.hist[0][0])[i] = 0u;
  return __syncthreads_or(act ? 1 : 0) != 0;
}

// the end of a histogram pass: the workgroup's non-zero bins to HBM
template <int QT>
__device__ __forceinline__ void radix_flush(RadixLds<QT>& s, const RadixArgs& a, uint32_t q0) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (uint32_t)QT * RADIX_BINS; i += 256u) {
    const uint32_t c = (&s.hist[0][0])[i], q = q0 + i / RADIX_BINS;
    if (c != 0u && q < a.nq)
      (void)__hip_atomic_fetch_add((uint32_t GAS*)a.bins + (uint64_t)q * RADIX_BINS + i % RADIX_BINS, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The lanes with `c` hold a key of query q that counts (histogram: into hrow) or belongs to the answer (emit).  HALVES: the two half-waves hold two
// different queries, q and hrow are theirs.  One ballot, one LDS add / one global counter add per query for the lanes that agree with the first
template <bool EMIT, bool HALVES>
__device__ __forceinline__ void radix_take(const RadixArgs& a, uint32_t* hrow, uint32_t q, bool c, uint64_t key, int lane) {
  const uint64_t cb = __ballot(c);
  if (cb == 0ull) return;                                                  // (uniform)
  const uint32_t half = HALVES ? ((uint32_t)lane & 32u) : 0u, sub = HALVES ? ((uint32_t)lane & 31u) : (uint32_t)lane;
  const uint64_t mine = HALVES ? (half ? cb >> 32 : cb & 0xFFFFFFFFull) : cb;       // the lanes of my query, bit = point: id order
  const uint32_t lead = mine != 0ull ? (uint32_t)__builtin_ctzll(mine) : 0u;
  if (EMIT) {
    uint32_t base = 0u;
    if (mine != 0ull && sub == lead)
      base = __hip_atomic_fetch_add((uint32_t GAS*)a.emitted + q, (uint32_t)__popcll(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (uint32_t)__shfl((int)base, (int)(half + lead));
    const uint32_t pos = base + (uint32_t)__popcll(mine & ((1ull << sub) - 1ull));
    if (c && pos < a.k) {                                                  // (U admits exactly min(k, matched) keys: the guard never drops one)
      const uint64_t at = (uint64_t)q * a.k + pos;
      ((uint32_t GAS*)a.row_ids)[at] = (uint32_t)key;
      ((uint32_t GAS*)a.row_dists)[at] = (uint32_t)(key >> 32);
    }
  } else {
    const uint32_t digit = (uint32_t)(key >> a.shift) & (RADIX_BINS - 1u);
    const uint32_t dl = (uint32_t)__shfl((int)digit, (int)(half + lead));
    const bool same = c && digit == dl;
    const uint64_t sb = __ballot(same);
    const uint64_t sm = HALVES ? (half ? sb >> 32 : sb & 0xFFFFFFFFull) : sb;
    if (same) {
      if (sub == lead) (void)__hip_atomic_fetch_add(hrow + dl, (uint32_t)__popcll(sm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (c) {
      (void)__hip_atomic_fetch_add(hrow + digit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

__device__ __forceinline__ int radix8_norm(i32x4 f, int norm) {
  norm = __builtin_amdgcn_sdot4(f.x, f.x, norm, false);
  norm = __builtin_amdgcn_sdot4(f.y, f.y, norm, false);
  norm = __builtin_amdgcn_sdot4(f.z, f.z, norm, false);
  return __builtin_amdgcn_sdot4(f.w, f.w, norm, false);
}

// the canonical chain of one (query row, point) pair: ascending, (float)(v - q), fmaf.  D % 4 == 0; the image holds the shifted query, real 0 in
// [qdim, D)
template <bool IS_U8>
__device__ __forceinline__ float radix8_chain(const uint32_t* img, uint32_t qrow, const uint8_t GAS* v, uint32_t D) {
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
__global__ __launch_bounds__(256) void scan_radix8_kernel(const RadixArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t radix_smem[];
  RadixLds<RADIX8_QT>& s = *(RadixLds<RADIX8_QT>*)radix_smem;
  i32x4* qimg = (i32x4*)(radix_smem + RADIX_IMG(RADIX8_QT));               // [KS][64]: piece 64 s + lane
  if (!EMIT && ((const uint32_t GAS*)a.unresolved)[0] == 0u) return;       // (uniform over the grid) every query has its bound
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t r = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
  const uint32_t q0 = blockIdx.x * RADIX8_QT, run = blockIdx.y * RADIX_WAVES + wave;
  const uint32_t D = a.D, qdim = a.qdim;
  const uint32_t KSF = D >> 5, KS = (D + 31u) >> 5;                        // (uniform) whole k-steps, all k-steps
  if (!radix_lds_init<RADIX8_QT, EMIT>(s, a, q0)) return;                  // (uniform over the workgroup)
  // the tile's queries, once per workgroup: shifted, real 0 in [qdim, D) (the MIPS coordinate), int8 0 behind D; a row behind nq repeats the last
  // query (its [lo, hi] is empty)
  for (uint32_t idx = threadIdx.x; idx < KS * 64u; idx += 256u) {
    const uint32_t rr = idx & 31u, b = 32u * (idx >> 6) + 16u * ((idx >> 5) & 1u);
    const uint32_t q = q0 + rr < a.nq ? q0 + rr : a.nq - 1u;
    const uint8_t GAS* src = (const uint8_t GAS*)a.queries + (uint64_t)q * qdim;     // (rows of D - 1 bytes are not dword-aligned: byte loads)
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t j = b + 4u * (uint32_t)i + (uint32_t)e;
        uint32_t x = j < qdim ? (uint32_t)src[j] : 0u;
        if (IS_U8) x ^= 0x80u;
        if (j < D) w[i] |= x << (8 * e);
      }
    }
    const i32x4 f = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    qimg[idx] = f;
    const int part = radix8_norm(f, 0);
    if (part != 0) (void)__hip_atomic_fetch_add(&s.qnorm[rr], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const bool mine_run = run < a.runs;                                      // (uniform per wave: the last workgroup of a column may hold idle waves)
  const uint64_t p_begin = (uint64_t)run * a.per;
  uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  if (!mine_run) p_stop = 0ull;
  // the short k-step: dwords of this lane's piece inside the row
  const uint32_t tail_at = 32u * KSF + 16u * h;
  const uint32_t tail_dw = D > tail_at ? ((D - tail_at) >> 2 < 4u ? (D - tail_at) >> 2 : 4u) : 0u;
  for (uint64_t base = p_begin; base < p_stop; base += 32u) {              // (uniform over the wave) one 32-point tile per trip, ascending
    const uint64_t pt64 = base + r;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;        // (p_begin < n_nodes here)
    const uint8_t GAS* row = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;
    const uint8_t GAS* mine = row + 16u * h;
    u32x4a cur[RADIX8_U], nxt[RADIX8_U];
#pragma unroll
    for (int u = 0; u < RADIX8_U; ++u) {
      cur[u] = (u32x4a){0u, 0u, 0u, 0u};
      if ((uint32_t)u < KSF) cur[u] = *(const u32x4a GAS*)(mine + 32u * (uint32_t)u);          // (uniform)
    }
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int pn = 0;
    for (uint32_t s0 = 0; s0 < KSF; s0 += RADIX8_U) {                      // (uniform)
#pragma unroll
      for (int u = 0; u < RADIX8_U; ++u) {
        nxt[u] = (u32x4a){0u, 0u, 0u, 0u};
        const uint32_t ks = s0 + RADIX8_U + (uint32_t)u;
        if (ks < KSF) nxt[u] = *(const u32x4a GAS*)(mine + 32u * ks);      // (uniform)
      }
#pragma unroll
      for (int u = 0; u < RADIX8_U; ++u) {
        const uint32_t ks = s0 + (uint32_t)u;
        if (ks < KSF) {                                                    // (uniform)
          u32x4a w = cur[u];
          if (IS_U8) { w.x ^= 0x80808080u; w.y ^= 0x80808080u; w.z ^= 0x80808080u; w.w ^= 0x80808080u; }
          const i32x4 bf = {(int)w.x, (int)w.y, (int)w.z, (int)w.w};
          pn = radix8_norm(bf, pn);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * ks + (uint32_t)lane], bf, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < RADIX8_U; ++u) cur[u] = nxt[u];
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
      pn = radix8_norm(bf, pn);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * KSF + (uint32_t)lane], bf, acc, 0, 0, 0);
    }
    pn += __shfl_xor(pn, 32);                                              // both halves of the column
    // register i of lane (r, h): query row (i & 3) + 8 (i >> 2) + 4 h, point column r -- a ballot of register i holds one query per half-wave
    uint32_t slow = 0u;                                                    // bit i: a sum beyond 2^24 whose query's [lo, hi] reaches such keys
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qrow = (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
      const int d = s.qnorm[qrow] + pn - 2 * acc[i];
      bool m = valid;
      if (filtered) m = m && scan_match(lab, s.flt[qrow][0], s.flt[qrow][1]);
      const uint64_t lo = s.lo[qrow], hi = s.hi[qrow];
      const uint64_t key = ((uint64_t)__float_as_uint((float)d) << 32) | pt;
      const bool big = d > (1 << 24);
      if (m && big && hi >= RADIX_KEY_2P24) slow |= 1u << i;
      radix_take<EMIT, true>(a, s.hist[qrow], q0 + qrow, m && !big && key >= lo && key <= hi, key, lane);
      __builtin_amdgcn_sched_barrier(0);                                   // (one row's ballots at a time: sixteen live ballots cost scalar registers)
    }
    if (__ballot(slow != 0u) != 0ull) {                                    // (uniform) only where sums pass 2^24 and the bounds reach them
#pragma unroll 1
      for (uint32_t i = 0; i < 16u; ++i) {
        const bool again = ((slow >> i) & 1u) != 0u;
        if (__ballot(again) == 0ull) continue;                             // (uniform)
        const uint32_t qrow = (i & 3u) + 8u * (i >> 2) + 4u * h;
        float c = 0.0f;
        if (again) c = radix8_chain<IS_U8>((const uint32_t*)qimg, qrow, row, D);
        const uint64_t key = ((uint64_t)__float_as_uint(c) << 32) | pt;
        radix_take<EMIT, true>(a, s.hist[qrow], q0 + qrow, again && key >= s.lo[qrow] && key <= s.hi[qrow], key, lane);
      }
    }
  }
  if (!EMIT) radix_flush(s, a, q0);
}

// ---------------------------------------------------------------------------------------------------------------------
// float vectors
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void radixf_step(float (&acc)[RADIXF_QT], float x, const float* qd) {
#pragma unroll
  for (int j = 0; j < RADIXF_QT; ++j) {
    const float diff = x - qd[j];                                          // vector - query, as orc_exact_dist
    acc[j] = __builtin_fmaf(diff, diff, acc[j]);                           // ascending dimension
  }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void scan_radix_f32_kernel(const RadixArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t radix_smem[];
  RadixLds<RADIXF_QT>& s = *(RadixLds<RADIXF_QT>*)radix_smem;
  float* qv = (float*)(radix_smem + RADIX_IMG(RADIXF_QT));                 // [D][16]: element d of the tile's queries, +0.0f in [qdim, D)
  if (!EMIT && ((const uint32_t GAS*)a.unresolved)[0] == 0u) return;       // (uniform over the grid)
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t q0 = blockIdx.x * RADIXF_QT, run = blockIdx.y * RADIX_WAVES + wave;
  const uint32_t D = a.D, D4 = a.D & ~3u, qdim = a.qdim;
  if (!radix_lds_init<RADIXF_QT, EMIT>(s, a, q0)) return;                  // (uniform over the workgroup)
  for (uint32_t i = threadIdx.x; i < D * RADIXF_QT; i += 256u) {
    const uint32_t d = i / RADIXF_QT, j = i % RADIXF_QT;
    const uint32_t q = q0 + j < a.nq ? q0 + j : a.nq - 1u;
    qv[i] = d < qdim ? ((const float GAS*)a.queries)[(uint64_t)q * qdim + d] : 0.0f;
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const bool mine_run = run < a.runs;                                      // (uniform per wave)
  const uint64_t p_begin = (uint64_t)run * a.per;
  uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  if (!mine_run) p_stop = 0ull;
  for (uint64_t base = p_begin; base < p_stop; base += WAVE) {             // (uniform over the wave) 64 points per trip, ascending
    const uint64_t pt64 = base + (uint32_t)lane;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;
    const uint8_t GAS* v = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;     // (dword-aligned only: u32x4a is typed so)
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    float acc[RADIXF_QT];
#pragma unroll
    for (int j = 0; j < RADIXF_QT; ++j) acc[j] = 0.0f;
    for (uint32_t d = 0; d < D4; d += 4u) {                                // (uniform) the whole 16-byte pieces
      const u32x4a w = *(const u32x4a GAS*)(v + 4u * d);
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) radixf_step(acc, __uint_as_float(ww[e]), qv + (d + (uint32_t)e) * RADIXF_QT);
    }
    for (uint32_t d = D4; d < D; ++d)                                      // (uniform) the last D % 4 elements, one dword each
      radixf_step(acc, __uint_as_float(*(const uint32_t GAS*)(v + 4u * d)), qv + d * RADIXF_QT);
#pragma unroll
    for (int j = 0; j < RADIXF_QT; ++j) {
      bool m = valid;
      if (filtered) m = m && scan_match(lab, s.flt[j][0], s.flt[j][1]);
      const uint64_t key = ((uint64_t)__float_as_uint(acc[j]) << 32) | pt;
      radix_take<EMIT, false>(a, s.hist[j], q0 + (uint32_t)j, m && key >= s.lo[j] && key <= s.hi[j], key, lane);
      __builtin_amdgcn_sched_barrier(0);                                   // (one query's ballots at a time)
    }
  }
  if (!EMIT) radix_flush(s, a, q0);
}

// ---------------------------------------------------------------------------------------------------------------------
// init: the state of every query (prefix 0, nothing fixed, rank k, unresolved), bins and counters cleared
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_radix_init_kernel(const RadixArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t < (uint64_t)a.nq * RADIX_BINS) ((uint32_t GAS*)a.bins)[t] = 0u;
  if (t < (uint64_t)a.nq) {
    ((uint64_t GAS*)a.prefix)[t] = 0ull;
    ((uint32_t GAS*)a.rank)[t] = a.k;
    ((uint32_t GAS*)a.fixed)[t] = 0u;
    ((uint32_t GAS*)a.flags)[t] = 0u;
    ((uint32_t GAS*)a.emitted)[t] = 0u;
    ((uint32_t GAS*)a.count)[t] = 0u;
  }
  if (t == 0ull) ((uint32_t GAS*)a.unresolved)[0] = a.nq;
}

// ---------------------------------------------------------------------------------------------------------------------
// pick: one wave per query, the digit in which the cumulative count crosses the rank
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_radix_pick_kernel(const RadixArgs a) {
  const int lane = lane_id();
  const uint32_t q = blockIdx.x * RADIX_WAVES + uni(threadIdx.x >> 6);
  if (q >= a.nq) return;                                                   // (uniform per wave; the kernel has no workgroup barrier)
  if ((uni(((const uint32_t GAS*)a.flags)[q]) & RADIX_RESOLVED) != 0u) return;     // (its bins were not counted into: they are zero)
  u32x4a GAS* mine = (u32x4a GAS*)((uint32_t GAS*)a.bins + (uint64_t)q * RADIX_BINS) + lane;      // bins 4 lane .. 4 lane + 3
  const u32x4a b = *mine;
  const uint32_t bb[4] = {b.x, b.y, b.z, b.w};
  const uint32_t sum = b.x + b.y + b.z + b.w;
  uint32_t incl = sum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= off) incl += t;
  }
  const uint32_t total = (uint32_t)__shfl((int)incl, WAVE - 1);
  const bool first = a.shift + 8u >= 64u;                                  // (uniform) the first pass counted every candidate
  uint32_t rk = uni(((const uint32_t GAS*)a.rank)[q]);
  uint64_t pre = ((const uint64_t GAS*)a.prefix)[q];
  bool resolved = false;
  if (first && total < rk) {                                               // fewer than k candidates: all of them
    pre = ~0ull; resolved = true;
  } else {
    const uint32_t excl = incl - sum;
    const bool here = excl < rk && rk <= incl;                             // (one lane: 1 <= rank <= total)
    uint32_t digit = 0u, below = excl, cnt = 0u;
    bool found = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (here && !found) {
        if (rk <= below + bb[e]) { digit = 4u * (uint32_t)lane + (uint32_t)e; cnt = bb[e]; found = true; }
        else below += bb[e];
      }
    }
    const uint64_t hb = __ballot(here);
    if (hb == 0ull) {                                                      // (uniform; cannot happen: the bins under a prefix hold at least rank keys)
      pre |= (1ull << a.shift) - 1ull; resolved = true;
    } else {
      const int src = __builtin_ctzll(hb);
      digit = (uint32_t)__shfl((int)digit, src); below = (uint32_t)__shfl((int)below, src); cnt = (uint32_t)__shfl((int)cnt, src);
      pre |= (uint64_t)digit << a.shift;
      rk -= below;
      if (rk == cnt) { pre |= (1ull << a.shift) - 1ull; resolved = true; }  // the bin is needed whole: an inclusive bound
    }
  }
  *mine = (u32x4a){0u, 0u, 0u, 0u};
  if (lane == 0) {
    if (first) ((uint32_t GAS*)a.matched)[q] = total;
    ((uint64_t GAS*)a.prefix)[q] = pre;
    ((uint32_t GAS*)a.rank)[q] = rk;
    ((uint32_t GAS*)a.fixed)[q] = 64u - a.shift;
    if (resolved) {
      ((uint32_t GAS*)a.flags)[q] = RADIX_RESOLVED;
      (void)__hip_atomic_fetch_add((uint32_t GAS*)a.unresolved, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the outputs: the sorted row of a query (n = count[q] keys) widened, transposed and padded
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_radix_out_kernel(const RadixArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= (uint64_t)a.nq * a.k) return;
  const uint32_t q = (uint32_t)(t / a.k), i = (uint32_t)(t % a.k);
  const bool in = i < ((const uint32_t GAS*)a.count)[q];
  ((uint64_t GAS*)a.ids_out)[t] = in ? (uint64_t)((const uint32_t GAS*)a.row_ids)[t] : ~0ull;                  // CANON 8
  ((float GAS*)a.dists_out)[(uint64_t)i * a.nq + q] = in ? __uint_as_float(((const uint32_t GAS*)a.row_dists)[t]) : BIG_DIST;
}

// ---------------------------------------------------------------------------------------------------------------------
// the entry: checks, then init, the digit passes, emit, sort, outputs in stream order -- nothing is read back
// ---------------------------------------------------------------------------------------------------------------------
// One launch of instance KERNEL.  The histograms beside the query image take more than the 64 KB of dynamic LDS a kernel may ask for unprompted:
// the instance's limit is raised once per device to lds_most, the most a launch of it ever asks for
template <auto KERNEL>
static int radix_launch(const RadixArgs& a, dim3 grid, size_t lds, size_t lds_most, void* stream) {
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
static int radix_pass(const RadixArgs& a, uint32_t dtype, dim3 grid, void* stream) {
  if (dtype == BANG_F32)
    return radix_launch<scan_radix_f32_kernel<EMIT>>(a, grid, RADIX_IMG(RADIXF_QT) + (size_t)a.D * RADIXF_QT * 4,
                                                     RADIX_IMG(RADIXF_QT) + (size_t)BANG_SCAN_ANY_MAX_D * RADIXF_QT * 4, stream);
  const size_t lds = RADIX_IMG(RADIX8_QT) + (size_t)((a.D + 31u) / 32u) * 1024u, most = RADIX_IMG(RADIX8_QT) + (size_t)BANG_SCAN_ANY_MAX_D * 32u;
  if (dtype == BANG_U8) return radix_launch<scan_radix8_kernel<true, EMIT>>(a, grid, lds, most, stream);
  return radix_launch<scan_radix8_kernel<false, EMIT>>(a, grid, lds, most, stream);
}

extern "C" int bang_k_scan_radix(const bang_scan_params* p, uint32_t qdim, void* stream) { return bang_k_scan_radix_marked(p, qdim, stream, nullptr); }

extern "C" int bang_k_scan_radix_marked(const bang_scan_params* p, uint32_t qdim, void* stream, void* ev_merge) {
  {
    const int rc = bang_scan_radix_check(p, qdim);
    if (rc != BANG_OK) return rc;
  }
  uint32_t tiles = 0, runs = 0;
  {
    const int rc = bang_scan_radix_geometry((int)p->dtype, p->D, p->nq, p->n_nodes, p->k, &tiles, &runs, nullptr);
    if (rc != BANG_OK) { bang_set_error("bang_k_scan_radix: no geometry for this launch"); return rc; }
  }
  if (p->stripes != 0u) runs = p->stripes;
  const size_t nq = p->nq;
  RadixArgs a;
  a.vec_base = p->d_vec_base; a.vec_stride = p->vec_stride; a.queries = p->d_queries;
  a.excl = p->d_excluded; a.removed = p->d_removed; a.labels = p->d_labels; a.filters = p->d_filters;
  a.prefix = (uint64_t*)p->d_scratch;                                      // the layout of bang_scan_radix_scratch_bytes
  a.bins = (uint32_t*)(a.prefix + nq);
  a.rank = a.bins + nq * RADIX_BINS; a.fixed = a.rank + nq; a.flags = a.fixed + nq; a.emitted = a.flags + nq; a.count = a.emitted + nq;
  a.row_ids = a.count + nq; a.row_dists = a.row_ids + nq * p->k;
  a.unresolved = a.row_dists + nq * p->k;
  a.matched = p->d_matched; a.ids_out = p->d_ids_out; a.dists_out = p->d_dists_out;
  a.D = p->D; a.qdim = qdim; a.n_nodes = p->n_nodes; a.nq = p->nq; a.k = p->k; a.runs = runs; a.shift = 56u;
  const uint64_t tiles32 = ((uint64_t)p->n_nodes + 31u) / 32u;
  a.per = (tiles32 + runs - 1u) / runs * 32u;                              // (runs behind the last point are empty)
  const dim3 grid(tiles, (runs + RADIX_WAVES - 1u) / RADIX_WAVES);
  const uint32_t per_query = (uint32_t)((nq + RADIX_WAVES - 1u) / RADIX_WAVES);
  hipLaunchKernelGGL(scan_radix_init_kernel, dim3((uint32_t)((nq * RADIX_BINS + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  // four digits of distance bits, then the id digits that n_nodes - 1 reaches (a digit above its width is 0 in every key and in the prefix); the
  // last digit always: it resolves whatever is left
  for (uint32_t shift = 56u;; shift -= 8u) {
    if (shift >= 32u || shift == 0u || ((p->n_nodes - 1u) >> shift) != 0u) {
      a.shift = shift;
      BANG_TRY(radix_pass<false>(a, p->dtype, grid, stream));
      hipLaunchKernelGGL(scan_radix_pick_kernel, dim3(per_query), dim3(256), 0, (hipStream_t)stream, a);
      HIP_TRY(hipGetLastError());
    }
    if (shift == 0u) break;
  }
  if (ev_merge) HIP_TRY(hipEventRecord((hipEvent_t)ev_merge, (hipStream_t)stream));
  BANG_TRY(radix_pass<true>(a, p->dtype, grid, stream));
  BANG_TRY(bang_k_range_sort(a.row_ids, (float*)a.row_dists, a.emitted, p->k, 0, p->nq, p->nq, a.count, stream));
  hipLaunchKernelGGL(scan_radix_out_kernel, dim3((uint32_t)((nq * p->k + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
