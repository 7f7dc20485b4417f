// bang_scan_mfma.hip -- the exact scan of float vectors on the fp32 MFMA (option scan_mfma): a matrix product with a proven
// error bound discards the pairs that cannot enter the answer, the canonical ascending fmaf chain runs for the rest.  Same answer, bit for bit, as
// scan_f32_kernel / scan_f32_any_kernel; 1 <= D <= 1024, queries of D or D - 1 elements (MIPS: the last coordinate is +0.0f).
// Grid, lists and selection are bang_scan.hip's (bang_scan_select.h, the 8-bit tile: 32 queries, lists of 256 keys, rounds of 128 points).
//
//  * Products.  d~ = |q|^2 + |p|^2 - 2 q.p with v_mfma_f32_32x32x2_f32: queries on the rows (A), points on the columns (B), scan8_kernel's map from
//    accumulator register to (query row, point column).  A k-GROUP is 8 elements: lane (r, h) holds elements [8 s + 4 h, 8 s + 4 h + 4) of row /
//    column r from one 16-byte load and feeds them to four MFMAs, element e of both operands to MFMA e (k = h there).  The row norms are fmaf on the
//    floats already loaded and one cross-half shuffle.
//  * Data.  The tile's queries stand in LDS as scan8_any_kernel's piece-major image -- piece 64 s + lane for k-group s: one ds_read_b128 of 1 KB per
//    wave and group, no bank conflict -- built in SLABS of 64 k-groups (512 elements, 64 KB).  D <= 512: staged once per stripe.  Wider: every
//    round walks the slabs, two barriers each.  The points stream from global memory, four 16-byte loads in flight per lane and the next four
//    requested in front of the MFMAs of these; the last k-group is loaded short, dwords of [row, row + D) only, zeros behind.
//  * Bound.  With E(q, p) = (D + 4) 2^-21 (|q|^2~ + |p|^2~) + (D + 4) 2^-120, |d~ - chain| <= E whatever order the matrix unit adds in, whether
//    it rounds or truncates, and whether it flushes subnormals (DESIGN.md 4.17 has the derivation).  A pair whose d~ - E is above the distance of
//    the query's threshold key cannot be offered and is dropped; before the list holds k keys every pair is a candidate.
//  * Refine.  A wave compacts the candidates of its 32 x 32 tile (ballot, mbcnt) into its own list of 1024 16-bit (row, column) entries in LDS --
//    no overflow, no barrier --, then one lane per pair runs orc_exact_dist's chain over both rows from global memory.  Only these keys are offered.
//  * Counters: pairs tested and pairs refined, summed per wave, per workgroup in LDS, one global atomic add per sum and workgroup.
//  * Typed global pointers (GAS), 64-bit row offsets, vector stores only, no private segment.
#include "bang_scan_select.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SCANM_IMG ((sizeof(Scan8Lds) + 15u) & ~(size_t)15u)                // offset of the query image in the workgroup's LDS
#define SCANM_SLAB_G 64u                                                    // k-groups of a slab: 64 KB of image beside 65 KB of lists and 9 KB static
#define SCANM_U 4                                                           // k-groups of point floats in flight per lane

// k-groups [g0, g0 + ng) of the tile's queries into the image: +0.0f in [qdim, ...) -- the MIPS coordinate and the padding of the last group
__device__ __forceinline__ void scanm_stage(f32x4* qimg, const ScanArgs& a, uint32_t q0, uint32_t qdim, uint32_t g0, uint32_t ng) {
  for (uint32_t idx = threadIdx.x; idx < ng * 64u; idx += 256u) {
    const uint32_t rr = idx & 31u, b = 8u * (g0 + (idx >> 6)) + 4u * ((idx >> 5) & 1u);
    const uint32_t q = q0 + rr < a.nq ? q0 + rr : a.nq - 1u;                // a row behind nq repeats the last query and is never a candidate
    const float GAS* src = (const float GAS*)a.queries + (uint64_t)q * qdim;
    f32x4 f;
    f.x = b < qdim ? src[b] : 0.0f;
    f.y = b + 1u < qdim ? src[b + 1u] : 0.0f;
    f.z = b + 2u < qdim ? src[b + 2u] : 0.0f;
    f.w = b + 3u < qdim ? src[b + 3u] : 0.0f;
    qimg[idx] = f;
  }
}

// one k-group: four MFMAs, the point's share of its norm
__device__ __forceinline__ void scanm_group(f32x16& acc, float& pn, const f32x4 qp, const u32x4a w) {
  const float x = __uint_as_float(w.x), y = __uint_as_float(w.y), z = __uint_as_float(w.z), t = __uint_as_float(w.w);
  pn = __builtin_fmaf(x, x, pn);
  pn = __builtin_fmaf(y, y, pn);
  pn = __builtin_fmaf(z, z, pn);
  pn = __builtin_fmaf(t, t, pn);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp.x, x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp.y, y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp.z, z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qp.w, t, acc, 0, 0, 0);
}

// the whole k-groups [g0, g1) of this lane's point against the slab that starts at group g0.  mine: the row + 16 h bytes
__device__ __forceinline__ void scanm_groups(f32x16& acc, float& pn, const uint8_t GAS* mine, const f32x4* qimg, uint32_t g0, uint32_t g1, int lane) {
  u32x4a cur[SCANM_U], nxt[SCANM_U];
#pragma unroll
  for (int u = 0; u < SCANM_U; ++u) {
    cur[u] = (u32x4a){0u, 0u, 0u, 0u};
    if (g0 + (uint32_t)u < g1) cur[u] = *(const u32x4a GAS*)(mine + 32u * (g0 + (uint32_t)u));       // (uniform)
  }
  for (uint32_t s0 = g0; s0 < g1; s0 += SCANM_U) {                           // (uniform)
#pragma unroll
    for (int u = 0; u < SCANM_U; ++u) {
      nxt[u] = (u32x4a){0u, 0u, 0u, 0u};
      const uint32_t gs = s0 + SCANM_U + (uint32_t)u;
      if (gs < g1) nxt[u] = *(const u32x4a GAS*)(mine + 32u * gs);           // (uniform)
    }
#pragma unroll
    for (int u = 0; u < SCANM_U; ++u) {
      const uint32_t gs = s0 + (uint32_t)u;
      if (gs < g1) scanm_group(acc, pn, qimg[64u * (gs - g0) + (uint32_t)lane], cur[u]);      // (uniform)
    }
#pragma unroll
    for (int u = 0; u < SCANM_U; ++u) cur[u] = nxt[u];
  }
}

// orc_exact_dist's chain of one pair: ascending, (vector - query), fmaf; rows read as 16-byte pieces and then dwords, never beyond D (qdim) elements
__device__ __forceinline__ float scanm_chain(const uint8_t GAS* v, const uint8_t GAS* q, uint32_t D, uint32_t qdim) {
  float acc = 0.0f;
  const uint32_t D4 = D & ~3u;
  for (uint32_t d = 0; d < D4; d += 4u) {                                    // (uniform)
    const u32x4a pw = *(const u32x4a GAS*)(v + 4u * d);
    u32x4a qw = {0u, 0u, 0u, 0u};                                            // (the bits of +0.0f: the MIPS coordinate)
    if (d + 4u <= qdim) {                                                    // (uniform)
      qw = *(const u32x4a GAS*)(q + 4u * d);
    } else {
      if (d < qdim) qw.x = *(const uint32_t GAS*)(q + 4u * d);
      if (d + 1u < qdim) qw.y = *(const uint32_t GAS*)(q + 4u * d + 4u);
      if (d + 2u < qdim) qw.z = *(const uint32_t GAS*)(q + 4u * d + 8u);
    }
    const uint32_t pp[4] = {pw.x, pw.y, pw.z, pw.w}, qq[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float diff = __uint_as_float(pp[e]) - __uint_as_float(qq[e]);
      acc = __builtin_fmaf(diff, diff, acc);
    }
  }
  for (uint32_t d = D4; d < D; ++d) {                                        // (uniform) the last D % 4 elements, one dword each
    const float x = __uint_as_float(*(const uint32_t GAS*)(v + 4u * d));
    const float y = d < qdim ? __uint_as_float(*(const uint32_t GAS*)(q + 4u * d)) : 0.0f;
    const float diff = x - y;
    acc = __builtin_fmaf(diff, diff, acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void scan_f32_mfma_kernel(const ScanArgs a, const uint32_t qdim, uint64_t* counters) {
  extern __shared__ __attribute__((aligned(16))) uint8_t scan_smem[];
  Scan8Lds& s = *(Scan8Lds*)scan_smem;
  f32x4* qimg = (f32x4*)(scan_smem + SCANM_IMG);                            // [groups of the slab][64]: piece 64 s + lane
  __shared__ float qnorm[SCAN8_QT];
  __shared__ float qpart[8][SCAN8_QT];
  __shared__ uint16_t pairs[4][1024];                                       // per wave: (query row << 5) | point column of its tile's candidates
  __shared__ unsigned long long wg_sums[2];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t r = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
  const uint32_t q0 = blockIdx.x * SCAN8_QT, stripe = blockIdx.y;
  const uint32_t D = a.D;
  const uint32_t KGF = D >> 3, KG = (D + 7u) >> 3;                          // (uniform) whole k-groups, all k-groups
  const bool one_slab = KG <= SCANM_SLAB_G;                                 // (uniform)
  const uint32_t nrows = a.nq - q0 < (uint32_t)SCAN8_QT ? a.nq - q0 : (uint32_t)SCAN8_QT;     // the tile's real queries
  scan_lds_init(s, a, q0);
  if (threadIdx.x == 0u) { wg_sums[0] = 0ull; wg_sums[1] = 0ull; }
  {
    // |q|^2~ of the tile's queries: eight strided partial chains per row, summed in a fixed order (the bound holds for any order)
    const uint32_t rr = threadIdx.x & 31u, part = threadIdx.x >> 5;
    const uint32_t q = q0 + rr < a.nq ? q0 + rr : a.nq - 1u;
    const float GAS* src = (const float GAS*)a.queries + (uint64_t)q * qdim;
    float n = 0.0f;
    for (uint32_t j = part; j < qdim; j += 8u) { const float x = src[j]; n = __builtin_fmaf(x, x, n); }
    qpart[part][rr] = n;
  }
  if (one_slab) scanm_stage(qimg, a, q0, qdim, 0u, KG);
  __syncthreads();
  if (threadIdx.x < (uint32_t)SCAN8_QT) {
    float n = qpart[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < 8; ++i) n += qpart[i][threadIdx.x];
    qnorm[threadIdx.x] = n;
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const uint64_t p_begin = (uint64_t)stripe * a.per;
  const uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  // the short k-group: dwords of this lane's piece inside the row
  const uint32_t tail_at = 8u * KGF + 4u * h;
  const uint32_t tail_dw = D > tail_at ? (D - tail_at < 4u ? D - tail_at : 4u) : 0u;
  // E = c_rel (|q|^2~ + |p|^2~) + c_abs.  Input values up to 2^56 (CANON 20) keep every norm finite at D = 1024: 1024 x 2^112 = 2^122, their sum
  // 2^123, d~ and the chain below 2^125, E below 2^114
  const float c_rel = (float)(D + 4u) * 0x1p-21f, c_abs = (float)(D + 4u) * 0x1p-120f;
  uint16_t* mypairs = pairs[wave];
  uint32_t unfiltered = 0u;                                                // (uniform) valid points of this wave's tiles
  uint64_t tested = 0ull, refined = 0ull;                                  // (uniform) this wave's pairs
  for (uint64_t base = p_begin; base < p_stop; base += SCAN8_ROUND) {      // (uniform over the workgroup)
    const uint64_t tile0 = base + wave * 32u;
    const uint64_t pt64 = tile0 + r;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;        // (p_begin < n_nodes here)
    const uint8_t GAS* row = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;
    const uint8_t GAS* mine = row + 16u * h;
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    f32x16 acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float pn = 0.0f;
    for (uint32_t g0 = 0; g0 < KG; g0 += SCANM_SLAB_G) {                   // (uniform) the slabs of the D axis
      const uint32_t g1 = g0 + SCANM_SLAB_G < KG ? g0 + SCANM_SLAB_G : KG;
      if (!one_slab) {
        __syncthreads();                                                   // every wave is done with the slab before
        scanm_stage(qimg, a, q0, qdim, g0, g1 - g0);
        __syncthreads();
      }
      scanm_groups(acc, pn, mine, qimg, g0, g1 < KGF ? g1 : KGF, lane);
      if (g1 == KG && KG != KGF) {                                         // (uniform) the short k-group: only the dwords that exist
        u32x4a w = {0u, 0u, 0u, 0u};
        const uint8_t GAS* t = row + 4u * tail_at;
        if (tail_dw == 4u) {
          w = *(const u32x4a GAS*)t;
        } else {
          if (tail_dw > 0u) w.x = *(const uint32_t GAS*)t;
          if (tail_dw > 1u) w.y = *(const uint32_t GAS*)(t + 4);
          if (tail_dw > 2u) w.z = *(const uint32_t GAS*)(t + 8);
        }
        scanm_group(acc, pn, qimg[64u * (KGF - g0) + (uint32_t)lane], w);
      }
    }
    pn += __shfl_xor(pn, 32);                                              // both halves of the column
    if (!filtered) unfiltered += (uint32_t)__popc((uint32_t)__ballot(valid));     // (the low half: each point once)
    // register i of lane (r, h): query row (i & 3) + 8 (i >> 2) + 4 h, point column r
    uint32_t ncand = 0u;                                                   // (uniform) entries of this wave's pair list
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qrow = (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[qrow][0], s.flt[qrow][1]);
        const uint64_t mb = __ballot(m);
        const uint32_t hm = h ? (uint32_t)(mb >> 32) : (uint32_t)mb;
        if (r == 0u && hm != 0u) (void)__hip_atomic_fetch_add(&s.mcnt[qrow], (uint32_t)__popc(hm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      m = m && qrow < nrows;
      const uint64_t thr = s.thr[qrow];
      const float sum = qnorm[qrow] + pn;
      const float dt = sum - 2.0f * acc[i];
      const float low = dt - __builtin_fmaf(c_rel, sum, c_abs);           // no chain value of this pair is below it
      // fewer than k keys (the padding key): every pair; else the pairs that may still be at or below the threshold's distance
      const bool cand = m && (thr == SCAN_PAD_KEY || !(low > __uint_as_float((uint32_t)(thr >> 32))));
      tested += (uint64_t)__popcll(__ballot(m));
      const uint64_t cb = __ballot(cand);
      if (cb != 0ull) {                                                    // (uniform)
        if (cand) mypairs[ncand + lanes_below(cb)] = (uint16_t)((qrow << 5) | r);
        ncand += (uint32_t)__popcll(cb);
      }
    }
    refined += ncand;
    wave_sync();
    for (uint32_t b0 = 0; b0 < ncand; b0 += WAVE) {                        // (uniform) 64 pairs at a time, one lane each
      const bool have = b0 + (uint32_t)lane < ncand;
      const uint32_t ent = have ? (uint32_t)mypairs[b0 + (uint32_t)lane] : 0u;
      const uint32_t qrow = ent >> 5;
      const uint32_t cpt = (uint32_t)(tile0 + (ent & 31u));                // (a candidate's point is below p_stop)
      float c = 0.0f;
      if (have) {
        c = scanm_chain((const uint8_t GAS*)a.vec_base + (uint64_t)cpt * a.vec_stride,
                        (const uint8_t GAS*)a.queries + (uint64_t)(q0 + qrow) * qdim * 4u, D, qdim);
      }
      const uint64_t key = ((uint64_t)__float_as_uint(c) << 32) | cpt;
      uint64_t todo = __ballot(have);
      while (todo != 0ull) {                                               // (uniform) one offer per query row among these pairs
        const uint32_t first = (uint32_t)__builtin_ctzll(todo);
        const uint32_t row_u = uni((uint32_t)__builtin_amdgcn_readlane((int)qrow, (int)first));
        const bool here = have && qrow == row_u;
        scan_offer<SCAN8_CAP, false>(s.keys[row_u], &s.cnt[row_u], here && key < s.thr[row_u], key, lane);
        todo &= ~__ballot(here);
      }
    }
    __syncthreads();
    scan_cut_full<SCAN8_QT, SCAN8_CAP, SCAN8_ROUND>(s, wave, a.k, lane);
    __syncthreads();
  }
  if (!filtered && lane == 0 && unfiltered != 0u) (void)__hip_atomic_fetch_add(&s.mall, unfiltered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (lane == 0) {
    (void)__hip_atomic_fetch_add(&wg_sums[0], (unsigned long long)tested, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(&wg_sums[1], (unsigned long long)refined, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (counters != nullptr && threadIdx.x < 2u && wg_sums[threadIdx.x] != 0ull)
    (void)__hip_atomic_fetch_add((unsigned long long GAS*)counters + threadIdx.x, wg_sums[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  scan_finish(s, a, q0, stripe, wave, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// the entry: checks, the counters cleared, one launch, then bang_scan.hip's merge and outputs
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int bang_k_scan_f32_mfma(const bang_scan_params* p, uint32_t qdim, uint64_t* d_counters, void* stream) {
  return bang_k_scan_f32_mfma_marked(p, qdim, d_counters, stream, nullptr);
}

extern "C" int bang_k_scan_f32_mfma_marked(const bang_scan_params* p, uint32_t qdim, uint64_t* d_counters, void* stream, void* ev_merge) {
  {
    const int rc = bang_scan_f32_mfma_check(p, qdim);
    if (rc != BANG_OK) return rc;
  }
  if (((uintptr_t)d_counters) & 7u) { bang_set_error("bang_k_scan_f32_mfma: d_counters is not 8-byte aligned"); return BANG_ERR_ARG; }
  uint32_t tiles = 0, stripes = 0;
  {
    const int rc = bang_scan_f32_mfma_geometry(p->D, p->nq, p->n_nodes, p->k, &tiles, &stripes);
    if (rc != BANG_OK) { bang_set_error("bang_k_scan_f32_mfma: no geometry for this launch"); return rc; }
  }
  if (p->stripes != 0u) stripes = p->stripes;
  ScanArgs a;
  uint32_t* d_count = nullptr;
  BANG_TRY(scan_prepare(p, stripes, SCAN8_ROUND, &a, &d_count, stream));
  if (d_counters) HIP_TRY(hipMemsetAsync(d_counters, 0, 2 * sizeof(uint64_t), (hipStream_t)stream));
  const uint32_t groups = (p->D + 7u) / 8u;
  const size_t lds = SCANM_IMG + (size_t)(groups < SCANM_SLAB_G ? groups : SCANM_SLAB_G) * 1024u, most = SCANM_IMG + (size_t)SCANM_SLAB_G * 1024u;
  BANG_TRY(scan_launch<scan_f32_mfma_kernel>(a, tiles, lds, most, stream, qdim, d_counters));
  return scan_merge_out(a, p, d_count, stream, ev_merge);
}
