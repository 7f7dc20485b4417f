// bang_scan_any.hip -- the exact scan of the layouts bang_scan.hip has no instance for (option scan_any; DESIGN.md section 2 CANON 25, section 4.17):
// float vectors of any D <= 1024, 8-bit vectors of whole dwords (D % 4 == 0, D <= 1024), queries of D - 1 elements (MIPS: the last coordinate is 0).
// Grid, rounds, lists and selection are bang_scan.hip's (bang_scan_select.h); D is a runtime value in both kernels.
//
//  * scan8_any_kernel: KS = ceil(D / 32) k-steps of v_mfma_i32_32x32x32_i8 with scan8_kernel's operand mapping.  The 32 queries of the tile are
//    staged ONCE per workgroup into an LDS image, shifted (^ 0x80 for uint8) and zero-padded to 32 KS bytes, PIECE-MAJOR: the 16-byte piece that lane
//    (r, h) feeds to k-step s stands at 16 (64 s + 32 h + r) = 16 (64 s + lane).  The 64 lanes of a wave read 1 KB of consecutive bytes per k-step: one
//    ds_read_b128 without a bank conflict under any bank model, where the row-major image (stride 32 KS between lanes) would hit the same banks 64
//    times.  The points stream from global memory, four k-steps of 16-byte loads in flight and the next four requested before the MFMAs of these.
//    The last k-step is loaded SHORT -- only the dwords of [row, row + D), zeros behind -- so that the last row of a packed table is never overrun.
//  * The 2^24 hand-over.  S = |q'|^2 + |p'|^2 - 2 q'.p' is the exact integer sum (< 2^31).  The partial sums of the canonical fmaf chain do not
//    decrease, so while S <= 2^24 none of them rounds and (float)S IS the chain's value.  For S > 2^24 the chain rounded somewhere and its value is
//    some float >= 2^24 (float addition of non-negative terms is monotone): such a lane is dropped when its row's threshold is below 2^24's bits, and
//    otherwise re-evaluates the chain element by element (query bytes from the LDS image, un-shifted; point dwords from global memory) before its key
//    is formed.  One ballot per tile decides whether that block runs at all.
//  * scan_f32_any_kernel: scan_f32_kernel's scheme with rows read as whole 16-byte pieces and then single dwords, never beyond D elements, and a
//    query image whose MIPS coordinate is +0.0f.
//  * Typed global pointers (GAS), 64-bit row offsets, vector stores only, no private segment.
#include "bang_scan_select.h"

#define SCAN8_ANY_IMG ((sizeof(Scan8Lds) + 15u) & ~(size_t)15u)            // offset of the query image in the workgroup's LDS
#define SCAN_KEY_2P24 ((uint64_t)0x4B800000u << 32)                         // (bits of 16777216.0f) << 32: no key of a sum beyond 2^24 is below it
#define SCAN8_ANY_U 4                                                       // k-steps of point bytes in flight per lane

// the canonical chain of one (query row, point) pair: ascending, (float)(v - q), fmaf.  D % 4 == 0; the image holds real 0 in [qdim, D)
template <bool IS_U8>
__device__ __forceinline__ float scan8_chain(const uint32_t* img, uint32_t qrow, const uint8_t GAS* v, uint32_t D) {
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

template <bool IS_U8>
__device__ __forceinline__ int scan8_any_norm(i32x4 f, int norm) {
  norm = __builtin_amdgcn_sdot4(f.x, f.x, norm, false);
  norm = __builtin_amdgcn_sdot4(f.y, f.y, norm, false);
  norm = __builtin_amdgcn_sdot4(f.z, f.z, norm, false);
  return __builtin_amdgcn_sdot4(f.w, f.w, norm, false);
}

template <bool IS_U8>
__global__ __launch_bounds__(256) void scan8_any_kernel(const ScanArgs a, const uint32_t qdim) {
  extern __shared__ __attribute__((aligned(16))) uint8_t scan_smem[];
  Scan8Lds& s = *(Scan8Lds*)scan_smem;
  i32x4* qimg = (i32x4*)(scan_smem + SCAN8_ANY_IMG);                       // [KS][64]: piece 64 s + lane
  __shared__ int qnorm[SCAN8_QT];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t r = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
  const uint32_t q0 = blockIdx.x * SCAN8_QT, stripe = blockIdx.y;
  const uint32_t D = a.D;
  const uint32_t KSF = D >> 5, KS = (D + 31u) >> 5;                        // (uniform) whole k-steps, all k-steps
  scan_lds_init(s, a, q0);
  if (threadIdx.x < (uint32_t)SCAN8_QT) qnorm[threadIdx.x] = 0;
  __syncthreads();
  // the tile's queries, once: shifted, real 0 in [qdim, D) (the MIPS coordinate), int8 0 behind D; a row behind nq repeats the last query
  for (uint32_t idx = threadIdx.x; idx < KS * 64u; idx += 256u) {
    const uint32_t rr = idx & 31u, b = 32u * (idx >> 6) + 16u * ((idx >> 5) & 1u);
    const uint32_t q = q0 + rr < a.nq ? q0 + rr : a.nq - 1u;
    const uint8_t GAS* src = (const uint8_t GAS*)a.queries + (uint64_t)q * qdim;   // (rows of D - 1 bytes are not dword-aligned: byte loads)
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
    const int part = scan8_any_norm<IS_U8>(f, 0);
    if (part != 0) (void)__hip_atomic_fetch_add(&qnorm[rr], part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const uint64_t p_begin = (uint64_t)stripe * a.per;
  const uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  // the short k-step: dwords of this lane's piece inside the row
  const uint32_t tail_at = 32u * KSF + 16u * h;
  const uint32_t tail_dw = D > tail_at ? ((D - tail_at) >> 2 < 4u ? (D - tail_at) >> 2 : 4u) : 0u;
  uint32_t unfiltered = 0u;                                                // (uniform) valid points of this wave's tiles
  for (uint64_t base = p_begin; base < p_stop; base += SCAN8_ROUND) {      // (uniform over the workgroup)
    const uint64_t pt64 = base + wave * 32u + r;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;        // (p_begin < n_nodes here)
    const uint8_t GAS* row = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;
    const uint8_t GAS* mine = row + 16u * h;
    u32x4a cur[SCAN8_ANY_U], nxt[SCAN8_ANY_U];
#pragma unroll
    for (int u = 0; u < SCAN8_ANY_U; ++u) {
      cur[u] = (u32x4a){0u, 0u, 0u, 0u};
      if ((uint32_t)u < KSF) cur[u] = *(const u32x4a GAS*)(mine + 32u * (uint32_t)u);          // (uniform)
    }
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int pn = 0;
    for (uint32_t s0 = 0; s0 < KSF; s0 += SCAN8_ANY_U) {                   // (uniform)
#pragma unroll
      for (int u = 0; u < SCAN8_ANY_U; ++u) {
        nxt[u] = (u32x4a){0u, 0u, 0u, 0u};
        const uint32_t ks = s0 + SCAN8_ANY_U + (uint32_t)u;
        if (ks < KSF) nxt[u] = *(const u32x4a GAS*)(mine + 32u * ks);      // (uniform)
      }
#pragma unroll
      for (int u = 0; u < SCAN8_ANY_U; ++u) {
        const uint32_t ks = s0 + (uint32_t)u;
        if (ks < KSF) {                                                    // (uniform)
          u32x4a w = cur[u];
          if (IS_U8) { w.x ^= 0x80808080u; w.y ^= 0x80808080u; w.z ^= 0x80808080u; w.w ^= 0x80808080u; }
          const i32x4 bf = {(int)w.x, (int)w.y, (int)w.z, (int)w.w};
          pn = scan8_any_norm<IS_U8>(bf, pn);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * ks + (uint32_t)lane], bf, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < SCAN8_ANY_U; ++u) cur[u] = nxt[u];
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
      pn = scan8_any_norm<IS_U8>(bf, pn);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qimg[64u * KSF + (uint32_t)lane], bf, acc, 0, 0, 0);
    }
    pn += __shfl_xor(pn, 32);                                              // both halves of the column
    if (!filtered) unfiltered += (uint32_t)__popc((uint32_t)__ballot(valid));     // (the low half: each point once)
    // register i of lane (r, h): query row (i & 3) + 8 (i >> 2) + 4 h, point column r
    uint32_t slow = 0u;                                                    // registers whose sum is beyond 2^24 and whose row still takes such keys
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qrow = (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
      const int d = qnorm[qrow] + pn - 2 * acc[i];
      const uint64_t key = ((uint64_t)__float_as_uint((float)d) << 32) | pt;
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[qrow][0], s.flt[qrow][1]);
        const uint64_t mb = __ballot(m);
        const uint32_t hm = h ? (uint32_t)(mb >> 32) : (uint32_t)mb;
        if (r == 0u && hm != 0u) (void)__hip_atomic_fetch_add(&s.mcnt[qrow], (uint32_t)__popc(hm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      const uint64_t thr = s.thr[qrow];
      const bool big = d > (1 << 24);
      if (m && big && thr >= SCAN_KEY_2P24) slow |= 1u << i;
      scan_offer<SCAN8_CAP, true>(s.keys[qrow], &s.cnt[qrow], m && !big && key < thr, key, lane);
    }
    if (__ballot(slow != 0u) != 0ull) {                                    // (uniform) rare once the lists have been cut
#pragma unroll 1
      for (uint32_t i = 0; i < 16u; ++i) {
        const bool again = ((slow >> i) & 1u) != 0u;
        if (__ballot(again) == 0ull) continue;                             // (uniform)
        const uint32_t qrow = (i & 3u) + 8u * (i >> 2) + 4u * h;
        float c = 0.0f;
        if (again) c = scan8_chain<IS_U8>((const uint32_t*)qimg, qrow, row, D);
        const uint64_t key = ((uint64_t)__float_as_uint(c) << 32) | pt;
        scan_offer<SCAN8_CAP, true>(s.keys[qrow], &s.cnt[qrow], again && key < s.thr[qrow], key, lane);
      }
    }
    __syncthreads();
    scan_cut_full<SCAN8_QT, SCAN8_CAP, SCAN8_ROUND>(s, wave, a.k, lane);
    __syncthreads();
  }
  if (!filtered && lane == 0 && unfiltered != 0u) (void)__hip_atomic_fetch_add(&s.mall, unfiltered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  scan_finish(s, a, q0, stripe, wave, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// float vectors of any D
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void scanf_any_step(float (&acc)[SCANF_QT], float x, const float* qd) {
#pragma unroll
  for (int j = 0; j < SCANF_QT; ++j) {
    const float diff = x - qd[j];                                          // vector - query, as orc_exact_dist
    acc[j] = __builtin_fmaf(diff, diff, acc[j]);                           // ascending dimension
  }
}

__global__ __launch_bounds__(256) void scan_f32_any_kernel(const ScanArgs a, const uint32_t qdim) {
  extern __shared__ __attribute__((aligned(16))) uint8_t scan_smem[];
  ScanFLds& s = *(ScanFLds*)scan_smem;
  float* qv = (float*)(scan_smem + sizeof(ScanFLds));                      // [D][16]: element d of the tile's queries, +0.0f in [qdim, D)
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t q0 = blockIdx.x * SCANF_QT, stripe = blockIdx.y;
  const uint32_t D = a.D, D4 = a.D & ~3u;
  scan_lds_init(s, a, q0);
  for (uint32_t i = threadIdx.x; i < D * SCANF_QT; i += blockDim.x) {
    const uint32_t d = i / SCANF_QT, j = i % SCANF_QT;
    const uint32_t q = q0 + j < a.nq ? q0 + j : a.nq - 1u;
    qv[i] = d < qdim ? ((const float GAS*)a.queries)[(uint64_t)q * qdim + d] : 0.0f;
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const uint64_t p_begin = (uint64_t)stripe * a.per;
  const uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  uint32_t unfiltered = 0u;
  for (uint64_t base = p_begin; base < p_stop; base += SCANF_ROUND) {      // (uniform over the workgroup)
    const uint64_t pt64 = base + threadIdx.x;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;
    const uint8_t GAS* v = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;     // (dword-aligned only: u32x4a is typed so)
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    float acc[SCANF_QT];
#pragma unroll
    for (int j = 0; j < SCANF_QT; ++j) acc[j] = 0.0f;
    for (uint32_t d = 0; d < D4; d += 4u) {                                // (uniform) the whole 16-byte pieces
      const u32x4a w = *(const u32x4a GAS*)(v + 4u * d);
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) scanf_any_step(acc, __uint_as_float(ww[e]), qv + (d + (uint32_t)e) * SCANF_QT);
    }
    for (uint32_t d = D4; d < D; ++d)                                      // (uniform) the last D % 4 elements, one dword each
      scanf_any_step(acc, __uint_as_float(*(const uint32_t GAS*)(v + 4u * d)), qv + d * SCANF_QT);
    if (!filtered) unfiltered += (uint32_t)__popcll(__ballot(valid));
#pragma unroll
    for (int j = 0; j < SCANF_QT; ++j) {
      const uint64_t key = ((uint64_t)__float_as_uint(acc[j]) << 32) | pt;
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[j][0], s.flt[j][1]);
        const uint64_t mb = __ballot(m);
        if (lane == 0 && mb != 0ull) (void)__hip_atomic_fetch_add(&s.mcnt[j], (uint32_t)__popcll(mb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      scan_offer<SCANF_CAP, false>(s.keys[j], &s.cnt[j], m && key < s.thr[j], key, lane);
    }
    __syncthreads();
    scan_cut_full<SCANF_QT, SCANF_CAP, SCANF_ROUND>(s, wave, a.k, lane);
    __syncthreads();
  }
  if (!filtered && lane == 0 && unfiltered != 0u) (void)__hip_atomic_fetch_add(&s.mall, unfiltered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  scan_finish(s, a, q0, stripe, wave, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// the entry: checks, one launch by dtype, then bang_scan.hip's merge and outputs
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int bang_k_scan_any(const bang_scan_params* p, uint32_t qdim, void* stream) { return bang_k_scan_any_marked(p, qdim, stream, nullptr); }

extern "C" int bang_k_scan_any_marked(const bang_scan_params* p, uint32_t qdim, void* stream, void* ev_merge) {
  {
    const int rc = bang_scan_any_check(p, qdim);
    if (rc != BANG_OK) return rc;
  }
  uint32_t tiles = 0, stripes = 0;
  {
    const int rc = bang_scan_any_geometry((int)p->dtype, p->D, p->nq, p->n_nodes, p->k, &tiles, &stripes);
    if (rc != BANG_OK) { bang_set_error("bang_k_scan_any: no geometry for this launch"); return rc; }
  }
  if (p->stripes != 0u) stripes = p->stripes;
  ScanArgs a;
  uint32_t* d_count = nullptr;
  BANG_TRY(scan_prepare(p, stripes, p->dtype == BANG_F32 ? SCANF_ROUND : SCAN8_ROUND, &a, &d_count, stream));
  if (p->dtype == BANG_F32) {
    BANG_TRY(scan_launch<scan_f32_any_kernel>(a, tiles, sizeof(ScanFLds) + (size_t)p->D * SCANF_QT * 4,
                                              sizeof(ScanFLds) + (size_t)BANG_SCAN_ANY_MAX_D * SCANF_QT * 4, stream, qdim));
  } else {
    const size_t lds = SCAN8_ANY_IMG + (size_t)((p->D + 31u) / 32u) * 1024u, most = SCAN8_ANY_IMG + (size_t)BANG_SCAN_ANY_MAX_D * 32u;
    if (p->dtype == BANG_U8) BANG_TRY(scan_launch<scan8_any_kernel<true>>(a, tiles, lds, most, stream, qdim));
    else BANG_TRY(scan_launch<scan8_any_kernel<false>>(a, tiles, lds, most, stream, qdim));
  }
  return scan_merge_out(a, p, d_count, stream, ev_merge);
}
