// bang_scan.hip -- the exact scan (DESIGN.md section 2 CANON 23, section 4.17): the k nearest of every live point, by brute force.
//
//  * A workgroup of four waves takes a tile of QT queries and one stripe of the points, a ROUND of points at a time; between two rounds the waves
//    meet at a barrier and each cuts the lists of its share of the queries.
//  * scan8_kernel (uint8 / int8): QT = 32, a round is four tiles of 32 points, one per wave.  |a - b|^2 = |a'|^2 - 2 a'.b' + |b'|^2 in i32, with
//    uint8 bytes taken as int8 after ^ 0x80 (a - b does not see the shift).  The products are v_mfma_i32_32x32x32_i8: queries on the rows (A), points
//    on the columns (B), so that the 32 lanes of a half-wave hold 32 different points of ONE query in every accumulator register.  Lane (r, h) loads
//    bytes [32 s + 16 h, 32 s + 16 h + 16) of row / column r for k-step s, A and B alike: the sum over k does not depend on which k a byte lands on
//    as long as both operands agree.  D = 16 is half a k-step: the lanes of h = 1 hold zeros.  The row norms are v_dot4 on the bytes already loaded.
//    The largest sum is 256 x 255^2 < 2^24: the float image is exact and equal to the ascending fmaf chain's (CANON 10).
//  * scan_f32_kernel: QT = 16, a round is 256 points, one per lane; the lane runs the 16 ascending fmaf chains of its point, (vector - query)^2, the
//    query elements broadcast from LDS.  No matrix instruction reproduces that chain.
//  * Selection, shared: per query a threshold key in LDS (the k-th smallest key so far, ~0 before there are k), a ballot of the lanes whose key is
//    below it, one LDS atomic per (query, wave) for the slots, mbcnt for a lane's slot.  A list holds CAP keys; a round adds at most ROUND, and a list
//    longer than CAP - ROUND at a barrier is sorted (the bitonic network of bang_range.hip, one wave) and cut to k.
//  * A (query, stripe) leaves its <= k keys, padded with ~0, in the scratch rows bang_k_range_sort reads; scan_out_kernel writes the first k of the
//    merged row in the output layout.  matched: popcounts per query in LDS, one global atomic add per (query, stripe).
//  * Typed global pointers (GAS), 64-bit row offsets, vector stores only, no private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct ScanArgs {
  const uint8_t* vec_base; uint64_t vec_stride;
  const void* queries;
  const uint32_t* excl; const uint32_t* removed; const uint32_t* labels; const uint32_t* filters;
  uint32_t* part_ids; uint32_t* part_dists; uint32_t* offered; uint32_t* matched;
  uint64_t per;                                          // points of a stripe, a multiple of the round
  uint32_t D, n_nodes, nq, k, stripes;
};

#define SCAN_PAD_KEY (~0ull)

// LDS of a workgroup, QT queries with lists of CAP keys
template <int QT, int CAP>
struct ScanLds {
  uint64_t keys[QT][CAP];
  uint64_t thr[QT];
  uint32_t cnt[QT];
  uint32_t mcnt[QT];
  uint32_t flt[QT][2];
  uint32_t mall;
};

template <int QT, int CAP>
__device__ __forceinline__ void scan_lds_init(ScanLds<QT, CAP>& s, const ScanArgs& a, uint32_t q0) {
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)QT) {
    s.thr[t] = SCAN_PAD_KEY; s.cnt[t] = 0u; s.mcnt[t] = 0u;
    const uint32_t q = q0 + t;
    const bool f = a.filters != nullptr && q < a.nq;
    s.flt[t][0] = f ? ((const uint32_t GAS*)a.filters)[2ull * q] : 0u;
    s.flt[t][1] = f ? ((const uint32_t GAS*)a.filters)[2ull * q + 1u] : 0u;
  }
  if (t == 0u) s.mall = 0u;
}

// the lanes with `pass` append their keys to the list of `row`; HALVES: the two half-waves offer to two different rows
template <int CAP, bool HALVES>
__device__ __forceinline__ void scan_offer(uint64_t* keys_row, uint32_t* cnt_row, bool pass, uint64_t key, int lane) {
  const uint64_t pb = __ballot(pass);
  if (pb == 0ull) return;                                                  // (uniform)
  uint32_t total, below;
  bool lead;
  if (HALVES) {
    const uint32_t hm = (lane & 32) ? (uint32_t)(pb >> 32) : (uint32_t)pb;
    total = (uint32_t)__popc(hm);
    below = (uint32_t)__popc(hm & ((1u << (lane & 31)) - 1u));
    lead = (lane & 31) == 0;
  } else {
    total = (uint32_t)__popcll(pb);
    below = lanes_below(pb);
    lead = lane == 0;
  }
  uint32_t base = 0u;
  if (lead && total != 0u) base = __hip_atomic_fetch_add(cnt_row, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  base = (uint32_t)__shfl((int)base, HALVES ? (lane & 32) : 0);
  if (pass && base + below < (uint32_t)CAP) keys_row[base + below] = key;      // (never beyond CAP: a list enters a round with <= CAP - ROUND keys)
}

// one wave sorts the list of query qi and cuts it to k; the threshold becomes the k-th key once there are k
template <int QT, int CAP>
__device__ __forceinline__ void scan_cut(ScanLds<QT, CAP>& s, uint32_t qi, uint32_t k, int lane) {
  uint64_t* keys = s.keys[qi];
  uint32_t c = uni(s.cnt[qi]);
  if (c > (uint32_t)CAP) c = (uint32_t)CAP;
  uint32_t P = 64u;
  while (P < c) P <<= 1;                                                   // (uniform; <= CAP)
  for (uint32_t i = (uint32_t)lane; i < P; i += WAVE) if (i >= c) keys[i] = SCAN_PAD_KEY;
  wave_sync();
  for (uint32_t kk = 2; kk <= P; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t t = (uint32_t)lane; t < (P >> 1); t += WAVE) {
        const uint32_t l = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
        const uint64_t x = keys[l], y = keys[l + j];
        const bool up = (l & kk) == 0u;
        if (up ? x > y : x < y) { keys[l] = y; keys[l + j] = x; }
      }
      wave_sync();
    }
  }
  if (lane == 0) {
    s.cnt[qi] = c < k ? c : k;
    if (c >= k) s.thr[qi] = keys[k - 1u];
  }
  wave_sync();
}

// between two rounds: wave w cuts the lists of its queries that could overflow in the next round.  Both barriers are the caller's
template <int QT, int CAP, int ROUND>
__device__ __forceinline__ void scan_cut_full(ScanLds<QT, CAP>& s, uint32_t wave, uint32_t k, int lane) {
  for (uint32_t qi = wave; qi < (uint32_t)QT; qi += 4u) {
    if (uni(s.cnt[qi]) > (uint32_t)(CAP - ROUND)) scan_cut(s, qi, k, lane);
  }
}

// the end of a stripe: every list sorted and cut, its keys to the scratch rows, the matched counts to HBM
template <int QT, int CAP>
__device__ __forceinline__ void scan_finish(ScanLds<QT, CAP>& s, const ScanArgs& a, uint32_t q0, uint32_t stripe, uint32_t wave, int lane) {
  const uint32_t cap = a.stripes * a.k;
  for (uint32_t qi = wave; qi < (uint32_t)QT; qi += 4u) {
    const uint32_t q = q0 + qi;
    if (q >= a.nq) break;                                                  // (uniform)
    scan_cut(s, qi, a.k, lane);
    const uint32_t n = uni(s.cnt[qi]);
    const uint64_t row = (uint64_t)q * cap + (uint64_t)stripe * a.k;
    uint32_t GAS* ids = (uint32_t GAS*)a.part_ids + row;
    uint32_t GAS* dists = (uint32_t GAS*)a.part_dists + row;
    for (uint32_t i = (uint32_t)lane; i < a.k; i += WAVE) {
      const uint64_t key = i < n ? s.keys[qi][i] : SCAN_PAD_KEY;
      ids[i] = (uint32_t)key;
      dists[i] = (uint32_t)(key >> 32);
    }
    if (lane == 0) {
      const uint32_t m = s.mcnt[qi] + s.mall;
      if (m != 0u) (void)__hip_atomic_fetch_add((uint32_t GAS*)a.matched + q, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (stripe == 0u) ((uint32_t GAS*)a.offered)[q] = cap;
    }
  }
}

__device__ __forceinline__ bool scan_bit(const uint32_t* map, uint32_t id) {
  return ((((const uint32_t GAS*)map)[id >> 5] >> (id & 31u)) & 1u) != 0u;
}
__device__ __forceinline__ bool scan_match(uint32_t lab, uint32_t any, uint32_t all) {                 // CANON 18
  return (any == 0u || (lab & any) != 0u) && (lab & all) == all;
}

// ---------------------------------------------------------------------------------------------------------------------
// 8-bit vectors: KS k-steps of 32 bytes (D = 32 KS), or D = 16 as half a step (HALF)
// ---------------------------------------------------------------------------------------------------------------------
#define SCAN8_QT 32
#define SCAN8_CAP 256
#define SCAN8_ROUND 128
typedef ScanLds<SCAN8_QT, SCAN8_CAP> Scan8Lds;

template <bool IS_U8, int KS, bool HALF>
__device__ __forceinline__ int scan8_load(i32x4 (&f)[KS], const uint8_t GAS* row, uint32_t h) {
  int norm = 0;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    u32x4a w = {0u, 0u, 0u, 0u};
    if (!HALF || h == 0u) w = *(const u32x4a GAS*)(row + 32u * (uint32_t)s + (HALF ? 0u : 16u * h));
    if (IS_U8 && (!HALF || h == 0u)) { w.x ^= 0x80808080u; w.y ^= 0x80808080u; w.z ^= 0x80808080u; w.w ^= 0x80808080u; }
    f[s].x = (int)w.x; f[s].y = (int)w.y; f[s].z = (int)w.z; f[s].w = (int)w.w;
    norm = __builtin_amdgcn_sdot4(f[s].x, f[s].x, norm, false);
    norm = __builtin_amdgcn_sdot4(f[s].y, f[s].y, norm, false);
    norm = __builtin_amdgcn_sdot4(f[s].z, f[s].z, norm, false);
    norm = __builtin_amdgcn_sdot4(f[s].w, f[s].w, norm, false);
  }
  return norm + __shfl_xor(norm, 32);                                      // both halves of the row / column
}

template <bool IS_U8, int KS, bool HALF>
__global__ __launch_bounds__(256) void scan8_kernel(const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t scan_smem[];
  Scan8Lds& s = *(Scan8Lds*)scan_smem;
  __shared__ int qnorm[SCAN8_QT];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t r = (uint32_t)lane & 31u, h = (uint32_t)lane >> 5;
  const uint32_t q0 = blockIdx.x * SCAN8_QT, stripe = blockIdx.y;
  const uint32_t D = a.D;
  scan_lds_init(s, a, q0);
  // the query fragments stay in registers for the stripe; a row behind nq repeats the last query and is never written
  i32x4 qf[KS];
  {
    const uint32_t q = q0 + r < a.nq ? q0 + r : a.nq - 1u;
    const int qn = scan8_load<IS_U8, KS, HALF>(qf, (const uint8_t GAS*)a.queries + (uint64_t)q * D, h);
    if (wave == 0u && h == 0u) qnorm[r] = qn;
  }
  __syncthreads();
  const bool filtered = a.filters != nullptr;                              // (uniform)
  const uint64_t p_begin = (uint64_t)stripe * a.per;
  const uint64_t p_stop = p_begin + a.per < (uint64_t)a.n_nodes ? p_begin + a.per : (uint64_t)a.n_nodes;
  uint32_t unfiltered = 0u;                                                // (uniform) valid points of this wave's tiles
  for (uint64_t base = p_begin; base < p_stop; base += SCAN8_ROUND) {      // (uniform over the workgroup)
    const uint64_t pt64 = base + wave * 32u + r;
    bool valid = pt64 < p_stop;
    const uint32_t pt = valid ? (uint32_t)pt64 : (uint32_t)p_begin;        // (p_begin < n_nodes here)
    i32x4 bf[KS];
    const int pn = scan8_load<IS_U8, KS, HALF>(bf, (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride, h);
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(qf[ks], bf[ks], acc, 0, 0, 0);
    if (!filtered) unfiltered += (uint32_t)__popc((uint32_t)__ballot(valid));     // (the low half: each point once)
    // register i of lane (r, h): query row (i & 3) + 8 (i >> 2) + 4 h, point column r
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t row = (uint32_t)((i & 3) + 8 * (i >> 2)) + 4u * h;
      const int d = qnorm[row] + pn - 2 * acc[i];
      const uint64_t key = ((uint64_t)__float_as_uint((float)d) << 32) | pt;
      bool m = valid;
      if (filtered) {
        m = m && scan_match(lab, s.flt[row][0], s.flt[row][1]);
        const uint64_t mb = __ballot(m);
        const uint32_t hm = h ? (uint32_t)(mb >> 32) : (uint32_t)mb;
        if (r == 0u && hm != 0u) (void)__hip_atomic_fetch_add(&s.mcnt[row], (uint32_t)__popc(hm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      scan_offer<SCAN8_CAP, true>(s.keys[row], &s.cnt[row], m && key < s.thr[row], key, lane);
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
// float vectors
// ---------------------------------------------------------------------------------------------------------------------
#define SCANF_QT 16
#define SCANF_CAP 512
#define SCANF_ROUND 256
typedef ScanLds<SCANF_QT, SCANF_CAP> ScanFLds;

__global__ __launch_bounds__(256) void scan_f32_kernel(const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t scan_smem[];
  ScanFLds& s = *(ScanFLds*)scan_smem;
  float* qv = (float*)(scan_smem + sizeof(ScanFLds));                      // [D][16]: element d of the tile's queries
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t q0 = blockIdx.x * SCANF_QT, stripe = blockIdx.y;
  const uint32_t D = a.D;
  scan_lds_init(s, a, q0);
  for (uint32_t i = threadIdx.x; i < D * SCANF_QT; i += blockDim.x) {
    const uint32_t d = i / SCANF_QT, j = i % SCANF_QT;
    const uint32_t q = q0 + j < a.nq ? q0 + j : a.nq - 1u;
    qv[i] = ((const float GAS*)a.queries)[(uint64_t)q * D + d];
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
    const uint8_t GAS* v = (const uint8_t GAS*)a.vec_base + (uint64_t)pt * a.vec_stride;
    if (a.excl != nullptr && scan_bit(a.excl, pt)) valid = false;
    if (a.removed != nullptr && scan_bit(a.removed, pt)) valid = false;
    const uint32_t lab = filtered ? ((const uint32_t GAS*)a.labels)[pt] : 0u;
    float acc[SCANF_QT];
#pragma unroll
    for (int j = 0; j < SCANF_QT; ++j) acc[j] = 0.0f;
    for (uint32_t d = 0; d < D; d += 4u) {                                 // (uniform) D % 4 == 0
      const u32x4a w = *(const u32x4a GAS*)(v + 4u * d);
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = __uint_as_float(ww[e]);
        const float* qd = qv + (d + (uint32_t)e) * SCANF_QT;
#pragma unroll
        for (int j = 0; j < SCANF_QT; ++j) {
          const float diff = x - qd[j];                                    // vector - query, as orc_exact_dist
          acc[j] = __builtin_fmaf(diff, diff, acc[j]);                     // ascending dimension
        }
      }
    }
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
// the outputs: the first k keys of a query's merged row (sorted by bang_k_range_sort, n = d_count[q] of them, a padding key among them at most once)
// ---------------------------------------------------------------------------------------------------------------------
struct ScanOutArgs {
  const uint32_t* ids; const uint32_t* dists; const uint32_t* count;
  uint64_t* ids_out; float* dists_out;
  uint32_t nq, k, cap;
};
__global__ __launch_bounds__(256) void scan_out_kernel(const ScanOutArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)a.nq * a.k) return;
  const uint32_t q = (uint32_t)(t / a.k), i = (uint32_t)(t % a.k);
  const uint32_t n = ((const uint32_t GAS*)a.count)[q];
  uint32_t id = 0xFFFFFFFFu, db = 0xFFFFFFFFu;
  if (i < n) { id = ((const uint32_t GAS*)a.ids)[(uint64_t)q * a.cap + i]; db = ((const uint32_t GAS*)a.dists)[(uint64_t)q * a.cap + i]; }
  const bool pad = id == 0xFFFFFFFFu && db == 0xFFFFFFFFu;
  ((uint64_t GAS*)a.ids_out)[(uint64_t)q * a.k + i] = pad ? ~0ull : (uint64_t)id;              // CANON 8
  ((float GAS*)a.dists_out)[(uint64_t)i * a.nq + q] = pad ? BIG_DIST : __uint_as_float(db);
}

struct BitmapOrArgs { uint32_t* dst; const uint32_t* src; uint64_t words, skip_word; uint32_t skip_mask; };
__global__ __launch_bounds__(256) void bitmap_or_kernel(const BitmapOrArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.words) return;
  uint32_t x = ((const uint32_t GAS*)a.src)[w];
  if (w == a.skip_word) x &= ~a.skip_mask;
  if (x != 0u) ((uint32_t GAS*)a.dst)[w] |= x;
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------------
#define BANG_TRY(x)               \
  do {                            \
    int _r = (x);                 \
    if (_r != BANG_OK) return _r; \
  } while (0)

// One launch of instance KERNEL.  The lists take more than the 64 KB of dynamic LDS a kernel may ask for unprompted: the instance's limit is raised
// once per device to lds_most, the most a launch of it ever asks for (KERNEL is a template argument, so every instance has its own flags)
template <void (*KERNEL)(const ScanArgs)>
static int scan_launch(const ScanArgs& a, uint32_t tiles, size_t lds, size_t lds_most, void* stream) {
  static bool raised[BANG_MAX_DEVICES] = {false};
  const int dev = current_device();
  if (!raised[dev]) {
    HIP_TRY(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_most));
    raised[dev] = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(tiles, a.stripes), dim3(256), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

template <bool IS_U8>
static int scan8_dispatch(const ScanArgs& a, uint32_t tiles, void* stream) {
  const size_t lds = sizeof(Scan8Lds);
  switch (a.D) {
    case 16: return scan_launch<scan8_kernel<IS_U8, 1, true>>(a, tiles, lds, lds, stream);
    case 32: return scan_launch<scan8_kernel<IS_U8, 1, false>>(a, tiles, lds, lds, stream);
    case 64: return scan_launch<scan8_kernel<IS_U8, 2, false>>(a, tiles, lds, lds, stream);
    case 128: return scan_launch<scan8_kernel<IS_U8, 4, false>>(a, tiles, lds, lds, stream);
    case 256: return scan_launch<scan8_kernel<IS_U8, 8, false>>(a, tiles, lds, lds, stream);
    default: break;
  }
  bang_set_error("bang_k_scan: no instance for 8-bit vectors of D = %u", a.D);
  return BANG_ERR_UNSUPPORTED;
}

extern "C" int bang_k_scan(const bang_scan_params* p, void* stream) { return bang_k_scan_marked(p, stream, nullptr); }

extern "C" int bang_k_scan_marked(const bang_scan_params* p, void* stream, void* ev_merge) {
  {
    const int rc = bang_scan_check(p);
    if (rc != BANG_OK) return rc;
  }
  uint32_t tiles = 0, stripes = 0;
  {
    const int rc = bang_scan_geometry((int)p->dtype, p->D, p->nq, p->n_nodes, p->k, &tiles, &stripes);
    if (rc != BANG_OK) { bang_set_error("bang_k_scan: no geometry for this launch"); return rc; }
  }
  if (p->stripes != 0u) stripes = p->stripes;
  const uint32_t round = p->dtype == BANG_F32 ? SCANF_ROUND : SCAN8_ROUND;
  const uint32_t cap = stripes * p->k;
  ScanArgs a;
  a.vec_base = p->d_vec_base; a.vec_stride = p->vec_stride; a.queries = p->d_queries;
  a.excl = p->d_excluded; a.removed = p->d_removed; a.labels = p->d_labels; a.filters = p->d_filters;
  a.part_ids = (uint32_t*)p->d_scratch;
  a.part_dists = a.part_ids + (size_t)p->nq * cap;
  a.offered = a.part_dists + (size_t)p->nq * cap;
  uint32_t* d_count = a.offered + p->nq;
  a.matched = p->d_matched;
  a.D = p->D; a.n_nodes = p->n_nodes; a.nq = p->nq; a.k = p->k; a.stripes = stripes;
  const uint64_t per = ((uint64_t)p->n_nodes + stripes - 1u) / stripes;
  a.per = (per + round - 1u) / round * round;
  HIP_TRY(hipMemsetAsync(p->d_matched, 0, (size_t)p->nq * 4, (hipStream_t)stream));
  if (p->dtype == BANG_F32) {
    BANG_TRY(scan_launch<scan_f32_kernel>(a, tiles, sizeof(ScanFLds) + (size_t)p->D * SCANF_QT * 4, sizeof(ScanFLds) + (size_t)256 * SCANF_QT * 4, stream));
  } else if (p->dtype == BANG_U8) {
    BANG_TRY(scan8_dispatch<true>(a, tiles, stream));
  } else {
    BANG_TRY(scan8_dispatch<false>(a, tiles, stream));
  }
  if (ev_merge) HIP_TRY(hipEventRecord((hipEvent_t)ev_merge, (hipStream_t)stream));
  BANG_TRY(bang_k_range_sort(a.part_ids, (float*)a.part_dists, a.offered, cap, 0, p->nq, p->nq, d_count, stream));
  ScanOutArgs o;
  o.ids = a.part_ids; o.dists = a.part_dists; o.count = d_count; o.ids_out = p->d_ids_out; o.dists_out = p->d_dists_out;
  o.nq = p->nq; o.k = p->k; o.cap = cap;
  const uint64_t threads = (uint64_t)p->nq * p->k;
  hipLaunchKernelGGL(scan_out_kernel, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, o);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_bitmap_or(uint32_t* d_dst, const uint32_t* d_src, uint64_t words, uint64_t skip_word, uint32_t skip_mask, void* stream) {
  if (!d_dst) { bang_set_error("bang_k_bitmap_or: d_dst is null"); return BANG_ERR_ARG; }
  if (!d_src) { bang_set_error("bang_k_bitmap_or: d_src is null"); return BANG_ERR_ARG; }
  if (words == 0) return BANG_OK;
  if (words > (1ull << 32)) { bang_set_error("bang_k_bitmap_or: words = %llu exceeds 2^32", (unsigned long long)words); return BANG_ERR_ARG; }
  BitmapOrArgs a;
  a.dst = d_dst; a.src = d_src; a.words = words; a.skip_word = skip_word; a.skip_mask = skip_mask;
  hipLaunchKernelGGL(bitmap_or_kernel, dim3((uint32_t)((words + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
