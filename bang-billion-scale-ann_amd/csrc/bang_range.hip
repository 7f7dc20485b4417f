// bang_range.hip -- range search (DESIGN.md section 2 CANON 19, section 4.14): what runs BEHIND the exact-distance launch that collected a batch's hit
// log (bang_k_search_exact_range).  A query's row of the log holds its first min(offered, cap) hits in evaluation order; range_sort_kernel
// (bang_k_range_sort) turns it into the query's answer: sorted ascending by the 64-bit key (distance bits << 32) | id, adjacent equal keys -- an id
// that an adjacency row lists twice is evaluated twice -- dropped, written back in place, the remaining number in d_count.
//
//  * One wave per query; RANGE_WAVES(cap) waves per workgroup.  n = min(offered, cap) keys, padded with ~0 to P = the next power of two (>= 64).
//  * P == 64: the row is one key per lane and the bitonic network runs in registers -- the partner's key comes through ds_bpermute, no LDS
//    words are touched.  P > 64: the keys sit in the wave's 8 P bytes of LDS (at most 32 KB at cap = 4096) and every lane takes P / 128 of a
//    stage's compare-exchanges; a wave runs its LDS instructions in program order, so the stages need no barrier beyond wave_sync.  In a stage of
//    distance j the lanes of a wave read 64 consecutive 8-byte keys (j >= 64) or two runs of them: no bank conflict beyond the 2-way one of
//    64 x 8 bytes over 64 banks x 4 bytes, which ds_read_b64 serves in two passes anyway.
//  * Duplicates: key[i] == key[i - 1], __ballot of the keepers, lanes_below for a keeper's slot behind a wave-uniform base, 64 keys at a time.
//  * Vector stores only; the dynamic LDS of a workgroup stays within the 64 KB every kernel may ask for.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"

struct RangeSortArgs {
  uint32_t* hit_ids;                 // [Q_total][cap]
  float* hit_dists;                  // [Q_total][cap]
  const uint32_t* offered;           // [Q_total]
  uint32_t* count;                   // [Q_total]
  uint32_t cap, q0, nq, wave_keys;   // wave_keys: 64-bit LDS words per wave (cap rounded up to a power of two, >= 64)
};

static inline uint32_t range_pow2(uint32_t n) {                    // the next power of two, at least 64
  uint32_t p = 64u;
  while (p < n) p <<= 1;
  return p;
}
// waves per workgroup: what 64 KB of LDS hold at 8 bytes x wave_keys per wave, at most four
static inline uint32_t range_waves(uint32_t wave_keys) {
  const uint32_t w = 65536u / (8u * wave_keys);
  return w > 4u ? 4u : (w < 1u ? 1u : w);
}

__device__ __forceinline__ uint64_t shfl_key(uint64_t k, uint32_t src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(uint32_t)k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)(uint32_t)(k >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void range_sort_kernel(const RangeSortArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t rkeys[];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t qi = blockIdx.x * (blockDim.x >> 6) + wave;
  if (qi >= a.nq) return;                                          // (uniform per wave; the kernel has no workgroup barrier)
  const uint32_t q = a.q0 + qi;
  uint32_t GAS* ids = (uint32_t GAS*)a.hit_ids + (uint64_t)q * a.cap;
  uint32_t GAS* dists = (uint32_t GAS*)a.hit_dists + (uint64_t)q * a.cap;      // (the distance bits)
  uint32_t n = uni(((const uint32_t GAS*)a.offered)[q]);
  if (n > a.cap) n = a.cap;                                        // (the kept hits never leave the query's row)
  uint32_t P = 64u;
  while (P < n) P <<= 1;                                           // (uniform; <= wave_keys)
  uint32_t base = 0;
  if (P == 64u) {
    // ---------------- one key per lane: the network in registers
    uint64_t key = ~0ull;
    if ((uint32_t)lane < n) key = ((uint64_t)dists[lane] << 32) | ids[lane];
    for (uint32_t k = 2; k <= 64u; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        const uint64_t other = shfl_key(key, (uint32_t)lane ^ j);
        const bool up = ((uint32_t)lane & k) == 0u;                // this k-block sorts ascending
        const bool lower = ((uint32_t)lane & j) == 0u;             // this lane keeps the smaller key of an ascending pair
        const bool take_min = up == lower;
        if (take_min ? other < key : other > key) key = other;
      }
    }
    const uint64_t prev = shfl_key(key, ((uint32_t)lane + 63u) & 63u);
    const bool keep = (uint32_t)lane < n && (lane == 0 || key != prev);
    const uint64_t mask = __ballot(keep);
    if (keep) { const uint32_t at = lanes_below(mask); ids[at] = (uint32_t)key; dists[at] = (uint32_t)(key >> 32); }
    base = (uint32_t)__popcll(mask);
  } else {
    // ---------------- P = 128 .. 4096 keys in the wave's LDS
    uint64_t* keys = rkeys + (size_t)wave * a.wave_keys;
    for (uint32_t i = (uint32_t)lane; i < P; i += WAVE) keys[i] = i < n ? (((uint64_t)dists[i] << 32) | ids[i]) : ~0ull;
    wave_sync();
    for (uint32_t k = 2; k <= P; k <<= 1) {
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t t = (uint32_t)lane; t < (P >> 1); t += WAVE) {       // compare-exchange t of the stage: (l, l + j)
          const uint32_t l = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
          const uint64_t x = keys[l], y = keys[l + j];
          const bool up = (l & k) == 0u;
          if (up ? x > y : x < y) { keys[l] = y; keys[l + j] = x; }
        }
        wave_sync();
      }
    }
    // the first n keys are the hits (every padding key ~0 is larger than any {distance bits, id}); all loads of the row are long done
    for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {                    // (uniform)
      const uint32_t i = i0 + (uint32_t)lane;
      const uint64_t key = keys[i < n ? i : 0u];
      const uint64_t prev = keys[(i < n && i > 0u) ? i - 1u : 0u];
      const bool keep = i < n && (i == 0u || key != prev);
      const uint64_t mask = __ballot(keep);
      if (keep) { const uint32_t at = base + lanes_below(mask); ids[at] = (uint32_t)key; dists[at] = (uint32_t)(key >> 32); }
      base += (uint32_t)__popcll(mask);
    }
  }
  if (lane == 0) ((uint32_t GAS*)a.count)[q] = base;
}

extern "C" int bang_k_range_sort(uint32_t* d_hit_ids, float* d_hit_dists, const uint32_t* d_offered, uint32_t cap, uint32_t q0, uint32_t nq,
                                 uint32_t Q_total, uint32_t* d_count, void* stream) {
  if (!d_hit_ids) { bang_set_error("bang_k_range_sort: d_hit_ids is null"); return BANG_ERR_ARG; }
  if (!d_hit_dists) { bang_set_error("bang_k_range_sort: d_hit_dists is null"); return BANG_ERR_ARG; }
  if (!d_offered) { bang_set_error("bang_k_range_sort: d_offered is null"); return BANG_ERR_ARG; }
  if (!d_count) { bang_set_error("bang_k_range_sort: d_count is null"); return BANG_ERR_ARG; }
  if (cap == 0 || cap > BANG_RANGE_MAX_HITS) { bang_set_error("bang_k_range_sort: cap = %u is outside [1, %u]", cap, BANG_RANGE_MAX_HITS); return BANG_ERR_ARG; }
  if ((uint64_t)q0 + nq > Q_total) { bang_set_error("bang_k_range_sort: q0 + nq = %llu exceeds Q_total = %u", (unsigned long long)q0 + nq, Q_total); return BANG_ERR_ARG; }
  if (nq == 0) return BANG_OK;
  RangeSortArgs a;
  a.hit_ids = d_hit_ids; a.hit_dists = d_hit_dists; a.offered = d_offered; a.count = d_count;
  a.cap = cap; a.q0 = q0; a.nq = nq; a.wave_keys = range_pow2(cap);
  const uint32_t waves = range_waves(a.wave_keys);
  const size_t lds = a.wave_keys > 64u ? (size_t)waves * a.wave_keys * 8u : 0u;     // (a row of <= 64 keys is sorted in registers)
  hipLaunchKernelGGL(range_sort_kernel, dim3((nq + waves - 1) / waves), dim3(waves * WAVE), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
