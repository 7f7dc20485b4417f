// bang_scan_select.h -- what the kernels of the exact scan share (bang_scan.hip: the narrow layouts; bang_scan_any.hip: option scan_any): the
// kernel arguments, the LDS of a workgroup and the selection -- threshold keys, offers, cuts, the end of a stripe.
// Whole device functions only: a kernel that includes this file inlines them as it inlined its own copy.
#ifndef BANG_SCAN_SELECT_H_
#define BANG_SCAN_SELECT_H_

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

// the tiles of the two schemes: 8-bit vectors on the i8 MFMA, float vectors one lane per point
#define SCAN8_QT 32
#define SCAN8_CAP 256
#define SCAN8_ROUND 128
typedef ScanLds<SCAN8_QT, SCAN8_CAP> Scan8Lds;
#define SCANF_QT 16
#define SCANF_CAP 512
#define SCANF_ROUND 256
typedef ScanLds<SCANF_QT, SCANF_CAP> ScanFLds;

#define BANG_TRY(x)               \
  do {                            \
    int _r = (x);                 \
    if (_r != BANG_OK) return _r; \
  } while (0)

// One launch of instance KERNEL with the arguments rest... behind ScanArgs.  The lists take more than the 64 KB of dynamic LDS a kernel may ask for
// unprompted: the instance's limit is raised once per device to lds_most, the most a launch of it ever asks for (KERNEL is a template argument, so
// every instance has its own flags)
template <auto KERNEL, class... Rest>
static int scan_launch(const ScanArgs& a, uint32_t tiles, size_t lds, size_t lds_most, void* stream, Rest... rest) {
  static bool raised[BANG_MAX_DEVICES] = {false};
  const int dev = current_device();
  if (!raised[dev]) {
    HIP_TRY(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_most));
    raised[dev] = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(tiles, a.stripes), dim3(256), lds, (hipStream_t)stream, a, rest...);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

// bang_scan.hip, host side, for both entries.  scan_prepare: the kernel arguments of a checked launch in `stripes` stripes of rounds of `round`
// points -- the lists, the offered words and *d_count laid out in p->d_scratch -- and the matched counts cleared on the stream.  scan_merge_out: what
// follows the scan launch in stream order -- the event, bang_k_range_sort over the stripes' lists, scan_out_kernel
int scan_prepare(const bang_scan_params* p, uint32_t stripes, uint32_t round, ScanArgs* a, uint32_t** d_count, void* stream);
int scan_merge_out(const ScanArgs& a, const bang_scan_params* p, uint32_t* d_count, void* stream, void* ev_merge);

#endif
