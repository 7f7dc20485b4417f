// bang_exact_dist.h -- what the wave-resident search kernels share beside bang_worklist.h: the LDS layout of a wave (bang_search_exact.hip,
// bang_search_beam.hip, bang_search_lut.hip) and the exact distances of the narrow vector layouts (the first two).  Whole device functions only:
// a kernel that includes this file inlines them as it inlined its own copy.
#ifndef BANG_EXACT_DIST_H_
#define BANG_EXACT_DIST_H_

#include "bang_device.h"

#define WAVE_SCRATCH_WORDS 144u      // sd/ti [72] + td/compaction [72] (the survivors' distances, then the sort)
#define WAVE_MAX_LDS BANG_WAVE_MAX_LDS   // 160 KB, what bang_wave_geometry divides among a CU's waves

// LDS words of a wave's worklist: 2L + ceil(L/4), rounded to 4
static __host__ __device__ inline uint32_t wave_wl_words(uint32_t L) { return (2u * L + (L + 3u) / 4u + 3u) & ~3u; }

template <bool SIGNED>
__device__ __forceinline__ int xdot4(uint32_t a, uint32_t b, int c) {
  if (SIGNED) return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
  return (int)__builtin_amdgcn_udot4(a, b, (uint32_t)c, false);
}

// exact distances of the n survivors (ids in LDS: sid[0, n)) -> dist[0, n) in LDS, 8-bit vectors.  qw: this lane's 16-byte piece of the
// query (piece lane % G), qq: the sum of its squares.  Every lane of the wave executes (the G lanes of a survivor reduce by xor-shuffles).
template <bool SIGNED>
__device__ __forceinline__ void exact_dist8(const uint8_t GAS* graph, uint64_t entry_len, uint32_t G, const uint32_t* sid, uint32_t n,
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

// the same for float vectors: lane i evaluates survivor i0 + i, the ascending fmaf chain over the D dimensions (D % 4 == 0, <= 256);
// qr[t]: lane l holds query element 64 t + l, read with v_readlane (the dimension index is uniform)
__device__ __forceinline__ void exact_dist_f32(const uint8_t GAS* graph, uint64_t entry_len, uint32_t D, const uint32_t* sid, uint32_t n,
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
              const float diff = __uint_as_float(ww[d]) - qv;     // parANN.cu:1139-1179 / orc_exact_dist: vector - query
              acc = __builtin_fmaf(diff, diff, acc);              // ascending dimension
            }
          }
        }
      }
    }
    if (i < n) dist[i] = acc;
  }
}

// pulled rows: the slice table's entry idx (biased base addresses, 0 = that slice is not there), through the scalar cache
__device__ __forceinline__ uint64_t slice_base(const uint64_t* tab, uint32_t idx) {
  uint64_t v;
  const uint64_t a = (uint64_t)(uintptr_t)tab + 8ull * idx;     // (uniform, but not provably so: made so)
  const uint64_t at = ((uint64_t)uni((uint32_t)(a >> 32)) << 32) | uni((uint32_t)a);
  asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(at) : "memory");
  return v;
}

#endif
