// bang_f16.h -- float -> IEEE fp16 as integer arithmetic on the bits: the rounding of option vectors_fp16 (f32_to_f16_kernel, bang_kernels.hip).
// Plain C++: compiled for the device by hipcc and for the HOST by tests/test_f16_convert_host.py, which compares it with numpy's conversion.
#ifndef BANG_F16_H_
#define BANG_F16_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define BANG_F16_FN __host__ __device__ __forceinline__
#else
#define BANG_F16_FN static inline
#endif

// float bits -> IEEE fp16 bits, round to nearest even, subnormals produced; integer arithmetic only (independent of the wave's rounding and
// denormal modes).  NaN keeps the top of its payload and stays a NaN; *overflow: a finite value became +-inf.
BANG_F16_FN uint32_t f32_to_f16_bits(uint32_t x, bool* overflow) {
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
  *overflow = false;
  if (a >= 0x7F800000u) {                                   // inf / NaN
    if (a == 0x7F800000u) return sign | 0x7C00u;
    uint32_t h = 0x7C00u + ((a & 0x007FFFFFu) >> 13);
    if (h == 0x7C00u) ++h;
    return sign | h;
  }
  if (a >= 0x477FF000u) { *overflow = true; return sign | 0x7C00u; }      // |x| >= 65520: rounds past the largest half (65504)
  if (a >= 0x38800000u) return sign | ((a - 0x38000000u + 0xFFFu + ((a >> 13) & 1u)) >> 13);      // normal halves (a carry moves into the exponent)
  if (a <= 0x33000000u) return sign;                        // |x| <= 2^-25: zero (2^-25 itself is the tie between 0 and 2^-24: even)
  const uint32_t sh = 126u - (a >> 23);                     // 14 .. 24: the half's unit is 2^-24
  const uint32_t mant = (a & 0x007FFFFFu) | 0x00800000u;
  uint32_t h = mant >> sh;
  const uint32_t rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  if (rem > half || (rem == half && (h & 1u))) ++h;         // (0x400: the smallest normal half)
  return sign | h;
}

#endif
