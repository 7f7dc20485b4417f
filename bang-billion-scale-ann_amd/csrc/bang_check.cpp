// bang_check.cpp -- the input domain of float data (CANON 20), checked on the host in front of every launch.  No HIP call
// and nothing of the engine in it: it loads and runs on a machine without a GPU, and builds alone under a sanitizer.
#include <stdint.h>
#include <string.h>

#include "bang_c.h"

// |x| <= 2^56, finite: with the sign bit cleared the float's bits compare as unsigned integers in the order of the magnitudes, 2^56 is
// 0x5B800000, and every larger finite value, +-inf (0x7F800000) and every NaN (above it, whatever the payload) lie beyond it.
#define BANG_FLOAT_DOMAIN_MAX_BITS 0x5B800000u

static inline uint32_t outside(const float* p) {
  uint32_t b;
  memcpy(&b, p, sizeof(b));
  return (uint32_t)((b & 0x7FFFFFFFu) > BANG_FLOAT_DOMAIN_MAX_BITS);
}

// One pass in blocks: the block loop has no exit and no dependence but an OR, so the compiler vectorises it (8 floats per AVX2 compare); only a
// block that holds an offender is walked a second time for its index.
extern "C" int bang_check_floats(const float* x, uint64_t n, uint64_t* first_bad) {
  if (n == 0) return BANG_OK;
  if (!x) { if (first_bad) *first_bad = 0; return BANG_ERR_ARG; }
  const uint64_t BLOCK = 1024;
  for (uint64_t i = 0; i < n; i += BLOCK) {
    const uint64_t len = n - i < BLOCK ? n - i : BLOCK;
    const float* p = x + i;
    uint32_t any = 0;
    for (uint64_t j = 0; j < len; ++j) any |= outside(p + j);
    if (any) {
      for (uint64_t j = 0; j < len; ++j)
        if (outside(p + j)) {
          if (first_bad) *first_bad = i + j;
          return BANG_ERR_ARG;
        }
    }
  }
  return BANG_OK;
}
