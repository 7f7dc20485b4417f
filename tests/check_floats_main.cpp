// check_floats_main.cpp -- the cases of tests/test_float_range_inputs.py::test_check_through_ctypes in C, for a build of csrc/bang_check.cpp under
// -fsanitize=address,undefined (tests/test_float_range_inputs.py::test_check_under_sanitizers compiles the two files and runs the program: host
// code only, no Python in the sanitized process).  Every buffer is heap-allocated to exactly n floats, so a read past the end of a vector tail is a
// heap-buffer-overflow report and a non-zero exit.  Prints "ok <cases>" and returns 0, or the first failing case and 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bang_c.h"

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static long g_cases = 0;

static int expect(const float* x, uint64_t n, int rc_want, uint64_t bad_want, const char* what, uint64_t a, uint64_t b) {
  uint64_t bad = 0xDEADBEEFull;
  const int rc = bang_check_floats(x, n, &bad);
  ++g_cases;
  if (rc != rc_want || (rc_want != BANG_OK && bad != bad_want) || (rc_want == BANG_OK && bad != 0xDEADBEEFull)) {
    fprintf(stderr, "FAIL %s (n = %llu, case %llu/%llu): rc %d (want %d), first_bad %llu (want %llu)\n", what, (unsigned long long)n,
            (unsigned long long)a, (unsigned long long)b, rc, rc_want, (unsigned long long)bad, (unsigned long long)bad_want);
    return 1;
  }
  return 0;
}

int main(void) {
  const float two56 = ldexpf(1.0f, 56);
  const float refused[] = {from_bits(0x7FC00000u), from_bits(0xFFC00000u), from_bits(0x7F800001u), from_bits(0xFFFFFFFFu), from_bits(0x7FA5A5A5u),
                           INFINITY, -INFINITY, nextafterf(two56, INFINITY), -nextafterf(two56, INFINITY), ldexpf(1.0f, 57), 3.402823e38f};
  const float accepted[] = {two56, -two56, from_bits(0x00000001u), from_bits(0x807FFFFFu), from_bits(0x00400000u), 0.0f, -0.0f, 1.0f, -128.0f,
                            nextafterf(two56, 0.0f)};
  const int n_ref = (int)(sizeof(refused) / sizeof(refused[0])), n_acc = (int)(sizeof(accepted) / sizeof(accepted[0]));
  // n = 0: accepted, with a null pointer too
  if (expect(NULL, 0, BANG_OK, 0, "n = 0, null", 0, 0)) return 1;
  for (uint64_t n = 1; n <= 67 + 3; ++n) {
    const uint64_t len = n <= 67 ? n : (n == 68 ? 1024 : n == 69 ? 1025 : 4099);            // ... and the block edge of the two-pass loop
    float* x = (float*)malloc(len * sizeof(float));
    if (!x) return 2;
    for (int a = 0; a < n_acc; ++a) {                                                        // accepted values everywhere
      for (uint64_t i = 0; i < len; ++i) x[i] = accepted[(a + i) % n_acc];
      if (expect(x, len, BANG_OK, 0, "accepted", a, 0)) return 1;
    }
    const uint64_t at[3] = {0, len / 2, len - 1};
    for (int r = 0; r < n_ref; ++r)
      for (int p = 0; p < 3; ++p) {
        for (uint64_t i = 0; i < len; ++i) x[i] = accepted[i % n_acc];
        x[at[p]] = refused[r];
        if (expect(x, len, BANG_ERR_ARG, at[p], "one offender", r, p)) return 1;
        x[len - 1] = refused[(r + 1) % n_ref];                                               // a second one behind it: the FIRST is reported
        if (expect(x, len, BANG_ERR_ARG, at[p] < len - 1 ? at[p] : len - 1, "two offenders", r, p)) return 1;
      }
    free(x);
  }
  {                                                                                          // first_bad may be NULL
    float* x = (float*)malloc(5 * sizeof(float));
    if (!x) return 2;
    for (int i = 0; i < 5; ++i) x[i] = 1.0f;
    if (bang_check_floats(x, 5, NULL) != BANG_OK) { fprintf(stderr, "FAIL null first_bad, clean\n"); return 1; }
    x[4] = NAN;
    if (bang_check_floats(x, 5, NULL) != BANG_ERR_ARG) { fprintf(stderr, "FAIL null first_bad, NaN\n"); return 1; }
    free(x);
  }
  printf("ok %ld\n", g_cases);
  return 0;
}
