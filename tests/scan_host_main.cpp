// Stand-alone driver of csrc/bang_scan_host.cpp (no HIP call in it) for a sanitizer build: the geometry over a grid of shapes -- every stripe
// count it returns is one bang_scan_check accepts, the stripes cover [0, n_nodes) in whole rounds, stripes * k stays within BANG_SCAN_MAX_KEYS --,
// the scratch size, and every refusal of bang_scan_check with the member it names.  Prints "ok <cases>".
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bang_c.h"

static char g_err[1024];
extern "C" void bang_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static bang_scan_params good(int dtype, uint32_t D, uint32_t n, uint32_t nq, uint32_t k, uint32_t stripes) {
  bang_scan_params p;
  memset(&p, 0, sizeof(p));
  p.d_vec_base = (const uint8_t*)0x10000; p.vec_stride = (dtype == BANG_F32 ? 4ull * D : D) + 4 + 4 * 64; p.dtype = (uint32_t)dtype; p.D = D; p.n_nodes = n;
  p.d_queries = (const void*)0x20000; p.nq = nq; p.k = k; p.stripes = stripes;
  p.d_scratch = (void*)0x30000;
  uint32_t t = 0, s = stripes;
  if (s == 0) bang_scan_geometry(dtype, D, nq, n, k, &t, &s);
  p.scratch_bytes = bang_scan_scratch_bytes(nq, k, s);
  p.d_ids_out = (uint64_t*)0x40000; p.d_dists_out = (float*)0x50000; p.d_matched = (uint32_t*)0x60000;
  return p;
}

static int refused(const bang_scan_params& p, int code, const char* word) {
  g_err[0] = 0;
  const int rc = bang_scan_check(&p);
  if (rc != code || !strstr(g_err, word) || !strstr(g_err, "bang_k_scan")) { printf("FAILED: rc %d (want %d), message '%s' (want '%s')\n", rc, code, g_err, word); return 1; }
  return 0;
}

int main() {
  int cases = 0, bad = 0;
  const int dtypes[] = {BANG_U8, BANG_I8, BANG_F32};
  const uint32_t ns[] = {1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 640, 4000, 1000000, 0xFFFFFFFFu};
  const uint32_t nqs[] = {1, 15, 16, 17, 31, 32, 33, 130, 4096, 1u << 20};
  const uint32_t ks[] = {1, 10, 100, 128};
  for (int dt : dtypes)
    for (uint32_t n : ns)
      for (uint32_t nq : nqs)
        for (uint32_t k : ks) {
          const uint32_t D = dt == BANG_F32 ? 96u : 128u;
          const uint32_t qt = dt == BANG_F32 ? 16u : 32u, round = dt == BANG_F32 ? 256u : 128u;
          uint32_t tiles = 0, stripes = 0;
          if (bang_scan_geometry(dt, D, nq, n, k, &tiles, &stripes) != BANG_OK) { printf("FAILED geometry %d %u %u %u\n", dt, n, nq, k); return 1; }
          const uint32_t most = bang_scan_max_stripes(dt, n, k);
          bad |= tiles != (nq + qt - 1) / qt || stripes < 1 || stripes > most || (uint64_t)stripes * k > BANG_SCAN_MAX_KEYS || most < 1;
          bad |= (uint64_t)most > ((uint64_t)n + round - 1) / round;
          const uint64_t per = (((uint64_t)n + stripes - 1) / stripes + round - 1) / round * round;      // the launcher's stripe length
          bad |= per * stripes < n;
          if (nq <= 4096) {                                                // (what a launch takes: the engine's chunks)
            bang_scan_params p = good(dt, D, n, nq, k, 0);
            bad |= bang_scan_check(&p) != BANG_OK;
            p = good(dt, D, n, nq, k, most);
            bad |= bang_scan_check(&p) != BANG_OK;
            p = good(dt, D, n, nq, k, most + 1);
            bad |= bang_scan_check(&p) != BANG_ERR_ARG;
          }
          if (bad) { printf("FAILED dtype %d n %u nq %u k %u: tiles %u stripes %u most %u\n", dt, n, nq, k, tiles, stripes, most); return 1; }
          ++cases;
        }
  uint32_t t = 0, s = 0;
  bad |= bang_scan_geometry(BANG_U8, 128, 0, 10, 1, &t, &s) != BANG_ERR_ARG || bang_scan_geometry(BANG_U8, 128, 1, 0, 1, &t, &s) != BANG_ERR_ARG;
  bad |= bang_scan_geometry(BANG_U8, 128, 1, 10, 0, &t, &s) != BANG_ERR_ARG || bang_scan_geometry(BANG_U8, 128, 1, 10, 129, &t, &s) != BANG_ERR_ARG;
  bad |= bang_scan_geometry(BANG_U8, 128, 1, 10, 1, nullptr, &s) != BANG_ERR_ARG || bang_scan_geometry(BANG_U8, 128, 1, 10, 1, &t, nullptr) != BANG_ERR_ARG;
  bad |= bang_scan_geometry(BANG_U8, 48, 1, 10, 1, &t, &s) != BANG_ERR_UNSUPPORTED || bang_scan_geometry(BANG_F32, 260, 1, 10, 1, &t, &s) != BANG_ERR_UNSUPPORTED;
  bad |= bang_scan_geometry(3, 128, 1, 10, 1, &t, &s) != BANG_ERR_UNSUPPORTED;
  bad |= bang_scan_scratch_bytes(3, 10, 7) != 8ull * 3 * 70 + 24 || bang_scan_max_stripes(BANG_U8, 0, 1) != 0 || bang_scan_max_stripes(BANG_U8, 10, 0) != 0;
  if (bad) { printf("FAILED: geometry refusals\n"); return 1; }
  cases += 12;
  // bang_scan_check: every refusal names its member
  g_err[0] = 0;
  if (bang_scan_check(nullptr) != BANG_ERR_ARG || !strstr(g_err, "null")) { printf("FAILED: null block\n"); return 1; }
  bang_scan_params p;
#define REFUSED(edit, code, word) do { p = good(BANG_U8, 128, 4000, 64, 10, 2); edit; if (refused(p, code, word)) return 1; ++cases; } while (0)
  REFUSED(p.d_vec_base = nullptr, BANG_ERR_ARG, "d_vec_base");
  REFUSED(p.d_vec_base = (const uint8_t*)0x10002, BANG_ERR_ARG, "d_vec_base");
  REFUSED(p.d_queries = nullptr, BANG_ERR_ARG, "d_queries");
  REFUSED(p.n_nodes = 0, BANG_ERR_ARG, "n_nodes");
  REFUSED(p.nq = 0, BANG_ERR_ARG, "nq = 0");
  REFUSED(p.nq = (1u << 20) + 1, BANG_ERR_ARG, "nq");
  REFUSED(p.k = 0, BANG_ERR_ARG, "k = 0");
  REFUSED(p.k = 129, BANG_ERR_ARG, "k = 129");
  REFUSED(p.D = 48, BANG_ERR_UNSUPPORTED, "layout");
  REFUSED(p.dtype = 3, BANG_ERR_UNSUPPORTED, "layout");
  REFUSED(p.vec_stride = 127, BANG_ERR_UNSUPPORTED, "layout");
  REFUSED(p.vec_stride = 64, BANG_ERR_UNSUPPORTED, "layout");
  REFUSED((p.dtype = BANG_F32, p.D = 260, p.vec_stride = 2000), BANG_ERR_UNSUPPORTED, "layout");
  REFUSED(p.d_labels = (const uint32_t*)0x70000, BANG_ERR_ARG, "d_labels");
  REFUSED(p.d_filters = (const uint32_t*)0x70000, BANG_ERR_ARG, "d_filters");
  REFUSED(p.stripes = 33, BANG_ERR_ARG, "stripes");          // ceil(4000 / 128) = 32
  REFUSED((p.k = 128, p.stripes = 33), BANG_ERR_ARG, "stripes");
  REFUSED(p.d_scratch = nullptr, BANG_ERR_ARG, "d_scratch");
  REFUSED(p.d_scratch = (void*)0x30004, BANG_ERR_ARG, "d_scratch");
  REFUSED(p.scratch_bytes -= 1, BANG_ERR_ARG, "scratch_bytes");
  REFUSED(p.d_ids_out = nullptr, BANG_ERR_ARG, "d_ids_out");
  REFUSED(p.d_dists_out = nullptr, BANG_ERR_ARG, "d_dists_out");
  REFUSED(p.d_matched = nullptr, BANG_ERR_ARG, "d_matched");
  printf("ok %d\n", cases);
  return 0;
}
