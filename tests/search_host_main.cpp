// Stand-alone driver of csrc/bang_search_host.cpp for a sanitizer build: the host side of a search-kernel launch with everything around it stubbed --
// bang_set_error keeps the message, bang_num_cus answers argv[1], bang::env_str reads the environment, and the three instance dispatches
// (bang_search_launch_part0 / 2 / 4) print the SearchArgs they were handed instead of launching.
// stdin: one launch per line, "<entry> key=value ...": entry = search | inmem | wf | null (a null parameter block); every key a member of
// bang_search_params, `prio` the value of BANG_SEARCH_PRIO (- = unset).  Members not named keep the values of a plain self-paced launch
// (good()); pointers take made-up addresses -- nothing here dereferences one.
// stdout: one line per launch, "rc=<code> part=<dispatch reached, -1 = none> ... err=<message>".
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "bang_c.h"
#include "bang_search_args.h"

static int g_cus = 256, g_part = -1;
static char g_err[512];
static std::string g_args;

extern "C" void bang_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" int bang_num_cus(void) { return g_cus; }
namespace bang {
const char* env_str(const char* name) {
  const char* v = getenv(name);
  return (v && *v) ? v : nullptr;
}
}  // namespace bang

static int dispatched(int part, const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds) {
  char buf[512];
  snprintf(buf, sizeof buf, "grid=%u block=%u lds=%zu nctx=%u gs=%u wl_words=%u wave_words=%u lds_piv_floats=%u summ_iters=%u summ_iters_p=%u prio=%u spec_rows=%u cap_iter=%u",
           grid, block, lds, a->nctx, a->gs, a->wl_words, a->wave_words, a->lds_piv_floats, a->iter.summ_iters, a->p.summ_iters, a->iter.prio, a->p.spec_rows,
           a->iter.cap_iter);
  g_part = part;
  g_args = buf;
  return BANG_OK;
}
extern "C" int bang_search_launch_part0(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void*) { return dispatched(0, a, grid, block, lds); }
extern "C" int bang_search_launch_part2(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void*) { return dispatched(2, a, grid, block, lds); }
extern "C" int bang_search_launch_part4(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void*) { return dispatched(4, a, grid, block, lds); }

static bang_search_params good() {
  bang_search_params p;
  memset(&p, 0, sizeof p);
  p.Q = 100; p.R = 64; p.m = 70; p.L = 152; p.cap_iter = p.L + BANG_EXTRA_ITERS - 1; p.psz = 2; p.mp = 72;
  p.d_seed = (const uint32_t*)0x1000; p.d_codes = (const uint8_t*)0x2000; p.d_pivots_packed = (const float*)0x3000; p.d_qc = (const float*)0x4000;
  p.d_graph = (const uint8_t*)0x5000; p.entry_len = 128 + 4 + 4 * 64; p.vec_bytes = 128;
  p.d_bloom = (uint32_t*)0x6000; p.d_cand_ids = (uint32_t*)0x7000; p.d_cand_cnt = (uint32_t*)0x8000; p.d_next_query = (uint32_t*)0x9000;
  p.d_rows = (const uint32_t*)0xA000; p.d_ctl = (const uint32_t*)0xB000; p.h_done = (uint32_t*)0xC000; p.h_parents = (uint32_t*)0xD000;
  return p;
}

#define U32_KEYS(X) X(Q) X(R) X(m) X(L) X(cap_iter) X(psz) X(mp) X(pq_nhi) X(max_wgs) X(max_waves) X(row_layout) X(ship_vectors) X(nctx) X(group_waves) \
  X(code_stride) X(summ_iters) X(spec_rows) X(rr_dtype) X(rr_D) X(rr_k) X(rr_q0) X(rr_Q_total)
#define PTR_KEYS(X) X(d_seed) X(d_codes) X(d_pivots_packed) X(d_qc) X(d_graph) X(d_bloom) X(d_cand_ids) X(d_cand_cnt) X(d_next_query) X(d_rows) X(d_ctl) \
  X(h_done) X(h_parents) X(h_pub_q) X(h_pub_c) X(rr_queries) X(rr_vec_base) X(rr_ids_out) X(rr_dists_out)

static bool set_member(bang_search_params& p, const char* key, unsigned long long v) {
#define SET_U32(f) if (strcmp(key, #f) == 0) { p.f = (uint32_t)v; return true; }
  U32_KEYS(SET_U32)
#undef SET_U32
#define SET_PTR(f) if (strcmp(key, #f) == 0) { p.f = (decltype(p.f))(uintptr_t)v; return true; }
  PTR_KEYS(SET_PTR)
#undef SET_PTR
  if (strcmp(key, "rr_vec_stride") == 0) { p.rr_vec_stride = v; return true; }
  return false;
}

int main(int argc, char** argv) {
  if (argc > 1) g_cus = atoi(argv[1]);
  char line[2048];
  while (fgets(line, sizeof line, stdin)) {
    bang_search_params p = good();
    char* save = nullptr;
    const char* entry = strtok_r(line, " \n", &save);
    if (!entry) continue;
    unsetenv("BANG_SEARCH_PRIO");
    for (char* tok = strtok_r(nullptr, " \n", &save); tok; tok = strtok_r(nullptr, " \n", &save)) {
      char* eq = strchr(tok, '=');
      if (!eq) { printf("FAILED: no value in %s\n", tok); return 1; }
      *eq = 0;
      if (strcmp(tok, "prio") == 0) { if (strcmp(eq + 1, "-") != 0) setenv("BANG_SEARCH_PRIO", eq + 1, 1); continue; }
      if (!set_member(p, tok, strtoull(eq + 1, nullptr, 0))) { printf("FAILED: no member %s\n", tok); return 1; }
    }
    g_part = -1;
    g_err[0] = 0;
    g_args.clear();
    const bang_search_params* arg = strcmp(entry, "null") == 0 ? nullptr : &p;
    int rc;
    if (strcmp(entry, "inmem") == 0) rc = bang_k_search_inmem(arg, nullptr);
    else if (strcmp(entry, "wf") == 0) rc = bang_k_search_wf(arg, nullptr);
    else rc = bang_k_search(arg, nullptr);
    printf("rc=%d part=%d %s err=%s\n", rc, g_part, g_args.c_str(), g_err);
  }
  return 0;
}
