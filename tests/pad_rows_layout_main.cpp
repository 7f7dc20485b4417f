// Stand-alone check of csrc/bang_pad_rows.h (adjacency rows in the code table's padding, option rows_pad) and of what csrc/bang_search_host.cpp makes
// of bang_search_params.n_rows_pad, for a plain and a sanitizer build (make pad_rows_layout_test).  No device, no HIP call: bang_set_error keeps the
// message, bang_num_cus answers 256 and the instance dispatch keeps the SearchArgs it was handed.
//  1. the layout of every (code_stride, m) of interest: pad_off, slots, lines_per_row, usable;
//  2. for N in {1, 4, 5, 6, 1003} and every (row < n_pad, slot < 64): the id's four bytes lie inside the N * code_stride bytes of the table, at or
//     behind pad_off within their line, dword-aligned, and no two (row, slot) share an offset; every line a padded row touches is its own;
//  3. bang_pad_row_byte(2^23, 63) is the exact 64-bit value, above 2^32;
//  4. a launch with n_rows_pad: accepted where the kernel reads padded rows (and n_pad reaches IterArgs), refused with the member's name elsewhere.
// Prints "ok <checks>" and returns 0, or the first failure and 1.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "bang_c.h"
#include "bang_pad_rows.h"
#include "bang_search_args.h"

static char g_err[512];
static SearchArgs g_args;
static int g_part = -1;
static long g_checks = 0;

extern "C" void bang_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
extern "C" int bang_num_cus(void) { return 256; }
namespace bang {
const char* env_str(const char*) { return nullptr; }
}  // namespace bang
static int dispatched(int part, const SearchArgs* a) { g_part = part; g_args = *a; return BANG_OK; }
extern "C" int bang_search_launch_part0(const SearchArgs* a, uint32_t, uint32_t, size_t, void*) { return dispatched(0, a); }
extern "C" int bang_search_launch_part2(const SearchArgs* a, uint32_t, uint32_t, size_t, void*) { return dispatched(2, a); }
extern "C" int bang_search_launch_part4(const SearchArgs* a, uint32_t, uint32_t, size_t, void*) { return dispatched(4, a); }

#define CHECK(c, ...) do { ++g_checks; if (!(c)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

struct Want { uint32_t stride, m, pad_off, slots, lines, usable; };
// 70 and 65 chunks are read as 18 code dwords (72 bytes), 74 as 19 (76); 32 chunks fill their 32-byte line
static const Want kLayouts[] = {{128, 70, 72, 14, 5, 1}, {128, 74, 76, 13, 5, 1}, {128, 65, 72, 14, 5, 1}, {32, 32, 0, 0, 0, 0}, {256, 70, 72, 46, 2, 1}};

static int check_layouts() {
  for (const Want& w : kLayouts) {
    const BangPadRowsLayout l = bang_pad_rows_layout(w.stride, w.m);
    CHECK(l.usable == w.usable, "stride %u m %u: usable %u", w.stride, w.m, l.usable);
    if (!w.usable) {
      for (uint32_t N : {1u, 5u, 1003u}) CHECK(bang_pad_rows_count(l, N) == 0, "unusable layout holds rows");
      continue;
    }
    CHECK(l.pad_off == w.pad_off && l.slots == w.slots && l.lines_per_row == w.lines, "stride %u m %u: pad_off %u slots %u lines %u", w.stride, w.m, l.pad_off,
          l.slots, l.lines_per_row);
    CHECK(l.pad_off >= w.m && l.pad_off % 4 == 0 && l.pad_off >= 4 * bang_pad_rows_ndw(w.m), "pad_off %u covers the code", l.pad_off);
    CHECK(l.slots >= 8 && l.lines_per_row <= 8 && l.slots * l.lines_per_row >= 64 && l.slots * (l.lines_per_row - 1) < 64, "slots and lines");
    for (uint32_t N : {1u, 4u, 5u, 6u, 1003u}) {
      const uint32_t n_pad = bang_pad_rows_count(l, N);
      CHECK(n_pad == N / l.lines_per_row && n_pad <= N, "N %u: n_pad %u", N, n_pad);
      const uint64_t bytes = (uint64_t)N * w.stride;
      std::set<uint64_t> seen;
      for (uint32_t row = 0; row < n_pad; ++row)
        for (uint32_t slot = 0; slot < 64; ++slot) {
          const uint64_t b = bang_pad_row_byte(l, w.stride, row, slot);
          CHECK(b + 4 <= bytes, "N %u row %u slot %u: byte %llu of %llu", N, row, slot, (unsigned long long)b, (unsigned long long)bytes);
          CHECK(b % 4 == 0 && b % w.stride >= l.pad_off && b % w.stride + 4 <= w.stride, "N %u row %u slot %u: byte %llu in its line", N, row, slot, (unsigned long long)b);
          const uint64_t line = b / w.stride;
          CHECK(line >= (uint64_t)row * l.lines_per_row && line < (uint64_t)(row + 1) * l.lines_per_row, "row %u slot %u: line %llu is another row's", row, slot, (unsigned long long)line);
          CHECK(seen.insert(b).second, "N %u row %u slot %u: offset %llu taken twice", N, row, slot, (unsigned long long)b);
        }
      CHECK(seen.size() == (size_t)n_pad * 64, "N %u: %zu offsets", N, seen.size());
    }
  }
  if (bang_pad_rows_count(bang_pad_rows_layout(128, 70), 1003) != 200) { printf("FAILED: n_pad of N = 1003 is not 200\n"); return 1; }
  // 64-bit: row 2^23, slot 63 = line 2^23 * 5 + 4, byte 72 + 4 * (63 - 56) of it
  const BangPadRowsLayout l = bang_pad_rows_layout(128, 70);
  const uint64_t b = bang_pad_row_byte(l, 128, 1u << 23, 63);
  CHECK(b == ((5ull << 23) + 4ull) * 128ull + 72ull + 28ull && b == 5368709732ull && b > (1ull << 32), "row 2^23 slot 63: byte %llu", (unsigned long long)b);
  // the first row whose offset passes 2^32 (6 710 887) and the last row of a 10^9-node table
  CHECK(bang_pad_row_byte(l, 128, 6710887u, 0) == 6710887ull * 640ull + 72ull && bang_pad_row_byte(l, 128, 6710887u, 0) > (1ull << 32), "row 6 710 887");
  CHECK(bang_pad_row_byte(l, 128, 199999999u, 63) + 4 <= 1000000000ull * 128ull, "last padded row of 10^9 nodes");
  // the kernel's split of the offset: uniform part row * lines_per_row * stride, lane part bang_pad_row_byte(l, stride, 0, slot) < 2^32
  for (uint32_t slot = 0; slot < 64; ++slot)
    CHECK(bang_pad_row_byte(l, 128, 12345678u, slot) == 12345678ull * (l.lines_per_row * 128ull) + bang_pad_row_byte(l, 128, 0, slot), "split at slot %u", slot);
  return 0;
}

static bang_search_params good() {
  bang_search_params p;
  memset(&p, 0, sizeof p);
  p.Q = 100; p.R = 64; p.m = 70; p.L = 152; p.cap_iter = p.L + BANG_EXTRA_ITERS - 1; p.psz = 2; p.mp = 72; p.pq_nhi = 58; p.code_stride = 128;
  p.d_seed = (const uint32_t*)0x1000; p.d_codes = (const uint8_t*)0x2000; p.d_pivots_packed = (const float*)0x3000; p.d_qc = (const float*)0x4000;
  p.d_graph = (const uint8_t*)0x5000; p.entry_len = 256; p.row_layout = 1; p.n_nodes = 1003; p.n_rows_pad = 200;
  p.d_bloom = (uint32_t*)0x6000; p.d_cand_ids = (uint32_t*)0x7000; p.d_cand_cnt = (uint32_t*)0x8000; p.d_next_query = (uint32_t*)0x9000;
  p.d_rows = (const uint32_t*)0xA000; p.d_ctl = (const uint32_t*)0xB000; p.h_done = (uint32_t*)0xC000; p.h_parents = (uint32_t*)0xD000;
  return p;
}

static int launch(int entry, const bang_search_params& p) {
  g_part = -1; g_err[0] = 0; memset(&g_args, 0, sizeof g_args);
  return entry == 2 ? bang_k_search_inmem(&p, nullptr) : entry == 4 ? bang_k_search_wf(&p, nullptr) : bang_k_search(&p, nullptr);
}

static int check_launches() {
  bang_search_params p = good();
  for (int entry : {0, 4}) {                       // bang_k_search and bang_k_search_wf read padded rows
    CHECK(launch(entry, p) == BANG_OK && g_part == entry, "entry %d: %s", entry, g_err);
    CHECK(g_args.iter.n_pad == 200 && ((const uint32_t*)&g_args.iter)[IA_N_PAD] == 200 && g_args.iter.d_codes == p.d_codes, "n_pad in IterArgs: %u", g_args.iter.n_pad);
  }
  p = good(); p.n_rows_pad = 0;
  CHECK(launch(0, p) == BANG_OK && g_args.iter.n_pad == 0, "without padded rows: %s", g_err);
  p = good(); p.n_rows_hbm = 256; p.d_rows_hbm = (const uint32_t*)0xE000;
  CHECK(launch(0, p) == BANG_OK && g_args.iter.n_pad == 200 && g_args.iter.n_rows_hbm == 256, "padded rows and the copy: %s", g_err);
  p = good(); p.n_rows_pad = 201;                  // row 200 would end in line 1004 of 1003
  CHECK(launch(0, p) == BANG_ERR_ARG && g_part == -1 && strstr(g_err, "n_rows_pad"), "n_rows_pad = 201: %s", g_err);
  p = good(); p.n_nodes = 0;
  CHECK(launch(0, p) == BANG_ERR_ARG && g_part == -1 && strstr(g_err, "n_rows_pad"), "n_nodes = 0: %s", g_err);
  struct { const char* what; void (*change)(bang_search_params&); int entry; } refused[] = {
      {"host-paced", [](bang_search_params& q) { q.d_graph = nullptr; }, 0},
      {"graph entries", [](bang_search_params& q) { q.row_layout = 0; }, 0},
      {"peer rows", [](bang_search_params& q) { q.n_slices = 2; q.slice_rows = 512; q.d_row_slices = (const uint64_t*)0xF000; }, 0},
      {"74 chunks", [](bang_search_params& q) { q.m = 74; q.mp = 76; q.pq_nhi = 22; }, 0},
      {"32 chunks", [](bang_search_params& q) { q.m = 32; q.mp = 32; q.psz = 4; q.pq_nhi = 0; q.code_stride = 32; }, 0},
      {"32 chunks, 128 apart", [](bang_search_params& q) { q.m = 32; q.mp = 32; q.psz = 4; q.pq_nhi = 0; }, 0},
      {"packed rows", [](bang_search_params& q) { q.code_stride = 0; }, 0},
      {"stride 256", [](bang_search_params& q) { q.code_stride = 256; }, 0},
      {"word filter, 74 chunks", [](bang_search_params& q) { q.m = 74; q.mp = 76; q.pq_nhi = 22; }, 4},
  };
  for (auto& r : refused) {
    p = good();
    r.change(p);
    CHECK(launch(r.entry, p) == BANG_ERR_ARG && g_part == -1 && strstr(g_err, "n_rows_pad") && strstr(g_err, "rows_pad"), "%s: rc / message %s", r.what, g_err);
    p.n_rows_pad = 0;                               // ... and the same launch without padded rows is no concern of the check
    const int rc = launch(r.entry, p);
    CHECK(!strstr(g_err, "n_rows_pad") && (rc == BANG_OK) == (g_part >= 0), "%s without padded rows: %s", r.what, g_err);
  }
  p = good(); p.row_layout = 0; p.entry_len = 388; p.vec_bytes = 128;      // semantics = 1 reads graph entries: refused either way, padded rows named first
  CHECK(launch(2, p) != BANG_OK && g_part == -1, "inmem with padded rows: %s", g_err);
  return 0;
}

int main() {
  static_assert(bang_pad_rows_layout(128, 72).pad_off == 72 && bang_pad_rows_layout(128, 72).lines_per_row == 5, "the search kernel's layout is a constant expression");
  static_assert(search_has_pad_rows(18, false) && !search_has_pad_rows(18, true) && !search_has_pad_rows(19, false) && !search_has_pad_rows(8, false), "instances with the padded branch");
  if (check_layouts() || check_launches()) return 1;
  printf("ok %ld\n", g_checks);
  return 0;
}
