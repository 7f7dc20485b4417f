// bang_pad_rows.h -- adjacency rows in the bytes of the PQ code table that no kernel interprets (pull mode, option rows_pad): ONE definition of
// where they are, for the load (bang_load.cpp, bang_pad_rows.hip), the search kernel's hand-over (bang_search.hip), the argument check
// (bang_search_host.cpp) and the layout test (tests/pad_rows_layout_main.cpp).  Compiles as host C++ and as HIP.  Not public.
//
// A code line is code_stride bytes; an instance of NDW code dwords interprets its first 4 NDW bytes (the chunks m .. 4 NDW - 1 are padding chunks: their
// pivot entries are zero, whatever the byte).  pq_row_load / CoopFetch LOAD 16 * ceil((NDW [+ 1 where m % 4 != 0]) / 4) bytes from the line's start --
// 80 for the 70- and 74-chunk rows -- but where lines start dword-aligned (code_stride % 4 == 0, demanded here) the funnel shift is by 0 bytes and
// every dword behind the NDW-th is dropped unread (v_alignbyte(w[k + 1], w[k], 0) == w[k]): what those loads bring along is never code.
// The bytes [pad_off, code_stride) of a line therefore hold `slots` ids, and lines_per_row consecutive lines hold one 64-id row; padded row r
// lives in the lines [r * lines_per_row, (r + 1) * lines_per_row), which are lines of the table for every r < N / lines_per_row.
#ifndef BANG_PAD_ROWS_H_
#define BANG_PAD_ROWS_H_

#include <stdint.h>

#include "bang_search_args.h"

struct BangPadRowsLayout {
  uint32_t pad_off;          // first byte of a code line that no kernel interprets as code (multiple of 4)
  uint32_t slots;            // ids a line's padding holds
  uint32_t lines_per_row;    // consecutive lines that hold one 64-id row
  uint32_t usable;           // 1: slots >= 8 and lines_per_row <= 8
};

// code dwords of the narrowest compiled layout that holds m chunks (0: none does).  An engine whose layout is wider than that (1-dim chunks in a
// 24-dword instance) interprets more of the line: bang_load compares its own mp against pad_off before it fills the padding.
BANG_HD constexpr uint32_t bang_pad_rows_ndw(uint32_t m) {
  uint32_t best = 0;
#define X(PSZ, NDW) if (4u * (NDW) >= m && (best == 0 || (uint32_t)(NDW) < best)) best = (NDW);
  BANG_PQ_LAYOUTS(X)
#undef X
  return best;
}

BANG_HD constexpr BangPadRowsLayout bang_pad_rows_layout(uint32_t code_stride, uint32_t m) {
  BangPadRowsLayout l = {0, 0, 0, 0};
  const uint32_t ndw = bang_pad_rows_ndw(m);
  if (m == 0 || ndw == 0 || (code_stride & 3u) != 0) return l;
  l.pad_off = 4u * ndw;
  if (code_stride <= l.pad_off) return l;
  l.slots = (code_stride - l.pad_off) / 4u;
  l.lines_per_row = (64u + l.slots - 1u) / l.slots;
  l.usable = (l.slots >= 8u && l.lines_per_row <= 8u) ? 1u : 0u;
  return l;
}

// padded rows are the nodes [0, n_pad): every line such a row touches is a line of the N-line table
BANG_HD constexpr uint32_t bang_pad_rows_count(const BangPadRowsLayout& l, uint32_t n_nodes) { return l.usable ? n_nodes / l.lines_per_row : 0u; }

// byte offset into the code table of id `slot` (< 64) of padded row `row`, 64-bit throughout (row * lines_per_row * code_stride passes 2^32 at
// row = 6.7 M of a 128-byte table)
BANG_HD constexpr uint64_t bang_pad_row_byte(const BangPadRowsLayout& l, uint32_t code_stride, uint32_t row, uint32_t slot) {
  return ((uint64_t)row * l.lines_per_row + slot / l.slots) * (uint64_t)code_stride + l.pad_off + 4u * (slot % l.slots);
}

#endif
