// bang_pad_rows.hip -- fills the padding of the PQ code table with adjacency rows (pull mode, option rows_pad; layout: bang_pad_rows.h).
//
// pad_rows_scatter_kernel (bang_k_pad_rows_scatter): a chunk of staged 256-byte rows, [n_rows][64] ids in HBM, goes into the code lines of the
// padded rows [row0, row0 + n_rows).  One thread per padding slot: thread t of a row writes slot t % slots of the row's line t / slots -- id
// number t of the row, or 0xFFFFFFFF (BANG_ADJ_PAD) in the slots of the last line behind the 64th id, which nobody reads.  Plain dword stores
// through vector registers; adjacent threads write adjacent dwords of one line.  The host entry checks that the last line written is a line of
// the table before anything is launched.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_pad_rows.h"

struct PadScatterArgs {
  uint8_t* codes;                    // [n_lines][code_stride]
  const uint32_t* rows;              // [n_rows][64] staged rows
  uint32_t code_stride, row0, n_rows;
  BangPadRowsLayout l;
};

__global__ __launch_bounds__(256) void pad_rows_scatter_kernel(const PadScatterArgs a) {
  const uint32_t per_row = a.l.slots * a.l.lines_per_row;                       // padding slots of a row (>= 64)
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint64_t)a.n_rows * per_row) return;
  const uint32_t r = (uint32_t)(i / per_row), t = (uint32_t)(i % per_row);
  const uint32_t v = t < 64u ? a.rows[(uint64_t)r * 64u + t] : 0xFFFFFFFFu;
  const uint64_t line = (uint64_t)(a.row0 + r) * a.l.lines_per_row + t / a.l.slots;
  *(uint32_t*)(a.codes + line * a.code_stride + a.l.pad_off + 4u * (t % a.l.slots)) = v;
}

extern "C" int bang_k_pad_rows_scatter(uint8_t* d_codes, uint64_t n_lines, uint32_t code_stride, uint32_t m, const uint32_t* d_rows, uint32_t row0,
                                       uint32_t n_rows, void* stream) {
  if (!d_codes || !d_rows) { bang_set_error("bang_k_pad_rows_scatter: null buffer"); return BANG_ERR_ARG; }
  const BangPadRowsLayout l = bang_pad_rows_layout(code_stride, m);
  if (!l.usable) { bang_set_error("bang_k_pad_rows_scatter: code_stride = %u leaves no usable padding behind %u chunks", code_stride, m); return BANG_ERR_ARG; }
  if (((uintptr_t)d_codes & 3u) != 0 || ((uintptr_t)d_rows & 3u) != 0) { bang_set_error("bang_k_pad_rows_scatter: buffers must be 4-byte aligned"); return BANG_ERR_ARG; }
  // the last line written, (row0 + n_rows) * lines_per_row - 1, is a line of the table
  if (((uint64_t)row0 + n_rows) * l.lines_per_row > n_lines) {
    bang_set_error("bang_k_pad_rows_scatter: rows [%u, +%u) need %llu code lines, the table has %llu", row0, n_rows,
                   (unsigned long long)(((uint64_t)row0 + n_rows) * l.lines_per_row), (unsigned long long)n_lines);
    return BANG_ERR_ARG;
  }
  if (n_rows == 0) return BANG_OK;
  PadScatterArgs a;
  a.codes = d_codes; a.rows = d_rows; a.code_stride = code_stride; a.row0 = row0; a.n_rows = n_rows; a.l = l;
  const uint64_t threads = (uint64_t)n_rows * l.slots * l.lines_per_row;
  const uint64_t blocks = (threads + 255u) / 256u;
  if (blocks > 0x7FFFFFFFull) { bang_set_error("bang_k_pad_rows_scatter: %u rows are too many for one launch", n_rows); return BANG_ERR_ARG; }
  hipLaunchKernelGGL(pad_rows_scatter_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
