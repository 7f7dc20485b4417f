// bang_reuse.hip -- the device side of re-using the ids of removed nodes (DESIGN.md section 2 CANON 24, section 4.18; engine: bang_insert_reuse_e,
// bang_set_removed_e, bang_get_removed_e in bang_reuse_host.cpp).
//
//  * bang_k_bitmap_select: the lowest `want` set bit positions of a & ~not below n_bits, ascending, and the number of all such bits.  Three
//    launches: select_count_kernel (one workgroup per SPAN of 1024 words: the popcount of its span), select_scan_kernel (ONE workgroup: the
//    exclusive prefix of the span counts, in place, and the total) and select_emit_kernel (a workgroup whose prefix is below `want` ranks its
//    lanes' words -- a wave prefix over the lanes' popcounts, the waves' sums through LDS -- and stores position prefix + rank).  No atomic: the
//    place of every id is a function of the bitmap alone.
//  * bang_k_copy_rows_by_id: one wave per row between row ids[i] of a strided table and row i of a packed buffer; 16-byte pieces, then dwords, then
//    bytes, as far as the alignment of both sides allows (decided on the host, uniform for the launch).
//  * bang_k_bitmap_set_ids / bang_k_bitmap_clear_ids: an atomic OR / AND per id.
//  * bang_k_rows_check: is every listed id a node, not the medoid, with an empty row?  The lowest list position that is not, by an atomic minimum.
//
// All addressing is 64-bit; every access to HBM goes through a global-address-space pointer (GAS); every store is a vector store; no kernel keeps
// anything in scratch.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"

#define SEL_THREADS 256u
#define SEL_WORDS 4u                                       // bitmap words per lane
#define SEL_SPAN (SEL_THREADS * SEL_WORDS)                 // words per workgroup: BANG_SELECT_SPAN_BITS / 32
static_assert(SEL_SPAN * 32u == BANG_SELECT_SPAN_BITS, "bang_c.h names the span of a workgroup");
#define RU_WAVES 4u                                        // waves per workgroup of the row kernels
#define RU_MAX_WGS 4096u                                   // workgroups of a copy launch at most: the waves stride over the rows

struct SelArgs {
  const uint32_t* a;                 // [ceil(n_bits / 32)]
  const uint32_t* nt;                // the same shape, or NULL
  uint32_t* counts;                  // [spans]: the spans' popcounts, then their exclusive prefix
  uint32_t* ids_out;                 // [min(want, total)]
  uint32_t* total;                   // [1]
  uint64_t n_words;
  uint32_t n_bits, want, spans;
};

// the lane's SEL_WORDS words of a & ~not, bits at or behind n_bits and words behind the bitmap read as 0; -> their popcount
__device__ __forceinline__ uint32_t sel_load(const SelArgs& a, uint64_t w0, uint32_t w[SEL_WORDS]) {
  const uint32_t GAS* bm = (const uint32_t GAS*)a.a;
  const uint32_t GAS* nt = (const uint32_t GAS*)a.nt;
  uint32_t c = 0;
#pragma unroll
  for (uint32_t j = 0; j < SEL_WORDS; ++j) {
    const uint64_t wi = w0 + j;
    uint32_t v = 0u;
    if (wi < a.n_words) {
      v = bm[wi];
      if (nt) v &= ~nt[wi];                                            // (uniform)
      if (wi == a.n_words - 1u && (a.n_bits & 31u) != 0u) v &= (1u << (a.n_bits & 31u)) - 1u;
    }
    w[j] = v;
    c += (uint32_t)__popc(v);
  }
  return c;
}

__global__ __launch_bounds__(256) void select_count_kernel(const SelArgs a) {
  __shared__ uint32_t wsum[SEL_THREADS / WAVE];
  uint32_t w[SEL_WORDS];
  uint32_t c = sel_load(a, (uint64_t)blockIdx.x * SEL_SPAN + (uint64_t)threadIdx.x * SEL_WORDS, w);
  for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) ((uint32_t GAS*)a.counts)[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ONE workgroup: thread t owns the spans [t * per, (t + 1) * per)
__global__ __launch_bounds__(256) void select_scan_kernel(const SelArgs a) {
  __shared__ uint32_t part[SEL_THREADS];
  uint32_t GAS* counts = (uint32_t GAS*)a.counts;
  const uint32_t per = (a.spans + SEL_THREADS - 1u) / SEL_THREADS;
  const uint32_t b0 = threadIdx.x * per < a.spans ? threadIdx.x * per : a.spans;
  const uint32_t b1 = b0 + per < a.spans ? b0 + per : a.spans;
  uint32_t s = 0;
  for (uint32_t b = b0; b < b1; ++b) s += counts[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (uint32_t i = 0; i < SEL_THREADS; ++i) { const uint32_t t = part[i]; part[i] = run; run += t; }
    *(uint32_t GAS*)a.total = run;                                     // (<= n_bits <= 2^32 - 2)
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (uint32_t b = b0; b < b1; ++b) { const uint32_t c = counts[b]; counts[b] = run; run += c; }
}

__global__ __launch_bounds__(256) void select_emit_kernel(const SelArgs a) {
  __shared__ uint32_t wsum[SEL_THREADS / WAVE];
  const uint32_t prefix = ((const uint32_t GAS*)a.counts)[blockIdx.x];
  if (prefix >= a.want) return;                                        // (uniform per workgroup, in front of the barrier)
  const int lane = lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint64_t w0 = (uint64_t)blockIdx.x * SEL_SPAN + (uint64_t)threadIdx.x * SEL_WORDS;
  uint32_t w[SEL_WORDS];
  const uint32_t c = sel_load(a, w0, w);
  uint32_t inc = c;                                                    // the wave's inclusive prefix of the lanes' counts
  for (int off = 1; off < WAVE; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, off);
    if (lane >= off) inc += t;
  }
  if (lane == WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  uint32_t at = prefix + inc - c;
  for (uint32_t v = 0; v < wave; ++v) at += wsum[v];
  uint32_t GAS* out = (uint32_t GAS*)a.ids_out;
#pragma unroll
  for (uint32_t j = 0; j < SEL_WORDS; ++j) {
    uint32_t word = w[j];
    const uint32_t first_bit = (uint32_t)((w0 + j) << 5);              // (< n_bits wherever word != 0)
    while (word != 0u) {
      const uint32_t b = (uint32_t)__builtin_ctz(word);
      word &= word - 1u;
      if (at < a.want) out[at] = first_bit + b;
      ++at;
    }
  }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));             // a 16-byte piece, 16-byte aligned

struct CopyArgs {
  uint8_t* table;                    // row x at table + x * table_stride + byte_offset
  uint64_t table_stride, byte_offset;
  const uint32_t* ids;               // [n]
  uint8_t* packed;                   // row i at packed + i * packed_stride
  uint64_t packed_stride;
  uint32_t* abort_word;              // or NULL
  uint32_t n, bytes, n_nodes, to_table, align;     // align: 16, 4 or 1 -- what every row of both sides is aligned to
};

__global__ __launch_bounds__(256) void copy_rows_kernel(const CopyArgs a) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t GAS* ids = (const uint32_t GAS*)a.ids;
  for (uint32_t i = blockIdx.x * RU_WAVES + wave; i < a.n; i += gridDim.x * RU_WAVES) {                  // (uniform per wave)
    const uint32_t id = uni(ids[i]);
    if (id >= a.n_nodes) {                                             // never dereferenced
      if (lane == 0 && a.abort_word) *(uint32_t GAS*)a.abort_word = 2u;
      continue;
    }
    uint8_t GAS* t = (uint8_t GAS*)a.table + (uint64_t)id * a.table_stride + a.byte_offset;
    uint8_t GAS* p = (uint8_t GAS*)a.packed + (uint64_t)i * a.packed_stride;
    uint8_t GAS* dst = a.to_table ? t : p;
    const uint8_t GAS* src = a.to_table ? p : t;
    uint32_t done = 0;
    if (a.align == 16u) {
      const uint32_t n16 = a.bytes >> 4;
      for (uint32_t k = lane; k < n16; k += WAVE) ((u32x4 GAS*)dst)[k] = ((const u32x4 GAS*)src)[k];
      done = n16 << 4;
    }
    if (a.align >= 4u) {
      const uint32_t n4 = (a.bytes - done) >> 2;
      for (uint32_t k = lane; k < n4; k += WAVE) ((uint32_t GAS*)(dst + done))[k] = ((const uint32_t GAS*)(src + done))[k];
      done += n4 << 2;
    }
    for (uint32_t k = done + lane; k < a.bytes; k += WAVE) dst[k] = src[k];
  }
}

struct BitIdsArgs {
  uint32_t* bitmap;                  // [ceil(n_bits / 32)]
  const uint32_t* ids;               // [n]
  uint64_t n;
  uint32_t n_bits, set;
};

__global__ __launch_bounds__(256) void bitmap_ids_kernel(const BitIdsArgs a) {
  uint32_t GAS* bm = (uint32_t GAS*)a.bitmap;
  const uint32_t GAS* ids = (const uint32_t GAS*)a.ids;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t id = ids[i];
    if (id >= a.n_bits) continue;                                      // (no word of the bitmap belongs to it)
    const uint32_t bit = 1u << (id & 31u);
    if (a.set) (void)__hip_atomic_fetch_or(bm + (id >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else (void)__hip_atomic_fetch_and(bm + (id >> 5), ~bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct RowsCheckArgs {
  const uint8_t* graph;
  uint64_t entry_len, byte_offset;   // the degree word of node x at graph + x * entry_len + byte_offset
  const uint32_t* ids;               // [n]
  uint32_t* first;                   // [1], 0xFFFFFFFF set by the caller: the lowest offending list position
  uint64_t n;
  uint32_t n_nodes, medoid;
};

__global__ __launch_bounds__(256) void rows_check_kernel(const RowsCheckArgs a) {
  const uint8_t GAS* graph = (const uint8_t GAS*)a.graph;
  const uint32_t GAS* ids = (const uint32_t GAS*)a.ids;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t id = ids[i];
    bool bad = id >= a.n_nodes || id == a.medoid;
    if (!bad) bad = *(const uint32_t GAS*)(graph + (uint64_t)id * a.entry_len + a.byte_offset) != 0u;
    if (bad) (void)__hip_atomic_fetch_min((uint32_t GAS*)a.first, (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------ launchers
static uint32_t stride_wgs(uint64_t n) {
  const uint64_t wgs = (n + 255u) / 256u;
  return (uint32_t)(wgs < RU_MAX_WGS ? wgs : RU_MAX_WGS);
}

extern "C" uint64_t bang_bitmap_select_scratch_words(uint32_t n_bits) { return ((uint64_t)n_bits + BANG_SELECT_SPAN_BITS - 1u) / BANG_SELECT_SPAN_BITS; }

extern "C" int bang_k_bitmap_select(const uint32_t* d_a, const uint32_t* d_not, uint32_t n_bits, uint32_t want, uint32_t* d_ids_out, uint32_t* d_total,
                                    uint32_t* d_scratch, void* stream) {
  if (!d_a || (((uintptr_t)d_a) & 3u)) { bang_set_error("bang_k_bitmap_select: d_a is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (((uintptr_t)d_not) & 3u) { bang_set_error("bang_k_bitmap_select: d_not is not 4-byte aligned"); return BANG_ERR_ARG; }
  if (n_bits == 0 || n_bits > 0xFFFFFFFEu) { bang_set_error("bang_k_bitmap_select: n_bits = %u is outside [1, 2^32 - 2]", n_bits); return BANG_ERR_ARG; }
  if (want != 0 && (!d_ids_out || (((uintptr_t)d_ids_out) & 3u))) { bang_set_error("bang_k_bitmap_select: d_ids_out is null or not 4-byte aligned (want = %u)", want); return BANG_ERR_ARG; }
  if (!d_total || (((uintptr_t)d_total) & 3u)) { bang_set_error("bang_k_bitmap_select: d_total is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!d_scratch || (((uintptr_t)d_scratch) & 3u)) { bang_set_error("bang_k_bitmap_select: d_scratch is null or not 4-byte aligned (bang_bitmap_select_scratch_words(n_bits) words)"); return BANG_ERR_ARG; }
  SelArgs a;
  a.a = d_a; a.nt = d_not; a.counts = d_scratch; a.ids_out = d_ids_out; a.total = d_total;
  a.n_words = ((uint64_t)n_bits + 31u) / 32u; a.n_bits = n_bits; a.want = want; a.spans = (uint32_t)bang_bitmap_select_scratch_words(n_bits);
  hipLaunchKernelGGL(select_count_kernel, dim3(a.spans), dim3(SEL_THREADS), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, (hipStream_t)stream, a);
  if (want != 0) hipLaunchKernelGGL(select_emit_kernel, dim3(a.spans), dim3(SEL_THREADS), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_copy_rows_by_id(void* d_table, uint64_t table_stride, uint64_t byte_offset, const uint32_t* d_ids, uint32_t n, uint32_t n_nodes,
                                      void* d_packed, uint64_t packed_stride, uint32_t bytes, int to_table, uint32_t* d_abort, void* stream) {
  if (!d_table) { bang_set_error("bang_k_copy_rows_by_id: d_table is null"); return BANG_ERR_ARG; }
  if (!d_packed) { bang_set_error("bang_k_copy_rows_by_id: d_packed is null"); return BANG_ERR_ARG; }
  if (!d_ids || (((uintptr_t)d_ids) & 3u)) { bang_set_error("bang_k_copy_rows_by_id: d_ids is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (((uintptr_t)d_abort) & 3u) { bang_set_error("bang_k_copy_rows_by_id: d_abort is not 4-byte aligned"); return BANG_ERR_ARG; }
  if (bytes == 0) { bang_set_error("bang_k_copy_rows_by_id: bytes = 0"); return BANG_ERR_ARG; }
  if (n_nodes == 0) { bang_set_error("bang_k_copy_rows_by_id: n_nodes = 0"); return BANG_ERR_ARG; }
  if (byte_offset > table_stride || bytes > table_stride - byte_offset) {
    bang_set_error("bang_k_copy_rows_by_id: byte_offset = %llu + bytes = %u leaves a table row of table_stride = %llu", (unsigned long long)byte_offset, bytes, (unsigned long long)table_stride);
    return BANG_ERR_ARG;
  }
  if (packed_stride < bytes) { bang_set_error("bang_k_copy_rows_by_id: packed_stride = %llu does not hold bytes = %u", (unsigned long long)packed_stride, bytes); return BANG_ERR_ARG; }
  if (n == 0) return BANG_OK;
  const uint64_t all = (uint64_t)(uintptr_t)d_table | table_stride | byte_offset | (uint64_t)(uintptr_t)d_packed | packed_stride;
  CopyArgs a;
  a.table = (uint8_t*)d_table; a.table_stride = table_stride; a.byte_offset = byte_offset; a.ids = d_ids; a.packed = (uint8_t*)d_packed;
  a.packed_stride = packed_stride; a.abort_word = d_abort; a.n = n; a.bytes = bytes; a.n_nodes = n_nodes; a.to_table = to_table ? 1u : 0u;
  a.align = (all & 15u) == 0 ? 16u : (all & 3u) == 0 ? 4u : 1u;
  const uint32_t wgs = (n + RU_WAVES - 1u) / RU_WAVES;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(wgs < RU_MAX_WGS ? wgs : RU_MAX_WGS), dim3(RU_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

static int bitmap_ids(const char* what, uint32_t set, uint32_t* d_bitmap, uint32_t n_bits, const uint32_t* d_ids, uint64_t n, void* stream) {
  if (!d_bitmap || (((uintptr_t)d_bitmap) & 3u)) { bang_set_error("%s: d_bitmap is null or not 4-byte aligned", what); return BANG_ERR_ARG; }
  if (n_bits == 0) { bang_set_error("%s: n_bits = 0", what); return BANG_ERR_ARG; }
  if (n == 0) return BANG_OK;
  if (!d_ids || (((uintptr_t)d_ids) & 3u)) { bang_set_error("%s: d_ids is null or not 4-byte aligned", what); return BANG_ERR_ARG; }
  BitIdsArgs a;
  a.bitmap = d_bitmap; a.ids = d_ids; a.n = n; a.n_bits = n_bits; a.set = set;
  hipLaunchKernelGGL(bitmap_ids_kernel, dim3(stride_wgs(n)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_bitmap_clear_ids(uint32_t* d_bitmap, uint32_t n_bits, const uint32_t* d_ids, uint64_t n, void* stream) {
  return bitmap_ids("bang_k_bitmap_clear_ids", 0u, d_bitmap, n_bits, d_ids, n, stream);
}
extern "C" int bang_k_bitmap_set_ids(uint32_t* d_bitmap, uint32_t n_bits, const uint32_t* d_ids, uint64_t n, void* stream) {
  return bitmap_ids("bang_k_bitmap_set_ids", 1u, d_bitmap, n_bits, d_ids, n, stream);
}

extern "C" int bang_k_rows_check(const uint8_t* d_graph, uint64_t entry_len, uint64_t byte_offset, const uint32_t* d_ids, uint64_t n, uint32_t n_nodes,
                                 uint32_t medoid, uint32_t* d_first, void* stream) {
  if (!d_graph || (((uintptr_t)d_graph) & 3u)) { bang_set_error("bang_k_rows_check: d_graph is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if ((entry_len & 3u) || (byte_offset & 3u) || byte_offset + 4u > entry_len) {
    bang_set_error("bang_k_rows_check: entry_len = %llu / byte_offset = %llu: both divisible by 4, the degree word inside the entry", (unsigned long long)entry_len, (unsigned long long)byte_offset);
    return BANG_ERR_ARG;
  }
  if (n_nodes == 0) { bang_set_error("bang_k_rows_check: n_nodes = 0"); return BANG_ERR_ARG; }
  if (!d_first || (((uintptr_t)d_first) & 3u)) { bang_set_error("bang_k_rows_check: d_first is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (n >= 0xFFFFFFFFull) { bang_set_error("bang_k_rows_check: n = %llu list positions do not fit the 32-bit report", (unsigned long long)n); return BANG_ERR_ARG; }
  if (n == 0) return BANG_OK;
  if (!d_ids || (((uintptr_t)d_ids) & 3u)) { bang_set_error("bang_k_rows_check: d_ids is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  RowsCheckArgs a;
  a.graph = d_graph; a.entry_len = entry_len; a.byte_offset = byte_offset; a.ids = d_ids; a.first = d_first; a.n = n; a.n_nodes = n_nodes; a.medoid = medoid;
  hipLaunchKernelGGL(rows_check_kernel, dim3(stride_wgs(n)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
