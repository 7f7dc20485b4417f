// bang_consolidate.hip -- the device side of folding the excluded nodes into the graph (DESIGN.md section 2 CANON 22, section 4.16; engine:
// bang_consolidate_e).  X is the engine's exclusion bitmap, med the medoid, D = X \ {med} the nodes removed; a node "in D" below is an id
// < n_nodes, != med, whose bit is set.  row(p) is the first min(degree word, R) ids of p's row, read as ending in front of its first id >= n_nodes
// (such an id is never dereferenced and sets *d_abort = 2, the insert kernels' convention).
//
//  * consolidate_scan_kernel (bang_k_consolidate_scan): one wave per node, grid-stride over [0, n_nodes).  Lane i loads slot i of the row (one
//    coalesced read of 4 R bytes) and tests its id against the bitmap; a ballot says whether the row lists a node of D, and lane 0 sets the
//    node's bit in the affected bitmap (atomic OR).  A node of D is never flagged.
//  * consolidate_gather_kernel (bang_k_consolidate_gather): one wave per affected node p.  The ids of row(p) outside D are compacted into the
//    wave's LDS in row order (ballot + mbcnt); then, in a wave-uniform loop over the slots of row(p) in D, the ids of that neighbour's row that
//    are neither in D nor p go behind them, in row order.  Duplicates stay.  The list is cut at 512 entries, what the cut drops is counted.
//    p's vector becomes the wave's query exactly as in backedge_kernel and exact_dist8 / exact_dist_f32 run on the list unchanged; ids and
//    distances go to row i of the candidate table, offered[i] = the count, own[i] = p: what bang_k_range_sort and bang_k_prune (out_by_own) take.
//  * consolidate_clear_kernel (bang_k_consolidate_clear): one wave per node; the row of a node of D becomes R + 1 zero words.
//
// Layouts are those of bang_search_can_rerank.  All addressing of vectors and rows is 64-bit (id * entry_len); every store to HBM is a vector
// store; no kernel has a workgroup barrier (waves return early).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_exact_dist.h"

#define CONS_MAX BANG_PRUNE_MAX_LIST                     // entries of a candidate list
#define CONS_WAVES 4u                                     // waves per workgroup (INS_WAVES of bang_insert.hip)
#define CONS_SCAN_WGS 4096u                               // workgroups of a scan / clear launch at most: the waves stride over the nodes

// is `id` a removed node?  `word` is bitmap[id >> 5] (word 0 for an id outside the index, which is in no set)
__device__ __forceinline__ uint32_t cons_word(const uint32_t GAS* bitmap, uint32_t id, uint32_t n_nodes) {
  return bitmap[id < n_nodes ? (id >> 5) : 0u];
}
__device__ __forceinline__ bool cons_removed(uint32_t word, uint32_t id, uint32_t n_nodes, uint32_t medoid) {
  return id < n_nodes && id != medoid && ((word >> (id & 31u)) & 1u) != 0u;
}

struct ScanArgs {
  const uint8_t* graph;              // [n_nodes][entry_len]
  uint64_t entry_len;
  const uint32_t* bitmap;            // X: [ceil(n_nodes / 32) + 1]
  uint32_t* affected;                // [ceil(n_nodes / 32)], zeroed by the caller
  uint32_t* abort_word;              // or NULL
  uint32_t n_nodes, R, vec_bytes, medoid;
};

__global__ __launch_bounds__(256) void consolidate_scan_kernel(const ScanArgs a) {
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint8_t GAS* graph = (const uint8_t GAS*)a.graph;
  const uint32_t GAS* bitmap = (const uint32_t GAS*)a.bitmap;
  for (uint32_t p = blockIdx.x * CONS_WAVES + wave; p < a.n_nodes; p += gridDim.x * CONS_WAVES) {       // (uniform per wave)
    const uint32_t pw = uni(bitmap[p >> 5]);
    if (cons_removed(pw, p, a.n_nodes, a.medoid)) continue;        // a removed node's row is cleared, never repaired
    const uint32_t GAS* row = (const uint32_t GAS*)(graph + (uint64_t)p * a.entry_len + a.vec_bytes);
    uint32_t deg = uni(row[0]);
    if (deg > a.R) deg = a.R;
    const uint32_t id = (uint32_t)lane < deg ? row[1u + (uint32_t)lane] : 0u;
    const uint64_t bad = __ballot((uint32_t)lane < deg && id >= a.n_nodes);
    const uint32_t lim = bad ? (uint32_t)__builtin_ctzll(bad) : deg;
    const uint32_t w = cons_word(bitmap, (uint32_t)lane < lim ? id : 0xFFFFFFFFu, a.n_nodes);
    const uint64_t hit = __ballot((uint32_t)lane < lim && cons_removed(w, id, a.n_nodes, a.medoid));
    if (lane == 0) {
      if (bad && a.abort_word) *a.abort_word = 2u;
      if (hit) (void)__hip_atomic_fetch_or(a.affected + (p >> 5), 1u << (p & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

struct GatherArgs {
  const uint8_t* graph;              // [n_nodes][entry_len]
  uint64_t entry_len;
  const uint32_t* bitmap;            // X
  const uint32_t* nodes;             // [n_lists] affected nodes of this chunk
  uint32_t* cand_ids;                // [n_lists][CONS_MAX]
  float* cand_dists;                 // [n_lists][CONS_MAX]
  uint32_t* offered;                 // [n_lists] candidates of a node
  uint32_t* own_out;                 // [n_lists] the node, or BANG_PRUNE_SKIP for an id outside the index
  uint32_t* stats;                   // [1] candidates dropped by the cut
  uint32_t* abort_word;              // or NULL
  uint32_t n_lists, n_nodes, D, R, vec_bytes, medoid;
};

template <int DT>
__global__ __launch_bounds__(256) void consolidate_gather_kernel(const GatherArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t clds[CONS_WAVES][2u * CONS_MAX];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t li = blockIdx.x * CONS_WAVES + wave;
  if (li >= a.n_lists) return;                                     // (uniform per wave; no workgroup barrier)
  uint32_t* sid = clds[wave];
  float* sdist = (float*)(sid + CONS_MAX);
  const uint8_t GAS* graph = (const uint8_t GAS*)a.graph;
  const uint32_t GAS* bitmap = (const uint32_t GAS*)a.bitmap;
  const uint32_t D = a.D, G = D >> 4, R = a.R;
  uint32_t GAS* offered = (uint32_t GAS*)a.offered;
  uint32_t GAS* own_out = (uint32_t GAS*)a.own_out;
  const uint32_t p = uni(((const uint32_t GAS*)a.nodes)[li]);
  if (p >= a.n_nodes) {                                            // never dereferenced: no list, and the prune skips it
    if (lane == 0) { offered[li] = 0u; own_out[li] = BANG_PRUNE_SKIP; if (a.abort_word) *a.abort_word = 2u; }
    return;
  }
  const uint8_t GAS* entry = graph + (uint64_t)p * a.entry_len;
  const uint32_t GAS* prow = (const uint32_t GAS*)(entry + a.vec_bytes);
  uint32_t deg = uni(prow[0]);
  if (deg > R) deg = R;
  const uint32_t id = (uint32_t)lane < deg ? prow[1u + (uint32_t)lane] : 0u;
  bool bad_seen = false;
  uint64_t bad = __ballot((uint32_t)lane < deg && id >= a.n_nodes);
  if (bad) { deg = (uint32_t)__builtin_ctzll(bad); bad_seen = true; }      // row(p) ends in front of the id
  const bool valid = (uint32_t)lane < deg;
  const uint32_t w = cons_word(bitmap, valid ? id : 0xFFFFFFFFu, a.n_nodes);
  const bool gone = valid && cons_removed(w, id, a.n_nodes, a.medoid);
  uint64_t gone_mask = __ballot(gone);
  const uint64_t live_mask = __ballot(valid && !gone);
  if (valid && !gone) sid[lanes_below(live_mask)] = id;            // (deg <= R <= 64 <= CONS_MAX)
  uint32_t total = (uint32_t)__popcll(live_mask), dropped = 0;
  // the rows of the removed neighbours, in the order row(p) lists them
  while (gone_mask != 0ull) {                                      // (uniform)
    const uint32_t slot = (uint32_t)__builtin_ctzll(gone_mask);
    gone_mask &= gone_mask - 1ull;
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)slot);      // (< n_nodes: it passed cons_removed)
    const uint32_t GAS* vrow = (const uint32_t GAS*)(graph + (uint64_t)v * a.entry_len + a.vec_bytes);
    uint32_t vdeg = uni(vrow[0]);
    if (vdeg > R) vdeg = R;
    const uint32_t vid = (uint32_t)lane < vdeg ? vrow[1u + (uint32_t)lane] : 0u;
    bad = __ballot((uint32_t)lane < vdeg && vid >= a.n_nodes);
    if (bad) { vdeg = (uint32_t)__builtin_ctzll(bad); bad_seen = true; }
    const bool vvalid = (uint32_t)lane < vdeg;
    const uint32_t vw = cons_word(bitmap, vvalid ? vid : 0xFFFFFFFFu, a.n_nodes);
    const bool keep = vvalid && vid != p && !cons_removed(vw, vid, a.n_nodes, a.medoid);
    const uint64_t keep_mask = __ballot(keep);
    const uint32_t at = total + lanes_below(keep_mask);
    if (keep && at < CONS_MAX) sid[at] = vid;
    total += (uint32_t)__popcll(keep_mask);
    if (total > CONS_MAX) { dropped += total - CONS_MAX; total = CONS_MAX; }       // the cut: counted, never stored
  }
  if (lane == 0) {
    if (bad_seen && a.abort_word) *a.abort_word = 2u;
    if (dropped != 0u) atomicAdd(a.stats, dropped);
  }
  wave_sync();
  uint32_t GAS* ci = (uint32_t GAS*)a.cand_ids + (uint64_t)li * CONS_MAX;
  float GAS* cd = (float GAS*)a.cand_dists + (uint64_t)li * CONS_MAX;
  if (total != 0u) {
    if (DT == BANG_F32) {
      float qr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const uint32_t j = (uint32_t)u * 64u + (uint32_t)lane; qr[u] = ((const float GAS*)entry)[j < D ? j : 0u]; }
      exact_dist_f32(graph, a.entry_len, D, sid, total, sdist, qr, lane);
    } else {
      const u32x4a qw = *(const u32x4a GAS*)(entry + 16u * ((uint32_t)lane & (G - 1u)));
      const int qq = xdot4<DT == BANG_I8>(qw.x, qw.x, xdot4<DT == BANG_I8>(qw.y, qw.y, xdot4<DT == BANG_I8>(qw.z, qw.z, xdot4<DT == BANG_I8>(qw.w, qw.w, 0))));
      exact_dist8<DT == BANG_I8>(graph, a.entry_len, G, sid, total, sdist, qw, qq, lane);
    }
    wave_sync();
    for (uint32_t i = (uint32_t)lane; i < total; i += WAVE) { ci[i] = sid[i]; cd[i] = sdist[i]; }
  }
  if (lane == 0) { offered[li] = total; own_out[li] = p; }
}

struct ClearArgs {
  uint8_t* graph;
  uint64_t entry_len;
  const uint32_t* bitmap;            // X
  uint32_t n_nodes, R, vec_bytes, medoid;
};

__global__ __launch_bounds__(256) void consolidate_clear_kernel(const ClearArgs a) {
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  uint8_t GAS* graph = (uint8_t GAS*)a.graph;
  const uint32_t GAS* bitmap = (const uint32_t GAS*)a.bitmap;
  for (uint32_t p = blockIdx.x * CONS_WAVES + wave; p < a.n_nodes; p += gridDim.x * CONS_WAVES) {       // (uniform per wave)
    const uint32_t pw = uni(bitmap[p >> 5]);
    if (!cons_removed(pw, p, a.n_nodes, a.medoid)) continue;
    uint32_t GAS* row = (uint32_t GAS*)(graph + (uint64_t)p * a.entry_len + a.vec_bytes);
    for (uint32_t i = (uint32_t)lane; i < a.R + 1u; i += WAVE) row[i] = 0u;
  }
}

// ------------------------------------------------------------------------------------------ launchers
// what every entry checks of the table it walks, before any HIP call; `what` names the entry in the message
static int cons_table_ok(const char* what, const void* d_graph, uint64_t entry_len, uint32_t dtype, uint32_t D, uint32_t R, uint32_t n_nodes,
                         uint32_t medoid, const void* d_excluded) {
  if (!d_graph || (((uintptr_t)d_graph) & 3u)) { bang_set_error("%s: d_graph is null or not 4-byte aligned", what); return BANG_ERR_ARG; }
  if (!d_excluded) { bang_set_error("%s: d_excluded is null", what); return BANG_ERR_ARG; }
  if (R == 0 || R > BANG_MAX_R) { bang_set_error("%s: R = %u is outside [1, %d]", what, R, BANG_MAX_R); return BANG_ERR_ARG; }
  if (n_nodes == 0) { bang_set_error("%s: n_nodes = 0", what); return BANG_ERR_ARG; }
  if (medoid >= n_nodes) { bang_set_error("%s: medoid = %u is not a node (n_nodes = %u)", what, medoid, n_nodes); return BANG_ERR_ARG; }
  const uint64_t vb = (uint64_t)D * (dtype == BANG_F32 ? 4u : 1u);
  if (!((dtype == BANG_U8 || dtype == BANG_I8 || dtype == BANG_F32) && bang_search_can_rerank((int)dtype, D, entry_len, 0)) ||
      entry_len < vb + 4ull * (R + 1u)) {
    bang_set_error("%s: unsupported vector layout or an entry stride that does not hold vector and row (dtype %u, D = %u, R = %u, entry stride %llu): "
                   "8-bit vectors need D %% 16 == 0 with D / 16 a power of two, float vectors D %% 4 == 0; D <= 256 (the wide layouts are refused)",
                   what, dtype, D, R, (unsigned long long)entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  return BANG_OK;
}

static uint32_t cons_stride_wgs(uint32_t n_nodes) {
  const uint32_t wgs = (n_nodes + CONS_WAVES - 1) / CONS_WAVES;
  return wgs < CONS_SCAN_WGS ? wgs : CONS_SCAN_WGS;
}

extern "C" int bang_k_consolidate_scan(const bang_consolidate_scan_params* p, void* stream) {
  if (!p) { bang_set_error("bang_k_consolidate_scan: the parameters are null"); return BANG_ERR_ARG; }
  const int rc = cons_table_ok("bang_k_consolidate_scan", p->d_graph, p->entry_len, p->dtype, p->D, p->R, p->n_nodes, p->medoid, p->d_excluded);
  if (rc != BANG_OK) return rc;
  if (!p->d_affected) { bang_set_error("bang_k_consolidate_scan: d_affected is null"); return BANG_ERR_ARG; }
  ScanArgs a;
  a.graph = p->d_graph; a.entry_len = p->entry_len; a.bitmap = p->d_excluded; a.affected = p->d_affected; a.abort_word = p->d_abort;
  a.n_nodes = p->n_nodes; a.R = p->R; a.vec_bytes = p->D * (p->dtype == BANG_F32 ? 4u : 1u); a.medoid = p->medoid;
  hipLaunchKernelGGL(consolidate_scan_kernel, dim3(cons_stride_wgs(p->n_nodes)), dim3(CONS_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_consolidate_gather(const bang_consolidate_gather_params* p, void* stream) {
  if (!p) { bang_set_error("bang_k_consolidate_gather: the parameters are null"); return BANG_ERR_ARG; }
  const int rc = cons_table_ok("bang_k_consolidate_gather", p->d_graph, p->entry_len, p->dtype, p->D, p->R, p->n_nodes, p->medoid, p->d_excluded);
  if (rc != BANG_OK) return rc;
  if (!p->d_nodes) { bang_set_error("bang_k_consolidate_gather: d_nodes is null"); return BANG_ERR_ARG; }
  if (!p->d_cand_ids || !p->d_cand_dists || !p->d_offered || !p->d_own_out) { bang_set_error("bang_k_consolidate_gather: d_cand_ids, d_cand_dists, d_offered or d_own_out is null"); return BANG_ERR_ARG; }
  if (!p->d_stats) { bang_set_error("bang_k_consolidate_gather: d_stats is null"); return BANG_ERR_ARG; }
  if (p->n_lists == 0) return BANG_OK;
  GatherArgs a;
  a.graph = p->d_graph; a.entry_len = p->entry_len; a.bitmap = p->d_excluded; a.nodes = p->d_nodes; a.cand_ids = p->d_cand_ids;
  a.cand_dists = p->d_cand_dists; a.offered = p->d_offered; a.own_out = p->d_own_out; a.stats = p->d_stats; a.abort_word = p->d_abort;
  a.n_lists = p->n_lists; a.n_nodes = p->n_nodes; a.D = p->D; a.R = p->R; a.vec_bytes = p->D * (p->dtype == BANG_F32 ? 4u : 1u); a.medoid = p->medoid;
  void (*k)(GatherArgs) = p->dtype == BANG_F32 ? consolidate_gather_kernel<BANG_F32>
                          : p->dtype == BANG_I8 ? consolidate_gather_kernel<BANG_I8> : consolidate_gather_kernel<BANG_U8>;
  hipLaunchKernelGGL(k, dim3((p->n_lists + CONS_WAVES - 1) / CONS_WAVES), dim3(CONS_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_consolidate_clear(const bang_consolidate_clear_params* p, void* stream) {
  if (!p) { bang_set_error("bang_k_consolidate_clear: the parameters are null"); return BANG_ERR_ARG; }
  const int rc = cons_table_ok("bang_k_consolidate_clear", p->d_graph, p->entry_len, p->dtype, p->D, p->R, p->n_nodes, p->medoid, p->d_excluded);
  if (rc != BANG_OK) return rc;
  ClearArgs a;
  a.graph = p->d_graph; a.entry_len = p->entry_len; a.bitmap = p->d_excluded;
  a.n_nodes = p->n_nodes; a.R = p->R; a.vec_bytes = p->D * (p->dtype == BANG_F32 ? 4u : 1u); a.medoid = p->medoid;
  hipLaunchKernelGGL(consolidate_clear_kernel, dim3(cons_stride_wgs(p->n_nodes)), dim3(CONS_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
