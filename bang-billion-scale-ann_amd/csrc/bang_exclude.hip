// bang_exclude.hip -- lazy deletes (DESIGN.md section 2 CANON 17, section 4.12): an engine's exclusion set X is a bitmap over the node ids in HBM, and
// everything that honours it sits BEHIND the walk -- no search kernel reads it.
//
//  * cand_live_kernel (bang_k_cand_live): the PQ walks.  Per query, the candidate log (d_cand_ids, d_cand_cnt) is copied to d_live_ids / d_live_cnt
//    without its entries in X, in log order; K6 + K7 (bang_k_rerank*) then run on that list as they would on the log.
//  * worklist_pick_kernel (bang_k_worklist_pick): the exact-distance walks.  The search kernel is launched at rr_k = L, so its "results" are the
//    whole final worklist; the first k entries not in X, in worklist order, become the query's results (padded with UINT64_MAX / 3.402823E+38f).
//
// Both: one wave per query, four waves per workgroup, the list walked in 64-entry pieces -- one coalesced load of the piece and one bitmap word
// (bitmap[id >> 5]) per lane -- with the loads of the pieces ahead in flight while the current one is compacted: __ballot of the survivors,
// lanes_below for a survivor's slot behind a wave-uniform base.  No LDS, no scratch, global_ accesses only.  An id >= n_nodes is kept and never
// looked up (the search kernels' abort word reports such rows): no access leaves the bitmap's ceil(n_nodes / 32) + 1 words.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"

#define EXCL_WAVES 4u                // waves (= queries) per workgroup

struct LiveArgs {
  const uint32_t* cand_ids;          // [Q][cand_stride]
  const uint32_t* cand_cnt;          // [Q]
  const uint32_t* bitmap;            // [ceil(n_nodes / 32) + 1]
  uint32_t* live_ids;                // [Q][cand_stride]
  uint32_t* live_cnt;                // [Q]
  uint32_t cand_stride, q0, nq, n_nodes;
};

// bit of `id` in the set; an id outside the index is in no set (and the word read for it is word 0)
__device__ __forceinline__ uint32_t excl_word(const uint32_t GAS* bitmap, uint32_t id, uint32_t n_nodes) {
  return bitmap[id < n_nodes ? (id >> 5) : 0u];
}
__device__ __forceinline__ bool excl_bit(uint32_t word, uint32_t id, uint32_t n_nodes) {
  return id < n_nodes && ((word >> (id & 31u)) & 1u) != 0u;
}

__global__ __launch_bounds__(256) void cand_live_kernel(const LiveArgs a) {
  const int lane = lane_id();
  const uint32_t qi = blockIdx.x * EXCL_WAVES + uni(threadIdx.x >> 6);
  if (qi >= a.nq) return;                                          // (uniform per wave)
  const uint32_t q = a.q0 + qi;
  const uint32_t GAS* bitmap = (const uint32_t GAS*)a.bitmap;
  const uint32_t GAS* log = (const uint32_t GAS*)a.cand_ids + (size_t)q * a.cand_stride;
  uint32_t GAS* live = (uint32_t GAS*)a.live_ids + (size_t)q * a.cand_stride;
  uint32_t n = uni(((const uint32_t GAS*)a.cand_cnt)[q]);
  if (n > a.cand_stride) n = a.cand_stride;                        // (a count never leaves the query's row of the log)
  // piece p: entry p * 64 + lane (a lane past the log re-reads entry 0: in bounds, dropped below).  Two pieces' ids and one piece's bitmap words
  // are in flight while a piece is compacted.
  auto load_id = [&](uint32_t p) { const uint32_t i = p * WAVE + (uint32_t)lane; return log[i < n ? i : 0u]; };
  uint32_t id0 = load_id(0), id1 = load_id(1);
  uint32_t w0 = excl_word(bitmap, id0, a.n_nodes);
  uint32_t base = 0;
  for (uint32_t p = 0; p * WAVE < n; ++p) {
    const uint32_t id2 = load_id(p + 2);
    const uint32_t w1 = excl_word(bitmap, id1, a.n_nodes);
    const bool keep = p * WAVE + (uint32_t)lane < n && !excl_bit(w0, id0, a.n_nodes);
    const uint64_t mask = __ballot(keep);
    if (keep) live[base + lanes_below(mask)] = id0;
    base += (uint32_t)__popcll(mask);
    id0 = id1; w0 = w1; id1 = id2;
  }
  if (lane == 0) ((uint32_t GAS*)a.live_cnt)[q] = base;
}

struct PickArgs {
  const uint64_t* wl_ids;            // [Q_total][L]
  const float* wl_dists;             // [L][Q_total]
  const uint32_t* bitmap;
  uint64_t* ids_out;                 // [Q_total][k]
  float* dists_out;                  // [k][Q_total]
  uint32_t L, k, q0, nq, Q_total, n_nodes;
};

__global__ __launch_bounds__(256) void worklist_pick_kernel(const PickArgs a) {
  const int lane = lane_id();
  const uint32_t qi = blockIdx.x * EXCL_WAVES + uni(threadIdx.x >> 6);
  if (qi >= a.nq) return;                                          // (uniform per wave)
  const uint32_t q = a.q0 + qi;
  const uint32_t L = a.L, k = a.k, Qt = a.Q_total;
  const uint32_t GAS* bitmap = (const uint32_t GAS*)a.bitmap;
  const uint64_t GAS* wi = (const uint64_t GAS*)a.wl_ids + (size_t)q * L;
  const float GAS* wd = (const float GAS*)a.wl_dists + q;
  uint64_t GAS* ids_out = (uint64_t GAS*)a.ids_out + (size_t)q * k;
  float GAS* dists_out = (float GAS*)a.dists_out + q;
  // piece p: rank p * 64 + lane (a lane past the worklist re-reads rank 0: in bounds, dropped below).  The next piece's ids and distances are in
  // flight while a piece is compacted.
  auto load_id = [&](uint32_t p) { const uint32_t r = p * WAVE + (uint32_t)lane; return wi[r < L ? r : 0u]; };
  auto load_d = [&](uint32_t p) { const uint32_t r = p * WAVE + (uint32_t)lane; return wd[(size_t)(r < L ? r : 0u) * Qt]; };
  uint64_t id0 = load_id(0);
  float d0 = load_d(0);
  uint32_t base = 0;
  for (uint32_t p = 0; p * WAVE < L; ++p) {
    const uint64_t id1 = load_id(p + 1);
    const float d1 = load_d(p + 1);
    const bool valid = p * WAVE + (uint32_t)lane < L;
    const uint64_t pad = __ballot(valid && id0 == ~0ull);         // padding ends the scan: nothing at or behind the first padding entry counts
    const bool before = pad == 0ull || (uint32_t)lane < (uint32_t)__builtin_ctzll(pad);
    const uint32_t x = (uint32_t)id0;
    const bool in_index = valid && before && (id0 >> 32) == 0ull;
    const uint32_t w = excl_word(bitmap, in_index ? x : 0xFFFFFFFFu, a.n_nodes);
    const bool keep = valid && before && !(in_index && excl_bit(w, x, a.n_nodes));
    const uint64_t mask = __ballot(keep);
    const uint32_t slot = base + lanes_below(mask);
    if (keep && slot < k) {
      ids_out[slot] = id0;                                         // [Q][k] u64
      dists_out[(size_t)slot * Qt] = d0;                           // [rank][Q]: the distance bits as the walk left them
    }
    base += (uint32_t)__popcll(mask);
    if (base >= k || pad != 0ull) break;                           // (uniform)
    id0 = id1; d0 = d1;
  }
  for (uint32_t r = base + (uint32_t)lane; r < k; r += WAVE) {     // fewer than k live entries: the padded tail (CANON 8)
    ids_out[r] = ~0ull;
    dists_out[(size_t)r * Qt] = BIG_DIST;
  }
}

extern "C" int bang_k_cand_live(const uint32_t* d_cand_ids, const uint32_t* d_cand_cnt, uint32_t cand_stride, uint32_t q0, uint32_t nq,
                                const uint32_t* d_bitmap, uint32_t n_nodes, uint32_t* d_live_ids, uint32_t* d_live_cnt, void* stream) {
  if (!d_cand_ids) { bang_set_error("bang_k_cand_live: d_cand_ids is null"); return BANG_ERR_ARG; }
  if (!d_cand_cnt) { bang_set_error("bang_k_cand_live: d_cand_cnt is null"); return BANG_ERR_ARG; }
  if (!d_bitmap) { bang_set_error("bang_k_cand_live: d_bitmap is null"); return BANG_ERR_ARG; }
  if (!d_live_ids) { bang_set_error("bang_k_cand_live: d_live_ids is null"); return BANG_ERR_ARG; }
  if (!d_live_cnt) { bang_set_error("bang_k_cand_live: d_live_cnt is null"); return BANG_ERR_ARG; }
  if (d_live_ids == d_cand_ids) { bang_set_error("bang_k_cand_live: d_live_ids is the log itself (d_cand_ids): the candidate log stays the walk's"); return BANG_ERR_ARG; }
  if (cand_stride == 0) { bang_set_error("bang_k_cand_live: cand_stride = 0"); return BANG_ERR_ARG; }
  if ((uint64_t)q0 + nq > 0xFFFFFFFFull) { bang_set_error("bang_k_cand_live: q0 + nq = %llu does not fit 32 bits", (unsigned long long)q0 + nq); return BANG_ERR_ARG; }
  if (nq == 0) return BANG_OK;
  LiveArgs a;
  a.cand_ids = d_cand_ids; a.cand_cnt = d_cand_cnt; a.bitmap = d_bitmap; a.live_ids = d_live_ids; a.live_cnt = d_live_cnt;
  a.cand_stride = cand_stride; a.q0 = q0; a.nq = nq; a.n_nodes = n_nodes;
  hipLaunchKernelGGL(cand_live_kernel, dim3((nq + EXCL_WAVES - 1) / EXCL_WAVES), dim3(EXCL_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_worklist_pick(const uint64_t* d_wl_ids, const float* d_wl_dists, uint32_t L, uint32_t q0, uint32_t nq, uint32_t Q_total,
                                    const uint32_t* d_bitmap, uint32_t n_nodes, uint32_t k, uint64_t* d_ids_out, float* d_dists_out, void* stream) {
  if (!d_wl_ids) { bang_set_error("bang_k_worklist_pick: d_wl_ids is null"); return BANG_ERR_ARG; }
  if (!d_wl_dists) { bang_set_error("bang_k_worklist_pick: d_wl_dists is null"); return BANG_ERR_ARG; }
  if (!d_bitmap) { bang_set_error("bang_k_worklist_pick: d_bitmap is null"); return BANG_ERR_ARG; }
  if (!d_ids_out) { bang_set_error("bang_k_worklist_pick: d_ids_out is null"); return BANG_ERR_ARG; }
  if (!d_dists_out) { bang_set_error("bang_k_worklist_pick: d_dists_out is null"); return BANG_ERR_ARG; }
  if (d_ids_out == d_wl_ids || d_dists_out == d_wl_dists) { bang_set_error("bang_k_worklist_pick: d_ids_out / d_dists_out are the worklist buffers themselves"); return BANG_ERR_ARG; }
  if (L == 0 || L > BANG_MAX_L) { bang_set_error("bang_k_worklist_pick: L = %u is outside [1, %d]", L, BANG_MAX_L); return BANG_ERR_ARG; }
  if (k == 0) { bang_set_error("bang_k_worklist_pick: k = 0"); return BANG_ERR_ARG; }
  if (k > L) { bang_set_error("bang_k_worklist_pick: k = %u exceeds L = %u", k, L); return BANG_ERR_ARG; }
  if (Q_total == 0) { bang_set_error("bang_k_worklist_pick: Q_total = 0 (the stride of the rank-major distances)"); return BANG_ERR_ARG; }
  if ((uint64_t)q0 + nq > Q_total) { bang_set_error("bang_k_worklist_pick: q0 + nq = %llu exceeds Q_total = %u", (unsigned long long)q0 + nq, Q_total); return BANG_ERR_ARG; }
  if (nq == 0) return BANG_OK;
  PickArgs a;
  a.wl_ids = d_wl_ids; a.wl_dists = d_wl_dists; a.bitmap = d_bitmap; a.ids_out = d_ids_out; a.dists_out = d_dists_out;
  a.L = L; a.k = k; a.q0 = q0; a.nq = nq; a.Q_total = Q_total; a.n_nodes = n_nodes;
  hipLaunchKernelGGL(worklist_pick_kernel, dim3((nq + EXCL_WAVES - 1) / EXCL_WAVES), dim3(EXCL_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}
