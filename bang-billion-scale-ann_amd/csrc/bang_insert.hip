// bang_insert.hip -- the device side of inserting points into a loaded index (DESIGN.md section 2 CANON 21, section 4.15; engine: bang_insert_e).
// A batch is one exact-distance search launch (bang_k_search_exact at rr_k = L: each new vector's whole final worklist) and then, on the same
// stream with no host round trip up to the new rows:
//
//  * worklist_lists_kernel (bang_k_worklist_lists): a query's final worklist -- ids u64 [Q][L], distances rank-major [L][Q] -- becomes a candidate
//    list: ids u32 and distances, row per query, its length the entries in front of the first pad entry.
//  * prune_kernel (bang_k_prune): RobustPrune of ordered lists (c_j, d_j) on squared distances.  Wave-resident: a wave owns one list at a time (ids,
//    distances and alive bits in its LDS) and takes list w, w + waves, ...  Walking j ascending, an alive c_j is appended to the row (stop at R); its
//    vector becomes the wave's query exactly as a search kernel holds one (qw / qq per 16-byte piece for 8-bit vectors, qr[4] read with v_readlane
//    for floats), the alive tail t > j is compacted into LDS scratch (ballot + mbcnt) and exact_dist8 / exact_dist_f32 run on it unchanged; c_t dies
//    if alpha2 * e <= d_t (one float multiply, one compare).  The row [u32 degree][u32 id x R] (unused slots 0) is stored with vector stores.
//    An id >= n_nodes is never dereferenced: the list counts as ended there and *d_abort = 2.
//  * backedge_kernel (bang_k_backedge): one wave per old node t that new rows list (CSR of the new ids per target, built on the host:
//    bang_insert_group).  deg_t + |I_t| <= R: the new ids are appended to t's row.  Otherwise the candidates old row ++ I_t (cut at 512) and their
//    exact distances to t's vector go to the target's row of a candidate table; bang_k_range_sort sorts and de-duplicates that row by
//    (distance bits << 32) | id and bang_k_prune writes t's new row.
//  * pq_argmin_kernel (bang_k_pq_encode): code[c] = the lowest k that minimises K1's table entry lut[c][k] (bang_k_lut_build with the new vectors as
//    the queries), one wave per point, the batch chunked to the caller's table buffer.
//
// Layouts are those of bang_search_can_rerank (8-bit: D % 16 == 0, D / 16 a power of two; float: D % 4 == 0; D <= 256).  All addressing of vectors
// and rows is 64-bit (id * entry_len).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_exact_dist.h"

#define PRUNE_MAX BANG_PRUNE_MAX_LIST                    // entries of a list
// LDS words of a wave of prune_kernel: ids, distances, alive bits (+ pad), the row, compacted tail {ids, positions, distances}
#define PRUNE_ALIVE_WORDS (PRUNE_MAX / 32u)
#define PRUNE_WAVE_WORDS (2u * PRUNE_MAX + PRUNE_ALIVE_WORDS + 64u + 3u * PRUNE_MAX)
#define INS_WAVES 4u                                      // waves per workgroup of the small kernels

struct PruneArgs {
  const uint8_t* graph;              // [n_nodes][entry_len]: a node's vector opens its entry
  uint64_t entry_len;
  const uint32_t* list_ids;          // [n_lists][list_stride]
  const float* list_dists;           // [n_lists][list_stride]
  const uint32_t* list_cnt;          // [n_lists]
  const uint32_t* own;               // [n_lists] the list's own node (dropped from it); BANG_PRUNE_SKIP: the list is not pruned, nothing is written
  uint8_t* out;                      // row of list i at out + (out_by_own ? own[i] : i) * out_stride
  uint64_t out_stride;
  uint32_t* abort_word;              // or NULL
  uint32_t list_stride, n_lists, n_nodes, D, R, out_by_own;
  float alpha2;
};

template <int DT>
__global__ __launch_bounds__(1024) void prune_kernel(const PruneArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t plds[];
  const int lane = lane_id();
  const uint32_t W = blockDim.x >> 6, wave = uni(threadIdx.x >> 6);
  uint32_t* ids = plds + (size_t)wave * PRUNE_WAVE_WORDS;
  float* dists = (float*)(ids + PRUNE_MAX);
  uint32_t* alive = ids + 2u * PRUNE_MAX;
  uint32_t* row = alive + PRUNE_ALIVE_WORDS;
  uint32_t* sid = row + 64u;
  uint32_t* spos = sid + PRUNE_MAX;
  float* sdist = (float*)(spos + PRUNE_MAX);
  const uint8_t GAS* graph = (const uint8_t GAS*)a.graph;
  const uint32_t D = a.D, G = D >> 4, R = a.R;
  for (uint32_t li = blockIdx.x * W + wave; li < a.n_lists; li += gridDim.x * W) {       // (uniform per wave; no workgroup barrier)
    const uint32_t own = uni(((const uint32_t GAS*)a.own)[li]);
    if (own == BANG_PRUNE_SKIP) continue;
    if (a.out_by_own && own >= a.n_nodes) {                        // (the row would lie outside the table)
      if (lane == 0 && a.abort_word) *a.abort_word = 2u;
      continue;
    }
    const uint32_t GAS* gi = (const uint32_t GAS*)a.list_ids + (uint64_t)li * a.list_stride;
    const float GAS* gd = (const float GAS*)a.list_dists + (uint64_t)li * a.list_stride;
    uint32_t n = uni(((const uint32_t GAS*)a.list_cnt)[li]);
    if (n > a.list_stride) n = a.list_stride;
    if (n > PRUNE_MAX) n = PRUNE_MAX;
    wave_sync();
    // the list into LDS, 64 entries at a time; it ends in front of the first id outside the index
    bool bad_seen = false;
    for (uint32_t p0 = 0; p0 < n; p0 += WAVE) {                    // (uniform)
      const uint32_t i = p0 + (uint32_t)lane;
      const uint32_t id = gi[i < n ? i : 0u];
      const float d = gd[i < n ? i : 0u];
      const uint64_t bad = __ballot(i < n && id >= a.n_nodes);
      const uint32_t lim = bad ? p0 + (uint32_t)__builtin_ctzll(bad) : n;
      if (i < lim) { ids[i] = id; dists[i] = d; }
      const uint64_t live = __ballot(i < lim && id != own);
      if (lane == 0) { alive[p0 >> 5] = (uint32_t)live; alive[(p0 >> 5) + 1u] = (uint32_t)(live >> 32); }
      if (bad) { n = lim; bad_seen = true; break; }
    }
    if (bad_seen && lane == 0 && a.abort_word) *a.abort_word = 2u;
    wave_sync();
    uint32_t outn = 0;
    for (uint32_t j = 0; j < n && outn < R; ++j) {                 // (uniform)
      if (((alive[j >> 5] >> (j & 31u)) & 1u) == 0u) continue;
      const uint32_t pid = ids[j];
      if (lane == 0) row[outn] = pid;
      ++outn;
      if (outn == R) break;
      // the alive tail behind j, compacted in list order
      uint32_t m = 0;
      for (uint32_t p0 = (j + 1u) & ~63u; p0 < n; p0 += WAVE) {    // (uniform)
        const uint32_t i = p0 + (uint32_t)lane;
        const bool on = i > j && i < n && ((alive[i >> 5] >> (i & 31u)) & 1u) != 0u;
        const uint64_t mask = __ballot(on);
        if (on) { const uint32_t at = m + lanes_below(mask); sid[at] = ids[i]; spos[at] = i; }
        m += (uint32_t)__popcll(mask);
      }
      if (m == 0) break;                                           // nothing is left to pick or to kill
      wave_sync();
      const uint8_t GAS* pv = graph + (uint64_t)pid * a.entry_len;
      if (DT == BANG_F32) {
        float qr[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { const uint32_t k = (uint32_t)t * 64u + (uint32_t)lane; qr[t] = ((const float GAS*)pv)[k < D ? k : 0u]; }
        exact_dist_f32(graph, a.entry_len, D, sid, m, sdist, qr, lane);
      } else {
        const u32x4a qw = *(const u32x4a GAS*)(pv + 16u * ((uint32_t)lane & (G - 1u)));
        const int qq = xdot4<DT == BANG_I8>(qw.x, qw.x, xdot4<DT == BANG_I8>(qw.y, qw.y, xdot4<DT == BANG_I8>(qw.z, qw.z, xdot4<DT == BANG_I8>(qw.w, qw.w, 0))));
        exact_dist8<DT == BANG_I8>(graph, a.entry_len, G, sid, m, sdist, qw, qq, lane);
      }
      wave_sync();
      for (uint32_t i = (uint32_t)lane; i < m; i += WAVE) {
        const uint32_t t = spos[i];
        const float scaled = a.alpha2 * sdist[i];                  // one float32 multiply (the build never contracts) ...
        if (scaled <= dists[t]) (void)__hip_atomic_fetch_and(&alive[t >> 5], ~(1u << (t & 31u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ... one compare
      }
      wave_sync();
    }
    wave_sync();
    uint32_t GAS* out = (uint32_t GAS*)((uint8_t GAS*)a.out + (uint64_t)(a.out_by_own ? own : li) * a.out_stride);
    for (uint32_t i = (uint32_t)lane; i < R + 1u; i += WAVE) out[i] = i == 0u ? outn : (i - 1u < outn ? row[i - 1u] : 0u);
  }
}

struct ListsArgs {
  const uint64_t* wl_ids;            // [Q_total][L]
  const float* wl_dists;             // [L][Q_total]
  uint32_t* list_ids;                // [Q_total][list_stride]
  float* list_dists;
  uint32_t* list_cnt;                // [Q_total]
  uint32_t L, q0, nq, Q_total, list_stride;
};

__global__ __launch_bounds__(256) void worklist_lists_kernel(const ListsArgs a) {
  const int lane = lane_id();
  const uint32_t qi = blockIdx.x * INS_WAVES + uni(threadIdx.x >> 6);
  if (qi >= a.nq) return;                                          // (uniform per wave)
  const uint32_t q = a.q0 + qi;
  const uint64_t GAS* wi = (const uint64_t GAS*)a.wl_ids + (uint64_t)q * a.L;
  const float GAS* wd = (const float GAS*)a.wl_dists + q;
  uint32_t GAS* oi = (uint32_t GAS*)a.list_ids + (uint64_t)q * a.list_stride;
  float GAS* od = (float GAS*)a.list_dists + (uint64_t)q * a.list_stride;
  uint32_t n = 0;
  for (uint32_t p0 = 0; p0 < a.L; p0 += WAVE) {                    // (uniform)
    const uint32_t r = p0 + (uint32_t)lane;
    const uint64_t id = wi[r < a.L ? r : 0u];
    const float d = wd[(uint64_t)(r < a.L ? r : 0u) * a.Q_total];
    const uint64_t pad = __ballot(r < a.L && (id >> 32) != 0ull);  // a pad entry (UINT64_MAX) ends the list
    const uint32_t lim = pad ? p0 + (uint32_t)__builtin_ctzll(pad) : (a.L < p0 + WAVE ? a.L : p0 + WAVE);
    if (r < lim) { oi[r] = (uint32_t)id; od[r] = d; }
    n = lim;
    if (pad) break;
  }
  if (lane == 0) ((uint32_t GAS*)a.list_cnt)[q] = n;
}

struct BackedgeArgs {
  uint8_t* graph;                    // [n_nodes][entry_len]
  uint64_t entry_len;
  const uint32_t* targets;           // [n_targets] old nodes that new rows list
  const uint32_t* offs;              // [n_targets + 1] CSR into srcs
  const uint32_t* srcs;              // the new ids that list a target, ascending
  uint32_t* cand_ids;                // [n_targets][PRUNE_MAX]
  float* cand_dists;                 // [n_targets][PRUNE_MAX]
  uint32_t* offered;                 // [n_targets] candidates of a target that overflows (0: appended)
  uint32_t* own_out;                 // [n_targets] the target, or BANG_PRUNE_SKIP where the ids were appended
  uint32_t* stats;                   // [3] {rows appended, rows pruned, incoming ids dropped by the cap}
  uint32_t* abort_word;              // or NULL
  uint32_t n_targets, n_nodes, n_old, D, R, vec_bytes;
};

template <int DT>
__global__ __launch_bounds__(256) void backedge_kernel(const BackedgeArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t blds[INS_WAVES][2u * PRUNE_MAX];
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t ti = blockIdx.x * INS_WAVES + wave;
  if (ti >= a.n_targets) return;                                   // (uniform per wave; no workgroup barrier)
  uint32_t* sid = blds[wave];
  float* sdist = (float*)(sid + PRUNE_MAX);
  uint8_t GAS* graph = (uint8_t GAS*)a.graph;
  const uint32_t D = a.D, G = D >> 4, R = a.R;
  const uint32_t t = uni(((const uint32_t GAS*)a.targets)[ti]);
  uint32_t GAS* offered = (uint32_t GAS*)a.offered;
  uint32_t GAS* own_out = (uint32_t GAS*)a.own_out;
  if (t >= a.n_old) {                                              // rows of new nodes (and ids outside the index) are never back-edge targets
    if (lane == 0) { offered[ti] = 0u; own_out[ti] = BANG_PRUNE_SKIP; if (a.abort_word) *a.abort_word = 2u; }
    return;
  }
  const uint32_t o0 = uni(((const uint32_t GAS*)a.offs)[ti]), o1 = uni(((const uint32_t GAS*)a.offs)[ti + 1u]);
  const uint32_t GAS* src = (const uint32_t GAS*)a.srcs + o0;
  const uint32_t k = o1 - o0;
  uint8_t GAS* entry = graph + (uint64_t)t * a.entry_len;
  uint32_t GAS* trow = (uint32_t GAS*)(entry + a.vec_bytes);
  uint32_t deg = uni(trow[0]);
  if (deg > R) deg = R;
  if (deg + k <= R) {
    for (uint32_t i = (uint32_t)lane; i < k; i += WAVE) trow[1u + deg + i] = src[i];
    if (lane == 0) { trow[0] = deg + k; offered[ti] = 0u; own_out[ti] = BANG_PRUNE_SKIP; atomicAdd(a.stats + 0, 1u); }
    return;
  }
  uint32_t total = deg + k;
  if (total > PRUNE_MAX) {
    if (lane == 0) atomicAdd(a.stats + 2, total - PRUNE_MAX);
    total = PRUNE_MAX;
  }
  uint32_t GAS* ci = (uint32_t GAS*)a.cand_ids + (uint64_t)ti * PRUNE_MAX;
  float GAS* cd = (float GAS*)a.cand_dists + (uint64_t)ti * PRUNE_MAX;
  bool bad_seen = false;
  for (uint32_t p0 = 0; p0 < total; p0 += WAVE) {                  // (uniform)
    const uint32_t i = p0 + (uint32_t)lane;
    uint32_t id = 0;
    if (i < deg) id = trow[1u + i];
    else if (i < total) id = src[i - deg];
    const uint64_t bad = __ballot(i < total && id >= a.n_nodes);   // never dereferenced: the list ends there
    const uint32_t lim = bad ? p0 + (uint32_t)__builtin_ctzll(bad) : total;
    if (i < lim) { sid[i] = id; ci[i] = id; }
    if (bad) { total = lim; bad_seen = true; break; }
  }
  if (bad_seen && lane == 0 && a.abort_word) *a.abort_word = 2u;
  wave_sync();
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
    for (uint32_t i = (uint32_t)lane; i < total; i += WAVE) cd[i] = sdist[i];
  }
  if (lane == 0) { offered[ti] = total; own_out[ti] = t; atomicAdd(a.stats + 1, 1u); }
}

struct ArgminArgs {
  const float* lut;                  // [n][m][256]
  uint8_t* codes;                    // row of point i at codes + i * code_stride
  uint64_t code_stride;
  uint32_t n, m;
};

__global__ __launch_bounds__(256) void pq_argmin_kernel(const ArgminArgs a) {
  const int lane = lane_id();
  const uint32_t pi = blockIdx.x * INS_WAVES + uni(threadIdx.x >> 6);
  if (pi >= a.n) return;                                           // (uniform per wave)
  const float GAS* lut = (const float GAS*)a.lut + (uint64_t)pi * a.m * 256u;
  uint8_t GAS* out = (uint8_t GAS*)a.codes + (uint64_t)pi * a.code_stride;
  for (uint32_t c0 = 0; c0 < a.m; c0 += WAVE) {                    // (uniform)
    uint32_t mine = 0;
    const uint32_t cn = a.m - c0 < WAVE ? a.m - c0 : WAVE;
    for (uint32_t c = 0; c < cn; ++c) {                            // (uniform)
      const float GAS* e = lut + (uint64_t)(c0 + c) * 256u;
      // lane l holds entries l, l + 64, l + 128, l + 192: ascending k, strict '<' keeps the lowest k of equal entries; the entries are sums of
      // squares (never negative, never NaN inside the input domain), so their bit patterns order like the floats
      uint32_t hi = __float_as_uint(e[lane]), lo = (uint32_t)lane;
#pragma unroll
      for (uint32_t s = 1; s < 4; ++s) {
        const uint32_t v = __float_as_uint(e[s * 64u + (uint32_t)lane]);
        if (v < hi) { hi = v; lo = s * 64u + (uint32_t)lane; }
      }
      wave_min_key(hi, lo);                                        // (every lane gets {smallest bits, lowest k})
      if ((uint32_t)lane == c) mine = lo;
    }
    if ((uint32_t)lane < cn) out[c0 + (uint32_t)lane] = (uint8_t)mine;
  }
  for (uint64_t b = a.m + (uint32_t)lane; b < a.code_stride; b += WAVE) out[b] = 0;     // the pad bytes of a row
}

// ------------------------------------------------------------------------------------------ launchers
static int insert_layout_ok(int dtype, uint32_t D, uint64_t entry_len) {
  return (dtype == BANG_U8 || dtype == BANG_I8 || dtype == BANG_F32) && bang_search_can_rerank(dtype, D, entry_len, 0) &&
         entry_len >= (uint64_t)D * (dtype == BANG_F32 ? 4u : 1u);
}

extern "C" int bang_k_prune(const bang_prune_params* p, void* stream) {
  if (!p) { bang_set_error("bang_k_prune: the parameters are null"); return BANG_ERR_ARG; }
  if (!p->d_graph || (((uintptr_t)p->d_graph) & 3u)) { bang_set_error("bang_k_prune: d_graph is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!p->d_list_ids) { bang_set_error("bang_k_prune: d_list_ids is null"); return BANG_ERR_ARG; }
  if (!p->d_list_dists) { bang_set_error("bang_k_prune: d_list_dists is null"); return BANG_ERR_ARG; }
  if (!p->d_list_cnt) { bang_set_error("bang_k_prune: d_list_cnt is null"); return BANG_ERR_ARG; }
  if (!p->d_own) { bang_set_error("bang_k_prune: d_own is null"); return BANG_ERR_ARG; }
  if (!p->d_out || (((uintptr_t)p->d_out) & 3u)) { bang_set_error("bang_k_prune: d_out is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (p->R == 0 || p->R > BANG_MAX_R) { bang_set_error("bang_k_prune: R = %u is outside [1, %d]", p->R, BANG_MAX_R); return BANG_ERR_ARG; }
  if (p->list_stride == 0) { bang_set_error("bang_k_prune: list_stride = 0"); return BANG_ERR_ARG; }
  if ((p->out_stride & 3u) || p->out_stride < 4ull * (p->R + 1u)) {
    bang_set_error("bang_k_prune: out_stride = %llu is not divisible by 4 or does not hold a row of R = %u", (unsigned long long)p->out_stride, p->R);
    return BANG_ERR_ARG;
  }
  if (p->n_nodes == 0) { bang_set_error("bang_k_prune: n_nodes = 0: the lists hold node ids and need the number of nodes"); return BANG_ERR_ARG; }
  if (!(p->alpha2 >= 1.0f && p->alpha2 <= 64.0f)) { bang_set_error("bang_k_prune: alpha2 = %g is outside [1, 64] (alpha in [1, 8])", (double)p->alpha2); return BANG_ERR_ARG; }
  if (!insert_layout_ok((int)p->dtype, p->D, p->entry_len)) {
    bang_set_error("bang_k_prune: unsupported vector layout (dtype %u, D = %u, entry stride %llu): 8-bit vectors need D %% 16 == 0 with D / 16 a power of "
                   "two, float vectors D %% 4 == 0; D <= 256; an entry stride divisible by 4 that holds the vector (the wide layouts are refused)",
                   p->dtype, p->D, (unsigned long long)p->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  if (p->n_lists == 0) return BANG_OK;
  PruneArgs a;
  a.graph = p->d_graph; a.entry_len = p->entry_len; a.list_ids = p->d_list_ids; a.list_dists = p->d_list_dists; a.list_cnt = p->d_list_cnt;
  a.own = p->d_own; a.out = (uint8_t*)p->d_out; a.out_stride = p->out_stride; a.abort_word = p->d_abort;
  a.list_stride = p->list_stride; a.n_lists = p->n_lists; a.n_nodes = p->n_nodes; a.D = p->D; a.R = p->R; a.out_by_own = p->out_by_own ? 1u : 0u;
  a.alpha2 = p->alpha2;
  static WaveKernelAttr attr[3];
  void (*k)(PruneArgs) = p->dtype == BANG_F32 ? prune_kernel<BANG_F32> : p->dtype == BANG_I8 ? prune_kernel<BANG_I8> : prune_kernel<BANG_U8>;
  uint32_t wgs = 0, waves = 0;
  const int rc = wave_kernel_geometry((const void*)k, attr[p->dtype], PRUNE_WAVE_WORDS * 4u, p->n_lists, p->max_wgs, p->max_waves, &wgs, &waves);
  if (rc == BANG_ERR_UNSUPPORTED) bang_set_error("bang_k_prune: not one wave fits a CU");
  if (rc != BANG_OK) return rc;
  const size_t lds = (size_t)waves * PRUNE_WAVE_WORDS * 4u;
  static bool attr_done[3][BANG_MAX_DEVICES] = {};
  const int dev = current_device();
  if (!attr_done[p->dtype][dev]) {
    HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WAVE_MAX_LDS));
    attr_done[p->dtype][dev] = true;
  }
  hipLaunchKernelGGL(k, dim3(wgs), dim3(waves * WAVE), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_worklist_lists(const uint64_t* d_wl_ids, const float* d_wl_dists, uint32_t L, uint32_t q0, uint32_t nq, uint32_t Q_total,
                                     uint32_t* d_list_ids, float* d_list_dists, uint32_t list_stride, uint32_t* d_list_cnt, void* stream) {
  if (!d_wl_ids) { bang_set_error("bang_k_worklist_lists: d_wl_ids is null"); return BANG_ERR_ARG; }
  if (!d_wl_dists) { bang_set_error("bang_k_worklist_lists: d_wl_dists is null"); return BANG_ERR_ARG; }
  if (!d_list_ids) { bang_set_error("bang_k_worklist_lists: d_list_ids is null"); return BANG_ERR_ARG; }
  if (!d_list_dists) { bang_set_error("bang_k_worklist_lists: d_list_dists is null"); return BANG_ERR_ARG; }
  if (!d_list_cnt) { bang_set_error("bang_k_worklist_lists: d_list_cnt is null"); return BANG_ERR_ARG; }
  if (L == 0 || L > BANG_MAX_L) { bang_set_error("bang_k_worklist_lists: L = %u is outside [1, %d]", L, BANG_MAX_L); return BANG_ERR_ARG; }
  if (list_stride < L) { bang_set_error("bang_k_worklist_lists: list_stride = %u does not hold L = %u entries", list_stride, L); return BANG_ERR_ARG; }
  if (Q_total == 0 || (uint64_t)q0 + nq > Q_total) { bang_set_error("bang_k_worklist_lists: q0 + nq = %llu exceeds Q_total = %u", (unsigned long long)q0 + nq, Q_total); return BANG_ERR_ARG; }
  if (nq == 0) return BANG_OK;
  ListsArgs a;
  a.wl_ids = d_wl_ids; a.wl_dists = d_wl_dists; a.list_ids = d_list_ids; a.list_dists = d_list_dists; a.list_cnt = d_list_cnt;
  a.L = L; a.q0 = q0; a.nq = nq; a.Q_total = Q_total; a.list_stride = list_stride;
  hipLaunchKernelGGL(worklist_lists_kernel, dim3((nq + INS_WAVES - 1) / INS_WAVES), dim3(INS_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_backedge(const bang_backedge_params* p, void* stream) {
  if (!p) { bang_set_error("bang_k_backedge: the parameters are null"); return BANG_ERR_ARG; }
  if (!p->d_graph || (((uintptr_t)p->d_graph) & 3u)) { bang_set_error("bang_k_backedge: d_graph is null or not 4-byte aligned"); return BANG_ERR_ARG; }
  if (!p->d_targets || !p->d_offs || !p->d_srcs) { bang_set_error("bang_k_backedge: d_targets, d_offs or d_srcs is null"); return BANG_ERR_ARG; }
  if (!p->d_cand_ids || !p->d_cand_dists || !p->d_offered || !p->d_own_out) { bang_set_error("bang_k_backedge: d_cand_ids, d_cand_dists, d_offered or d_own_out is null"); return BANG_ERR_ARG; }
  if (!p->d_stats) { bang_set_error("bang_k_backedge: d_stats is null"); return BANG_ERR_ARG; }
  if (p->R == 0 || p->R > BANG_MAX_R) { bang_set_error("bang_k_backedge: R = %u is outside [1, %d]", p->R, BANG_MAX_R); return BANG_ERR_ARG; }
  if (p->n_nodes == 0 || p->n_old > p->n_nodes) { bang_set_error("bang_k_backedge: n_old = %u exceeds n_nodes = %u (or n_nodes = 0)", p->n_old, p->n_nodes); return BANG_ERR_ARG; }
  if (!insert_layout_ok((int)p->dtype, p->D, p->entry_len) || p->entry_len < (uint64_t)p->D * (p->dtype == BANG_F32 ? 4u : 1u) + 4ull * (p->R + 1u)) {
    bang_set_error("bang_k_backedge: unsupported vector layout or an entry stride that does not hold vector and row (dtype %u, D = %u, R = %u, entry stride %llu)",
                   p->dtype, p->D, p->R, (unsigned long long)p->entry_len);
    return BANG_ERR_UNSUPPORTED;
  }
  if (p->n_targets == 0) return BANG_OK;
  BackedgeArgs a;
  a.graph = p->d_graph; a.entry_len = p->entry_len; a.targets = p->d_targets; a.offs = p->d_offs; a.srcs = p->d_srcs;
  a.cand_ids = p->d_cand_ids; a.cand_dists = p->d_cand_dists; a.offered = p->d_offered; a.own_out = p->d_own_out; a.stats = p->d_stats;
  a.abort_word = p->d_abort; a.n_targets = p->n_targets; a.n_nodes = p->n_nodes; a.n_old = p->n_old; a.D = p->D; a.R = p->R;
  a.vec_bytes = p->D * (p->dtype == BANG_F32 ? 4u : 1u);
  void (*k)(BackedgeArgs) = p->dtype == BANG_F32 ? backedge_kernel<BANG_F32> : p->dtype == BANG_I8 ? backedge_kernel<BANG_I8> : backedge_kernel<BANG_U8>;
  hipLaunchKernelGGL(k, dim3((p->n_targets + INS_WAVES - 1) / INS_WAVES), dim3(INS_WAVES * WAVE), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return BANG_OK;
}

extern "C" int bang_k_pq_encode(const float* d_pivots_T, const void* d_vectors, int dtype, const float* d_centroid, const uint32_t* d_chunk_off,
                                float* d_lut, uint32_t lut_points, uint32_t n, uint32_t D, uint32_t m, uint8_t* d_codes, uint64_t code_stride,
                                void* stream) {
  if (!d_pivots_T) { bang_set_error("bang_k_pq_encode: d_pivots_T is null"); return BANG_ERR_ARG; }
  if (!d_vectors) { bang_set_error("bang_k_pq_encode: d_vectors is null"); return BANG_ERR_ARG; }
  if (!d_centroid) { bang_set_error("bang_k_pq_encode: d_centroid is null"); return BANG_ERR_ARG; }
  if (!d_chunk_off) { bang_set_error("bang_k_pq_encode: d_chunk_off is null"); return BANG_ERR_ARG; }
  if (!d_lut) { bang_set_error("bang_k_pq_encode: d_lut (the table buffer) is null"); return BANG_ERR_ARG; }
  if (!d_codes) { bang_set_error("bang_k_pq_encode: d_codes is null"); return BANG_ERR_ARG; }
  if (dtype < BANG_U8 || dtype > BANG_F32) { bang_set_error("bang_k_pq_encode: dtype = %d", dtype); return BANG_ERR_ARG; }
  if (D == 0 || m == 0 || m > D) { bang_set_error("bang_k_pq_encode: D = %u, m = %u (1 <= m <= D)", D, m); return BANG_ERR_ARG; }
  if (lut_points == 0) { bang_set_error("bang_k_pq_encode: lut_points = 0: d_lut must hold the tables of at least one point"); return BANG_ERR_ARG; }
  if (code_stride < m) { bang_set_error("bang_k_pq_encode: code_stride = %llu is smaller than a row (m = %u)", (unsigned long long)code_stride, m); return BANG_ERR_ARG; }
  const size_t vb = (size_t)D * (dtype == BANG_F32 ? 4u : 1u);
  for (uint32_t p0 = 0; p0 < n; p0 += lut_points) {
    const uint32_t np = n - p0 < lut_points ? n - p0 : lut_points;
    const int rc = bang_k_lut_build(d_pivots_T, (const uint8_t*)d_vectors + (size_t)p0 * vb, dtype, d_centroid, d_chunk_off, d_lut, np, D, m, 0, stream);
    if (rc != BANG_OK) return rc;
    ArgminArgs a;
    a.lut = d_lut; a.codes = d_codes + (uint64_t)p0 * code_stride; a.code_stride = code_stride; a.n = np; a.m = m;
    hipLaunchKernelGGL(pq_argmin_kernel, dim3((np + INS_WAVES - 1) / INS_WAVES), dim3(INS_WAVES * WAVE), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
  }
  return BANG_OK;
}
