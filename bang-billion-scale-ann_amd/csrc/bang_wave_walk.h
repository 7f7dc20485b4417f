// bang_wave_walk.h -- the stages of the wave-resident walk that bang_search_exact.hip, bang_search_lut.hip and bang_search_beam.hip share, each
// written once.  A wave owns one query from its first iteration to its last (worklist + survivors in LDS), then takes the next unstarted query
// from *d_next_query.  What differs between the forms -- the distance stage, the label and range blocks, the wide tile, the beam's steps 1-5 with
// its four-row filter -- stays in the kernels; a stage here never asks which kernel calls it.  Whole device functions only: a kernel that includes
// this file inlines them as it inlined its own copy.  A stage takes the members of bang_search_params it uses BY VALUE, never the struct: a
// reference to the kernel's argument handed to a function keeps the argument in memory until the inliner has run, and every load from the kernarg
// segment then loses its no-clobber marking (measured: up to 12 VGPRs and the waves per CU of the beam instances moved).
//
// Reference line numbers: the reference's BANG_Base/bang_search.cu.
#ifndef BANG_WAVE_WALK_H_
#define BANG_WAVE_WALK_H_

#include "bang_device.h"
#include "bang_worklist.h"
#include "bang_exact_dist.h"

// ---------------------------------------------------------------------------------------------------------------------
// around the kernel: the {start, end} stamps of a workgroup (d_ktime, or null)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void walk_stamp_start(unsigned long long* d_ktime) {
  if (d_ktime && threadIdx.x == 0) d_ktime[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void walk_stamp_end(unsigned long long* d_ktime) {
  if (d_ktime) {
    __syncthreads();
    if (threadIdx.x == 0) d_ktime[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the next query: the first one by position (wave gw of total_waves), then from the hand-out counter
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t walk_next_query(bool first_q, uint32_t gw, uint32_t total_waves, uint32_t* d_next_query, int lane) {
  if (first_q) return gw;
  uint32_t t = 0;
  if (lane == 0) t = __hip_atomic_fetch_add(d_next_query, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return total_waves + uni(t);
}

// ---------------------------------------------------------------------------------------------------------------------
// a wave's LDS: a sorted list of capacity L at wbase ([L distances][L ids][L visited bytes]) and, scratch_at words behind wbase, the
// WAVE_SCRATCH_WORDS of sort scratch, which carry the survivors between the filter and the sort
// ---------------------------------------------------------------------------------------------------------------------
struct WalkLds {
  WaveLds s;
  uint32_t* scratch;                 // what a form adds (row tile, survivor arrays) starts at scratch + WAVE_SCRATCH_WORDS
  float* sdist;                      // the survivors' distances (dead before the sort writes sd)
  uint32_t* sc;                      // the survivors' ids, in input order (== td: dead before the sort)
};
__device__ __forceinline__ WalkLds walk_lds(uint32_t* wbase, uint32_t L, uint32_t scratch_at) {
  WalkLds w;
  uint32_t* scratch = wbase + scratch_at;
  w.s.wd = (float*)wbase; w.s.wi = wbase + L; w.s.wv = (uint8_t*)(wbase + 2 * L);
  w.s.sd = (float*)scratch; w.s.ti = scratch; w.s.td = (float*)(scratch + 72);
  w.scratch = scratch;
  w.sdist = (float*)scratch;
  w.sc = scratch + 72;
  return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// the raw query of the narrow layouts, in registers.  Float: qr[t] of lane l holds element 64 t + l.  8-bit: G = D / 16 adjacent lanes per
// survivor, qw this lane's 16-byte piece (piece lane % G), qq the sum of its squares
// ---------------------------------------------------------------------------------------------------------------------
template <bool SIGNED>
__device__ __forceinline__ int query_sumsq(u32x4a qw) {
  return xdot4<SIGNED>(qw.x, qw.x, xdot4<SIGNED>(qw.y, qw.y, xdot4<SIGNED>(qw.z, qw.z, xdot4<SIGNED>(qw.w, qw.w, 0))));
}

struct NarrowQuery { float qr[4]; u32x4a qw; int qq; uint32_t G; };
template <int DT>
__device__ __forceinline__ NarrowQuery walk_load_query_narrow(const void* queries, size_t qabs, uint32_t D, int lane) {
  NarrowQuery nq;
  nq.qw = (u32x4a){0u, 0u, 0u, 0u};
  nq.qq = 0;
  nq.G = 1;
#pragma unroll
  for (int t = 0; t < 4; ++t) nq.qr[t] = 0.0f;
  if (DT == BANG_F32) {
    const float GAS* qsrc = (const float GAS*)queries + qabs * D;
#pragma unroll
    for (int t = 0; t < 4; ++t) { const uint32_t j = (uint32_t)t * 64u + (uint32_t)lane; nq.qr[t] = qsrc[j < D ? j : 0u]; }
  } else {
    nq.G = D >> 4;
    nq.qw = *(const u32x4a GAS*)((const uint8_t GAS*)queries + qabs * D + 16u * ((uint32_t)lane & (nq.G - 1u)));
    nq.qq = query_sumsq<DT == BANG_I8>(nq.qw);
  }
  return nq;
}

// ---------------------------------------------------------------------------------------------------------------------
// per-query state (bang_init :440-489): candidate log = [MEDOID]; the first row is the seed list [MEDOID, adj(MEDOID)...], its 65th id in x1
// ---------------------------------------------------------------------------------------------------------------------
struct WalkSeed { uint32_t cnt, x0, x1; };
__device__ __forceinline__ WalkSeed walk_begin_query(uint32_t* d_cand_ids, const uint32_t* d_seed, uint32_t q, uint32_t cand_stride, uint32_t medoid,
                                                     int lane) {
  if (lane == 0) d_cand_ids[(size_t)q * cand_stride] = medoid;
  WalkSeed sd;
  sd.cnt = d_seed[0]; sd.x0 = d_seed[1 + lane]; sd.x1 = d_seed[65];
  return sd;
}
__device__ __forceinline__ WlHead walk_empty_head() {
  WlHead head;
  head.found = false; head.idx = 0; head.id = 0; head.d = 0.0f; head.tail = 0.0f;
  return head;
}

// ---------------------------------------------------------------------------------------------------------------------
// the length of the row an iteration consumes: capped at R (R + 1: the seed list), and 0 -- with *d_abort = 2 -- where one of its ids is >= lim
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t walk_ids_in_range(uint32_t ci, uint32_t lim, uint32_t x0, uint32_t x1, uint32_t* d_abort, int lane) {
  if (__ballot((uint32_t)lane < ci && x0 >= lim) != 0ull || (ci > 64u && uni(x1) >= lim)) {
    if (lane == 0 && d_abort) *d_abort = 2u;
    ci = 0;
  }
  return ci;
}

// a graph entry's row: the degree word travels with the ids.  n_nodes == 0: ids are not checked
__device__ __forceinline__ uint32_t walk_row_len_entry(bool have_row, uint32_t cnt_in, bool first, uint32_t R, uint32_t n_nodes, uint32_t x0,
                                                       uint32_t x1, uint32_t* d_abort, int lane) {
  uint32_t ci = have_row ? uni(cnt_in) : 0u;
  const uint32_t cap = R + (first ? 1u : 0u);
  if (ci > cap) ci = cap;
  if (n_nodes != 0u) ci = walk_ids_in_range(ci, n_nodes, x0, x1, d_abort, lane);
  return ci;
}

// a 256-byte adjacency row (row_layout 1): ids first, BANG_ADJ_PAD behind them; the seed list keeps its count.  A pad value in front of an id -- a
// row overwritten since bang_load -- is an id out of range whether or not n_nodes was given
__device__ __forceinline__ uint32_t walk_row_len_pulled(bool have_row, uint32_t cnt_in, bool first, uint32_t R, uint32_t n_nodes, uint32_t x0,
                                                        uint32_t x1, uint32_t* d_abort, int lane) {
  uint32_t ci = have_row ? uni(cnt_in) : 0u;
  if (!first && have_row) ci = (uint32_t)__popcll(__ballot(x0 != BANG_ADJ_PAD));
  const uint32_t cap = R + (first ? 1u : 0u);
  if (ci > cap) ci = cap;
  return walk_ids_in_range(ci, n_nodes != 0u ? n_nodes : BANG_ADJ_PAD, x0, x1, d_abort, lane);
}

// ---------------------------------------------------------------------------------------------------------------------
// K5: filter (neighbor_filtering_new :1140-1165).  The ci ids of the row (lane l: x0; the seed list's 65th: x1) against the query's filter
// words; the n survivors' ids go to sc[0, n) in input order and come back in registers (lane l: sid0 = sc[l]; lane 0: sid1 = sc[64])
// ---------------------------------------------------------------------------------------------------------------------
struct WalkSurvivors { uint32_t n, sid0, sid1; };
__device__ __forceinline__ WalkSurvivors walk_filter(uint32_t GAS* bloom, uint32_t ci, uint32_t x0, uint32_t x1, uint32_t* sc, int lane) {
  const bool v0 = (uint32_t)lane < ci;
  const bool v1 = ci > 64;                                        // the 65th id exists in the seed list only (uniform)
  const uint32_t h0a = hash1(x0), h0b = hash2(x0);
  uint32_t h1a = 0, h1b = 0, w0a = 0, w0b = 0, w1a = 0, w1b = 0;
  // CANON 3: every id is tested against the filter state at entry -- both words in one round trip, read past L1; the previous iteration's atomic
  // ORs have completed (s_waitcnt vmcnt(0) ahead of the probes, behind the adjacency row they need anyway).  The claim table of bang_search.hip
  // (plain stores, same-word lanes merged in LDS) is for a kernel whose iteration is bound by requests past L2; here an evaluation already costs
  // 2-6 lines of vector or a table gather
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (v0) { w0a = ld_bypass_l1(&bloom[h0a >> 5]); w0b = ld_bypass_l1(&bloom[h0b >> 5]); }
  if (v1) {
    h1a = hash1(x1); h1b = hash2(x1);
    if (lane == 0) { w1a = ld_bypass_l1(&bloom[h1a >> 5]); w1b = ld_bypass_l1(&bloom[h1b >> 5]); }
  }
  const bool pass0 = v0 && !(((w0a >> (h0a & 31)) & 1u) && ((w0b >> (h0b & 31)) & 1u));
  const bool pass1 = v1 && (lane == 0) && !(((w1a >> (h1a & 31)) & 1u) && ((w1b >> (h1b & 31)) & 1u));
  const uint64_t m0 = __ballot(pass0);
  const uint64_t m1 = __ballot(pass1);
  const uint32_t n0 = (uint32_t)__popcll(m0);
  WalkSurvivors sv;
  sv.n = n0 + (uint32_t)__popcll(m1);
  // ... then every survivor's two bits are set (:1159-1160), with atomic ORs into the query's private words: one request per bit, no LDS
  if (pass0) {
    (void)__hip_atomic_fetch_or(&bloom[h0a >> 5], 1u << (h0a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_or(&bloom[h0b >> 5], 1u << (h0b & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (pass1) {
    (void)__hip_atomic_fetch_or(&bloom[h1a >> 5], 1u << (h1a & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_or(&bloom[h1b >> 5], 1u << (h1b & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // ordered compaction through LDS: survivors keep input order (CANON; the reference emits in atomicAdd order :1161)
  if (pass0) sc[lanes_below(m0)] = x0;
  if (pass1) sc[n0] = x1;
  wave_sync();
  sv.sid0 = ((uint32_t)lane < sv.n) ? sc[lane] : 0u;
  sv.sid1 = (lane == 0 && sv.n > 64) ? sc[64] : 0u;
  return sv;
}

// ---------------------------------------------------------------------------------------------------------------------
// K4: parent (compute_parent1 :1464-1521 / compute_parent2 :1384-1459), as bang_search.hip: the closest survivor that is not the medoid against
// the worklist's first unvisited entry (head, as the previous merge left it).  A parent taken from the worklist is marked visited there; one
// taken from the survivors becomes mark, which the merge sets.  found: the candidate log grows by one (cc)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void walk_parent(const WaveLds& s, const WlHead& head, uint32_t n, uint32_t sid0, uint32_t sid1, float d0, float d1,
                                            bool first, uint32_t w_n, uint32_t medoid, uint32_t& mark, uint32_t& cc, uint32_t& parent, bool& found,
                                            int lane) {
  const bool elig = (uint32_t)lane < n && sid0 != medoid && d0 < BIG_DIST;
  // (squared distances are non-negative: their bit patterns order like the floats; {bits, lane}: first minimum wins)
  uint32_t khi = elig ? __float_as_uint(d0) : 0xFFFFFFFFu, klo = (uint32_t)lane;
  wave_min_key(khi, klo);
  uint32_t bi = (khi != 0xFFFFFFFFu) ? klo : 0xFFFFu;
  float bd = (khi != 0xFFFFFFFFu) ? __uint_as_float(khi) : BIG_DIST;
  uint32_t bid = (uint32_t)__builtin_amdgcn_readlane((int)sid0, (int)(klo & 63u));
  if (n > 64) {                                                   // element 64 can only win with a strictly smaller distance
    const float e_d = __shfl(d1, 0);
    const uint32_t e_id = (uint32_t)__shfl((int)sid1, 0);
    if (e_id != medoid && e_d < BIG_DIST && (bi == 0xFFFFu || e_d < bd)) { bd = e_d; bi = 64; bid = e_id; }
  }
  const bool have_best = (bi != 0xFFFFu);
  if (!have_best) bd = BIG_DIST;
  bool from_best = false;
  if (first) {
    if (have_best) { found = true; parent = bid; from_best = true; }
  } else {
    if (head.found) {                                             // first unvisited entry :1425-1439
      found = true;
      if (bd < head.d) { parent = bid; from_best = true; }
      else { parent = head.id; if (lane == 0) s.wv[head.idx] = 1; }
    } else if (w_n > 0) {                                         // corner case :1442-1446
      if (bd < head.tail) { found = true; parent = bid; from_best = true; }
    }
  }
  parent = uni(parent);
  if (found) {
    if (from_best) mark = parent;
    ++cc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// a parent's adjacency row, requested as soon as the parent is known: it travels during the sort / merge
// ---------------------------------------------------------------------------------------------------------------------
// from its graph entry [vec][u32 degree][u32 id x R]: the degree, and id `lane` of the row
struct WalkEntryRow { uint32_t cnt, x; };
__device__ __forceinline__ WalkEntryRow walk_fetch_entry_row(const uint8_t GAS* graph, uint64_t entry_len, uint32_t vec_bytes, uint32_t R,
                                                             uint32_t parent, int lane) {
  const uint32_t GAS* nrow = (const uint32_t GAS*)(graph + (uint64_t)parent * entry_len + vec_bytes);
  WalkEntryRow r;
  r.cnt = nrow[0];
  r.x = nrow[1 + ((uint32_t)lane < R ? (uint32_t)lane : 0u)];
  return r;
}

// a 256-byte row (row_layout 1): all 64 lanes load one dword.  Slice parent / slice_rows of the node's HBM-resident rows (this GPU's HBM or a
// peer's over xGMI; 0: that slice is not there), else the HBM copy of the first n_rows_hbm rows, else pinned host memory over PCIe
__device__ __forceinline__ uint32_t walk_fetch_pulled_row(uint32_t n_slices, uint32_t slice_rows, const uint64_t* d_row_slices, uint32_t n_rows_hbm,
                                                          const uint32_t* d_rows_hbm, const uint8_t* d_graph, uint32_t parent, int lane) {
  uint32_t x;
  const uint32_t GAS* hb = nullptr;
  if (n_slices > 1u) {
    const uint32_t sl = parent / slice_rows;                      // (uniform: scalar)
    if (sl < n_slices) hb = (const uint32_t GAS*)slice_base(d_row_slices, sl);
  } else if (parent < n_rows_hbm) hb = (const uint32_t GAS*)d_rows_hbm;
  if (hb) x = hb[(uint64_t)parent * 64u + (uint32_t)lane];
  else {
    x = __builtin_nontemporal_load((const uint32_t GAS*)d_graph + (uint64_t)parent * 64u + (uint32_t)lane);
    asm volatile("; row from host memory");                       // (keeps this load apart from the plain one: merged, the two lose the hint)
  }
  return x;
}

// ---------------------------------------------------------------------------------------------------------------------
// the query is finished: its counters, and -- where the results are a sorted list in LDS (CANON 11: replaces K6 + K7) -- its first k entries
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void walk_finish_query(uint32_t* d_cand_cnt, uint32_t* d_qstats, uint32_t* d_qiters, uint32_t q, uint32_t cc, uint32_t evals,
                                                  uint32_t fetched, uint32_t iter, int lane) {
  if (lane == 0) {
    d_cand_cnt[q] = cc;
    if (d_qstats) { d_qstats[(size_t)q * 2] = evals; d_qstats[(size_t)q * 2 + 1] = fetched; }
    if (d_qiters) d_qiters[q] = iter;
  }
}

__device__ __forceinline__ void walk_write_results(const WaveLds& list, uint32_t n_have, uint64_t* rr_ids_out, float* rr_dists_out, uint32_t k, uint32_t Qt,
                                                   size_t qabs, int lane) {
  uint64_t GAS* ids_out = (uint64_t GAS*)rr_ids_out;
  float GAS* dists_out = (float GAS*)rr_dists_out;
  for (uint32_t r = (uint32_t)lane; r < k; r += WAVE) {
    const bool have = r < n_have;                                 // a short list is padded (CANON 8)
    ids_out[qabs * k + r] = have ? (uint64_t)list.wi[r] : ~0ull;                    // [Q][k] u64
    dists_out[(size_t)r * Qt + qabs] = have ? list.wd[r] : BIG_DIST;                // [rank][Q]
  }
}

#endif
