// bang_search_exact.hip -- the EXACT-DISTANCE search kernel (option distance = 1): the BANG_Base search loop of bang_search.hip with every
// neighbour's distance the exact L2 against its full-precision vector instead of a PQ estimate (the reference's BANG_Exactdistance variant,
// BANG_Exactdistance/parANN.cu:1139-1179), and the results the first k entries of the worklist as the loop leaves it (:1275) -- no re-rank.
// DESIGN.md section 2 lists the two changes (CANON 10, 11); everything else -- filter, eager parent, merge, per-query activity, the L + 49 cap --
// is the loop bang_search.hip runs, and the sort / merge / parent code is the same device code (bang_worklist.h, bang_device.h).
//
//  * Query-resident, self-paced: a wave owns one query from its first iteration to its last (worklist + survivors in LDS, the query in
//    registers), then pulls the next unstarted query from *d_next_query.  Graph and vectors resident in HBM (d_graph = graph entries
//    [vec][u32 degree][u32 id x R]); the vector of node x is the first D elements of its entry.
//  * Distances.  8-bit vectors: G = D / 16 adjacent lanes per survivor, one 16-byte piece each, and the v_dot4 identity
//    sum (a - b)^2 = sum a^2 - 2 sum a b + sum b^2 on integers below 2^24 -- exact, so its float image is what orc_exact_dist's ascending
//    fmaf chain gives (the arithmetic of wave_rerank8).  Float vectors: one lane per survivor runs the ascending fmaf chain over its
//    vector, four 16-byte loads in flight (the arithmetic of wave_rerank_f32).  The query sits in registers in both cases.  Both routines
//    live in bang_exact_dist.h, which the beam form (bang_search_beam.hip) includes too.
//  * The walk's stages that do not depend on the distance -- query hand-out, LDS carve, narrow query load, seed list, row length and the
//    ids-in-range guard, the K5 filter (CANON 3), the K4 parent, the row fetches, counters, results, stamps -- are the functions of
//    bang_wave_walk.h, shared with bang_search_lut.hip and bang_search_beam.hip; this file holds the distance stages and the blocks of its builds.
//  * No pivot table: LDS holds 2L + L/4 + 144 words per wave and the launch is bound by VGPRs.  bang_search_exact_geometry reads the
//    instance's register count and launch bound; the grid is bang_wave_geometry's (bang_wave_host.cpp).
//  * ONE OBJECT PER FORM.  The Makefile builds this file once per form below, each under the flag named with it; the flags give the build its
//    tag (EXACT_TAG), and kernel, geometry function and entry point are named after it (search_exact_wide_pull_kernel, ...), so that the
//    instances of every other build stay the code they are.  The arguments are checked and routed to a build by bang_wave_host.cpp.
//  * WIDE LAYOUTS (BANG_EXACT_WIDE).  D up to 1024; 8-bit vectors with any D / 16.
//    The same loop; what changes is the distance stage (exact_dist_wide below): the survivors' rows are fetched COOPERATIVELY, 64 bytes
//    of 16 rows per wave instruction (four adjacent lanes per row), staged through registers into a 4 KB LDS tile of the wave (64 rows x
//    64 B, 16-byte slots XOR-swizzled so that the tile's ds_write_b128 and ds_read_b128 are free of bank conflicts), and lane i runs
//    survivor i's chain out of the tile while the next tile's loads are in flight.  Tiles are consumed in ascending order, so the chain
//    is orc_exact_dist's.  Float: the query in up to 16 registers.  8-bit: lane l holds the query's 16-byte piece l; a 16-dimension piece
//    is added as an integer (v_dot4) while EVERY survivor's running sum stays <= 2^24 -- all partial sums of the chain are then integers
//    a float holds, the chain rounds nowhere and its value is the integer -- and from the first piece that takes a survivor past 2^24 the
//    wave continues with the float chain, dimension by dimension, from the integer it has (CANON 10).
//
//  * PULLED ROWS (BANG_EXACT_PULL, narrow and wide; row_layout 1).  The same loop; a node's vector comes from the packed table
//    rr_vec_base + id * rr_vec_stride and the parent's adjacency row as 256 bytes -- one dword per lane -- from a slice of the node's
//    HBM-resident rows, from the HBM copy of the first rows or from pinned host memory over PCIe.
//  * FP16 VECTOR TABLE (BANG_EXACT_PULL with BANG_EXACT_F16; ONE instance; rr_vec_f16 = 1).  The pulled-rows loop on a float index whose
//    table holds IEEE fp16 rows (engine option vectors_fp16): D % 8 == 0, D <= 256, the query float in registers as above; a lane reads its
//    survivor's row eight elements per 16-byte load, four loads in flight, and runs the same ascending chain on float(h[j]) - q[j]
//    (exact_dist_f16).  Everything it adds sits under BANG_EXACT_F16.
//  * LABEL FILTERS (BANG_EXACT_LABELS, with and without BANG_EXACT_PULL; the narrow layouts only; entry bang_k_search_exact_labels).
//    The same walk, bit for bit; beside its worklist a wave keeps a second sorted list of capacity L in LDS, the RESULT
//    LIST.  Every survivor carries a 32-bit label word (d_labels[id]) and every query two words {any, all}; in every iteration whose survivors are
//    merged into the worklist, those that match -- and are not in the exclusion bitmap -- are compacted in input order, with the distance bits the
//    walk computed, and go through the same sort_and_merge into the result list.  The results are the first k entries of that list
//    (CANON 18).  Everything it adds sits under BANG_EXACT_LABELS.
//  * RANGE SEARCH (BANG_EXACT_RANGE, with and without BANG_EXACT_PULL; the narrow layouts only; entry bang_k_search_exact_range).  The same walk,
//    bit for bit, and the same results; beside them every query collects a HIT LOG in HBM: in EVERY iteration -- the first with its seed list and the
//    cap iteration, whose survivors are not merged, included -- the survivors with distance <= d_radius[query] that are not in the exclusion bitmap are
//    compacted in input order (__ballot + lanes_below, element 64 behind the first 64) and written, id and distance bits, to the query's row of
//    d_hit_ids / d_hit_dists while positions < cap last; d_offered counts them all.  Two plain vector stores per hit, nothing waits for them, no
//    LDS (CANON 19; bang_range.hip sorts the rows behind the launch).  Everything it adds sits under BANG_EXACT_RANGE.
//
// Reference line numbers: the reference's BANG_Base/bang_search.cu unless a file is named.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "bang_c.h"
#include "bang_internal.h"
#include "bang_device.h"
#include "bang_worklist.h"
#include "bang_exact_dist.h"
#include "bang_wave_walk.h"

// ---------------------------------------------------------------------------------------------------------------------
// this build: one tag from the flags; the kernel, the geometry function and the entry point are named after it
// ---------------------------------------------------------------------------------------------------------------------
#if defined(BANG_EXACT_F16) && (!defined(BANG_EXACT_PULL) || defined(BANG_EXACT_WIDE))
#error "BANG_EXACT_F16 builds the narrow pulled-rows instance only"
#endif
#if defined(BANG_EXACT_LABELS) && defined(BANG_EXACT_WIDE)
#error "BANG_EXACT_LABELS builds the narrow instances only"
#endif
#if defined(BANG_EXACT_LABELS) && defined(BANG_EXACT_F16)
#error "BANG_EXACT_LABELS builds the narrow instances on float / 8-bit rows only"
#endif

#if defined(BANG_EXACT_RANGE) && defined(BANG_EXACT_WIDE)
#error "BANG_EXACT_RANGE builds the narrow instances only"
#endif
#if defined(BANG_EXACT_RANGE) && defined(BANG_EXACT_F16)
#error "BANG_EXACT_RANGE builds the narrow instances on float / 8-bit rows only"
#endif
#if defined(BANG_EXACT_RANGE) && defined(BANG_EXACT_LABELS)
#error "BANG_EXACT_RANGE and BANG_EXACT_LABELS are builds of their own: radii and label filters do not combine"
#endif

#if defined(BANG_EXACT_WIDE) && defined(BANG_EXACT_PULL)
#define EXACT_TAG _wide_pull
#elif defined(BANG_EXACT_WIDE)
#define EXACT_TAG _wide
#elif defined(BANG_EXACT_LABELS) && defined(BANG_EXACT_PULL)
#define EXACT_TAG _labels_pull
#elif defined(BANG_EXACT_LABELS)
#define EXACT_TAG _labels
#define EXACT_ENTRY bang_k_search_exact_labels_hbm
#elif defined(BANG_EXACT_RANGE) && defined(BANG_EXACT_PULL)
#define EXACT_TAG _range_pull
#elif defined(BANG_EXACT_RANGE)
#define EXACT_TAG _range
#define EXACT_ENTRY bang_k_search_exact_range_hbm
#elif defined(BANG_EXACT_F16)
#define EXACT_TAG _pull_f16
#elif defined(BANG_EXACT_PULL)
#define EXACT_TAG _pull
#else
#define EXACT_TAG
#define EXACT_ENTRY bang_k_search_exact_hbm
#endif
#define EXACT_PASTE_(a, b, c) a##b##c
#define EXACT_PASTE(a, b, c) EXACT_PASTE_(a, b, c)
#define EXACT_KERNEL EXACT_PASTE(search_exact, EXACT_TAG, _kernel)
#define EXACT_GEOMETRY EXACT_PASTE(bang_search_exact, EXACT_TAG, _geometry)
#ifndef EXACT_ENTRY                                                // (the two graph-entry builds of the narrow layouts: _hbm behind the tag)
#define EXACT_ENTRY EXACT_PASTE(bang_k_search_exact, EXACT_TAG, )
#endif
#ifdef BANG_EXACT_PULL
#define EXACT_PULL 1
#else
#define EXACT_PULL 0
#endif

struct ExactArgs {
  bang_search_params p;
  uint32_t wave_words;               // LDS words per wave: worklist + scratch
  uint32_t wl_words;                 // LDS words of the worklist (2L + ceil(L/4), rounded to 4)
#ifdef BANG_EXACT_LABELS
  bang_label_filter f;               // labels, the batch's filters, the exclusion bitmap, the matched counts
#endif
#ifdef BANG_EXACT_RANGE
  bang_range_out r;                  // the batch's radii, the exclusion bitmap, the hit log and its counts
#endif
};

#ifdef BANG_EXACT_F16
__device__ __forceinline__ float half_bits_to_float(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }   // exact (v_cvt_f32_f16)

// exact_dist_f32 on rows of IEEE fp16 (D % 8 == 0, <= 256; rows 4-byte aligned): lane i evaluates survivor i0 + i, eight elements per 16-byte
// load, the ascending fmaf chain on float(h[j]) - q[j]
__device__ __forceinline__ void exact_dist_f16(const uint8_t GAS* tab, uint64_t stride, uint32_t D, const uint32_t* sid, uint32_t n,
                                               float* dist, const float (&qr)[4], int lane) {
  constexpr int RF = 4;                                           // 16-byte loads in flight per lane
  for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {                     // (uniform)
    const uint32_t i = i0 + (uint32_t)lane;
    const uint32_t id = sid[i < n ? i : 0u];
    const uint8_t GAS* v = tab + (uint64_t)id * stride;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t jt = (uint32_t)t * 64u;
      if (jt >= D) break;                                         // (uniform)
      const uint32_t dt = D - jt < 64u ? D - jt : 64u;
      for (uint32_t jl = 0; jl < dt; jl += 8u * RF) {             // (uniform)
        u32x4a w[RF];
#pragma unroll
        for (int u = 0; u < RF; ++u) {
          const uint32_t j = jl + 8u * (uint32_t)u;
          w[u] = *(const u32x4a GAS*)(v + 2u * (jt + (j < dt ? j : 0u)));
        }
#pragma unroll
        for (int u = 0; u < RF; ++u) {
          const uint32_t j = jl + 8u * (uint32_t)u;
          if (j < dt) {                                           // (uniform)
            const uint32_t ww[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
#pragma unroll
              for (int b = 0; b < 2; ++b) {
                const float qv = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(qr[t]), (int)(j + 2u * (uint32_t)d + (uint32_t)b)));
                const float diff = half_bits_to_float(b ? ww[d] >> 16 : ww[d] & 0xFFFFu) - qv;      // vector - query, as exact_dist_f32
                acc = __builtin_fmaf(diff, diff, acc);            // ascending dimension
              }
            }
          }
        }
      }
    }
    if (i < n) dist[i] = acc;
  }
}
#endif

#ifdef BANG_EXACT_WIDE
// ---------------------------------------------------------------------------------------------------------------------
// wide layouts: rows fetched cooperatively through an LDS tile (one per wave: 64 rows x 64 bytes)
// ---------------------------------------------------------------------------------------------------------------------
#define EXACT_TILE_WORDS 1024u
#define EXACT_QREGS 16               // float query registers: 64 dimensions each

// word offset of 16-byte piece c (0..3) of row s (0..63) in the tile.  ds_read_b128 banks over 256 B (16 slots) in four 16-lane groups
// {0-3,12-15,20-27} {4-11,16-19,28-31} {32-35,44-47,52-59} {36-43,48-51,60-63}: lane s reads slot 4 (s & 3) + (c ^ (s >> 2 & 3)), and
// s >> 2 & 3 takes four values in every group -- 16 slots, no conflict.  ds_write_b128 banks over 128 B in groups of 8 adjacent lanes =
// two adjacent rows x four pieces: 8 slots, no conflict.
typedef uint32_t u32x4t __attribute__((ext_vector_type(4)));     // 16-byte aligned: the tile's slots (ds_write_b128 / ds_read_b128)
__device__ __forceinline__ uint32_t tile_word(uint32_t s, uint32_t c) { return 16u * s + 4u * (c ^ ((s >> 2) & 3u)); }

__device__ __forceinline__ int rdlane(int v, uint32_t l) { return __builtin_amdgcn_readlane(v, (int)l); }

// exact distances of the n survivors (ids in LDS: sid[0, n)) -> dist[0, n) in LDS.  DT == BANG_F32: qr[t] holds query element 64 t + lane.
// 8-bit: qw = the query's 16-byte piece `lane`, qq the sum of its squares.  Every lane of the wave executes.
template <int DT>
__device__ __forceinline__ void exact_dist_wide(const uint8_t GAS* graph, uint64_t entry_len, uint32_t vec_bytes, uint32_t D, const uint32_t* sid,
                                                uint32_t n, float* dist, uint32_t* tile, const float (&qr)[EXACT_QREGS], u32x4a qw, int qq, int lane) {
  constexpr bool SG = (DT == BANG_I8);
  const uint32_t T = (vec_bytes + 63u) >> 6;                      // 64-byte tiles per row
  const uint32_t ls = (uint32_t)lane >> 2, lc = (uint32_t)lane & 3u;   // fetch: row ls + 16 u, piece lc
  for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {                     // (uniform; a second pass for the 65th id of the seed list only)
    const uint32_t np = n - i0 < WAVE ? n - i0 : WAVE;
    u32x4a st[4] = {};
    auto fetch = [&](uint32_t t) {                                // tile t of up to 64 rows: four loads of 16 rows x 64 B
      uint32_t o = 64u * t + 16u * lc;
      if (o >= vec_bytes) o = 0;                                  // (behind the vector's end: a piece again, never used)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = 16u * (uint32_t)u + ls;                // (the ids are re-read from LDS per tile: four registers less across the chain)
        if (16u * (uint32_t)u < np) st[u] = *(const u32x4a GAS*)(graph + (uint64_t)sid[i0 + (i < np ? i : 0u)] * entry_len + o);   // (uniform)
      }
    };
    auto turn = [&](uint32_t t) {                                 // staged tile t -> LDS; tile t + 1 requested
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (16u * (uint32_t)u < np) *(u32x4t*)(tile + tile_word(16u * (uint32_t)u + ls, lc)) = (u32x4t){st[u].x, st[u].y, st[u].z, st[u].w};
      wave_sync();
      if (t + 1u < T) fetch(t + 1u);
    };
    auto piece = [&](int c) { return *(const u32x4t*)(tile + tile_word((uint32_t)lane, (uint32_t)c)); };   // this lane's row
    fetch(0);
    float acc = 0.0f;
    if (DT == BANG_F32) {
      for (uint32_t tq = 0; 64u * tq < D; ++tq) {                 // (uniform; qr[tq]: a register picked by index, s_set_gpr_idx)
        const int qcur = (int)__float_as_uint(qr[tq]);
        for (uint32_t tt = 0; tt < 4u; ++tt) {
          const uint32_t t = 4u * tq + tt;
          if (t >= T) break;                                      // (uniform)
          turn(t);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (16u * t + 4u * (uint32_t)c < D) {                 // (uniform; D % 4 == 0)
              const u32x4t w = piece(c);
              const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
              for (int d = 0; d < 4; ++d) {
                const float qv = __uint_as_float((uint32_t)rdlane(qcur, 16u * tt + 4u * (uint32_t)c + (uint32_t)d));
                const float diff = __uint_as_float(ww[d]) - qv;   // parANN.cu:1139-1179 / orc_exact_dist: vector - query
                acc = __builtin_fmaf(diff, diff, acc);            // ascending dimension
              }
            }
          }
        }
      }
    } else {
      int sum = 0;                                                // the chain's value while it is an integer <= 2^24
      bool chain = false;                                         // (uniform) the wave has left the integers
      const uint32_t P = D >> 4;                                  // 16-byte pieces per vector
      for (uint32_t t = 0; t < T; ++t) {
        turn(t);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const uint32_t pc = 4u * t + (uint32_t)c;
          if (pc < P) {                                           // (uniform)
            const u32x4t w = piece(c);
            const uint32_t qx = (uint32_t)rdlane((int)qw.x, pc), qy = (uint32_t)rdlane((int)qw.y, pc), qz = (uint32_t)rdlane((int)qw.z, pc),
                           qv = (uint32_t)rdlane((int)qw.w, pc);
            if (!chain) {
              const int vv = xdot4<SG>(w.x, w.x, xdot4<SG>(w.y, w.y, xdot4<SG>(w.z, w.z, xdot4<SG>(w.w, w.w, rdlane(qq, pc)))));
              const int vq = xdot4<SG>(w.x, qx, xdot4<SG>(w.y, qy, xdot4<SG>(w.z, qz, xdot4<SG>(w.w, qv, 0))));
              const int next = sum + vv - 2 * vq;                 // < 2^31: 1024 x 255^2 = 66 585 600
              if (__ballot((uint32_t)lane < np && next > (1 << 24)) == 0ull) { sum = next; continue; }
              chain = true;
              acc = (float)sum;
            }
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w}, qs[4] = {qx, qy, qz, qv};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                const int vb = SG ? (int)(int8_t)(ww[d] >> (8 * b)) : (int)((ww[d] >> (8 * b)) & 255u);
                const int qb = SG ? (int)(int8_t)(qs[d] >> (8 * b)) : (int)((qs[d] >> (8 * b)) & 255u);
                const float diff = (float)(vb - qb);              // orc_exact_dist: the subtraction in int, then to float
                acc = __builtin_fmaf(diff, diff, acc);
              }
            }
          }
        }
      }
      if (!chain) acc = (float)sum;
    }
    if ((uint32_t)lane < np) dist[i0 + (uint32_t)lane] = acc;
  }
}
// the float instance keeps 16 query registers across the whole loop and needs a few registers more than the 128 that 16 waves per CU leave a
// wave: 12 waves per CU, no scratch (bang_search_exact_wide_geometry reads both figures off the instance)
#define EXACT_MAX_THREADS(DT) ((DT) == BANG_F32 ? 768 : 1024)
#define EXACT_EXTRA_WORDS EXACT_TILE_WORDS                        // the wave's row tile, behind its scratch
#else
#define EXACT_MAX_THREADS(DT) 1024
#define EXACT_EXTRA_WORDS 0u
#endif

// PULLED ROWS (EXACT_PULL).  row_layout 1: the vectors in the packed table rr_vec_base (stride rr_vec_stride), the adjacency lists as 256-byte
// rows of 64 ids (ids first, BANG_ADJ_PAD behind them) in pinned host memory (d_graph), in the HBM copy of the first rows (d_rows_hbm) or in a
// slice of the node's HBM-resident rows (d_row_slices), read as bang_search.hip's self-paced form reads them.

template <int DT>
__global__ __launch_bounds__(EXACT_MAX_THREADS(DT)) void EXACT_KERNEL(const ExactArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t xlds[];
  const bang_search_params& p = a.p;
  const int lane = lane_id();
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t nwaves = blockDim.x >> 6;
  const uint32_t L = p.L, medoid = p.medoid, cap_iter = p.cap_iter, R = p.R, n_nodes = p.n_nodes;
  const uint32_t cand_stride = L + BANG_EXTRA_ITERS;
#if EXACT_PULL
  const uint8_t GAS* graph = (const uint8_t GAS*)p.rr_vec_base;   // the vectors: node x's at graph + x * entry_len
  const uint64_t entry_len = p.rr_vec_stride;
#else
  const uint8_t GAS* graph = (const uint8_t GAS*)p.d_graph;
  const uint64_t entry_len = p.entry_len;
#endif
  uint32_t* wbase = xlds + (size_t)wave * a.wave_words;
#ifdef BANG_EXACT_LABELS
  const WalkLds w = walk_lds(wbase, L, 2u * a.wl_words);          // [worklist][result list][scratch]
#else
  const WalkLds w = walk_lds(wbase, L, a.wl_words);
#endif
  const WaveLds& s = w.s;
  float* sdist = w.sdist;
  uint32_t* sc = w.sc;
#ifdef BANG_EXACT_LABELS
  // the result list: a second sorted list of capacity L behind the worklist; it sorts and merges through the same scratch words, after the worklist's
  // merge is done (the survivors' ids and distances are in registers by then).  Its visited flags are written and never read.
  const WaveLds rl = walk_lds(wbase + a.wl_words, L, a.wl_words).s;
  const uint32_t GAS* labels = (const uint32_t GAS*)a.f.d_labels;
  const uint32_t GAS* excluded = (const uint32_t GAS*)a.f.d_excluded;    // or null
#endif
#ifdef BANG_EXACT_RANGE
  const uint32_t GAS* excluded = (const uint32_t GAS*)a.r.d_excluded;    // or null
  const uint32_t hit_cap = a.r.cap;
#endif
  walk_stamp_start(p.d_ktime);
  const uint32_t total_waves = gridDim.x * nwaves;
  const uint32_t gw = blockIdx.x * nwaves + wave;

  for (bool first_q = true;; first_q = false) {
    const uint32_t q = walk_next_query(first_q, gw, total_waves, p.d_next_query, lane);
    if (q >= p.Q) break;
    const size_t qabs = (size_t)p.rr_q0 + q;
    uint32_t GAS* bloom = (uint32_t GAS*)p.d_bloom + (size_t)q * BANG_BF_WORDS;

    // the raw query, in registers
    const uint32_t D = p.rr_D;
#ifdef BANG_EXACT_WIDE
    u32x4a qw = {0u, 0u, 0u, 0u};
    int qq = 0;
    float qr[EXACT_QREGS];
    if (DT == BANG_F32) {
      const float GAS* qsrc = (const float GAS*)p.rr_queries + qabs * D;
#pragma unroll
      for (int t = 0; t < EXACT_QREGS; ++t) { const uint32_t j = (uint32_t)t * 64u + (uint32_t)lane; qr[t] = qsrc[j < D ? j : 0u]; }
    } else {
#pragma unroll
      for (int t = 0; t < EXACT_QREGS; ++t) qr[t] = 0.0f;
      qw = *(const u32x4a GAS*)((const uint8_t GAS*)p.rr_queries + qabs * D + 16u * ((uint32_t)lane < (D >> 4) ? (uint32_t)lane : 0u));
      qq = query_sumsq<DT == BANG_I8>(qw);
    }
#else
    const NarrowQuery nq = walk_load_query_narrow<DT>(p.rr_queries, qabs, D, lane);
#endif

    uint32_t iter = 1, w_n = 0, cc = 1, mark = 0x01010101u, evals = 0, fetched = 0;
#ifdef BANG_EXACT_LABELS
    const uint32_t f_any = uni(((const uint32_t GAS*)a.f.d_filters)[2u * qabs]), f_all = uni(((const uint32_t GAS*)a.f.d_filters)[2u * qabs + 1u]);
    uint32_t r_n = 0, matched = 0;
    float r_tail = 0.0f;                          // the result list's last distance (read while r_n > 0 only)
#endif
#ifdef BANG_EXACT_RANGE
    // CANON 19: the query's radius (wave-uniform), its row of the hit log (64-bit address arithmetic) and the running count of hits offered to it
    const float radius = __uint_as_float(uni(__float_as_uint(((const float GAS*)a.r.d_radius)[qabs])));
    uint32_t GAS* hit_ids = (uint32_t GAS*)a.r.d_hit_ids + (uint64_t)qabs * hit_cap;
    float GAS* hit_dists = (float GAS*)a.r.d_hit_dists + (uint64_t)qabs * hit_cap;
    uint32_t offered = 0;
#endif
    WlHead head = walk_empty_head();
    const WalkSeed seed = walk_begin_query(p.d_cand_ids, p.d_seed, q, cand_stride, medoid, lane);
    uint32_t cnt_in = seed.cnt, x0 = seed.x0;
    const uint32_t x1 = seed.x1;
    bool have_row = true;

    for (;;) {
      const bool first = (iter == 1);
      // ---------------- K5: filter
#if EXACT_PULL
      const uint32_t ci = walk_row_len_pulled(have_row, cnt_in, first, R, n_nodes, x0, x1, p.d_abort, lane);
#else
      const uint32_t ci = walk_row_len_entry(have_row, cnt_in, first, R, n_nodes, x0, x1, p.d_abort, lane);
#endif
      fetched += ci;
      const WalkSurvivors sv = walk_filter(bloom, ci, x0, x1, sc, lane);
      const uint32_t n = sv.n, sid0 = sv.sid0, sid1 = sv.sid1;
      evals += n;
#ifdef BANG_EXACT_LABELS
      // the survivors' label words, and their words of the exclusion bitmap: requested here, so that they travel with the vectors (every survivor id
      // is < n_nodes: the check above, and bang_k_search_exact_labels refuses n_nodes == 0)
      uint32_t lab0 = 0, lab1 = 0, ex0 = 0, ex1 = 0;
      if ((uint32_t)lane < n) { lab0 = labels[sid0]; if (excluded) ex0 = excluded[sid0 >> 5]; }
      if (lane == 0 && n > 64) { lab1 = labels[sid1]; if (excluded) ex1 = excluded[sid1 >> 5]; }
#endif
#ifdef BANG_EXACT_RANGE
      // the survivors' words of the exclusion bitmap: requested here, so that they travel with the vectors (with a bitmap n_nodes != 0 -- refused
      // otherwise by bang_k_search_exact_range -- and every survivor id is < n_nodes: the check above)
      uint32_t ex0 = 0, ex1 = 0;
      if (excluded) {                                             // (uniform)
        if ((uint32_t)lane < n) ex0 = excluded[sid0 >> 5];
        if (lane == 0 && n > 64) ex1 = excluded[sid1 >> 5];
      }
#endif

      // ---------------- exact distances (CANON 10: replaces K2) ----------------
      if (n > 0) {
#ifdef BANG_EXACT_WIDE
        exact_dist_wide<DT>(graph, entry_len, p.vec_bytes, D, sc, n, sdist, w.scratch + WAVE_SCRATCH_WORDS, qr, qw, qq, lane);
#else
#ifdef BANG_EXACT_F16
        if (DT == BANG_F32) exact_dist_f16(graph, entry_len, D, sc, n, sdist, nq.qr, lane);
#else
        if (DT == BANG_F32) exact_dist_f32(graph, entry_len, D, sc, n, sdist, nq.qr, lane);
#endif
        else exact_dist8<DT == BANG_I8>(graph, entry_len, nq.G, sc, n, sdist, nq.qw, nq.qq, lane);
#endif
      }
      wave_sync();
      const float d0 = ((uint32_t)lane < n) ? sdist[lane] : BIG_DIST;
      const float d1 = (lane == 0 && n > 64) ? sdist[64] : BIG_DIST;
      wave_sync();
#ifdef BANG_EXACT_RANGE
      // ---------------- CANON 19: the hits of this iteration (every iteration: the cap iteration too), in input order, to the query's hit log.  A plain
      // float compare on the distance bits the walk computed (a NaN or negative radius admits nothing); fire-and-forget stores below the cap
      {
        const bool ht0 = (uint32_t)lane < n && d0 <= radius && ((ex0 >> (sid0 & 31u)) & 1u) == 0u;
        const bool ht1 = lane == 0 && n > 64 && d1 <= radius && ((ex1 >> (sid1 & 31u)) & 1u) == 0u;
        const uint64_t hm0 = __ballot(ht0), hm1 = __ballot(ht1);
        const uint32_t nh0 = (uint32_t)__popcll(hm0);
        const uint32_t at0 = offered + lanes_below(hm0), at1 = offered + nh0;             // (element 64 behind the first 64)
        if (ht0 && at0 < hit_cap) { hit_ids[at0] = sid0; hit_dists[at0] = d0; }
        if (ht1 && at1 < hit_cap) { hit_ids[at1] = sid1; hit_dists[at1] = d1; }
        offered += nh0 + (uint32_t)__popcll(hm1);
      }
#endif

      // ---------------- K4: parent
      uint32_t parent = 0;
      bool found = false;
      walk_parent(s, head, n, sid0, sid1, d0, d1, first, w_n, medoid, mark, cc, parent, found, lane);

      // ---------------- hand the parent over: its adjacency row is requested now and travels during the sort/merge
      if (found && iter < cap_iter) {
#if EXACT_PULL
        x0 = walk_fetch_pulled_row(p.n_slices, p.slice_rows, p.d_row_slices, p.n_rows_hbm, p.d_rows_hbm, p.d_graph, parent, lane);
        cnt_in = 64u;                                             // counted when the row is consumed
#else
        const WalkEntryRow row = walk_fetch_entry_row(graph, entry_len, p.vec_bytes, R, parent, lane);
        cnt_in = row.cnt; x0 = row.x;
#endif
      }
      if (found && lane == 0) p.d_cand_ids[(size_t)q * cand_stride + cc - 1u] = parent;      // :1451-1458

      // ---------------- K3a + K3b: sort the survivors, merge them into the worklist (not at the cap: CANON 6) ----------------
      if (n > 0 && iter < cap_iter) w_n = sort_and_merge(s, n, d0, sid0, d1, sid1, iter, w_n, L, medoid, mark, head.tail, lane);
#ifdef BANG_EXACT_LABELS
      // ---------------- CANON 18: the matching survivors of a merged iteration, in input order, go through the same K3a + K3b into the result list
      if (n > 0 && iter < cap_iter) {
        const bool mt0 = (uint32_t)lane < n && (f_any == 0u || (lab0 & f_any) != 0u) && (lab0 & f_all) == f_all && ((ex0 >> (sid0 & 31u)) & 1u) == 0u;
        const bool mt1 = lane == 0 && n > 64 && (f_any == 0u || (lab1 & f_any) != 0u) && (lab1 & f_all) == f_all && ((ex1 >> (sid1 & 31u)) & 1u) == 0u;
        const uint64_t mm0 = __ballot(mt0), mm1 = __ballot(mt1);
        const uint32_t nm0 = (uint32_t)__popcll(mm0), nm = nm0 + (uint32_t)__popcll(mm1);
        matched += nm;
        if (nm > 0) {                                             // (uniform)
          // (the worklist's merge has left the scratch words: its last LDS access is behind a wave_sync)
          if (mt0) { const uint32_t at = lanes_below(mm0); sdist[at] = d0; sc[at] = sid0; }
          if (mt1) { sdist[nm0] = d1; sc[nm0] = sid1; }
          wave_sync();
          const float cd0 = ((uint32_t)lane < nm) ? sdist[lane] : BIG_DIST;
          const uint32_t ci0 = ((uint32_t)lane < nm) ? sc[lane] : 0u;
          const float cd1 = (lane == 0 && nm > 64) ? sdist[64] : BIG_DIST;
          const uint32_t ci1 = (lane == 0 && nm > 64) ? sc[64] : 0u;
          wave_sync();
          // an empty list takes the iteration-1 path (the first min(nm, L) sorted entries); r_tail is the list's own last distance
          r_n = sort_and_merge(rl, nm, cd0, ci0, cd1, ci1, r_n == 0u ? 1u : 2u, r_n, L, medoid, mark, r_tail, lane);
          r_tail = __uint_as_float(uni(__float_as_uint(rl.wd[r_n - 1u])));     // (nm > 0: r_n >= 1)
        }
      }
#endif

      // a query is active while it has a parent or unmerged survivors (CANON 4); the loop ends at the cap (:950-956)
      if ((!found && n == 0) || iter == cap_iter) break;
      ++iter;
      have_row = found;
      head = worklist_head(s, w_n, lane);
    }

    // ---------------- the query is finished: counters, then the results straight from the worklist (CANON 11: replaces K6 + K7)
    walk_finish_query(p.d_cand_cnt, p.d_qstats, p.d_qiters, q, cc, evals, fetched, iter, lane);
#ifdef BANG_EXACT_RANGE
    if (lane == 0) ((uint32_t GAS*)a.r.d_offered)[qabs] = offered;
#endif
#ifdef BANG_EXACT_LABELS
    if (lane == 0 && a.f.d_matched) ((uint32_t GAS*)a.f.d_matched)[qabs] = matched;
    walk_write_results(rl, r_n, p.rr_ids_out, p.rr_dists_out, p.rr_k, p.rr_Q_total, qabs, lane);   // CANON 18: the result list, not the worklist
#else
    // walk_write_results(s, w_n, ...), written out: inlined from the header the loop's two conditional stores become one store of a phi, and that
    // moves the narrow graph-entry and range instances from 97-98 VGPRs to 95-96 -- another allocation, another number of waves per CU
    // (profiles/wave_walk_device_code.md)
    const uint32_t k = p.rr_k, Qt = p.rr_Q_total;
    uint64_t GAS* ids_out = (uint64_t GAS*)p.rr_ids_out;
    float GAS* dists_out = (float GAS*)p.rr_dists_out;
    for (uint32_t r = (uint32_t)lane; r < k; r += WAVE) {
      const bool have = r < w_n;                                  // a short worklist is padded (CANON 8)
      ids_out[qabs * k + r] = have ? (uint64_t)s.wi[r] : ~0ull;                     // [Q][k] u64
      dists_out[(size_t)r * Qt + qabs] = have ? s.wd[r] : BIG_DIST;                 // [rank][Q]
    }
#endif
    wave_sync();                                                  // (the list is read before the next query overwrites it)
  }
  walk_stamp_end(p.d_ktime);
}

// ---------------------------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------------------------
static const void* exact_instance(int dtype) {
#ifndef BANG_EXACT_F16                                             // (float queries on fp16 rows: the one instance of that build)
  if (dtype == BANG_U8) return (const void*)EXACT_KERNEL<BANG_U8>;
  if (dtype == BANG_I8) return (const void*)EXACT_KERNEL<BANG_I8>;
#endif
  if (dtype == BANG_F32) return (const void*)EXACT_KERNEL<BANG_F32>;
  return nullptr;
}
static WaveKernelAttr exact_attr[3];                               // per instance: its figures, per device

// LDS words per wave: worklist + scratch (+ the row tile of the wide builds); the label-filter builds hold a second list, the result list --
// 2 (2L + L/4) + 144 words, 16 waves per CU up to L = 512
#ifdef BANG_EXACT_LABELS
#define EXACT_LISTS 2u
#else
#define EXACT_LISTS 1u
#endif
static uint32_t exact_wave_words(uint32_t L) { return EXACT_LISTS * wave_wl_words(L) + WAVE_SCRATCH_WORDS + EXACT_EXTRA_WORDS; }

// The grid of a launch (bang_wave_geometry on the instance's own figures).  The three narrow instances compile to 97-98 VGPRs and no scratch (the
// merge of bang_worklist.h keeps up to 8 worklist entries per lane in registers): 104 allocated, 4 waves per SIMD, 16 per CU -- one workgroup of
// 16 waves per CU; LDS holds 16 waves' worklists up to L = 512.  The wide instances (at most 128 VGPRs, no scratch: DESIGN.md section 4.6) run 16
// waves per CU as well, up to L = 704.  The label-filter builds compile to 114-118 VGPRs, no scratch: 120 allocated, 16 waves per CU again.  The
// pulled-rows builds: 99-100 VGPRs narrow, 108-109 / 134 wide, no scratch -- the same waves per CU, read off the pulled instance.  The range builds
// (hit log in HBM, no LDS added): 97-99 VGPRs with graph entries, 99-100 with pulled rows, no scratch -- 104 allocated, 16 waves per CU, LDS as
// the plain builds.
extern "C" int EXACT_GEOMETRY(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves) {
  if (!workgroups || !waves || Q == 0) return BANG_ERR_ARG;
  const void* k = exact_instance(dtype);
  if (!k || L == 0 || L > BANG_MAX_L) { bang_set_error("distance = 1: bad dtype / L"); return BANG_ERR_ARG; }
  const int rc = wave_kernel_geometry(k, exact_attr[dtype], exact_wave_words(L) * 4u, Q, max_wgs, max_waves, workgroups, waves);
  if (rc == BANG_ERR_UNSUPPORTED) bang_set_error("distance = 1: one wave's worklist does not fit LDS at L=%u", L);
  return rc;
}

// one launch of this translation unit's instances (the arguments are checked: bang_k_search_exact)
#if defined(BANG_EXACT_LABELS)
static int exact_launch(const bang_search_params* p, const bang_label_filter* f, void* stream) {
#elif defined(BANG_EXACT_RANGE)
static int exact_launch(const bang_search_params* p, const bang_range_out* r, void* stream) {
#else
static int exact_launch(const bang_search_params* p, void* stream) {
#endif
  uint32_t grid_n = 0, waves = 0;
  const int rc = EXACT_GEOMETRY((int)p->rr_dtype, p->L, p->Q, p->max_wgs, p->max_waves, &grid_n, &waves);
  if (rc != BANG_OK) return rc;
  ExactArgs a;
  a.p = *p;
  a.wl_words = wave_wl_words(p->L);
  a.wave_words = exact_wave_words(p->L);
#ifdef BANG_EXACT_LABELS
  a.f = *f;
#endif
#ifdef BANG_EXACT_RANGE
  a.r = *r;
#endif
  return wave_kernel_launch(exact_instance((int)p->rr_dtype), exact_attr[p->rr_dtype], grid_n, waves, a.wave_words * 4u, stream, a);
}

// This build's entry point (EXACT_ENTRY: bang_internal.h), called by bang_k_search_exact / bang_k_search_exact_labels (bang_wave_host.cpp) with
// the arguments checked; what the kernel's own addressing rests on is looked at once more.
#if defined(BANG_EXACT_RANGE)
extern "C" int EXACT_ENTRY(const bang_search_params* p, const bang_range_out* r, void* stream) {
  if (!p || !r || p->row_layout != (uint32_t)EXACT_PULL ||
      !bang_search_can_rerank((int)p->rr_dtype, p->rr_D, EXACT_PULL ? p->rr_vec_stride : p->entry_len, 0)) return BANG_ERR_ARG;
  if (!r->d_radius || !r->d_hit_ids || !r->d_hit_dists || !r->d_offered || r->cap == 0u || r->cap > BANG_RANGE_MAX_HITS ||
      (r->d_excluded && p->n_nodes == 0u)) return BANG_ERR_ARG;
  return exact_launch(p, r, stream);
}
#elif defined(BANG_EXACT_LABELS)
extern "C" int EXACT_ENTRY(const bang_search_params* p, const bang_label_filter* f, void* stream) {
  if (!p || !f || p->row_layout != (uint32_t)EXACT_PULL ||
      !bang_search_can_rerank((int)p->rr_dtype, p->rr_D, EXACT_PULL ? p->rr_vec_stride : p->entry_len, 0)) return BANG_ERR_ARG;
  if (!f->d_labels || !f->d_filters || p->n_nodes == 0u) return BANG_ERR_ARG;
  return exact_launch(p, f, stream);
}
#else
extern "C" int EXACT_ENTRY(const bang_search_params* p, void* stream) {
  if (!p) return BANG_ERR_ARG;
#if defined(BANG_EXACT_F16)
  if (p->row_layout != 1u || p->rr_vec_f16 != 1u || p->rr_dtype != BANG_F32 || p->rr_D % 8u != 0u || p->rr_D > 256u || (p->rr_vec_stride & 3u) ||
      p->rr_vec_stride < 2ull * p->rr_D) return BANG_ERR_ARG;
#elif EXACT_PULL
  if (p->row_layout != 1u || !bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->rr_vec_stride)) return BANG_ERR_ARG;
#else
  if (!bang_search_exact_supported((int)p->rr_dtype, p->rr_D, p->entry_len)) return BANG_ERR_ARG;
#endif
  return exact_launch(p, stream);
}
#endif
