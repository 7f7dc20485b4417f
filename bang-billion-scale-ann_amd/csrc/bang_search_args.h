// bang_search_args.h -- what the host side of a search-kernel launch (bang_search_host.cpp, plain C++) and the kernel (bang_search.hip) have to
// agree on: the kernel's argument block, the LDS budget of a wave, and the list of compiled PQ layouts.  Compiles as host C++ and as HIP.  Not public.
#ifndef BANG_SEARCH_ARGS_H_
#define BANG_SEARCH_ARGS_H_

#include <stddef.h>
#include <stdint.h>

#include "bang_c.h"

#ifdef __HIPCC__
#define BANG_HD __host__ __device__
#else
#define BANG_HD
#endif

// The compiled PQ layouts (PSZ floats per pivot entry, NDW code dwords per row: mp = 4 NDW chunks), ONE list for every switch over them
// (search_dispatch, launch_front, bang_k_pqdist_stream) and for the host's answers (bang_pq_layout, bang_search_wf_has_instance).
// LDS need of a pivot table = NDW*4*256*PSZ*4 B.  Ascending NDW within a PSZ: bang_pq_layout takes the first that holds the chunks.
#define BANG_PQ_LAYOUTS(X) X(1, 8) X(1, 16) X(1, 24) X(1, 32) X(2, 8) X(2, 16) X(2, 18) X(2, 19) X(4, 4) X(4, 8) X(8, 2) X(8, 4)
// ... and those the search kernel and the streaming K2 are compiled for.  Build switch BANG_DEV_ONLY_218 -- development builds (ISA dumps, quick
// A/B libraries): the SIFT1B layout only.  (Like BANG_LONG_MAXT below it has to reach the host objects too: pass both through EXTRA_CXXFLAGS.)
#ifdef BANG_DEV_ONLY_218
#define BANG_SEARCH_LAYOUTS(X) X(2, 18)
#else
#define BANG_SEARCH_LAYOUTS(X) BANG_PQ_LAYOUTS(X)
#endif
constexpr uint32_t bang_layout_key(uint32_t psz, uint32_t ndw) { return psz * 100u + ndw; }
// exact-size pivot table: compiled for the two layouts of the BASELINE configs (128 dims in 70 chunks: 58 x 2 + 12 x 1;
// 96 dims in 74 chunks: 22 x 2 + 52 x 1) -- the number of leading 2-dim chunks of the layout's instance, 0 where there is none
constexpr int bang_layout_nhi(int psz, int ndw) { return (psz == 2 && ndw == 18) ? 58 : (psz == 2 && ndw == 19) ? 22 : 0; }

// floats of the packed pivot table (multiple of 4: it is staged into LDS with 16-byte copies)
static inline uint32_t pivot_table_floats(uint32_t psz, uint32_t mp, uint32_t nhi) {
  if (psz == 2 && nhi != 0) return ((nhi * 512u + (mp - nhi) * 256u + 3u) & ~3u) + 4u;
  return mp * 256u * psz;
}

// What an ITERATION needs of the launch's arguments (as opposed to a query: KARG) -- where the code table, the filters, the candidate log and the next
// adjacency row are -- travels in the LANES OF ONE VECTOR REGISTER of the wave (lane k = dword k of this block, loaded once at the wave's start) and is
// read with v_readlane where it is used: no memory round trip.  History of these ~24 dwords: as ordinary kernel arguments they are loop-invariant, get
// hoisted and take scalar registers the search loop has none to spare of (106 of 106: spills, or re-loads from the kernarg segment the compiler places
// where it pleases: d_bloom, summ_iters and cap_iter were re-read on the chain of every iteration); read from the kernarg segment one by one where the
// branches need them (round 5: KARG) the hand-over alone was five dependent scalar-cache round trips between "the parent is known" and "its row is
// requested" (as one block: 1 250-query SIFT1B-shape shard 1.63 -> 1.53 ms, 10 K batch 8.32 -> 8.15).  The register passes through an empty asm in front
// of each use site so that the reads stay THERE (a v_readlane of a loop-invariant register is loop-invariant too and would be hoisted back into scalar
// registers).  Pointers rebuilt from these dwords are typed GAS (bang_device.h): generic, every access through them is a flat_ instruction.
struct IterArgs {
  const uint8_t* d_codes; uint32_t n_nodes, prio;                                               // dwords 0-1, 2, 3
  uint32_t* d_cand_ids; const uint8_t* d_graph; uint64_t entry_len;                             // 4-5, 6-7, 8-9
  uint32_t vec_bytes, row_layout, n_rows_hbm, n_slices;                                         // 10, 11, 12, 13
  const uint32_t* d_rows_hbm; const uint64_t* d_row_slices;                                     // 14-15, 16-17
  uint32_t slice_rows, summ_iters;                                                              // 18, 19
  uint32_t* d_bloom; uint32_t cap_iter, n_pad;                                                   // 20-21, 22, 23
};
enum { IA_CODES = 0, IA_N_NODES = 2, IA_PRIO = 3, IA_CAND_IDS = 4, IA_GRAPH = 6, IA_ENTRY_LEN = 8, IA_VEC_BYTES = 10, IA_ROW_LAYOUT = 11, IA_N_ROWS_HBM = 12,
       IA_N_SLICES = 13, IA_ROWS_HBM = 14, IA_ROW_SLICES = 16, IA_SLICE_ROWS = 18, IA_SUMM_ITERS = 19, IA_BLOOM = 20, IA_CAP_ITER = 22, IA_N_PAD = 23, IA_DWORDS = 24 };
static_assert(sizeof(IterArgs) == 4 * IA_DWORDS && offsetof(IterArgs, d_cand_ids) == 4 * IA_CAND_IDS && offsetof(IterArgs, vec_bytes) == 4 * IA_VEC_BYTES &&
              offsetof(IterArgs, d_rows_hbm) == 4 * IA_ROWS_HBM && offsetof(IterArgs, slice_rows) == 4 * IA_SLICE_ROWS && offsetof(IterArgs, d_bloom) == 4 * IA_BLOOM && offsetof(IterArgs, cap_iter) == 4 * IA_CAP_ITER && offsetof(IterArgs, n_pad) == 4 * IA_N_PAD,
              "IterArgs dword map");
struct SearchArgs {
  bang_search_params p;
  IterArgs iter __attribute__((aligned(16)));
  uint32_t lds_piv_floats;
  uint32_t wave_words;       // LDS words per wave: nctx worklists + 144 scratch (+ 32 parked context state when nctx == 2)
  uint32_t wl_words;         // LDS words of one worklist (2L + ceil(L/4), rounded to 4)
  uint32_t nctx;             // query contexts per wave: 1, or 2 in the host-paced form
  uint32_t gs;               // host-paced form: waves per pacing group (a workgroup's waves advance in lock-step per GROUP)
};

// Code rows are fetched cooperatively (CoopFetch, bang_device.h) from three 16-byte pieces per row on (rows of 12+ code dwords,
// m > 44): two-piece rows (m = 32) gain nothing in the kernel (2.69 vs 2.70 ms on SIFT1M-like) and would only lose LDS to the staging
// area.  The host-paced instances do so for the long-row layouts only (12 waves x 168 VGPRs, with the filter summary).
BANG_HD constexpr bool search_coop(int ndw, bool host_paced) { return ndw >= 12 && (!host_paced || ndw >= 16); }
// self-paced instances with the speculative row request (SPEC) exist for the long-row layouts of the BASELINE configs (70 / 74 chunks: 168-VGPR
// instances); the 128-VGPR instance of the 32-chunk layout measured 2-5 % slower with it
BANG_HD constexpr bool search_has_spec(int ndw) { return ndw == 18 || ndw == 19; }
// The instances whose hand-over reads adjacency rows kept in the code table's padding (option rows_pad, bang_pad_rows.h; n_pad of IterArgs): the
// self-paced instances of the 70-chunk layout for dword-aligned rows, at a code stride of 128 bytes.  The 74-chunk instances pay for the same branch
// with 72-112 B of scratch per lane (profiles/rows_pad.md) and stay, like every other instance, the code they were without the option
BANG_HD constexpr bool search_has_pad_rows(int ndw, bool host_paced) { return !host_paced && ndw == 18; }

// MAXT: threads per workgroup the instance is compiled for -- 1024 (16 waves, 128 VGPRs each) or, for the instances of the long code
// rows (>= 64 chunks), 768 (12 waves, 168 VGPRs each).  Build switch BANG_LONG_MAXT=1024: the self-paced long-row instances as 16-wave
// instances -- 120-127 VGPRs without scratch (LANE_FRESH below), 144 words of scratch per wave (the cooperative fetch hands its pieces over in
// rounds, 128-slot claim table), 16 x (2L + L/4 + 144) words beside the 128 KB pivot table up to L = 161.  Measured (round 6, docs/HISTORY.md):
// 16 waves run the 10 K SIFT1B-shape batch no faster than the 12 of the 168-VGPR build (8.31 vs 8.30 ms: the launch sits on the rate of requests
// past L2, not on waves in flight) and the 128-VGPR code loses 3-9 % where fewer waves are resident: 768 stays the default.
// (The geometry in bang_search_host.cpp reads it too: a build with the switch passes it to every object, through EXTRA_CXXFLAGS.)
#ifndef BANG_LONG_MAXT
#define BANG_LONG_MAXT 768
#endif

BANG_HD constexpr int search_maxt(int ndw, bool host_paced) { return (search_coop(ndw, host_paced) && ndw >= 16) ? (host_paced ? 768 : BANG_LONG_MAXT) : 1024; }
// per-wave scratch: sd/ti [72] + td/compaction [72]; the filter claim table (128 slots; 256 where the scratch has them) and the
// summary's transposition area alias both, and so does the staging area of the cooperative code-row fetch (256 words: one wave
// instruction's worth of 16-byte pieces)
// 256 words where 12 waves share the LDS beside the pivot table; the 16-wave instances hand the pieces of the cooperative fetch over in rounds (144)
BANG_HD constexpr uint32_t search_scratch_words(int ndw, bool host_paced) {
  return search_coop(ndw, host_paced) ? ((ndw >= 16 && search_maxt(ndw, host_paced) >= 1024) ? 144u : 256u) : 144u;
}

BANG_HD inline uint32_t search_wl_words(uint32_t L) { return (2u * L + (L + 3u) / 4u + 3u) & ~3u; }
BANG_HD inline uint32_t search_wave_words(uint32_t L, uint32_t nctx, int ndw, bool host_paced) {
  return nctx * search_wl_words(L) + search_scratch_words(ndw, host_paced) + (nctx == 2 ? 32u : 0u);
}

#define SRCH_WG_SHARED_BYTES 2048u     // group-shared LDS behind the waves' regions (host-paced form): 128 words per pacing group, up to 4 groups
#define SRCH_DEFAULT_GROUP_WAVES 8u

// The instances live in TWO translation units of bang_search.hip per variant (Makefile): part 0 (BANG_SEARCH_PART = 0: bang_search.o, built with
// -mllvm -amdgpu-sched-strategy=iterative-ilp -- round 6: every BASELINE layout 1-5 % faster under it, a 1 250-query SIFT1B-shape shard 1.52 -> 1.45 ms) and part 1
// (bang_search_b.o, the default scheduler): the instances the ILP strategy costs scratch -- rows of 96+ chunks, 74-chunk rows that are not dword-aligned
// (0 -> 72-116 B per lane), and the host-paced instances of the long-row layouts (20-68 -> 116-168 B).  Both units compile the same dispatch; each instantiates only its own instances.
constexpr bool search_in_part1(int ndw, bool aligned, bool host_paced) { return ndw >= 24 || (ndw == 19 && !aligned) || (host_paced && ndw >= 16); }
// semantics = 1: parts 2 (bang_search_inmem.o, iterative-ILP) and 3 (bang_search_inmem_b.o, the default scheduler) split the instances the way
// parts 0 and 1 do; filter_layout = 1: parts 4 (bang_search_wf.o) and 5 (bang_search_wf_b.o), split the same way.
// Every part exports one entry, the instance dispatch of its translation unit.  The host side calls the first part of a variant (0, 2, 4), which
// hands the instances it does not hold to the second.
extern "C" {
int bang_search_launch_part0(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
int bang_search_launch_part1(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
int bang_search_launch_part2(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
int bang_search_launch_part3(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
int bang_search_launch_part4(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
int bang_search_launch_part5(const SearchArgs* a, uint32_t grid, uint32_t block, size_t lds, void* stream);
}

#endif
