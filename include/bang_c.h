/*
 * bang_c.h -- C-ABI of the MI355X-native BANG_Base search engine (libbang.so).
 *
 * Plain pointers and sizes only; every function returns an int status (0 = BANG_OK).
 * Two layers:
 *
 *  (1) ENGINE level -- the live version of the C mirror the reference sketches but compiles out
 *      (BANG_Base/bang.h:89-101, bang_search.cu:1787-1807; uint8-only there).  Same call order
 *      as BANGSearch<T> (bang.h:36-84).  This is what a ctypes / cgo / JNI binding uses.
 *
 *  (2) KERNEL level -- the seam between the C++ host graph walker and the HIP kernels: one
 *      entry per reference kernel (or fused group of kernels), device pointers + an explicit
 *      hipStream_t passed as void*, no hidden globals, no allocation inside.  Each entry cites
 *      the reference kernel it replaces.  tests/ drive these one by one against the oracle.
 *
 * All "d_" pointers are device pointers; "h_" host pointers.
 */
#ifndef BANG_C_H_
#define BANG_C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ constants */
#define BANG_OK 0
#define BANG_ERR_ARG (-1)       /* bad argument / call order */
#define BANG_ERR_IO (-2)        /* missing / malformed index file (bang_load -> false) */
#define BANG_ERR_NOMEM (-3)
#define BANG_ERR_HIP (-4)       /* a HIP runtime call failed; see bang_last_error() */
#define BANG_ERR_UNSUPPORTED (-5)
#define BANG_ERR_NOGPU (-6)     /* no HIP device: the product has NO CPU fallback */

#define BANG_MAX_L 512          /* bang.h:20 */
#define BANG_MAX_R 64           /* bang_search.cu:35 */
#define BANG_EXTRA_ITERS 50     /* NAX_EXTRA_ITERATION, bang_search.cu:53 */
#define BANG_INMEM_EXTRA_ITERS 120 /* semantics = 1: MAX_PARENTS_PERQUERY = L + 120, BANG_Inmemory/parANN.cu:30 (cap: iteration L + 119, :603-609) */
#define BANG_BF_ENTRIES 399887u /* bang_search.cu:48 */
#define BANG_BF_WORDS 12512u    /* bit-packed filter, u32 words per query (>= ceil(399887/32), 64-B multiple) */
#define BANG_NO_PARENT 0xFFFFFFFFu   /* parents[q]: query is finished */
#define BANG_IDLE_PARENT 0xFFFFFFFEu /* parents[q]: no parent this step, unmerged survivors pending */
#define BANG_NBR_STRIDE 72u     /* u32 stride of the per-query neighbour / distance rows (>= R+1) */
#define BANG_STAGE_STRIDE 65u   /* u32 stride of a staged adjacency row: [count][id x R] */

enum { BANG_U8 = 0, BANG_I8 = 1, BANG_F32 = 2 };            /* element type of vectors/queries */
enum { BANG_DIST_L2 = 0, BANG_DIST_MIPS = 1 };              /* DistFunc, bang.h:26-30 */
enum { BANG_GRAPH_HOST = 0,      /* graph in host RAM, C++ walker + staged H2D (BANG_Base) */
       BANG_GRAPH_DEVICE = 1,    /* graph + vectors resident in HBM (BANG_Inmemory placement) */
       BANG_GRAPH_AUTO = 2 };    /* resolved by bang_load: DEVICE when graph + vectors fit the free HBM next to the PQ codes
                                    (with 16 GB to spare for the per-batch state), else HOST.  288 GB hold SIFT1M .. DEEP100M
                                    (configs[1], [2]) whole; SIFT1B's 388 GB graph stays in host RAM (configs[3]) */

/* ------------------------------------------------------------------ (1) engine level */
typedef struct bang_engine bang_engine_t;

const char* bang_last_error(void);          /* thread-local message of the last failure */
int bang_device_count(void);                /* 0 if no HIP device */

int bang_create(int dtype, bang_engine_t** out);             /* BANGSearch<T>() bang.h:42 */
int bang_destroy(bang_engine_t* e);                          /* ~BANGSearch()   bang.h:43 */

/* options must be set before bang_load_e / bang_alloc_e:
 *   "graph"   : BANG_GRAPH_HOST | BANG_GRAPH_DEVICE | BANG_GRAPH_AUTO (default: auto; environment BANG_GRAPH=host|device|auto)
 *   "lanes"   : number of independent query groups pipelined against each other (>=1)
 *   "threads" : host walker threads per lane (>=1)
 *   "device"  : HIP device ordinal
 *   "pq"      : 0 = pivot-stationary fused distance (default when it fits LDS), 1 = LUT path (K1+K2)
 *   "timing"  : 1 = stamp every front-kernel launch in-kernel (s_memrealtime) for bang_get_stats
 *   "numa"    : graph in host RAM: 1 = pin the walker threads (and the caller during bang_query) to the CPUs of the GPU's NUMA node,
 *               one physical core each; 0 = leave them where the OS puts them; -1 = auto = 0 (pinning measured slower on the
 *               2-socket measurement box)
 *   "search"  : graph in HBM: 1 = the query-resident search kernel (bang_k_search; on the LUT path bang_k_search_lut), 0 = the round-1 loops,
 *               -1 = auto (the LUT path keeps the round-1 loop) */
int bang_set_option(bang_engine_t* e, const char* key, long value);
/* The whole table of options and environment switches as text (csrc/bang_options.cpp is the one place they are defined): writes at
 * most cap bytes (NUL-terminated) to buf, returns the size needed.  buf may be NULL. */
int bang_describe_options(char* buf, size_t cap);

/* bang_load, bang.h:51 / bang_search.cu:138-362 */
int bang_load_e(bang_engine_t* e, const char* indexfile_path_prefix);

/* Same as bang_load_e but from memory (synthetic / already-mapped indices).  The graph pointer
 * must stay valid until bang_unload_e (it is NOT copied in BANG_GRAPH_HOST mode); everything
 * else is copied.  pivots is the file-order [256][D] table. */
typedef struct {
  uint64_t medoid, entry_len;
  uint32_t D, R, N, m;
  const uint8_t* graph;      /* N * entry_len bytes */
  const uint8_t* codes;      /* N * m bytes (host) -- or NULL when d_codes is given */
  const void* d_codes;       /* optional: codes already on the device (N*m + 256 bytes; N*code_stride + 256 with code_stride != 0).  The engine reads the
                                first m bytes of a row -- and, pull mode with option "rows_pad" != 0 (auto included), a 72-chunk pivot layout (m = 65..72, chunks of at most 2 dims) and code_stride = 128,
                                WRITES adjacency ids into the bytes 72..127 of each row, which hold no code: set rows_pad = 0 to keep it out of them */
  const float* pivots;       /* [256][D] */
  const float* centroid;     /* [D] */
  const uint32_t* chunk_off; /* [m+1] */
  uint32_t code_stride;      /* d_codes only: bytes between the rows of consecutive nodes, 0 = m (packed).  Host codes are always packed;
                                the engine lays them out itself (option "code_stride") */
  uint32_t vectors_ready;    /* bang_load_shared_e: 1 = d_vectors already holds the vectors */
  void* d_vectors;           /* optional, streamed / shared loads: a DEVICE buffer of the caller, N * D * sizeof(T) + 256 bytes, that holds the
                                full-precision vectors instead of an allocation of the engine (it must outlive the index).
                                bang_load_stream_e fills it; the caller may then hand it on to the other GPUs of the node */
  uint64_t rows_hash;        /* bang_load_shared_e: what bang_get_rows_hash reported on the rank that loaded the index */
} bang_index_desc;
int bang_load_mem_e(bang_engine_t* e, const bang_index_desc* desc);

/* STREAMED load (host placement, pull mode only): the graph entries are handed over chunk by chunk and are never held in host
 * memory as a whole.  The engine calls src(ctx, first, count, dst) for consecutive node ranges; the source writes `count`
 * entries in the reference layout ([T vec[D]][u32 degree][u32 id x R], entry_len bytes each) to dst and returns 0.  Of each entry
 * the vector goes to HBM and the adjacency list into the 256-byte pull rows in pinned host memory: a 10^9-node SIFT index then
 * needs 256 GB of host RAM instead of 388 GB + 256 GB.  desc->graph must be NULL.  Fails (BANG_ERR_UNSUPPORTED / BANG_ERR_NOMEM)
 * where the pull mode is not possible -- vectors that do not fit HBM, rows that do not fit the host, R > 64, option pull = 0 --
 * because nothing else can run without the graph.  bang_load_e streams `<p>_disk.bin` through the same path when the pull mode
 * applies (BANG_STREAM_LOAD=0: map the file as before); should a walker form be asked for later, the file is mapped then. */
/* The reference's preprocessing step as a library call (host only, no device needed): DiskANN's sector-padded `_disk.index` ->
 * `<out_prefix>_disk.bin` + `<out_prefix>_disk_metadata.bin`, byte for byte what BANG_Base/bang_preprocess.py writes (header parse
 * :28-64, sector walk :75-80, ascending adjacency lists :81-109, metadata :42-51,116).  dtype: BANG_U8 / BANG_I8 / BANG_F32.
 * bang_load_e does the same conversion on the fly when only the `_disk.index` exists. */
int bang_convert_diskann_index(const char* index_path, const char* out_prefix, int dtype);

typedef int (*bang_entry_source)(void* ctx, uint64_t first, uint64_t count, uint8_t* dst);
int bang_load_stream_e(bang_engine_t* e, const bang_index_desc* desc, bang_entry_source src, void* ctx);
/* SHARED load, for the ranks of a multi-GPU node that did NOT read the index: the rank that did (bang_load_e / bang_load_stream_e with
 * desc->d_vectors) has built the node's ONE pull-rows file (BANG_PULL_ROWS_DIR) and holds the full-precision vectors in its HBM; the
 * others receive the vectors from there (RCCL broadcast over xGMI into their own desc->d_vectors, vectors_ready = 1) and the hash of
 * the adjacency lists (bang_get_rows_hash), map the rows file and are done -- no index entry is read a second time.  PQ codes as in
 * every load (desc->codes / d_codes). */
int bang_load_shared_e(bang_engine_t* e, const bang_index_desc* desc);
int bang_get_rows_hash(bang_engine_t* e, uint64_t* out);

/* PEER ROWS: the adjacency rows of a multi-GPU node in the NODE's spare HBM, read over xGMI, host DRAM only for the remainder.
 * After bang_load* in pull mode every GPU has HBM left (SIFT1B: ~46 GB = 178 M rows of 256 B): rank r of W keeps the rows
 * [r * n, (r + 1) * n) there (bang_rows_slice_e), exports that allocation (bang_rows_export_e: a 64-byte hipIpcMemHandle), and every rank
 * imports the W - 1 others (bang_rows_import_e).  The search kernel then reads the row of parent p from slice p / n -- its own HBM, a
 * peer's HBM through the IPC mapping, or, for p >= W * n, pinned host memory over PCIe as before.  W x 18 % of SIFT1B's rows: 72 % at
 * W = 4, all of them at W = 8.  Call order: load -> slice -> export / (exchange handles) / import -> bang_alloc.  Results never change.
 * bang_rows_slice_e replaces the default copy (rows [0, auto)); rows = 0 drops it.  A slice that has been exported is never freed before
 * bang_unload (bang_alloc does not take it back when HBM is short: BANG_ERR_NOMEM instead). */
/* PADDED ROWS (option "rows_pad"): adjacency rows of the nodes [0, *rows_out) of the loaded index that sit in the padding of its PQ code table and are
 * read there by the self-paced PQ search kernel; the HBM row copy holds the rows behind them.  0: none (option off, another code layout, the rows all
 * fit HBM, given up for a form that cannot read them).  Peer rows and padded rows exclude each other: with rows_pad = -1 (auto) bang_rows_slice_e, _export_e and _import_e give
 * the padded rows up, with rows_pad = 1 they are refused. */
int bang_rows_pad_e(bang_engine_t* e, uint64_t* rows_out);
#define BANG_MAX_ROW_SLICES 16
int bang_get_num_nodes(bang_engine_t* e, uint64_t* nodes_out);    /* N of the loaded index (the reference reads it from <p>_disk_metadata.bin, bang_search.cu:176-189) */
int bang_rows_capacity_e(bang_engine_t* e, uint64_t* rows_out);   /* rows of 256 B this engine's free HBM holds now (6 GB kept back for the batch state) + what its row copy holds */
int bang_rows_slice_e(bang_engine_t* e, uint64_t first_row, uint64_t rows);
int bang_rows_export_e(bang_engine_t* e, void* handle64, uint64_t* first_row, uint64_t* rows);
int bang_rows_import_e(bang_engine_t* e, uint32_t slot, uint32_t n_slots, uint64_t slice_rows, uint64_t rows /* what the exporter's bang_rows_export_e
                       * reported: a peer allocation shorter than the slot's rows min(slice_rows, N - slot * slice_rows) is refused -- the kernel reads
                       * base + p * 256 for every p of the slot; ignored for the own slice */,
                       const void* handle64 /* NULL: this engine's own slice */);
/* Tear-down in two phases: every rank closes its mappings of the OTHER ranks' slices (this call; after bang_free), the ranks meet (a barrier of
 * the caller's process group), and only then does anyone bang_unload -- which frees the slice the others had mapped. */
int bang_rows_close_peers_e(bang_engine_t* e);

int bang_set_searchparams_e(bang_engine_t* e, int recall, int worklist_length, int distfn); /* bang.h:60 */
int bang_alloc_e(bang_engine_t* e, int num_queries);                                        /* bang.h:53 */
int bang_init_e(bang_engine_t* e, int num_queries);                                         /* bang.h:56 */
/* THE INPUT DOMAIN OF FLOAT DATA (DESIGN.md section 2 CANON 20): float queries and the float tables of an index (vectors, pivots, centroid) must be
 * finite with |x| <= 2^56 -- the largest power of two for which no distance of a supported layout reaches the sentinel 3.402823E+38f; inside it no
 * kernel ever sees an inf or a NaN (a NaN distance breaks a wave's rank sort and ends in a read outside the index).  bang_check_floats is the check:
 * host code, no device needed, one pass on the bits ((bits & 0x7FFFFFFF) > 0x5B800000: NaN of either sign and any payload, +-inf, finite values
 * beyond 2^56).  Returns BANG_OK, or BANG_ERR_ARG with the index of the FIRST offending element in *first_bad (may be NULL); n = 0 is BANG_OK.
 * Every load checks the pivot table and the centroid of the index, whatever its vector type, and fails with BANG_ERR_ARG naming the table and the
 * element.  NOT checked: the float vectors of an index file (up to 512 GB) -- their range is the index's contract. */
int bang_check_floats(const float* x, uint64_t n, uint64_t* first_bad);

/* bang_query, bang.h:75: ids [Q][k] u64, dists [k][Q] f32 (rank-major, bang_search.cu:999).  A float engine checks the batch with bang_check_floats
 * before a lane is started or a copy issued: a query element outside the domain is BANG_ERR_ARG with the query and the dimension in the message;
 * allocation, bang_init state, radii, filters and exclusion set are untouched and the next clean batch runs on them.  (A MIPS batch is
 * [Q][D - 1] floats and is checked, and its offender named, at that row length.) */
int bang_query_e(bang_engine_t* e, const void* h_queries, int num_queries, uint64_t* h_ids, float* h_dists);
/* The same search with the results LEFT ON THE DEVICE: d_ids [Q][k] u64 and (optional, may be NULL) d_dists [k][Q] f32 are device
 * buffers of the caller on the engine's device; nothing but the per-query iteration counts returns to the host.  For callers that
 * hand the ids on from device memory -- the multi-GPU job all-gathers the shards' id blocks over xGMI straight from here (SURVEY
 * 8(e)) instead of bouncing them through the host.  Complete (stream synchronised) on return.  The float domain check of bang_query_e runs here
 * too, before anything is launched: on a refusal d_ids / d_dists are not written. */
int bang_query_dev_e(bang_engine_t* e, const void* h_queries, int num_queries, uint64_t* d_ids, float* d_dists);
int bang_free_e(bang_engine_t* e);                                                          /* bang.h:80 */

/* EXCLUDED IDS (lazy deletes, DESIGN.md section 2 CANON 17): an engine carries a set X of node ids that bang_query_e / bang_query_dev_e never
 * return.  The walk ignores X -- excluded nodes are evaluated, expanded and logged like any other, so counters and candidate log are those of the
 * same run with X empty, bit for bit -- and the results are composed behind it: on the PQ walks the re-rank (K6 + K7) runs on the candidate log
 * without its entries in X (bang_k_cand_live; the re-rank is then a launch of its own: bang_stats.rerank_fused = 0), with distance = 1 the results
 * are the first k entries of the final worklist that are not in X (bang_k_worklist_pick).  Fewer than k left: the tail is UINT64_MAX /
 * 3.402823E+38f.  An allow-list is the exclusion of its complement.
 * bang_set_excluded_e REPLACES the set by the n ids (duplicates are fine; n = 0 clears it; ids may be NULL then): a bitmap of ceil(N / 32) + 1
 * words is built on the host and copied to HBM (125 MB at N = 10^9).  An id >= N is refused (BANG_ERR_ARG, "out of range") before anything is
 * copied and the set stays what it was.  Both calls need a loaded index and are refused while an allocation is live (bang_free_e first): the
 * allocation holds the buffers the set needs.  bang_unload_e drops the set.  With X empty nothing changes -- same launches, the fused re-rank where
 * it was fused.  Not served, refused by bang_alloc_e with "excluded" in the message: the forms whose re-rank reads a vector LOG (graph in host RAM
 * without the vectors resident in HBM).
 * Environment, for callers of the bang.h class and the bang_search CLI: BANG_EXCLUDE_FILE names a .bin file (i32 count, i32 1, count u32 ids)
 * that every load (bang_load_e, _mem_e, _stream_e, _shared_e) reads as its last step; an unreadable file or an id out of range fails the load. */
int bang_set_excluded_e(bang_engine_t* e, const uint32_t* ids, uint64_t n);
int bang_clear_excluded_e(bang_engine_t* e);

/* LABELS AND PER-QUERY FILTERS (DESIGN.md section 2 CANON 18, section 4.13): every point carries a 32-bit label word (up to 32 tags), every query of
 * a batch two words, `any` and `all`; node x MATCHES when (any == 0 || (labels[x] & any) != 0) && (labels[x] & all) == all (any = all = 0: an
 * unfiltered query).  A filtered batch runs the exact-distance walk unchanged -- counters and candidate log are those of the same batch without
 * filters, bit for bit -- and collects each query's results from EVERY node the walk evaluates: the matching survivors of an iteration go through
 * the worklist's sort + merge rule into a second sorted list of capacity L, whose first k entries are the results (bang_k_search_exact_labels); the
 * tail behind fewer than k is UINT64_MAX / 3.402823E+38f.  An unfiltered query of a filtered batch returns exactly today's ids and distance bits.  A
 * node in the engine's exclusion set never enters the list (the kernel tests the bitmap itself; bang_k_worklist_pick is not launched).
 * bang_set_labels_e REPLACES the table: n must be N ("labels" and both numbers in the message), n = 0 clears it (labels may be NULL then).  Both
 * calls need a loaded index and are refused while an allocation is live; bang_unload_e drops the table.  An engine with labels and no filters runs
 * today's launches unchanged.
 * bang_set_query_filters_e sets the filters of the batches to come, nq of them (row i for query i): valid while an allocation is live, nq <= the
 * allocated batch size, nq = 0 clears; copied to HBM and kept until replaced, cleared or bang_free_e.  bang_query_e / bang_query_dev_e refuse a
 * batch whose size differs from nq ("filters" in the message).  Refused at bang_set_query_filters_e, with "labels" in the message, no fallback: no
 * labels set; distance = 0 (the PQ walks have no exact distance when a node is evaluated); beam > 1; vectors_fp16 = 1; a vector layout of the wide
 * instances.
 * bang_get_matched_counts: per query of the last filtered batch, the number of matching survivors offered to its result list -- a caller sees from
 * it when a filter was too selective for its L.
 * Environment, for callers of the bang.h class and the bang_search CLI: BANG_LABEL_FILE names a .bin file (i32 N, i32 1, N u32 label words) that
 * every load reads as its last step, behind BANG_EXCLUDE_FILE, with the same failure behaviour; BANG_QUERY_FILTER_FILE names a .bin file (i32 Q,
 * i32 2, Q x {any, all}) whose row i the bang.h bang_query applies to query i of every batch (read once per allocation; fewer rows than
 * queries is an error). */
int bang_set_labels_e(bang_engine_t* e, const uint32_t* labels, uint64_t n);
int bang_clear_labels_e(bang_engine_t* e);
int bang_set_query_filters_e(bang_engine_t* e, const uint32_t* any, const uint32_t* all, int nq);
int bang_clear_query_filters_e(bang_engine_t* e);
int bang_get_matched_counts(bang_engine_t* e, uint32_t* out, uint32_t num_queries);

/* RANGE SEARCH (DESIGN.md section 2 CANON 19, section 4.14; option range_hits, distance = 1): "every point within distance r of the query", a variable
 * number of results per query.  With option range_hits = cap (1 .. 4096) bang_alloc_e holds a hit log of cap entries per query, and a batch that
 * runs with RADII collects, beside its k results, every node its walk EVALUATES whose squared L2 distance is <= the query's radius and that is not in
 * the engine's exclusion set.  The walk is the one without radii, bit for bit: the k ids and distance bits, the four per-query counters and the
 * candidate log are those of the same batch without radii.  Hits are taken in every iteration, the first (seed list) and the cap iteration (evaluated,
 * not merged) included; the compare is a plain float compare on the distance bits the walk computed, so a NaN or negative radius gives a query with
 * no range and +inf takes every evaluated node.  The first cap hits in evaluation order are kept; behind the launch each query's kept hits are sorted
 * ascending by (distance bits, id) and adjacent equal entries -- an id that an adjacency row lists twice -- dropped (bang_k_search_exact_range +
 * bang_k_range_sort).  Recall of the answer depends on L, as for top-k; nothing grows L automatically: offered / count tell a caller when to.
 * bang_set_query_radii_e sets the radii of the batches to come, nq of them (row i for query i): valid while an allocation is live, refused with
 * range_hits = 0, nq <= the allocated batch size, nq = 0 clears; copied to HBM and kept until replaced, cleared or bang_free_e.  bang_query_e /
 * bang_query_dev_e refuse a batch whose size differs from nq ("radii" in the message).  Radii and label filters together are refused, at whichever
 * of the two setters comes second.  An allocation with range_hits set and no radii runs today's launches unchanged.  bang_alloc_e refuses
 * range_hits > 0, with "range" in the message and no fallback, with distance = 0, beam > 1, vectors_fp16 = 1 or a vector layout of the wide instances.
 * bang_get_range_counts: per query of the last batch with radii, count = the hits in its answer and offered = all hits its walk met
 * (offered > cap: the answer was truncated to the first cap in evaluation order); either pointer may be NULL.
 * bang_get_range_results: the answers of that batch packed CSR in query order: lims[0] = 0, query q's hits at [lims[q], lims[q + 1]) of ids (u64, as
 * the top-k ids) and dists; lims has (queries of the batch) + 1 entries.  capacity = the entries ids / dists hold: below lims[nq] is BANG_ERR_ARG
 * and nothing is written. */
int bang_set_query_radii_e(bang_engine_t* e, const float* radii, int nq);
int bang_clear_query_radii_e(bang_engine_t* e);
int bang_get_range_counts(bang_engine_t* e, uint32_t* counts, uint32_t* offered, uint32_t num_queries);
int bang_get_range_results(bang_engine_t* e, uint64_t* lims, uint64_t* ids, float* dists, uint64_t capacity);
/* INSERTS (DESIGN.md section 2 CANON 21, section 4.15; option capacity): new points go into a loaded index without a rebuild.  With option
 * capacity = C > N and graph = device given explicitly, bang_load_mem_e / bang_load_e allocate the graph entries, the PQ codes (256-byte slack kept)
 * and the exclusion bitmap for C nodes.  Refused at load, with "capacity" in the message: host placement (auto included), streamed and shared loads,
 * a caller's code or vector buffer, vectors_fp16, capacity < N, R > 64.
 * bang_insert_e adds the n vectors ([n][D], the engine's element type) as ONE batch; their ids are N .. N + n - 1 in input order, *first_id = N (may
 * be NULL).  All n searches run on the graph as it was before the call: points of one batch do not see each other, a second call sees the first.
 * Per point: the candidates are its final worklist of the exact-distance walk (bang_k_search_exact at L = k = L_build, cap L_build + 49; the
 * exclusion set is NOT consulted -- a deleted node stays a graph node and may become a neighbour), RobustPrune(alpha) gives its row, every old node
 * in a new row receives the back-edge (appended while the row has room, else the row is re-pruned from old row ++ new ids), the PQ code of chunk c is
 * the lowest k minimising K1's table, and the seed list is rebuilt.  Valid after a load, refused while an allocation is live (bang_free_e first).
 * Refused with a message and no side effect: no capacity or N + n > capacity; n = 0 or n > 16384; L_build < 1 or > BANG_MAX_L; alpha not finite or
 * outside [1, 8]; MIPS search parameters; a layout outside bang_search_can_rerank; a label table set (clear it, insert, set one for the new N);
 * float vectors that bang_check_floats refuses.  N moves only after the last kernel of the call succeeded; a call that fails behind its checks
 * (a HIP error, an abort word) leaves N where it was; if it had reached the back-edge launches, old rows may already list ids >= N: the engine then
 * refuses every further bang_insert_e and bang_alloc_e with a message that says so, until bang_unload_e. */
#define BANG_INSERT_MAX_BATCH 16384u
int bang_insert_e(bang_engine_t* e, const void* h_vectors, uint32_t n, uint32_t L_build, float alpha, uint64_t* first_id);
/* graph entries [first, first + n) of the loaded index (graph in HBM) as the index file holds them, n * entry_len bytes; and the packed PQ codes
 * (n * m bytes, whatever the stride in HBM).  first + n <= N. */
int bang_get_entries_e(bang_engine_t* e, uint64_t first, uint64_t n, void* out);
int bang_get_codes_e(bang_engine_t* e, uint64_t first, uint64_t n, void* out);
/* CONSOLIDATION (DESIGN.md section 2 CANON 22, section 4.16; FreshDiskANN Algorithm 4): folds the exclusion set X into the graph, in HBM.  med = the
 * medoid, D = X \ {med} the nodes removed (an excluded medoid stays a routing node: live below, its row repaired like any other, still excluded from
 * answers).  Every p not in D whose row lists a node of D is AFFECTED; its candidates are the ids of its row outside D, then for each v of its row in
 * D the ids of row(v) that are neither in D nor p (row order, duplicates kept, cut at BANG_PRUNE_MAX_LIST = 512, the rest counted as dropped); each
 * gets its exact distance to vector(p); the list is sorted and de-duplicated by (distance bits << 32) | id (bang_k_range_sort) and RobustPruned at
 * alpha2 = fl32(fl32(alpha) * fl32(alpha)) into p's row (bang_k_prune; an empty list gives degree 0).  Every affected row goes through the prune --
 * DiskANN's copy of a candidate set of at most R ids without pruning is not built.  Rows are computed from the graph as it stood at the call, so
 * the result does not depend on the order or chunking.  Then the row of every node of D becomes degree 0 with all R slots 0 (vector and PQ code
 * stay, ids are not renumbered, N does not move), the seed list is rebuilt from the medoid's row and the exclusion set becomes X & {med}.  Rows of
 * nodes that are not affected, and every byte outside rows, are unchanged.
 * out_stats4 (may be NULL): {rows rewritten, nodes removed, candidates dropped by the cut, ids still excluded (0 or 1)} of this call.
 * Refused with "bang_consolidate" in the message and no side effect: a null engine or no index loaded; a live allocation (bang_free_e first); an
 * engine whose insert failed half-way; no option capacity (the mutable, HBM-resident engine of bang_insert_e: capacity = N is enough); alpha not
 * finite or outside [1, 8] (BANG_ERR_ARG); MIPS search parameters; a layout outside bang_search_can_rerank (BANG_ERR_UNSUPPORTED).  A label table
 * may stay set.  An empty exclusion set is BANG_OK with zero statistics and writes nothing.  A row that lists an id >= N: the id is never
 * dereferenced, the call returns BANG_ERR_IO and names the step.  A call that fails before the rows of D are cleared leaves a graph that every
 * walk may run on -- rewritten rows list live nodes only, the others nodes that still exist -- and the exclusion set untouched.
 * The nodes of D are also ORed into the engine's REMOVED bitmap (the shape of the exclusion bitmap), which bang_scan_e alone reads -- the removed
 * nodes keep their vectors, and X no longer names them --, bang_insert_reuse_e hands out again and bang_unload_e drops; it is not part of an index
 * file (bang_get_removed_e / bang_set_removed_e carry it across an export). */
int bang_consolidate_e(bang_engine_t* e, float alpha, uint64_t* out_stats4);
/* REUSE OF REMOVED IDS (DESIGN.md section 2 CANON 24, section 4.18).  F = the nodes x < N whose bit is set in the removed bitmap, X the exclusion
 * set at the call, E = F \ X the eligible free slots.  bang_insert_reuse_e adds the n vectors as ONE batch like bang_insert_e, at the ids
 * ids[i] = the i-th smallest element of E for i < f = min(n, |E|) and N + (i - f) behind: strictly ascending in input order, written to
 * ids_out[n].  Everything else is bang_insert_e with "N + i" read as ids[i]: the searches run on the graph as it stood (n_nodes = N; no walk
 * reaches a node of F), entry and code row go to slot ids[i], back-edge targets are old live nodes.  Last, and only after the last kernel
 * succeeded, the removed bits of ids[0 .. f) are cleared and N grows by n - f.  With F empty (or f = 0) the bytes are bang_insert_e's.
 * Refused with "bang_insert_reuse" in the message and no side effect: every refusal of bang_insert_e, with N + (n - f) > capacity in the place
 * of N + n > capacity (a batch that fits its free slots succeeds at capacity == N), and ids_out NULL.  A new row that lists an id of the batch
 * is BANG_ERR_IO.  A failure before the back-edge step leaves N, the bitmap and every reachable row as they were (the overwritten slots are
 * still free); behind it the engine refuses further inserts as bang_insert_e does.  bang_insert_e itself never consults F.
 * bang_get_insert_times reports the last call of either kind: here [2] also holds the select of E, the upload of the entries to their slots and
 * the download of the new rows, [4] the copy of the code rows to their slots.
 * bang_get_free_slots_e: out3 = {|F|, |E|, slots reused since the load}.
 * bang_get_removed_e: the ids of F ascending into ids_out (room for cap ids; BANG_ERR_ARG if |F| > cap), *count = |F|; ids_out NULL: the count alone.
 * bang_set_removed_e REPLACES F by the n ids (n = 0 clears it): what a caller persists beside an exported index (formats.write_removed) and
 * restores after a load.  Needs the graph in HBM and no live allocation.  Checked on the GPU before anything changes: every id is < N and not
 * the medoid, its row has degree 0, and no row of a node outside the list names a listed id; else BANG_ERR_ARG, the message names the first
 * offending id, and the old F stays. */
int bang_insert_reuse_e(bang_engine_t* e, const void* h_vectors, uint32_t n, uint32_t L_build, float alpha, uint64_t* ids_out);
int bang_get_free_slots_e(bang_engine_t* e, uint64_t* out3);
int bang_get_removed_e(bang_engine_t* e, uint32_t* ids_out, uint64_t cap, uint64_t* count);
int bang_set_removed_e(bang_engine_t* e, const uint32_t* ids, uint64_t n);
int bang_unload_e(bang_engine_t* e);                                                        /* bang.h:82 */

/* statistics of the last bang_query_e */
typedef struct {
  double wall_ms;             /* bang_query_e wall time */
  uint64_t iterations;        /* max `iter` reached over the lanes */
  uint64_t dist_evals;        /* total surviving neighbours whose PQ distance was computed */
  uint64_t fetched;           /* total adjacency ids offered to the filter */
  uint64_t candidates;        /* total expanded nodes re-ranked */
  uint64_t front_launches;    /* launches of the filter+distance+parent kernel */
  double front_ms;            /* sum of their durations from in-kernel s_memrealtime stamps ("timing"=1, else 0):
                                 per launch max(end) - min(start) over its workgroups */
  double back_ms;             /* unused (kept for layout; rocprofv3 reports the sort+merge kernel) */
  double rerank_ms;
  double walker_ms;           /* host time in the adjacency gather, summed over lanes */
  double sync_ms;             /* host time blocked waiting for the parents of an iteration, summed over lanes */
  double enqueue_ms;          /* host time spent inside launch / memcpy-enqueue calls, summed over lanes */
  double front_busy_ms;       /* length of the UNION of the front-kernel launch intervals of all lanes ("timing"=1): the time
                                 during which at least one front kernel was running (lanes overlap) */
  uint64_t persistent;        /* 1: the batch ran as ONE persistent search kernel (host-graph mode, "persistent" option).  Then
                                 front_launches = 1, front_busy_ms = duration of that launch (first to last in-kernel stamp) and
                                 front_ms = time a workgroup spent in its front phases, mean over the workgroups */
  uint64_t h2d_bytes;         /* host-graph mode: bytes the walker handed to the device (adjacency rows + full-precision vectors) */
  uint64_t vectors_on_device; /* host-graph mode: 1 = the re-rank read a packed copy of the vectors in HBM ("vectors" option),
                                 0 = the walker shipped every expanded node's vector (the reference's data flow) */
  /* effective configuration of the allocation the query ran on (what "auto" resolved to) */
  uint64_t graph_mode;        /* BANG_GRAPH_HOST | BANG_GRAPH_DEVICE */
  uint64_t lanes;             /* independent query groups (1 with the persistent search kernel) */
  uint64_t walker_threads;    /* host walker threads per lane (0 in device-graph mode) */
  uint64_t wg_queries;        /* persistent search kernel: queries per workgroup block, 0 otherwise */
  uint64_t workgroups;        /* persistent search kernel: workgroups of the launch, 0 otherwise */
  /* expansions (= graph hops = iterations in which the query had a parent) per query: median, 99th percentile, maximum */
  uint64_t hops_p50, hops_p99, hops_max;
  uint64_t search_kernel;     /* 1: the batch ran on the query-resident search kernel (bang_k_search) */
  uint64_t pacing_groups;     /* host-paced search kernel: groups of waves the walker threads serve (0 otherwise) */
  uint64_t graph_pull;        /* host-graph placement: 1 = PULL mode -- the adjacency lists live as 256-byte rows in pinned host memory
                                 and the self-paced search kernel fetches them over PCIe by itself (no walker thread in the loop) */
  uint64_t pulled_bytes;      /* pull mode: bytes of adjacency rows the kernel fetched over PCIe (256 per expansion) */
  uint64_t rows_in_hbm;       /* pull mode: nodes whose adjacency row ALSO sits in HBM (no PCIe read for them), option "rows_hbm" */
  uint64_t code_stride;       /* bytes between PQ code rows in HBM (m = packed; 128 = rows padded to their own 128-byte line) */
  uint64_t filter_loads_skipped; /* search kernel, self-paced form: visited-filter word loads NOT issued because the wave's on-chip
                                 summary knew the word was still zero (of 2 x `fetched` probes) */
  uint64_t rows_from_peer;    /* pull mode with peer rows: expansions of the last batch whose adjacency row came from ANOTHER GPU's HBM (over xGMI) */
  uint64_t rows_from_own_hbm; /* ... from this GPU's own HBM copy / slice */
  uint64_t walker_rows;       /* host-paced search kernel: 1 = the walker threads read the 256-byte pull rows (option "walker"), not graph entries */
  uint64_t rerank_fused;      /* 1: K6 + K7 ran inside the search launch (the wave that finished a query re-ranked it), no re-rank launch followed */
  uint64_t vectors_fp16;      /* host-graph mode: 1 = the vector table in HBM holds IEEE fp16 rows (option "vectors_fp16"): every exact distance is the usual
                                 arithmetic applied to the vectors rounded to fp16 */
  uint64_t vector_table_bytes; /* bytes of that table (N rows + 256 bytes of slack), 0 where the index keeps none */
} bang_stats;
int bang_get_stats(bang_engine_t* e, bang_stats* out);
/* bang_stats with what later options report appended BEHIND it: bang_stats itself keeps its size and offsets, so callers built against it are
 * not disturbed.  The first sizeof(bang_stats) bytes are what bang_get_stats fills. */
typedef struct {
  bang_stats base;
  uint64_t filter_layout;     /* layout of the visited filter the batch ran on (option "filter_layout"): 0 = split, 1 = word (bang_k_search_wf; then
                                 base.filter_loads_skipped counts of 1 x `fetched` probes) */
} bang_stats_ext;
int bang_get_stats_ext(bang_engine_t* e, bang_stats_ext* out);
/* ... and the same once more for the excluded ids (bang_set_excluded_e): bang_stats_ext keeps its size and offsets as bang_stats did, the two new
 * fields sit at the end of the statistics, behind it.  The first sizeof(bang_stats_ext) bytes are what bang_get_stats_ext fills. */
typedef struct {
  bang_stats_ext ext;
  uint64_t excluded;          /* distinct ids in the engine's exclusion set, 0 = none */
  uint64_t exclude_launches;  /* launches of bang_k_cand_live / bang_k_worklist_pick of the last bang_query_e, summed over the lanes (0 with an empty set) */
} bang_stats_ext2;
int bang_get_stats_ext2(bang_engine_t* e, bang_stats_ext2* out);
/* ... and once more for labels and per-query filters (bang_set_labels_e / bang_set_query_filters_e): the earlier structs keep size and offsets */
typedef struct {
  bang_stats_ext2 ext2;
  uint64_t labelled;          /* nodes the engine's label table covers (N), 0 = no table */
  uint64_t filtered_queries;  /* queries of the last bang_query_e that ran with a filter other than any = all = 0 */
  uint64_t label_launches;    /* launches of bang_k_search_exact_labels of the last bang_query_e (0 without filters) */
} bang_stats_ext3;
int bang_get_stats_ext3(bang_engine_t* e, bang_stats_ext3* out);
/* ... and once more for range search (option range_hits + bang_set_query_radii_e): the earlier structs keep size and offsets */
typedef struct {
  bang_stats_ext3 ext3;
  uint64_t range_hits;        /* option range_hits: the capacity of a query's hit log, 0 = off */
  uint64_t range_queries;     /* queries of the last bang_query_e that ran with a radius */
  uint64_t range_launches;    /* launches of bang_k_search_exact_range of the last bang_query_e (0 without radii) */
  uint64_t range_truncated;   /* ... of those queries, how many met more hits than the log holds (offered > range_hits) */
} bang_stats_ext4;
int bang_get_stats_ext4(bang_engine_t* e, bang_stats_ext4* out);
/* ... and once more for inserts (option capacity + bang_insert_e): the earlier structs keep size and offsets.  The four counters are totals since
 * the load */
typedef struct {
  bang_stats_ext4 ext4;
  uint64_t capacity;          /* option capacity: nodes the tables hold, 0 = off */
  uint64_t inserted;          /* points inserted */
  uint64_t backedge_appended; /* old rows that took their new ids by appending */
  uint64_t backedge_pruned;   /* old rows re-pruned from old row ++ new ids */
  uint64_t backedge_dropped;  /* incoming ids dropped because a target's candidates exceeded BANG_PRUNE_MAX_LIST */
} bang_stats_ext5;
int bang_get_stats_ext5(bang_engine_t* e, bang_stats_ext5* out);
/* Where the last bang_insert_e spent its time, milliseconds: ms6[0] the candidate searches, [1] worklist -> lists + prune of the new rows, [3] the
 * back-edge launches (CSR upload included), [4] the PQ encode -- stream time between event stamps --, [2] the new rows' download + the host-side
 * grouping and [5] the whole call, host wall time (allocations and copies included). */
int bang_get_insert_times(bang_engine_t* e, double* ms6);
/* ... and once more for consolidation (bang_consolidate_e): the earlier structs keep size and offsets.  The three counters are totals since the load */
typedef struct {
  bang_stats_ext5 ext5;
  uint64_t consolidated_rows;   /* rows rewritten by bang_consolidate_e */
  uint64_t removed;             /* nodes whose rows it emptied */
  uint64_t consolidate_dropped; /* candidates dropped because a row's list exceeded BANG_PRUNE_MAX_LIST */
} bang_stats_ext6;
int bang_get_stats_ext6(bang_engine_t* e, bang_stats_ext6* out);
/* Where the last bang_consolidate_e spent its time, milliseconds of host wall time: ms4[0] the scan, the download of the affected bitmap and the
 * list, [1] the gather / sort / prune chunks, [2] the clear, the seed list and the exclusion set, [3] the whole call (allocations included). */
int bang_get_consolidate_times(bang_engine_t* e, double* ms4);
/* Per-query counters of the last bang_query_e (arrays of num_queries words; any pointer may be NULL): PQ distance evaluations,
 * adjacency ids offered to the filter, expanded nodes (candidate-log length) and -- search kernel only, else zeros -- the number
 * of iterations the query ran.  Test hook: the oracle reports the same four numbers per query. */
int bang_get_query_counters(bang_engine_t* e, uint32_t* dist_evals, uint32_t* fetched, uint32_t* candidates, uint32_t* iterations);

/* The candidate log of the last bang_query_e (bang_search.cu:1451-1458: the nodes a query expanded, in expansion order, [0] = MEDOID): ids
 * [num_queries][stride] with stride >= L + 50, counts [num_queries]; num_queries = rows the caller's buffers hold, refused when smaller than
 * the last batch (the rows of that batch are what is copied).  Analysis hook (which adjacency rows a batch really reads). */
int bang_get_candidate_log(bang_engine_t* e, uint32_t* ids, uint32_t stride, uint32_t* counts, uint32_t num_queries);

/* The reference's own C mirror (bang.h:91-100), uint8 only, one process-global engine. */
int bang_load_c(char* indexfile_path_prefix);
int bang_set_searchparams_c(int recall, int worklist_length, int nDistFunc);
int bang_alloc_c(int num_queries);
int bang_init_c(int num_queries);
int bang_query_c(uint8_t* query_array, int num_queries, unsigned long* nearestNeighbours,
                 float* nearestNeighbours_dist);
int bang_free_c(void);
int bang_unload_c(void);

/* ------------------------------------------------------------------ device helpers */
/* Raw device memory for callers without a tensor library (tests, bindings). */
int bang_dev_malloc(void** d_ptr, size_t bytes);
int bang_dev_free(void* d_ptr);
int bang_dev_memset(void* d_ptr, int value, size_t bytes);
int bang_dev_h2d(void* d_dst, const void* h_src, size_t bytes);
int bang_dev_d2h(void* h_dst, const void* d_src, size_t bytes);
int bang_dev_sync(void);

/* ------------------------------------------------------------------ (2) kernel level */

/* Layout of the LDS-resident ("pivot-stationary") distance kernel for an index: every chunk is padded
 * to psz floats (1,2,4,8 >= the largest chunk) and the chunk count to mp (a multiple of 4 with a
 * compiled kernel instance).  psz == 0 on return means "use the LUT path" (chunks wider than 8 dims or a
 * table that cannot fit the 160 KB LDS). */
int bang_pq_layout(const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t* psz_out, uint32_t* mp_out);

/* Host-side re-layout of the file-order pivot table [256][D]:
 * out[(c*256 + code)*psz + i] = pivots[code][chunk_off[c] + i], zero beyond the chunk and for c >= m.
 * out holds mp*256*psz floats. */
int bang_pack_pivots(const float* pivots, const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t psz,
                     uint32_t mp, float* out);
/* Exact-size table for layouts whose chunks have 2 dims first and then 1 (DiskANN's split when D/m is between 1 and 2, e.g.
 * 128 dims in 70 chunks, 96 in 74): [nhi][256][2] f32 followed by [mp - nhi][256][1], zero entries for the padding chunks, rounded up
 * to a multiple of 4 floats plus 4 (the kernel reads one float past a 1-dim entry).  *nhi_out = 0 and nothing is written if the
 * layout is not of that form.  out may be NULL to query the size.  256*D floats instead of 512*mp: 96 KB instead of 152 KB of LDS for
 * DEEP100M's layout, 128 KB instead of 144 KB for SIFT1B's. */
int bang_pack_pivots_ragged(const float* pivots, const uint32_t* chunk_off, uint32_t D, uint32_t m, uint32_t mp, uint32_t* nhi_out,
                            float* out, uint64_t* floats_out);

/* Centred queries in the same padded layout: d_qc[q][c*psz + i] = float(query[j]) - centroid[j],
 * j = chunk_off[c] + i (0 in the padding and beyond D - dim_adjust).  First half of
 * populate_pqDist_par (bang_search.cu:1099-1113,1124).  d_qc holds Q*mp*psz floats. */
int bang_k_center_queries(const void* d_queries, int dtype, const float* d_centroid, const uint32_t* d_chunk_off,
                          float* d_qc, uint32_t Q, uint32_t D, uint32_t m, uint32_t mp, uint32_t psz,
                          uint32_t dim_adjust, void* stream);

/* K1 populate_pqDist_par (bang_search.cu:1083-1130): d_lut [Q][m][256] f32. d_pivots_T is [D][256]. */
int bang_k_lut_build(const float* d_pivots_T, const void* d_queries, int dtype, const float* d_centroid,
                     const uint32_t* d_chunk_off, float* d_lut, uint32_t Q, uint32_t D, uint32_t m,
                     uint32_t dim_adjust, void* stream);

/* Parameters of the per-iteration kernels.  One row per query in every [Q][...] array. */
typedef struct {
  uint32_t Q, R, m, L, medoid, iter;   /* iter = reference's 1-based iteration number */
  uint32_t psz, mp;                    /* pivot layout (bang_pq_layout); psz == 0 => LUT path */
  uint32_t first;                      /* 1: use the seed list + compute_parent1 semantics */
  uint32_t max_wgs;                    /* cap on workgroups of the front kernel (0 = one per CU); lanes share the GPU */
  /* straggler compaction: when d_qmap != NULL the kernels iterate over Q SLOTS and slot s works on query d_qmap[s]
   * (all per-query arrays stay indexed by the query); n_all = number of queries behind the arrays (parents copy). */
  const uint32_t* d_qmap;
  uint32_t n_all;                      /* (bang_k_pqdist_stream: != 0 = the Q neighbour rows belong to n_all distinct queries, row q -> query q mod n_all) */
  /* inputs */
  const uint32_t* d_stage;             /* [Q][BANG_STAGE_STRIDE] staged adjacency {count, ids} (first==0) */
  const uint32_t* d_seed;              /* [1 + R+1] {count, MEDOID, adj(MEDOID)...}  (first==1) */
  const uint8_t* d_codes;              /* [N][m] + 256 B slack */
  const float* d_pivots_packed;        /* [mp][256][psz] (psz != 0); with pq_nhi != 0 (psz == 2): [pq_nhi][256][2] then [mp - pq_nhi][256][1] */
  const float* d_qc;                   /* [Q][mp*psz]                           (psz != 0) */
  const float* d_lut;                  /* [Q][m][256]                           (psz == 0) */
  /* graph-on-device mode: adjacency read by the kernel itself from d_graph via d_parents */
  const uint8_t* d_graph;              /* NULL in host-graph mode */
  uint64_t entry_len;
  uint32_t vec_bytes;                  /* D*sizeof(T): offset of the degree word inside an entry */
  /* state */
  uint32_t* d_bloom;                   /* [Q][BANG_BF_WORDS] bit-packed visited filter */
  uint32_t* d_nbrs;                    /* [Q][BANG_NBR_STRIDE] survivors of this iteration */
  float* d_dist;                       /* [Q][BANG_NBR_STRIDE] their PQ distances */
  uint32_t* d_cnt;                     /* [Q] survivor count */
  uint32_t* d_wl_ids;                  /* [Q][L] worklist */
  float* d_wl_dist;                    /* [Q][L] */
  uint8_t* d_wl_vis;                   /* [Q][L] */
  uint32_t* d_wl_cnt;                  /* [Q] */
  uint32_t* d_mark;                    /* [Q] */
  uint32_t* d_parents;                 /* [Q] parent id | BANG_NO_PARENT | BANG_IDLE_PARENT (device memory) */
  uint32_t* d_cand_ids;                /* [Q][L+50] expanded nodes (compact) */
  uint32_t* d_cand_row;                /* [Q][L+50] iteration row holding the node's vector */
  uint32_t* d_cand_cnt;                /* [Q] */
  uint32_t* d_active;                  /* [1] set to 1 if any query is still active (plain store; may be NULL) */
  uint32_t* d_qstats;                  /* [Q][2] per-query running totals {survivors, ids fetched} (may be NULL) */
  /* completion signal of the front kernel (host-graph mode): the last workgroup to finish stores done_value to
   * h_done_flag (mapped pinned host memory) after copying the parents to h_parents and a system-scope release, so the
   * walker thread can spin on it instead of calling into the HIP runtime.  d_done_count is a zero-initialised device word. NULL = off. */
  uint32_t* d_done_count;
  uint32_t* h_done_flag;
  unsigned long long* d_ktime;         /* [gridDim.x][2] per-workgroup {start,end} s_memrealtime stamps (100 MHz) of this launch, or NULL */
  uint32_t* h_parents;                 /* mapped pinned [Q]: the last workgroup copies d_parents there (coalesced) before the flag */
  uint32_t done_value;
  uint32_t pq_nhi;                     /* psz == 2 only: exact-size ("ragged") pivot table -- the first pq_nhi chunks have 2 dims, the rest 1
                                          (bang_pack_pivots_ragged); 0 = every chunk padded to psz floats (bang_pack_pivots) */
  uint32_t code_stride;                /* bytes between the code rows of consecutive nodes in d_codes; 0 = m (the packed layout of
                                          <p>_pq_compressed.bin).  128 for 64 < m <= 128: a row never leaves its 128-byte line */
} bang_iter_params;

/* Fused K5 + K2 + K4: neighbor_filtering_new (bang_search.cu:1140-1165) -> compute_neighborDist_par
 * (:1201-1241) -> compute_parent1 / compute_parent2 (:1464-1521 / :1384-1459), one wavefront per query. */
int bang_k_front(const bang_iter_params* p, void* stream);

/* ---- the query-resident search kernel (csrc/bang_search.hip) ----
 * ONE launch runs the whole search loop of a batch (bang_search.cu:650-958): K5 neighbor_filtering_new (:1140-1165) ->
 * K2 compute_neighborDist_par (:1201-1241) -> K4 compute_parent1/2 (:1464-1521 / :1384-1459) -> K3a/K3b
 * compute_BestLSets_par_sort_msort / _merge (:1533-1585 / :1605-1715), iteration after iteration.  A wavefront owns ONE query at a
 * time from its first iteration to its last (worklist, survivors and counters stay in LDS / registers) and then pulls the next
 * unstarted query from *d_next_query.  Graph resident in HBM (d_graph); the candidate log feeds bang_k_rerank.
 * Same per-query results as bang_k_front / bang_k_back iterated by a host loop. */
typedef struct {
  uint32_t Q, R, m, L, medoid;
  uint32_t cap_iter;                   /* last iteration a query may run: L + BANG_EXTRA_ITERS - 1 (bang_search.cu:950) */
  uint32_t psz, mp, pq_nhi;            /* pivot layout (bang_pq_layout / bang_pack_pivots[_ragged]); psz != 0 */
  uint32_t max_wgs, max_waves;         /* 0 = one workgroup per CU / as many waves per workgroup as LDS holds (<= 16) */
  const uint32_t* d_seed;              /* [2 + R + 1] {count, MEDOID, adj(MEDOID)...} */
  const uint8_t* d_codes;              /* [N][m] + 256 B slack */
  const float* d_pivots_packed;
  const float* d_qc;                   /* [Q][mp*psz] centred queries (bang_k_center_queries) */
  const uint8_t* d_graph;              /* [N][entry_len] */
  uint64_t entry_len;
  uint32_t vec_bytes;
  uint32_t row_layout;                 /* 0: d_graph = graph entries [vec][u32 degree][u32 id x R] at entry_len.  1: d_graph = ADJACENCY ROWS only,
                                          [N][64] u32 at a stride of 256 B, unused slots = 0xFFFFFFFF (BANG_ADJ_PAD) -- the layout the engine
                                          keeps in pinned HOST memory for the pull mode: the kernel fetches rows over PCIe by itself */
  uint32_t* d_bloom;                   /* [Q][BANG_BF_WORDS] visited filters, zeroed (bang_init) */
  uint32_t* d_cand_ids;                /* [Q][L + 50] out: expanded nodes in expansion order, [0] = MEDOID */
  uint32_t* d_cand_cnt;                /* [Q] out */
  uint32_t* d_qstats;                  /* [Q][2] out {distance evaluations, adjacency ids offered to the filter} or NULL */
  uint32_t* d_qiters;                  /* [Q] out: iterations the query ran, or NULL */
  uint32_t* d_next_query;              /* [1] hand-out counter, zeroed before the launch */
  unsigned long long* d_ktime;         /* [workgroups][2] {start, end} s_memrealtime stamps (100 MHz), or NULL */
  /* host-paced form (d_graph == NULL: graph in host RAM, bang_search.cu:771-813 stays on the CPU).  A wave holds nctx (1 or 2)
   * query contexts and the W waves of a workgroup (bang_search_geometry) form groups of group_waves waves; pacing GROUP grp =
   * (g * groups_per_workgroup + group) * nctx + c, whose v-th wave owns slot 16*grp + v.  Every round of a group the workgroup stores its parents to h_parents[slot] (BANG_NO_PARENT: nothing to fetch) and
   * then the round number to h_done[16 grp] (0xFFFFFFFF: the group has finished).  The walker writes the parents' adjacency ids to
   * d_rows[slot][64] and then the group's control line d_ctl[grp][16] = {round number (0xFFFFFFFF = stop), 16 count bytes, 0...} --
   * both in LOCAL fine-grained device memory, through the PCIe BAR, rows before the control line.  ship_vectors: the walker also
   * needs to know where an expanded node's full-precision vector goes in the vector log ([Q][L + 50][vec_bytes], by query and
   * candidate index): h_pub_q[slot] = query | (row wanted) << 31, h_pub_c[slot] = candidate index. */
  const uint32_t* d_rows;              /* [G*nctx*16][64] */
  const uint32_t* d_ctl;               /* [G*nctx][16] */
  uint32_t* h_done;                    /* mapped pinned [G*nctx][16] */
  uint32_t* h_parents;                 /* mapped pinned [G*nctx][16] */
  uint32_t* h_pub_q;                   /* mapped pinned [G*nctx][16] (ship_vectors) */
  uint32_t* h_pub_c;                   /* mapped pinned [G*nctx][16] (ship_vectors) */
  uint32_t* d_abort;                   /* [1] set when a workgroup gave up waiting for the host, or NULL */
  uint32_t ship_vectors;
  uint32_t nctx;                       /* 0 = auto (bang_search_geometry) */
  uint32_t group_waves;                /* waves per pacing group, 4..16 (0 = 8): a workgroup's W waves form ceil(W / group_waves) groups that
                                          advance independently; pacing group index = (g * groups_per_workgroup + group) * nctx + c */
  unsigned long long* d_prof;          /* diagnostic, host-paced form: [G][8] 100 MHz ticks thread 0 of each workgroup spent {waiting for
                                          rows, in the front half up to the publish barrier, publishing, in sort/merge}, [4] = half-rounds; or NULL */
  uint32_t code_stride;                /* bytes between code rows in d_codes; 0 = m (see bang_iter_params) */
  uint32_t n_rows_hbm;                 /* row_layout = 1: the adjacency rows of the nodes [0, n_rows_hbm) are ALSO in device memory at d_rows_hbm */
  const uint32_t* d_rows_hbm;          /* [n_rows_hbm][64] u32, or NULL */
  /* row_layout = 1, n_slices > 1 (peer rows): node p's row is read from d_row_slices[p / slice_rows] + p * 256 when p / slice_rows <
   * n_slices and that entry is not 0 (the entries are BIASED device addresses: slice s's first row is node s * slice_rows), else from
   * d_graph.  n_rows_hbm / d_rows_hbm are ignored then. */
  const uint64_t* d_row_slices;        /* [n_slices] device array of biased base addresses (this GPU's HBM or a peer's, hipIpcOpenMemHandle), or NULL */
  uint32_t n_slices, slice_rows;
  unsigned long long go_timeout_ticks; /* host-paced form: a pacing group that has waited this many 100 MHz ticks for its rows sets *d_abort and
                                          leaves (the host is gone); 0 = 30 s */
  uint32_t* d_qskip;                   /* [Q] out, or NULL: filter-word loads the query did NOT issue because its on-chip summary knew the
                                          word was still zero (self-paced form; 0 in the host-paced form) */
  uint32_t n_nodes;                    /* nodes of the index, or 0: an adjacency id >= n_nodes (and not the pad value) is never expanded nor evaluated -- the row
                                          counts as empty and *d_abort is set to 2 (a corrupt row must not become a wild read of the code table) */
  uint32_t summ_iters;                 /* self-paced form: the on-chip filter summary is consulted and maintained for a query's first summ_iters iterations only
                                          (0xFFFFFFFF = always; 0 = auto: always, except 1 -- i.e. off -- for launches of at most 5 queries per CU, where its
                                          LDS-crossbar work on the chain of every iteration costs more than the requests it saves) */
  uint32_t spec_rows;                  /* self-paced form, 70- and 74-chunk layouts (the other instances ignore it): the PQ code rows of ALL ids of an adjacency row are
                                          requested together with their filter probes (1) -- one memory latency less per iteration, the rows of the ids the
                                          filter drops fetched in vain -- or behind the filter, survivors only (2); 0 = auto: 1 where the rows are pulled (row_layout), and
                                          for launches of <= 8 queries per CU where the graph is in HBM. */
  uint32_t n_rows_pad;                 /* padded rows (engine option "rows_pad"; bang_k_search / bang_k_search_wf, self-paced form, row_layout = 1, n_slices <= 1, the
                                          70-chunk layout -- mp = 72 -- at code_stride = 128): the adjacency rows of the nodes [0, n_rows_pad) sit in d_codes itself,
                                          in the bytes of its lines behind the code (csrc/bang_pad_rows.h: 14 ids per line, 5 lines per row, 5 * n_rows_pad <=
                                          n_nodes), and d_rows_hbm holds the rows of the nodes [n_rows_pad, n_rows_pad + n_rows_hbm).  Non-zero anywhere else is
                                          BANG_ERR_ARG naming the member; the other entry points ignore it.  (It takes the four bytes of padding that lay between
                                          spec_rows and the pointer below: no member moves, sizeof is what it was, and a caller zeroes the struct before filling it.) */
  /* K6 + K7 FUSED into the launch (self-paced form, 8-bit vectors; compute_L2Dist :1254-1299, compute_NearestNeighbours :1312-1368): the wave
   * that finishes a query re-ranks its candidate log on the spot -- exact distances to the full-precision vectors at rr_vec_base + id *
   * rr_vec_stride, stable rank by (distance, expansion order) -- and writes the query's k results; no second launch behind the search, and
   * the re-rank of all but the last queries runs under the search of the others.  rr_queries == NULL: not fused (bang_k_rerank* follows).
   * 8-bit vectors: D % 16 == 0, D <= 256, D / 16 a power of two (D / 16 lanes per candidate, exact integers by v_dot4); float vectors: D % 4 == 0, D <= 256
   * (one lane per candidate runs the ascending fmaf chain); rr_vec_stride % 4 == 0, no MIPS padding (bang_search_can_rerank).  Same bits as bang_k_rerank. */
  const void* rr_queries;              /* [rr_Q_total][D] raw queries (u8 / i8 / f32), row rr_q0 + q belongs to this launch's query q */
  const uint8_t* rr_vec_base;
  uint64_t rr_vec_stride;
  uint64_t* rr_ids_out;                /* [rr_Q_total][k] */
  float* rr_dists_out;                 /* [k][rr_Q_total] (rank-major, :999) */
  uint32_t rr_dtype, rr_D, rr_k, rr_q0, rr_Q_total;
  /* bang_k_search_exact's pulled-rows form only (row_layout = 1, rr_dtype = BANG_F32): 1 = rr_vec_base holds IEEE fp16 rows at rr_vec_stride (a float
   * index loaded with option "vectors_fp16"); the query stays float.  rr_D % 8 == 0, rr_D <= 256.  Every other entry point ignores it.  (The newest
   * member: it takes the four bytes of padding that lay between rr_Q_total and the pointer below -- no member moves and sizeof is what it was.
   * bang_k_search_exact therefore READS bytes that used to be padding: a caller must zero the whole struct (memset) before filling it member by
   * member; garbage there is BANG_ERR_ARG (a value > 1) or, worse, the fp16 reading of a float table (a value of 1).) */
  uint32_t rr_vec_f16;
  /* bang_k_search_lut only (psz == 0): the per-query look-up tables of K1 (bang_k_lut_build), read-only for the launch; query q's table is
   * d_lut + q * m * 256.  The other entries ignore it.  (Appended last: the layout of every earlier member is unchanged.) */
  const float* d_lut;                  /* [Q][m][256] */
} bang_search_params;
/* 1 if a launch with these vectors can carry the fused re-rank (bang_search_params.rr_*) */
int bang_search_can_rerank(int dtype, uint32_t D, uint64_t vec_stride, uint32_t dim_adjust);
int bang_k_search(const bang_search_params* p, void* stream);
/* waves per workgroup that fit the 160 KB of LDS beside the pivot table at worklist length L (0: the kernel cannot run) */
int bang_search_supported(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L);
/* grid of a bang_k_search launch over Q queries: workgroups (<= CUs, <= max_wgs if nonzero), waves per workgroup (every wave that fits,
 * <= max_waves if nonzero; no more than a workgroup's share of Q needs; a self-paced batch of one to two wave-fulls per CU: half its share,
 * two equal rounds) and query contexts per wave (*nctx in: 0 = auto, out: 1 or 2) and, host-paced form, waves per pacing group (*group_waves in: 0 = auto = 8) */
int bang_search_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                         int host_paced, uint32_t* workgroups, uint32_t* waves, uint32_t* nctx, uint32_t* group_waves);

/* Fused K3a + K3b: compute_BestLSets_par_sort_msort (bang_search.cu:1533-1585) ->
 * compute_BestLSets_par_merge (:1605-1715), one wavefront per query. */
int bang_k_back(const bang_iter_params* p, void* stream);

/* Unfused stage entries (parity tests; same device code as the fused kernels). */
int bang_k_filter(const bang_iter_params* p, void* stream);   /* K5 only: d_stage/d_seed -> d_nbrs, d_cnt */
int bang_k_pqdist(const bang_iter_params* p, void* stream);   /* K2 only: d_nbrs,d_cnt -> d_dist */
int bang_k_parent(const bang_iter_params* p, void* stream);   /* K4 only */
/* K2 only, streaming form (csrc/bang_search.hip): the same distances as bang_k_pqdist for the first min(d_cnt[q], 64) neighbours of
 * every query (R <= 64: every row the search path ever produces but the 65-entry seed list), with the next row's ids and code rows in
 * flight while the current one is reduced.  This is the launch the K2-alone HBM roofline figure is measured on. */
int bang_k_pqdist_stream(const bang_iter_params* p, void* stream);

/* Fused K6 + K7: compute_L2Dist (bang_search.cu:1254-1299) -> compute_NearestNeighbours (:1312-1368).
 * Candidate i of query q has its vector at d_vec_base + (row*Q + q)*vec_stride (row = d_cand_row, host-graph
 * mode: the per-iteration vector log) or at d_vec_base + id*vec_stride (d_cand_row == NULL: graph on device).
 * d_ids_out [Q][k] u64; d_dists_out [k][Q] f32. */
int bang_k_rerank(const void* d_vec_base, uint64_t vec_stride, const void* d_medoid_vec, const void* d_queries,
                  int dtype, const uint32_t* d_cand_ids, const uint32_t* d_cand_row, const uint32_t* d_cand_cnt,
                  uint32_t cand_stride, uint32_t Q, uint32_t D, uint32_t k, uint32_t dim_adjust,
                  uint64_t* d_ids_out, float* d_dists_out, void* stream);

/* FP16 VECTOR TABLE (engine option "vectors_fp16" = 1: a float index on the host placement keeps its HBM vector table as IEEE fp16, half the bytes;
 * results are the usual arithmetic applied to the vectors rounded to fp16, bit for bit).
 *
 * bang_k_f32_to_f16: `rows` rows of D floats at d_src + r * src_stride -> rows of halves at d_dst + r * dst_stride (strides in bytes; both
 * divisible by 4, src_stride >= 4 D, dst_stride >= align4(2 D); both pointers 4-byte aligned).  Round to nearest even, fp16 subnormals produced;
 * for odd D the padding half behind a row is written as 0.  A FINITE source value that becomes +-inf (|x| >= 65520) is converted all the same and
 * counted in *d_bad_count (a device word the caller zeroed; may be NULL) -- the engine fails the load on a non-zero count.  inf stays inf, NaN
 * stays NaN. */
int bang_k_f32_to_f16(const void* d_src, void* d_dst, uint64_t rows, uint32_t D, uint64_t src_stride, uint64_t dst_stride,
                      uint32_t* d_bad_count, void* stream);
/* bang_k_rerank's device-vector form (d_cand_row == NULL) for float queries on an fp16 table: candidate id's row is d_vec_base + id * vec_stride
 * (vec_stride % 4 == 0, >= align4(2 D)); distance = the ascending chain diff = float(h[j]) - q[j], acc = fmaf(diff, diff, acc) over the D
 * dimensions (the query MIPS-padded by dim_adjust as in bang_k_rerank); the same stable rank.  Any D. */
int bang_k_rerank_f16(const void* d_vec_base, uint64_t vec_stride, const void* d_queries, const uint32_t* d_cand_ids,
                      const uint32_t* d_cand_cnt, uint32_t cand_stride, uint32_t Q, uint32_t D, uint32_t k, uint32_t dim_adjust,
                      uint64_t* d_ids_out, float* d_dists_out, void* stream);

/* EXACT-DISTANCE search kernel (csrc/bang_search_exact.hip; engine option "distance" = 1; the reference's BANG_Exactdistance,
 * BANG_Exactdistance/parANN.cu:1139-1179, :1275): the loop of bang_k_search with every neighbour's distance the exact L2 against its full-precision
 * vector -- the first vec_bytes of its graph entry in d_graph (row_layout 0: graph in HBM; row_layout 1: below) -- and no re-rank: each query's results are the
 * first min(k, worklist length) worklist entries when its loop ends (padded with UINT64_MAX / 3.402823E+38f), written to rr_ids_out [rr_Q_total][k]
 * (u64) / rr_dists_out [k][rr_Q_total] at row rr_q0 + q.  Uses Q, R, L, medoid, cap_iter, max_wgs, max_waves, d_seed, d_graph, entry_len,
 * vec_bytes, d_bloom (zeroed), d_cand_ids / d_cand_cnt (the expanded nodes, [0] = MEDOID), d_qstats, d_qiters, d_next_query (zeroed), d_abort,
 * d_ktime, n_nodes and rr_queries (raw queries), rr_dtype, rr_D, rr_k, rr_q0, rr_Q_total, rr_ids_out, rr_dists_out; the PQ fields and rr_vec_* are
 * ignored.  Vector layouts: bang_search_exact_supported(rr_dtype, rr_D, entry_len); others are BANG_ERR_UNSUPPORTED.  The layouts of the fused re-rank
 * (bang_search_can_rerank with rr_vec_stride = entry_len) run on the instances that share its arithmetic, the others -- D up to BANG_EXACT_MAX_D,
 * 8-bit vectors with any D / 16 -- on the wide instances (rows fetched cooperatively through an LDS tile; 8-bit sums leave the integers at 2^24 and
 * continue as orc_exact_dist's float chain).  Same bits as bang_k_rerank either way.
 *
 * PULLED ROWS (row_layout = 1; engine: graph = host with pull = 1 given explicitly): the adjacency lists are the 256-byte rows bang_k_search's
 * self-paced form reads -- 64 ids, the unused slots behind them BANG_ADJ_PAD -- and a node's vector sits at rr_vec_base + id * rr_vec_stride (the
 * packed table in HBM).  The row of node x is read from slice x / slice_rows of d_row_slices where n_slices > 1 (biased base addresses; a zero entry
 * or a slice past the table: from d_graph), else from d_rows_hbm where x < n_rows_hbm, else from d_graph (pinned host memory, over PCIe, with the
 * non-temporal hint).  Contract: d_graph = the rows, 4-byte aligned; rr_vec_base non-null and 4-byte aligned;
 * bang_search_exact_supported(rr_dtype, rr_D, rr_vec_stride); vec_bytes == rr_D * the element size; R <= 64; n_slices > 1 needs d_row_slices and
 * slice_rows != 0; n_rows_hbm != 0 needs d_rows_hbm.  A violation is BANG_ERR_ARG with a message naming the member; entry_len is ignored.  An id
 * >= n_nodes in a row -- the pad value in front of an id included, also where n_nodes == 0 -- is never followed (*d_abort = 2).  Results, counters
 * and candidate log are those of the graph-entry form, bit for bit.  row_layout > 1 is BANG_ERR_UNSUPPORTED.  Arguments are checked before any HIP
 * call in both forms. */
int bang_k_search_exact(const bang_search_params* p, void* stream);
/* grid of a bang_k_search_exact launch (layouts of bang_search_can_rerank) over Q queries for vectors of dtype at worklist length L: workgroups and waves per workgroup (as many
 * waves per CU as the instance's registers and LDS allow, <= 16 per workgroup; max_wgs / max_waves: caps if nonzero; a batch of fewer than a
 * workgroup-full of queries per CU is spread over all CUs) */
int bang_search_exact_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
/* the same for a launch of the pulled-rows form (row_layout = 1): the register count read is that of the pulled instance */
int bang_search_exact_pull_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
/* ... and of the pulled-rows form on an fp16 vector table (rr_vec_f16 = 1; dtype must be BANG_F32): the register count of that instance */
int bang_search_exact_pull_f16_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);

/* BEAM form of the exact-distance search kernel (csrc/bang_search_beam.hip; engine options "distance" = 1 and "beam" = W, 2 <= W <= 4): up to beam
 * parents are expanded per iteration.  Every id of the <= beam adjacency rows of an iteration is tested against the filter state at the
 * iteration's entry, then the survivors' bits are set; a survivor whose id also survived in an earlier row of the iteration is dropped; the rows
 * are sorted and merged one after the other with no mark; then the first P = min(beam, room in the candidate log, unvisited entries) unvisited
 * worklist entries are marked visited, logged in d_cand_ids and expanded together.  P == 0 ends the query; at iteration cap_iter the parents are
 * logged, not expanded.  Results as bang_k_search_exact: the first min(k, worklist length) worklist entries.  beam = 1 is the post-merge-parent walk
 * with exact distances (NOT the walk of bang_k_search_exact); the engine never launches it.
 * Arguments and their checks are those of bang_k_search_exact in both forms (row_layout 0: graph entries in HBM; 1: pulled rows), all made before
 * any HIP call; beam travels as an argument -- bang_search_params is what it was.  Refused, with a message naming beam: beam == 0 or beam > 4
 * (BANG_ERR_ARG); rr_vec_f16 = 1 and the wide layouts, i.e. those bang_search_exact_beam_supported refuses (BANG_ERR_UNSUPPORTED). */
int bang_k_search_exact_beam(const bang_search_params* p, uint32_t beam, void* stream);
/* 1 if the beam form evaluates vectors of this layout: bang_search_exact_supported and bang_search_can_rerank (8-bit: D % 16 == 0, D / 16 a power
 * of two; float: D % 4 == 0; D <= 256; a stride divisible by 4 that holds the vector) */
int bang_search_exact_beam_supported(int dtype, uint32_t D, uint64_t stride);
/* grid of a bang_k_search_exact_beam launch, as bang_search_exact_geometry; LDS per wave is 2L + L/4 + 144 + 2 (64 beam + 4) words */
int bang_search_exact_beam_geometry(int dtype, uint32_t L, uint32_t beam, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
/* the same for the pulled-rows form (row_layout = 1) */
int bang_search_exact_beam_pull_geometry(int dtype, uint32_t L, uint32_t beam, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);

/* BANG_INMEMORY SEMANTICS of the query-resident search kernel (csrc/bang_search.hip built as bang_search_inmem.o / bang_search_inmem_b.o; engine
 * option "semantics" = 1; the reference's BANG_Inmemory, BANG_Inmemory/parANN.cu:1287-1420): the loop of bang_k_search with the parent taken AFTER
 * the merge -- the first unvisited worklist entry, marked visited -- and an iteration cap of L + 119 (cap_iter <= L + BANG_INMEM_EXTRA_ITERS - 1; the
 * candidate log d_cand_ids has a stride of L + BANG_INMEM_EXTRA_ITERS).  Graph entries in HBM only (d_graph, row_layout 0); spec_rows is ignored (off).
 * Arguments otherwise as for bang_k_search's self-paced form, the fused re-rank (rr_*) included. */
int bang_k_search_inmem(const bang_search_params* p, void* stream);
/* grid of a bang_k_search_inmem launch: that of bang_search_geometry's self-paced form (host_paced = 0) */
int bang_search_inmem_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                               uint32_t* workgroups, uint32_t* waves);

/* WORD-LOCAL VISITED FILTER of the query-resident search kernel (csrc/bang_search.hip built as bang_search_wf.o / bang_search_wf_b.o; engine option
 * "filter_layout" = 1): the loop of bang_k_search, self-paced form only (d_graph != NULL: graph entries in HBM, or
 * row_layout = 1 with the pulled rows, their HBM copy and peer slices), with both filter bits of an id x in ONE word of the query's filter: word
 * hash1(x) >> 5, bits hash1(x) & 31 and (hash2(x) >> 5) & 31 (one bit where they coincide).  An id is dropped iff all bits of its mask are set in
 * the word as it stood at the iteration's entry; a survivor sets its mask.  The filter memory (BANG_BF_WORDS words per query, zeroed by the
 * caller) and bang_search_params are what they are for bang_k_search; spec_rows, summ_iters, the fused re-rank and the counters work as there.
 * Results differ from bang_k_search's only where the two layouts drop different ids. */
int bang_k_search_wf(const bang_search_params* p, void* stream);
/* grid of a bang_k_search_wf launch: that of bang_search_geometry's self-paced form (host_paced = 0) */
int bang_search_wf_geometry(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                            uint32_t* workgroups, uint32_t* waves);
/* 1 if a search_wf_kernel instance exists for this pivot layout and code-row stride (every layout bang_k_search dispatches, rows dword-aligned or not) */
int bang_search_wf_has_instance(uint32_t psz, uint32_t mp, uint32_t code_stride);

/* LUT-PATH search kernel (csrc/bang_search_lut.hip; engine option "search" = 1 on an index with psz == 0: chunks wider than 8 dimensions, a pivot
 * table too large for LDS, or option "pq" = 1): the loop of bang_k_search's self-paced form -- one wave per query from its first iteration to its
 * last, worklist in LDS, one launch per batch -- with every neighbour's PQ distance gathered from the query's look-up table d_lut (K1,
 * bang_k_lut_build) in the arithmetic of the per-iteration kernels (compute_neighborDist_par, bang_search.cu:1229-1239: the same bits).  Any m,
 * any code_stride.  The result is the candidate log (d_cand_ids [Q][L + 50], d_cand_cnt); bang_k_rerank follows.  Graph entries in HBM only
 * (d_graph, row_layout 0) and psz == 0, else BANG_ERR_UNSUPPORTED.  Uses Q, R, m, L, medoid, cap_iter, max_wgs, max_waves, d_seed, d_codes,
 * code_stride, d_graph, entry_len, vec_bytes, d_bloom (zeroed), d_cand_ids, d_cand_cnt, d_qstats, d_qiters, d_next_query (zeroed), d_abort,
 * d_ktime, n_nodes and d_lut; the pivot-table fields and rr_* are ignored.  Arguments are checked before any HIP call. */
int bang_k_search_lut(const bang_search_params* p, void* stream);
/* 1 if one wave's state (2L + L/4 + 144 words of LDS) fits: m >= 1 and 1 <= L <= BANG_MAX_L; else 0 */
int bang_search_lut_supported(uint32_t m, uint32_t L);
/* grid of a bang_k_search_lut launch over Q queries at worklist length L: as bang_search_exact_geometry (waves per CU from the instance's
 * registers and LDS, <= 16 per workgroup; max_wgs / max_waves: caps if nonzero; small batches spread over all CUs) */
int bang_search_lut_geometry(uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);

/* EXCLUDED IDS, device side (csrc/bang_exclude.hip; engine: bang_set_excluded_e).  d_bitmap holds bit (id & 31) of word id >> 5 for every id of the
 * set: ceil(n_nodes / 32) words plus one word of slack.  An id >= n_nodes is in no set and is never looked up.  Both kernels: one wave per query,
 * four waves per workgroup, no LDS; both entries check their arguments before any HIP call -- a null buffer, cand_stride = 0, k = 0, k > L,
 * Q_total = 0 or < q0 + nq is BANG_ERR_ARG with the member named -- and nq = 0 is no launch.
 *
 * bang_k_cand_live, the PQ walks: for the queries q0 .. q0 + nq - 1 (rows of the [Q][cand_stride] arrays, as in bang_k_rerank's sub-range form) the
 * first min(d_cand_cnt[q], cand_stride) entries of the candidate log row d_cand_ids[q] that are NOT in the set go to d_live_ids[q], in log order,
 * their number to d_live_cnt[q].  The log and its counts are only read.  bang_k_rerank / bang_k_rerank_f16 then take d_live_ids / d_live_cnt where
 * they took the log: same arithmetic, same stable rank, ties in expansion order. */
int bang_k_cand_live(const uint32_t* d_cand_ids, const uint32_t* d_cand_cnt, uint32_t cand_stride, uint32_t q0, uint32_t nq,
                     const uint32_t* d_bitmap, uint32_t n_nodes, uint32_t* d_live_ids, uint32_t* d_live_cnt, void* stream);
/* bang_k_worklist_pick, the exact-distance walks: the input is what bang_k_search_exact / _beam write at rr_k = L -- d_wl_ids [Q_total][L] u64, the
 * whole final worklist of a query (UINT64_MAX behind a short one), and d_wl_dists [L][Q_total] f32, rank-major.  For the queries q0 .. q0 + nq - 1
 * the first k entries in worklist order that are not in the set go to d_ids_out [Q_total][k] / d_dists_out [k][Q_total], distance bits unchanged;
 * every copy of an id that the worklist holds twice is kept or dropped alike; an entry UINT64_MAX ends the scan; the tail is padded with
 * UINT64_MAX / 3.402823E+38f.  The outputs must not be the inputs. */
int bang_k_worklist_pick(const uint64_t* d_wl_ids, const float* d_wl_dists, uint32_t L, uint32_t q0, uint32_t nq, uint32_t Q_total,
                         const uint32_t* d_bitmap, uint32_t n_nodes, uint32_t k, uint64_t* d_ids_out, float* d_dists_out, void* stream);

/* LABEL FILTERS on the exact-distance walk (csrc/bang_search_exact.hip built as bang_search_exact_labels.o / bang_search_exact_labels_pull.o; engine:
 * bang_set_labels_e + bang_set_query_filters_e; DESIGN.md section 2, CANON 18).  Every node carries a 32-bit label word, every query two words:
 * node x MATCHES query q when (any == 0 || (d_labels[x] & any) != 0) && (d_labels[x] & all) == all; any = all = 0 matches every node.  The walk is
 * bang_k_search_exact's, bit for bit -- filter, parent, worklist, the L + 49 cap, candidate log, counters.  Beside its worklist a query keeps a
 * RESULT LIST of capacity L: in every iteration whose survivors are merged into the worklist (not the cap iteration) the matching survivors that
 * are not in d_excluded are taken in input order, with the distance bits the walk computed, and merged into the result list by the worklist's own
 * K3a + K3b rule (stable rank sort; a full list takes only entries strictly closer than its last; new before equal old; an empty list takes the
 * first min(n, L) sorted survivors).  The query's results are the first k entries of that list, padded with UINT64_MAX / 3.402823E+38f; an id that
 * a row lists twice is in twice, as in the worklist.  d_matched[rr_q0 + q] = the number of matching survivors offered to the list.  An unfiltered
 * query returns exactly what bang_k_search_exact returns.
 * bang_search_params is what it is for bang_k_search_exact (no member added or moved); the new arguments travel beside it.  Routed on row_layout to
 * search_exact_labels_kernel (0) / search_exact_labels_pull_kernel (1).  Every check of bang_k_search_exact is made, before any HIP call; refused in
 * addition, with the member named: f, d_labels or d_filters null and n_nodes == 0 -- the tables are indexed by node id -- (BANG_ERR_ARG);
 * rr_vec_f16 = 1 and the layouts of the wide instances, i.e. those bang_search_can_rerank refuses (BANG_ERR_UNSUPPORTED). */
typedef struct {
  const uint32_t* d_labels;   /* [n_nodes] */
  const uint32_t* d_filters;  /* [rr_Q_total][2] {any, all}; row rr_q0 + q is this launch's query q */
  const uint32_t* d_excluded; /* bitmap as bang_k_worklist_pick reads it, or NULL */
  uint32_t* d_matched;        /* [rr_Q_total] out, or NULL */
} bang_label_filter;
int bang_k_search_exact_labels(const bang_search_params* p, const bang_label_filter* f, void* stream);
/* grid of a bang_k_search_exact_labels launch, as bang_search_exact_geometry: LDS per wave is 2 (2L + L/4) + 144 words (worklist + result list), the
 * register count that of the label-filter instance; the second one for the pulled-rows form (row_layout = 1) */
int bang_search_exact_labels_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
int bang_search_exact_labels_pull_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);

/* RANGE SEARCH on the exact-distance walk (csrc/bang_search_exact.hip built as bang_search_exact_range.o / bang_search_exact_range_pull.o; engine:
 * option range_hits + bang_set_query_radii_e; DESIGN.md section 2, CANON 19).  The walk and the results are bang_k_search_exact's, bit for bit --
 * filter, parent, worklist, the L + 49 cap, candidate log, counters, the k results (rr_k = L with bang_k_worklist_pick behind the launch works as
 * ever).  Beside them query q collects a HIT LOG: in EVERY iteration, the first with its up-to-65-id seed list and the cap iteration (whose
 * survivors are evaluated but not merged) included, each survivor x with dist(x) <= d_radius[rr_q0 + q] -- a plain float compare on the squared-L2
 * bits the walk computed, so a NaN or negative radius admits nothing and +inf every evaluated node -- that is not in d_excluded is appended in
 * input order (element 64 of the seed list behind the first 64): id to d_hit_ids[(rr_q0 + q) * cap + i], distance bits to d_hit_dists at the same
 * place, for the first `cap` hits in evaluation order; d_offered[rr_q0 + q] counts ALL hits (offered > cap: the row was truncated).  An id that a
 * row lists twice is evaluated twice and logged twice; bang_k_range_sort drops the copy.  Row positions at and behind min(offered, cap) are not
 * written.
 * bang_search_params is what it is for bang_k_search_exact (no member added or moved); the new arguments travel beside it.  Routed on row_layout to
 * search_exact_range_kernel (0) / search_exact_range_pull_kernel (1).  Every check of bang_k_search_exact is made, before any HIP call; refused in
 * addition, with the member named: r, d_radius, d_hit_ids, d_hit_dists or d_offered null, cap = 0 or cap > BANG_RANGE_MAX_HITS, d_excluded set
 * with n_nodes == 0 -- the bitmap is indexed by node id -- (BANG_ERR_ARG); rr_vec_f16 = 1 and the layouts of the wide instances, i.e. those
 * bang_search_can_rerank refuses (BANG_ERR_UNSUPPORTED). */
#define BANG_RANGE_MAX_HITS 4096u
typedef struct {
  const float*    d_radius;    /* [rr_Q_total]; row rr_q0 + q is this launch's query q */
  const uint32_t* d_excluded;  /* bitmap as bang_k_worklist_pick reads it, or NULL */
  uint32_t*       d_hit_ids;   /* [rr_Q_total][cap] out */
  float*          d_hit_dists; /* [rr_Q_total][cap] out */
  uint32_t*       d_offered;   /* [rr_Q_total] out */
  uint32_t        cap;         /* 1 .. BANG_RANGE_MAX_HITS (4096) */
} bang_range_out;
int bang_k_search_exact_range(const bang_search_params* p, const bang_range_out* r, void* stream);
/* grid of a bang_k_search_exact_range launch, as bang_search_exact_geometry (the hit log lives in HBM: LDS per wave is the plain build's), the
 * register count that of the range instance; the second one for the pulled-rows form (row_layout = 1) */
int bang_search_exact_range_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
int bang_search_exact_range_pull_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
/* bang_k_range_sort (csrc/bang_range.hip, range_sort_kernel), behind a bang_k_search_exact_range launch on the same stream: for the queries
 * q0 .. q0 + nq - 1, the n = min(d_offered[q], cap) hits of row q are sorted ascending by the 64-bit key (distance bits << 32) | id -- squared
 * distances are non-negative, so their bit patterns order like the floats; equal distances order by id -- adjacent equal keys are dropped, the row
 * is written back in place and d_count[q] = what remains.  One wave per query; a row of more than 64 keys is sorted in 8 x (n rounded up to a power of two)
 * bytes of LDS, at most 32 KB.  Checked before any HIP call, with the argument named (BANG_ERR_ARG): a null buffer, cap = 0 or
 * cap > BANG_RANGE_MAX_HITS, Q_total < q0 + nq.  nq = 0 is no launch. */
int bang_k_range_sort(uint32_t* d_hit_ids, float* d_hit_dists, const uint32_t* d_offered, uint32_t cap, uint32_t q0, uint32_t nq, uint32_t Q_total,
                      uint32_t* d_count, void* stream);

/* INSERTS, device side (csrc/bang_insert.hip; engine: bang_insert_e; DESIGN.md section 2 CANON 21, section 4.15).  Layouts are those of
 * bang_search_can_rerank with the entry stride as the vector stride (8-bit: D % 16 == 0, D / 16 a power of two; float: D % 4 == 0; D <= 256); the
 * wide layouts are BANG_ERR_UNSUPPORTED.  Every entry checks its arguments before any HIP call and names the offending one.
 *
 * bang_k_prune (prune_kernel): RobustPrune of n_lists ordered candidate lists on squared distances.  List i is the first
 * min(d_list_cnt[i], list_stride, BANG_PRUNE_MAX_LIST) entries (c_j, d_j) of row i of d_list_ids / d_list_dists.  An entry whose id is d_own[i] is
 * dropped.  Walking j ascending: an alive c_j is appended to the row, and the walk stops once the row holds R ids; otherwise every alive c_t, t > j,
 * gets e = the exact distance of vector(c_t) to the query vector(c_j) -- exact_dist8 / exact_dist_f32, the arithmetic of bang_k_search_exact -- and
 * dies if alpha2 * e <= d_t (one float32 multiply, one float32 compare).  The row goes to d_out + (out_by_own ? d_own[i] : i) * out_stride as
 * [u32 degree][u32 id x R], unused slots 0.  d_own[i] == BANG_PRUNE_SKIP: list i is skipped and nothing is written for it.  An id >= n_nodes in a
 * list is never dereferenced: the list counts as ended in front of it and *d_abort = 2 (out_by_own with d_own[i] >= n_nodes: skipped, *d_abort = 2).
 * Wave-resident, one list per wave at a time, full workgroups sized by bang_wave_geometry (max_wgs / max_waves: caps if nonzero); wave w of the
 * launch takes the lists w, w + waves, ... */
#define BANG_PRUNE_MAX_LIST 512u
#define BANG_PRUNE_SKIP 0xFFFFFFFFu
typedef struct {
  const uint8_t* d_graph;      /* [n_nodes][entry_len]: a node's vector opens its entry */
  uint64_t entry_len;
  uint32_t dtype, D, n_nodes, R;
  float alpha2;                /* fl32(alpha) * fl32(alpha) rounded to float32, in [1, 64] */
  uint32_t n_lists, list_stride;
  const uint32_t* d_list_ids;  /* [n_lists][list_stride] */
  const float* d_list_dists;   /* [n_lists][list_stride] */
  const uint32_t* d_list_cnt;  /* [n_lists] */
  const uint32_t* d_own;       /* [n_lists] */
  void* d_out;
  uint64_t out_stride;         /* bytes, divisible by 4, >= 4 (R + 1) */
  uint32_t out_by_own;
  uint32_t max_wgs, max_waves;
  uint32_t* d_abort;           /* [1] or NULL */
} bang_prune_params;
int bang_k_prune(const bang_prune_params* p, void* stream);
/* bang_k_worklist_lists: what bang_k_search_exact wrote at rr_k = L (d_wl_ids [Q_total][L] u64, d_wl_dists [L][Q_total]) as candidate lists for
 * bang_k_prune, for the queries q0 .. q0 + nq - 1: row q of d_list_ids / d_list_dists ([Q_total][list_stride], list_stride >= L) holds the worklist
 * entries in worklist order, d_list_cnt[q] the number in front of the first pad entry. */
int bang_k_worklist_lists(const uint64_t* d_wl_ids, const float* d_wl_dists, uint32_t L, uint32_t q0, uint32_t nq, uint32_t Q_total,
                          uint32_t* d_list_ids, float* d_list_dists, uint32_t list_stride, uint32_t* d_list_cnt, void* stream);
/* bang_k_backedge: one wave per target.  Target i is the old node t = d_targets[i] (t < n_old, else it is skipped and *d_abort = 2) and
 * I_t = d_srcs[d_offs[i] .. d_offs[i + 1]) the new ids that list it.  deg_t + |I_t| <= R: I_t is appended to t's row in its graph entry,
 * d_offered[i] = 0, d_own_out[i] = BANG_PRUNE_SKIP.  Otherwise row i of d_cand_ids / d_cand_dists ([n_targets][BANG_PRUNE_MAX_LIST]) receives the
 * old row followed by I_t, cut at BANG_PRUNE_MAX_LIST entries, and each one's exact distance to the query vector(t); d_offered[i] = their number,
 * d_own_out[i] = t.  bang_k_range_sort (cap = BANG_PRUNE_MAX_LIST) and bang_k_prune (out_by_own) then write t's row.  d_stats[0..2] are incremented
 * by the rows appended, the rows handed to the prune and the incoming ids the cut dropped. */
typedef struct {
  uint8_t* d_graph;
  uint64_t entry_len;
  uint32_t dtype, D, R, n_nodes, n_old, n_targets;
  const uint32_t* d_targets;   /* [n_targets] */
  const uint32_t* d_offs;      /* [n_targets + 1] */
  const uint32_t* d_srcs;
  uint32_t* d_cand_ids;
  float* d_cand_dists;
  uint32_t* d_offered;         /* [n_targets] */
  uint32_t* d_own_out;         /* [n_targets] */
  uint32_t* d_stats;           /* [3] */
  uint32_t* d_abort;           /* [1] or NULL */
} bang_backedge_params;
int bang_k_backedge(const bang_backedge_params* p, void* stream);
/* bang_k_pq_encode (pq_argmin_kernel behind bang_k_lut_build): the PQ codes of n vectors ([n][D], packed).  code[c] of a vector is the lowest k
 * that minimises lut[c][k], K1's table with the vector as the query.  Row i goes to d_codes + i * code_stride (>= m), its bytes behind m written 0.
 * d_lut holds the tables of lut_points vectors (lut_points * m * 256 floats): the batch runs in chunks of that many. */
int bang_k_pq_encode(const float* d_pivots_T, const void* d_vectors, int dtype, const float* d_centroid, const uint32_t* d_chunk_off,
                     float* d_lut, uint32_t lut_points, uint32_t n, uint32_t D, uint32_t m, uint8_t* d_codes, uint64_t code_stride, void* stream);
/* Host side of an insert, no HIP call in it (csrc/bang_insert_group.cpp): the new rows of a batch grouped by target.  rows: n rows of row_stride
 * words {degree, ids...} (row i belongs to the new node first_id + i).  Every (target, source) pair is sorted and the CSR written: targets
 * ascending, offs, srcs (the new ids that list a target, ascending); the three arrays hold n * R, n * R + 1 and n * R words, R = row_stride - 1.
 * BANG_ERR_ARG (no message) on a null argument, row_stride < 2, a degree > R or an id >= n_old. */
int bang_insert_group(const uint32_t* rows, uint32_t n, uint32_t row_stride, uint32_t first_id, uint32_t n_old, uint32_t* targets, uint32_t* offs,
                      uint32_t* srcs, uint32_t* n_targets);

/* CONSOLIDATION, device side (csrc/bang_consolidate.hip; engine: bang_consolidate_e; DESIGN.md section 2 CANON 22, section 4.16).  d_excluded is the
 * exclusion bitmap X as bang_k_worklist_pick reads it (ceil(n_nodes / 32) words plus one of slack); a node is REMOVED when its id is < n_nodes, is
 * not `medoid` and has its bit set (D = X \ {medoid}).  row(p) is the first min(degree word, R) ids of p's row, read as ending in front of its
 * first id >= n_nodes: such an id is never dereferenced and *d_abort = 2.  Layouts are those of bang_k_backedge (the entry stride holds vector
 * and row); the wide layouts are BANG_ERR_UNSUPPORTED.  Every entry checks its arguments before any HIP call and names the offending one:
 * a null or misaligned d_graph, d_excluded null, R outside [1, 64], n_nodes = 0, medoid >= n_nodes, a null output (BANG_ERR_ARG).
 *
 * bang_k_consolidate_scan: one wave per node over [0, n_nodes).  Bit p of d_affected (ceil(n_nodes / 32) words, ZEROED BY THE CALLER) is set
 * when p is not removed and row(p) lists a removed node.  Nothing else is written. */
typedef struct {
  const uint8_t* d_graph;      /* [n_nodes][entry_len] */
  uint64_t entry_len;
  uint32_t dtype, D, R, n_nodes, medoid;
  const uint32_t* d_excluded;
  uint32_t* d_affected;        /* [ceil(n_nodes / 32)] */
  uint32_t* d_abort;           /* [1] or NULL */
} bang_consolidate_scan_params;
int bang_k_consolidate_scan(const bang_consolidate_scan_params* p, void* stream);
/* bang_k_consolidate_gather: one wave per list.  List i belongs to node p = d_nodes[i] (p >= n_nodes: d_offered[i] = 0, d_own_out[i] =
 * BANG_PRUNE_SKIP, *d_abort = 2).  Its candidates, in this order: the ids of row(p) that are not removed, in row order; then, for each removed v of
 * row(p) in row order, the ids of row(v) that are neither removed nor p, in row order.  Duplicates stay.  The first BANG_PRUNE_MAX_LIST of them go
 * to row i of d_cand_ids ([n_lists][BANG_PRUNE_MAX_LIST]), each one's exact distance to the query vector(p) -- exact_dist8 / exact_dist_f32 -- to
 * the same place of d_cand_dists; d_offered[i] = their number (0: nothing of the row is written), d_own_out[i] = p; d_stats[0] is incremented by
 * the candidates the cut dropped.  bang_k_range_sort (cap = BANG_PRUNE_MAX_LIST) and bang_k_prune (out_by_own) then write p's row.  The graph is
 * only read. */
typedef struct {
  const uint8_t* d_graph;
  uint64_t entry_len;
  uint32_t dtype, D, R, n_nodes, medoid, n_lists;
  const uint32_t* d_excluded;
  const uint32_t* d_nodes;     /* [n_lists] */
  uint32_t* d_cand_ids;
  float* d_cand_dists;
  uint32_t* d_offered;         /* [n_lists] */
  uint32_t* d_own_out;         /* [n_lists] */
  uint32_t* d_stats;           /* [1] */
  uint32_t* d_abort;           /* [1] or NULL */
} bang_consolidate_gather_params;
int bang_k_consolidate_gather(const bang_consolidate_gather_params* p, void* stream);
/* bang_k_consolidate_clear: one wave per node over [0, n_nodes); the row of every removed node becomes R + 1 zero words (degree 0, every slot 0).
 * Its vector, and every other node's entry, are not written. */
typedef struct {
  uint8_t* d_graph;
  uint64_t entry_len;
  uint32_t dtype, D, R, n_nodes, medoid;
  const uint32_t* d_excluded;
} bang_consolidate_clear_params;
int bang_k_consolidate_clear(const bang_consolidate_clear_params* p, void* stream);
/* Host side of a consolidation, no HIP call in it (csrc/bang_consolidate_group.cpp): the affected bitmap as the ascending list of its node ids.
 * bitmap holds ceil(n_nodes / 32) words; bits of the last word at or behind n_nodes are ignored.  ids holds up to n_nodes words.  BANG_ERR_ARG
 * (no message) on a null argument. */
int bang_consolidate_group(const uint32_t* bitmap, uint32_t n_nodes, uint32_t* ids, uint32_t* n_ids);

/* EXACT SCAN (csrc/bang_scan.hip, bang_scan_host.cpp, bang_scan_engine.cpp; DESIGN.md section 2 CANON 23, section 4.17): the k nearest of EVERY
 * live point, by brute force.  The CANDIDATES of query q are the node ids x < N that are not in the exclusion set, were not removed by a
 * consolidation of this load and match q's filter by the rule of bang_set_query_filters_e (any = all = 0, or any == all == NULL: every node).
 * A candidate's distance is the exact one of the narrow layouts (8-bit: the integer as a float; float: the ascending fmaf chain); the answer is the
 * k smallest keys (distance bits << 32) | id, ascending -- equal distances in id order --, whatever the tiling; ids_out [nq][k] u64 and
 * dists_out [k][nq] f32 as bang_query_e's, a short answer padded with UINT64_MAX / 3.402823E+38f; matched_out[q] (may be NULL) = the number of
 * candidates.  The call reads the engine's tables only, allocates and frees its own scratch and runs with or without a live allocation; batches
 * are cut into chunks inside.  Vectors come from the graph entries in HBM or, host placement, from the packed vector table.
 * Refused before any HIP call, nothing written: a null engine, nothing loaded, null queries / outputs, nq = 0 or > BANG_SCAN_MAX_QUERIES, k = 0 or
 * > BANG_SCAN_MAX_K, exactly one of any / all, filters without a label table, float queries that bang_check_floats refuses (BANG_ERR_ARG); MIPS
 * search parameters, an fp16 vector table, no resident vectors, a layout outside bang_search_can_rerank (BANG_ERR_UNSUPPORTED).
 * The removed set is not part of an index file: a reloaded index is scanned with its removed nodes until bang_set_removed_e restores the set. */
#define BANG_SCAN_MAX_K 128u
#define BANG_SCAN_MAX_QUERIES (1u << 20)
#define BANG_SCAN_MAX_KEYS 4096u              /* stripes * k: what bang_k_range_sort merges per query */
int bang_scan_e(bang_engine_t* e, const void* h_queries, uint32_t nq, uint32_t k, const uint32_t* any, const uint32_t* all, uint64_t* ids_out,
                float* dists_out, uint32_t* matched_out);
int bang_get_scan_times(bang_engine_t* e, double* ms3);        /* the last bang_scan_e: scan launches, merge (GPU time), the whole call (host) */
/* Kernel level: device pointers only, every argument checked before any HIP call with the member named.  Workgroups take a tile of queries (32 for
 * 8-bit vectors, on the i8 MFMA; 16 for float vectors) and one of `stripes` stripes of the points [0, n_nodes); each (query, stripe) leaves at most
 * k keys in d_scratch, bang_k_range_sort merges a query's stripes and a last kernel writes the outputs.  stripes = 0: bang_scan_geometry's choice;
 * else 1 <= stripes, stripes * k <= BANG_SCAN_MAX_KEYS and stripes <= ceil(n_nodes / points per round) (128 for 8-bit, 256 for float vectors).
 * d_excluded / d_removed: bitmaps of ceil(n_nodes / 32) words or NULL; d_labels [n_nodes] with d_filters [nq][2] {any, all}, or both NULL.
 * d_scratch: bang_scan_scratch_bytes(nq, k, stripes) bytes, 8-byte aligned.  vec_stride % 4 == 0 holds the vector; layouts as
 * bang_search_can_rerank (others: BANG_ERR_UNSUPPORTED). */
typedef struct {
  const uint8_t* d_vec_base;   /* vector of node x at d_vec_base + x * vec_stride */
  uint64_t vec_stride;
  uint32_t dtype, D, n_nodes;
  const void* d_queries;       /* [nq][D] */
  uint32_t nq, k;
  const uint32_t* d_excluded;
  const uint32_t* d_removed;
  const uint32_t* d_labels;
  const uint32_t* d_filters;
  uint32_t stripes;
  void* d_scratch;
  uint64_t scratch_bytes;
  uint64_t* d_ids_out;         /* [nq][k] */
  float* d_dists_out;          /* [k][nq] */
  uint32_t* d_matched;         /* [nq] */
} bang_scan_params;
int bang_k_scan(const bang_scan_params* p, void* stream);
/* Host side, no HIP call in it (csrc/bang_scan_host.cpp): the grid of a scan -- query tiles and the default number of stripes (BANG_ERR_ARG on a
 * zero or null argument, BANG_ERR_UNSUPPORTED on a layout outside bang_search_can_rerank) --, the largest `stripes` a launch accepts (0 where
 * none), the scratch a launch needs, and bang_k_scan's argument checks on their own */
int bang_scan_geometry(int dtype, uint32_t D, uint32_t nq, uint32_t n_nodes, uint32_t k, uint32_t* tiles, uint32_t* stripes);
uint32_t bang_scan_max_stripes(int dtype, uint32_t n_nodes, uint32_t k);
uint64_t bang_scan_scratch_bytes(uint32_t nq, uint32_t k, uint32_t stripes);
int bang_scan_check(const bang_scan_params* p);
/* dst[w] |= src[w] for w < words, except the bits skip_mask of word skip_word (bang_consolidate_e: the removed set, without the medoid) */
int bang_k_bitmap_or(uint32_t* d_dst, const uint32_t* d_src, uint64_t words, uint64_t skip_word, uint32_t skip_mask, void* stream);

/* REUSE OF REMOVED IDS, device side (csrc/bang_reuse.hip; engine: bang_insert_reuse_e, bang_set_removed_e; DESIGN.md section 2 CANON 24, section
 * 4.18).  Every entry checks its arguments before any HIP call and names the offending one.
 *
 * bang_k_bitmap_select: d_ids_out receives the min(want, total) lowest set bit positions of a & ~not below n_bits (1 .. 2^32 - 2), ascending;
 * *d_total the number of all such bits.  d_not may be NULL; both bitmaps hold ceil(n_bits / 32) words, bits of the last word at or behind n_bits
 * are ignored.  Nothing is written behind d_ids_out[min(want, total)]; want = 0 only counts (d_ids_out may be NULL).  The result is a function
 * of the bitmaps alone (no atomic decides a position).  d_scratch: bang_bitmap_select_scratch_words(n_bits) words, one per span of
 * BANG_SELECT_SPAN_BITS bits (a workgroup's share). */
#define BANG_SELECT_SPAN_BITS 32768u
uint64_t bang_bitmap_select_scratch_words(uint32_t n_bits);
int bang_k_bitmap_select(const uint32_t* d_a, const uint32_t* d_not, uint32_t n_bits, uint32_t want, uint32_t* d_ids_out, uint32_t* d_total,
                         uint32_t* d_scratch, void* stream);
/* bang_k_copy_rows_by_id: `bytes` bytes between row d_ids[i] of a strided table (d_table + id * table_stride + byte_offset) and row i of a packed
 * buffer (d_packed + i * packed_stride), i < n, one wave per row; to_table != 0 writes the table, else the packed buffer.  16-byte pieces where
 * bases, strides and offset are all divisible by 16, dwords where by 4, bytes otherwise (and for what is left of a row).  An id >= n_nodes is
 * skipped, never dereferenced, and *d_abort = 2 (d_abort may be NULL).  On the write side the ids must be distinct. */
int bang_k_copy_rows_by_id(void* d_table, uint64_t table_stride, uint64_t byte_offset, const uint32_t* d_ids, uint32_t n, uint32_t n_nodes,
                           void* d_packed, uint64_t packed_stride, uint32_t bytes, int to_table, uint32_t* d_abort, void* stream);
/* bit d_ids[i] of d_bitmap (ceil(n_bits / 32) words) cleared / set for every i < n, one atomic AND / OR each; an id >= n_bits is skipped */
int bang_k_bitmap_clear_ids(uint32_t* d_bitmap, uint32_t n_bits, const uint32_t* d_ids, uint64_t n, void* stream);
int bang_k_bitmap_set_ids(uint32_t* d_bitmap, uint32_t n_bits, const uint32_t* d_ids, uint64_t n, void* stream);
/* bang_k_rows_check: *d_first (SET TO 0xFFFFFFFF BY THE CALLER) becomes the lowest i < n whose d_ids[i] is >= n_nodes, is `medoid`, or names a
 * node whose degree word (d_graph + id * entry_len + byte_offset) is not 0; it stays 0xFFFFFFFF where there is none. */
int bang_k_rows_check(const uint8_t* d_graph, uint64_t entry_len, uint64_t byte_offset, const uint32_t* d_ids, uint64_t n, uint32_t n_nodes,
                      uint32_t medoid, uint32_t* d_first, void* stream);
/* Host side, no HIP call in it (csrc/bang_reuse_group.cpp).  bang_reuse_assign: the ids of a batch of n points from the n_free eligible free
 * slots (strictly ascending, each < N): f = min(n, n_free), ids_out[i] = free_ids[i] for i < f, N + (i - f) behind; *appended_out = n - f.
 * bang_insert_group_ids: bang_insert_group with explicit source ids -- row i belongs to node ids[i]; ids strictly ascending.  BANG_ERR_ARG (no
 * message) on a null argument, ids that are not strictly ascending (free_ids likewise, or one >= N), row_stride < 2, a degree > R, a listed
 * id >= n_old, or a row that lists an id of the batch. */
int bang_reuse_assign(const uint32_t* free_ids, uint32_t n_free, uint32_t n, uint32_t N, uint32_t* ids_out, uint32_t* appended_out);
int bang_insert_group_ids(const uint32_t* rows, uint32_t n, uint32_t row_stride, const uint32_t* ids, uint32_t n_old, uint32_t* targets,
                          uint32_t* offs, uint32_t* srcs, uint32_t* n_targets);

/* 1 if bang_k_search_exact (engine option "distance" = 1) evaluates vectors of this layout, else 0: float vectors with D % 4 == 0, 8-bit vectors
 * with D % 16 == 0; D <= BANG_EXACT_MAX_D; a graph-entry stride divisible by 4 that holds the vector.  L2 only (no MIPS padding). */
#define BANG_EXACT_MAX_D 1024u
int bang_search_exact_supported(int dtype, uint32_t D, uint64_t entry_len);

#ifdef __cplusplus
}
#endif
#endif /* BANG_C_H_ */
