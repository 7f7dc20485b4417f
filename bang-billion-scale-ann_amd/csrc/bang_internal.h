// bang_internal.h -- declarations shared by the kernel launchers and the host engine (not public).
#ifndef BANG_INTERNAL_H_
#define BANG_INTERNAL_H_

#include <stdint.h>

#include "bang_c.h"

#ifdef __cplusplus
extern "C" {
#endif

// printf-style; stores a thread-local message returned by bang_last_error()
void bang_set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// bang_k_rerank on the sub-range [q0, q0+nq) of a batch of Q_total queries (one lane's share)
int bang_k_rerank_range(const void* d_vec_base, uint64_t vec_stride, const void* d_medoid_vec, const void* d_queries,
                        int dtype, const uint32_t* d_cand_ids, const uint32_t* d_cand_row, const uint32_t* d_cand_cnt,
                        uint32_t cand_stride, uint32_t q0, uint32_t nq, uint32_t Q_total, uint32_t D, uint32_t k,
                        uint32_t dim_adjust, uint64_t* d_ids_out, float* d_dists_out, void* stream);

// the same with the vector log laid out [query][candidate index][vec_stride] (host-paced search kernel with shipped vectors)
int bang_k_rerank_byquery(const void* d_fp, uint64_t vec_stride, const void* d_medoid_vec, const void* d_queries, int dtype,
                          const uint32_t* d_cand_ids, const uint32_t* d_cand_cnt, uint32_t cand_stride, uint32_t q0, uint32_t nq,
                          uint32_t Q_total, uint32_t D, uint32_t k, uint32_t dim_adjust, uint64_t* d_ids_out, float* d_dists_out,
                          void* stream);

// bang_k_rerank_f16 (float queries, fp16 vector table) on the sub-range [q0, q0+nq) of a batch of Q_total queries
int bang_k_rerank_f16_range(const void* d_vec_base, uint64_t vec_stride, const void* d_queries, const uint32_t* d_cand_ids,
                            const uint32_t* d_cand_cnt, uint32_t cand_stride, uint32_t q0, uint32_t nq, uint32_t Q_total, uint32_t D,
                            uint32_t k, uint32_t dim_adjust, uint64_t* d_ids_out, float* d_dists_out, void* stream);

// device side of bang_init: candidate log = [MEDOID], empty worklists, mark = 0x01010101
int bang_k_init_state(uint32_t Q, uint32_t medoid, uint32_t cand_stride, uint32_t* d_cand_ids, uint32_t* d_cand_row,
                      uint32_t* d_cand_cnt, uint32_t* d_wl_cnt, uint32_t* d_mark, uint32_t* d_parents, uint32_t* d_cnt,
                      void* stream);

// padded rows (option rows_pad; bang_pad_rows.hip, layout in bang_pad_rows.h): the staged 256-byte rows d_rows[n_rows][64] go into the padding of
// the code lines of the padded rows [row0, row0 + n_rows) of a table of n_lines lines; m = the chunks the lines are interpreted as (the layout's mp).
// Refused (BANG_ERR_ARG, nothing launched) where the layout is unusable or the last line lies behind the table
int bang_k_pad_rows_scatter(uint8_t* d_codes, uint64_t n_lines, uint32_t code_stride, uint32_t m, const uint32_t* d_rows, uint32_t row0,
                            uint32_t n_rows, void* stream);

#define BANG_ADJ_PAD 0xFFFFFFFFu      /* unused slot of a 256-byte adjacency row (bang_search_params.row_layout = 1) */

// bang_init in one launch: clears the visited filters, resets the per-query state (as bang_k_init_state) and the diagnostic counters
typedef struct {
  uint32_t Q, medoid, cand_stride, n_active;
  uint32_t* d_bloom;                                   /* [Q][BANG_BF_WORDS] */
  uint32_t *d_cand_ids, *d_cand_row, *d_cand_cnt, *d_wl_cnt, *d_mark, *d_parents, *d_cnt;
  uint32_t *d_qstats, *d_qskip, *d_active;   /* may be NULL */
} bang_init_params;
int bang_k_init_all(const bang_init_params* a, void* stream);

// Hand-shake timeouts of the host-paced search kernel are run-time options (host_walk_timeout_ms = 20 000, kernel_go_timeout_ms =
// 30 000: bang_options.cpp).  The HOST gives up first -- it then stores STOP into every pacing word, which ends the kernel at once;
// a pacing group only gives up on its own (the host process is gone) well after that.  Default of a launch without the field set:
#define BANG_KERNEL_GO_TIMEOUT_TICKS 3000000000ull   /* 30 s of the 100 MHz s_memrealtime clock */
#define BANG_RESULT_MAILBOX_BYTES (8 * 1024 * 1024)   // results (ids + distances) up to this size return through the pinned mirror in one copy (BANG_MAILBOX_BYTES)

#define BANG_MAX_LANES 256          /* option "lanes" / BANG_LANES; one abort word per lane sits behind the result mirror */
#define BANG_ERR_STALE_ROWS (-100)  /* internal: a pull-rows file of another graph was found (and removed); the caller rebuilds */

int bang_num_cus(void);
// 1 if the fused kernel has an instance for the exact-size ("ragged") pivot table of this layout
int bang_ragged_supported(uint32_t psz, uint32_t mp, uint32_t nhi, uint32_t m);


#define BANG_WAVE_MAX_LDS (160u * 1024u)   /* LDS of a CU */
// Launch geometry of the wave-resident search kernels (exact-distance, beam, LUT), pure arithmetic: a kernel of `regs` VGPRs whose launch bound is
// max_waves_wg waves and whose waves take wave_bytes of LDS each, Q queries on `cus` CUs; max_wgs / max_waves cap the result (0: no cap).
// BANG_ERR_ARG on a zero or null argument, BANG_ERR_UNSUPPORTED when not one wave fits a CU (no message set: the caller names its kernel)
int bang_wave_geometry(uint32_t regs, uint32_t max_waves_wg, uint32_t wave_bytes, uint32_t cus, uint32_t Q, uint32_t max_wgs, uint32_t max_waves,
                       uint32_t* workgroups, uint32_t* waves);

// The argument checks of an exact-distance launch, made before any HIP call, for bang_k_search_exact, _labels and _beam; every message opens with
// `prefix` ("distance = 1", "distance = 1, beam = 4").  In call order: bang_exact_check_args (R/L, row_layout, buffers, iteration cap, k / result
// rows, rr_vec_f16 > 1), the caller's own rule for rr_vec_f16 = 1, then bang_exact_check_layout (the pulled-rows contract or the graph-entry layout)
__attribute__((visibility("hidden"))) int bang_exact_check_args(const bang_search_params* p, const char* prefix);
__attribute__((visibility("hidden"))) int bang_exact_check_layout(const bang_search_params* p, const char* prefix);

// the instances of the exact-distance search kernel, one entry per build of bang_search_exact.hip; bang_k_search_exact hands them its checked
// arguments.  Graph entries in HBM, the layouts of bang_search_can_rerank (bang_search_exact.o) ...
int bang_k_search_exact_hbm(const bang_search_params* p, void* stream);
// ... and the layouts it refuses (the wide instances, BANG_EXACT_WIDE: bang_search_exact_wide.o); the grid as bang_search_exact_geometry
int bang_k_search_exact_wide(const bang_search_params* p, void* stream);
int bang_search_exact_wide_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
// the pulled-rows instances of both (row_layout 1; the same source built with BANG_EXACT_PULL as bang_search_exact_pull.o / bang_search_exact_wide_pull.o):
// bang_k_search_exact hands them its checked arguments; each geometry reads the register count of the instance it launches
int bang_k_search_exact_pull(const bang_search_params* p, void* stream);
int bang_k_search_exact_wide_pull(const bang_search_params* p, void* stream);
int bang_search_exact_wide_pull_geometry(int dtype, uint32_t L, uint32_t Q, uint32_t max_wgs, uint32_t max_waves, uint32_t* workgroups, uint32_t* waves);
// the pulled-rows instance on an fp16 vector table (rr_vec_f16 = 1; the same source built with BANG_EXACT_PULL and BANG_EXACT_F16 as
// bang_search_exact_pull_f16.o), handed bang_k_search_exact's checked arguments
int bang_k_search_exact_pull_f16(const bang_search_params* p, void* stream);
// the pulled-rows instances of the beam form (bang_search_beam.hip built with BANG_EXACT_PULL as bang_search_beam_pull.o), handed
// bang_k_search_exact_beam's checked arguments
int bang_k_search_exact_beam_pull(const bang_search_params* p, uint32_t beam, void* stream);
// the label-filter instances of the exact-distance search kernel (the same source built with BANG_EXACT_LABELS as bang_search_exact_labels.o and, with
// BANG_EXACT_PULL, bang_search_exact_labels_pull.o), handed bang_k_search_exact_labels' checked arguments
int bang_k_search_exact_labels_hbm(const bang_search_params* p, const bang_label_filter* f, void* stream);
int bang_k_search_exact_labels_pull(const bang_search_params* p, const bang_label_filter* f, void* stream);
// the range-search instances (the same source built with BANG_EXACT_RANGE as bang_search_exact_range.o and, with BANG_EXACT_PULL,
// bang_search_exact_range_pull.o), handed bang_k_search_exact_range's checked arguments
int bang_k_search_exact_range_hbm(const bang_search_params* p, const bang_range_out* r, void* stream);
int bang_k_search_exact_range_pull(const bang_search_params* p, const bang_range_out* r, void* stream);
// BANG_QUERY_FILTER_FILE (bang_cabi.cpp), for the bang.h class alone: applies the file's first num_queries rows as the filters of the batch about to
// run (bang_set_query_filters_e); no-op without the variable.  The file is read once per allocation
int bang_apply_query_filter_file_e(bang_engine_t* e, int num_queries);

// bang_k_scan with a HIP event (hipEvent_t, or NULL) recorded between the scan launch and the merge of the stripes' lists (bang_scan_e's times)
int bang_k_scan_marked(const bang_scan_params* p, void* stream, void* ev_merge);

#ifdef __cplusplus
}
#endif
#endif
