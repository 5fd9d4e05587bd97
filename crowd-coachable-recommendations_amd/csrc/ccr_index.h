// ccr_index.h -- the index object and the launchers shared by the host-side translation units
// (ccr_api.hip: ccr_search; ccr_special.hip: blocked / sparse-prior searches).  The planner's interface is ccr_plan.h.
#pragma once
#include "ccr_common.h"
#include "ccr_plan.h"

namespace ccr {

// kernels implemented in the other translation units
// the fused GEMM + top-k kernels (ccr_main_pass.hip): 256 x 256 tiles on the 32x32x16 MFMA (every epi) or the 16x16x32 MFMA (no EPI_GMAX), or
// 256 x 384 tiles on the 16x16x32 MFMA (MAIN_WIDE: a.qblocks = blocks of 384 queries, EPI_FILTER and dim % 32 == 0 only)
enum MainKernel { MAIN_32X32, MAIN_16X16, MAIN_WIDE };
int launch_gemm(const GemmArgs &a, int dt, MainKernel kind, int epi, int grid, hipStream_t s);   // dt: element type of a.D and a.Q (CCR_DTYPE_BF16 / _F16), here and below
// one wave on `s` that returns when `want` workgroups have counted themselves in at `arrive` (GemmArgs::arrive), or when its bounds run out
int launch_main_pass_gate(const uint32_t *arrive, uint32_t want, hipStream_t s);
int launch_shard_header(const ccr_shard_header &h, void *message, hipStream_t s);   // ccr_merge.hip: the 32-byte header, by value
int ensure_dynamic_lds(const void *kernel, size_t lds);   // ccr_api.hip: per (kernel, device) opt-in to > 64 KiB of dynamic LDS
// the norm bounds (ccr_threshold.hip).  tile_bits (optional): bit patterns of the largest row norm of every 256-row tile, max-accumulated (zeroed by the caller)
int launch_row_norms(const uint16_t *X, int dt, int64_t rows, int dim, float *norms, uint32_t *max_bits, uint32_t *tile_bits,
                     hipStream_t s);
int launch_tile_norms(const float *row_bounds, int64_t rows, uint32_t *tile_bits, uint32_t *max_bits, hipStream_t s);
// The stages of a fused search (ccr_search), each in the source file of its name; no [Q, N] score matrix ever exists in HBM:
//   sample pass  (launch_gemm, EPI_GMAX)  : score every `stride`-th 256-row corpus tile, reduce each 16-row MFMA
//                              fragment to its maximum -> gmax[group][query]
//   threshold    (launch_threshold): tau_q = k-th largest group maximum (a lower bound of the k-th
//                              largest score: k disjoint groups hold a score >= tau_q), minus the
//                              MFMA error margins (cq * tile norm)
//   main pass    (launch_gemm, EPI_FILTER): score the whole shard; accumulators >= thr_q are appended to the
//                              (range, query) candidate list (LDS counter, 8-byte records); between two of its phases
//                              launch_threshold_update re-tightens thr from the candidates found so far
//   select       (launch_select_rescore): per query radix-select the k-th largest MFMA score among
//                              the candidates, keep everything whose error interval reaches it, re-score those
//                              canonically (fp64 ordered) and sort by (score desc, id asc).
// The three stage launchers take an argument struct; an optional field that is left at its initialiser is switched off.

// thr[q] = tau_q (lower bound of the k-th largest exact score), cq[q] = gamma ||q|| (margin per unit of row norm)
struct ThresholdArgs {
    const float *gmax;        // the sample pass's group maxima [n_groups][nq_pad]
    int64_t n_groups, sample_stride;
    int n_q, nq_pad, dim;
    int k;                    // the rank of the group maximum that becomes tau_q
    int tile_cap = GROUPS_PER_TILE;   // ... among the groups that are among the tile_cap largest of their own sampled tile (16 = among all)
    const float *qnorm, *tile_norm;
    const uint32_t *dmax_bits;
    float *thr, *cq;
    uint32_t *zero_cnt = nullptr; int zero_per_query = 0;   // n_q x zero_per_query counters to clear on the way
    uint32_t *glist = nullptr; int list_cap = 0;   // [nq_pad][list_cap + 1]: per query {count, groups whose upper bound reaches tau}
    int phases = 0;                 // 0 = by the sample's size, 16 / 64 = pinned
};
int launch_threshold(const ThresholdArgs &a, hipStream_t s, int *phases_used = nullptr);   // *phases_used: 16 / 64, 0 = the small-batch kernel

// nsub: sub-lists of the fully scored ranges; queries whose block position inside its XCD group is < part_blocks have nsub_part.
// prev_*: the same at the previous re-tightening of this search (top_in: its k best lower bounds per query are in `top` and only
// the sub-lists completed since are read); top_out: leave the k best for the next one.
struct ThresholdUpdateArgs {
    const uint2 *cand;
    const uint32_t *cnt;
    CandLayout lay;
    int sp;                   // sub-lists per (range, query)
    int n_q, nq_pad, k, nsub;
    const float *cq, *tile_norm;
    float *thr;
    // the progressive main pass
    int nsub_part = 0, part_blocks = 0, prev_nsub = 0, prev_part = 0, prev_blocks = 0;
    int qb_per = 1;           // query blocks per XCD group
    uint32_t *top = nullptr;  // [nq_pad + n_q * k] u32 or null
    bool top_in = false, top_out = false;
    int tile_q = TILE_Q;      // queries per block of the main pass that filled the lists (a query's block position decides which ranges it has seen)
};
int launch_threshold_update(const ThresholdUpdateArgs &a, hipStream_t s);

int select_compact_entries(int dim, int ranges, int rescore_cap, int64_t want);
struct SelectArgs {
    // the candidate lists
    const uint2 *cand;
    const uint32_t *cnt;
    CandLayout lay;
    int ranges, sp, n_q, nq_pad;
    // the limits
    int k, rescore_cap, compact;
    int regular_cap;          // limit of the recorded rows (0: rescore_cap)
    // the index view
    const uint16_t *D;
    int dt, dim;
    int64_t n_rows, id_offset;
    const float *tile_norm, *row_norm;
    const uint32_t *dmax_bits;
    // the queries and their bounds.  thr (device, [n_q]): the thresholds the main pass filtered with.  The select VERIFIES them -- the
    // k-th largest lower bound L of the candidates must reach thr[q], else rows below an over-estimated threshold may be missing: the
    // query is flagged for the retry pass and thr[q] is replaced by L (a valid bound); with fewer than k candidates thr[q] = -inf and
    // the dense path.
    const uint16_t *Q;
    float *thr;
    const float *cq;
    // the outputs
    float *out_scores;
    int64_t *out_ids;
    const uint32_t *out_rows = nullptr;   // destination row of every query (null: its own)
    // the flag area
    uint32_t *flag_count, *flag_list;
    unsigned long long *stat_cand = nullptr;   // the search's candidate count (null: not kept)
    // the join.  gmax (device, null: no join): the sample pass's group maxima [sample_tiles * 16][gmax_pitch] of a search whose main
    // pass left out the sampled tiles j * sample_stride -- every group that can reach L joins the re-scored rows (the first select of
    // such a search only).  glist / list_cap (may be null): launch_threshold's short lists of the groups to test; without one the
    // query's column of gmax is walked.
    const float *gmax = nullptr; int sample_tiles = 0, sample_stride = 0, gmax_pitch = 0;
    const uint32_t *glist = nullptr; int list_cap = 0;
};
int launch_select_rescore(const SelectArgs &a, hipStream_t s);
int launch_partition_flags(const uint32_t *flags, int begin, int n, uint32_t *retry_list, uint32_t *dense_list, uint32_t *counts,
                           hipStream_t s);
int launch_underfilled_to_retry(uint32_t *flags, int begin, int n, const float *thr_safe, float *thr, hipStream_t s);
int launch_scatter_thresholds(const uint32_t *list, int n, const float *thr2, float *thr, hipStream_t s);
int launch_gather_queries(const uint16_t *Q, int dim, const uint32_t *list, int n, const float *thr, const float *cq, uint16_t *Q2,
                          float *thr2, float *cq2, hipStream_t s);
// dense exact path.  qlist: query rows to score (nullptr: q_begin + qi); out_rows: destination rows of the select
// (nullptr: q_begin + qi); count_dev (device, may be null): only the first *count_dev - q_begin entries of the list exist
// (the on-stream fallback chunk of an asynchronous search -- the host does not know the count yet).
int launch_dense_scores(const uint16_t *D, int dt, int64_t n_rows, int dim, const uint16_t *Q, const uint32_t *qlist,
                        int q_begin, int nq_chunk, const uint32_t *count_dev, float *out, hipStream_t s);
int launch_dense_select(const float *scores, int64_t n_rows, int k, const uint32_t *out_rows, int q_begin, int nq_chunk,
                        const uint32_t *count_dev, int64_t id_offset, float *out_scores, int64_t *out_ids, hipStream_t s,
                        bool aggregate = true, const uint32_t *in_rows = nullptr, bool in_rows_compact = false);
// in_rows: block b ranks the score row in_rows[b] (in_rows_compact: score row b) and writes output row q_begin + in_rows[b]; with count_dev
// only the first *count_dev blocks

// Exact top-k from MFMA score rows [nq_chunk][pitch] + error margins (ccr_dense.hip); the chunk's query rows are contiguous at Q.
// hint (per chunk query, or null): a valid lower bound of its k-th largest score -- one scan of the row instead of five.
// Queries it cannot finish (more than 8 192 rows inside the margin, non-finite margins) are appended to flag_list with FLAG_DENSE.
int launch_margin_select(const float *scores, int64_t pitch, int64_t n_rows, int k, int dim, const uint16_t *Q, const uint16_t *D, int dt,
                         const float *tile_norm, const float *row_norm, const uint32_t *dmax_bits, const float *hint, const uint32_t *out_rows,
                         int q_begin, int nq_chunk, int64_t id_offset, float *out_scores, int64_t *out_ids, uint32_t *flag_count, uint32_t *flag_list,
                         hipStream_t s);

// Events of a search at its phase boundaries.  EV_MAIN_END: what ccr_search_stream_wait_main_pass orders against (EV_MAIN_BEGIN and
// the gate kernel when the main pass left side CUs); EV_DONE: the
// flagged queries re-done (or the dense path finished); EV_ASYNC_END: an asynchronous search's flag line copied to the host.
enum SearchEvent { EV_BEGIN, EV_SAMPLE_BEGIN, EV_SAMPLE_END, EV_MAIN_BEGIN, EV_MAIN_END, EV_SELECT_END, EV_DONE, EV_ASYNC_END, EV_COUNT };

}  // namespace ccr

struct ccr_index {
    const uint16_t *D;
    int dtype;            // CCR_DTYPE_BF16 or CCR_DTYPE_F16: the element type of D and of every query matrix searched against it
    int64_t n_rows;
    int dim;
    int64_t offset;
    int64_t id_out;       // what the running search writes as ids: `offset` (int64 global ids) or ID_LOCAL_U32 (u32 local rows of a shard message)
    uint32_t *dmax_bits;  // device: bits of the max row norm (a slot of the per-device slab)
    float *tile_norm;     // device [ceil(n_rows / 256)]: bound of the row norms of each 256-row tile (per-device block cache)
    size_t tile_bytes;
    const float *row_norm;   // device [n_rows]: norm bound of every row -- the caller's array (borrowed) or the index's own pass
    float *row_norm_own;     // the latter (per-device block cache), else null
    size_t row_bytes;
    bool have_events;
    int thr_phases_used;       // group phases of the last search's threshold kernel (16 / 64; 0: the small-batch kernel, or no fused search yet)
    bool main_pass_recorded;   // EV_MAIN_END was recorded by the last search (fused path): ccr_search_stream_wait_main_pass has something to wait for
    int num_cu;
    int device;
    ccr::Knobs knobs;
    hipEvent_t ev[ccr::EV_COUNT];
    volatile uint32_t *host_flags;   // pinned host line {flag count, -, candidate count (8 B)} of the per-device slab
    ccr::Plan plan;       // plan of the last search and its key (the planner simulates item assignments: ~25 us)
    int plan_nq, plan_k, plan_flags;
    bool plan_side_hint;
    const uint32_t *side_arrive;   // the last fused search's arrival counter in its workspace (the gate of ccr_search_stream_wait_main_pass polls it)
    ccr_search_stats stats;
    // an asynchronous search (CCR_SEARCH_ASYNC) that ccr_search_finish has not completed yet
    struct {
        bool active;
        const uint16_t *Q;
        int n_q, k;
        float *out_scores;
        int64_t *out_ids;
        char *ws;
        hipStream_t stream;
    } pending;
};
