// ccr_plan.h -- the search planner's interface (ccr_plan.hip): the knobs, the plan of one search and the layout of its workspace.
// Host code only: no kernel, no GPU call.  The geometry constants and the layouts the kernels share are in ccr_common.h.
#pragma once
#include "ccr_common.h"
#include "ccr_narrow.h"

namespace ccr {

// Tuning knobs from the environment, read ONCE when an index is created (never inside a search).
struct Knobs {
    int qgroups;       // CCR_QGROUPS      0 = planner's choice, else 1/2/4/8
    int progressive;   // CCR_PROGRESSIVE  0 = single main-pass launch
    int max_phases;    // CCR_PHASES       2 = at most one re-tightening (default 3)
    int mfma16;        // CCR_MFMA16       -1 = planner's choice, 0 = 32x32x16 kernel, 1 = 16x16x32 kernel
    int sample_div;    // CCR_SAMPLE_DIV   0 = planner's choice, else the pinned sample fraction 1/div
    int ranges;        // CCR_RANGES       0 = planner's choice, else the pinned range count (rounded to a multiple of 8)
    int optimistic;    // CCR_OPTIMISTIC   -1 = planner's choice, 0 = conservative thresholds only, 1 = estimated thresholds wherever the sample allows
    int opt_rank;      // CCR_OPT_RANK     0 = planner's choice (optimistic_rank), else the pinned rank (tests: a small rank makes the verification fail)
    int max_lists;     // CCR_MAX_LISTS    0 = planner's limit, else a cap on ranges x sublists (A/B of the select stage's walk)
    int narrow;        // CCR_NARROW       -1 = planner's choice (n_q <= 64 whose rows fit the LDS), 0 = tile kernels only (the A/B knob)
    int narrow_grid;   // CCR_NARROW_GRID  0 = planner's choice, else workgroups of the streaming kernel
    int skip_sampled;  // CCR_SKIP_SAMPLED -1 = planner's choice, 0 = the main pass scores every tile (the A/B knob), 1 = it leaves out the sampled tiles wherever the plan allows
    int skip_list;     // CCR_SKIP_LIST    1 = the select's join reads the threshold kernel's short list of sampled groups (default), 0 = it walks the query's column of group maxima (the A/B knob)
    int qsplit;        // CCR_QSPLIT       -1 = planner's choice, 0 = equal query groups only (the A/B knob), 1 = unequal groups (left-over blocks shared) wherever a single-launch main pass has a block count they apply to; a CCR_QGROUPS that does not divide the block count names their number
    int wide;          // CCR_WIDE         -1 = planner's choice, 0 = 256 x 256 main-pass tiles only (the A/B knob), 1 = 256 x 384 wherever the kernel applies
    int thr_phases;    // CCR_THR_PHASES   0 = launcher's choice by the sample's size, 16 / 64 = the threshold kernel's group phases per query, pinned (tests, the A/B)
    int narrow_groups; // CCR_NARROW_GROUPS 2 = batches of 65 .. 128 queries stream as two query groups (default), 1 = tile kernels above 64 queries (the A/B knob)
    int tile_cap;      // CCR_TILE_CAP     0 = planner's choice (tile_cap_for), else the pinned number of groups one sampled tile may give an estimated threshold; 16 = no cap (the A/B knob)
    int side_cus;      // CCR_SIDE_CUS     -1 = planner's choice (side_cus_for), 0 = the main pass takes every CU (the A/B knob), n = the CUs (rounded to a multiple of 8) a single-launch main pass leaves to side work, pinned; either way only for a search the hint allows (make_plan)
};
// One row per knob -- its variable, its field, its default: the ONE place a default is written.
struct KnobDef {
    const char *env;
    int Knobs::*field;
    int dflt;
};
inline constexpr KnobDef KNOB_DEFS[] = {
    {"CCR_QGROUPS", &Knobs::qgroups, 0},           {"CCR_PROGRESSIVE", &Knobs::progressive, 1},   {"CCR_PHASES", &Knobs::max_phases, 3},
    {"CCR_MFMA16", &Knobs::mfma16, -1},            {"CCR_SAMPLE_DIV", &Knobs::sample_div, 0},     {"CCR_RANGES", &Knobs::ranges, 0},
    {"CCR_OPTIMISTIC", &Knobs::optimistic, -1},    {"CCR_OPT_RANK", &Knobs::opt_rank, 0},         {"CCR_MAX_LISTS", &Knobs::max_lists, 0},
    {"CCR_NARROW", &Knobs::narrow, -1},            {"CCR_NARROW_GRID", &Knobs::narrow_grid, 0},   {"CCR_SKIP_SAMPLED", &Knobs::skip_sampled, -1},
    {"CCR_SKIP_LIST", &Knobs::skip_list, 1},       {"CCR_QSPLIT", &Knobs::qsplit, -1},            {"CCR_WIDE", &Knobs::wide, -1},
    {"CCR_THR_PHASES", &Knobs::thr_phases, 0},     {"CCR_NARROW_GROUPS", &Knobs::narrow_groups, NARROW_MAX_GROUPS},
    {"CCR_TILE_CAP", &Knobs::tile_cap, 0},         {"CCR_SIDE_CUS", &Knobs::side_cus, -1},
};
static_assert(sizeof(KNOB_DEFS) / sizeof(KNOB_DEFS[0]) * sizeof(int) == sizeof(Knobs), "a row for every knob");
inline Knobs default_knobs() {   // what an empty environment gives
    Knobs kn;
    for (const KnobDef &d : KNOB_DEFS) kn.*d.field = d.dflt;
    return kn;
}
Knobs read_knobs();   // default_knobs(), each field overridden by its CCR_* variable

struct Plan {
    int fused;            // 1 = fused MFMA path usable
    int nq_pad;           // n_q rounded up to TILE_Q (256 x 384 main pass: at least main_qblocks * 384)
    int qblocks;          // nq_pad / TILE_Q: the query blocks of the sample pass (and of every 256 x 256 kernel)
    int tile_q;           // queries per tile of the MAIN pass: TILE_Q, or 384 (gemm_topk16w_kernel)
    int main_qblocks;     // query blocks of the main pass: ceil(n_q / tile_q)
    int main_qgroups;     // ... and their groups over the XCDs (divides main_qblocks)
    int main_qsplit;      // 0, or the UNEQUAL groups (2, 4, 8; do not divide main_qblocks) of a single-launch main pass: main_item()
    int64_t tiles;        // ceil(n_rows / TILE_DOCS)
    int64_t full_tiles;   // floor(n_rows / TILE_DOCS)
    int sample_tiles;     // tiles scored by the threshold pass
    int64_t sample_stride;
    int sample_ranges;    // range count of the sample pass (chosen by simulating its item assignment)
    int ranges;           // corpus ranges of the main pass (multiple of NUM_XCD)
    int item_a;           // phase A = work items [0, item_a) of every XCD set (0 = single phase); thresholds are re-tightened after it
    int item_b;           // end of the second phase in items (0: two phases)
    int opt_rank;         // > 0: estimated thresholds = the opt_rank-th largest sampled group maximum (single launch; the select verifies)
    int tile_cap;         // opt_rank > 0: only the tile_cap largest groups of a sampled tile count towards that rank (GROUPS_PER_TILE = no cap)
    int cap_rank;         // opt_rank > 0: the rank the capacities are sized for (opt_rank, or the floor of 40 above a smaller planner's rank)
    int skip_sampled;     // 1: the main pass does not score the sample_tiles sampled tiles again; the select joins their rows from gmax
    int qgroups;          // query-block groups over the XCDs
    int cap;              // candidate slots per sub-list (the largest segment's: statistics)
    CandLayout cand;      // per-phase segments of the candidate area
    int grid;             // persistent workgroups (multiple of NUM_XCD): the sample pass, the retry pass, EPI_STORE, a phased main pass
    int main_grid;        // ... of the single-launch main pass on a tile kernel: grid - side_cus (multiple of NUM_XCD); every main-pass item is priced and mapped on it
    int side_cus;         // CUs that main pass leaves free for side work (ccr_search_stream_wait_main_pass releases the side stream when its workgroups are resident); 0: none
    int rescore_cap;      // max rows re-scored per query (power of two)
    int rescore_regular;  // ... of them recorded candidates (skip_sampled: rescore_cap also holds the joined rows of the sampled tiles)
    int select_compact;   // candidates per query the select kernel gathers into LDS
    int mfma16;           // 1: main pass on the 16x16x32 MFMA kernel
    int sublists;         // candidate sub-lists per (range, query): 4 (32x32x16 kernel) or 8 (16x16x32 kernel)
    // small query batches (n_q <= 64, query rows resident in LDS): the FIRST main pass is the streaming kernel (ccr_narrow.hip) with
    // its own list layout -- one range, two sub-lists per query; the retry pass of flagged queries keeps the tile kernels' layout above
    int narrow;           // 0, or the query tiles of 16 the streaming kernel computes (1, 2, 4)
    int narrow_groups;    // 1, or 2: 65 .. 128 queries as two groups of <= 64, each streamed by half of the workgroups (pairs on one XCD)
    int first_nsub;       // sub-lists per query the first main pass fills (ranges * sublists, or 2) ...
    int first_sp;         // ... per cell (sublists, or 2) ...
    CandLayout first_lay; // ... and where they are (cand, or one segment of narrow capacity)
    int64_t cand_recs;    // 8-byte records of the candidate area
    size_t total;         // bytes of the search workspace (search_ws lays it out)
    int64_t dense_rows_per_chunk;  // queries per dense chunk
};

// Estimated thresholds take the opt_rank-th largest among the groups that are among the tile_cap largest of their own sampled tile:
// tile_cap = ceil(opt_rank / TILE_CAP_TILES), at least TILE_CAP_MIN, so that TILE_CAP_TILES tiles at least set a threshold -- which asks
// for a rank above TILE_CAP_MIN * (TILE_CAP_TILES - 1) (ccr_plan.hip: optimistic_rank, tile_cap_for).
constexpr int TILE_CAP_MIN = 4, TILE_CAP_TILES = 5;
constexpr int OPT_RANK_MIN = TILE_CAP_MIN * (TILE_CAP_TILES - 1) + 1;
// ... which a plan may take when it leaves out the sampled tiles of a sample of REDUCED_RANK_MIN_TILES tiles or more; every other
// estimated plan keeps the earlier floor under its rank (optimistic_rank says why).  Capacities stay sized for the floor's rank.
constexpr int OPT_RANK_FLOOR = 40, REDUCED_RANK_MIN_TILES = 40;

constexpr int FALLBACK_ROWS = 16;   // dense score rows reserved for flagged queries (one on-stream chunk)

// side_hint: the caller ran side work beside the previous search's main pass (ccr_search_stream_wait_main_pass), so this one may
// leave CUs free for it (CCR_SIDE_CUS says how many; without the hint no plan does)
Plan make_plan(int64_t n_rows, int dim, int n_q, int k, int flags, int num_cu, const Knobs &kn, bool side_hint = false);
// The side CUs of the planner's own choice never take more than this share of the grid from the main pass.
constexpr int SIDE_CUS_MAX_DIV = 4;
// the two times that choice compares (ms, the planner's model): a fused tile plan's single-launch main pass, a re-pack of the shard on the whole chip
double side_main_pass_ms(const Plan &p, int dim);
double side_pack_ms(int64_t n_rows, int dim);

// pieces of the planner that the retry pass of a search (ccr_api.hip) lays out its own launch with
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
int pick_qgroups(int qblocks, int dim, const Knobs &kn, int tile_q = TILE_Q);   // equal query-block groups over the XCDs
CandLayout one_segment(int cap);                                                 // candidate layout of one segment over every range

// Workspace layouts: take() places a buffer at the current offset and moves on to the next 256-byte boundary.
struct Bump {
    size_t off;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; }
};

// The workspace of one search, typed: search_ws() is the one description of its layout (with a null base the pointers are byte
// offsets; the planner takes `total` from there).  A dense plan has the flag area and the dense scratch only.
struct SearchWs {
    float *qnorm, *thr, *cq, *gmax;     // thr, cq (margin coefficients gamma ||q||): [nq_pad] each, cq right after thr
    uint32_t *cnt;                      // sub-list counters
    uint2 *cand;                        // candidate area (cand_bytes): free once the select stage has run
    uint32_t *flag_count, *flag_list;   // flag area: flag count at +0, candidate count (stat_cand) at +8, main-pass arrivals at +16, flagged queries at +64
    uint32_t *arrive;                   // workgroups of a main pass with side CUs that have started (cleared with the flag count)
    unsigned long long *stat_cand;
    uint32_t *top;                      // the k best lower bounds per query between two re-tightenings (three-phase plans)
    float *thr_safe, *cq_safe, *dense;  // estimated thresholds: the conservative bounds of a failing search; dense scratch (dense_bytes)
    uint32_t *glist;                    // skip_sampled: [nq_pad][skip_list_cap(opt_rank) + 1] short lists of sampled groups for the select's join
    // retry area (retry_bytes from Q2 on): compact query rows, their thresholds and margin coefficients, the retry and dense
    // lists, two partition counts, a second flag area, and the two lists the rounds of a group alternate on
    uint16_t *Q2;
    float *thr2, *cq2;
    uint32_t *retry_list, *dense_list, *counts, *flag2, *list_b, *list_c;
    size_t cand_bytes, dense_bytes, retry_bytes, total;
};
SearchWs search_ws(const Plan &p, int64_t n_rows, int dim, int n_q, int k, char *base);
// entries of a query's short list: about opt_rank groups reach tau (it IS the opt_rank-th largest lower bound), a few more inside the margin
inline int skip_list_cap(int opt_rank) { return 2 * opt_rank + 30; }

}  // namespace ccr
