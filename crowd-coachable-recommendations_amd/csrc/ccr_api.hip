// ccr_api.hip -- host side of the C ABI: index object, ccr_search orchestration (the planner: ccr_plan.hip).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "ccr_index.h"
#include "ccr_narrow.h"
#include "ccr_topk_device.h"

namespace ccr {

// ------------------------------------------------------------------ error text (thread-local)
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace ccr

using namespace ccr;

// Per-device slab of 256-byte slots for the indices' small device state: building an index per active-learning
// step must not cost a hipMalloc / hipFree pair (hipFree synchronises the device).
namespace {
constexpr int SLAB_SLOTS = 1024, SLAB_SLOT_BYTES = 256, MAX_DEVICES = 64;
struct Slab {
    char *base = nullptr;
    char *host = nullptr;   // pinned host twin (one 64-byte line per slot): where an asynchronous search leaves its flag count
    std::vector<int> free_slots;
};
constexpr int SLAB_HOST_BYTES = 64;
std::mutex g_slab_mutex;
Slab g_slabs[MAX_DEVICES];

int slab_take(int device, uint32_t **out, volatile uint32_t **host_out) {
    std::lock_guard<std::mutex> lock(g_slab_mutex);
    CCR_REQUIRE(device >= 0 && device < MAX_DEVICES, "device ordinal %d out of range", device);
    Slab &sl = g_slabs[device];
    if (!sl.base) {
        CCR_HIP_CHECK(hipMalloc((void **)&sl.base, (size_t)SLAB_SLOTS * SLAB_SLOT_BYTES));
        if (hipHostMalloc((void **)&sl.host, (size_t)SLAB_SLOTS * SLAB_HOST_BYTES, hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(sl.base);
            sl.base = nullptr;
            set_error("ccr_index_create: hipHostMalloc of the pinned flag lines failed");
            return CCR_ERR_HIP;
        }
        for (int i = SLAB_SLOTS - 1; i >= 0; --i) sl.free_slots.push_back(i);
    }
    if (sl.free_slots.empty()) {
        set_error("ccr_index_create: more than %d live indices on device %d", SLAB_SLOTS, device);
        return CCR_ERR_INVALID;
    }
    *out = reinterpret_cast<uint32_t *>(sl.base + (size_t)sl.free_slots.back() * SLAB_SLOT_BYTES);
    *host_out = reinterpret_cast<volatile uint32_t *>(sl.host + (size_t)sl.free_slots.back() * SLAB_HOST_BYTES);
    sl.free_slots.pop_back();
    return CCR_OK;
}

void slab_give(int device, uint32_t *p) {
    if (!p || device < 0 || device >= MAX_DEVICES) return;
    std::lock_guard<std::mutex> lock(g_slab_mutex);
    Slab &sl = g_slabs[device];
    sl.free_slots.push_back((int)((reinterpret_cast<char *>(p) - sl.base) / SLAB_SLOT_BYTES));
}
}  // namespace

extern "C" const char *ccr_last_error(void) { return g_err; }
extern "C" int ccr_version(void) { return 114; }

// The hint behind side CUs, per device: did the caller order a side stream against the main pass of the previous fused search
// (ccr_search_stream_wait_main_pass)?  Then the next fused search on the device may leave CUs free for that side work; it takes the
// hint with it, so a search that is not followed by the call switches the carve off again and the first search of a loop never has it.
namespace {
bool g_side_hint[MAX_DEVICES];
bool side_hint_take(int device) {
    std::lock_guard<std::mutex> lock(g_slab_mutex);
    const bool hint = g_side_hint[device];
    g_side_hint[device] = false;
    return hint;
}
void side_hint_set(int device) {
    std::lock_guard<std::mutex> lock(g_slab_mutex);
    g_side_hint[device] = true;
}
}  // namespace

extern "C" int ccr_index_destroy(ccr_index *ix);

// Per-device cache of the indices' tile-norm arrays (4 B per 256 corpus rows): an index built per step gets the block the
// previous one gave back instead of a hipMalloc / hipFree pair.
namespace {
struct CachedBlock {
    void *p;
    size_t bytes;
};
std::vector<CachedBlock> g_blocks[MAX_DEVICES];
constexpr size_t BLOCK_CACHE_ENTRIES = 8;

int block_take(int device, size_t bytes, void **out, size_t *got) {
    CCR_REQUIRE(device >= 0 && device < MAX_DEVICES, "device ordinal %d out of range", device);
    bytes = (bytes + 4095) / 4096 * 4096;
    {
        std::lock_guard<std::mutex> lock(g_slab_mutex);
        auto &v = g_blocks[device];
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].bytes >= bytes && v[i].bytes <= 2 * bytes) {
                *out = v[i].p;
                *got = v[i].bytes;
                v.erase(v.begin() + i);
                return CCR_OK;
            }
    }
    CCR_HIP_CHECK(hipMalloc(out, bytes));
    *got = bytes;
    return CCR_OK;
}

void block_give(int device, void *p, size_t bytes) {
    if (!p) return;
    void *drop = nullptr;
    if (device >= 0 && device < MAX_DEVICES && bytes <= ((size_t)64 << 20)) {   // larger blocks are not worth pinning
        std::lock_guard<std::mutex> lock(g_slab_mutex);
        auto &v = g_blocks[device];
        v.push_back({p, bytes});
        if (v.size() > BLOCK_CACHE_ENTRIES) {   // oldest out
            drop = v.front().p;
            v.erase(v.begin());
        }
    } else {
        drop = p;
    }
    if (drop) (void)hipFree(drop);
}
}  // namespace

// The dynamic-LDS opt-in (> 64 KiB) is a per-device function attribute: it is set the first time a kernel is launched
// on a device and remembered per (kernel, device) -- not on every launch.
int ccr::ensure_dynamic_lds(const void *kernel, size_t lds) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    CCR_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({kernel, dev})) return CCR_OK;
    CCR_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    done.insert({kernel, dev});
    return CCR_OK;
}

// row_bounds (device, n_rows floats, or null): upper bounds of the packed rows' norms as ccr_pack_bf16_ex wrote them (borrowed for
// the life of the index: the select stage reads them per candidate); without them the index makes its own pass over the shard.
static int index_create_impl(const uint16_t *D_bf16, int half_dtype, int64_t n_rows, int dim, int64_t global_row_offset, const float *row_bounds,
                             void *stream, ccr_index **out) {
    CCR_REQUIRE(D_bf16 && out, "ccr_index_create: null pointer");
    if (const int rc = check_half("ccr_index_create", half_dtype)) return rc;
    CCR_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 32), "ccr_index_create: n_rows=%lld out of range [1, 2^32)",
                (long long)n_rows);
    CCR_REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= 4096, "ccr_index_create: dim=%d must be a multiple of 8 in [8, 4096]", dim);
    CCR_REQUIRE((uintptr_t)D_bf16 % 16 == 0, "ccr_index_create: corpus pointer must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ccr_index *ix = new ccr_index();
    memset(ix, 0, sizeof(*ix));
    ix->D = D_bf16;
    ix->dtype = half_dtype;
    ix->n_rows = n_rows;
    ix->dim = dim;
    ix->offset = ix->id_out = global_row_offset;
    ix->knobs = read_knobs();
    // on any failure below the partially built index is released before returning
    auto build = [&]() -> int {
        CCR_HIP_CHECK(hipGetDevice(&ix->device));
        CCR_HIP_CHECK(hipDeviceGetAttribute(&ix->num_cu, hipDeviceAttributeMultiprocessorCount, ix->device));
        int rc = slab_take(ix->device, &ix->dmax_bits, &ix->host_flags);
        if (rc != CCR_OK) return rc;
        const int64_t tiles = (n_rows + TILE_DOCS - 1) / TILE_DOCS;
        void *tn = nullptr;
        rc = block_take(ix->device, (size_t)tiles * 4, &tn, &ix->tile_bytes);
        if (rc != CCR_OK) return rc;
        ix->tile_norm = (float *)tn;
        uint32_t *tile_bits = reinterpret_cast<uint32_t *>(ix->tile_norm);   // non-negative floats: bit patterns order as unsigned
        if (row_bounds) {   // no pass over the shard, no synchronisation (max_tile_norm_kernel WRITES the maximum: no memset)
            ix->row_norm = row_bounds;
            rc = launch_tile_norms(row_bounds, n_rows, tile_bits, ix->dmax_bits, s);
            if (rc != CCR_OK) return rc;
        } else {
            void *rn = nullptr;
            rc = block_take(ix->device, (size_t)n_rows * 4, &rn, &ix->row_bytes);
            if (rc != CCR_OK) return rc;
            ix->row_norm = ix->row_norm_own = (float *)rn;
            CCR_HIP_CHECK(hipMemsetAsync(ix->dmax_bits, 0, 4, s));   // (this path max-accumulates with atomics)
            CCR_HIP_CHECK(hipMemsetAsync(tile_bits, 0, (size_t)tiles * 4, s));
            rc = launch_row_norms(D_bf16, half_dtype, n_rows, dim, ix->row_norm_own, ix->dmax_bits, tile_bits, s);
            if (rc != CCR_OK) return rc;
            CCR_HIP_CHECK(hipStreamSynchronize(s));
        }
        return CCR_OK;
    };
    const int rc = build();
    if (rc != CCR_OK) {
        ccr_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return CCR_OK;
}

extern "C" int ccr_index_create_half(const uint16_t *D, int64_t n_rows, int dim, int half_dtype, int64_t global_row_offset, void *stream,
                                     ccr_index **out) {
    return index_create_impl(D, half_dtype, n_rows, dim, global_row_offset, nullptr, stream, out);
}

extern "C" int ccr_index_create_with_norms_half(const uint16_t *D, int64_t n_rows, int dim, int half_dtype, int64_t global_row_offset,
                                                const float *row_norm_bounds, void *stream, ccr_index **out) {
    CCR_REQUIRE(row_norm_bounds, "ccr_index_create_with_norms: null row_norm_bounds");
    return index_create_impl(D, half_dtype, n_rows, dim, global_row_offset, row_norm_bounds, stream, out);
}

extern "C" int ccr_index_create(const uint16_t *D_bf16, int64_t n_rows, int dim, int64_t global_row_offset, void *stream,
                                ccr_index **out) {
    return ccr_index_create_half(D_bf16, n_rows, dim, CCR_DTYPE_BF16, global_row_offset, stream, out);
}

extern "C" int ccr_index_create_with_norms(const uint16_t *D_bf16, int64_t n_rows, int dim, int64_t global_row_offset,
                                           const float *row_norm_bounds, void *stream, ccr_index **out) {
    return ccr_index_create_with_norms_half(D_bf16, n_rows, dim, CCR_DTYPE_BF16, global_row_offset, row_norm_bounds, stream, out);
}

extern "C" int ccr_index_destroy(ccr_index *ix) {
    if (!ix) return CCR_OK;
    // an asynchronous search the caller never finished: its kernels still read the index's arrays -- wait for THAT search (not
    // for the stream) before the blocks go back to the cache; queries it flagged beyond the on-stream chunk stay un-redone
    if (ix->pending.active && ix->have_events) (void)hipEventSynchronize(ix->ev[EV_ASYNC_END]);
    ix->pending.active = false;
    // a slot / block handed back may be rewritten by the next index's create on ITS stream; the caller destroys an index only
    // after the work that uses it has completed (the same contract as for the borrowed corpus)
    slab_give(ix->device, ix->dmax_bits);
    block_give(ix->device, ix->tile_norm, ix->tile_bytes);
    block_give(ix->device, ix->row_norm_own, ix->row_bytes);
    if (ix->have_events)
        for (int i = 0; i < EV_COUNT; ++i)
            if (ix->ev[i]) (void)hipEventDestroy(ix->ev[i]);
    delete ix;
    return CCR_OK;
}

extern "C" int64_t ccr_index_rows(const ccr_index *ix) { return ix ? ix->n_rows : -1; }
extern "C" int ccr_index_dim(const ccr_index *ix) { return ix ? ix->dim : -1; }
extern "C" int ccr_index_dtype(const ccr_index *ix) { return ix ? ix->dtype : -1; }

extern "C" size_t ccr_search_workspace_bytes(const ccr_index *ix, int n_q, int k) {
    if (!ix || n_q <= 0 || k <= 0) return 0;
    // the largest of the plans, so that flags may be chosen at call time and the fused plans may or may not leave side CUs
    size_t total = make_plan(ix->n_rows, ix->dim, n_q, k, CCR_SEARCH_FORCE_DENSE, ix->num_cu, ix->knobs).total;
    for (int flags : {CCR_SEARCH_DEFAULT, CCR_SEARCH_FORCE_FUSED})
        for (bool side_hint : {false, true}) total = std::max(total, make_plan(ix->n_rows, ix->dim, n_q, k, flags, ix->num_cu, ix->knobs, side_hint).total);
    return total + 256;
}

extern "C" int ccr_search_stream_wait_main_pass(const ccr_index *ix, void *stream) {
    CCR_REQUIRE(ix, "ccr_search_stream_wait_main_pass: null index");
    if (!ix->main_pass_recorded) return CCR_OK;   // dense path / no search yet: nothing to order against
    side_hint_set(ix->device);
    if (ix->plan.side_cus == 0) {
        CCR_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, ix->ev[EV_MAIN_END], 0));
        return CCR_OK;
    }
    // the main pass left CUs free: the stream goes on when that pass BEGINS -- behind a gate that lets its workgroups take their
    // CUs first (a workgroup of the main pass needs a whole empty CU and would starve behind a flood of short side workgroups)
    CCR_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, ix->ev[EV_MAIN_BEGIN], 0));
    return launch_main_pass_gate(ix->side_arrive, (uint32_t)ix->plan.main_grid, (hipStream_t)stream);
}

extern "C" int ccr_search_last_stats(const ccr_index *ix, ccr_search_stats *stats) {
    CCR_REQUIRE(ix && stats, "ccr_search_last_stats: null pointer");
    CCR_REQUIRE(!ix->pending.active, "ccr_search_last_stats: an asynchronous search is pending (call ccr_search_finish first)");
    *stats = ix->stats;
    return CCR_OK;
}

extern "C" int ccr_search_last_main_split(const ccr_index *ix) {
    if (!ix || ix->plan_nq <= 0 || !ix->plan.fused) return 0;   // no search yet / dense path
    return ix->plan.main_qsplit;
}

extern "C" int ccr_search_last_threshold_phases(const ccr_index *ix) {
    if (!ix || ix->plan_nq <= 0 || !ix->plan.fused) return 0;   // no search yet / dense path
    return ix->thr_phases_used;
}

// Exact dense path for n queries: the rows d_qlist[0 .. n) (or 0 .. n when d_qlist is null), results to the same rows of the outputs.
static int dense_for_list(const ccr_index *ix, const uint16_t *Q, const uint32_t *d_qlist, int n, int k, float *scratch, int64_t rows_per_chunk,
                          float *out_scores, int64_t *out_ids, hipStream_t s) {
    for (int lo = 0; lo < n; lo += (int)rows_per_chunk) {
        const int m = std::min<int64_t>(rows_per_chunk, n - lo);
        int rc = launch_dense_scores(ix->D, ix->dtype, ix->n_rows, ix->dim, Q, d_qlist ? d_qlist + lo : nullptr, lo, m, nullptr, scratch, s);
        if (rc != CCR_OK) return rc;
        rc = launch_dense_select(scratch, ix->n_rows, k, d_qlist ? d_qlist + lo : nullptr, lo, m, nullptr, ix->id_out, out_scores, out_ids, s);
        if (rc != CCR_OK) return rc;
    }
    return CCR_OK;
}

static bool margin_path_ok(const ccr_index *ix, int k) { return ix->dim % 8 == 0 && k <= MAX_K; }
static int64_t tiles_of(const ccr_index *ix) { return (ix->n_rows + TILE_DOCS - 1) / TILE_DOCS; }

// kernel arguments of n_q query rows at Q (nq_pad / TILE_Q blocks) against the index's corpus, all work items
static GemmArgs gemm_args(const ccr_index *ix, const uint16_t *Q, int n_q, int nq_pad) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.D = ix->D;
    g.n_rows = ix->n_rows;
    g.dim = ix->dim;
    g.Q = Q;
    g.n_q = n_q;
    g.nq_pad = nq_pad;
    g.qblocks = nq_pad / TILE_Q;
    g.item_end = INT32_MAX;
    return g;
}

// EPI_FILTER arguments: every corpus tile in the plan's ranges, candidates to the workspace's lists as `lay` places them
static GemmArgs filter_args(const ccr_index *ix, const Plan &p, const SearchWs &w, const uint16_t *Q, int n_q, int nq_pad, int qblocks,
                            int qgroups, const float *thr, const float *cq, const CandLayout &lay) {
    GemmArgs g = gemm_args(ix, Q, n_q, nq_pad);
    g.qblocks = qblocks;
    g.qgroups = qgroups;
    g.n_vt = p.tiles;
    g.tile_stride = 1;
    g.ranges = p.ranges;
    g.thr = thr;
    g.cq = cq;
    g.tile_norm = ix->tile_norm;
    g.cnt = w.cnt;
    g.cand = w.cand;
    g.lay = lay;
    return g;
}

// Arguments of the stage launchers for the search in ix->plan and ix->pending, whole batch: what follows from the index, the plan and
// the workspace, a line per group of the struct.  A call site sets what is particular to it.
// thresholds of rank k from the sample's group maxima, to w.thr / w.cq
static ThresholdArgs threshold_args(const ccr_index *ix, const SearchWs &w) {
    const Plan &p = ix->plan;
    ThresholdArgs t{};
    t.gmax = w.gmax, t.n_groups = (int64_t)p.sample_tiles * GROUPS_PER_TILE, t.sample_stride = p.sample_stride;
    t.n_q = ix->pending.n_q, t.nq_pad = p.nq_pad, t.k = ix->pending.k, t.qnorm = w.qnorm;
    t.dmax_bits = ix->dmax_bits, t.dim = ix->dim, t.tile_norm = ix->tile_norm;
    t.thr = w.thr, t.cq = w.cq, t.phases = ix->knobs.thr_phases;
    return t;
}

// w.thr re-tightened from candidate lists of the main pass's sub-list count; the call site says which lists (nsub, lay)
static ThresholdUpdateArgs update_args(const ccr_index *ix, const SearchWs &w) {
    ThresholdUpdateArgs u{};
    u.cand = w.cand, u.cnt = w.cnt, u.sp = ix->plan.sublists;
    u.n_q = ix->pending.n_q, u.nq_pad = ix->plan.nq_pad, u.k = ix->pending.k;
    u.cq = w.cq, u.tile_norm = ix->tile_norm, u.thr = w.thr;
    return u;
}

// the select of the batch's own query rows and bounds, to its outputs; the call site says which lists (ranges, sp, lay) and where the flags go
static SelectArgs select_args(const ccr_index *ix, const SearchWs &w) {
    const Plan &p = ix->plan;
    const auto &pd = ix->pending;
    SelectArgs a{};
    a.cand = w.cand, a.cnt = w.cnt, a.n_q = pd.n_q, a.nq_pad = p.nq_pad;
    a.k = pd.k, a.rescore_cap = p.rescore_cap, a.regular_cap = p.rescore_regular, a.compact = p.select_compact;
    a.D = ix->D, a.dt = ix->dtype, a.dim = ix->dim, a.n_rows = ix->n_rows;
    a.tile_norm = ix->tile_norm, a.row_norm = ix->row_norm, a.dmax_bits = ix->dmax_bits, a.id_offset = ix->id_out;
    a.Q = pd.Q, a.thr = w.thr, a.cq = w.cq;
    a.out_scores = pd.out_scores, a.out_ids = pd.out_ids;
    return a;
}

// EPI_STORE: MFMA score rows of the n_q queries at Q against every corpus row, in `ranges` ranges, to out [n_q][pitch] (0: n_rows)
static int store_scores(const ccr_index *ix, const uint16_t *Q, int n_q, int ranges, float *out, int64_t pitch, hipStream_t s) {
    GemmArgs g = gemm_args(ix, Q, n_q, (int)round_up(n_q, TILE_Q));
    g.n_vt = tiles_of(ix);
    g.tile_stride = 1;
    g.ranges = ranges;
    g.qgroups = 1;
    g.store = out;
    g.store_pitch = pitch;
    return launch_gemm(g, ix->dtype, ix->knobs.mfma16 != 0 ? MAIN_16X16 : MAIN_32X32, EPI_STORE, std::max(NUM_XCD, ix->num_cu / NUM_XCD * NUM_XCD), s);
}

// The same for inner-product scores the fast way: MFMA score rows of the chunk (EPI_STORE of the fused kernel) + margin select
// (ccr_dense.hip).  Queries are the rows Qc[0 .. n) -- contiguous: the caller gathers a list first -- results go to rows
// out_rows[i] (or i).  Queries the margin select cannot finish are appended to flag_list (flag_count is NOT reset here).
static int margin_for_rows(const ccr_index *ix, const uint16_t *Qc, const float *hint, const uint32_t *out_rows, int n, int k, float *scratch,
                           size_t scratch_bytes, float *out_scores, int64_t *out_ids, uint32_t *flag_count, uint32_t *flag_list, hipStream_t s) {
    const int64_t pitch = round_up(ix->n_rows, 4);
    int64_t chunk = (int64_t)(scratch_bytes / ((size_t)pitch * 4));   // score rows the scratch holds: any number of query blocks per launch
    CCR_REQUIRE(chunk >= 1, "margin path: no room for one score row");
    if (chunk > TILE_Q) chunk = chunk / TILE_Q * TILE_Q;
    const int ranges = (int)round_up(std::min<int64_t>(std::max<int64_t>(1, tiles_of(ix) / 4), 1024), NUM_XCD);   // ~4 tiles per work item
    for (int lo = 0; lo < n; lo += (int)chunk) {
        const int m = std::min<int64_t>(chunk, n - lo);
        const uint16_t *Q = Qc + (int64_t)lo * ix->dim;
        int rc = store_scores(ix, Q, m, ranges, scratch, pitch, s);
        if (rc != CCR_OK) return rc;
        rc = launch_margin_select(scratch, pitch, ix->n_rows, k, ix->dim, Q, ix->D, ix->dtype, ix->tile_norm, ix->row_norm, ix->dmax_bits,
                                  hint ? hint + lo : nullptr, out_rows ? out_rows + lo : nullptr, lo, m, ix->id_out, out_scores, out_ids, flag_count, flag_list, s);
        if (rc != CCR_OK) return rc;
    }
    return CCR_OK;
}

// The main pass: one launch per phase (work items [begin, end) of every XCD set), the thresholds re-tightened from the candidates
// of the ranges completed so far between two launches.
static int run_main_pass(const ccr_index *ix, const Plan &p, const SearchWs &w, const uint16_t *Q, int n_q, hipStream_t s) {
    // (blocks of p.tile_q queries; the sample pass walks blocks of TILE_Q)
    GemmArgs gm = filter_args(ix, p, w, Q, n_q, p.nq_pad, p.main_qblocks, p.main_qgroups, w.thr, w.cq, p.cand);
    gm.qsplit = p.main_qsplit;   // (single launch: items keeps its value, every XCD set holds ranges / 8 * blocks items either way)
    if (p.skip_sampled) {   // the unsampled tiles only, in ascending order (unsampled_tile); the select joins the sampled ones
        gm.n_vt = p.tiles - p.sample_tiles;
        gm.skip_stride = (int)p.sample_stride;
        gm.skip_count = p.sample_tiles;
    }
    const int nrc = NUM_XCD / gm.qgroups, qb_per = gm.qblocks / gm.qgroups, items = p.ranges / nrc * qb_per;
    const int bounds[4] = {0, p.item_a, p.item_b, items};
    ThresholdUpdateArgs u = update_args(ix, w);   // (prev_*: nothing before the first re-tightening)
    u.lay = p.cand, u.qb_per = qb_per, u.tile_q = p.tile_q, u.top = p.item_b ? w.top : nullptr;
    int done = 0;
    for (int ph = 1; ph < 4; ++ph) {
        if (bounds[ph] <= done) continue;
        if (done > 0) {
            const int rl_full = done / qb_per;   // complete range rows
            u.part_blocks = done % qb_per;       // blocks done of the started one
            u.nsub = rl_full * nrc * p.sublists;
            u.nsub_part = u.part_blocks ? (rl_full + 1) * nrc * p.sublists : 0;
            u.top_out = bounds[ph] < items && ph < 3;   // another re-tightening follows this phase
            const int rc = launch_threshold_update(u, s);
            if (rc != CCR_OK) return rc;
            u.prev_nsub = u.nsub, u.prev_part = u.nsub_part, u.prev_blocks = u.part_blocks, u.top_in = true;
        }
        gm.item_begin = done;
        gm.item_end = bounds[ph];
        const MainKernel kind = p.tile_q == WIDE_Q ? MAIN_WIDE : p.mfma16 ? MAIN_16X16 : MAIN_32X32;
        // (side CUs: a single launch on main_grid workgroups that count themselves in; every other plan has main_grid = grid)
        gm.arrive = p.side_cus ? w.arrive : nullptr;
        const int rc = launch_gemm(gm, ix->dtype, kind, EPI_FILTER, p.main_grid, s);
        if (rc != CCR_OK) return rc;
        done = bounds[ph];
    }
    return CCR_OK;
}

// Small batch: the corpus is STREAMED past query rows resident in LDS (ccr_narrow.hip); two atomically filled sub-lists per query
// (their counters were cleared by launch_threshold)
static int run_narrow_pass(const ccr_index *ix, const Plan &p, const SearchWs &w, const uint16_t *Q, int n_q, hipStream_t s) {
    NarrowArgs na;
    memset(&na, 0, sizeof(na));
    na.D = ix->D;
    na.n_rows = ix->n_rows;
    na.dim = ix->dim;
    na.Q = Q;
    na.n_q = n_q;
    na.q_stride = narrow_query_stride(ix->dim);
    na.thr = w.thr;
    na.cq = w.cq;
    na.tile_norm = ix->tile_norm;
    na.cand = w.cand;
    na.cnt = w.cnt;
    na.cap = p.first_lay.cap[0];
    na.groups = p.narrow_groups;
    // one workgroup (8 waves x 12 KiB of loads in flight) per CU: measured at NQ 6.2 / 6.2 / 6.0 TB/s of corpus bytes at n_q = 1 / 16 / 64;
    // two or four per CU -- the 16- and 32-query images would fit -- stream no faster (6.2 / 5.9 TB/s at 1 / 16)
    int ngrid = ix->knobs.narrow_grid > 0 ? ix->knobs.narrow_grid : ix->num_cu;
    const int64_t blocks = (ix->n_rows + 16 * NARROW_WAVES - 1) / (16 * NARROW_WAVES);
    if ((int64_t)ngrid > blocks) ngrid = (int)std::max<int64_t>(1, blocks);
    if (p.narrow_groups == 2) ngrid = std::max(16, ngrid / 16 * 16);   // whole sets of eight (b, b + 8) pairs; a pair shares its row stream
    return launch_narrow_filter(na, ix->dtype, p.narrow, ngrid, s);
}

// n 32-bit words from the device to the host; synchronises the stream
static int read_words(void *host, const void *dev, int n, hipStream_t s) {
    CCR_HIP_CHECK(hipMemcpyAsync(host, dev, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    CCR_HIP_CHECK(hipStreamSynchronize(s));
    return CCR_OK;
}

// The stages of the completion of a fused search (search_complete) read the search from ix->plan and ix->pending.

// Statistics of the search from its events (all of them complete) and its flag line.
static int fused_stats(ccr_index *ix, uint32_t nflag, unsigned long long ncand) {
    const Plan &p = ix->plan;
    ccr_search_stats &st = ix->stats;
    float a = 0, b = 0;
    CCR_HIP_CHECK(hipEventElapsedTime(&st.ms_sample, ix->ev[EV_SAMPLE_BEGIN], ix->ev[EV_SAMPLE_END]));
    CCR_HIP_CHECK(hipEventElapsedTime(&a, ix->ev[EV_BEGIN], ix->ev[EV_SAMPLE_BEGIN]));
    CCR_HIP_CHECK(hipEventElapsedTime(&b, ix->ev[EV_SAMPLE_END], ix->ev[EV_MAIN_BEGIN]));
    st.ms_threshold = a + b;
    CCR_HIP_CHECK(hipEventElapsedTime(&st.ms_main, ix->ev[EV_MAIN_BEGIN], ix->ev[EV_MAIN_END]));
    CCR_HIP_CHECK(hipEventElapsedTime(&st.ms_select, ix->ev[EV_MAIN_END], ix->ev[EV_SELECT_END]));
    CCR_HIP_CHECK(hipEventElapsedTime(&st.ms_total, ix->ev[EV_BEGIN], ix->ev[EV_SELECT_END]));
    st.path = 1;
    st.n_fallback = (int32_t)nflag;
    st.sample_tiles = p.sample_tiles;
    st.ranges = p.narrow ? 1 : p.ranges;                      // (streaming main pass of a small batch: one range, two sub-lists per query)
    st.cap = p.narrow ? p.first_lay.cap[0] : p.cap;
    st.sublists = p.narrow ? p.first_sp : p.sublists;
    st.main_launches = 1 + (p.item_a ? 1 : 0) + (p.item_b ? 1 : 0);
    st.opt_rank = p.opt_rank;
    st.tile_cap = p.opt_rank ? p.tile_cap : 0;
    st.main_grid = p.narrow ? 0 : p.main_grid;
    st.side_cus = p.side_cus;
    st.skipped_tiles = p.skip_sampled ? p.sample_tiles : 0;
    st.main_tile_queries = p.narrow ? 0 : p.tile_q;
    st.n_candidates = (int64_t)ncand;
    return CCR_OK;
}

// Estimated thresholds: a query for which fewer than k rows passed has no list to take a bound from (the select left thr = -inf
// and FLAG_DENSE).  The sample's group maxima are still in the workspace: the CONSERVATIVE threshold (the k-th largest, a valid
// bound) is computed now -- only on this path -- and those of the nflag flagged queries join the retry under it.
static int recover_thresholds(const ccr_index *ix, const SearchWs &w, int nflag) {
    hipStream_t s = ix->pending.stream;
    ThresholdArgs t = threshold_args(ix, w);
    t.thr = w.thr_safe, t.cq = w.cq_safe;
    const int rc = launch_threshold(t, s);
    if (rc != CCR_OK) return rc;
    return launch_underfilled_to_retry(w.flag_list, 0, nflag, w.thr_safe, w.thr, s);
}

// appends the n queries of a device list to the dense list (n_dense entries so far)
static int to_dense(const SearchWs &w, const uint32_t *list, int n, int &n_dense, hipStream_t s) {
    CCR_HIP_CHECK(hipMemcpyAsync(w.dense_list + n_dense, list, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    n_dense += n;
    return CCR_OK;
}

// One group of flagged queries in up to three rounds: a round retries what the previous one flagged again, under thresholds
// re-tightened from the previous round's (truncated) lists.  What is left joins the dense list.
static int retry_group(ccr_index *ix, const SearchWs &w, const uint32_t *cur, int n_cur, int &n_dense) {
    const Plan &p = ix->plan;
    const auto &pd = ix->pending;
    hipStream_t s = pd.stream;
    const int nsub_all = p.ranges * p.sublists;
    for (int round = 0;; ++round) {
        int rc = launch_gather_queries(pd.Q, ix->dim, cur, n_cur, w.thr, w.cq, w.Q2, w.thr2, w.cq2, s);
        if (rc != CCR_OK) return rc;
        const int pad2 = (int)round_up(n_cur, TILE_Q);
        const int64_t cap2 = std::min<int64_t>(8192, (int64_t)(w.cand_bytes / 8) / ((int64_t)nsub_all * pad2) / 4 * 4);
        if (cap2 < 16) break;
        const CandLayout lay2 = one_segment((int)cap2);
        CCR_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)nsub_all * pad2 * 4, s));
        CCR_HIP_CHECK(hipMemsetAsync(w.flag2, 0, 64, s));
        const GemmArgs g = filter_args(ix, p, w, w.Q2, n_cur, pad2, pad2 / TILE_Q, pick_qgroups(pad2 / TILE_Q, ix->dim, ix->knobs), w.thr2, w.cq2, lay2);
        rc = launch_gemm(g, ix->dtype, p.mfma16 ? MAIN_16X16 : MAIN_32X32, EPI_FILTER, p.grid, s);   // TILE_Q blocks: never the wide kernel
        if (rc != CCR_OK) return rc;
        SelectArgs sel = select_args(ix, w);   // of the gathered queries: row i is query cur[i]
        sel.ranges = nsub_all, sel.sp = p.sublists, sel.lay = lay2, sel.n_q = n_cur, sel.nq_pad = pad2;
        sel.Q = w.Q2, sel.thr = w.thr2, sel.cq = w.cq2, sel.out_rows = cur;
        sel.flag_count = w.flag2, sel.flag_list = w.flag2 + 16;
        rc = launch_select_rescore(sel, s);
        if (rc != CCR_OK) return rc;
        ix->stats.n_retried += n_cur;
        uint32_t again = 0;
        rc = read_words(&again, w.flag2, 1, s);
        if (rc != CCR_OK || again == 0) return rc;
        uint32_t *next = (cur == w.list_b) ? w.list_c : w.list_b;
        rc = launch_partition_flags(w.flag2 + 16, 0, (int)again, next, w.dense_list + n_dense, w.counts, s);
        if (rc != CCR_OK) return rc;
        uint32_t hc[2] = {0, 0};
        rc = read_words(hc, w.counts, 2, s);
        if (rc != CCR_OK) return rc;
        n_dense += (int)hc[1];
        const uint32_t *list = cur;
        const int n = n_cur;
        cur = next;
        n_cur = (int)hc[0];
        // none left, three rounds done, or no progress (every retried query overflowed again): the dense path takes them
        if (n_cur == 0 || round == 2 || n_cur >= n) break;
        ThresholdUpdateArgs u = update_args(ix, w);   // of the round's gathered queries, from its lists
        u.nsub = nsub_all, u.lay = lay2, u.n_q = n, u.nq_pad = pad2, u.cq = w.cq2, u.thr = w.thr2;
        rc = launch_threshold_update(u, s);
        if (rc != CCR_OK) return rc;
        rc = launch_scatter_thresholds(list, n, w.thr2, w.thr, s);
        if (rc != CCR_OK) return rc;
    }
    return n_cur > 0 ? to_dense(w, cur, n_cur, n_dense, s) : CCR_OK;
}

// Retry of the n_retry queries of the retry list on the fused path; what it cannot finish joins the dense list.
static int retry_flagged(ccr_index *ix, const SearchWs &w, int n_retry, int &n_dense) {
    const Plan &p = ix->plan;
    const auto &pd = ix->pending;
    const int nsub_all = p.ranges * p.sublists;
    if (nsub_all > 2048) return to_dense(w, w.retry_list, n_retry, n_dense, pd.stream);
    // thresholds re-tightened from everything the first attempt recorded (truncated lists included) -- for every flagged
    // query at once, before the candidate area is reused
    ThresholdUpdateArgs u = update_args(ix, w);
    u.nsub = p.first_nsub, u.sp = p.first_sp, u.lay = p.first_lay;
    int rc = launch_threshold_update(u, pd.stream);
    if (rc != CCR_OK) return rc;
    // The flagged queries are retried in GROUPS that get the whole candidate area to themselves: the fewer queries share
    // it, the larger every sub-list.  A group is as large as still leaves four times the first attempt's capacity (when
    // most of a batch is flagged -- the lists were flooded, not unlucky -- one group per query block: about one corpus
    // pass of ONE block per 256 queries instead of 0.65 ms of fp64 scoring per query).
    const int64_t want_cap = std::min<int64_t>(8192, 4 * (int64_t)p.cap);
    int64_t group = (int64_t)(w.cand_bytes / 8) / ((int64_t)nsub_all * want_cap) / TILE_Q * TILE_Q;
    group = std::max<int64_t>(TILE_Q, std::min<int64_t>(group, round_up(n_retry, TILE_Q)));
    for (int g0 = 0; g0 < n_retry && rc == CCR_OK; g0 += (int)group)
        rc = retry_group(ix, w, w.retry_list + g0, std::min<int>((int)group, n_retry - g0), n_dense);
    return rc;
}

// The exact dense path for the n_dense queries of the dense list: MFMA score rows + margin select first (0.9 ms of GEMM per 256
// queries + one row scan each, against 0.65 ms of fp64 scoring per query); only what that cannot finish -- more than 8 192 rows
// inside the margin, non-finite embeddings -- is left to the fp64 path.
static int complete_dense(ccr_index *ix, const SearchWs &w, int n_dense) {
    const Plan &p = ix->plan;
    const auto &pd = ix->pending;
    hipStream_t s = pd.stream;
    // The candidate area is free by now.  The margin path scores in it when it is larger than the reserved rows.  The fp64 path
    // moves there when it holds 64 rows or more and more than one chunk of queries waits: its 64 x 64 score tiles are a quarter
    // full with the 16 reserved rows (2.2 instead of 0.65 ms per NQ query) -- 64 (or more) queries per chunk in there.
    const bool margin_in_cand = w.cand_bytes > w.dense_bytes;
    const int64_t fit = (int64_t)(w.cand_bytes / ((size_t)ix->n_rows * 4)) / 64 * 64;
    const bool fp64_in_cand = n_dense > p.dense_rows_per_chunk && fit >= 64;
    const int64_t chunk = fp64_in_cand ? std::min<int64_t>(fit, 256) : p.dense_rows_per_chunk;
    float *fp64_scr = fp64_in_cand ? (float *)w.cand : w.dense;
    if (!margin_path_ok(ix, pd.k))
        return dense_for_list(ix, pd.Q, w.dense_list, n_dense, pd.k, fp64_scr, chunk, pd.out_scores, pd.out_ids, s);
    CCR_HIP_CHECK(hipMemsetAsync(w.flag2, 0, 64, s));
    for (int lo = 0; lo < n_dense; lo += p.nq_pad) {   // Q2 holds nq_pad gathered query rows
        const int m = std::min(p.nq_pad, n_dense - lo);
        int rc = launch_gather_queries(pd.Q, ix->dim, w.dense_list + lo, m, w.thr, w.cq, w.Q2, w.thr2, w.cq2, s);
        if (rc != CCR_OK) return rc;
        // (thr2: the gathered thresholds of these queries -- valid lower bounds of their k-th largest scores)
        rc = margin_for_rows(ix, w.Q2, w.thr2, w.dense_list + lo, m, pd.k, margin_in_cand ? (float *)w.cand : w.dense,
                             margin_in_cand ? w.cand_bytes : w.dense_bytes, pd.out_scores, pd.out_ids, w.flag2, w.flag2 + 16, s);
        if (rc != CCR_OK) return rc;
    }
    uint32_t left = 0;
    const int rc = read_words(&left, w.flag2, 1, s);
    if (rc != CCR_OK || left == 0) return rc;
    return dense_for_list(ix, pd.Q, w.flag2 + 16, (int)left, pd.k, fp64_scr, chunk, pd.out_scores, pd.out_ids, s);
}

// Completion of a fused search: read how many queries the select stage flagged and re-do them.
//   * a query whose candidates were dropped (sub-list overflow: a corpus in topical order floods the lists of the query's
//     own cluster) is RETRIED on the fused path: its truncated lists still hold real rows, so the k-th largest of them is a
//     valid -- and now nearly final -- threshold; the flagged queries are compacted and one more main pass + select runs
//     for them alone (about one corpus pass per 256 flagged queries instead of 1.8 ms of fp64 scoring per query);
//   * a query the selection cannot finish (mass ties around the cut) and a query flagged again by the retry take the exact
//     dense path.
// Synchronises the stream.
static int search_complete(ccr_index *ix) {
    auto &pd = ix->pending;
    hipStream_t s = pd.stream;
    const bool was_async = pd.active;
    pd.active = false;
    const SearchWs w = search_ws(ix->plan, ix->n_rows, ix->dim, pd.n_q, pd.k, pd.ws);
    struct { uint32_t nflag, pad; unsigned long long ncand; } host;   // the flag line
    int rc = CCR_OK;
    if (was_async) {
        // the search itself copied its flag line to pinned host memory and recorded EV_ASYNC_END behind it: wait for THAT event,
        // not for the stream -- work enqueued after the search (the next step's pack and search, the exchange) is not waited for
        CCR_HIP_CHECK(hipEventSynchronize(ix->ev[EV_ASYNC_END]));
        host.nflag = ix->host_flags[0];
        host.ncand = *reinterpret_cast<volatile unsigned long long *>(ix->host_flags + 2);
    } else {
        rc = read_words(&host, w.flag_count, 4, s);
        if (rc != CCR_OK) return rc;
    }
    rc = fused_stats(ix, host.nflag, host.ncand);
    if (rc != CCR_OK || host.nflag == 0) return rc;
    rc = ix->plan.opt_rank ? recover_thresholds(ix, w, (int)host.nflag) : CCR_OK;
    if (rc != CCR_OK) return rc;
    rc = launch_partition_flags(w.flag_list, 0, (int)host.nflag, w.retry_list, w.dense_list, w.counts, s);
    if (rc != CCR_OK) return rc;
    uint32_t hc[2] = {0, 0};   // queries to retry, queries for the dense path
    rc = read_words(hc, w.counts, 2, s);
    if (rc != CCR_OK) return rc;
    int n_dense = (int)hc[1];
    if (hc[0] > 0) rc = retry_flagged(ix, w, (int)hc[0], n_dense);
    if (rc == CCR_OK && n_dense > 0) rc = complete_dense(ix, w, n_dense);
    if (rc != CCR_OK) return rc;
    ix->stats.n_dense += n_dense;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_DONE], s));
    CCR_HIP_CHECK(hipStreamSynchronize(s));
    CCR_HIP_CHECK(hipEventElapsedTime(&ix->stats.ms_fallback, ix->ev[EV_SELECT_END], ix->ev[EV_DONE]));
    ix->stats.ms_total += ix->stats.ms_fallback;
    return CCR_OK;
}

extern "C" int ccr_search_finish(ccr_index *ix) {
    CCR_REQUIRE(ix, "ccr_search_finish: null index");
    return ix->pending.active ? search_complete(ix) : CCR_OK;
}

// A search on a plan without the fused path: MFMA score rows + margin select where they apply; what that cannot finish (mass
// ties, non-finite embeddings) and every query of a forced-dense or asynchronous search take the fp64 path.
static int search_dense(ccr_index *ix, const SearchWs &w, const uint16_t *Q, int n_q, int k, float *out_scores, int64_t *out_ids,
                        int flags, hipStream_t s) {
    const bool async = (flags & CCR_SEARCH_ASYNC) != 0;
    const int64_t chunk = ix->plan.dense_rows_per_chunk;
    int rc;
    if (!async && !(flags & CCR_SEARCH_FORCE_DENSE) && margin_path_ok(ix, k)) {
        CCR_HIP_CHECK(hipMemsetAsync(w.flag_count, 0, 64, s));
        rc = margin_for_rows(ix, Q, nullptr, nullptr, n_q, k, w.dense, w.dense_bytes, out_scores, out_ids, w.flag_count, w.flag_list, s);
        if (rc != CCR_OK) return rc;
        uint32_t nf = 0;
        rc = read_words(&nf, w.flag_count, 1, s);
        if (rc != CCR_OK) return rc;
        ix->stats.n_fallback = ix->stats.n_dense = (int32_t)nf;
        if (nf > 0) rc = dense_for_list(ix, Q, w.flag_list, (int)nf, k, w.dense, chunk, out_scores, out_ids, s);
    } else {
        rc = dense_for_list(ix, Q, nullptr, n_q, k, w.dense, chunk, out_scores, out_ids, s);
    }
    if (rc != CCR_OK) return rc;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_DONE], s));
    if (async) return CCR_OK;   // nothing to complete: the dense path has no flagged queries (no timing statistics either)
    CCR_HIP_CHECK(hipStreamSynchronize(s));
    CCR_HIP_CHECK(hipEventElapsedTime(&ix->stats.ms_total, ix->ev[EV_BEGIN], ix->ev[EV_DONE]));
    ix->stats.ms_fallback = ix->stats.ms_total;
    return CCR_OK;
}

// id_out: what the result ids are (ix->offset: int64 global ids; ID_LOCAL_U32: u32 local rows of a shard message).
// flagged_out (device, may be null; zero on entry): an ASYNCHRONOUS search leaves the select stage's flag count there, on the stream.
static int search_impl(ccr_index *ix, const uint16_t *Q_bf16, int n_q, int k, float *out_scores, int64_t *out_ids, int64_t id_out,
                       uint32_t *flagged_out, void *workspace, size_t ws_bytes, int flags, void *stream) {
    CCR_REQUIRE(ix && Q_bf16 && out_scores && out_ids, "ccr_search: null pointer");
    CCR_REQUIRE(n_q >= 0, "ccr_search: n_q=%d", n_q);
    CCR_REQUIRE(k >= 1 && k <= MAX_K && (int64_t)k <= ix->n_rows, "ccr_search: k=%d must be in [1, min(n_rows=%lld, %d)]", k,
                (long long)ix->n_rows, MAX_K);
    CCR_REQUIRE((uintptr_t)Q_bf16 % 16 == 0, "ccr_search: query pointer must be 16-byte aligned");
    CCR_REQUIRE(!ix->pending.active, "ccr_search: an asynchronous search is pending on this index (call ccr_search_finish first)");
    memset(&ix->stats, 0, sizeof(ix->stats));
    ix->main_pass_recorded = false;
    ix->thr_phases_used = 0;
    if (n_q == 0) return CCR_OK;
    hipStream_t s = (hipStream_t)stream;
    ix->id_out = id_out;
    const bool async = (flags & CCR_SEARCH_ASYNC) != 0;
    const int plan_flags = flags & ~CCR_SEARCH_ASYNC;
    const bool side_hint = side_hint_take(ix->device);   // (a dense search takes it as well: the hint is about the search just before)
    if (!(ix->plan_nq == n_q && ix->plan_k == k && ix->plan_flags == plan_flags && ix->plan_side_hint == side_hint)) {
        ix->plan = make_plan(ix->n_rows, ix->dim, n_q, k, plan_flags, ix->num_cu, ix->knobs, side_hint);
        ix->plan_nq = n_q;
        ix->plan_k = k;
        ix->plan_flags = plan_flags;
        ix->plan_side_hint = side_hint;
    }
    const Plan p = ix->plan;
    if (!workspace || ws_bytes < p.total || (uintptr_t)workspace % 256 != 0) {
        set_error("ccr_search: workspace %zu bytes (256-byte aligned) required, got %zu at %p", p.total, ws_bytes, workspace);
        return CCR_ERR_WORKSPACE;
    }
    const SearchWs w = search_ws(p, ix->n_rows, ix->dim, n_q, k, (char *)workspace);
    ix->side_arrive = w.arrive;

    if (!ix->have_events) {   // phase-boundary events of the statistics, created on first use
        for (int i = 0; i < EV_COUNT; ++i) CCR_HIP_CHECK(hipEventCreate(&ix->ev[i]));
        ix->have_events = true;
    }
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_BEGIN], s));
    if (!p.fused) return search_dense(ix, w, Q_bf16, n_q, k, out_scores, out_ids, flags, s);
    ix->pending = {false, Q_bf16, n_q, k, out_scores, out_ids, (char *)workspace, s};   // what the stages below and search_complete read

    CCR_HIP_CHECK(hipMemsetAsync(w.flag_count, 0, 64, s));   // (the main pass's arrival counter with it)
    // every (range, query block) item with at least one tile writes its counters at its end, for the columns below
    // main_qblocks * tile_q (the 256 x 384 kernel leaves [main_qblocks * 384, nq_pad) unwritten: no reader goes past n_q);
    // only a plan with more ranges than tiles (forced fused searches of tiny corpora) leaves counters unwritten
    if ((int64_t)p.ranges > p.tiles - (p.skip_sampled ? p.sample_tiles : 0)) CCR_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)p.ranges * p.nq_pad * p.sublists * 4, s));
    int rc = launch_row_norms(Q_bf16, ix->dtype, n_q, ix->dim, w.qnorm, nullptr, nullptr, s);
    if (rc != CCR_OK) return rc;

    // sample pass -> group maxima -> thresholds
    GemmArgs gs = gemm_args(ix, Q_bf16, n_q, p.nq_pad);
    gs.qgroups = p.qgroups;
    gs.n_vt = p.sample_tiles;
    gs.tile_stride = p.sample_stride;
    gs.ranges = p.sample_ranges;
    gs.gmax = w.gmax;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_SAMPLE_BEGIN], s));
    rc = launch_gemm(gs, ix->dtype, MAIN_32X32, EPI_GMAX, p.grid, s);
    if (rc != CCR_OK) return rc;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_SAMPLE_END], s));
    // (small batches: the streaming pass's sub-list counters are cleared by the threshold launch)
    const bool skip_list = p.skip_sampled && ix->knobs.skip_list;   // the select joins the sampled tiles from the threshold's short lists
    ThresholdArgs t = threshold_args(ix, w);
    if (p.opt_rank) t.k = p.opt_rank, t.tile_cap = p.tile_cap;
    if (p.narrow) t.zero_cnt = w.cnt, t.zero_per_query = NARROW_SUBLISTS;
    if (skip_list) t.glist = w.glist, t.list_cap = skip_list_cap(p.opt_rank);
    rc = launch_threshold(t, s, &ix->thr_phases_used);
    if (rc != CCR_OK) return rc;

    // main pass -> candidates -> select
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_MAIN_BEGIN], s));
    rc = p.narrow ? run_narrow_pass(ix, p, w, Q_bf16, n_q, s) : run_main_pass(ix, p, w, Q_bf16, n_q, s);
    if (rc != CCR_OK) return rc;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_MAIN_END], s));
    ix->main_pass_recorded = true;
    SelectArgs sel = select_args(ix, w);
    sel.ranges = p.first_nsub, sel.sp = p.first_sp, sel.lay = p.first_lay;
    sel.flag_count = w.flag_count, sel.flag_list = w.flag_list, sel.stat_cand = w.stat_cand;
    if (p.skip_sampled)   // the join of the tiles the main pass left out
        sel.gmax = w.gmax, sel.sample_tiles = p.sample_tiles, sel.sample_stride = (int)p.sample_stride, sel.gmax_pitch = p.nq_pad;
    if (skip_list) sel.glist = w.glist, sel.list_cap = t.list_cap;
    rc = launch_select_rescore(sel, s);
    if (rc != CCR_OK) return rc;
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_SELECT_END], s));

    if (!async) return search_complete(ix);   // (synchronous form: every flagged query has been re-done, the header's zero stands)
    // The host does not learn the flag count here, and nothing is re-done on the stream: flagged queries (rare: a sub-list
    // overflow, mass ties, an estimated threshold that failed its check) are completed by ccr_search_finish(), which has the
    // retry pass and the margin path at its disposal (2-3 ms for a handful of NQ queries; an unconditional on-stream chunk of
    // the fp64 path cost 35 ms as soon as ONE query was flagged, and two no-op launches per search when none was).
    // the shard message's header learns the count on the stream: the exchange can be enqueued without the host knowing it
    if (flagged_out) CCR_HIP_CHECK(hipMemcpyAsync(flagged_out, w.flag_count, 4, hipMemcpyDeviceToDevice, s));
    CCR_HIP_CHECK(hipMemcpyAsync((void *)ix->host_flags, w.flag_count, 16, hipMemcpyDeviceToHost, s));   // pinned: stays asynchronous
    CCR_HIP_CHECK(hipEventRecord(ix->ev[EV_ASYNC_END], s));
    ix->pending.active = true;
    return CCR_OK;
}

extern "C" int ccr_search(ccr_index *ix, const uint16_t *Q_bf16, int n_q, int k, float *out_scores, int64_t *out_ids,
                          void *workspace, size_t ws_bytes, int flags, void *stream) {
    CCR_REQUIRE(ix, "ccr_search: null index");
    return search_impl(ix, Q_bf16, n_q, k, out_scores, out_ids, ix->offset, nullptr, workspace, ws_bytes, flags, stream);
}

// ------------------------------------------------------------------ packed shard message (row-sharded multi-GPU search)
static inline size_t shard_rows_at(int n_q, int k) { return (sizeof(ccr_shard_header) + (size_t)n_q * k * 4 + 15) / 16 * 16; }

extern "C" size_t ccr_shard_message_bytes(int n_q, int k) {
    if (n_q < 0 || k < 1) return 0;
    return (shard_rows_at(n_q, k) + (size_t)n_q * k * 4 + 15) / 16 * 16;
}

extern "C" int ccr_search_shard(ccr_index *ix, const uint16_t *Q_bf16, int n_q, int k, void *message, void *workspace, size_t ws_bytes,
                                int flags, void *stream) {
    CCR_REQUIRE(ix && message, "ccr_search_shard: null pointer");
    CCR_REQUIRE((uintptr_t)message % 16 == 0, "ccr_search_shard: message must be 16-byte aligned");
    CCR_REQUIRE(n_q >= 0 && k >= 1, "ccr_search_shard: bad shape n_q=%d k=%d", n_q, k);
    hipStream_t s = (hipStream_t)stream;
    ccr_shard_header h;
    memset(&h, 0, sizeof(h));
    h.magic = CCR_SHARD_MAGIC;
    h.k_valid = (uint32_t)k;
    h.n_covered = 0u;   // (an asynchronous search completes no flagged query by itself: ccr_search_finish does)
    h.row_offset = ix->offset;
    h.n_rows = ix->n_rows;
    int rc = launch_shard_header(h, message, s);   // by value through a kernel: no host buffer, no synchronisation
    if (rc != CCR_OK) return rc;
    if (n_q == 0) return CCR_OK;
    char *m = (char *)message;
    uint32_t *flagged = reinterpret_cast<uint32_t *>(m + offsetof(ccr_shard_header, n_flagged));
    return search_impl(ix, Q_bf16, n_q, k, reinterpret_cast<float *>(m + sizeof(ccr_shard_header)),
                       reinterpret_cast<int64_t *>(m + shard_rows_at(n_q, k)), ID_LOCAL_U32, flagged, workspace, ws_bytes, flags, stream);
}

// ------------------------------------------------------------------ dense score matrix
extern "C" int ccr_scores(const ccr_index *ix, const uint16_t *Q_bf16, int n_q, int mode, float *out, void *stream) {
    CCR_REQUIRE(ix && Q_bf16 && out && n_q > 0, "ccr_scores: bad argument");
    CCR_REQUIRE((uintptr_t)Q_bf16 % 16 == 0, "ccr_scores: query pointer must be 16-byte aligned");
    if (mode == CCR_SCORES_CANONICAL)
        return launch_dense_scores(ix->D, ix->dtype, ix->n_rows, ix->dim, Q_bf16, nullptr, 0, n_q, nullptr, out, (hipStream_t)stream);
    CCR_REQUIRE(mode == CCR_SCORES_MFMA, "ccr_scores: unknown mode %d", mode);
    CCR_REQUIRE(ix->dim % 8 == 0, "ccr_scores: CCR_SCORES_MFMA needs dim %% 8 == 0 (dim=%d)", ix->dim);
    return store_scores(ix, Q_bf16, n_q, (int)round_up(std::min<int64_t>(64, tiles_of(ix)), NUM_XCD), out, 0, (hipStream_t)stream);
}
