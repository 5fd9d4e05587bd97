// ccr_common.h -- shared host/device helpers for the gfx950 retrieval library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "ccr_retrieval.h"

namespace ccr {

void set_error(const char *fmt, ...);

#define CCR_HIP_CHECK(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ccr::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return CCR_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define CCR_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            ccr::set_error(__VA_ARGS__);  \
            return CCR_ERR_INVALID;       \
        }                                 \
    } while (0)

#define CCR_LAUNCH_CHECK()                                                              \
    do {                                                                                \
        hipError_t _e = hipGetLastError();                                              \
        if (_e != hipSuccess) {                                                         \
            ccr::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return CCR_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// ---- geometry of the fused MFMA path (one definition for kernels and planner)
constexpr int TILE_DOCS = 256;      // corpus rows per GEMM tile
constexpr int TILE_Q = 256;         // queries per GEMM tile
constexpr int WIDE_Q = 384;         // ... of the 256 x 384 form of the main pass (gemm_topk16w_kernel)
constexpr int TILE_K = 32;          // K granularity of the fused kernels (one LDS sub-stage = 32 bf16 = 64 B per row): dim % 32 == 0
constexpr int GEMM_THREADS = 512;   // 8 waves: 2 (doc halves) x 4 (query quarters)
constexpr int GROUPS_PER_TILE = 16; // group maxima per (sample tile, query): 2 wave rows x 4 MFMA tiles x 2 lane halves
constexpr int MAX_K = 4096;
constexpr uint32_t FLAG_DENSE = 0x80000000u;   // flagged-list entry: the query needs the exact dense path (not a retry)
constexpr int NUM_XCD = 8;

// Candidate storage of the main pass.  The ranges of one launch (phase) form a segment with its own sub-list capacity:
// the later phases run under re-tightened thresholds and need far fewer slots per sub-list than phase A.
// The sp sub-lists of one (range r, query q) share a CELL of sp * cap[g] records at base[g] + ((r - begin(g)) * nq_pad + q) * sp * cap[g],
// stored SLOT-MAJOR: record `slot` of sub-list (part) s sits at cell + slot * sp + s.  Lists hold one or two records on
// average, so a cell's records fill its first one or two 128-byte lines instead of one line per sub-list -- the readers
// (threshold update, select) are bound by the number of scattered lines they touch, not by bytes.
struct CandLayout {
    int nseg;
    int seg_end[3];     // exclusive end range of each segment (ascending; unused entries = INT_MAX)
    int cap[3];
    long long base[3];  // in 8-byte records from the start of the candidate area
};
// segment of range r: capacity, first range, first record
__host__ __device__ __forceinline__ void cand_segment(const CandLayout &L, int r, int &cap, int &r0, long long &base) {
    const int g = (r >= L.seg_end[0] ? 1 : 0) + (r >= L.seg_end[1] ? 1 : 0);
    r0 = g ? L.seg_end[g - 1] : 0;
    cap = L.cap[g];
    base = L.base[g];
}
// first record (slot 0) of sub-list (r, q, s); slot sl is sp * sl records further
__host__ __device__ __forceinline__ long long cand_sublist(const CandLayout &L, int r, int q, int s, int nq_pad, int sp, int &cap) {
    const int g = (r >= L.seg_end[0] ? 1 : 0) + (r >= L.seg_end[1] ? 1 : 0);
    const int r0 = g ? L.seg_end[g - 1] : 0;
    cap = L.cap[g];
    return L.base[g] + (((long long)(r - r0) * nq_pad + q) * sp) * (long long)cap + s;
}

// The sample pass scores the tiles j * s, j < n (s = sample stride, n = sample tiles).  The v-th of the OTHER tiles in ascending
// order: below n * (s - 1) every run of s - 1 unsampled tiles sits behind one sampled tile, beyond the last sampled tile the shift
// is n.  s = 0: no tile is left out.  Tile counts fit 32 bits (n_rows < 2^32).
__host__ __device__ __forceinline__ int64_t unsampled_tile(int64_t v, int s, int n) {
    if (s == 0) return v;
    const uint32_t u = (uint32_t)v, d = (uint32_t)(s - 1);
    return u < (uint32_t)n * d ? (int64_t)(u + u / d + 1u) : v + n;
}

// Work items of a main-pass launch: item i of the XCD set of XCD `xcd` -> range r and query block qb; returns the range's count of
// virtual tiles (<= 0: nothing to do).  Every XCD set holds (ranges / 8) * qblocks items.
//   qsplit == 0   EQUAL groups: qgroups divides qblocks.  XCD x keeps the qblocks / qgroups blocks of group x % qgroups and the ranges
//                 x / qgroups + (8 / qgroups) * rl; item = rl * blocks_per_group + block_in_group.
//   qsplit == G   UNEQUAL groups, G in {2, 4, 8} with qblocks = G * base + rem: group g = x % G owns the blocks [g * base, (g + 1) * base)
//                 in every range row rl of its range class x / G, as above; the rem SHARED blocks G * base ... of range row rl go to
//                 the group rl % G -- the XCD that walks this very range for its own blocks -- and sit behind them in that row.  G range
//                 rows hold G * base + rem = qblocks items of the XCD, so item i lies in the period i / qblocks; an XCD touches base + rem
//                 blocks, and consecutive items still share a range.
__host__ __device__ __forceinline__ int64_t main_item(int i, int xcd, int qblocks, int qgroups, int qsplit, int ranges, int64_t n_vt, int &r,
                                                      int &qb) {
    const int groups = qsplit ? qsplit : qgroups, g = xcd % groups, rc = xcd / groups, nrc = NUM_XCD / groups;
    const int base = qblocks / groups;   // whole blocks of a group
    int rl, b;
    if (qsplit == 0) {
        rl = i / base;
        b = g * base + i % base;
    } else {
        const int rem = qblocks - base * groups;
        const int period = i / qblocks, o = i - period * qblocks;   // position in the period's G rows: g short rows, the long row g, ...
        int row = g, k = o - g * base;                  // the long row: base own blocks, then the rem shared ones
        if (k < 0) {                                    // a short row before it (base >= 1 here)
            row = o / base;
            k = o - row * base;
        } else if (k >= base + rem) {                   // ... or behind it
            row = (o - rem) / base;
            k = o - rem - row * base;
        }
        rl = period * groups + row;
        b = k >= base ? groups * base + (k - base) : g * base + k;
    }
    const int ri = rc + nrc * rl;
    const int64_t ntile = (n_vt - ri + ranges - 1) / ranges;
    r = ri;   // (outputs written last: storing r before the division changes hipcc's code for the division)
    qb = b;
    return ntile;
}

// epilogues of the fused GEMM kernel; EPI_FILTER's candidate record = one corpus row {MFMA score, row}
enum { EPI_FILTER = 0, EPI_GMAX = 1, EPI_STORE = 2 };

// arguments of the fused GEMM kernels (ccr_main_pass.hip)
struct GemmArgs {
    const uint16_t *D;
    int64_t n_rows;
    int dim;
    const uint16_t *Q;
    int n_q;
    int nq_pad;
    int qblocks;
    int64_t n_vt;         // virtual tiles; real tile = vt * tile_stride
    int64_t tile_stride;
    int ranges;           // item (r, qb) covers virtual tiles r, r + ranges, ...
    // main pass that leaves out the sampled tiles j * skip_stride, j < skip_count: virtual tile v is real tile unsampled_tile(v)
    // (0 / 0: every tile -- all the sample pass, the retry pass and EPI_STORE ever see)
    int skip_stride, skip_count;
    int qgroups;          // query-block groups spread over the XCDs (1, 2, 4 or 8; divides qblocks)
    int qsplit;           // 0, or unequal groups (2, 4, 8) that replace qgroups: main_item() (single-launch main pass only)
    // Work items of an XCD set are numbered item = (range / classes) * blocks_per_group + block_in_group; a launch covers the
    // items [item_begin, item_end) of every XCD set, so a phase can be EXACTLY whole rounds of items whatever the range count
    int item_begin, item_end;
    // EPI_FILTER
    const float *thr;     // [nq_pad] tau_q: a lower bound of the query's k-th largest EXACT score
    const float *cq;      // [nq_pad] margin coefficient gamma * ||q||: |mfma - exact| <= cq * ||d||
    const float *tile_norm;   // [ceil(n_rows / TILE_DOCS)] bound of the row norms of each 256-row tile (the index's)
    uint2 *cand;          // candidate area {score bits, local row}; sub-list addresses and capacities from `lay`
    uint32_t *cnt;        // [ranges][nq_pad][sublists]
    CandLayout lay;
    uint32_t *arrive;     // null, or the counter every workgroup adds 1 to when it starts (a main pass that leaves CUs to side work)
    // EPI_GMAX
    float *gmax;          // [n_vt * 16][nq_pad]
    // EPI_STORE (debug)
    float *store;         // [n_q][store_pitch]
    int64_t store_pitch;  // floats per stored query row (0: n_rows); a multiple of 4 lets a lane store its 4 consecutive rows as 16 bytes
};


// ---- the 16-bit element type of an index and its queries: CCR_DTYPE_BF16 or CCR_DTYPE_F16.  Every kernel that reads an element as a
// NUMBER takes it as the template argument DT; what moves rows around (LDS-DMA, gathers, merges) is byte-level and has none.
// Host side: a run-time type becomes the template argument in ONE place per launcher.  f is a generic lambda whose parameter is a
// std::integral_constant (read its ::value); it returns the launch's status.
template <class F>
inline int dispatch_half(int half_dtype, F &&f) {   // CCR_DTYPE_F16 or CCR_DTYPE_BF16 (the caller has checked)
    return half_dtype == CCR_DTYPE_F16 ? f(std::integral_constant<int, CCR_DTYPE_F16>{}) : f(std::integral_constant<int, CCR_DTYPE_BF16>{});
}
inline int check_half(const char *who, int half_dtype) {
    CCR_REQUIRE(half_dtype == CCR_DTYPE_BF16 || half_dtype == CCR_DTYPE_F16, "%s: half_dtype=%d (CCR_DTYPE_F16 or CCR_DTYPE_BF16)", who, half_dtype);
    return CCR_OK;
}

// ---- device helpers
// The value of a 16-bit element, exactly (both types embed in fp32; fp16 subnormals are kept: v_cvt_f32_f16 follows the kernel's
// fp16/fp64 denormal mode, which hipcc leaves on).  elem_lo / elem_hi: the two elements of a 32-bit word, element 0 in the low half.
template <int DT>
__device__ __forceinline__ float elem_to_f32(uint16_t h) {
    if constexpr (DT == CCR_DTYPE_F16)
        return (float)__builtin_bit_cast(_Float16, h);
    else
        return __uint_as_float(((uint32_t)h) << 16);
}
template <int DT>
__device__ __forceinline__ float elem_lo(uint32_t w) {
    if constexpr (DT == CCR_DTYPE_F16)
        return elem_to_f32<DT>((uint16_t)w);
    else
        return __uint_as_float(w << 16);
}
template <int DT>
__device__ __forceinline__ float elem_hi(uint32_t w) {
    if constexpr (DT == CCR_DTYPE_F16)
        return elem_to_f32<DT>((uint16_t)(w >> 16));
    else
        return __uint_as_float(w & 0xffff0000u);
}

// The canonical fp64 sum of squares of an fp32 row (dim % 4 == 0, 16-byte aligned), one wave per row: lane l owns the float4 chunks c with
// c % 64 == l, accumulated in increasing index, then the butterfly p += shfl_xor(p, off) for off = 32..1 (every lane ends with the same
// sum).  This order is part of the canonical definition (index_ref.row_sumsq); the normalising pack and the kept fp32 rows share it.
__device__ __forceinline__ double wave_sumsq(const float *__restrict__ x, int dim, int lane) {
    double p = 0.0;
    const int nchunk = dim >> 2;
    for (int c = lane; c < nchunk; c += 64) {
        float4 v = reinterpret_cast<const float4 *>(x)[c];
        p = p + (double)v.x * (double)v.x;
        p = p + (double)v.y * (double)v.y;
        p = p + (double)v.z * (double)v.z;
        p = p + (double)v.w * (double)v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    return p;
}

// monotone map float -> uint32 (larger float <-> larger uint); NaN maps above +inf (never produced here)
__device__ __forceinline__ uint32_t f32_orderable(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float orderable_to_f32(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Result ids are written as int64 global ids (row + id_offset) or, for a packed shard message (ccr_search_shard), as the u32 LOCAL row:
// the exchange then moves 8 instead of 12 bytes per entry and the merge adds the shard's row offset from the message header.
constexpr int64_t ID_LOCAL_U32 = INT64_MIN;
__device__ __forceinline__ void store_id(int64_t *out_ids, int64_t pos, int64_t id_offset, uint32_t row) {
    if (id_offset == ID_LOCAL_U32)
        reinterpret_cast<uint32_t *>(out_ids)[pos] = row;
    else
        out_ids[pos] = id_offset + (int64_t)row;
}

// worst-case |mfma fp32 score - exact| <= gamma(dim) * ||q|| * ||d||  (any summation order, each
// fp32 add within 2^-23 relative: see DESIGN.md "filter margins")
__host__ __device__ __forceinline__ float mfma_gamma(int dim) { return (float)dim * 1.1920929e-7f * 1.02f; }

}  // namespace ccr
