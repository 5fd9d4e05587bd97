// ccr_fused.hip -- the fused MFMA path: S^T = D . Q^T on the matrix cores with the top-k filter
// in the epilogue, so the [Q, N] score matrix never exists in HBM.
//
//   sample pass  (EPI_GMAX)  : score every `stride`-th 256-row corpus tile, reduce each 16-row MFMA
//                              fragment to its maximum -> gmax[group][query]
//   threshold    (threshold_kernel): tau_q = k-th largest group maximum (a lower bound of the k-th
//                              largest score: k disjoint groups hold a score >= tau_q), minus the
//                              MFMA error margins (cq * tile norm)
//   main pass    (EPI_FILTER): score the whole shard; accumulators >= thr_q are appended to the
//                              (range, query) candidate list (LDS counter, 8-byte records)
//   select       (select_rescore_kernel): per query radix-select the k-th largest MFMA score among
//                              the candidates, keep everything whose error interval reaches it, re-score those
//                              canonically (fp64 ordered) and sort by (score desc, id asc).
//
// GEMM geometry (gfx950): 256 docs x 256 queries per workgroup tile, 512 threads = 8 waves as
// 2 (doc halves) x 4 (query quarters); each wave owns 128 docs x 64 queries (docs on the accumulator
// rows/registers, queries on the lanes, so a lane compares its registers against ONE threshold per
// query column).  Staging: global_load_lds_dwordx4 into a ring of four 32-KiB sub-stages (32 K
// elements = 64-B rows), the 16-byte chunk index XOR-swizzled on the SOURCE address and on the
// fragment read (conflict-free ds_read_b128).  One body, main_pass_256, serves two MFMA shapes:
//   gemm_topk_kernel     v_mfma_f32_32x32x16_bf16 / _f16 (Mfma32): the sample pass (EPI_GMAX), and EPI_FILTER / EPI_STORE where
//                        the plan or CCR_MFMA16=0 picks it
//   gemm_topk16_kernel   v_mfma_f32_16x16x32_bf16 / _f16 (Mfma16): the default 256 x 256 main pass (EPI_FILTER) and EPI_STORE
// gemm_topk16w_kernel is the 256 x 384 form of the 16x16 main pass (EPI_FILTER, dim % 32 == 0) on a body of its own.
#include <stdlib.h>

#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "ccr_gemm_common.h"
#include "ccr_index.h"
#include "ccr_topk_device.h"

namespace ccr {

// 16 zero bytes: what the LDS-DMA reads for the K chunks of the LAST sub-stage that lie beyond the row end when dim % 32 != 0
// (TAIL instantiations; rows are dim * 2 bytes, dim % 8 == 0, so a 16-byte chunk is wholly inside or wholly outside a row)
__device__ __attribute__((aligned(16))) uint32_t g_zero_chunk[4];

// Wave-uniform 4-byte load through the scalar cache (lgkmcnt, not vmcnt), complete on return.
__device__ __forceinline__ float load_uniform_f32(const float *p) {
    float v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}

// s_waitcnt vmcnt(N) with a compile-time N
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef float f32x4v __attribute__((ext_vector_type(4)));

// Maximum of a 16x16 MFMA tile's four registers in two VALU instructions (fmaxf() costs four: hipcc canonicalises the operands first).
// Every VALU instruction of the filter counts: it is issued while the partner wave of the SIMD runs its MFMAs and gets a slot only now
// and then (in-kernel stamps: the tile epilogue was 17 % of a wave's time with fmaxf trees and the first hit path).
__device__ __forceinline__ float max4_asm(const f32x4v &c) {
    float m;
    asm("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %0, %4" : "=&v"(m) : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]));
    return m;
}
__device__ __forceinline__ float max3_asm(float a, float b, float c) {
    float m;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}

// Real corpus tile of virtual tile vt (wave-uniform: scalar registers).  A main pass that leaves out the sampled tiles (a.skip_stride:
// its tile_stride is 1) maps through unsampled_tile(); every other launch keeps vt * tile_stride.
__device__ __forceinline__ int64_t real_tile(const GemmArgs &a, int64_t vt) {
    return a.skip_stride ? unsampled_tile(vt, a.skip_stride, a.skip_count) : vt * a.tile_stride;
}

// Work items (range r, query block qb) of a main-pass launch.  Blocks b and b+8 share an XCD (its 4-MiB L2), so XCD x takes
// query-block group x % groups (its query rows stay L2-resident) and the ranges r = x / groups (mod 8 / groups).  Item order:
// consecutive items (the co-resident workgroups of an XCD) share a RANGE and walk its corpus tiles for different query blocks.
// The map itself is main_item() (ccr_common.h: equal groups, or a.qsplit unequal ones whose left-over blocks are shared).
//   for (int item = walk.first(a); item < walk.end; item += walk.step) { ntile = walk.item(a, item, r, qb); ... }
struct ItemWalk {
    int jx, step, xcd, end;   // end: one past this XCD set's last item of the launch
    __device__ __forceinline__ explicit ItemWalk(const GemmArgs &a) {
        xcd = blockIdx.x & (NUM_XCD - 1);
        jx = blockIdx.x >> 3;
        step = gridDim.x >> 3;
        const int count_x = (a.ranges / NUM_XCD) * a.qblocks;   // items of this XCD set over the whole pass (any grouping)
        end = a.item_end < count_x ? a.item_end : count_x;
    }
    __device__ __forceinline__ int first(const GemmArgs &a) const { return a.item_begin + jx; }
    // range r and query block qb of item i; returns the range's tile count (nothing to do when <= 0)
    __device__ __forceinline__ int64_t item(const GemmArgs &a, int i, int &r, int &qb) const {
        return main_item(i, xcd, a.qblocks, a.qgroups, a.qsplit, a.ranges, a.n_vt, r, qb);
    }
};

// =============================================================================================
// The two MFMA shapes of the 256 x 256 tile.  Each wave tile is 128 corpus rows x 64 queries of DT x QT square MFMA tiles of
// edge TILE; a lane holds query column lane % TILE and, per MFMA tile, REGS registers = REGS / 4 groups of four consecutive
// corpus rows, the first at row 4 * (lane / TILE) + 8 * group.  A lane's candidates of one query go to its own sub-list
// wd * SUBLISTS / 2 + lane / TILE of the (range, query) cell.

// v_mfma_f32_32x32x16_bf16: 4 x 2 MFMA tiles, two K steps of 16 per sub-stage: 16 MFMAs, 12 ds_read_b128.
//   C layout: lane -> query column (lane & 31); register e -> corpus row (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) of the 32-row
//   MFMA tile -> 4 candidate sub-lists per (range, query): (wave row, lane >> 5).
//   LDS image: 16-byte chunk c of row r stored at chunk c ^ ((r >> 2) & 3).
template <int ET>
struct Mfma32 {
    typedef f32x16 Acc;
    static constexpr int TILE = 32, REGS = 16, DT = 4, QT = 2, SUBLISTS = 4;
    struct Frags { bf16x8 a[2][4], b[2][2]; };

    static __device__ __forceinline__ int src_swizzle(int row) { return (row >> 2) & 3; }

    int a_base, b_base, cofs[2];   // this lane's fragment offsets in a sub-stage
    __device__ __forceinline__ Mfma32(int lane, int wd, int wq) {
        const int swz = (lane >> 2) & 3;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) cofs[ks] = (((2 * ks + (lane >> 5)) ^ swz) << 4);
        a_base = (wd * 128 + (lane & 31)) * 64;                 // + dt*2048
        b_base = SUB_Q_REGION + (wq * 64 + (lane & 31)) * 64;   // + qt*2048
    }
    __device__ __forceinline__ void read(const char *buf, Frags &f) const {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) f.a[ks][dt] = *reinterpret_cast<const bf16x8 *>(buf + a_base + dt * 2048 + cofs[ks]);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) f.b[ks][qt] = *reinterpret_cast<const bf16x8 *>(buf + b_base + qt * 2048 + cofs[ks]);
        }
    }
    // the MFMAs of one sub-stage; the first sub-stage of a tile starts from C = 0 (no accumulator clearing pass)
    static __device__ __forceinline__ void mma(Acc (&acc)[4][2], const Frags &f, bool first) {
        if (first) {
            const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = mfma_32x32x16<ET>(f.a[0][dt], f.b[0][qt], z);
        } else {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = mfma_32x32x16<ET>(f.a[0][dt], f.b[0][qt], acc[dt][qt]);
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) acc[dt][qt] = mfma_32x32x16<ET>(f.a[1][dt], f.b[1][qt], acc[dt][qt]);
    }

    // maxima of query tile qt: per group of four registers, and per MFMA tile (two 16-row groups, one per lane half)
    static __device__ __forceinline__ void tile_max(const Acc (&acc)[4][2], int qt, float (&sub)[4][4], float (&mdt)[4]) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                sub[dt][g] = fmaxf(fmaxf(acc[dt][qt][4 * g], acc[dt][qt][4 * g + 1]), fmaxf(acc[dt][qt][4 * g + 2], acc[dt][qt][4 * g + 3]));
            mdt[dt] = fmaxf(fmaxf(sub[dt][0], sub[dt][1]), fmaxf(sub[dt][2], sub[dt][3]));
        }
    }
    // The epilogues of a finished wave tile.  row_base: corpus row of this lane's first register; this lane's column of query tile
    // qt is q0 + wq * 64 + qt * 32 + (lane & 31).  Each epilogue walks the query tiles itself: handed one query tile at a time,
    // the filter costs hipcc more registers.
    // EPI_GMAX: the maximum of each 16-row group -> gmax[group][query]
    static __device__ __forceinline__ void gmax(const Acc (&acc)[4][2], const GemmArgs &a, int64_t vt, int q0, int wd, int wq, int lane) {
        const int h = lane >> 5;
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float sub[4][4], mdt[4];
            tile_max(acc, qt, sub, mdt);
            const int ql = wq * 64 + qt * 32 + (lane & 31);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) a.gmax[(vt * GROUPS_PER_TILE + wd * 8 + dt * 2 + h) * a.nq_pad + q0 + ql] = mdt[dt];
        }
    }
    // EPI_FILTER: append every row that may reach its query's threshold to the lane's sub-list
    static __device__ __forceinline__ void filter(const Acc (&acc)[4][2], const float (&thr)[2], const float (&cqv)[2], float nt,
                                                  int64_t row_base, const GemmArgs &a, uint2 *const (&clist)[2], uint32_t (&ncand)[2],
                                                  int cap) {
        const uint32_t row32 = (uint32_t)row_base;
        const int64_t left = a.n_rows - row_base;
        const uint32_t rows_left = left <= 0 ? 0u : (left > 128 ? 128u : (uint32_t)left);   // rows of this block inside the shard
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float sub[4][4], mdt[4];
            tile_max(acc, qt, sub, mdt);
            // a row of this tile can reach tau_q only if mfma + cq * ||d|| >= tau_q, and ||d|| <= nt
            const float t = fmaf(-cqv[qt], nt, thr[qt]);
            const float mall = fmaxf(fmaxf(mdt[0], mdt[1]), fmaxf(mdt[2], mdt[3]));
            if (__ballot(mall >= t) == 0ull) continue;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                if (__ballot(mdt[dt] >= t) == 0ull) continue;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (sub[dt][g] >= t) {  // rare, divergent: <= 4 rows to test
#pragma unroll
                        for (int e2 = 0; e2 < 4; ++e2) {
                            const float v = acc[dt][qt][4 * g + e2];
                            // 32-bit row arithmetic (local rows < 2^32; rows_left = n_rows - first row of this lane's block,
                            // clamped): the hit path is instruction-bound beside the partner's MFMAs
                            const uint32_t off = (uint32_t)(dt * 32 + 8 * g + e2);
                            if (v >= t && off < rows_left) {
                                if (ncand[qt] < (uint32_t)cap) clist[qt][ncand[qt] * 4] = make_uint2(__float_as_uint(v), row32 + off);
                                ++ncand[qt];
                            }
                        }
                    }
                }
            }
        }
    }
};

// v_mfma_f32_16x16x32_bf16: 8 x 4 MFMA tiles, one K step of 32 per sub-stage: 32 MFMAs, 8 + 4 ds_read_b128.  The chip holds a higher
// clock on this shape in power-limited loops (MI355X_MICROARCH 'DVFS give-back' item 7).
//   C layout: lane -> query column (lane & 15), register e -> corpus row 4 * (lane >> 4) + e of the 16-row tile
//   -> a lane owns 4 query columns x 32 rows; 8 candidate sub-lists per (range, query): (wave row, lane >> 4).
//   LDS image: 16-byte chunk c of row r stored at chunk c ^ (((r >> 2) & 1) << 1) (conflict-free for the 16x16 fragment read
//   pattern; brute-forced over all xor tables).
template <int ET>
struct Mfma16 {
    typedef f32x4v Acc;
    static constexpr int TILE = 16, REGS = 4, DT = 8, QT = 4, SUBLISTS = 8;
    struct Frags { bf16x8 a[8], b[4]; };

    static __device__ __forceinline__ int src_swizzle(int row) { return ((row >> 2) & 1) << 1; }

    int a_base, b_base;   // this lane's fragment offsets in a sub-stage
    __device__ __forceinline__ Mfma16(int lane, int wd, int wq) {
        const int cofs = (((lane >> 4) ^ (((lane >> 2) & 1) << 1)) << 4);   // lane >> 4: K chunk of the operand fragments
        a_base = (wd * 128 + (lane & 15)) * 64 + cofs;                      // + dt*1024
        b_base = SUB_Q_REGION + (wq * 64 + (lane & 15)) * 64 + cofs;        // + qt*1024
    }
    __device__ __forceinline__ void read(const char *buf, Frags &f) const {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) f.a[dt] = *reinterpret_cast<const bf16x8 *>(buf + a_base + dt * 1024);
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) f.b[qt] = *reinterpret_cast<const bf16x8 *>(buf + b_base + qt * 1024);
    }
    static __device__ __forceinline__ void mma(Acc (&acc)[8][4], const Frags &f, bool first) {
        if (first) {
            const f32x4v z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
#pragma unroll
                for (int qt = 0; qt < 4; ++qt) acc[dt][qt] = mfma_16x16x32<ET>(f.a[dt], f.b[qt], z);
            return;
        }
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) acc[dt][qt] = mfma_16x16x32<ET>(f.a[dt], f.b[qt], acc[dt][qt]);
    }

    // EPI_FILTER of a finished wave tile (see Mfma32::filter; a query tile's column of this lane is q0 + wq * 64 + qt * 16 + (lane & 15))
    static __device__ __forceinline__ void filter(const Acc (&acc)[8][4], const float (&thr)[4], const float (&cqv)[4], float nt,
                                                  int64_t row_base, const GemmArgs &a, uint2 *const (&clist)[4], uint32_t (&ncand)[4],
                                                  int cap) {
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            float sub[8];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) sub[dt] = max4_asm(acc[dt][qt]);   // (two VALU instructions per tile instead of fmaxf's four)
            const float t = fmaf(-cqv[qt], nt, thr[qt]);   // per-tile margin: mfma + cq * ||d|| >= tau_q with ||d|| <= nt
            float mall = max3_asm(sub[0], sub[1], sub[2]);
            mall = max3_asm(mall, sub[3], sub[4]);
            mall = max3_asm(mall, sub[5], sub[6]);
            mall = fmaxf(mall, sub[7]);
            if (__ballot(mall >= t) == 0ull) continue;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                if (sub[dt] >= t) {  // rare, divergent: 4 rows to test
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = acc[dt][qt][e];
                        const int64_t doc = row_base + dt * 16 + e;
                        if (v >= t && doc < a.n_rows) {
                            if (ncand[qt] < (uint32_t)cap) clist[qt][ncand[qt] * 8] = make_uint2(__float_as_uint(v), (uint32_t)doc);
                            ++ncand[qt];
                        }
                    }
                }
            }
        }
    }
};

// =============================================================================================
// The 256 x 256 main-pass body on MFMA shape S.  Ping-pong schedule: K is walked in 32-element sub-stages through a ring of four
// 32-KiB LDS buffers (up to 3 sub-stages of LDS-DMA in flight, counted vmcnt, raw s_barrier).  The two waves that share a SIMD
// (wave w and w+4) run one barrier interval apart: while one executes its MFMAs, the other reads its next operands from LDS,
// issues the next sub-stage's DMA and runs the top-k filter of a finished tile (VALU beside the partner's MFMAs).
//   per wave and sub-stage u:
//     mem(u):  [filter of a finished tile] wait OWN DMA of u+1 | 12 ds_read_b128 of u | DMA of u+3 | lgkmcnt(0)
//     barrier A_u | MFMAs of u | barrier B_u
// LDS ring protocol (why this is race free):
//   RAW  a wave confirms (vmcnt) its own DMA of sub-stage u in mem(u-1), i.e. before its barrier
//        A_{u-1}; every reader of u starts mem(u) after a later barrier instance.
//   WAR  DMA of u+3 overwrites the buffer of u-1.  It is issued in mem(u); every wave's reads of
//        u-1 were retired (lgkmcnt(0)) before its barrier A_{u-1}, and for both groups that
//        barrier instance precedes every mem(u).
template <class S, int EPI, bool TAIL>
__device__ __forceinline__ void main_pass_256(const GemmArgs &a) {
    static_assert(EPI != EPI_GMAX || S::TILE == 32, "EPI_GMAX exists on the 32x32 shape only");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // (the mask costs nothing once inlined into a kernel with GEMM_THREADS threads, but tells hipcc the range of the thread id while it
    // optimises this body on its own: without it the lane and wave roles are treated as wider and the kernels need more registers)
    const int tid = threadIdx.x & (GEMM_THREADS - 1);
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wd = wv >> 2;   // doc half of the tile
    const int wq = wv & 3;    // query quarter of the tile
    const int lc = lane & (S::TILE - 1);   // query column of the MFMA tiles
    const int lh = lane / S::TILE;         // row group of the accumulators
    const int cell = wd * (S::SUBLISTS / 2) + lh;   // this lane's sub-list of a (range, query)
    const bool g1 = (wv >= 4);  // the trailing half of the ping-pong (wave-uniform)
    const int KS2 = TAIL ? (a.dim + SUB_K - 1) / SUB_K : a.dim / SUB_K;   // TAIL: the last sub-stage is partly zero-filled

    // DMA role: 4 x 1-KiB pieces per sub-stage (16 rows x 64 B each); LDS image is lane-linear, the
    // 16-byte chunk swizzle is applied on the SOURCE address and on the read
    const int srow = wv * 16 + (lane >> 2);  // + piece*128
    const int schunk = (lane & 3) ^ S::src_swizzle(srow);
    const S mfma(lane, wd, wq);

    const ItemWalk walk(a);
    for (int item = walk.first(a); item < walk.end; item += walk.step) {
        int r, qb;
        const int64_t ntile = walk.item(a, item, r, qb);
        if (ntile <= 0) continue;
        const int q0 = qb * TILE_Q;

        // Each lane owns ONE candidate sub-list per query column, so the append counter is a plain
        // register: no atomics anywhere in the filter.
        float thr[S::QT] = {}, cqv[S::QT] = {};
        uint32_t ncand[S::QT] = {};
        uint2 *clist[S::QT] = {};
        int cap = 0;
        if (EPI == EPI_FILTER) {
            int seg_r0;
            long long seg_base;
            cand_segment(a.lay, r, cap, seg_r0, seg_base);   // this range's segment of the candidate area (wave-uniform)
#pragma unroll
            for (int qt = 0; qt < S::QT; ++qt) {
                const int q = q0 + wq * 64 + qt * S::TILE + lc;
                thr[qt] = (q < a.n_q) ? a.thr[q] : __builtin_nanf("");
                cqv[qt] = (q < a.n_q) ? a.cq[q] : 0.f;
                clist[qt] = a.cand + seg_base + ((int64_t)(r - seg_r0) * a.nq_pad + q) * S::SUBLISTS * cap + cell;   // slot-major cell
            }
            // make hipcc wait for the threshold loads HERE, before any LDS-DMA is in flight: its own
            // wait at the first use inside the tile epilogue would be vmcnt(0) and drain the DMA ring
#pragma unroll
            for (int qt = 0; qt < S::QT; ++qt) asm volatile("" : "+v"(thr[qt]), "+v"(cqv[qt]));
        }
        // EPI_STORE: this lane's score row of each query tile, null past the last query (set once per item, like the filter's lists)
        float *dst[S::QT] = {};
        if (EPI == EPI_STORE) {
            const int64_t pitch = a.store_pitch ? a.store_pitch : a.n_rows;
#pragma unroll
            for (int qt = 0; qt < S::QT; ++qt) {
                const int q = q0 + wq * 64 + qt * S::TILE + lc;
                if (q < a.n_q) dst[qt] = a.store + (int64_t)q * pitch;
            }
        }
        const uint16_t *qsrc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int qrow = q0 + i * 128 + srow;
            if (qrow > a.n_q - 1) qrow = a.n_q - 1;
            qsrc[i] = a.Q + (int64_t)qrow * a.dim + schunk * 8;
        }

        typename S::Acc acc[S::DT][S::QT];
        const int64_t U = ntile * KS2;

        // ---- DMA issue stream (runs up to 3 sub-stages ahead of the consumer).  Per-thread source pointers
        // are recomputed once per tile; a sub-stage adds only the K offset.
        int64_t iu = 0, it = 0;
        int iks = 0;
        const uint16_t *dsrc[2];
        auto tile_ptrs = [&]() {
            const int64_t row0 = real_tile(a, r + it * a.ranges) * TILE_DOCS;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int64_t drow = row0 + (i * 128 + srow);
                if (drow > a.n_rows - 1) drow = a.n_rows - 1;
                dsrc[i] = a.D + drow * a.dim + schunk * 8;
            }
        };
        tile_ptrs();
        auto issue = [&]() {
            char *buf = smem + (int)(iu & (RING - 1)) * SUB_BYTES;
            const int k0 = iks * SUB_K;
            if (TAIL && iks == KS2 - 1) {   // wave-uniform: chunks beyond the row end come from the zero chunk
                const bool in = k0 + schunk * 8 < a.dim;
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    glds16(in ? (const void *)(dsrc[i] + k0) : (const void *)g_zero_chunk, buf + (i * 512 + wv * 64) * 16);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    glds16(in ? (const void *)(qsrc[i] + k0) : (const void *)g_zero_chunk, buf + SUB_Q_REGION + (i * 512 + wv * 64) * 16);
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) glds16(dsrc[i] + k0, buf + (i * 512 + wv * 64) * 16);
#pragma unroll
                for (int i = 0; i < 2; ++i) glds16(qsrc[i] + k0, buf + SUB_Q_REGION + (i * 512 + wv * 64) * 16);
            }
            ++iu;
            if (++iks == KS2) {
                iks = 0;
                ++it;
                tile_ptrs();
            }
        };

        // ---- epilogue of a finished 256x256 tile (accumulators still live)
        auto epilogue = [&](int64_t vt, int64_t rt, float nt) {   // rt: the real tile; nt: norm bound of its rows (wave-uniform)
            const int64_t row_base = rt * TILE_DOCS + wd * 128 + 4 * lh;   // + dt * TILE + 8 * group + register
            if constexpr (EPI == EPI_GMAX) {
                S::gmax(acc, a, vt, q0, wd, wq, lane);
            } else if constexpr (EPI == EPI_FILTER) {
                S::filter(acc, thr, cqv, nt, row_base, a, clist, ncand, cap);
            } else {
                const int64_t pitch = a.store_pitch ? a.store_pitch : a.n_rows;
#pragma unroll
                for (int qt = 0; qt < S::QT; ++qt) {
                    if (!dst[qt]) continue;
#pragma unroll
                    for (int dt = 0; dt < S::DT; ++dt)
#pragma unroll
                        for (int g = 0; g < S::REGS / 4; ++g) {   // registers 4g .. 4g+3 are four consecutive corpus rows
                            const int64_t doc = row_base + dt * S::TILE + 8 * g;
                            if ((pitch & 3) == 0 && doc + 3 < a.n_rows) {
                                *reinterpret_cast<float4 *>(dst[qt] + doc) = make_float4(acc[dt][qt][4 * g], acc[dt][qt][4 * g + 1],
                                                                                             acc[dt][qt][4 * g + 2], acc[dt][qt][4 * g + 3]);
                            } else {
#pragma unroll
                                for (int e2 = 0; e2 < 4; ++e2)
                                    if (doc + e2 < a.n_rows) dst[qt][doc + e2] = acc[dt][qt][4 * g + e2];
                            }
                        }
                }
            }
        };

        // ---- prologue: up to 3 sub-stages in flight, sub-stage 0 confirmed and published
        const int npro = U < 3 ? (int)U : 3;
        for (int i = 0; i < npro; ++i) issue();
        if (npro == 3)
            CCR_WAIT_VM(8);
        else if (npro == 2)
            CCR_WAIT_VM(4);
        else
            CCR_WAIT_VM(0);
        CCR_BARRIER();
        if (g1) CCR_BARRIER();

        int cks = 0;
        int64_t ct = 0;
        bool pending = false;
        int64_t pending_vt = 0, pending_rt = 0;
        float pending_nt = 0.f;
        for (int64_t u = 0; u < U; ++u) {
            // ================= mem phase
            if (pending) {
                epilogue(pending_vt, pending_rt, pending_nt);
                pending = false;
            }
            if (u + 1 < U) {  // confirm OWN DMA of sub-stage u+1 (published by the barrier below)
                if (u + 2 < U)
                    CCR_WAIT_VM(4);
                else
                    CCR_WAIT_VM(0);
            }
            typename S::Frags f;
            mfma.read(smem + (int)(u & (RING - 1)) * SUB_BYTES, f);
            if (u + 3 < U) issue();  // into the buffer of sub-stage u-1 (see the WAR note above)
            CCR_WAIT_LGKM0();        // operands in registers BEFORE the barrier; free behind the DMA issue
            CCR_BARRIER();
            // ================= mfma phase
            // no s_setprio(1) here: the partner wave's mem phase carries VALU work (filter, addresses) that a
            // raised MFMA wave would starve (MI355X_MICROARCH 'Two waves per SIMD', item 2)
            S::mma(acc, f, cks == 0);   // first sub-stage of a tile: C = 0 (no accumulator clearing pass)
            if (++cks == KS2) {
                cks = 0;
                // Tile finished.  The leading group filters it at the start of its next mem phase; the trailing
                // group (one barrier interval behind) filters it right here, so that BOTH filters fall into the
                // same interval instead of stalling the partner twice per tile.
                // (the tile's norm bound: a SCALAR load + wait right here, behind the MFMAs just issued -- a vector load would
                // sit in vmcnt among the LDS-DMA pieces and hipcc's own wait for it would drain the ring)
                const int64_t vt_done = r + ct * a.ranges;
                const int64_t rt_done = real_tile(a, vt_done);
                const float nt_done = EPI == EPI_FILTER ? load_uniform_f32(a.tile_norm + rt_done) : 0.f;
                if (g1) {
                    epilogue(vt_done, rt_done, nt_done);
                } else {
                    pending = true;
                    pending_vt = vt_done;
                    pending_rt = rt_done;
                    pending_nt = nt_done;
                }
                ++ct;
            }
            CCR_BARRIER();
        }
        if (pending) epilogue(pending_vt, pending_rt, pending_nt);
        if (!g1) CCR_BARRIER();  // every wave executes the same number of barriers

        if (EPI == EPI_FILTER) {
#pragma unroll
            for (int qt = 0; qt < S::QT; ++qt)
                a.cnt[((int64_t)r * a.nq_pad + q0 + wq * 64 + qt * S::TILE + lc) * S::SUBLISTS + cell] = ncand[qt];
        }
        __syncthreads();  // LDS ring free for the next item
    }
}

template <int ET, int EPI, bool TAIL = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_topk_kernel(const GemmArgs a) { main_pass_256<Mfma32<ET>, EPI, TAIL>(a); }
template <int ET, int EPI, bool TAIL = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_topk16_kernel(const GemmArgs a) { main_pass_256<Mfma16<ET>, EPI, TAIL>(a); }

// =============================================================================================
// WIDE form of the 16x16x32 main pass (round 6): a 256 x 384 tile on the same eight waves.
// Why: the 256 x 256 kernel is bound by the CU's L1 miss path (~48 cycles per 1-KiB LDS-DMA piece, 32 pieces per K step of
// 32 against 1 070 cycles of MFMA).  A wave tile of 128 x 96 -- 192 accumulator registers of the wave's 256 -- takes (256 + 384) x 64 B
// per K step for 1.5x the multiply-adds: -17 % bytes per flop through that path, 14 instead of 18 operand reads per 48 MFMAs, and a
// query count like 3 452 pads to 3 456 (nine blocks) instead of 3 584.  Same occupancy (two waves per SIMD), same ping-pong of the two
// wave groups, same LDS image and swizzle, same candidate layout (8 sub-lists per (range, query): wave row x lane >> 4).
//   registers: 192 accumulators + 8 corpus fragments (32) + 6 query fragments (24) = 248 -- so nothing else may live in registers across
//     the K loop but two lane offsets (WIDE_BFR = 3, the first form: three query fragments, the other three refilled IN PLACE behind
//     the MFMAs of the first three query tiles; 1.4 % slower -- the refills queue behind the partner's operand reads): the thresholds and margin
//     coefficients of the block's 384 queries and the sub-list counters sit in LDS, candidate addresses are rebuilt on a hit, the lane
//     id is recomputed where it is needed (fresh_lane) and the DMA source of every piece is a wave-uniform base + one clamped per-lane
//     offset computed at issue;
//   LDS: a ring of three 40-KiB slots ([256 corpus rows x 64 B][384 query rows x 64 B]; two K steps = 80 KiB in flight) + 3 KiB
//     thresholds + 12 KiB counters = 135 KiB; 5 LDS-DMA pieces (16 rows x 64 B = 1 KiB) per wave and K step.  A second form with
//     separate rings -- corpus four slots deep, fetched by group 0, queries three, fetched by group 1 -- measured 2-3 % slower;
//   protocol, K step u (A_u / B_u: the barriers in front of and behind the step's MFMAs; g1 runs one barrier behind: g1's A_u is the
//     barrier instance of g0's B_u):
//     mem(u): pieces of u + 2 into the slot of u - 1 | [g0: filter of a finished tile] | 8 + 6 ds_read_b128 of u | own pieces of u + 1
//             landed (vmcnt) | lgkmcnt(0) | A_u | 48 MFMAs | [g1: filter] | lgkmcnt(0) | B_u
//     RAW: a wave confirms its pieces of u + 1 before its A_u; the first reader of u + 1 starts behind a later barrier instance.
//     WAR: the slot of u - 1 is rewritten in mem(u).  Fragments read in mem(u - 1) were retired before the reader's A_{u-1}, which
//          for both groups precedes every mem(u).  With WIDE_BFR = 3 the REFILLS (query tiles 3-5 of a wave = rows 48-95 of its
//          96-row group) are read during the MFMAs and retired only before B_{u-1}: g1's B_{u-1} is behind the start of g0's mem(u),
//          so GROUP 0 FETCHES NO REFILL ROW -- its waves take the 16 corpus pieces and rows 0-15 of each query group, group 1 (whose
//          mem(u) starts behind its own B_{u-1} and behind g0's) the query rows 16-95.  (The assignment is kept with six resident
//          fragments: it costs nothing.)
// dim % 32 == 0 only (the planner keeps the 256 x 256 kernel elsewhere).

// The lane id, computed where it is needed (two VALU instructions) instead of living in a register across the K loop: the wide kernel
// has no register to spare for lane coordinates and the addresses derived from them.
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// LDS accesses of the filter as inline asm.  hipcc (ROCm 7.2) tracks LDS-DMA: in front of a C++ load from LDS that it cannot prove
// disjoint from the destination of an LDS-DMA instruction in flight it inserts s_waitcnt vmcnt(0) -- in the pending epilogue, which runs
// right behind the DMA issue of its memory phase, that drained the whole ring once per tile (cycle stamps: 8 500 cycles per epilogue
// WITHOUT a single hit).  The thresholds and counters are never the target of a DMA piece; these accessors say so by not being C++ loads.
__device__ __forceinline__ uint32_t lds_offset(const void *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
// The wide epilogue's cells -- a lane's {tau, cq} pairs and its sub-list counters -- are LANE-PRIVATE: no other lane or wave reads or
// writes them between the item's set-up and its last tile, so nothing here is atomic.  The reads are ISSUED ONLY (no wait): a tile's
// twelve go out back to back and lds_wait_cells() retires them in one round trip instead of twelve.  (Its "+v" operands make every
// use of a cell depend on the wait.)  The counter store is issued only as well: LDS serves a wave's accesses in order, so the next
// tile's read of the same cell sees it, and the K loop's s_waitcnt lgkmcnt(0) in front of the next barrier retires it.
template <int OFF>
__device__ __forceinline__ uint64_t lds_issue_read_b64(uint32_t addr) {
    uint64_t v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ uint32_t lds_issue_read_b32(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ void lds_issue_write_b32(uint32_t addr, uint32_t v) {
    asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
__device__ __forceinline__ void lds_wait_cells(uint64_t (&tc)[6], uint32_t (&cn)[6]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(tc[0]), "+v"(tc[1]), "+v"(tc[2]), "+v"(tc[3]), "+v"(tc[4]), "+v"(tc[5]), "+v"(cn[0]), "+v"(cn[1]), "+v"(cn[2]), "+v"(cn[3]),
                   "+v"(cn[4]), "+v"(cn[5])
                 :
                 : "memory");
}
constexpr int WIDE_SUB_BYTES = (TILE_DOCS + WIDE_Q) * SUB_K * 2;   // 40960
constexpr int WIDE_Q_REGION = TILE_DOCS * SUB_K * 2;               // 16384
constexpr int WIDE_RING = 3;
constexpr int WIDE_PIECES = 5;                                     // 40 pieces of 1 KiB per K step over 8 waves
constexpr int WIDE_QT = 6;                                         // query tiles of 16 per wave
#ifndef WIDE_BFR
#define WIDE_BFR 6                                                 // query fragments resident per K step: 6, or 3 + three refills (the A/B)
#endif
constexpr int WIDE_RING_BYTES = WIDE_RING * WIDE_SUB_BYTES;        // 122880
constexpr size_t WIDE_LDS = (size_t)WIDE_RING_BYTES + WIDE_Q * 8 + (size_t)(GEMM_THREADS / 64) * WIDE_QT * 64 * 4;   // 138240

template <int ET>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_topk16w_kernel(const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *s_tc = reinterpret_cast<float2 *>(smem + WIDE_RING_BYTES);                     // [384] {tau_q, cq} of the item's query block
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(smem + WIDE_RING_BYTES + WIDE_Q * 8);   // [wave][query tile][lane]
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wd = wv >> 2;
    const int wq = wv & 3;
    const bool g1 = (wv >= 4);
    const int KS2 = a.dim / SUB_K;
    const uint32_t pitch = (uint32_t)a.dim * 2u;    // bytes per row
    // TWO lane-dependent registers live across the K loop -- the DMA source offset of a lane inside a piece and its operand-read offset
    // inside a slot --; everything else that depends on the lane is rebuilt from fresh_lane() where it is needed.  (VALU instructions of
    // the memory phase are issued beside the partner wave's MFMAs and wait for a slot: 34 of them per K step for addresses were 30 % of
    // a wave's time.)
    uint32_t lane_src, lane_lds;
    {
        const int ln = fresh_lane();
        const int pr = ln >> 2;                        // row of a DMA piece this lane fetches a 16-byte chunk of
        lane_src = (uint32_t)pr * pitch + (uint32_t)(((ln & 3) ^ (((pr >> 2) & 1) << 1)) << 4);
        lane_lds = (uint32_t)((ln & 15) * 64 + (((ln >> 4) ^ (((ln >> 2) & 1) << 1)) << 4));
    }

    const ItemWalk walk(a);
    for (int item = walk.first(a); item < walk.end; item += walk.step) {
        int r, qb;
        const int64_t ntile = walk.item(a, item, r, qb);
        if (ntile <= 0) continue;
        // (Measured at NQ, nine blocks = 5 MiB of query rows per XCD against 4 MiB of L2: sharing the query block instead of the
        // range, main pass 12.05 ms against 11.49; blocks in two halves, all ranges x first half then x second: 11.75.)
        const int q0 = qb * WIDE_Q;

        int cap, seg_r0;
        long long seg_base;
        cand_segment(a.lay, r, cap, seg_r0, seg_base);   // this range's segment of the candidate area (wave-uniform)
        {
            const int ln = fresh_lane();
            const int tid = wv * 64 + ln;
            if (tid < WIDE_Q) {
                const int q = q0 + tid;
                s_tc[tid] = make_float2((q < a.n_q) ? a.thr[q] : __builtin_nanf(""), (q < a.n_q) ? a.cq[q] : 0.f);
            }
#pragma unroll
            for (int qt = 0; qt < WIDE_QT; ++qt) s_cnt[(wv * WIDE_QT + qt) * 64 + ln] = 0u;
        }
        // (the first read of s_tc is behind at least one barrier; the vector loads above are complete before the first DMA piece is counted)
        CCR_WAIT_VM(0);

        const int qlimit = (a.n_q - 1 - q0 < WIDE_Q - 1) ? a.n_q - 1 - q0 : WIDE_Q - 1;   // last valid row of the query block
        const char *qblk = reinterpret_cast<const char *>(a.Q) + (int64_t)q0 * pitch;

        f32x4v acc[8][WIDE_QT];
        const int U = (int)(ntile * KS2);   // K steps of the item (< 2^31: tiles / ranges x dim / 32)
        // issue state, wave-uniform and advanced incrementally (no per-step multiplies): ring slot, K step inside the tile and -- group 0 --
        // the tile's base address and its last valid row
        int islot = 0, iks = 0;
        int64_t it = 0;
        const char *dtile = nullptr;
        int dlimit = 0;
        auto tile_base = [&]() __attribute__((always_inline)) {
            const int64_t row0 = real_tile(a, r + it * a.ranges) * TILE_DOCS;
            dlimit = (a.n_rows - 1 - row0 < TILE_DOCS - 1) ? (int)(a.n_rows - 1 - row0) : TILE_DOCS - 1;
            dtile = reinterpret_cast<const char *>(a.D) + row0 * pitch;
        };
        tile_base();
        // one K step's pieces of this wave (a piece = 16 image rows x 64 B): group 0, wave w: corpus rows (4 w + i) * 16 .. + 15 (i < 4) and
        // query rows 96 w .. + 15; group 1, wave w: query rows 96 w + 16 (1 + i) .. + 15 (i < 5).  The per-lane offsets are rebuilt at every
        // issue (hoisted out of the K loop they would cost registers the accumulators need); rows beyond the end re-read the last row
        // (their scores are never recorded)
        // do ALL the query rows this wave fetches exist (wave-uniform, fixed for the item)?  Group 0, wave w: rows 96 w .. + 15; group 1: 96 w + 16 .. + 95
        const bool q_whole = g1 ? ((wv - 4) * 96 + 95 <= qlimit) : (wv * 96 + 15 <= qlimit);
        auto issue = [&]() __attribute__((always_inline)) {
            char *buf = smem + islot * WIDE_SUB_BYTES;
            const uint32_t kb = (uint32_t)iks * (SUB_K * 2);
            if (q_whole && (g1 || dlimit == TILE_DOCS - 1)) {
                // every row of every piece exists: wave-uniform bases (scalar arithmetic) + ONE per-lane offset for all the pieces
                const uint32_t voff = lane_src + kb;
                if (!g1) {
                    const char *rows = dtile + (size_t)(wv * 64) * pitch;
#pragma unroll
                    for (int i = 0; i < 4; ++i) glds16(rows + (size_t)(i * 16) * pitch + voff, buf + (wv * 4 + i) * 1024);
                    glds16(qblk + (size_t)(wv * 96) * pitch + voff, buf + WIDE_Q_REGION + wv * 96 * 64);
                } else {
                    const char *rows = qblk + (size_t)((wv - 4) * 96 + 16) * pitch;
                    char *dst = buf + WIDE_Q_REGION + ((wv - 4) * 96 + 16) * 64;
#pragma unroll
                    for (int i = 0; i < WIDE_PIECES; ++i) glds16(rows + (size_t)(i * 16) * pitch + voff, dst + i * 1024);
                }
            } else {
                // the last tile of the shard / the last block of the batch: rows beyond the end re-read the last row (never recorded)
                const int iln = fresh_lane();
                const int pr = iln >> 2;
                const uint32_t co = (uint32_t)(((iln & 3) ^ (((pr >> 2) & 1) << 1)) << 4) + kb;
                auto piece = [&](const char *rows, int row0, int limit, char *dst) __attribute__((always_inline)) {
                    int row = row0 + pr;
                    row = row < limit ? row : limit;
                    glds16(rows + ((uint32_t)row * pitch + co), dst);
                };
                if (!g1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) piece(dtile, (wv * 4 + i) * 16, dlimit, buf + (wv * 4 + i) * 1024);
                    piece(qblk, wv * 96, qlimit, buf + WIDE_Q_REGION + wv * 96 * 64);
                } else {
#pragma unroll
                    for (int i = 0; i < WIDE_PIECES; ++i)
                        piece(qblk, (wv - 4) * 96 + 16 * (1 + i), qlimit, buf + WIDE_Q_REGION + ((wv - 4) * 96 + 16 * (1 + i)) * 64);
                }
            }
            islot = islot == WIDE_RING - 1 ? 0 : islot + 1;
            if (++iks == KS2) {
                iks = 0;
                ++it;
                if (!g1) tile_base();
            }
        };

        auto epilogue = [&](int64_t rt, float nt) __attribute__((always_inline)) {   // rt: the real tile; nt: norm bound of its rows (wave-uniform)
            // (every address below is rebuilt here instead of living in registers across the K loop)
            const int eln = fresh_lane();
            const int l15o = eln & 15, lqo = eln >> 4;
            // candidate cell of (this range, query q0 + ql, sub-list wd * 4 + lqo): a wave-uniform base + a 32-bit byte offset
            // (slot-major: slot n of the cell is 8 records further; 384 queries x 8 x cap <= 8192 x 8 B < 2^32)
            char *const cbase = reinterpret_cast<char *>(a.cand + seg_base + ((int64_t)(r - seg_r0) * a.nq_pad + q0) * 8 * cap + wd * 4);
            const uint32_t row_lo = (uint32_t)(wd * 128 + 4 * lqo);       // + dt * 16 + e: row inside the tile
            const uint32_t tc_addr = lds_offset(s_tc) + (uint32_t)(wq * 96 + l15o) * 8u;                        // + qt * 16 * 8
            const uint32_t cnt_addr = lds_offset(s_cnt) + (uint32_t)(wv * WIDE_QT * 64 + lqo * 16 + l15o) * 4u;   // + qt * 64 * 4
            const int64_t tile_row0 = rt * TILE_DOCS;      // wave-uniform
            const uint32_t rows_left = a.n_rows - tile_row0 < TILE_DOCS ? (uint32_t)(a.n_rows - tile_row0) : (uint32_t)TILE_DOCS;
            // ONE LDS round trip per tile: the six {tau, cq} pairs and the lane's six counters go out back to back, the row maxima of the
            // first query tile are taken while they travel, one wait.  (The operand fragments are dead here in both groups: the registers exist.)
            uint64_t tcr[WIDE_QT];
            uint32_t cnr[WIDE_QT];
            tcr[0] = lds_issue_read_b64<0 * 128>(tc_addr);
            tcr[1] = lds_issue_read_b64<1 * 128>(tc_addr);
            tcr[2] = lds_issue_read_b64<2 * 128>(tc_addr);
            tcr[3] = lds_issue_read_b64<3 * 128>(tc_addr);
            tcr[4] = lds_issue_read_b64<4 * 128>(tc_addr);
            tcr[5] = lds_issue_read_b64<5 * 128>(tc_addr);
            cnr[0] = lds_issue_read_b32<0 * 256>(cnt_addr);
            cnr[1] = lds_issue_read_b32<1 * 256>(cnt_addr);
            cnr[2] = lds_issue_read_b32<2 * 256>(cnt_addr);
            cnr[3] = lds_issue_read_b32<3 * 256>(cnt_addr);
            cnr[4] = lds_issue_read_b32<4 * 256>(cnt_addr);
            cnr[5] = lds_issue_read_b32<5 * 256>(cnt_addr);
            float sub0[8];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) sub0[dt] = max4_asm(acc[dt][0]);
            __builtin_amdgcn_sched_barrier(0);
            lds_wait_cells(tcr, cnr);
#pragma unroll
            for (int qt = 0; qt < WIDE_QT; ++qt) {
                float sub[8];
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) sub[dt] = qt == 0 ? sub0[dt] : max4_asm(acc[dt][qt]);
                // per-tile margin: mfma + cq * ||d|| >= tau_q with ||d|| <= nt
                const float t = fmaf(-__uint_as_float((uint32_t)(tcr[qt] >> 32)), nt, __uint_as_float((uint32_t)tcr[qt]));
                float mall = max3_asm(sub[0], sub[1], sub[2]);
                mall = max3_asm(mall, sub[3], sub[4]);
                mall = max3_asm(mall, sub[5], sub[6]);
                mall = fmaxf(mall, sub[7]);
                if (__ballot(mall >= t) != 0ull) {
                    const uint32_t ql = (uint32_t)(wq * 96 + qt * 16 + l15o);
                    const uint32_t cell = (ql * 8u * (uint32_t)cap + (uint32_t)lqo) * 8u;    // byte offset of slot 0
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt) {
                        if (sub[dt] >= t) {  // divergent: 4 rows to test
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float v = acc[dt][qt][e];
                                const uint32_t row = row_lo + dt * 16 + e;
                                if (v >= t && row < rows_left) {
                                    const uint32_t n = cnr[qt]++;   // the count keeps running past cap: the select flags the overflow
                                    if (n < (uint32_t)cap)
                                        *reinterpret_cast<uint2 *>(cbase + (cell + n * 64u)) = make_uint2(__float_as_uint(v), (uint32_t)tile_row0 + row);
                                }
                            }
                        }
                    }
                }
            }
            lds_issue_write_b32<0 * 256>(cnt_addr, cnr[0]);
            lds_issue_write_b32<1 * 256>(cnt_addr, cnr[1]);
            lds_issue_write_b32<2 * 256>(cnt_addr, cnr[2]);
            lds_issue_write_b32<3 * 256>(cnt_addr, cnr[3]);
            lds_issue_write_b32<4 * 256>(cnt_addr, cnr[4]);
            lds_issue_write_b32<5 * 256>(cnt_addr, cnr[5]);
        };

        const int npro = U < 2 ? U : 2;
        for (int i = 0; i < npro; ++i) issue();
        if (npro == 2)
            wait_vm<WIDE_PIECES>();   // all but the last K step's pieces
        else
            CCR_WAIT_VM(0);
        CCR_BARRIER();
        if (g1) CCR_BARRIER();

        int cks = 0;
        int64_t ct = 0;
        bool pending = false;
        int64_t pending_rt = 0;
        float pending_nt = 0.f;
        int uslot = 0;
        for (int u = 0; u < U; ++u) {
            // the pieces of u + 2 go out FIRST (into the slot of u - 1, free since the barrier just passed): the L1 miss path, which bounds
            // the pass, gets its work at the start of the phase instead of behind the filter and the operand reads (-1 %; two pieces in
            // front of the operand reads and three behind them: +3 %)
            if (u + 2 < U) issue();
            __builtin_amdgcn_sched_barrier(0);
            if (pending) {
                epilogue(pending_rt, pending_nt);
                pending = false;
            }
            const char *abuf = smem + uslot * WIDE_SUB_BYTES;
            const char *bbuf = abuf + WIDE_Q_REGION;
            uslot = uslot == WIDE_RING - 1 ? 0 : uslot + 1;
            const int a_base = wd * 128 * 64 + (int)lane_lds;   // + dt * 1024
            const int b_base = wq * 96 * 64 + (int)lane_lds;    // + qt * 1024
            bf16x8 af[8], bfr[WIDE_BFR];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) af[dt] = *reinterpret_cast<const bf16x8 *>(abuf + a_base + dt * 1024);
#pragma unroll
            for (int qt = 0; qt < WIDE_BFR; ++qt) bfr[qt] = *reinterpret_cast<const bf16x8 *>(bbuf + b_base + qt * 1024);
            if (u + 2 < U)
                wait_vm<WIDE_PIECES>();           // own pieces of u + 1 have landed
            else
                CCR_WAIT_VM(0);
            // (group 0 could confirm its pieces as late as its B_u -- the barrier instance of g1's A_u --: measured 3 % slower)
            CCR_WAIT_LGKM0();
            CCR_BARRIER();
            if (cks == 0) {
                const f32x4v z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int qt = 0; qt < WIDE_QT; ++qt) {
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt) acc[dt][qt] = mfma_16x16x32<ET>(af[dt], bfr[qt % WIDE_BFR], z);
                    if (WIDE_BFR == 3 && qt < 3) {
                        __builtin_amdgcn_sched_barrier(0);
                        bfr[qt] = *reinterpret_cast<const bf16x8 *>(bbuf + b_base + (qt + 3) * 1024);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
#pragma unroll
                for (int qt = 0; qt < WIDE_QT; ++qt) {
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt)
                        acc[dt][qt] = mfma_16x16x32<ET>(af[dt], bfr[qt % WIDE_BFR], acc[dt][qt]);
                    if (WIDE_BFR == 3 && qt < 3) {
                        __builtin_amdgcn_sched_barrier(0);
                        bfr[qt] = *reinterpret_cast<const bf16x8 *>(bbuf + b_base + (qt + 3) * 1024);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (++cks == KS2) {
                cks = 0;
                // (the tile's norm bound: a SCALAR load + wait right here, behind the MFMAs just issued)
                const int64_t rt_done = real_tile(a, r + ct * a.ranges);
                const float nt_done = load_uniform_f32(a.tile_norm + rt_done);
                if (g1) {
                    epilogue(rt_done, nt_done);
                } else {
                    pending = true;
                    pending_rt = rt_done;
                    pending_nt = nt_done;
                }
                ++ct;
            }
            CCR_WAIT_LGKM0();   // the refills of this K step are retired before the barrier behind which group 1 rewrites their rows
            CCR_BARRIER();
        }
        if (pending) epilogue(pending_rt, pending_nt);
        CCR_WAIT_LGKM0();   // the last tile's counter stores, in front of the barrier and the read-out below
        if (!g1) CCR_BARRIER();

        {
            const int ln = fresh_lane();
#pragma unroll
            for (int qt = 0; qt < WIDE_QT; ++qt)
                a.cnt[((int64_t)r * a.nq_pad + q0 + wq * 96 + qt * 16 + (ln & 15)) * 8 + wd * 4 + (ln >> 4)] = s_cnt[(wv * WIDE_QT + qt) * 64 + ln];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// row norms of 16-bit rows (fp32 accumulate: an fp16 square is at most 2^32, at least 2^-48; used only for error margins, inflated by the caller).  With tile_bits (the index's own
// pass over a shard it was given without norms) a wave takes 64 CONSECUTIVE rows at a time and max-accumulates their norms
// into the word of their 256-row tile (four adds per tile); norms of non-negative floats order as unsigned bit patterns and a
// NaN (row with a NaN) stays on top.
template <int ET>
__global__ __launch_bounds__(256) void row_norms_kernel(const uint16_t *__restrict__ X, int64_t rows, int dim,
                                                            float *__restrict__ norms, uint32_t *__restrict__ max_bits,
                                                            uint32_t *__restrict__ tile_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int chunk = tile_bits ? 64 : 1;
    uint32_t wbits = 0u;
    for (int64_t r0 = wave * chunk; r0 < rows; r0 += nwaves * chunk) {
        uint32_t cbits = 0u;
        const int64_t r1 = r0 + chunk < rows ? r0 + chunk : rows;
        for (int64_t r = r0; r < r1; ++r) {
            const uint16_t *x = X + r * dim;
            float s = 0.f;
            for (int c = lane * 8; c < dim; c += 64 * 8) {
                const uint4 v = *reinterpret_cast<const uint4 *>(x + c);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = elem_lo<ET>(w[e]), hi = elem_hi<ET>(w[e]);
                    s = fmaf(lo, lo, s);
                    s = fmaf(hi, hi, s);
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            const float n = sqrtf(s);
            if (norms && lane == 0) norms[r] = n;
            const uint32_t nb = __float_as_uint(n) & 0x7fffffffu;
            cbits = nb > cbits ? nb : cbits;
        }
        if (tile_bits && lane == 0) atomicMax(tile_bits + r0 / TILE_DOCS, cbits);
        wbits = cbits > wbits ? cbits : wbits;
    }
    // one look first: only a wave that would raise the maximum touches the atomic
    if (max_bits && lane == 0 && wbits > __hip_atomic_load(max_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_bits, wbits);
}

// tile_norm[t] = the largest of the row-norm bounds of rows [256 t, 256 t + 256) the pack kernels wrote (bit patterns: a NaN
// bound stays on top).  grid = tiles, block = 256.  No shared maximum here: the ~2 K blocks resident at the start would all
// see the initial zero and queue their atomics on one address (measured: 38 us for this kernel instead of 4).
__global__ __launch_bounds__(256) void tile_norms_kernel(const float *__restrict__ row_bounds, int64_t rows,
                                                        uint32_t *__restrict__ tile_bits) {
    __shared__ uint32_t s_w[4];
    const int64_t r = (int64_t)blockIdx.x * TILE_DOCS + threadIdx.x;
    uint32_t b = r < rows ? (__float_as_uint(row_bounds[r]) & 0x7fffffffu) : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(b, off, 64);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m01 = s_w[0] > s_w[1] ? s_w[0] : s_w[1], m23 = s_w[2] > s_w[3] ? s_w[2] : s_w[3];
        tile_bits[blockIdx.x] = m01 > m23 ? m01 : m23;
    }
}

// max_bits = the largest tile bound (a NaN / Inf poisons the thresholds -> dense path).  One workgroup of 1 024 threads.
__global__ __launch_bounds__(1024) void max_tile_norm_kernel(const uint32_t *__restrict__ tile_bits, int64_t tiles,
                                                            uint32_t *__restrict__ max_bits) {
    __shared__ uint32_t s_w[16];
    uint32_t b = 0u;
    for (int64_t t = threadIdx.x; t < tiles; t += 1024) {
        const uint32_t v = tile_bits[t];
        b = v > b ? v : b;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(b, off, 64);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0u;
        for (int w = 0; w < 16; ++w) m = s_w[w] > m ? s_w[w] : m;
        *max_bits = m;
    }
}

// The wide threshold form: queries per workgroup (x 64 phases) and the smallest sample it is launched for (launch_threshold).
// 16 queries = 1 024 threads reading 64-byte segments of a gmax row: 113 us at NQ (5 248 groups x 3 584 columns) against 161 us for
// the 16-phase form.  8 queries x 64 phases (512 threads, twice the workgroups, 32-byte segments) took 187 us: half-used 64-byte
// sectors cost more than the second workgroup per CU hides (profiles/threshold_epilogue.md).
constexpr int THR_WIDE_QUERIES = 16;
constexpr int THR_WIDE_MIN_BATCHES = 2;

// Sample thresholds.  A sampled 16-row group whose maximum MFMA score is m holds a row whose EXACT score is at least
// m - cq * nt (cq = gamma * ||q||, nt = norm bound of the group's tile), so tau_q = the k-th largest of those lower bounds is
// a lower bound of the query's k-th largest exact score: thr[q] = tau_q, cq[q] = the margin coefficient the later stages use.
// One workgroup = QB queries x PH group phases (thread = ql + QB * ph): a gmax row is read as QB * 4-byte segments (query-contiguous
// layout), every query has its own 256-bin LDS histogram (no same-address atomics), 4 MSB-first passes.  A pass is a chain of
// n_groups / (16 PH) dependent batches of 16 loads per thread and nothing bounds the kernel but that chain: the launcher gives a
// large sample 64 phases (16 waves per workgroup) instead of 16.  The histogram counts do not depend on the order of the adds: every
// form computes the same thresholds bit for bit and the same short list as a set.
// grid = nq_pad / QB, block = QB * PH.
// glist (may be null; [nq_pad][list_cap + 1]): the query's SHORT LIST for the select stage's join of the sampled tiles -- entry 0 the
// count, then the groups whose UPPER bound m + cq * nt reaches tau (written in the last radix pass against tau's upper 24 bits, a value
// <= tau).  The select joins groups whose upper bound reaches L >= tau: all of them are on the list.  About k of the groups qualify
// (k is the threshold's rank here); a count above list_cap tells the select to walk the query's whole column instead.
// (LIST: a kernel of its own, so that the search without lists keeps the registers and the time of the plain kernel)
// Barriers: the waves exchange histogram data through LDS, so every __syncthreads() has its explicit s_waitcnt lgkmcnt(0) in front
// (hipcc emits a bare s_barrier in loops of this kind).
template <bool LIST, int PH, int QB>
__global__ __launch_bounds__(QB * PH) void threshold_kernel(const float *__restrict__ gmax, int64_t n_groups, int n_q, int nq_pad,
                                                           int k, const float *__restrict__ qnorm,
                                                           const uint32_t *__restrict__ dmax_bits, float gamma,
                                                           const float *__restrict__ tile_norm, int64_t sample_stride,
                                                           float *__restrict__ thr, float *__restrict__ cq,
                                                           uint32_t *__restrict__ glist, int list_cap) {
    constexpr int THREADS = QB * PH;
    constexpr int PICK = QB * 16;   // threads of the digit pick: 16 per query, the first PICK of the workgroup (whole waves)
    static_assert(THREADS >= PICK && PICK % 64 == 0 && (QB & (QB - 1)) == 0, "threshold_kernel: shape");
    __shared__ uint32_t s_hist[QB][256];
    __shared__ uint32_t s_prefix[QB], s_remaining[QB], s_nlist[QB];
    const int tid = threadIdx.x;
    const int ql = tid & (QB - 1), ph = tid / QB;
    const int q = blockIdx.x * QB + ql;
    if (tid < QB) {
        s_prefix[tid] = 0;
        s_remaining[tid] = (uint32_t)k;
        s_nlist[tid] = 0;
    }
    uint32_t *const my_list = LIST ? glist + (int64_t)q * (list_cap + 1) : nullptr;

    // |mfma - exact| <= gamma * ||q|| * ||d||; a non-finite row norm anywhere in the shard (NaN / Inf embeddings) poisons
    // every threshold, so that all queries take the exact dense path
    const float dmax = __uint_as_float(*dmax_bits);
    const float c = (q < n_q) ? ((dmax < INFINITY) ? gamma * (qnorm[q] * 1.001f) * 1.001f : __builtin_nanf("")) : 0.f;
    // norm bound of the sampled tile of group g (plain vector loads: staging them in LDS, or scalar loads of the wave-uniform
    // index, both made this kernel slower -- 84 vs 70 us at NQ: they share lgkmcnt with the histogram's LDS atomics)
    auto tile_of = [&](int64_t g) { return tile_norm[(g / GROUPS_PER_TILE) * sample_stride]; };
    auto emit = [&](int64_t g, float v, float tn, uint32_t prefix) {   // last pass only: prefix = tau's upper 24 bits
        if (f32_orderable(fmaf(c, tn, v)) >= prefix) {
            const uint32_t p = atomicAdd(&s_nlist[ql], 1u);
            if (p < (uint32_t)list_cap) my_list[1 + p] = (uint32_t)g;
        }
    };
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        const bool listing = LIST && shift == 0;
        for (int b = tid; b < QB * 256; b += THREADS) (&s_hist[0][0])[b] = 0;
        CCR_WAIT_LGKM0();
        __syncthreads();
        const uint32_t prefix = s_prefix[ql];
        int64_t i = ph;
        for (; i + 15 * PH < n_groups; i += 16 * PH) {   // 16 independent loads in flight per thread (the loop is latency-bound)
            float v[16], tn[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                v[j] = gmax[(i + PH * j) * nq_pad + q];
                tn[j] = tile_of(i + PH * j);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t o = f32_orderable(fmaf(-c, tn[j], v[j]));
                if ((o & mask) == prefix) atomicAdd(&s_hist[ql][(o >> shift) & 255u], 1u);
                if (listing) emit(i + PH * j, v[j], tn[j], prefix);
            }
        }
        for (; i < n_groups; i += PH) {
            const float v = gmax[i * nq_pad + q], tn = tile_of(i);
            const uint32_t o = f32_orderable(fmaf(-c, tn, v));
            if ((o & mask) == prefix) atomicAdd(&s_hist[ql][(o >> shift) & 255u], 1u);
            if (listing) emit(i, v, tn, prefix);
        }
        CCR_WAIT_LGKM0();
        __syncthreads();
        // digit pick on the first PICK threads: 16 lanes per query (16 bins each), shuffle suffix-scan instead of a 256-step serial
        // walk.  Every thread of the workgroup passes the same barriers.
        const bool picker = tid < PICK;
        const int qi = (tid >> 4) & (QB - 1), part = tid & 15;
        uint32_t remaining = 0, own = 0, incl = 0, above = 0, total = 0;
        uint32_t hb[16];
        if (picker) {
            remaining = s_remaining[qi];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                hb[j] = s_hist[qi][16 * part + j];
                own += hb[j];
            }
            incl = own;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const uint32_t t = __shfl_down(incl, off, 16);
                if (part + off < 16) incl += t;
            }
            above = incl - own;
            total = __shfl(incl, 0, 16);
        }
        CCR_WAIT_LGKM0();
        __syncthreads();   // every lane has read s_remaining before the crossing lane rewrites it
        if (picker) {
            if (above < remaining && remaining <= incl) {
                uint32_t cum = above;
                int d = 16 * part;
#pragma unroll
                for (int j = 15; j >= 1; --j) {
                    if (cum + hb[j] >= remaining) {
                        d = 16 * part + j;
                        break;
                    }
                    cum += hb[j];
                }
                s_prefix[qi] |= (uint32_t)d << shift;
                s_remaining[qi] = remaining - cum;
            } else if (part == 0 && total < remaining) {   // fewer groups than k (cannot happen: the planner samples >= 2k)
                s_remaining[qi] = remaining - (total - hb[0]);
            }
        }
        mask |= 0xffu << shift;
        CCR_WAIT_LGKM0();
        __syncthreads();
    }
    if (tid < QB) {
        const int qq = blockIdx.x * QB + tid;
        if (qq < n_q) {
            const float tau = orderable_to_f32(s_prefix[tid]);
            cq[qq] = c;   // tid < QB: q == qq
            thr[qq] = (c < INFINITY) ? tau : __builtin_nanf("");
        }
        if (LIST) my_list[0] = s_nlist[tid];
    }
}


// Visit every record (sub-list j, slot sl) with first <= sl < count[j]: the (sub-list, slot) rectangle is padded to a
// power of two per sub-list, BATCH independent 8-byte loads are issued before the first record is consumed.
template <int THREADS, int BATCH, class At, class Want, class Put>
__device__ __forceinline__ void sweep_sublists(int tid, int n_lists, int first, int longest, const uint32_t *s_cnt, At at,
                                               Want want, Put put) {
    if (longest <= first) return;
    int lw = 0;
    while ((1 << lw) < longest - first) ++lw;
    const int sweep = n_lists << lw;
    for (int i0 = tid; i0 < sweep; i0 += THREADS * BATCH) {
        uint2 e[BATCH];
        int jj[BATCH], ss[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int i = i0 + u * THREADS;
            const int j = i >> lw, sl = first + (i & ((1 << lw) - 1));
            jj[u] = -1;
            ss[u] = sl;
            if (i < sweep && (uint32_t)sl < s_cnt[j] && want(j, sl)) {
                jj[u] = j;
                e[u] = at(j, sl);
            }
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u)
            if (jj[u] >= 0) put(jj[u], ss[u], e[u]);
    }
}

// Progressive thresholds: after a phase of the main pass the k-th largest LOWER BOUND (mfma - cq * tile norm) among the
// candidates found so far is a tighter valid lower bound of the k-th largest exact score (the candidates are real rows with
// their real MFMA scores, whether or not a sub-list overflowed).  thr[q] = max(thr[q], that).
// The candidate lists are one or two 128-byte lines per sub-list scattered over the shard-sized candidate area: reading them
// is what this kernel costs (measured at NQ: 1.4 TB/s of line traffic, 52 us for the 160 sub-lists per query after phase A,
// 138-185 us for the 448 after phase B1).  So the second re-tightening does not read phase A's lists again: the first one
// leaves the k best lower bounds of every query in `top` (k contiguous values), the second merges them with the sub-lists
// completed since.
// grid = n_q, block = 256.  top: [nq_pad] valid counts, then [n_q][k] values (may be null when top_in == top_out == 0).
__global__ __launch_bounds__(256) void threshold_update_kernel(const uint2 *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                              int nsub_full, int nsub_part, int part_blocks, int prev_full,
                                                              int prev_part, int prev_blocks, int qb_per, int sp, int nq_pad,
                                                              const CandLayout lay, int k, int compact,
                                                              const float *__restrict__ cq, const float *__restrict__ tile_norm,
                                                              uint32_t *__restrict__ top, int top_in, int top_out,
                                                              float *__restrict__ thr, int tile_q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_val[];   // [compact] orderable lower bounds of the candidates found so far
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_ctl[4];
    __shared__ uint32_t s_cnt[2048];
    __shared__ uint32_t s_total, s_maxc, s_fill, s_eq;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    // sub-lists complete so far: those of the fully scored ranges, plus one more row of ranges for the queries whose block
    // (position inside its XCD group) was already scored in the partially finished one
    const int qpos = (q / tile_q) % qb_per;
    const int nsub = qpos < part_blocks ? nsub_part : nsub_full;
    uint32_t *top_n = top;
    uint32_t *top_v = top ? top + nq_pad + (int64_t)q * k : nullptr;
    const bool have_prev = top_in && top_n[q] == (uint32_t)k;
    const int j0 = have_prev ? (qpos < prev_blocks ? prev_part : prev_full) : 0;   // lists the previous update already covered
    if (tid == 0) {
        s_total = have_prev ? (uint32_t)k : 0u;
        s_maxc = 0;
        s_fill = 0;
    }
    __syncthreads();
    uint32_t my = 0, mymax = 0;
    for (int j = j0 + tid; j < nsub; j += blockDim.x) {
        uint32_t c = cnt[((int64_t)(j / sp) * nq_pad + q) * sp + (j % sp)];
        int cap;
        (void)cand_sublist(lay, j / sp, q, j % sp, nq_pad, sp, cap);
        if (c > (uint32_t)cap) c = (uint32_t)cap;
        s_cnt[j - j0] = c;
        my += c;
        mymax = c > mymax ? c : mymax;
    }
    if (my) {
        atomicAdd(&s_total, my);
        atomicMax(&s_maxc, mymax);
    }
    __syncthreads();
    if (s_total < (uint32_t)k) {   // not enough rows seen yet: keep the sample threshold
        if (top_out && tid == 0) top_n[q] = 0u;
        return;
    }
    auto sub_base = [&](int j) -> int64_t {
        int cap;
        return cand_sublist(lay, (j0 + j) / sp, q, (j0 + j) % sp, nq_pad, sp, cap);
    };
    uint32_t kth = 0;
    int need_eq = 0, M = 0;
    bool selected = false;   // s_val[0, M) is the set kth was selected from
    {
        // The sub-lists are sparse: one sweep over (sub-list, slot < longest list) with independent loads gathers the
        // scores into LDS, the four radix passes then never touch global memory.  If more candidates exist than the LDS
        // holds, the first `compact` the sweep meets give a first bound (the k-th largest score of ANY k or more real rows
        // is a valid lower bound of the query's k-th largest score); the sweep is then repeated over the records at or above
        // that bound -- far fewer -- until they all fit, so the final bound is the k-th largest of EVERYTHING recorded (a
        // corpus in topical order leaves the good rows in a few sub-lists that a first-come subset would miss).
        const int maxc = (int)s_maxc;
        const float c = cq[q];
        uint32_t keep = 0u;   // orderable bound: records below it are skipped
        auto append = [&](uint32_t o) {
            if (o >= keep) {
                const uint32_t p = atomicAdd(&s_fill, 1u);
                if (p < (uint32_t)compact) s_val[p] = o;
            }
        };
        for (int round = 0; round < 4; ++round) {
            __syncthreads();
            if (tid == 0) s_fill = 0;
            __syncthreads();
            selected = false;
            if (have_prev)
                for (int i = tid; i < k; i += blockDim.x) append(top_v[i]);
            sweep_sublists<256, 8>(
                tid, nsub - j0, 0, maxc, s_cnt, [&](int j, int sl) -> uint2 { return cand[sub_base(j) + (int64_t)sl * sp]; },
                [](int, int) { return true; },
                [&](int, int, uint2 e) { append(f32_orderable(fmaf(-c, tile_norm[e.y / TILE_DOCS], __uint_as_float(e.x)))); });
            __syncthreads();
            const uint32_t filled = s_fill;
            M = (int)(filled < (uint32_t)compact ? filled : (uint32_t)compact);
            if (M < k) break;   // (ties at the bound cut off by the LDS size: keep the bound of the previous round)
            block_radix_select(
                [&](int64_t i, bool &skip) -> uint32_t {
                    (void)skip;
                    return s_val[i];
                },
                (int64_t)M, k, s_hist, s_ctl, kth, need_eq);
            selected = true;
            if (filled <= (uint32_t)compact || kth <= keep) break;   // everything at or above the bound was seen / no progress
            keep = kth;
        }
    }
    if (top_out) {   // the k best lower bounds seen so far, for the next re-tightening (any order)
        if (!selected) {
            if (tid == 0) top_n[q] = 0u;
        } else {
            __syncthreads();
            if (tid == 0) s_fill = s_eq = 0u;
            __syncthreads();
            for (int i = tid; i < M; i += blockDim.x) {
                const uint32_t v = s_val[i];
                bool take = v > kth;
                if (v == kth) take = atomicAdd(&s_eq, 1u) < (uint32_t)need_eq;
                if (take) top_v[atomicAdd(&s_fill, 1u)] = v;
            }
            if (tid == 0) top_n[q] = (uint32_t)k;
        }
    }
    if (tid == 0) {
        const float t1 = orderable_to_f32(kth);
        if (t1 > thr[q]) thr[q] = t1;
    }
}

// Stage-2: per query, candidates -> exact canonical top-k.  grid = n_q, block = THREADS (256; 1024 for large k).
// dyn LDS: [dim bf16 query row][sub-list counts][sub-list offsets][rescore_cap u64 keys][compact x 8-byte candidates]
//
// JOIN of the sampled tiles (gmax != null: the main pass left out the tiles j * sample_stride, j < sample_tiles, and gmax[group][query],
// pitch gmax_pitch, still holds the sample pass's maximum MFMA score of each of their 16-row groups).  Why the result is unchanged:
//   * L, the k-th largest lower bound of the recorded candidates, is the k-th largest lower bound of a SUBSET of the rows, so it is
//     at most the k-th largest exact score -- and it is still taken from the recorded candidates alone;
//   * an unsampled row whose exact score reaches L >= tau was recorded by the filter (the argument without the join);
//   * a sampled row's exact score is at most its sample-pass MFMA score + c ||d||, at most gmax + c * tile_norm of its group: the
//     margin holds for any fp32 summation order, the sample pass's 32x32 shape included;
//   * so a group with gmax + c * tile_norm < L holds no result row, and a group at or above L is re-scored WHOLE (its 16 rows
//     join the collected rows through the same counter and capacity check; an overflow takes the dense path);
//   * ties are settled by the sort on (score, ~row) as before.
template <int ET, int THREADS>
__global__ __launch_bounds__(THREADS) void select_rescore_kernel(const uint2 *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                            int ranges, int sp, int nq_pad, const CandLayout lay, int k, int rescore_cap, int compact,
                                                            int64_t n_rows, float *__restrict__ thr, const float *__restrict__ cq,
                                                            const float *__restrict__ tile_norm, const float *__restrict__ row_norm,
                                                            const uint32_t *__restrict__ dmax_bits,
                                                            const uint16_t *__restrict__ Q, const uint16_t *__restrict__ D,
                                                            int dim, int64_t id_offset, float *__restrict__ out_scores,
                                                            int64_t *__restrict__ out_ids, uint32_t *__restrict__ flag_count,
                                                            uint32_t *__restrict__ flag_list,
                                                            unsigned long long *__restrict__ stat_cand,
                                                            const uint32_t *__restrict__ out_rows, const float *__restrict__ gmax,
                                                            int sample_tiles, int sample_stride, int gmax_pitch,
                                                            const uint32_t *__restrict__ glist, int list_cap, int regular_cap) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const size_t cnt_bytes = ((size_t)(ranges + 1) * 4 + 15) & ~(size_t)15;
    uint16_t *s_q = reinterpret_cast<uint16_t *>(sm);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(sm + (((size_t)dim * 2 + 15) & ~(size_t)15));
    uint32_t *s_off = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(s_cnt) + cnt_bytes);
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(s_off) + cnt_bytes);
    uint2 *s_comp = reinterpret_cast<uint2 *>(s_keys + rescore_cap);   // [compact] gathered candidates
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_ctl[4];
    __shared__ uint32_t s_wsum[THREADS / 64];
    __shared__ int s_flag;
    __shared__ uint32_t s_total, s_maxc, s_fill;
    __shared__ uint32_t s_ncoll;

    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    if (tid == 0) {
        s_flag = 0;
        s_total = 0;
        s_ncoll = 0;
        s_maxc = 0;
        s_fill = 0;
    }
    __syncthreads();
    // `ranges` counts SUB-LISTS here (sp per (range, query)); thread t owns the contiguous sub-lists [t*per, t*per+per)
    // so that the exclusive scan of the counts below is a plain block scan of per-thread sums
    const int per = (ranges + THREADS - 1) / THREADS;
    uint32_t my = 0, mymax = 0;
    for (int j = tid * per; j < min(ranges, tid * per + per); ++j) {
        uint32_t c = cnt[((int64_t)(j / sp) * nq_pad + q) * sp + (j % sp)];
        int cap;
        (void)cand_sublist(lay, j / sp, q, j % sp, nq_pad, sp, cap);
        if (c > (uint32_t)cap) {
            s_flag = 1;  // overflow: some survivors were dropped
            c = (uint32_t)cap;
        }
        s_cnt[j] = c;
        my += c;
        mymax = c > mymax ? c : mymax;
    }
    {   // block exclusive scan of `my` -> s_off[]
        const int lane = tid & 63, wid = tid >> 6;
        uint32_t incl = my;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_wsum[wid] = incl;
        if (my) atomicMax(&s_maxc, mymax);
        for (int c = tid; c < dim / 8; c += THREADS)
            reinterpret_cast<uint4 *>(s_q)[c] = reinterpret_cast<const uint4 *>(Q + (int64_t)q * dim)[c];
        __syncthreads();
        uint32_t base = incl - my;
        for (int w = 0; w < wid; ++w) base += s_wsum[w];
        for (int j = tid * per; j < min(ranges, tid * per + per); ++j) {
            s_off[j] = base;
            base += s_cnt[j];
        }
        if (tid == THREADS - 1) s_total = base;
        __syncthreads();
    }
    if (tid == 0 && stat_cand) atomicAdd(stat_cand, (unsigned long long)s_total);
    // A query the fused path cannot finish is flagged.  Two kinds: candidates were DROPPED (a sub-list overflowed, or fewer
    // than k rows passed) -- the caller retries the main pass for it under the re-tightened threshold its truncated lists
    // still give (FLAG_RETRY); or the selection itself cannot be done here (mass ties around the cut, k beyond the LDS
    // budget) -- only the exact dense path helps (FLAG_DENSE, the top bit of the list entry).
    bool bad = (s_flag != 0) || (s_total < (uint32_t)k);
    bool dense_only = (s_flag == 0) && bad;   // nothing was dropped and still fewer than k rows passed: a retry cannot find more
    // (fewer than k rows passed an ESTIMATED threshold: it was too high, and no list gives a bound -- the exact path, without a hint)
    if (dense_only && thr && tid == 0) thr[q] = -INFINITY;

    // sub-list j = (range j / sp, wave-row / lane part j % sp): cand_sublist() gives its first record and capacity
    auto sub_base = [&](int j) -> int64_t {
        int cap;
        return cand_sublist(lay, j / sp, q, j % sp, nq_pad, sp, cap);
    };
    auto at = [&](int j, int sl) -> uint2 { return cand[sub_base(j) + (int64_t)sl * sp]; };
    const int coll_cap = rescore_cap;
    uint32_t kth = 0;
    int need_eq = 0;
    int n_lds = 0;   // candidates resident in s_comp
    // Every candidate (mfma score m, row d of tile t) has its exact score inside [m - c ||d||, m + c ||d||] (c = gamma ||q||), and
    // ||d|| <= nt.  The LDS records carry the lower bound m - c nt; the k-th largest of them, L, is a lower bound of the k-th
    // largest exact score, and only candidates whose UPPER bound m + c ||d|| -- the ROW's own norm here, so one huge row widens
    // nobody else's interval -- reaches L can be in the result.
    const float c = cq[q];
    bool row_lb = false;   // the records' lower bounds use the row's own norm (the rare overflow sweep) instead of its tile's

    if (!bad && s_total <= (uint32_t)compact) {
        // The sub-lists are sparse: one sweep over (sub-list, slot < longest list) gathers them into LDS at their
        // scanned offsets (independent loads, no atomics); the select then never touches global memory.
        // (1) the first FIRST slots of every cell -- whole 16-byte pairs (slot, parts 2p and 2p + 1), contiguous and
        //     independent of the counts: a cell's slots 0..3 are its first one (sp = 4) or two (sp = 8) lines (issuing these
        //     loads at kernel start, ahead of the count scan, was measured: 398 -> 488 us, the 32 live registers cost more);
        // (2) only lists longer than that are swept: (sub-list, slot FIRST + s), s < W = pow2 >= longest - FIRST.
        // (large k -- the 1 024-thread form -- has lists of three to six records: eight unconditional slots there)
        constexpr int FIRST = THREADS >= 1024 ? 8 : 4, MAXL = 8;   // ranges * FIRST / 2 <= MAXL * THREADS (1 024 / 2 048 sub-lists)
        {
            const int per_cell = FIRST * sp / 2;               // 16-byte pairs per cell
            const int nload = (ranges / sp) * per_cell;
            uint4 v[MAXL];
#pragma unroll
            for (int t = 0; t < MAXL; ++t) {
                const int x = tid + t * THREADS;
                if (x < nload) {
                    const int cell = x / per_cell, w = x - cell * per_cell;
                    int cap;
                    v[t] = *reinterpret_cast<const uint4 *>(cand + cand_sublist(lay, cell, q, 0, nq_pad, sp, cap) + 2 * w);
                }
            }
#pragma unroll
            for (int t = 0; t < MAXL; ++t) {
                const int x = tid + t * THREADS;
                if (x < nload) {
                    const int cell = x / per_cell, w = x - cell * per_cell;
                    const int slot = (2 * w) / sp, part = (2 * w) % sp;
                    const int j = cell * sp + part;
                    if ((uint32_t)slot < s_cnt[j]) s_comp[s_off[j] + slot] = make_uint2(v[t].x, v[t].y);
                    if ((uint32_t)slot < s_cnt[j + 1]) s_comp[s_off[j + 1] + slot] = make_uint2(v[t].z, v[t].w);
                }
            }
        }
        sweep_sublists<THREADS, 8>(tid, ranges, FIRST, (int)s_maxc, s_cnt, at, [](int, int) { return true; },
                                   [&](int j, int sl, uint2 e) { s_comp[s_off[j] + sl] = e; });
        __syncthreads();
        n_lds = (int)s_total;
        for (int i0 = tid; i0 < n_lds; i0 += 4 * THREADS) {   // lower bounds with the TILE's norm (a 42-KB table: cache hits)
            uint2 e[4];
            float rn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * THREADS;
                e[u] = s_comp[i < n_lds ? i : i0];
                rn[u] = tile_norm[e[u].y / TILE_DOCS];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * THREADS;
                if (i < n_lds) s_comp[i] = make_uint2(__float_as_uint(fmaf(-c, rn[u], __uint_as_float(e[u].x))), e[u].y);
            }
        }
        __syncthreads();
    } else if (!bad && compact < k) {
        bad = dense_only = true;   // the LDS budget cannot even hold k records (huge dim * k): exact dense path
    } else if (!bad) {
        // More candidates than the LDS holds.  The k-th largest lower bound of ANY `compact` of them is a valid lower bound of
        // the query's k-th largest, so: keep the first `compact` records whose upper bound passes the current bound (none at
        // first), and while more than that passed, tighten the bound to the k-th largest lower bound of the kept ones and sweep again.
        // Every sweep at least halves what passes (the kept ones are a random part of what passed); 4 sweeps cover
        // 16 x the LDS capacity, beyond that the exact dense path takes the query.
        float keep = -INFINITY;
        bool fits = false;
        row_lb = true;
        for (int round = 0; round < 4 && !fits; ++round) {
            __syncthreads();   // everybody is done with s_comp / s_fill of the previous round
            if (tid == 0) s_fill = 0u;
            __syncthreads();
            sweep_sublists<THREADS, 8>(tid, ranges, 0, (int)s_maxc, s_cnt, at, [](int, int) { return true; },
                                       [&](int, int, uint2 e) {
                                           // (the ROW's own norm on both sides here: records of a tile that holds one huge row
                                           // would otherwise pass every sweep and contribute nothing to the bound)
                                           const float cn = c * row_norm[e.y];
                                           if (__uint_as_float(e.x) + cn >= keep) {
                                               const uint32_t p = atomicAdd(&s_fill, 1u);
                                               if (p < (uint32_t)compact) s_comp[p] = make_uint2(__float_as_uint(__uint_as_float(e.x) - cn), e.y);
                                           }
                                       });
            __syncthreads();
            if (s_fill <= (uint32_t)compact) {
                fits = true;
            } else {
                uint32_t kth0 = 0;
                int eq0 = 0;
                block_radix_select(
                    [&](int64_t i, bool &skip) -> uint32_t {
                        (void)skip;
                        return f32_orderable(__uint_as_float(s_comp[i].x));
                    },
                    compact, k, s_hist, s_ctl, kth0, eq0);
                keep = orderable_to_f32(kth0);
            }
        }
        if (fits)
            n_lds = (int)s_fill;
        else
            bad = dense_only = true;   // (near-)constant scores or k close to the LDS capacity: the exact dense path takes the query
    }
    if (!bad) {
        const int M = n_lds;
        block_radix_select(
            [&](int64_t i, bool &skip) -> uint32_t {
                (void)skip;
                return f32_orderable(__uint_as_float(s_comp[i].x));
            },
            M, k, s_hist, s_ctl, kth, need_eq);
        const float low = orderable_to_f32(kth);                                  // L: the k-th largest lower bound
        // Verification of the threshold the main pass filtered with.  Every row whose exact score reaches tau was recorded; if k
        // candidates have lower bounds >= tau (L >= tau), the k-th largest exact score is >= tau and nothing is missing.  A valid
        // lower bound (conservative thresholds, re-tightened ones) always passes; an ESTIMATED threshold that came out too high
        // fails: the query is retried under L, which is a valid bound.
        if (thr && low < thr[q]) {
            __syncthreads();
            if (tid == 0) {
                thr[q] = low;
                const uint32_t p = atomicAdd(flag_count, 1u);
                flag_list[p] = (out_rows ? out_rows[q] : (uint32_t)q);
            }
            return;
        }
        const float loose = fmaf(-2.f * c, __uint_as_float(*dmax_bits), low);    // no row's upper bound is further above its lower one
        for (int i = tid; i < M; i += THREADS) {
            const uint2 e = s_comp[i];
            const float lb = __uint_as_float(e.x);
            // (the row's own norm only here, for the few records near the cut: 4-byte reads scattered over an n_rows table --
            // taken for every record they cost the k = 1001 select +0.25 ms)
            if (lb >= loose && fmaf(c, row_norm[e.y], fmaf(c, row_lb ? row_norm[e.y] : tile_norm[e.y / TILE_DOCS], lb)) >= low) {
                const uint32_t p = atomicAdd(&s_ncoll, 1u);
                if (p < (uint32_t)coll_cap) s_keys[p] = (unsigned long long)e.y;  // local row for now
            }
        }
        // INVARIANT: `bad` and `dense_only` are workgroup-uniform -- every thread takes the same returns and the same barriers.  So the
        // counter is read where nobody can be adding to it: behind the barrier that ends the collection, and (join) in front of the
        // barrier that starts the joiners.
        // The recorded candidates keep their own limit (regular_cap: what rescore_cap is without the join -- mass ties around the cut
        // take the dense path exactly as they do when every tile is scored, in the retry pass too); joined rows may fill the rest.
        __syncthreads();
        const uint32_t n_recorded = s_ncoll;
        if (n_recorded > (uint32_t)regular_cap) bad = dense_only = true;  // mass ties around the cut
        if (gmax && !bad) {
            __syncthreads();   // every thread has read n_recorded: the joiners may add
            // The groups to test: the threshold kernel's short list of this query (the groups whose upper bound reaches tau <= L: a
            // few dozen 4-byte reads) -- or, without a list or when it overflowed, the query's whole column of the group maxima
            // (one value per 128-byte line: 2.3 GB of line traffic at NQ, measured +0.12 ms of select and a slower pack beside it).
            // Group gi of a sampled tile (Mfma32::gmax): wave row gi >> 3, MFMA tile (gi >> 1) & 3, lane half gi & 1; register e of its
            // 16 holds row (e & 3) + 8 * (e >> 2) of the lane half's rows.
            const int ngroups = sample_tiles * GROUPS_PER_TILE;
            const uint32_t *const my_list = glist ? glist + (int64_t)q * (list_cap + 1) : nullptr;
            const int nlist = my_list ? (int)min(my_list[0], (uint32_t)list_cap + 1u) : list_cap + 1;
            const bool listed = nlist <= list_cap;
            for (int x = tid; x < (listed ? nlist : ngroups); x += THREADS) {
                const int g = listed ? (int)my_list[1 + x] : x;
                const int64_t tile = (int64_t)(g / GROUPS_PER_TILE) * sample_stride;
                if (fmaf(c, tile_norm[tile], gmax[(int64_t)g * gmax_pitch + q]) >= low) {
                    const int gi = g % GROUPS_PER_TILE;
                    const uint32_t row0 = (uint32_t)(tile * TILE_DOCS) + (uint32_t)((gi >> 3) * 128 + ((gi >> 1) & 3) * 32 + (gi & 1) * 4);
                    for (int e = 0; e < 16; ++e) {   // (one slot at a time, exactly as the recorded candidates above)
                        const uint32_t p = atomicAdd(&s_ncoll, 1u);
                        if (p < (uint32_t)coll_cap) s_keys[p] = (unsigned long long)(row0 + (uint32_t)((e & 3) + 8 * (e >> 2)));
                    }
                }
            }
            __syncthreads();   // (no thread adds behind this barrier: the read below is uniform)
            if (s_ncoll > (uint32_t)coll_cap) bad = dense_only = true;  // the joined rows do not fit beside the recorded ones
        }
    }
    if (bad) {
        if (tid == 0) {
            const uint32_t p = atomicAdd(flag_count, 1u);
            flag_list[p] = (out_rows ? out_rows[q] : (uint32_t)q) | (dense_only ? FLAG_DENSE : 0u);
        }
        return;
    }
    const int ncoll = (int)s_ncoll;
    const int np2 = pow2_ceil(ncoll);
    // Canonical re-score.  The candidate rows are scattered over the shard; a thread walking "its" row 16 bytes at a
    // time makes every wave-load touch 64 different cache lines (measured 1.5 TB/s at k = 1000).  Instead the rows are
    // staged through the (now free) candidate area of the LDS in K slices of SB bytes per row: lanes_per_row adjacent
    // lanes fetch one row's slice (whole 64/128-byte segments, all loads of a slice in flight), then every thread runs
    // the fp64 chain of its own row(s) over the slice from LDS.  Element order inside a row is unchanged.
    const size_t stage_bytes = (size_t)compact * 8;
    // (both variants: before the slices were software-pipelined the barriers cost the 256-thread form more than they saved;
    // with the pipeline the NQ select goes 405 -> 308 us -- its re-score 228 -> 130 us -- and a 1/8 shard, whose rows sit in the
    // Infinity Cache, is unchanged)
    int SB = (size_t)ncoll * 144 <= stage_bytes ? 128 : ((size_t)ncoll * 80 <= stage_bytes ? 64 : 0);
    constexpr int PRE = 8;                                               // 16-byte pieces a thread keeps in flight for the next slice
    if (SB == 128 && ncoll * 8 > PRE * THREADS) SB = 64;
    if (SB != 0 && ncoll <= 2 * THREADS && ncoll * (SB / 16) <= PRE * THREADS) {
        char *stage = reinterpret_cast<char *>(s_comp);
        const int stride = SB + 16;                 // +16: consecutive rows start 4 banks apart (conflict-free b128 reads)
        const int lpr = SB / 16;                    // lanes per row and slice (THREADS % lpr == 0: a thread's pieces share one column)
        const int row_bytes = dim * 2;
        const char *Dbytes = reinterpret_cast<const char *>(D);
        const int col = (tid % lpr) * 16;           // byte column of this thread's pieces inside a slice
        // Software pipeline: the pieces of slice s + 1 are loaded into registers while slice s is consumed from the LDS, so the
        // scattered row reads (the bulk of this stage: ~1.5 KB per re-scored row) overlap the fp64 chains instead of sitting
        // between two barriers 24 times per query.
        // (every piece is loaded unconditionally -- an unused slot reads row 0, a column past the row end re-reads column 0 --
        // so that the prefetched values stay in registers; only the store into the LDS is conditional)
        // piece j of this thread belongs to candidate (tid + j * THREADS) / lpr; only its row pointer is kept.  Eight named
        // values, not an array: hipcc leaves a uint4[8] in scratch memory under the 128-register budget of 1 024 threads.
#define CCR_PIECES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
        // address column: a column past the row end (dim = 32 under a 128-byte slice) reads column 0 -- the FIRST load too, not only
        // the refills below: the last corpus row may end exactly at the end of the caller's allocation
        const int acol = col < row_bytes ? col : 0;
        const char *Dcol = Dbytes + acol;
        const int npiece = ncoll * lpr;
#define CCR_DECL(j)                                                                                              \
    const int idx##j = tid + j * THREADS;                                                                        \
    const char *src##j = Dcol + (int64_t)(uint32_t)s_keys[idx##j < npiece ? idx##j / lpr : 0] * row_bytes;      \
    uint4 pre##j = *reinterpret_cast<const uint4 *>(src##j);
        CCR_PIECES(CCR_DECL)
#undef CCR_DECL
        double acc[2] = {0.0, 0.0};
        for (int k0 = 0; k0 < row_bytes; k0 += SB) {
            __syncthreads();                        // the previous slice has been consumed (first pass: s_comp is free)
            const bool col_in = k0 + col < row_bytes;
#define CCR_PUT(j) \
    if (col_in && idx##j < npiece) *reinterpret_cast<uint4 *>(stage + (idx##j / lpr) * stride + col) = pre##j;
            CCR_PIECES(CCR_PUT)
#undef CCR_PUT
            __syncthreads();
            {   // next slice: in flight during the fp64 chains below
                const int kn = (k0 + SB + col < row_bytes) ? k0 + SB : -acol;
#define CCR_GET(j) pre##j = *reinterpret_cast<const uint4 *>(src##j + kn);
                CCR_PIECES(CCR_GET)
#undef CCR_GET
            }
#undef CCR_PIECES
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * THREADS;
                if (i < ncoll) {
                    double a = acc[j];
                    for (int c = 0; c < lpr && k0 + c * 16 < row_bytes; ++c) {
                        const uint4 dv = *reinterpret_cast<const uint4 *>(stage + (size_t)i * stride + c * 16);
                        const uint4 qv = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(s_q) + k0 + c * 16);
                        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
                        const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            a = fma((double)elem_lo<ET>(qw[e]), (double)elem_lo<ET>(dw[e]), a);
                            a = fma((double)elem_hi<ET>(qw[e]), (double)elem_hi<ET>(dw[e]), a);
                        }
                    }
                    acc[j] = a;
                }
            }
        }
        __syncthreads();                            // every loader is done reading the row ids in s_keys
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + j * THREADS;
            if (i < np2) s_keys[i] = i < ncoll ? make_key((float)acc[j], (uint32_t)s_keys[i]) : 0ull;
        }
    } else {
        // each thread reads and rewrites only its own key slots
        for (int i = tid; i < np2; i += blockDim.x) {
            unsigned long long key = 0ull;
            if (i < ncoll) {
                const uint32_t row = (uint32_t)s_keys[i];
                key = make_key(canonical_dot<ET>(s_q, D + (int64_t)row * dim, dim), row);
            }
            s_keys[i] = key;
        }
    }
    block_bitonic_sort_desc(s_keys, np2);
    const int64_t orow = out_rows ? (int64_t)out_rows[q] : (int64_t)q;   // retry pass: compacted query i -> original row
    for (int i = tid; i < k; i += blockDim.x) {
        const unsigned long long key = s_keys[i];
        out_scores[orow * k + i] = key_score(key);
        store_id(out_ids, orow * k + i, id_offset, key_idx(key));
    }
}

// Retry pass set-up: split the flagged list into the queries to retry and the ones that need the dense path, and gather
// the retried queries' rows, thresholds and margins into compact arrays.  One workgroup; counts[0] = retried, counts[1] = dense.
__global__ __launch_bounds__(256) void partition_flags_kernel(const uint32_t *__restrict__ flags, int begin, int n,
                                                             uint32_t *__restrict__ retry_list, uint32_t *__restrict__ dense_list,
                                                             uint32_t *__restrict__ counts) {   // dense_list: the caller's append position
    __shared__ uint32_t s_n[2];
    if (threadIdx.x == 0) s_n[0] = s_n[1] = 0;
    __syncthreads();
    // order inside the two lists does not matter (each entry is a whole query)
    for (int i = begin + threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t f = flags[i];
        if (f & FLAG_DENSE)
            dense_list[atomicAdd(&s_n[1], 1u)] = f & ~FLAG_DENSE;
        else
            retry_list[atomicAdd(&s_n[0], 1u)] = f;
    }
    __syncthreads();
    if (threadIdx.x < 2) counts[threadIdx.x] = s_n[threadIdx.x];
}

// Estimated thresholds: a query for which FEWER than k rows passed (the select left thr[q] = -inf and FLAG_DENSE) gets the conservative
// bound of the sample instead -- a valid lower bound of its k-th largest score -- and becomes an ordinary retry.
__global__ __launch_bounds__(256) void underfilled_to_retry_kernel(uint32_t *__restrict__ flags, int begin, int n,
                                                                  const float *__restrict__ thr_safe, float *__restrict__ thr) {
    const int i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    const uint32_t q = f & ~FLAG_DENSE;
    if ((f & FLAG_DENSE) && thr[q] == -INFINITY && thr_safe[q] > -INFINITY) {   // (a NaN bound -- non-finite embeddings -- stays on the exact path)
        thr[q] = thr_safe[q];
        flags[i] = q;
    }
}

// thr[list[i]] = thr2[i]: the re-tightened thresholds of a retry round go back to the original query order
__global__ __launch_bounds__(256) void scatter_thresholds_kernel(const uint32_t *__restrict__ list, int n, const float *__restrict__ thr2,
                                                                float *__restrict__ thr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) thr[list[i]] = thr2[i];
}

__global__ __launch_bounds__(256) void gather_queries_kernel(const uint16_t *__restrict__ Q, int dim, const uint32_t *__restrict__ list,
                                                            int n, const float *__restrict__ thr, const float *__restrict__ delta,
                                                            uint16_t *__restrict__ Q2, float *__restrict__ thr2,
                                                            float *__restrict__ delta2) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const uint32_t q = list[i];
    for (int c = threadIdx.x; c < dim / 8; c += blockDim.x)
        reinterpret_cast<uint4 *>(Q2 + (int64_t)i * dim)[c] = reinterpret_cast<const uint4 *>(Q + (int64_t)q * dim)[c];
    if (threadIdx.x == 0) {
        thr2[i] = thr[q];
        delta2[i] = delta[q];
    }
}

// ---------------------------------------------------------------------------------------------
// The dynamic-LDS opt-in (> 64 KiB) is a per-device function attribute: it is set the first time a kernel is launched
// on a device and remembered per (kernel, device) -- not on every launch.
int ensure_dynamic_lds(const void *kernel, size_t lds) {
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

template <class K>
static int launch_kernel(K kernel, size_t lds, const GemmArgs &a, int grid, hipStream_t s) {
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), lds);
    if (rc != CCR_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(GEMM_THREADS), lds, s, a);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

// the kernel table of one element type
template <int ET>
static int launch_gemm_of(const GemmArgs &a, MainKernel kind, int epi, int grid, hipStream_t s) {
    if (epi != EPI_FILTER && epi != EPI_GMAX && epi != EPI_STORE) {
        set_error("launch_gemm: unknown epilogue %d", epi);
        return CCR_ERR_INVALID;
    }
    if (kind == MAIN_WIDE) {   // the 256 x 384 form: a.qblocks counts blocks of WIDE_Q queries
        if (epi != EPI_FILTER || a.dim % SUB_K != 0 || a.dim < SUB_K) {
            set_error("launch_gemm: the 256 x 384 kernel takes EPI_FILTER and dim %% %d == 0 only (epi %d, dim %d)", SUB_K, epi, a.dim);
            return CCR_ERR_INVALID;
        }
        return launch_kernel(&gemm_topk16w_kernel<ET>, WIDE_LDS, a, grid, s);
    }
    typedef void (*Kernel)(const GemmArgs);
    static const Kernel k256[2][3][2] = {   // [kind][epi][TAIL: dim % 32 != 0, the last K sub-stage zero-filled]
        {{gemm_topk_kernel<ET, EPI_FILTER>, gemm_topk_kernel<ET, EPI_FILTER, true>},
         {gemm_topk_kernel<ET, EPI_GMAX>, gemm_topk_kernel<ET, EPI_GMAX, true>},
         {gemm_topk_kernel<ET, EPI_STORE>, gemm_topk_kernel<ET, EPI_STORE, true>}},
        {{gemm_topk16_kernel<ET, EPI_FILTER>, gemm_topk16_kernel<ET, EPI_FILTER, true>},
         {nullptr, nullptr},
         {gemm_topk16_kernel<ET, EPI_STORE>, gemm_topk16_kernel<ET, EPI_STORE, true>}},
    };
    const Kernel k = k256[kind == MAIN_16X16][epi][a.dim % SUB_K != 0];
    if (!k) {
        set_error("launch_gemm: the 16x16x32 kernel has no EPI_GMAX");
        return CCR_ERR_INVALID;
    }
    return launch_kernel(k, RING * (size_t)SUB_BYTES, a, grid, s);
}

int launch_gemm(const GemmArgs &a, int dt, MainKernel kind, int epi, int grid, hipStream_t s) {
    return dispatch_half(dt, [&](auto et) { return launch_gemm_of<decltype(et)::value>(a, kind, epi, grid, s); });
}

int launch_row_norms(const uint16_t *X, int dt, int64_t rows, int dim, float *norms, uint32_t *max_bits, uint32_t *tile_bits,
                     hipStream_t s) {
    if (rows <= 0) return CCR_OK;
    int64_t blocks = tile_bits ? (rows + 255) / 256 : (rows + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    return dispatch_half(dt, [&](auto et) {
        hipLaunchKernelGGL(row_norms_kernel<decltype(et)::value>, dim3((unsigned)blocks), dim3(256), 0, s, X, rows, dim, norms, max_bits, tile_bits);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    });
}

int launch_tile_norms(const float *row_bounds, int64_t rows, uint32_t *tile_bits, uint32_t *max_bits, hipStream_t s) {
    if (rows <= 0) return CCR_OK;
    const int64_t tiles = (rows + TILE_DOCS - 1) / TILE_DOCS;
    hipLaunchKernelGGL(tile_norms_kernel, dim3((unsigned)tiles), dim3(256), 0, s, row_bounds, rows, tile_bits);
    hipLaunchKernelGGL(max_tile_norm_kernel, dim3(1), dim3(1024), 0, s, tile_bits, tiles, max_bits);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

// The same thresholds for a SMALL batch (the streaming main pass, n_q <= 128): threshold_kernel gives a query 16 threads, which walk its
// ~4 000 sampled lower bounds four times from global memory -- 70 us for ONE query, a tenth of the whole search.  Here a workgroup
// per query: the lower bounds are staged in LDS once (every load independent, one round trip), the four radix passes read LDS.
// zero_cnt (may be null): the streaming pass's sub-list counters of this query are cleared here instead of by a memset node.
// grid = n_q, block = 256, dyn LDS = n_groups * 4 bytes.
__global__ __launch_bounds__(256) void threshold_small_kernel(const float *__restrict__ gmax, int n_groups, int nq_pad, int k,
                                                             const float *__restrict__ qnorm, const uint32_t *__restrict__ dmax_bits,
                                                             float gamma, const float *__restrict__ tile_norm, int64_t sample_stride,
                                                             float *__restrict__ thr, float *__restrict__ cq, uint32_t *__restrict__ zero_cnt,
                                                             int zero_per_query, uint32_t *__restrict__ glist, int list_cap) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_low[];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_ctl[4];
    __shared__ uint32_t s_nlist;
    const int tid = threadIdx.x, q = blockIdx.x;
    const float dmax = __uint_as_float(*dmax_bits);
    const float c = (dmax < INFINITY) ? gamma * (qnorm[q] * 1.001f) * 1.001f : __builtin_nanf("");
    for (int g = tid; g < n_groups; g += 256)
        s_low[g] = f32_orderable(fmaf(-c, tile_norm[(int64_t)(g / GROUPS_PER_TILE) * sample_stride], gmax[(int64_t)g * nq_pad + q]));
    if (zero_cnt && tid < zero_per_query) zero_cnt[q * zero_per_query + tid] = 0u;
    __syncthreads();
    uint32_t kth = 0;
    int need_eq = 0;
    block_radix_select<true>(
        [&](int64_t i, bool &skip) -> uint32_t {
            (void)skip;
            return s_low[i];
        },
        n_groups, k, s_hist, s_ctl, kth, need_eq);
    if (tid == 0) {
        cq[q] = c;
        thr[q] = (c < INFINITY) ? orderable_to_f32(kth) : __builtin_nanf("");
    }
    if (glist) {   // the select's short list (threshold_kernel): groups whose upper bound reaches tau
        uint32_t *const my_list = glist + (int64_t)q * (list_cap + 1);
        if (tid == 0) s_nlist = 0u;
        __syncthreads();
        for (int g = tid; g < n_groups; g += 256) {
            const float up = fmaf(c, tile_norm[(int64_t)(g / GROUPS_PER_TILE) * sample_stride], gmax[(int64_t)g * nq_pad + q]);
            if (f32_orderable(up) >= kth) {
                const uint32_t p = atomicAdd(&s_nlist, 1u);
                if (p < (uint32_t)list_cap) my_list[1 + p] = (uint32_t)g;
            }
        }
        __syncthreads();
        if (tid == 0) my_list[0] = s_nlist;
    }
}

int launch_threshold(const float *gmax, int64_t n_groups, int n_q, int nq_pad, int k, const float *qnorm,
                     const uint32_t *dmax_bits, int dim, const float *tile_norm, int64_t sample_stride, float *thr, float *cq,
                     hipStream_t s, uint32_t *zero_cnt, int zero_per_query, uint32_t *glist, int list_cap, int phases, int *phases_used) {
    if (phases_used) *phases_used = 0;
    // small batches: a workgroup per query (needs k <= n_groups -- the planner samples >= 2k groups -- and the bounds in 64 KiB of LDS);
    // *zero_cnt tells the caller whether its counters have been cleared here
    if (n_q <= 128 && n_groups >= k && n_groups <= 16384 && zero_per_query <= 256) {
        if (n_groups * 4 > 32 * 1024) {   // (the kernel's static LDS sits on top of the dynamic part: opt in with head room)
            const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&threshold_small_kernel), 72 * 1024);
            if (rc != CCR_OK) return rc;
        }
        hipLaunchKernelGGL(threshold_small_kernel, dim3(n_q), dim3(256), (size_t)n_groups * 4, s, gmax, (int)n_groups, nq_pad, k, qnorm, dmax_bits,
                           mfma_gamma(dim), tile_norm, sample_stride, thr, cq, zero_cnt, zero_per_query, glist, list_cap);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    }
    if (zero_cnt) CCR_HIP_CHECK(hipMemsetAsync(zero_cnt, 0, (size_t)n_q * zero_per_query * 4, s));
    // The wide form (THR_WIDE_QUERIES x 64 phases) wherever every phase still walks at least THR_WIDE_MIN_BATCHES full batches of 16
    // loads per radix pass, n_groups >= 2 x 16 x 64 = 2 048: below that a 64-phase pass is mostly its remainder loop and its barriers
    // across 16 waves, and the 16-phase chain it would shorten is only a few batches long.  `phases` (16 / 64, CCR_THR_PHASES) pins the form.
    const bool wide = phases == 64 || (phases != 16 && n_groups >= (int64_t)THR_WIDE_MIN_BATCHES * 16 * 64);
    if (phases_used) *phases_used = wide ? 64 : 16;
    if (wide)
        hipLaunchKernelGGL((glist ? threshold_kernel<true, 64, THR_WIDE_QUERIES> : threshold_kernel<false, 64, THR_WIDE_QUERIES>),
                           dim3(nq_pad / THR_WIDE_QUERIES), dim3(64 * THR_WIDE_QUERIES), 0, s, gmax, n_groups, n_q, nq_pad, k, qnorm, dmax_bits,
                           mfma_gamma(dim), tile_norm, sample_stride, thr, cq, glist, list_cap);
    else
        hipLaunchKernelGGL((glist ? threshold_kernel<true, 16, 16> : threshold_kernel<false, 16, 16>), dim3(nq_pad / 16), dim3(256), 0, s, gmax,
                           n_groups, n_q, nq_pad, k, qnorm, dmax_bits, mfma_gamma(dim), tile_norm, sample_stride, thr, cq, glist, list_cap);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_threshold_update(const uint2 *cand, const uint32_t *cnt, int nsub, int nsub_part, int part_blocks, int prev_nsub, int prev_part,
                            int prev_blocks, int qb_per, int sp, int n_q, int nq_pad, const CandLayout &lay, int k, const float *cq,
                            const float *tile_norm, uint32_t *top, bool top_in, bool top_out, float *thr, hipStream_t s, int tile_q) {
    if (nsub_part < nsub) nsub_part = nsub;
    if (prev_part < prev_nsub) prev_part = prev_nsub;
    if (nsub_part > 2048) {
        set_error("threshold_update: %d sub-lists exceed 2048", nsub_part);
        return CCR_ERR_INVALID;
    }
    if (!top) top_in = top_out = false;
    // LDS score buffer: comfortably more than k (the bound tightens with the number of rows seen), 16 KiB at least
    int compact = std::max(4096, 8 * pow2_ceil(k));
    if (compact > 32768) compact = 32768;
    const size_t lds = (size_t)compact * 4;
    if (lds > 48 * 1024) {
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&threshold_update_kernel), 128 * 1024);
        if (rc != CCR_OK) return rc;
    }
    hipLaunchKernelGGL(threshold_update_kernel, dim3(n_q), dim3(256), lds, s, cand, cnt, nsub, nsub_part, part_blocks, prev_nsub, prev_part,
                       prev_blocks, qb_per > 0 ? qb_per : 1, sp, nq_pad, lay, k, compact, cq, tile_norm, top, top_in ? 1 : 0, top_out ? 1 : 0,
                       thr, tile_q > 0 ? tile_q : TILE_Q);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

constexpr size_t SELECT_LDS_BUDGET = 150 * 1024;   // dynamic LDS the select kernel may ask for (160 KiB per CU)

static size_t select_fixed_lds(int dim, int ranges, int rescore_cap) {
    const size_t cnt_bytes = ((size_t)(ranges + 1) * 4 + 15) & ~(size_t)15;
    return (((size_t)dim * 2 + 15) & ~(size_t)15) + 2 * cnt_bytes + (size_t)rescore_cap * 8;
}

// Candidates per query the select kernel can gather into LDS: `want` (the planner's expectation with head room),
// at least 2048 (a smaller area lets more queries share a CU: the re-score is latency-bound, 0.39 -> 0.37 ms at NQ and
// 0.25 -> 0.21 ms on a 1/8 shard against a 4096 floor), never more than the LDS budget allows.
int select_compact_entries(int dim, int ranges, int rescore_cap, int64_t want) {
    const size_t fixed = select_fixed_lds(dim, ranges, rescore_cap);
    const int64_t fit = fixed + 2048 < SELECT_LDS_BUDGET ? (int64_t)((SELECT_LDS_BUDGET - fixed) / 8) : 256;
    return (int)std::min<int64_t>(std::max<int64_t>(want, 2048), fit) / 256 * 256;
}

int launch_partition_flags(const uint32_t *flags, int begin, int n, uint32_t *retry_list, uint32_t *dense_list, uint32_t *counts,
                           hipStream_t s) {
    hipLaunchKernelGGL(partition_flags_kernel, dim3(1), dim3(256), 0, s, flags, begin, n, retry_list, dense_list, counts);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_underfilled_to_retry(uint32_t *flags, int begin, int n, const float *thr_safe, float *thr, hipStream_t s) {
    if (n <= begin) return CCR_OK;
    hipLaunchKernelGGL(underfilled_to_retry_kernel, dim3((n - begin + 255) / 256), dim3(256), 0, s, flags, begin, n, thr_safe, thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_scatter_thresholds(const uint32_t *list, int n, const float *thr2, float *thr, hipStream_t s) {
    if (n <= 0) return CCR_OK;
    hipLaunchKernelGGL(scatter_thresholds_kernel, dim3((n + 255) / 256), dim3(256), 0, s, list, n, thr2, thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_gather_queries(const uint16_t *Q, int dim, const uint32_t *list, int n, const float *thr, const float *delta, uint16_t *Q2,
                          float *thr2, float *delta2, hipStream_t s) {
    if (n <= 0) return CCR_OK;
    hipLaunchKernelGGL(gather_queries_kernel, dim3(n), dim3(256), 0, s, Q, dim, list, n, thr, delta, Q2, thr2, delta2);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_select_rescore(const uint2 *cand, const uint32_t *cnt, int ranges, int sp, int n_q, int nq_pad, const CandLayout &lay, int k,
                          int rescore_cap, int compact, int64_t n_rows, float *thr, const float *cq, const float *tile_norm, const float *row_norm,
                          const uint32_t *dmax_bits, const uint16_t *Q,
                          const uint16_t *D, int dt, int dim, int64_t id_offset, float *out_scores, int64_t *out_ids,
                          uint32_t *flag_count, uint32_t *flag_list, unsigned long long *stat_cand, const uint32_t *out_rows,
                          hipStream_t s, const float *gmax, int sample_tiles, int sample_stride, int gmax_pitch, const uint32_t *glist, int list_cap,
                          int regular_cap) {
    if (regular_cap <= 0 || regular_cap > rescore_cap) regular_cap = rescore_cap;
    const size_t lds = select_fixed_lds(dim, ranges, rescore_cap) + (size_t)compact * 8;
    const bool wide = rescore_cap > 512 || compact > 8192 || ranges > 1024;   // 1024 threads: one re-scored row per thread at large k
    auto go = [&](auto kernel, int threads) -> int {
        if (lds > 48 * 1024) {
            const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), SELECT_LDS_BUDGET + 8192);
            if (rc != CCR_OK) return rc;
        }
        hipLaunchKernelGGL(kernel, dim3(n_q), dim3(threads), lds, s, cand, cnt, ranges, sp, nq_pad, lay, k, rescore_cap, compact,
                           n_rows, thr, cq, tile_norm, row_norm, dmax_bits, Q, D, dim, id_offset, out_scores, out_ids, flag_count, flag_list, stat_cand,
                           out_rows, gmax, sample_tiles, sample_stride, gmax_pitch, glist, list_cap, regular_cap);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    };
    return dispatch_half(dt, [&](auto et) {
        constexpr int ET = decltype(et)::value;
        if (wide) return go(&select_rescore_kernel<ET, 1024>, 1024);
        return go(&select_rescore_kernel<ET, 256>, 256);
    });
}

}  // namespace ccr
