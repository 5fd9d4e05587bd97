// ccr_main_pass.hip -- the GEMM + top-k kernels of the search (stages: ccr_index.h): S^T = D . Q^T on the matrix cores with the
// epilogue of the stage that launches them -- EPI_GMAX (sample pass), EPI_FILTER (main pass, retry pass) or EPI_STORE (score rows of
// the margin path) --, so the [Q, N] score matrix never exists in HBM.
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
#include "ccr_gemm_common.h"
#include "ccr_index.h"

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

// A main pass that leaves CUs to side work counts its workgroups in as they start (a.arrive; null: nobody waits): the gate kernel
// behind ccr_search_stream_wait_main_pass (ccr_api.hip) holds the side work back until all of them are resident.  Once per
// workgroup, in front of the item loop.
__device__ __forceinline__ void announce_arrival(const GemmArgs &a) {
    if (a.arrive != nullptr && threadIdx.x == 0) atomicAdd(a.arrive, 1u);
}

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

    if constexpr (EPI == EPI_FILTER) announce_arrival(a);
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
//   registers: 192 accumulators + 8 corpus fragments (32) + 6 query fragments (24) = 248 -- all six are resident: refilled in place behind
//     the MFMAs, three of them would queue behind the partner's operand reads -- so nothing else may live in registers
//     across the K loop but two lane offsets: the thresholds and margin
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
//          for both groups precedes every mem(u).  Group 0's waves fetch the 16 corpus pieces and rows 0-15 of each 96-row query
//          group, group 1's the query rows 16-95.
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

    announce_arrival(a);
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
            bf16x8 af[8], bfr[WIDE_QT];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) af[dt] = *reinterpret_cast<const bf16x8 *>(abuf + a_base + dt * 1024);
#pragma unroll
            for (int qt = 0; qt < WIDE_QT; ++qt) bfr[qt] = *reinterpret_cast<const bf16x8 *>(bbuf + b_base + qt * 1024);
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
                for (int qt = 0; qt < WIDE_QT; ++qt)
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt) acc[dt][qt] = mfma_16x16x32<ET>(af[dt], bfr[qt], z);
            } else {
#pragma unroll
                for (int qt = 0; qt < WIDE_QT; ++qt)
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt) acc[dt][qt] = mfma_16x16x32<ET>(af[dt], bfr[qt], acc[dt][qt]);
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
            CCR_WAIT_LGKM0();   // group 1's filter has issued LDS reads and counter stores: retired before the barrier
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

// The gate of ccr_search_stream_wait_main_pass: one wave that returns when `want` workgroups of the main pass have counted themselves
// in (announce_arrival) -- or after GATE_MAX_POLLS polls, or GATE_MAX_TICKS of the 100-MHz wall clock (300 us), whichever comes
// first.  It can delay the side work behind it; it can never hang it.
constexpr int GATE_MAX_POLLS = 1024;
constexpr long long GATE_MAX_TICKS = 30000;
__global__ __launch_bounds__(64) void main_pass_gate_kernel(const uint32_t *arrive, uint32_t want) {
    const long long t0 = wall_clock64();
    for (int i = 0; i < GATE_MAX_POLLS; ++i) {
        if (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return;
        if (wall_clock64() - t0 > GATE_MAX_TICKS) return;
        __builtin_amdgcn_s_sleep(64);
    }
}

int launch_main_pass_gate(const uint32_t *arrive, uint32_t want, hipStream_t s) {
    hipLaunchKernelGGL(main_pass_gate_kernel, dim3(1), dim3(64), 0, s, arrive, want);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_gemm(const GemmArgs &a, int dt, MainKernel kind, int epi, int grid, hipStream_t s) {
    return dispatch_half(dt, [&](auto et) { return launch_gemm_of<decltype(et)::value>(a, kind, epi, grid, s); });
}

}  // namespace ccr
