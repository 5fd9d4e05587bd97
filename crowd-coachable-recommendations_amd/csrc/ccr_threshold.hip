// ccr_threshold.hip -- the threshold stage of the search (stages: ccr_index.h) and the bounds it is built from:
//   row_norms_kernel / tile_norms_kernel / max_tile_norm_kernel   the norm bounds of the error margins: the index's row and tile norms
//                              at its creation, the query norms at the head of every search.  (They are here, not beside
//                              index_create_impl: ccr_api.hip holds no kernel, and every reader of these bounds but the select is below.)
//   threshold_kernel           tau_q = k-th largest group maximum of the sample pass (a lower bound of the k-th largest score: k
//                              disjoint groups hold a score >= tau_q), minus the MFMA error margins (cq * tile norm);
//                              an ESTIMATED tau_q takes its rank among at most tile_cap groups of each sampled tile (tile_top_mask)
//   threshold_small_kernel     the same for a small batch, a workgroup per query
//   threshold_update_kernel    the re-tightening between two phases of the main pass and in front of a retry, from the candidates
#include <algorithm>

#include "ccr_gemm_common.h"
#include "ccr_index.h"
#include "ccr_topk_device.h"

namespace ccr {

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

// The tile cap of estimated thresholds (ccr_plan.hip, optimistic_rank): of the 16 orderable lower bounds o[] of ONE sampled tile and
// query, bit j of the result says that group j is among the `cap` largest -- fewer than `cap` of the others rank before it, and on
// equal values the lower group index ranks first, so the answer is a function of the values alone.  From registers: one compare per
// pair (i < j) and one counter per group -- before[j] starts at the 15 - j pairs with the groups after j, as if j lost them all; a
// pair that i wins takes one off before[i] and puts one on before[j].
__device__ __forceinline__ uint32_t tile_top_mask(const uint32_t (&o)[GROUPS_PER_TILE], int cap) {
    int before[GROUPS_PER_TILE];
#pragma unroll
    for (int j = 0; j < GROUPS_PER_TILE; ++j) before[j] = GROUPS_PER_TILE - 1 - j;
#pragma unroll
    for (int i = 0; i < GROUPS_PER_TILE; ++i)
#pragma unroll
        for (int j = i + 1; j < GROUPS_PER_TILE; ++j) {
            const int first = o[i] >= o[j] ? 1 : 0;   // i ranks before j
            before[j] += first;
            before[i] -= first;
        }
    uint32_t in = 0u;
#pragma unroll
    for (int j = 0; j < GROUPS_PER_TILE; ++j) in |= (before[j] < cap ? 1u : 0u) << j;
    return in;
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
// large sample 64 phases (16 waves per workgroup) instead of 16.  A batch is the 16 groups of ONE sampled tile (the phases stride
// over the tiles; n_groups is whole tiles), so that a thread holds a tile's lower bounds together.  The histogram counts do not
// depend on the order of the adds: every form computes the same thresholds bit for bit and the same short list as a set.
// tile_cap < 16 (estimated thresholds): only the groups among the tile_cap largest of their tile (tile_top_mask) enter the histograms
// -- the same decision in every radix pass, it is a function of the tile's values alone.  The short list keeps every group.
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
                                                           int k, int tile_cap, const float *__restrict__ qnorm,
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
    // norm bound of the t-th sampled tile (plain vector loads: staging them in LDS, or scalar loads of the wave-uniform
    // index, both made this kernel slower -- 84 vs 70 us at NQ: they share lgkmcnt with the histogram's LDS atomics)
    auto tile_of = [&](int64_t t) { return tile_norm[t * sample_stride]; };
    const int64_t n_tiles = n_groups / GROUPS_PER_TILE;
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
        for (int64_t t = ph; t < n_tiles; t += PH) {   // 16 independent loads in flight per thread (the loop is latency-bound)
            const int64_t g0 = t * GROUPS_PER_TILE;
            float v[GROUPS_PER_TILE];
            uint32_t o[GROUPS_PER_TILE];
#pragma unroll
            for (int j = 0; j < GROUPS_PER_TILE; ++j) v[j] = gmax[(g0 + j) * nq_pad + q];
            const float tn = tile_of(t);
            if (listing) {   // (before the lower bounds exist: the last pass holds the maxima no longer than this)
#pragma unroll
                for (int j = 0; j < GROUPS_PER_TILE; ++j) emit(g0 + j, v[j], tn, prefix);
            }
#pragma unroll
            for (int j = 0; j < GROUPS_PER_TILE; ++j) o[j] = f32_orderable(fmaf(-c, tn, v[j]));
            const uint32_t in = tile_cap < GROUPS_PER_TILE ? tile_top_mask(o, tile_cap) : 0xffffu;
#pragma unroll
            for (int j = 0; j < GROUPS_PER_TILE; ++j)
                if (((in >> j) & 1u) && (o[j] & mask) == prefix) atomicAdd(&s_hist[ql][(o[j] >> shift) & 255u], 1u);
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

// The same thresholds for a SMALL batch (the streaming main pass, n_q <= 128): threshold_kernel gives a query 16 threads, which walk its
// ~4 000 sampled lower bounds four times from global memory -- 70 us for ONE query, a tenth of the whole search.  Here a workgroup
// per query: the lower bounds are staged in LDS once (every load independent, one round trip), the four radix passes read LDS.
// tile_cap < 16: the same in-tile rule as threshold_kernel, applied while staging.
// zero_cnt (may be null): the streaming pass's sub-list counters of this query are cleared here instead of by a memset node.
// grid = n_q, block = 256, dyn LDS = n_groups * 4 bytes.
__global__ __launch_bounds__(256) void threshold_small_kernel(const float *__restrict__ gmax, int n_groups, int nq_pad, int k, int tile_cap,
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
    if (tile_cap < GROUPS_PER_TILE) {
        // the tile cap (threshold_kernel): a thread stages a whole sampled tile, and a group outside its tile's tile_cap largest is
        // staged as 0, below every real value -- it stays in the count and out of the rank (the planner leaves k groups eligible)
        for (int t = tid; t < n_groups / GROUPS_PER_TILE; t += 256) {
            const float tn = tile_norm[(int64_t)t * sample_stride];
            uint32_t o[GROUPS_PER_TILE];
#pragma unroll
            for (int j = 0; j < GROUPS_PER_TILE; ++j) o[j] = f32_orderable(fmaf(-c, tn, gmax[(int64_t)(t * GROUPS_PER_TILE + j) * nq_pad + q]));
            const uint32_t in = tile_top_mask(o, tile_cap);
#pragma unroll
            for (int j = 0; j < GROUPS_PER_TILE; ++j) s_low[t * GROUPS_PER_TILE + j] = ((in >> j) & 1u) ? o[j] : 0u;
        }
    } else {
        for (int g = tid; g < n_groups; g += 256)
            s_low[g] = f32_orderable(fmaf(-c, tile_norm[(int64_t)(g / GROUPS_PER_TILE) * sample_stride], gmax[(int64_t)g * nq_pad + q]));
    }
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

int launch_threshold(const ThresholdArgs &a, hipStream_t s, int *phases_used) {
    if (phases_used) *phases_used = 0;
    if (a.n_groups % GROUPS_PER_TILE || a.tile_cap < 1) {   // every form walks whole sampled tiles
        set_error("threshold: %lld groups are not whole tiles, or tile cap %d", (long long)a.n_groups, a.tile_cap);
        return CCR_ERR_INVALID;
    }
    // a capped selection needs its rank among the capped groups: the small-batch kernel stages a left-out group as 0, which is no
    // threshold (the planner's tile_cap_for sees to this; other callers of this launcher are held to it here)
    if (a.tile_cap < GROUPS_PER_TILE && (int64_t)a.tile_cap * (a.n_groups / GROUPS_PER_TILE) < a.k) {
        set_error("threshold: rank %d above the %d x %lld groups the tile cap leaves", a.k, a.tile_cap, (long long)(a.n_groups / GROUPS_PER_TILE));
        return CCR_ERR_INVALID;
    }
    // small batches: a workgroup per query (needs k <= n_groups -- the planner samples >= 2k groups -- and the bounds in 64 KiB of LDS);
    // its kernel clears the caller's counters itself
    if (a.n_q <= 128 && a.n_groups >= a.k && a.n_groups <= 16384 && a.zero_per_query <= 256) {
        if (a.n_groups * 4 > 32 * 1024) {   // (the kernel's static LDS sits on top of the dynamic part: opt in with head room)
            const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&threshold_small_kernel), 72 * 1024);
            if (rc != CCR_OK) return rc;
        }
        hipLaunchKernelGGL(threshold_small_kernel, dim3(a.n_q), dim3(256), (size_t)a.n_groups * 4, s, a.gmax, (int)a.n_groups, a.nq_pad, a.k,
                           a.tile_cap, a.qnorm, a.dmax_bits, mfma_gamma(a.dim), a.tile_norm, a.sample_stride, a.thr, a.cq, a.zero_cnt, a.zero_per_query,
                           a.glist, a.list_cap);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    }
    if (a.zero_cnt) CCR_HIP_CHECK(hipMemsetAsync(a.zero_cnt, 0, (size_t)a.n_q * a.zero_per_query * 4, s));
    // The wide form (THR_WIDE_QUERIES x 64 phases) wherever every phase still walks at least THR_WIDE_MIN_BATCHES full batches of 16
    // loads per radix pass, n_groups >= 2 x 16 x 64 = 2 048: below that a 64-phase pass is mostly its remainder loop and its barriers
    // across 16 waves, and the 16-phase chain it would shorten is only a few batches long.  `phases` (16 / 64, CCR_THR_PHASES) pins the form.
    const bool wide = a.phases == 64 || (a.phases != 16 && a.n_groups >= (int64_t)THR_WIDE_MIN_BATCHES * 16 * 64);
    if (phases_used) *phases_used = wide ? 64 : 16;
    const auto kernel = wide ? (a.glist ? threshold_kernel<true, 64, THR_WIDE_QUERIES> : threshold_kernel<false, 64, THR_WIDE_QUERIES>)
                             : (a.glist ? threshold_kernel<true, 16, 16> : threshold_kernel<false, 16, 16>);
    const int qb = wide ? THR_WIDE_QUERIES : 16, ph = wide ? 64 : 16;   // queries and group phases of a workgroup
    hipLaunchKernelGGL(kernel, dim3(a.nq_pad / qb), dim3(qb * ph), 0, s, a.gmax, a.n_groups, a.n_q, a.nq_pad, a.k, a.tile_cap, a.qnorm, a.dmax_bits,
                       mfma_gamma(a.dim), a.tile_norm, a.sample_stride, a.thr, a.cq, a.glist, a.list_cap);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
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

int launch_threshold_update(const ThresholdUpdateArgs &a, hipStream_t s) {
    const int nsub_part = std::max(a.nsub_part, a.nsub), prev_part = std::max(a.prev_part, a.prev_nsub);
    if (nsub_part > 2048) {
        set_error("threshold_update: %d sub-lists exceed 2048", nsub_part);
        return CCR_ERR_INVALID;
    }
    // LDS score buffer: comfortably more than k (the bound tightens with the number of rows seen), 16 KiB at least
    int compact = std::max(4096, 8 * pow2_ceil(a.k));
    if (compact > 32768) compact = 32768;
    const size_t lds = (size_t)compact * 4;
    if (lds > 48 * 1024) {
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&threshold_update_kernel), 128 * 1024);
        if (rc != CCR_OK) return rc;
    }
    hipLaunchKernelGGL(threshold_update_kernel, dim3(a.n_q), dim3(256), lds, s, a.cand, a.cnt, a.nsub, nsub_part, a.part_blocks, a.prev_nsub,
                       prev_part, a.prev_blocks, a.qb_per > 0 ? a.qb_per : 1, a.sp, a.nq_pad, a.lay, a.k, compact, a.cq, a.tile_norm, a.top,
                       a.top && a.top_in ? 1 : 0, a.top && a.top_out ? 1 : 0, a.thr, a.tile_q > 0 ? a.tile_q : TILE_Q);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

}  // namespace ccr
