// ccr_rank_f32.hip -- the fp32 ranking on top of a 16-bit search (library version 111):
//   keep_f32_kernel      beside a packed shard, keep the fp32 rows y the pack rounded (zero-padded to the packed width) and a bound of
//                        every row's rounding residual ||y - unpack(h)||
//   rescore_f32_kernel   per query: re-score the first n_cand rows of the 16-bit search on the fp32 rows (fp64 ordered), sort them by
//                        (score desc, id asc), write the top k, and decide by ONE inequality whether a row outside the list could
//                        belong to the fp32 top-k (flag 0: it cannot)
// ccrec_amd/rank_f32_ref.py restates both on the CPU, bit for bit.
#include "ccr_index.h"
#include "ccr_topk_device.h"

namespace ccr {

// (double) v rounded UP to fp32: the conversion rounds to nearest, one step up where that fell below v (v >= 0; inf and NaN pass through)
__device__ __forceinline__ float f32_round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

// ---------------------------------------------------------------- keep: the fp32 rows beside their packed rows
// One wave per row, like pack_rows_kernel.  VEC (dim % 8 == 0, so dim == pdim and every row is 16-byte aligned): float4 loads and
// stores and the pack's own wave_sumsq; otherwise element-wise accesses and the same sum in the same order (element i belongs to
// chunk i / 4 of lane (i / 4) % 64 -- pack_rows_padded_kernel's loop).  y_i = x_i, or (float)((double) x_i / max(sqrt(ss), 1e-12)):
// the value the pack rounded.  Residual: fp64 sum of (y_i - h_i)^2 (lane partials, butterfly), sqrt, inflated by 2^-20 for the
// summation's own rounding (dim <= 2^16 terms of relative error 2^-52 each), rounded up to fp32.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void keep_f32_kernel(const float *__restrict__ src, const uint16_t *__restrict__ half_rows, int normalize,
                                                      float *__restrict__ dst, float *__restrict__ res_bounds, int64_t rows, int dim,
                                                      int pdim) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int nchunk = pdim >> 2;
    for (int64_t r = wave; r < rows; r += nwaves) {
        const float *x = src + r * dim;
        const uint16_t *h = half_rows + r * pdim;
        float *y = dst + r * pdim;
        double den = 1.0;
        if (normalize) {
            double ss;
            if constexpr (VEC) {
                ss = wave_sumsq(x, dim, lane);
            } else {
                double p = 0.0;
                for (int c = lane; c < nchunk; c += 64) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = 4 * c + e;
                        const double v = i < dim ? (double)x[i] : 0.0;
                        p = p + v * v;
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
                ss = p;
            }
            const double nrm = sqrt(ss);
            den = nrm > 1e-12 ? nrm : 1e-12;
        }
        double res = 0.0;
        for (int c = lane; c < nchunk; c += 64) {
            float v[4];
            uint16_t hb[4];
            if constexpr (VEC) {
                const float4 xv = reinterpret_cast<const float4 *>(x)[c];
                const uint2 hv = reinterpret_cast<const uint2 *>(h)[c];
                v[0] = xv.x, v[1] = xv.y, v[2] = xv.z, v[3] = xv.w;
                hb[0] = (uint16_t)hv.x, hb[1] = (uint16_t)(hv.x >> 16), hb[2] = (uint16_t)hv.y, hb[3] = (uint16_t)(hv.y >> 16);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * c + e;
                    v[e] = i < dim ? x[i] : 0.f;
                    hb[e] = h[i];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (normalize && 4 * c + e < dim) v[e] = (float)((double)v[e] / den);
                const double diff = (double)v[e] - (double)elem_to_f32<DT>(hb[e]);
                res = fma(diff, diff, res);
            }
            if constexpr (VEC) {
                reinterpret_cast<float4 *>(y)[c] = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[4 * c + e] = v[e];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) res = res + __shfl_xor(res, off, 64);
        if (lane == 0) res_bounds[r] = f32_round_up(sqrt(res) * (1.0 + 0x1p-20));
    }
}

// ---------------------------------------------------------------- re-score on the fp32 rows + verification
constexpr int RESCORE_THREADS = 256;   // candidates of one chunk: one fp64 chain per thread
constexpr int RESCORE_SB = 128;        // bytes of a row staged per K slice (whole 128-byte segments)
constexpr int RESCORE_STRIDE = RESCORE_SB + 16;   // +16: consecutive rows start 4 banks apart (conflict-free b128 reads)
constexpr int RESCORE_MAX_PDIM = 4096;   // the widest row an index takes

// keys sorted per query: a power of two, at least 2 (the row slices behind them stay 16-byte aligned)
__host__ __device__ __forceinline__ int rescore_keys(int n_cand) { return n_cand < 2 ? 2 : pow2_ceil(n_cand); }

static size_t rescore_lds_bytes(int pdim, int n_cand) {
    return (size_t)pdim * 4 + (size_t)rescore_keys(n_cand) * 8 + (size_t)RESCORE_THREADS * RESCORE_STRIDE + 16;
}

// grid = n_q, block = RESCORE_THREADS.  dyn LDS: [pdim fp32 query row][rescore_keys(n_cand) u64 keys][RESCORE_THREADS x 144-byte row slices][flag]
// The candidates are walked in chunks of RESCORE_THREADS rows.  Inside a chunk the rows go through the LDS in K slices of 128 bytes, as in
// select_rescore_kernel: 8 adjacent lanes fetch one row's slice (a whole 128-byte segment, every load of the slice in flight), the pieces
// of slice s + 1 are loaded into registers while slice s is consumed, and every thread runs the fp64 chain of its own row over the slice
// from the LDS.  A row is pdim * 4 bytes (3 KiB at 768: twice the 16-bit row), so a chunk never holds more than its current slice.
// Element order inside a row is unchanged: s32(q, j) = (float) sum_i ascending fma((double) y_q[i], (double) y_j[i], acc).
__global__ __launch_bounds__(RESCORE_THREADS) void rescore_f32_kernel(
    const float *__restrict__ Q, const float *__restrict__ D, int64_t n_rows, int pdim, const int64_t *__restrict__ cand_ids,
    const float *__restrict__ cand_s16, int n_cand, int k, int64_t id_offset, const float *__restrict__ q_norm_bounds,
    const float *__restrict__ q_res_bounds, const float *__restrict__ corpus_max, float *__restrict__ out_scores,
    int64_t *__restrict__ out_ids, int32_t *__restrict__ flags, float *__restrict__ diag) {
    constexpr int THREADS = RESCORE_THREADS, SB = RESCORE_SB, stride = RESCORE_STRIDE, lpr = SB / 16;
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int np2 = rescore_keys(n_cand);
    float *s_q = reinterpret_cast<float *>(sm);
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(sm + (size_t)pdim * 4);
    char *stage = reinterpret_cast<char *>(s_keys + np2);
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int64_t *ids = cand_ids + (int64_t)q * n_cand;
    const float *s16 = cand_s16 + (int64_t)q * n_cand;
    for (int c = tid; c < pdim / 4; c += THREADS) reinterpret_cast<float4 *>(s_q)[c] = reinterpret_cast<const float4 *>(Q + (int64_t)q * pdim)[c];

    const int row_bytes = pdim * 4;
    const char *Dbytes = reinterpret_cast<const char *>(D);
    const int col = (tid % lpr) * 16;           // byte column of this thread's pieces inside a slice
    // address column: a column past the row end (pdim = 8 under a 128-byte slice) reads column 0 -- the last corpus row may end exactly
    // at the end of the caller's allocation
    const int acol = col < row_bytes ? col : 0;
    // a candidate id outside the shard: its row is not read (row 0 stands in) and the query is reported unverified
    int *s_bad = reinterpret_cast<int *>(stage + THREADS * stride);
    if (tid == 0) *s_bad = 0;
    // Eight named pieces, not arrays: hipcc leaves a uint4[8] whose loads and stores sit in different loops in scratch memory.
#define CCR_PIECES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
    for (int base = 0; base < n_cand; base += THREADS) {
        const int nc = min(THREADS, n_cand - base);
        __syncthreads();   // (first pass: s_bad is initialised before anybody sets it)
        // piece j of this thread belongs to candidate base + (tid + j * THREADS) / lpr; every piece is loaded unconditionally (an unused
        // slot reads row 0) so that the prefetched values stay in registers; only the store into the LDS is conditional
#define CCR_DECL(j)                                                       \
    const int cj##j = (tid + j * THREADS) / lpr;                          \
    int64_t row##j = cj##j < nc ? ids[base + cj##j] - id_offset : 0;      \
    if (row##j < 0 || row##j >= n_rows) {                                 \
        row##j = 0;                                                       \
        *s_bad = 1;                                                       \
    }                                                                     \
    const char *src##j = Dbytes + row##j * row_bytes + acol;              \
    uint4 pre##j = *reinterpret_cast<const uint4 *>(src##j);
        CCR_PIECES(CCR_DECL)
#undef CCR_DECL
        double acc = 0.0;
        for (int k0 = 0; k0 < row_bytes; k0 += SB) {
            __syncthreads();                        // the previous slice has been consumed (first pass: the query row is staged)
            const bool col_in = k0 + col < row_bytes;
#define CCR_PUT(j) \
    if (col_in && cj##j < nc) *reinterpret_cast<uint4 *>(stage + cj##j * stride + col) = pre##j;
            CCR_PIECES(CCR_PUT)
#undef CCR_PUT
            __syncthreads();
            {   // next slice: in flight during the fp64 chains below
                const int kn = (k0 + SB + col < row_bytes) ? k0 + SB : -acol;
#define CCR_GET(j) pre##j = *reinterpret_cast<const uint4 *>(src##j + kn);
                CCR_PIECES(CCR_GET)
#undef CCR_GET
            }
            if (tid < nc) {
                double a = acc;
                for (int c = 0; c < lpr && k0 + c * 16 < row_bytes; ++c) {
                    const float4 dv = *reinterpret_cast<const float4 *>(stage + (size_t)tid * stride + c * 16);
                    const float4 qv = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(s_q) + k0 + c * 16);
                    a = fma((double)qv.x, (double)dv.x, a);
                    a = fma((double)qv.y, (double)dv.y, a);
                    a = fma((double)qv.z, (double)dv.z, a);
                    a = fma((double)qv.w, (double)dv.w, a);
                }
                acc = a;
            }
        }
        if (tid < nc) {
            int64_t row = ids[base + tid] - id_offset;
            if (row < 0 || row >= n_rows) row = 0;
            // a blocked row keeps its -1e6 (it stays in the ranking, as in every search path)
            s_keys[base + tid] = make_key(s16[base + tid] == -1e6f ? -1e6f : (float)acc, (uint32_t)row);
        }
    }
#undef CCR_PIECES
    for (int i = n_cand + tid; i < np2; i += THREADS) s_keys[i] = 0ull;   // below every real key
    __syncthreads();
    const int any_bad = *s_bad;
    block_bitonic_sort_desc(s_keys, np2);
    for (int i = tid; i < k; i += THREADS) {
        const unsigned long long key = s_keys[i];
        out_scores[(int64_t)q * k + i] = key_score(key);
        out_ids[(int64_t)q * k + i] = id_offset + (int64_t)key_idx(key);
    }
    if (tid == 0) {
        // verified <=> every row was fetched, or a blocked row was fetched (then every unblocked row was), or
        //              (double) cut + E + slack < (double) tau          (rank_f32_ref.verified: the same fp64 steps, none contracted)
        const float tau = key_score(s_keys[k - 1]);
        const float cut = s16[n_cand - 1];
        const double A = (double)q_norm_bounds[q], r = (double)q_res_bounds[q];
        const double Rmax = (double)corpus_max[0], Nmax = (double)corpus_max[1];
        const double E = __dadd_rn(__dmul_rn(A, Rmax), __dmul_rn(r, Nmax));
        const double slack = __dadd_rn(__dmul_rn(0x1p-21, __dadd_rn(fabs((double)cut), fabs((double)tau))),
                                       __dmul_rn(0x1p-40, __dmul_rn(A, __dadd_rn(Nmax, Rmax))));
        const bool ok = (int64_t)n_cand == n_rows || cut == -1e6f || __dadd_rn(__dadd_rn((double)cut, E), slack) < (double)tau;
        flags[q] = (ok && !any_bad) ? 0 : 1;
        if (diag) {
            diag[4 * q + 0] = tau;
            diag[4 * q + 1] = cut;
            diag[4 * q + 2] = (float)E;
            diag[4 * q + 3] = (float)slack;
        }
    }
}

}  // namespace ccr

using namespace ccr;

extern "C" int ccr_keep_f32(const float *src, const uint16_t *half_rows, int half_dtype, int normalize, float *dst_f32, float *res_bounds,
                            int64_t rows, int dim, void *stream) {
    if (const int rc = check_half("ccr_keep_f32", half_dtype)) return rc;
    CCR_REQUIRE(src && half_rows && dst_f32 && res_bounds, "ccr_keep_f32: null pointer");
    CCR_REQUIRE(rows >= 0 && dim > 0 && dim <= 65536, "ccr_keep_f32: bad shape rows=%lld dim=%d", (long long)rows, dim);
    if (rows == 0) return CCR_OK;
    const int pdim = (dim + 7) / 8 * 8;
    const bool vec = pdim == dim;
    CCR_REQUIRE(!vec || (((uintptr_t)src | (uintptr_t)dst_f32) % 16 == 0 && (uintptr_t)half_rows % 8 == 0),
                "ccr_keep_f32: buffers must be 16-byte aligned");
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 65536) blocks = 65536;   // (as the normalising pack: short-lived waves of a few rows each)
    return dispatch_half(half_dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (vec)
            hipLaunchKernelGGL((keep_f32_kernel<DT, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, half_rows, normalize,
                               dst_f32, res_bounds, rows, dim, pdim);
        else
            hipLaunchKernelGGL((keep_f32_kernel<DT, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, half_rows, normalize,
                               dst_f32, res_bounds, rows, dim, pdim);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    });
}

static int rescore_check_shape(int n_q, int n_cand, int k, int pdim) {
    CCR_REQUIRE(n_q >= 0 && n_cand >= 1 && n_cand <= MAX_K && k >= 1 && k <= n_cand,
                "ccr_rescore_f32: bad shape n_q=%d n_cand=%d k=%d (1 <= k <= n_cand <= %d)", n_q, n_cand, k, MAX_K);
    CCR_REQUIRE(pdim >= 8 && pdim % 8 == 0 && pdim <= RESCORE_MAX_PDIM, "ccr_rescore_f32: pdim=%d (a multiple of 8, <= %d)", pdim,
                RESCORE_MAX_PDIM);
    return CCR_OK;
}

extern "C" size_t ccr_rescore_f32_workspace_bytes(int n_q, int n_cand, int k, int pdim) {
    if (rescore_check_shape(n_q, n_cand, k, pdim) != CCR_OK) return 0;
    return (size_t)(n_q > 0 ? n_q : 1) * 16;   // {tau, cut, E, slack} per query
}

extern "C" int ccr_rescore_f32(const float *queries_f32, const float *corpus_f32, int64_t n_rows, int pdim, const int64_t *cand_ids,
                               const float *cand_s16, int n_q, int n_cand, int k, int64_t id_offset, const float *q_norm_bounds,
                               const float *q_res_bounds, const float *corpus_max, float *out_scores, int64_t *out_ids, int32_t *flags,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = rescore_check_shape(n_q, n_cand, k, pdim)) return rc;
    CCR_REQUIRE(n_rows >= n_cand, "ccr_rescore_f32: n_cand=%d exceeds the shard's %lld rows", n_cand, (long long)n_rows);
    if (n_q == 0) return CCR_OK;
    CCR_REQUIRE(queries_f32 && corpus_f32 && cand_ids && cand_s16 && q_norm_bounds && q_res_bounds && corpus_max && out_scores && out_ids &&
                    flags && workspace,
                "ccr_rescore_f32: null pointer");
    CCR_REQUIRE(((uintptr_t)queries_f32 | (uintptr_t)corpus_f32 | (uintptr_t)workspace) % 16 == 0, "ccr_rescore_f32: buffers must be 16-byte aligned");
    if (workspace_bytes < ccr_rescore_f32_workspace_bytes(n_q, n_cand, k, pdim)) {
        set_error("ccr_rescore_f32: workspace of %zu bytes, %zu needed", workspace_bytes, ccr_rescore_f32_workspace_bytes(n_q, n_cand, k, pdim));
        return CCR_ERR_WORKSPACE;
    }
    const size_t lds = rescore_lds_bytes(pdim, n_cand);   // <= 16 KiB + 32 KiB + 36 KiB
    if (lds > 48 * 1024) {
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&rescore_f32_kernel), rescore_lds_bytes(RESCORE_MAX_PDIM, MAX_K));
        if (rc != CCR_OK) return rc;
    }
    hipLaunchKernelGGL(rescore_f32_kernel, dim3(n_q), dim3(RESCORE_THREADS), lds, (hipStream_t)stream, queries_f32, corpus_f32, n_rows, pdim,
                       cand_ids, cand_s16, n_cand, k, id_offset, q_norm_bounds, q_res_bounds, corpus_max, out_scores, out_ids, flags,
                       reinterpret_cast<float *>(workspace));
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}
