// ccr_embed_train.hip -- the gradient of an embedding table from the gradient of its gathered rows (ccr_embedding_grad): the last piece
// of the embedding block's backward (ccr_embed_layernorm_bwd_half writes d_x, the three tables of BertEmbeddings each take one call).
//
// grad[r] = sum of d_x[row] over the token rows whose clamped id is r.  The caller hands over `order`, the permutation that sorts
// (clamped id, row) ascending, so the rows of one id -- its RUN -- are consecutive in sorted position and ascending in token row.  No
// atomics; the summation order is part of the interface (include/ccr_retrieval.h, restated by ccrec_amd/embed_grad_ref.py): the run is cut
// into chunks of CCR_EMBED_GRAD_CHUNK = 64 consecutive entries, a chunk is summed sequentially from its first entry, the chunk sums
// are added sequentially in order.  Only additions: there is nothing to contract.
//
//   memset                        every row +0 (ids that do not occur keep it)
//   embedding_grad_short_kernel   one wave per sorted position; the wave at a run's first position measures the run (ballots over 64
//                                 positions at a time) and, up to EG_LONG = 256 entries, sums it: a lane owns four columns of every
//                                 256-column slice, the row numbers of a chunk travel by shuffle.
//   embedding_grad_long_kernel    runs above EG_LONG (type 0 holds every token of a batch): such a run covers a sorted position that is
//                                 a multiple of EG_LONG, and the workgroups of the first such position own it -- one per 16 columns, so a
//                                 768-wide table spreads one run over 48 workgroups.  1024 threads = 64 chunk slots x 16 columns: 64 chunks
//                                 are summed side by side, parked in LDS, and added in order by the slot-0 threads (the fixed-order
//                                 second stage), round after round.
#include "ccr_common.h"

namespace ccr {

constexpr int EG_CHUNK = CCR_EMBED_GRAD_CHUNK;
constexpr int EG_LONG = 256;    // the longest run the wave-per-run kernel takes (a multiple of EG_CHUNK)
constexpr int EG_COLS = 16;     // columns per workgroup of the long-run kernel
constexpr int EG_SLOTS = 64;    // chunks it sums side by side
static_assert(EG_CHUNK == 64 && EG_LONG % EG_CHUNK == 0 && EG_COLS * EG_SLOTS == 1024, "embedding_grad layout");

// token row at sorted position k; a value outside [0, T) is clamped (memory safety: `order` is the caller's)
__device__ __forceinline__ int eg_row(const int64_t *__restrict__ order, int64_t k, int64_t T) {
    const int64_t r = order[k];
    return (int)(r < 0 ? 0 : (r >= T ? T - 1 : r));
}
// ... and its table row: the id, clamped as the forward clamps it
__device__ __forceinline__ int64_t eg_key(const int64_t *__restrict__ idx, const int64_t *__restrict__ order, int64_t k, int64_t T,
                                          int64_t n_rows) {
    const int64_t v = idx[eg_row(order, k, T)];
    return v < 0 ? 0 : (v >= n_rows ? n_rows - 1 : v);
}

__global__ __launch_bounds__(256) void embedding_grad_short_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ order,
                                                                  const float *__restrict__ dx, int64_t T, int dim,
                                                                  float *__restrict__ grad, int64_t n_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= T) return;
    const int64_t r = eg_key(idx, order, k, T, n_rows);
    if (k > 0 && eg_key(idx, order, k - 1, T, n_rows) == r) return;   // not the first entry of its run (wave-uniform)
    int len = 0;
    for (;;) {
        const int64_t q = k + len + lane;
        const bool same = q < T && eg_key(idx, order, q, T, n_rows) == r;
        const unsigned long long m = __ballot(same);
        if (m == ~0ull) {
            len += 64;
            if (len > EG_LONG) return;   // the long-run kernel's
            continue;
        }
        len += __builtin_ctzll(~m);
        break;
    }
    if (len > EG_LONG) return;
    const int n4 = dim >> 2;
    for (int base = 0; base < n4; base += 64) {   // (uniform trip count: the shuffles below need every lane)
        const int c4 = base + lane;
        const bool live = c4 < n4;
        const float *src = dx + 4 * (live ? c4 : 0);
        float4 total = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c0 = 0; c0 < len; c0 += EG_CHUNK) {
            const int n = len - c0 < EG_CHUNK ? len - c0 : EG_CHUNK;
            const int mine = lane < n ? eg_row(order, k + c0 + lane, T) : 0;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int e0 = 0; e0 < n; e0 += 8) {   // eight rows in flight, added in order
                float4 x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u < n ? e0 + u : n - 1;
                    x[u] = *reinterpret_cast<const float4 *>(src + (int64_t)__shfl(mine, e) * dim);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (e0 + u == 0) {
                        s = x[u];
                    } else if (e0 + u < n) {
                        s.x += x[u].x, s.y += x[u].y, s.z += x[u].z, s.w += x[u].w;
                    }
                }
            }
            if (c0 == 0) {
                total = s;
            } else {
                total.x += s.x, total.y += s.y, total.z += s.z, total.w += s.w;
            }
        }
        if (live) *reinterpret_cast<float4 *>(grad + r * dim + 4 * c4) = total;
    }
}

__global__ __launch_bounds__(1024) void embedding_grad_long_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ order,
                                                                  const float *__restrict__ dx, int64_t T, int dim,
                                                                  float *__restrict__ grad, int64_t n_rows) {
    __shared__ int64_t s_run[2];
    __shared__ float sh[EG_SLOTS][EG_COLS];
    const int64_t p = (int64_t)blockIdx.x * EG_LONG;   // < T (the grid)
    const int64_t r = eg_key(idx, order, p, T, n_rows);
    if (threadIdx.x == 0) {
        int64_t lo = -1, hi = -1;
        // the run of r reaches back beyond p - EG_LONG: an earlier multiple of EG_LONG owns it
        if (p < EG_LONG || eg_key(idx, order, p - EG_LONG, T, n_rows) != r) {
            int64_t a = p < EG_LONG ? 0 : p - EG_LONG + 1, b = p;
            while (a < b) {   // first position of the run (keys ascend: at or before p, "== r" is ">= r")
                const int64_t m = (a + b) >> 1;
                if (eg_key(idx, order, m, T, n_rows) == r) b = m; else a = m + 1;
            }
            lo = a;
            a = p + 1, b = T;
            while (a < b) {   // first position after it
                const int64_t m = (a + b) >> 1;
                if (eg_key(idx, order, m, T, n_rows) == r) a = m + 1; else b = m;
            }
            hi = a;
        }
        s_run[0] = lo, s_run[1] = hi;
    }
    __syncthreads();
    const int64_t lo = s_run[0], hi = s_run[1];
    if (lo < 0 || hi - lo <= EG_LONG) return;   // (workgroup-uniform) not the owner, or the wave-per-run kernel's
    const int cl = threadIdx.x & (EG_COLS - 1), slot = threadIdx.x >> 4;
    const int col = blockIdx.y * EG_COLS + cl;
    const bool live = col < dim;
    const int64_t n_chunks = (hi - lo + EG_CHUNK - 1) / EG_CHUNK;
    float total = 0.f;
    for (int64_t q0 = 0; q0 < n_chunks; q0 += EG_SLOTS) {
        const int64_t chunk = q0 + slot;
        if (live && chunk < n_chunks) {
            const int64_t b = lo + chunk * EG_CHUNK;
            const int n = hi - b < EG_CHUNK ? (int)(hi - b) : EG_CHUNK;
            float s = dx[(int64_t)eg_row(order, b, T) * dim + col];
#pragma unroll 8
            for (int e = 1; e < n; ++e) s += dx[(int64_t)eg_row(order, b + e, T) * dim + col];
            sh[slot][cl] = s;
        }
        __syncthreads();
        if (live && slot == 0) {
            const int m = n_chunks - q0 < EG_SLOTS ? (int)(n_chunks - q0) : EG_SLOTS;
            int i = 0;
            if (q0 == 0) total = sh[0][cl], i = 1;
            for (; i < m; ++i) total += sh[i][cl];
        }
        __syncthreads();
    }
    if (live && slot == 0) grad[r * dim + col] = total;
}

}  // namespace ccr

using namespace ccr;

extern "C" int ccr_embedding_grad(const int64_t *idx, const int64_t *order, const float *d_x, int64_t T, int dim, float *grad,
                                  int64_t n_rows, void *stream) {
    CCR_REQUIRE(grad && (T == 0 || (idx && order && d_x)), "ccr_embedding_grad: null pointer");
    CCR_REQUIRE(T >= 0 && T <= 0x7fffffffll && n_rows > 0 && dim > 0 && dim % 4 == 0,
                "ccr_embedding_grad: T=%lld n_rows=%lld dim=%d (dim %% 4 == 0, T < 2^31)", (long long)T, (long long)n_rows, dim);
    CCR_REQUIRE(((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(d_x)) & 15) == 0, "ccr_embedding_grad: 16-byte aligned arrays");
    hipStream_t s = (hipStream_t)stream;
    CCR_HIP_CHECK(hipMemsetAsync(grad, 0, (size_t)n_rows * dim * sizeof(float), s));
    if (T == 0) return CCR_OK;
    hipLaunchKernelGGL(embedding_grad_short_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, idx, order, d_x, T, dim, grad, n_rows);
    CCR_LAUNCH_CHECK();
    if (T > EG_LONG) {   // (no run is longer than T)
        hipLaunchKernelGGL(embedding_grad_long_kernel, dim3((unsigned)((T + EG_LONG - 1) / EG_LONG), (unsigned)((dim + EG_COLS - 1) / EG_COLS)),
                           dim3(1024), 0, s, idx, order, d_x, T, dim, grad, n_rows);
        CCR_LAUNCH_CHECK();
    }
    return CCR_OK;
}
