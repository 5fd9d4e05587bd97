// ccr_bpr.hip -- the "bpr" objective of _BertBPR.training_and_validation_step (src/ccrec/models/bbpr.py:153-185).
//
// (a) bpr_sample_kernel: negatives from softmax(f(prior) + log proposal) (bbpr.py:160-179) without the dense [B][n_items] matrix.
//     With t = f(prior value) on the row's m stored entries (c_1 < ... < c_m) and t0 = f(0) everywhere else, in fp64
//       M = max(t0, max t_k),  e0 = exp(t0 - M),  e_k = exp(t_k - M)
//       F(j) = e0 cdf[j] + sum_{k: c_k <= j} proposal[c_k] (e_k - e0),   Z = F(n_items - 1)
//     is the running sum of the softmax's numerators (cdf = inclusive prefix sums of the proposal), and a draw is the smallest j
//     with F(j) > u Z.  One wave per batch row: the m corrections' prefix sums S_k and F(c_k) go to LDS once, each lane then takes
//     draws: a binary search over F(c_k) in LDS names the segment between two entries, a second one over cdf inside it the item.
//     A draw that rounding put on an item of weight exactly 0 steps to the nearest live item (the reference never returns such an item).
//     ptr = NULL is the no-prior branch (bbpr.py:176-179): F = cdf.
// (b) bpr_frozen_*: the frozen-tower step (all_cls cached, only the LayerNorm trains, bbpr.py:436-438): gather -> LayerNorm ->
//     products -> logsigmoid -> weighted sum (bbpr.py:144-147, 180-185) in ONE pass over the gathered rows.  With
//     xh = (x - mean) rstd,  e = xh gamma + beta:
//       D_nb = e_i . e_j - e_i . e_nb = sum_d q_d (xh_j - xh_nb)_d,   q = e_i gamma
//       loss = sum_nb w_b softplus(-D_nb) / (n_neg sum_b w_b)
//     and, with g_nb = -w_b sigmoid(-D_nb), G_b = sum_n g_nb, C_b = sum_n g_nb xh_nb, R_b = G_b xh_j - C_b:
//       dgamma = sum_b R_b (2 xh_i gamma + beta),   dbeta = sum_b R_b gamma        (times grad_out / (n_neg sum w))
//     so the backward keeps ONE accumulator row per batch row and recomputes the LayerNorms (nothing is saved by the forward).
//     One wave per batch row, lane l owns the 16-byte chunks l, l + 64, ... of a row (every load instruction reads 1 KiB of one
//     row), the next row's loads are issued before the current row's reductions.  D_nb is ONE sum over q (xh_j - xh_nb), its
//     products explicit fmaf: a negative that is the positive's row gives exactly 0, and no two large products cancel.
//     No MFMA: 2 + n_neg rows of `dim` floats are read for n_neg dim-length dot products.
// Deterministic: no atomics, every sum has one fixed order.  No read-back: a pointer outside [0, n_rows) makes the loss and both
// gradients NaN; every address is formed from clamped indices.
#include <algorithm>

#include "ccr_loss_common.h"

namespace ccr {
namespace bpr {

constexpr int MAX_ROW_NNZ = 4096;   // entries of one prior row (the limit of ccr_search_sparse_prior)
constexpr int MAX_DIM = 2048, MAX_B = 1 << 20, MAX_NEG = 4096;
constexpr int MAX_BWD_BLOCKS = 512;    // partial gradient rows of the backward (4 waves each: 2 048 waves, what the chip holds at width 768)

// ---- (a) sampler -------------------------------------------------------------------------------------------------------------
// grid = B, block = one wave, dynamic LDS = 2 * max_row_nnz doubles: S_k (inclusive prefix of the corrections) and F(c_k).
__global__ __launch_bounds__(64) void bpr_sample_kernel(const int64_t *__restrict__ users, int B, int n_neg, int64_t n_users,
                                                       const int64_t *__restrict__ ptr, const int64_t *__restrict__ idx,
                                                       const float *__restrict__ t, double t0, const float *__restrict__ proposal,
                                                       const double *__restrict__ cdf, int n_items, const double *__restrict__ uniforms,
                                                       int max_row_nnz, int64_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double s_bpr[];
    double *s_S = s_bpr, *s_F = s_bpr + max_row_nnz;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int64_t u = users[b];
    int64_t p0 = 0;
    int m = 0;
    bool bad = false;   // a user outside the prior, a row longer than the caller said: every draw of the row is -1
    if (ptr) {
        bad = u < 0 || u >= n_users;
        if (!bad) {
            p0 = ptr[u];
            const int64_t len = ptr[u + 1] - p0;
            bad = len < 0 || len > max_row_nnz;
            m = bad ? 0 : (int)len;
        }
    }
    auto column = [&](int k) { return (int)min(max(idx[p0 + k], (int64_t)0), (int64_t)n_items - 1); };   // (clamped: an address)
    double M = t0;
    for (int k = lane; k < m; k += 64) M = fmax(M, (double)t[p0 + k]);
    M = wave_max(M);
    const double e0 = exp(t0 - M);
    double carry = 0.0;
    for (int k0 = 0; k0 < m; k0 += 64) {   // (uniform trip count: every lane takes part in the scan)
        const int k = k0 + lane;
        int c = 0;
        double v = 0.0;
        if (k < m) {
            c = column(k);
            v = (double)proposal[c] * (exp((double)t[p0 + k] - M) - e0);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(v, off, 64);
            if (lane >= off) v += o;
        }
        v += carry;
        if (k < m) s_S[k] = v, s_F[k] = fma(e0, cdf[c], v);
        carry = __shfl(v, 63, 64);
    }
    __syncthreads();
    const double S_m = m ? s_S[m - 1] : 0.0;
    const double Z = fma(e0, cdf[n_items - 1], S_m);
    for (int n = lane; n < n_neg; n += 64) {
        const double target = uniforms[(int64_t)n * B + b] * Z;
        int lo = 0, hi = m;   // k* = the first entry with F(c_k) > target (m: none)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_F[mid] > target) hi = mid; else lo = mid + 1;
        }
        const int ks = lo;
        const double S = ks ? s_S[ks - 1] : 0.0;
        // items after entry k* - 1 and before entry k* carry e0 cdf[j] + S_{k* - 1}; if none of them passes, it is entry k* itself
        int jlo = ks ? column(ks - 1) + 1 : 0, jhi = ks < m ? column(ks) : n_items - 1;
        while (jlo < jhi) {
            const int mid = (jlo + jhi) >> 1;
            if (fma(e0, cdf[mid], S) > target) jhi = mid; else jlo = mid + 1;
        }
        // A draw never names an item of weight 0.  Its F equals its predecessor's in exact arithmetic, but the scan rounds S_k in an order
        // that differs from lane to lane, so F of a zero-weight item can come out a spacing above it and win a target that lies in between
        // (u = 1 - 2^-53 behind the last live item, u = 0 before the first): the draw then moves to the nearest live item before it, or
        // after it when there is none.  k = the first entry whose column is >= j.
        int j = min(jlo, n_items - 1), k = ks;   // (the clamp acts only when the target is not a number)
        if (k > 0 && column(k - 1) >= j) --k;
        auto dead = [&](int j_, int k_) {
            if (proposal[j_] == 0.f) return true;
            return k_ < m && column(k_) == j_ ? exp((double)t[p0 + k_] - M) == 0.0 : e0 == 0.0;
        };
        if (!bad && dead(j, k)) {
            int jb = j, kb = k;
            while (jb >= 0 && dead(jb, kb)) {
                --jb;
                if (kb > 0 && column(kb - 1) >= jb) --kb;
            }
            if (jb >= 0) {
                j = jb;
            } else {
                while (j < n_items - 1 && dead(j, k)) {
                    if (k < m && column(k) == j) ++k;
                    ++j;
                }
            }
        }
        out[(int64_t)n * B + b] = bad ? -1 : (int64_t)j;
    }
}

// ---- (b) frozen-tower loss -----------------------------------------------------------------------------------------------------
// A row in registers: NV float4 per lane, chunk lane + 64 v (a chunk beyond dim / 4 holds zeros and stays out of every sum).
template <int NV>
struct Row {
    float4 v[NV];
};

template <int NV>
__device__ __forceinline__ Row<NV> load_row(const float *__restrict__ base, int lane, int nchunks) {
    Row<NV> r;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        r.v[i] = c < nchunks ? *reinterpret_cast<const float4 *>(base + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return r;
}

// x -> xh = (x - mean) rstd in place (torch's LayerNorm: biased variance); chunks beyond the row stay zero.
// Every product-sum is an explicit fmaf and contraction is off: the same row gives the same bits wherever the call is inlined.
template <int NV>
__device__ __forceinline__ void normalize(Row<NV> &r, int lane, int nchunks, float inv_dim, float eps) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (r.v[i].x + r.v[i].y) + (r.v[i].z + r.v[i].w);
    const float mean = wave_sum(s) * inv_dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool in = lane + 64 * i < nchunks;
        float4 &v = r.v[i];
        v.x = in ? v.x - mean : 0.f, v.y = in ? v.y - mean : 0.f, v.z = in ? v.z - mean : 0.f, v.w = in ? v.w - mean : 0.f;
        q = fmaf(v.x, v.x, q), q = fmaf(v.y, v.y, q), q = fmaf(v.z, v.z, q), q = fmaf(v.w, v.w, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) * inv_dim + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i].x *= rstd, r.v[i].y *= rstd, r.v[i].z *= rstd, r.v[i].w *= rstd;
}

// sum_d q_d (a - b)_d: exactly 0 for two rows of the same bits
template <int NV>
__device__ __forceinline__ float dot_diff(const Row<NV> &q, const Row<NV> &a, const Row<NV> &b) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        s = fmaf(q.v[i].x, a.v[i].x - b.v[i].x, s), s = fmaf(q.v[i].y, a.v[i].y - b.v[i].y, s);
        s = fmaf(q.v[i].z, a.v[i].z - b.v[i].z, s), s = fmaf(q.v[i].w, a.v[i].w - b.v[i].w, s);
    }
    return wave_sum(s);
}

__device__ __forceinline__ float softplus_neg(float d) { return fmaxf(-d, 0.f) + log1pf(expf(-fabsf(d))); }   // softplus(-d) = -logsigmoid(d)
__device__ __forceinline__ float sigmoid_neg(float d) {                                                       // sigmoid(-d), no overflow
    const float e = expf(-fabsf(d));
    return (d >= 0.f ? e : 1.f) / (1.f + e);
}

// a pointer -> the row's address (clamped) and whether it was inside the table
__device__ __forceinline__ const float *row_of(const float *__restrict__ table, int64_t p, int64_t n_rows, int dim, bool &ok) {
    ok = ok && p >= 0 && p < n_rows;
    return table + min(max(p, (int64_t)0), n_rows - 1) * dim;
}

// The shared walk over one batch row: xh_i, xh_j, then every negative.  per_neg(D, xh_n) sees each negative's difference and row.
template <int NV, typename F>
__device__ __forceinline__ void walk(const float *__restrict__ table, int64_t n_rows, int dim, const Row<NV> &gamma, const Row<NV> &beta, float eps,
                                     const int64_t *__restrict__ ptr_i, const int64_t *__restrict__ ptr_j, const int64_t *__restrict__ ptr_nj,
                                     int B, int n_neg, int b, int lane, Row<NV> &xi, Row<NV> &xj, bool &ok, F per_neg) {
    const int nchunks = dim >> 2;
    const float inv_dim = 1.f / (float)dim;
    ok = true;
    xi = load_row<NV>(row_of(table, ptr_i[b], n_rows, dim, ok), lane, nchunks);
    xj = load_row<NV>(row_of(table, ptr_j[b], n_rows, dim, ok), lane, nchunks);
    Row<NV> next = load_row<NV>(row_of(table, ptr_nj[b], n_rows, dim, ok), lane, nchunks);
    normalize<NV>(xi, lane, nchunks, inv_dim, eps);
    normalize<NV>(xj, lane, nchunks, inv_dim, eps);
    Row<NV> q;   // e_i gamma
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        q.v[i].x = (xi.v[i].x * gamma.v[i].x + beta.v[i].x) * gamma.v[i].x, q.v[i].y = (xi.v[i].y * gamma.v[i].y + beta.v[i].y) * gamma.v[i].y;
        q.v[i].z = (xi.v[i].z * gamma.v[i].z + beta.v[i].z) * gamma.v[i].z, q.v[i].w = (xi.v[i].w * gamma.v[i].w + beta.v[i].w) * gamma.v[i].w;
    }
    for (int n = 0; n < n_neg; ++n) {
        Row<NV> xn = next;
        if (n + 1 < n_neg) next = load_row<NV>(row_of(table, ptr_nj[(int64_t)(n + 1) * B + b], n_rows, dim, ok), lane, nchunks);
        normalize<NV>(xn, lane, nchunks, inv_dim, eps);
        per_neg(dot_diff<NV>(q, xj, xn), xn);   // (ptr_nj == ptr_j: the same bits after normalize, a difference of exactly 0)
    }
}

template <int NV>
__device__ __forceinline__ void load_affine(const float *__restrict__ gamma, const float *__restrict__ beta, int lane, int nchunks, Row<NV> &g, Row<NV> &bt) {
    g = gamma ? load_row<NV>(gamma, lane, nchunks) : Row<NV>();
    bt = beta ? load_row<NV>(beta, lane, nchunks) : Row<NV>();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!gamma) g.v[i] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (!beta) bt.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// grid = ceil(B / 4), block = 4 waves, a wave per batch row: part[b] = w_b sum_n softplus(-D_nb) (NaN for a pointer outside the table)
template <int NV>
__global__ __launch_bounds__(256) void bpr_frozen_fwd_kernel(const float *__restrict__ table, int64_t n_rows, int dim, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float eps, const int64_t *__restrict__ ptr_i,
                                                            const int64_t *__restrict__ ptr_j, const int64_t *__restrict__ ptr_nj,
                                                            const float *__restrict__ w, int B, int n_neg, float *__restrict__ part) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;   // (uniform for the wave)
    Row<NV> g, bt, xi, xj;
    load_affine<NV>(gamma, beta, lane, dim >> 2, g, bt);
    bool ok;
    float acc = 0.f;
    walk<NV>(table, n_rows, dim, g, bt, eps, ptr_i, ptr_j, ptr_nj, B, n_neg, b, lane, xi, xj, ok, [&](float D, const Row<NV> &) { acc += softplus_neg(D); });
    if (lane == 0) part[b] = ok ? w[b] * acc : __builtin_nanf("");
}

// out3 = {loss, numerator sum_b part_b, denominator n_neg sum_b w_b}: fp64, one fixed order
__global__ __launch_bounds__(256) void bpr_finish_kernel(const float *__restrict__ part, const float *__restrict__ w, int B, int n_neg,
                                                        float *__restrict__ out3) {
    block256_sum2(part, w, B, [&](double num, double wsum) {
        const double den = wsum * (double)n_neg;
        out3[0] = (float)(num / den), out3[1] = (float)num, out3[2] = (float)den;
    });
}

// grid = nblocks, block = 4 waves; wave (block, y) takes the batch rows 4 block + y, + 4 nblocks, ... and keeps its share of
// sum_b R_b (2 xh_i gamma + beta) and sum_b R_b gamma in registers; the block's four shares are added in wave order through LDS
// -> partial [nblocks][2][dim].
template <int NV>
__global__ __launch_bounds__(256) void bpr_frozen_bwd_kernel(const float *__restrict__ table, int64_t n_rows, int dim, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float eps, const int64_t *__restrict__ ptr_i,
                                                            const int64_t *__restrict__ ptr_j, const int64_t *__restrict__ ptr_nj,
                                                            const float *__restrict__ w, int B, int n_neg, float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_acc[2 * MAX_DIM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nchunks = dim >> 2;
    Row<NV> g, bt, xi, xj, dg, db;
    load_affine<NV>(gamma, beta, lane, nchunks, g, bt);
#pragma unroll
    for (int i = 0; i < NV; ++i) dg.v[i] = db.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = blockIdx.x * 4 + wv; b < B; b += gridDim.x * 4) {
        Row<NV> C;
#pragma unroll
        for (int i = 0; i < NV; ++i) C.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        float G = 0.f;
        const float wb = w[b];
        bool ok;
        walk<NV>(table, n_rows, dim, g, bt, eps, ptr_i, ptr_j, ptr_nj, B, n_neg, b, lane, xi, xj, ok, [&](float D, const Row<NV> &xn) {
            const float gn = -wb * sigmoid_neg(D);
            G += gn;
#pragma unroll
            for (int i = 0; i < NV; ++i) C.v[i].x += gn * xn.v[i].x, C.v[i].y += gn * xn.v[i].y, C.v[i].z += gn * xn.v[i].z, C.v[i].w += gn * xn.v[i].w;
        });
        if (!ok) G = __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            auto one = [&](float xi_, float xj_, float c, float ga, float be, float &og, float &ob) {
                const float R = G * xj_ - c;
                og += R * (2.f * xi_ * ga + be);
                ob += R * ga;
            };
            one(xi.v[i].x, xj.v[i].x, C.v[i].x, g.v[i].x, bt.v[i].x, dg.v[i].x, db.v[i].x);
            one(xi.v[i].y, xj.v[i].y, C.v[i].y, g.v[i].y, bt.v[i].y, dg.v[i].y, db.v[i].y);
            one(xi.v[i].z, xj.v[i].z, C.v[i].z, g.v[i].z, bt.v[i].z, dg.v[i].z, db.v[i].z);
            one(xi.v[i].w, xj.v[i].w, C.v[i].w, g.v[i].w, bt.v[i].w, dg.v[i].w, db.v[i].w);
        }
    }
    for (int y = 0; y < 4; ++y) {   // wave 0 stores, waves 1 .. 3 add in turn
        if (wv == y) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = lane + 64 * i;
                if (c < nchunks) {
                    float4 *pg = reinterpret_cast<float4 *>(s_acc + 4 * c), *pb = reinterpret_cast<float4 *>(s_acc + dim + 4 * c);
                    float4 a = dg.v[i], d = db.v[i];
                    if (y) {
                        const float4 og = *pg, ob = *pb;
                        a.x += og.x, a.y += og.y, a.z += og.z, a.w += og.w, d.x += ob.x, d.y += ob.y, d.z += ob.z, d.w += ob.w;
                    }
                    *pg = a, *pb = d;
                }
            }
        }
        __syncthreads();
    }
    float4 *dst = reinterpret_cast<float4 *>(partial + (int64_t)blockIdx.x * 2 * dim);
    for (int c = threadIdx.x; c < 2 * nchunks; c += 256) dst[c] = reinterpret_cast<const float4 *>(s_acc)[c];
}

// grad [2][dim] = (sum over the partial rows, in a fixed order) / denominator * grad_out.
// grid = ceil(2 dim / 256), block = 1024 = 16 waves: wave y adds the rows y, y + 16, ... of 64 float4 columns, then the 16 shares in wave order.
__global__ __launch_bounds__(1024) void bpr_grad_sum_kernel(const float *__restrict__ partial, int nblocks, int dim, const float *__restrict__ den_dev,
                                                           const float *__restrict__ grad_out_dev, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ __attribute__((aligned(16))) float4 s_p[16][64];
    const int lane = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, total = 2 * (dim >> 2);   // float4 column of the [2 dim] row
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < total)
        for (int r = y; r < nblocks; r += 16) {
            const float4 v = *reinterpret_cast<const float4 *>(partial + (int64_t)r * 2 * dim + 4 * c);
            a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
        }
    s_p[y][lane] = a;
    __syncthreads();
    if (y == 0 && c < total) {
        for (int r = 1; r < 16; ++r) {
            const float4 v = s_p[r][lane];
            a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
        }
        const float den = den_dev[0], go = grad_out_dev[0];   // (s / den) go: grad_out scales the unit gradient exactly
        a.x = a.x / den * go, a.y = a.y / den * go, a.z = a.z / den * go, a.w = a.w / den * go;
        float *dst = 4 * c < dim ? dgamma + 4 * c : dbeta + (4 * c - dim);
        *reinterpret_cast<float4 *>(dst) = a;
    }
}

static bool shape_ok(const char *who, int B, int n_neg, int dim) {
    if (B < 1 || n_neg < 1 || dim < 64 || dim % 64 != 0) {
        set_error("%s: B=%d n_neg=%d dim=%d (B >= 1, n_neg >= 1, dim %% 64 == 0)", who, B, n_neg, dim);
        return false;
    }
    if (B > MAX_B || n_neg > MAX_NEG || dim > MAX_DIM) {
        set_error("%s: B=%d n_neg=%d dim=%d beyond the supported range (B <= %d, n_neg <= %d, dim <= %d)", who, B, n_neg, dim, MAX_B, MAX_NEG, MAX_DIM);
        return false;
    }
    return true;
}
static int bwd_blocks(int B) { return std::min((B + 3) / 4, MAX_BWD_BLOCKS); }
// workspace: the forward's [B] partial losses, or the backward's [blocks][2][dim] partial gradients (one after the other: the larger)
static size_t ws_bytes_for(int B, int dim) {
    return std::max((size_t)B * sizeof(float), (size_t)bwd_blocks(B) * 2 * dim * sizeof(float)) + 256;   // + 256: the caller's pointer need only be 16-byte aligned
}

#define BPR_DISPATCH_NV(dim, CALL)          \
    switch (((dim) + 255) / 256) {          \
        case 1: { CALL(1); } break;         \
        case 2: { CALL(2); } break;         \
        case 3: { CALL(3); } break;         \
        case 4: { CALL(4); } break;         \
        case 5: { CALL(5); } break;         \
        case 6: { CALL(6); } break;         \
        case 7: { CALL(7); } break;         \
        default: { CALL(8); } break;        \
    }

}  // namespace bpr
}  // namespace ccr

using namespace ccr;
using namespace ccr::bpr;

extern "C" int ccr_bpr_sample(const int64_t *users, int B, int n_neg, int64_t n_users, const int64_t *prior_ptr, const int64_t *prior_idx,
                              const float *prior_t, float t0, const float *proposal, const double *proposal_cdf, int n_items,
                              const double *uniforms, int max_row_nnz, int64_t *out_nj, void *stream) {
    CCR_REQUIRE(B >= 1 && B <= MAX_B && n_neg >= 1 && n_neg <= MAX_NEG && n_items >= 1, "ccr_bpr_sample: B=%d n_neg=%d n_items=%d (1 <= B <= %d, 1 <= n_neg <= %d, n_items >= 1)",
                B, n_neg, n_items, MAX_B, MAX_NEG);
    CCR_REQUIRE(users && proposal && proposal_cdf && uniforms && out_nj, "ccr_bpr_sample: null pointer");
    if (prior_ptr) {
        CCR_REQUIRE(n_users >= 1 && (max_row_nnz == 0 || (prior_idx && prior_t)), "ccr_bpr_sample: a prior needs n_users >= 1, prior_idx and prior_t");
        CCR_REQUIRE(max_row_nnz >= 0 && max_row_nnz <= MAX_ROW_NNZ, "ccr_bpr_sample: max_row_nnz=%d: at most %d prior entries per row", max_row_nnz, MAX_ROW_NNZ);
    } else {
        max_row_nnz = 0;
    }
    hipLaunchKernelGGL(bpr_sample_kernel, dim3(B), dim3(64), (size_t)max_row_nnz * 2 * sizeof(double), (hipStream_t)stream, users, B, n_neg, n_users, prior_ptr,
                       prior_idx, prior_t, (double)t0, proposal, proposal_cdf, n_items, uniforms, max_row_nnz, out_nj);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

extern "C" size_t ccr_bpr_frozen_workspace_bytes(int B, int n_neg, int dim) {
    if (!shape_ok("ccr_bpr_frozen_workspace_bytes", B, n_neg, dim)) return 0;
    return ws_bytes_for(B, dim);
}

extern "C" int ccr_bpr_frozen_fwd(const float *table, int64_t n_rows, int dim, const float *gamma, const float *beta, float eps, const int64_t *ptr_i,
                                  const int64_t *ptr_j, const int64_t *ptr_nj, const float *w, int B, int n_neg, float *out3, void *workspace,
                                  size_t ws_bytes, void *stream) {
    if (!shape_ok("ccr_bpr_frozen_fwd", B, n_neg, dim)) return CCR_ERR_INVALID;
    CCR_REQUIRE(table && ptr_i && ptr_j && ptr_nj && w && out3 && n_rows >= 1, "ccr_bpr_frozen_fwd: null pointer or empty table");
    CCR_REQUIRE(((uintptr_t)table | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "ccr_bpr_frozen_fwd: table, gamma and beta must be 16-byte aligned");
    if (const int rc = check_workspace("ccr_bpr_frozen_fwd", workspace, ws_bytes_for(B, dim), ws_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)align256(workspace);
#define CALL(NV) \
    hipLaunchKernelGGL(bpr_frozen_fwd_kernel<NV>, dim3((B + 3) / 4), dim3(256), 0, s, table, n_rows, dim, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w, B, n_neg, part)
    BPR_DISPATCH_NV(dim, CALL)
#undef CALL
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(bpr_finish_kernel, dim3(1), dim3(256), 0, s, part, w, B, n_neg, out3);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

extern "C" int ccr_bpr_frozen_bwd_dev(const float *table, int64_t n_rows, int dim, const float *gamma, const float *beta, float eps, const int64_t *ptr_i,
                                      const int64_t *ptr_j, const int64_t *ptr_nj, const float *w, int B, int n_neg, const float *den_dev,
                                      const float *grad_out_dev, float *dgamma, float *dbeta, void *workspace, size_t ws_bytes, void *stream) {
    if (!shape_ok("ccr_bpr_frozen_bwd_dev", B, n_neg, dim)) return CCR_ERR_INVALID;
    CCR_REQUIRE(gamma && beta, "ccr_bpr_frozen_bwd_dev: no gradient without gamma and beta (elementwise_affine=False has nothing to train)");
    CCR_REQUIRE(table && ptr_i && ptr_j && ptr_nj && w && den_dev && grad_out_dev && dgamma && dbeta && n_rows >= 1,
                "ccr_bpr_frozen_bwd_dev: null pointer or empty table");
    CCR_REQUIRE(((uintptr_t)table | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)dgamma | (uintptr_t)dbeta) % 16 == 0,
                "ccr_bpr_frozen_bwd_dev: table, gamma, beta and the gradients must be 16-byte aligned");
    if (const int rc = check_workspace("ccr_bpr_frozen_bwd_dev", workspace, ws_bytes_for(B, dim), ws_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *partial = (float *)align256(workspace);
    const int nblocks = bwd_blocks(B);
#define CALL(NV) \
    hipLaunchKernelGGL(bpr_frozen_bwd_kernel<NV>, dim3(nblocks), dim3(256), 0, s, table, n_rows, dim, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w, B, n_neg, partial)
    BPR_DISPATCH_NV(dim, CALL)
#undef CALL
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(bpr_grad_sum_kernel, dim3((2 * (dim / 4) + 63) / 64), dim3(1024), 0, s, partial, nblocks, dim, den_dev, grad_out_dev, dgamma, dbeta);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}
