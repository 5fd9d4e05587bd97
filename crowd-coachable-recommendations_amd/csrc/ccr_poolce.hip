// ccr_poolce.hip -- contrastive cross-entropy of n_q queries over a pool of n_c candidates, with a label and a weight per query.
//
//   s_ij = inv_T <Q_i, C_j>,   ce_i = logsumexp_j s_ij - s_{i,label_i},   loss = sum_i w_i ce_i / sum_i w_i
//
// The square loss of ccr_inbatch.hip reads its MFMA fragments straight from L2: at pool shapes (1 024 x 16 384 x 768:
// 26 GFLOP forward, 2 x that backward, three bf16 parts each) that no longer carries.  Every GEMM here stages BOTH operands of a
// 64-deep K chunk in LDS (pitch 72 bf16 = 144 B: the 16 lanes of a ds_read_b128 group land on 16 different bank quads) and its four
// waves share them; the next chunk's global loads are issued before the current chunk's MFMAs.
//   fwd : pool_logits_kernel   128 queries x 128 candidates per workgroup -> the scaled logits S [n_q][ldS] fp32 (kept for the backward)
//         pool_lse_kernel      one workgroup per query: max, sum of exponentials (fixed tree), the label's logit -> lse_i, w_i ce_i
//         pool_finish_kernel   one workgroup: numerator and denominator in fp64, fixed order -> loss, and the stamp the backward checks
//   bwd : pool_transpose_kernel  Q^T and C^T (bf16, contraction index contiguous, zero padded to whole tiles)
//         pool_grad_kernel<false>  dQ = G C    (64 queries x 128 columns per workgroup, K = candidates, split over gridDim.z)
//         pool_grad_kernel<true>   dC = G^T Q  (64 candidates x 128 columns, K = queries)
//         G_ij = (exp(s_ij - lse_i) - [j = label_i]) w_i inv_T grad_out / W is evaluated from S while a chunk is staged and split into
//         THREE bf16 parts (hi + mid + lo = g to 2^-24 relative, as ccr_inbatch.hip): fp32-product accuracy on v_mfma_f32_32x32x16_bf16.
//         A K split writes its partial tile to the workspace; pool_sum_kernel adds the splits in split order.
// Deterministic: no atomics anywhere, every sum has one fixed order.  No read-back: a label outside [0, n_c) makes lse_i, the
// numerator and (through the numerator) every gradient NaN; a workspace whose stamp is not this (n_q, n_c, dim, inv_T) forward's
// makes every gradient NaN.  Every address is formed from clamped or padded indices, whatever label[] holds.
#include <algorithm>

#include "ccr_loss_common.h"

namespace ccr {
namespace poolce {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a 16-byte vector of 8 bf16 in flight between global memory and LDS

constexpr int KC = TILE64;         // contraction depth of one staged chunk
constexpr int LP = TILE64_PITCH;   // LDS row pitch in bf16 elements (KC + 8)
constexpr uint32_t POOL_MAGIC = 0x43435043u;   // 'CCPC'
constexpr int MAX_NQ = 1 << 16, MAX_NC = 1 << 20, MAX_DIM = 8192;
constexpr int64_t MAX_LOGITS = (int64_t)1 << 28;   // elements of S: 4 096 x 65 536 = 1 GiB of fp32, the largest shape asked for

// head of the workspace: words 0 .. 4 = {magic, n_q, n_c, dim, inv_T bits}, floats 8, 9 = numerator, denominator
struct PoolHead {
    uint32_t magic, n_q, n_c, dim, inv_t_bits, pad0, pad1, pad2;
    float num, den;
};

// fp32 -> bf16 (RNE: torch's .to(bfloat16) bits) of the queries (blockIdx.y = 0) and the candidates (1).  counts % 8 == 0.
__global__ __launch_bounds__(256) void pool_pack_kernel(const float *__restrict__ q, const float *__restrict__ c, int64_t count_q, int64_t count_c,
                                                       uint16_t *__restrict__ out) {
    const float *src = blockIdx.y == 0 ? q : c;
    const int64_t count = blockIdx.y == 0 ? count_q : count_c;
    uint16_t *dst = out + (blockIdx.y == 0 ? 0 : count_q);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < count; i += (int64_t)gridDim.x * 256 * 8)
        *reinterpret_cast<uint4 *>(dst + i) = pack8_bf16(src + i);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// grid = (candidate tiles of 128, query tiles of 128), block = 4 waves as 2 (queries) x 2 (candidates), a wave = 64 x 64 = 2 x 2 MFMA
// tiles.  Queries are the MFMA's A operand (accumulator rows), candidates its B operand (lanes): a half wave stores 32 consecutive
// candidates of one query = one 128-byte segment of S.
__global__ __launch_bounds__(256) void pool_logits_kernel(const uint16_t *__restrict__ Q, const uint16_t *__restrict__ C, int n_q, int n_c, int dim,
                                                         float inv_t, float *__restrict__ S, int64_t ldS, PoolHead *__restrict__ head) {
    __shared__ __attribute__((aligned(16))) uint16_t sA[128 * LP];
    __shared__ __attribute__((aligned(16))) uint16_t sB[128 * LP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5, wm = wv >> 1, wn = wv & 1;
    const int i0 = blockIdx.y * 128, j0 = blockIdx.x * 128;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) head->magic = 0u;   // this workspace's logits are being replaced
    uint4 ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u, r = idx >> 3, kv = (idx & 7) * 8;
            const int qi = min(i0 + r, n_q - 1), cj = min(j0 + r, n_c - 1);   // rows beyond the matrices repeat the last one; never stored
            const bool in = k0 + kv < dim;                                     // dim % 8 == 0: whole 16-byte vectors
            ra[u] = in ? *reinterpret_cast<const uint4 *>(Q + (int64_t)qi * dim + k0 + kv) : make_uint4(0, 0, 0, 0);
            rb[u] = in ? *reinterpret_cast<const uint4 *>(C + (int64_t)cj * dim + k0 + kv) : make_uint4(0, 0, 0, 0);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    const int nchunks = (dim + KC - 1) / KC;
    fetch(0);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();   // the previous chunk's fragment reads are done
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u, r = idx >> 3, kv = (idx & 7) * 8;
            *reinterpret_cast<uint4 *>(&sA[r * LP + kv]) = ra[u];
            *reinterpret_cast<uint4 *>(&sB[r * LP + kv]) = rb[u];
        }
        __syncthreads();
        if (c + 1 < nchunks) fetch((c + 1) * KC);
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const bf16x8 *>(&sA[(wm * 64 + t * 32 + l31) * LP + ks * 16 + 8 * h]);
                b[t] = *reinterpret_cast<const bf16x8 *>(&sB[(wn * 64 + t * 32 + l31) * LP + ks * 16 + 8 * h]);
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        }
    }
    // C layout of v_mfma_f32_32x32x16: column = lane & 31, register e -> row mfma32_row(0, e, lane >> 5)
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int j = j0 + wn * 64 + tn * 32 + l31;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = mfma32_row(i0 + wm * 64 + tm * 32, e, h);
                if (i < n_q && j < n_c) S[(int64_t)i * ldS + j] = acc[tm][tn][e] * inv_t;
            }
        }
}

// one workgroup per query: lse_i (NaN for a label outside the pool), cew_i = w_i ce_i, wq_i = w_i
__global__ __launch_bounds__(256) void pool_lse_kernel(const float *__restrict__ S, int64_t ldS, int n_c, const int32_t *__restrict__ label,
                                                      const float *__restrict__ weight, float *__restrict__ lse, float *__restrict__ cew,
                                                      float *__restrict__ wq) {
    __shared__ float s_red[8];
    const int tid = threadIdx.x, i = blockIdx.x;
    const float *row = S + (int64_t)i * ldS;   // 256-byte aligned: ldS % 64 == 0
    const int n4 = n_c & ~3;
    float m = -INFINITY;
    for (int j = tid * 4; j < n4; j += 1024) {
        const float4 v = *reinterpret_cast<const float4 *>(row + j);
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    if (n4 + tid < n_c) m = fmaxf(m, row[n4 + tid]);
    m = wave_max(m);
    if ((tid & 63) == 0) s_red[tid >> 6] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    float l = 0.f;
    for (int j = tid * 4; j < n4; j += 1024) {
        const float4 v = *reinterpret_cast<const float4 *>(row + j);
        l += (__expf(v.x - M) + __expf(v.y - M)) + (__expf(v.z - M) + __expf(v.w - M));
    }
    if (n4 + tid < n_c) l += __expf(row[n4 + tid] - M);
    l = wave_sum(l);
    if ((tid & 63) == 0) s_red[4 + (tid >> 6)] = l;
    __syncthreads();
    if (tid == 0) {
        const float L = ((s_red[4] + s_red[5]) + s_red[6]) + s_red[7];
        const int lab = label[i];
        const bool ok = lab >= 0 && lab < n_c;
        const float w = weight ? weight[i] : 1.f;
        const float v = ok ? M + __logf(L) : __builtin_nanf("");
        const float sl = row[ok ? lab : 0];
        lse[i] = v;
        cew[i] = w * (v - sl);
        wq[i] = w;
    }
}

// out = {loss, numerator, denominator}; the same two sums and the stamp go to the workspace's head
__global__ __launch_bounds__(256) void pool_finish_kernel(const float *__restrict__ cew, const float *__restrict__ wq, int n_q, int n_c, int dim,
                                                         uint32_t inv_t_bits, float *__restrict__ out, PoolHead *__restrict__ head) {
    block256_sum2(cew, wq, n_q, [&](double num, double den) {
        out[0] = (float)(num / den), out[1] = (float)num, out[2] = (float)den;
        head->num = (float)num, head->den = (float)den;
        head->n_q = (uint32_t)n_q, head->n_c = (uint32_t)n_c, head->dim = (uint32_t)dim, head->inv_t_bits = inv_t_bits;
        head->magic = POOL_MAGIC;   // every logit of this forward is in the workspace
    });
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// X [rows][dim] bf16 -> XT [dimp][ld] (dimp = dim rounded up to 128, ld = rows rounded up to 64), zeros beyond the matrix.
// grid = (ld / 64 of the larger matrix, dimp / 64, 2: queries | candidates), block = 256.
__global__ __launch_bounds__(256) void pool_transpose_kernel(const uint16_t *__restrict__ Q, const uint16_t *__restrict__ C, int n_q, int n_c, int dim,
                                                            uint16_t *__restrict__ QT, uint16_t *__restrict__ CT, int64_t ldq, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) uint16_t s_t[64][LP];
    const bool isq = blockIdx.z == 0;
    const int rows = isq ? n_q : n_c;
    const int64_t ld = isq ? ldq : ldc;
    const int r0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
    if (r0 >= ld) return;   // (uniform for the workgroup)
    const uint16_t *X = isq ? Q : C;
    uint16_t *XT = isq ? QT : CT;
    const int tid = threadIdx.x, r = tid >> 2, c0 = (tid & 3) * 16;
    uint16_t v[16];
    tile64_load16(X + (int64_t)(r0 + r) * dim, r0 + r < rows, d0 + c0, dim, v);
    tile64_scatter16(s_t, r, c0, v);
    __syncthreads();
    const uint4 *src = reinterpret_cast<const uint4 *>(&s_t[r][c0]);
    uint16_t *dst = XT + (int64_t)(d0 + r) * ld + r0 + c0;
    *reinterpret_cast<uint4 *>(dst) = src[0];
    *reinterpret_cast<uint4 *>(dst + 8) = src[1];
}

// out [M][dim] fp32 = sum over the three parts and over k of G_part[m][k] BT[n][k].
//   TRANS = false: dQ.  m = query i, k = candidate j, BT = CT [dimp][ldb = ldS].
//   TRANS = true : dC.  m = candidate j, k = query i, BT = QT [dimp][ldb = round_up(n_q, 64)].
// grid = (M tiles of 64, column tiles of 128, K splits), block = 4 waves as 2 (m) x 2 (n), a wave = 32 x 64 = 1 x 2 MFMA tiles x 3 parts.
// S is allocated with round_up(n_q, 64) rows of ldS = round_up(n_c, 64) floats and the transposes are padded to whole tiles, so no
// load of the K loop needs a bound; positions outside the matrix are SELECTED to zero (they may hold anything).
template <bool TRANS>
__global__ __launch_bounds__(256) void pool_grad_kernel(const float *__restrict__ S, int64_t ldS, const float *__restrict__ lse,
                                                       const int32_t *__restrict__ label, const float *__restrict__ weight, int n_q, int n_c, int dim,
                                                       const uint16_t *__restrict__ BT, int64_t ldb, float inv_t, const float *__restrict__ grad_out_dev,
                                                       const float *__restrict__ W_dev, const PoolHead *__restrict__ head, uint32_t inv_t_bits,
                                                       float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint16_t sG[3][64 * LP];
    __shared__ __attribute__((aligned(16))) uint16_t sB[128 * LP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5, wm = wv >> 1, wn = wv & 1;
    const int M = TRANS ? n_c : n_q, K = TRANS ? n_q : n_c;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 128;
    const int kchunks = (K + KC - 1) / KC, ksplit = gridDim.z;
    const int c_lo = (int)((int64_t)blockIdx.z * kchunks / ksplit), c_hi = (int)((int64_t)(blockIdx.z + 1) * kchunks / ksplit);
    // scale of every G element; NaN unless the workspace holds this forward's logits and its numerator is a number
    float gs = inv_t * grad_out_dev[0] / (W_dev ? W_dev[0] : head->den);
    {
        const float num = head->num;
        if (head->magic != POOL_MAGIC || head->n_q != (uint32_t)n_q || head->n_c != (uint32_t)n_c || head->dim != (uint32_t)dim ||
            head->inv_t_bits != inv_t_bits || num != num)
            gs = __builtin_nanf("");
    }
    // thread -> elements of the 64 (queries) x 64 (candidates) tile of S of one chunk
    //   dQ: query m0 + tid / 4, 16 consecutive candidates;   dC: queries k0 + 2 (tid / 8) + {0, 1}, 8 consecutive candidates
    constexpr int NR = TRANS ? 2 : 1, NCOL = TRANS ? 8 : 16;
    const int tr = TRANS ? 2 * (tid >> 3) : (tid >> 2), tc = TRANS ? (tid & 7) * 8 : (tid & 3) * 16;
    float4 sv[NR * NCOL / 4];
    float r_lse[NR], r_coef[NR];
    int r_lab[NR];
    u32x4 rb[4];
    auto row_params = [&](int t, int i) {   // clamped loads; rows beyond n_q get coefficient 0 by selection
        const int ic = min(i, n_q - 1);
        r_lse[t] = lse[ic];
        r_lab[t] = label[ic];
        r_coef[t] = (weight ? weight[ic] : 1.f) * gs;
        if (i >= n_q) r_coef[t] = 0.f, r_lse[t] = 0.f;
    };
    if constexpr (!TRANS) row_params(0, m0 + tr);
    auto fetch = [&](int c) {
        const int k0 = c * KC;
        const int ib = TRANS ? k0 + tr : m0 + tr, jb = TRANS ? m0 + tc : k0 + tc;
#pragma unroll
        for (int t = 0; t < NR; ++t) {
            if constexpr (TRANS) row_params(t, ib + t);
#pragma unroll
            for (int q4 = 0; q4 < NCOL / 4; ++q4) {
                sv[t * (NCOL / 4) + q4] = *reinterpret_cast<const float4 *>(S + (int64_t)(ib + t) * ldS + jb + 4 * q4);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u, r = idx >> 3, kv = (idx & 7) * 8;
            rb[u] = *reinterpret_cast<const u32x4 *>(BT + (int64_t)(n0 + r) * ldb + k0 + kv);
        }
    };
    auto stage = [&](int c) {
        const int k0 = c * KC;
        const int ib = TRANS ? k0 + tr : m0 + tr, jb = TRANS ? m0 + tc : k0 + tc;
        // word e of part p = two G elements.  dQ: candidates 2 e, 2 e + 1 of the thread's query; dC: the thread's two queries at candidate e
        uint32_t w[3][8];
        auto G = [&](float sval, int t, int j) {
            float g = __expf(sval - r_lse[t]);
            if (j == r_lab[t]) g -= 1.f;
            return (j < n_c && ib + t < n_q) ? g * r_coef[t] : 0.f;   // (a select: positions outside the matrix may hold anything)
        };
        auto pack3 = [&](float g0, float g1, int e) {
            uint16_t a0, a1, a2, b0, b1, b2;
            split3(g0, a0, a1, a2);
            split3(g1, b0, b1, b2);
            w[0][e] = (uint32_t)a0 | ((uint32_t)b0 << 16), w[1][e] = (uint32_t)a1 | ((uint32_t)b1 << 16), w[2][e] = (uint32_t)a2 | ((uint32_t)b2 << 16);
        };
        if constexpr (TRANS) {
#pragma unroll
            for (int q4 = 0; q4 < 2; ++q4) {
                const float4 v0 = sv[q4], v1 = sv[2 + q4];
                const int j = jb + 4 * q4;
                pack3(G(v0.x, 0, j), G(v1.x, 1, j), 4 * q4);
                pack3(G(v0.y, 0, j + 1), G(v1.y, 1, j + 1), 4 * q4 + 1);
                pack3(G(v0.z, 0, j + 2), G(v1.z, 1, j + 2), 4 * q4 + 2);
                pack3(G(v0.w, 0, j + 3), G(v1.w, 1, j + 3), 4 * q4 + 3);
            }
        } else {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 v = sv[q4];
                const int j = jb + 4 * q4;
                pack3(G(v.x, 0, j), G(v.y, 0, j + 1), 2 * q4);
                pack3(G(v.z, 0, j + 2), G(v.w, 0, j + 3), 2 * q4 + 1);
            }
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if constexpr (TRANS) {   // G^T: row = candidate, two consecutive queries per 4-byte store
#pragma unroll
                for (int e = 0; e < 8; ++e) *reinterpret_cast<uint32_t *>(&sG[p][(tc + e) * LP + tr]) = w[p][e];
            } else {
                *reinterpret_cast<uint4 *>(&sG[p][tr * LP + tc]) = make_uint4(w[p][0], w[p][1], w[p][2], w[p][3]);
                *reinterpret_cast<uint4 *>(&sG[p][tr * LP + tc + 8]) = make_uint4(w[p][4], w[p][5], w[p][6], w[p][7]);
            }
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    fetch(c_lo);   // (never more splits than chunks: c_lo < c_hi)
    for (int c = c_lo; c < c_hi; ++c) {
        __syncthreads();
        stage(c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u, r = idx >> 3, kv = (idx & 7) * 8;
            *reinterpret_cast<u32x4 *>(&sB[r * LP + kv]) = rb[u];
        }
        __syncthreads();
        fetch(c + 1 < c_hi ? c + 1 : c);   // (unconditional: the last chunk is fetched again and not used)
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            bf16x8 a[3], b[2];
#pragma unroll
            for (int p = 0; p < 3; ++p) a[p] = *reinterpret_cast<const bf16x8 *>(&sG[p][(wm * 32 + l31) * LP + ks * 16 + 8 * h]);
#pragma unroll
            for (int t = 0; t < 2; ++t) b[t] = *reinterpret_cast<const bf16x8 *>(&sB[(wn * 64 + t * 32 + l31) * LP + ks * 16 + 8 * h]);
#pragma unroll
            for (int p = 2; p >= 0; --p)   // small parts first
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[p], b[t], acc[t], 0, 0, 0);
        }
    }
    float *dst = out + (int64_t)blockIdx.z * M * dim;   // (one split: the gradient itself; more: its partial in the workspace)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = n0 + wn * 64 + t * 32 + l31;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = mfma32_row(m0 + wm * 32, e, h);
            if (m < M && n < dim) dst[(int64_t)m * dim + n] = acc[t][e];
        }
    }
}

// out[x] = partial[0][x] + partial[1][x] + ... in split order.  count % 4 == 0.
__global__ __launch_bounds__(256) void pool_sum_kernel(const float *__restrict__ partial, int64_t count, int ksplit, float *__restrict__ out) {
    for (int64_t x = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; x < count; x += (int64_t)gridDim.x * 1024) {
        float4 a = *reinterpret_cast<const float4 *>(partial + x);
        for (int s = 1; s < ksplit; ++s) {
            const float4 b = *reinterpret_cast<const float4 *>(partial + (int64_t)s * count + x);
            a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
        }
        *reinterpret_cast<float4 *>(out + x) = a;
    }
}

// K splits of a gradient GEMM: enough workgroups for ~4 per CU, never more splits than chunks, at most 32
static int pick_ksplit(int M, int K, int dim) {
    const int64_t base = (int64_t)((M + 63) / 64) * ((dim + 127) / 128);
    const int kchunks = (K + KC - 1) / KC;
    int64_t s = 1024 / base;
    if (s > 32) s = 32;
    if (s > kchunks) s = kchunks;
    return s < 1 ? 1 : (int)s;
}

// workspace: [head 256 B][S: round_up(n_q, 64) rows of ldS floats][cew, wq: n_q floats each][QT][CT][partial gradient tiles of a K split]
struct PoolWs {
    PoolHead *head;
    float *S, *cew, *wq, *partial;
    uint16_t *QT, *CT;
    int64_t ldS, ldq;
    int ks_q, ks_c;
    size_t total;
};
static PoolWs pool_ws(void *workspace, int n_q, int n_c, int dim) {
    PoolWs w;
    w.ldS = ((int64_t)n_c + 63) / 64 * 64;
    w.ldq = ((int64_t)n_q + 63) / 64 * 64;
    const size_t dimp = (size_t)(dim + 127) / 128 * 128;
    Carver c{(char *)workspace};
    w.head = c.take<PoolHead>(256);
    w.S = c.take<float>((size_t)w.ldq * w.ldS * sizeof(float));
    w.cew = c.take<float>((size_t)n_q * sizeof(float));
    w.wq = c.take<float>((size_t)n_q * sizeof(float));
    w.QT = c.take<uint16_t>(dimp * w.ldq * 2);
    w.CT = c.take<uint16_t>(dimp * w.ldS * 2);
    w.ks_q = pick_ksplit(n_q, n_c, dim);
    w.ks_c = pick_ksplit(n_c, n_q, dim);
    const size_t pq = w.ks_q > 1 ? (size_t)w.ks_q * n_q * dim * sizeof(float) : 0, pc = w.ks_c > 1 ? (size_t)w.ks_c * n_c * dim * sizeof(float) : 0;
    w.partial = c.take<float>(std::max(pq, pc));
    w.total = c.off + 256;   // + 256: the caller's pointer need only be 16-byte aligned
    return w;
}

static bool shape_ok(const char *who, int n_q, int n_c, int dim) {
    if (n_q < 1 || n_c < 1 || dim < 8 || dim % 8 != 0) {
        set_error("%s: n_q=%d n_c=%d dim=%d (n_q >= 1, n_c >= 1, dim %% 8 == 0)", who, n_q, n_c, dim);
        return false;
    }
    const int64_t logits = (((int64_t)n_q + 63) / 64 * 64) * (((int64_t)n_c + 63) / 64 * 64);
    if (n_q > MAX_NQ || n_c > MAX_NC || dim > MAX_DIM || logits > MAX_LOGITS) {
        set_error("%s: n_q=%d n_c=%d dim=%d beyond the supported range (n_q <= %d, n_c <= %d, dim <= %d, padded n_q x n_c <= 2^28 logits)", who, n_q, n_c,
                  dim, MAX_NQ, MAX_NC, MAX_DIM);
        return false;
    }
    return true;
}

}  // namespace poolce
}  // namespace ccr

using namespace ccr;
using namespace ccr::poolce;

extern "C" size_t ccr_pool_ce_workspace_bytes(int n_q, int n_c, int dim) {
    if (!shape_ok("ccr_pool_ce_workspace_bytes", n_q, n_c, dim)) return 0;
    return pool_ws(nullptr, n_q, n_c, dim).total;
}

extern "C" int ccr_pool_ce_fwd(const uint16_t *Q, const uint16_t *C, const int32_t *label, const float *weight, int n_q, int n_c, int dim,
                               float inv_temperature, float *out3, float *lse, void *workspace, size_t ws_bytes, void *stream) {
    if (!shape_ok("ccr_pool_ce_fwd", n_q, n_c, dim)) return CCR_ERR_INVALID;
    CCR_REQUIRE(Q && C && label && out3 && lse, "ccr_pool_ce_fwd: null pointer");
    CCR_REQUIRE(((uintptr_t)Q | (uintptr_t)C) % 16 == 0, "ccr_pool_ce_fwd: embedding pointers must be 16-byte aligned");
    if (const int rc = check_workspace("ccr_pool_ce_fwd", workspace, pool_ws(nullptr, n_q, n_c, dim).total, ws_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PoolWs w = pool_ws(align256(workspace), n_q, n_c, dim);
    hipLaunchKernelGGL(pool_logits_kernel, dim3((n_c + 127) / 128, (n_q + 127) / 128), dim3(256), 0, s, Q, C, n_q, n_c, dim, inv_temperature, w.S, w.ldS,
                       w.head);
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_lse_kernel, dim3(n_q), dim3(256), 0, s, w.S, w.ldS, n_c, label, weight, lse, w.cew, w.wq);
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_finish_kernel, dim3(1), dim3(256), 0, s, w.cew, w.wq, n_q, n_c, dim, __builtin_bit_cast(uint32_t, inv_temperature), out3, w.head);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

extern "C" int ccr_pool_ce_fwd_f32(const float *q, const float *c, const int32_t *label, const float *weight, int n_q, int n_c, int dim,
                                   float inv_temperature, uint16_t *packed, float *out3, float *lse, void *workspace, size_t ws_bytes, void *stream) {
    if (!shape_ok("ccr_pool_ce_fwd_f32", n_q, n_c, dim)) return CCR_ERR_INVALID;
    CCR_REQUIRE(q && c && packed, "ccr_pool_ce_fwd_f32: null pointer");
    CCR_REQUIRE(((uintptr_t)q | (uintptr_t)c | (uintptr_t)packed) % 16 == 0, "ccr_pool_ce_fwd_f32: pointers must be 16-byte aligned");
    const int64_t count_q = (int64_t)n_q * dim, count_c = (int64_t)n_c * dim;
    const int64_t blocks = (std::max(count_q, count_c) / 8 + 255) / 256;
    hipLaunchKernelGGL(pool_pack_kernel, dim3((unsigned)std::min<int64_t>(blocks, 8192), 2), dim3(256), 0, (hipStream_t)stream, q, c, count_q, count_c, packed);
    CCR_LAUNCH_CHECK();
    return ccr_pool_ce_fwd(packed, packed + count_q, label, weight, n_q, n_c, dim, inv_temperature, out3, lse, workspace, ws_bytes, stream);
}

extern "C" int ccr_pool_ce_bwd_dev(const uint16_t *Q, const uint16_t *C, const int32_t *label, const float *weight, const float *lse, int n_q, int n_c,
                                   int dim, float inv_temperature, const float *grad_out_dev, const float *W_dev, float *dQ, float *dC,
                                   void *workspace, size_t ws_bytes, void *stream) {
    if (!shape_ok("ccr_pool_ce_bwd_dev", n_q, n_c, dim)) return CCR_ERR_INVALID;
    CCR_REQUIRE(Q && C && label && lse && grad_out_dev && dQ && dC, "ccr_pool_ce_bwd_dev: null pointer");
    CCR_REQUIRE(((uintptr_t)Q | (uintptr_t)C | (uintptr_t)dQ | (uintptr_t)dC) % 16 == 0, "ccr_pool_ce_bwd_dev: pointers must be 16-byte aligned");
    if (const int rc = check_workspace("ccr_pool_ce_bwd_dev", workspace, pool_ws(nullptr, n_q, n_c, dim).total, ws_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PoolWs w = pool_ws(align256(workspace), n_q, n_c, dim);   // the FORWARD's workspace: the scaled logits and the stamp
    const uint32_t inv_t_bits = __builtin_bit_cast(uint32_t, inv_temperature);
    const int dimp = (dim + 127) / 128 * 128;
    hipLaunchKernelGGL(pool_transpose_kernel, dim3((unsigned)(std::max(w.ldq, w.ldS) / 64), dimp / 64, 2), dim3(256), 0, s, Q, C, n_q, n_c, dim, w.QT, w.CT,
                       w.ldq, w.ldS);
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pool_grad_kernel<false>, dim3((n_q + 63) / 64, dimp / 128, w.ks_q), dim3(256), 0, s, w.S, w.ldS, lse, label, weight, n_q, n_c, dim, w.CT,
                       w.ldS, inv_temperature, grad_out_dev, W_dev, w.head, inv_t_bits, w.ks_q > 1 ? w.partial : dQ);
    CCR_LAUNCH_CHECK();
    if (w.ks_q > 1) {
        const int64_t count = (int64_t)n_q * dim;
        hipLaunchKernelGGL(pool_sum_kernel, dim3((unsigned)std::min<int64_t>((count / 4 + 255) / 256, 4096)), dim3(256), 0, s, w.partial, count, w.ks_q, dQ);
        CCR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pool_grad_kernel<true>, dim3((n_c + 63) / 64, dimp / 128, w.ks_c), dim3(256), 0, s, w.S, w.ldS, lse, label, weight, n_q, n_c, dim, w.QT,
                       w.ldq, inv_temperature, grad_out_dev, W_dev, w.head, inv_t_bits, w.ks_c > 1 ? w.partial : dC);
    CCR_LAUNCH_CHECK();
    if (w.ks_c > 1) {
        const int64_t count = (int64_t)n_c * dim;
        hipLaunchKernelGGL(pool_sum_kernel, dim3((unsigned)std::min<int64_t>((count / 4 + 255) / 256, 4096)), dim3(256), 0, s, w.partial, count, w.ks_c, dC);
        CCR_LAUNCH_CHECK();
    }
    return CCR_OK;
}
