// ccr_dropout.hip -- the keep bits of the encoder's training dropout, and the one dropout site that has no layer kernel of its own.
// The reference fine-tunes its towers in train() with the checkpoints' dropout 0.1 (src/ccrec/models/bbpr.py:195-197,
// bert_mt.py:105-113).  The layer kernels (ccr_encoder.hip, ccr_encoder_bwd.hip) draw no random numbers: they read PACKED KEEP BITS
// that the two generator kernels here write, plus one scale factor, so the forward and both backward passes read the same stored
// decisions and a test can hand them any mask it likes.
//
//   dropout_bits_rows_kernel       bits [rows][dim / 32] for a row-wise site (hidden-state dropout in front of a residual + LayerNorm)
//   dropout_bits_attention_kernel  keep_q / keep_k [T][H][W] for the attention probabilities: the same decisions by query row and by key row
//   dropout_apply_kernel           y = x * keep * inv_keep, fp32 -> fp32 and its 16-bit copy (the dropout after the embedding LayerNorm)
//
// A decision is a pure function of (seed, stream, indices): Philox4x32-10 with key = the seed's two words, one call = four words =
// eight 16-bit lanes = the decisions of eight consecutive elements; keep iff lane >= thr = round(p * 65536).  Nothing depends on the
// launch geometry; ccrec_amd/dropout_ref.py restates it on the CPU bit for bit.
#include <math.h>

#include "ccr_common.h"
#include "ccr_encoder_common.h"

namespace ccr {

struct Philox4 {
    uint32_t w[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 o;
    o.w[0] = c0, o.w[1] = c1, o.w[2] = c2, o.w[3] = c3;
    return o;
}

// the eight keep bits of one call: bit j <-> lane j = (j & 1 ? high : low) half of word j >> 1
__device__ __forceinline__ uint32_t keep8(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t thr) {
    const Philox4 o = philox4x32_10(c0, c1, c2, c3, k0, k1);
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        b |= ((o.w[i] & 0xffffu) >= thr ? 1u : 0u) << (2 * i);
        b |= ((o.w[i] >> 16) >= thr ? 1u : 0u) << (2 * i + 1);
    }
    return b;
}

// the 32 keep bits of elements 32 w .. 32 w + 31 of index row `a`: counters (a, 4 w + i, stream, d), i = 0 .. 3
__device__ __forceinline__ uint32_t keep32(uint32_t a, uint32_t w, uint32_t stream, uint32_t d, uint32_t k0, uint32_t k1, uint32_t thr) {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) bits |= keep8(a, 4 * w + i, stream, d, k0, k1, thr) << (8 * i);
    return bits;
}

// one thread per output word
__global__ __launch_bounds__(256) void dropout_bits_rows_kernel(uint32_t *__restrict__ bits, int64_t n_words, int words_per_row,
                                                               uint32_t k0, uint32_t k1, uint32_t stream, uint32_t thr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / words_per_row;
        const int w = (int)(i - row * words_per_row);
        bits[i] = keep32((uint32_t)row, (uint32_t)w, stream, 0u, k0, k1, thr);
    }
}

// One wave per (sequence, head, 32 queries x 64 keys): lane -> query 32 tq + (lane & 31), key word 2 tp + (lane >> 5).  The lane's word IS
// keep_q's; keep_k's words are the same 32 x 32 tiles transposed -- bit kk of every lane gathered by one ballot, whose low half belongs to
// key 64 tp + kk and whose high half to key 64 tp + 32 + kk, kept by the lane of that number.
__global__ __launch_bounds__(256) void dropout_bits_attention_kernel(uint32_t *__restrict__ keep_q, uint32_t *__restrict__ keep_k,
                                                                    const int32_t *__restrict__ seq_start,
                                                                    const int32_t *__restrict__ seq_len, int64_t T, int H, int W,
                                                                    int max_len, uint32_t k0, uint32_t k1, uint32_t stream,
                                                                    uint32_t thr) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int pairs = (W + 1) >> 1;
    const int tq = item / pairs, tp = item - tq * pairs;
    const int b = blockIdx.z, h = blockIdx.y;
    int len = seq_len[b];
    if (len > max_len) len = max_len;
    if (tq >= W || 32 * tq >= len || 64 * tp >= len) return;   // (wave-uniform) nothing below the length in this tile
    const int64_t row0 = seq_start[b];
    const int ql = lane & 31, g = lane >> 5;
    const int q = 32 * tq + ql, wk = 2 * tp + g;
    const int64_t qrow = row0 + q;
    const uint32_t word = keep32((uint32_t)qrow, (uint32_t)wk, stream, (uint32_t)h, k0, k1, thr);
    if (q < len && wk < W && qrow >= 0 && qrow < T) keep_q[(qrow * H + h) * W + wk] = word;
    uint32_t mine = 0;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
        const uint64_t m = __ballot((word >> kk) & 1u);
        if (ql == kk) mine = g ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
    const int key = 32 * wk + ql;
    const int64_t krow = row0 + key;
    if (key < len && krow >= 0 && krow < T) keep_k[(krow * H + h) * W + tq] = mine;
}

// y = x * (keep ? inv_keep : 0): a thread takes four columns = one nibble of word (column >> 5) of its row
template <int DT>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const float4 *__restrict__ x, const uint32_t *__restrict__ bits, float inv_keep,
                                                           float4 *__restrict__ out_f32, uint2 *__restrict__ out_half, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t nib = bits[i >> 3] >> (4 * (int)(i & 7));   // dim % 32 == 0: the words of all rows are one array over the flat index
        const float4 v = x[i];
        float4 y;
        y.x = v.x * (nib & 1u ? inv_keep : 0.f);
        y.y = v.y * (nib & 2u ? inv_keep : 0.f);
        y.z = v.z * (nib & 4u ? inv_keep : 0.f);
        y.w = v.w * (nib & 8u ? inv_keep : 0.f);
        if (out_f32) out_f32[i] = y;
        if (out_half) out_half[i] = round4<typename Half16<DT>::elem>(y.x, y.y, y.z, y.w);
    }
}

// thr = round(p * 65536) for 0 <= p < 1; -1 when p is outside that or leaves nothing to keep
static inline int64_t dropout_threshold(double p) {
    if (!(p >= 0.0) || !(p < 1.0)) return -1;
    const int64_t thr = (int64_t)floor(p * 65536.0 + 0.5);
    return thr < 65536 ? thr : -1;
}

}  // namespace ccr

using namespace ccr;

extern "C" int ccr_dropout_bits_rows(uint32_t *bits, int64_t rows, int dim, uint64_t seed, uint32_t stream_id, double p, void *stream) {
    CCR_REQUIRE(bits, "ccr_dropout_bits_rows: null pointer");
    CCR_REQUIRE(rows >= 0 && rows <= 0xffffffffll && dim > 0 && dim % 256 == 0 && dim <= 2048,
                "ccr_dropout_bits_rows: rows=%lld dim=%d (dim %% 256 == 0, dim <= 2048)", (long long)rows, dim);
    const int64_t thr = dropout_threshold(p);
    CCR_REQUIRE(thr >= 0, "ccr_dropout_bits_rows: p=%g (0 <= p, round(p * 65536) < 65536)", p);
    if (rows == 0) return CCR_OK;
    const int64_t n_words = rows * (dim / 32);
    int64_t blocks = (n_words + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(dropout_bits_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bits, n_words, dim / 32,
                       (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, (uint32_t)thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

extern "C" int ccr_dropout_bits_attention(uint32_t *keep_q, uint32_t *keep_k, const int32_t *seq_start, const int32_t *seq_len,
                                          int64_t n_tokens, int n_seq, int n_heads, int max_len, uint64_t seed, uint32_t stream_id, double p,
                                          void *stream) {
    CCR_REQUIRE(keep_q && keep_k && seq_start && seq_len, "ccr_dropout_bits_attention: null pointer");
    CCR_REQUIRE(n_tokens >= 0 && n_tokens <= 0xffffffffll && n_seq >= 0 && n_seq <= 65535 && n_heads > 0 && n_heads <= 1024,
                "ccr_dropout_bits_attention: bad shape n_tokens=%lld n_seq=%d n_heads=%d", (long long)n_tokens, n_seq, n_heads);
    CCR_REQUIRE(max_len > 0 && max_len <= 512, "ccr_dropout_bits_attention: max_len=%d (1..512 tokens per sequence)", max_len);
    const int64_t thr = dropout_threshold(p);
    CCR_REQUIRE(thr >= 0, "ccr_dropout_bits_attention: p=%g (0 <= p, round(p * 65536) < 65536)", p);
    if (n_seq == 0 || n_tokens == 0) return CCR_OK;
    const int W = (max_len + 31) / 32;
    const int items = W * ((W + 1) / 2);
    hipLaunchKernelGGL(dropout_bits_attention_kernel, dim3((unsigned)((items + 3) / 4), n_heads, n_seq), dim3(256), 0, (hipStream_t)stream,
                       keep_q, keep_k, seq_start, seq_len, n_tokens, n_heads, W, max_len, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id,
                       (uint32_t)thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

extern "C" int ccr_dropout_apply(const float *x, const uint32_t *bits, float inv_keep, float *out_f32, uint16_t *out_half, int64_t rows,
                                 int dim, int half_dtype, void *stream) {
    CCR_REQUIRE(x && bits && (out_f32 || out_half), "ccr_dropout_apply: null pointer");
    CCR_REQUIRE_HALF(half_dtype, "ccr_dropout_apply");
    CCR_REQUIRE(rows >= 0 && dim > 0 && dim % 256 == 0 && dim <= 2048, "ccr_dropout_apply: rows=%lld dim=%d (dim %% 256 == 0, dim <= 2048)",
                (long long)rows, dim);
    CCR_REQUIRE(inv_keep >= 1.f && inv_keep <= 65536.f, "ccr_dropout_apply: inv_keep=%g (1 .. 65536)", (double)inv_keep);
    if (rows == 0) return CCR_OK;
    const int64_t n4 = rows * (dim / 4);
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (half_dtype == CCR_DTYPE_F16)
        hipLaunchKernelGGL(dropout_apply_kernel<CCR_DTYPE_F16>, grid, block, 0, s, reinterpret_cast<const float4 *>(x), bits, inv_keep,
                           reinterpret_cast<float4 *>(out_f32), reinterpret_cast<uint2 *>(out_half), n4);
    else
        hipLaunchKernelGGL(dropout_apply_kernel<CCR_DTYPE_BF16>, grid, block, 0, s, reinterpret_cast<const float4 *>(x), bits, inv_keep,
                           reinterpret_cast<float4 *>(out_f32), reinterpret_cast<uint2 *>(out_half), n4);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}
