// ccr_encoder.hip -- the non-GEMM pieces of a BERT encoder layer as gfx950 kernels (encoder-side fusion).
// The reference encodes with transformers' BertModel under autocast (src/ccrec/models/item_tower.py:122, scripts/al_0_rank.py:92-101);
// measured on one MI355X (profiles/r03_encode_kernel_stats.csv) its projections run at hipBLASLt speed (38 % of the GPU time) and
// the rest is attention at 57 TFLOP/s (22 %) plus separate residual-add / LayerNorm / cast passes (30 %).  Two kernels replace those:
//
//   attention_kernel      softmax(Q K^T * scale + key mask) V for every (sequence, head) of a batch of right-padded or packed
//                         sequences, head width 64, straight from the fused QKV projection's output.  VALU (exp) bound.
//   add_layernorm_kernel  LayerNorm(x_bf16 + residual_f32) -> the fp32 residual stream AND its bf16 copy (the next
//                         projection's operand) in one pass: 12 bytes per element instead of 28 over three kernels.  HBM bound.
//
// Arithmetic = what autocast(bf16) does in the reference's layer: bf16 operands, fp32 scores / softmax / accumulation,
// probabilities rounded to bf16 for the P V product, fp32 residual sum and LayerNorm.
#include <stdlib.h>

#include "ccr_common.h"
#include "ccr_encoder_common.h"
#include "ccr_index.h"

namespace ccr {

constexpr int ATT_MAX_THREADS = 512;   // up to 8 waves: one workgroup per (sequence, head) stages K / V once, wave w takes query blocks w, w + waves, ..
constexpr int ATT_QW = 32;             // query rows per wave step (the N side of one 32x32 MFMA tile)
constexpr int ATT_KMAX = 8, ATT_VMAX = 4;   // 16-byte key pieces / value-row pairs a thread stages (all in flight at once)
constexpr int ATT_KB = 64;         // keys per loop step (two 32-key score tiles: halves the online-softmax rescaling)
constexpr int ATT_HEAD = 64;       // head width
constexpr int ATT_KROW = 144;      // bytes per key row in LDS: 128 + 16, so the 16 lanes of a ds_read_b128 group hit distinct banks

// LDS: K [lk_pad rows][144 B] row-major | V.  TR = true (r6, the default): V stays ROW-MAJOR, [lk_pad keys][128 B], staged with
// ds_write_b128 as it arrives, the 64-byte halves of a row swapped on rows whose index has bit 1 set; the V^T fragments of the second
// MFMA come from ds_read_b64_tr_b16 (guide T10: a 16-lane group reads a 4-key x 16-column block and receives it column-major), whose
// 32-lane half then touches 4 rows x 64 B on 64 distinct banks.  TR = false (r3-r5, CCR_ATT_TR=0): V TRANSPOSED [64 d][2 * lk_pad + 8 B],
// written two keys per dword (23 % of the LDS-active cycles were bank-conflict cycles of those stores, profiles/r05_attention_pmc.txt).
// lk_pad = longest sequence rounded up to 64.
__host__ __device__ inline size_t attention_lds_bytes(int lk_pad) {
    return (size_t)lk_pad * ATT_KROW + (size_t)ATT_HEAD * (2 * (size_t)lk_pad + 8);   // (the row-major image needs 512 bytes less)
}
// BIAS = true: behind that image, the window of the head's relative-bias row that this launch can reach, lk_pad + max_len - 1 floats
// (entry i <-> offset key - query = i - (max_len - 1); the entries past offset max_len - 1 belong to keys >= max_len and hold zeros).
__host__ __device__ inline size_t attention_bias_lds_bytes(int lk_pad) { return 2 * (size_t)lk_pad * sizeof(float); }
// S^T = K Q^T on v_mfma_f32_32x32x16_bf16: A = 32 keys (lane & 31) x 8 head columns (8 * (lane >> 5) + j), B = 32 queries
// likewise -- both operands are 16 contiguous bytes of a row, no transposition.  C layout: lane -> query (lane & 31),
// register e -> key (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5): a lane owns ONE query and 16 of the tile's 32 keys, so the
// softmax row reductions are in-lane plus one exchange with lane ^ 32, and the probabilities, rounded to bf16, ARE the B
// operand of O^T = V^T P^T (contraction index = key; the A operand V^T is read from the transposed LDS image with the
// same key permutation: element j of lane half g <-> key 16 s + 4 g + (j & 3) + 8 (j >> 2)).
// LSE = true (the training forward, ccr_attention_fwd_train_half): the kernel also writes lse [T][H] fp32, the natural-log log-sum-exp of
// every live query row's scaled scores (0 on padding rows) -- what the backward (ccr_encoder_bwd.hip) rebuilds the probabilities from.
// LSE = false takes an empty struct in the pointer's place: the inference instantiations keep their argument layout and their code.
// DROP = true (ccr_attention_fwd_train_drop_half): the probability that is rounded to 16 bits for the P V product becomes
// p * keep * inv_keep with the keep bit of (query row, head, key) from keep_q [T][H][W]; the online softmax, lsum and lse stay those of
// the undropped scores.  A lane's 32 keys of a 64-key step are 16 bits each of words 2 kb and 2 kb + 1 of its own query's row.
// BIAS = true (the inference forward of an encoder with a shared relative position bias, ccr_attention_bias_half): the probability of
// (query, key) is proportional to exp(scale * q.k + table[head][R + key - query]).  The table entries are staged in LDS divided by scale
// and are what the score tiles' MFMA accumulators start from in place of zero, so every line after the MFMAs is the plain kernel's code
// on x = bias / scale + q.k: scale_log2e * x = log2e * (scale * q.k + bias).  An all-zero table starts them from zero: the plain kernel's
// bits.  BIAS = false takes an empty struct, like LSE and DROP: the other instantiations keep their arguments and their code.
struct NoBias {};
struct RelBias {
    const float *table;   // [n_heads][2 R + 1] fp32
    int R;                // the table's centre column: offset 0
    float inv_scale;      // 1 / scale
};
template <bool BIAS>
struct BiasArg {
    typedef NoBias type;
};
template <>
struct BiasArg<true> {
    typedef RelBias type;
};
struct NoLse {};
template <bool LSE>
struct LseArg {
    typedef NoLse type;
};
template <>
struct LseArg<true> {
    typedef float *type;
};
template <int DT, bool TR, bool LSE = false, bool DROP = false, bool BIAS = false>
__global__ __launch_bounds__(ATT_MAX_THREADS) void attention_kernel(const uint16_t *__restrict__ qkv,
                                                                  const int32_t *__restrict__ seq_start,
                                                                  const int32_t *__restrict__ seq_len,
                                                                  uint16_t *__restrict__ out, int H, int pad_len, int max_len,
                                                                  int lk_pad, float scale_log2e, typename LseArg<LSE>::type lse,
                                                                  typename KeepArg<DROP>::type keep = {},
                                                                  typename BiasArg<BIAS>::type rb = {}) {
    typedef Half16<DT> HT;
    typedef typename HT::vec8 vec8;
    typedef typename HT::elem elem;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = nthreads >> 6;
    const int wq = (wv + blockIdx.x) % nwaves;   // the wave's first query block rotates with the head: second rounds spread over the SIMDs
    const int b = blockIdx.y, h = blockIdx.x;
    int len = seq_len[b];
    if (len > max_len) len = max_len;   // the LDS image holds max_len keys: a longer entry is cut (the caller's contract: seq_len <= max_len)
    if (len < 0) len = 0;
    const int rows = len > pad_len ? len : pad_len;   // rows the sequence occupies in the token arrays (padding rows get zeros)
    const int HD = H * ATT_HEAD;
    const int64_t stride = 3 * (int64_t)HD;
    const int64_t row0 = seq_start[b];
    const uint16_t *Qg = qkv + row0 * stride + h * ATT_HEAD;
    const uint16_t *Kg = Qg + HD;
    const uint16_t *Vg = Qg + 2 * HD;
    uint16_t *Og = out + row0 * HD + h * ATT_HEAD;
    const int ql = lane & 31, g = lane >> 5;
    if (len == 0) {   // an empty sequence (workgroup-uniform): its padding rows get zeros, nothing is read
        for (int q = tid; q < rows; q += nthreads) {
            uint4 *dst = reinterpret_cast<uint4 *>(Og + (int64_t)q * HD);
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i] = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (LSE) lse[(row0 + q) * H + h] = 0.f;
        }
        return;
    }

    char *Ks = smem;
    char *Vt = smem + (size_t)lk_pad * ATT_KROW;
    const int VS = 2 * lk_pad + 8;
    const int nkb = (len + ATT_KB - 1) / ATT_KB;
    const int nk = nkb * ATT_KB;

    // ---- stage K (row-major) and V (transposed, two keys per dword) of this (sequence, head); rows beyond len are zeros.
    // Every load of the staging -- and the wave's first query fragment -- is issued before the first LDS store: one memory
    // latency per workgroup instead of one per piece.  The launcher sizes the workgroup so that a thread has at most
    // ATT_KMAX key pieces and ATT_VMAX value pairs.
    uint4 kreg[ATT_KMAX], va[ATT_VMAX], vb[ATT_VMAX];
#pragma unroll
    for (int u = 0; u < ATT_KMAX; ++u) {
        const int i = tid + u * nthreads;
        const int r = i >> 3, c = i & 7;
        kreg[u] = make_uint4(0u, 0u, 0u, 0u);
        if (r < len) kreg[u] = *reinterpret_cast<const uint4 *>(Kg + (int64_t)r * stride + c * 8);
    }
#pragma unroll
    for (int u = 0; u < ATT_VMAX; ++u) {
        const int i = tid + u * nthreads;
        const int p = i >> 3, c = i & 7;
        va[u] = vb[u] = make_uint4(0u, 0u, 0u, 0u);
        if (2 * p < len) va[u] = *reinterpret_cast<const uint4 *>(Vg + (int64_t)(2 * p) * stride + c * 8);
        if (2 * p + 1 < len) vb[u] = *reinterpret_cast<const uint4 *>(Vg + (int64_t)(2 * p + 1) * stride + c * 8);
    }
    vec8 qf[4];
    {
        const int q = wq * ATT_QW + ql;
        const int qr = q < len ? q : len - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const vec8 *>(Qg + (int64_t)qr * stride + 16 * s + 8 * g);
    }
    // BIAS: entries 0 .. lk_pad + max_len - 2 of the window, at most two per thread (the launcher's staging bound: lk_pad <= nthreads);
    // entry i is the table's column R - (max_len - 1) + i while that offset is at most max_len - 1, and zero beyond
    float breg[2] = {0.f, 0.f};
    float *Bs = reinterpret_cast<float *>(smem + attention_lds_bytes(lk_pad));
    if constexpr (BIAS) {
        const float *brow = rb.table + (int64_t)h * (2 * rb.R + 1) + (rb.R - (max_len - 1));
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * nthreads;
            if (i <= 2 * (max_len - 1)) breg[u] = brow[i] * rb.inv_scale;
        }
    }
#pragma unroll
    for (int u = 0; u < ATT_KMAX; ++u) {
        const int i = tid + u * nthreads;
        if (i < nk * 8) *reinterpret_cast<uint4 *>(Ks + (i >> 3) * ATT_KROW + (i & 7) * 16) = kreg[u];
    }
    if constexpr (BIAS) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * nthreads;
            if (i < lk_pad + max_len - 1) Bs[i] = breg[u];
        }
    }
#pragma unroll
    for (int u = 0; u < ATT_VMAX; ++u) {
        const int i = tid + u * nthreads;
        if (i < nk * 4) {
            const int p = i >> 3, c = i & 7;
            if constexpr (TR) {   // rows 2p and 2p + 1 as they came: one ds_write_b128 each; 64-byte halves swapped where bit 1 of the row is set
                char *dst = Vt + (size_t)(2 * p) * 128 + ((c ^ ((p & 1) << 2)) << 4);
                *reinterpret_cast<uint4 *>(dst) = va[u];
                *reinterpret_cast<uint4 *>(dst + 128) = vb[u];
            } else {
                const uint32_t a[4] = {va[u].x, va[u].y, va[u].z, va[u].w}, bb[4] = {vb[u].x, vb[u].y, vb[u].z, vb[u].w};
                char *dst = Vt + (size_t)(8 * c) * VS + 4 * p;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    *reinterpret_cast<uint32_t *>(dst + (size_t)(2 * j) * VS) = (a[j] & 0xffffu) | (bb[j] << 16);
                    *reinterpret_cast<uint32_t *>(dst + (size_t)(2 * j + 1) * VS) = (a[j] >> 16) | (bb[j] & 0xffff0000u);
                }
            }
        }
    }
    __syncthreads();
    // TR: this lane's part of every transposed read.  A 16-lane group fetches a block of 4 keys x 16 head columns: lane 4 qq + pp of the
    // group supplies the address of key row (base + qq), columns 4 pp .. 4 pp + 3 (8 bytes) and receives column (lane & 15), keys base .. + 3.
    // Groups 0 / 1 of a 32-lane half take columns 0-15 / 16-31 (the lane's own column d = lane & 31); key base = ... + 4 g (multiple of 4),
    // so bit 1 of the row index is bit 1 of qq: the half swap is a per-lane constant.
    const int tr_qq = (lane & 15) >> 2, tr_pp = lane & 3;
    const int tr_off = (4 * g + tr_qq) * 128 + ((32 * ((lane >> 4) & 1) + 8 * tr_pp) ^ (((tr_qq >> 1) & 1) << 6));
    const int tr_other = (tr_off ^ 64) - tr_off;   // +64 or -64

    for (int q0w = wq * ATT_QW; q0w < rows; q0w += nwaves * ATT_QW) {   // wave-uniform; no barrier below
        const int q = q0w + ql;
        if (q0w >= len) {   // a block of padding rows only: defined output (zeros), no NaNs into the next projection
            if (q < rows) {
                uint2 *dst = reinterpret_cast<uint2 *>(Og + (int64_t)q * HD);
#pragma unroll
                for (int i = 0; i < 8; ++i) dst[i * 2 + g] = make_uint2(0u, 0u);
                if constexpr (LSE) {
                    if (g == 0) lse[(row0 + q) * H + h] = 0.f;
                }
            }
            continue;
        }
        if (q0w != wq * ATT_QW) {   // the wave's next query block (sequences beyond 32 x waves tokens)
            const int qr = q < len ? q : len - 1;
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const vec8 *>(Qg + (int64_t)qr * stride + 16 * s + 8 * g);
        }

        ef32x16 o0, o1;
#pragma unroll
        for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;
        float m = -INFINITY, lsum = 0.f;
        const uint32_t *keep_row = nullptr;   // DROP: the words of this lane's query row (a lane beyond the sequence repeats its last row)
        if constexpr (DROP) keep_row = keep.bits + ((row0 + (q < len ? q : len - 1)) * H + h) * keep.W;
        // BIAS: the window entry of (this lane's query, key 4 g); a lane beyond the sequence repeats its last row, so with key < nk <= lk_pad
        // every index below lies in 0 .. lk_pad + max_len - 2
        const float *bias_q = nullptr;
        if constexpr (BIAS) bias_q = Bs + ((max_len - 1) - (q < len ? q : len - 1) + 4 * g);

        for (int kb = 0; kb < nkb; ++kb) {
            uint32_t kw0 = 0, kw1 = 0;   // DROP: bit (e & 3) + 8 ((e & 15) >> 2) of kw0 >> 4 g <-> register e < 16, of kw1 >> 4 g <-> register 16 + e
            if constexpr (DROP) {
                kw0 = keep_row[2 * kb] >> (4 * g);                          // 2 kb < W: the step holds a key below len <= max_len
                if (2 * kb + 1 < keep.W) kw1 = keep_row[2 * kb + 1] >> (4 * g);   // (keys of a word beyond W are beyond len: their x is 0)
            }
            ef32x16 s0, s1;
            if constexpr (BIAS) {   // the score tiles start from bias / scale instead of zero: the MFMAs add q.k onto it, no extra registers
                const float *bp = bias_q + kb * ATT_KB;   // register e <-> key kb * 64 + (0 | 32) + (e & 3) + 8 (e >> 2) + 4 g, as in the mask below
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    s0[e] = bp[(e & 3) + 8 * (e >> 2)];
                    s1[e] = bp[32 + (e & 3) + 8 * (e >> 2)];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) s0[e] = s1[e] = 0.f;
            }
            const char *kp = Ks + (kb * ATT_KB + ql) * ATT_KROW + g * 16;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const vec8 k0 = *reinterpret_cast<const vec8 *>(kp + 32 * s);
                const vec8 k1 = *reinterpret_cast<const vec8 *>(kp + 32 * ATT_KROW + 32 * s);
                s0 = HT::mfma(k0, qf[s], s0);
                s1 = HT::mfma(k1, qf[s], s1);
            }
            float x[32];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                x[e] = s0[e];
                x[16 + e] = s1[e];
            }
            if (kb * ATT_KB + ATT_KB > len) {   // the last step: keys beyond the sequence
#pragma unroll
                for (int e = 0; e < 32; ++e) {
                    const int key = kb * ATT_KB + (e >> 4) * 32 + (e & 3) + 8 * ((e & 15) >> 2) + 4 * g;
                    if (key >= len) x[e] = -INFINITY;
                }
            }
            float mx = x[0];
#pragma unroll
            for (int e = 1; e < 32; ++e) mx = fmaxf(mx, x[e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);            // finite: every step holds at least one key < len
            const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale_log2e);   // m = -inf on the first step: 0
            const float bias = -mn * scale_log2e;
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                x[e] = __builtin_amdgcn_exp2f(fmaf(x[e], scale_log2e, bias));
                ps += x[e];
            }
            lsum = fmaf(lsum, alpha, ps);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                o0[e] *= alpha;
                o1[e] *= alpha;
            }
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    vec8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if constexpr (DROP) {
                            const int e = s2 * 8 + j;
                            const uint32_t bit = ((hb ? kw1 : kw0) >> ((e & 3) + 8 * (e >> 2))) & 1u;
                            pf[j] = (elem)(x[hb * 16 + e] * (bit ? keep.inv_keep : 0.f));
                        } else {
                            pf[j] = (elem)x[hb * 16 + s2 * 8 + j];
                        }
                    }
                    if constexpr (TR) {
                        // keys kbase .. + 3 and kbase + 8 .. + 11 (kbase = kb * 64 + hb * 32 + s2 * 16 + 4 g) of this lane's column d (a0) and d + 32 (a1)
                        typedef __attribute__((address_space(3))) es16x4 *lds_tr_ptr;
                        const char *vp = Vt + (size_t)(kb * ATT_KB + hb * 32 + s2 * 16) * 128 + tr_off;
                        union {
                            es16x4 h[2];
                            vec8 v;
                        } a0, a1;
                        a0.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vp));
                        a0.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vp + 8 * 128));
                        const char *vq = vp + tr_other;   // columns d + 32: the other 64-byte half of the same rows
                        a1.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vq));
                        a1.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vq + 8 * 128));
                        o0 = HT::mfma(a0.v, pf, o0);
                        o1 = HT::mfma(a1.v, pf, o1);
                    } else {
                        const int kbase = kb * ATT_KB + hb * 32 + s2 * 16 + 4 * g;
                        const char *vp = Vt + (size_t)ql * VS + 2 * kbase;
                        union {
                            uint2 u[2];
                            vec8 v;
                        } a0, a1;
                        a0.u[0] = *reinterpret_cast<const uint2 *>(vp);
                        a0.u[1] = *reinterpret_cast<const uint2 *>(vp + 16);
                        a1.u[0] = *reinterpret_cast<const uint2 *>(vp + (size_t)32 * VS);
                        a1.u[1] = *reinterpret_cast<const uint2 *>(vp + (size_t)32 * VS + 16);
                        o0 = HT::mfma(a0.v, pf, o0);
                        o1 = HT::mfma(a1.v, pf, o1);
                    }
                }
            }
        }

        const float inv = 1.f / (lsum + __shfl_xor(lsum, 32));
        if constexpr (LSE) {   // ln sum_k exp(scale s_k) = scale m + ln sum_k exp(scale (s_k - m)); m and the sum are the same in both lane halves
            const float ltot = lsum + __shfl_xor(lsum, 32);
            if (g == 0 && q < rows) lse[(row0 + q) * H + h] = q < len ? fmaf(m * scale_log2e, 0.6931471805599453f, logf(ltot)) : 0.f;
        }
        if (q < len) {
            // O^T tile: lane -> query, register e -> head column 32 db + (e & 3) + 8 (e >> 2) + 4 g: four consecutive columns per 8-byte store
            uint16_t *dst = Og + (int64_t)q * HD + 4 * g;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                *reinterpret_cast<uint2 *>(dst + 8 * c4) =
                    round4<elem>(o0[4 * c4] * inv, o0[4 * c4 + 1] * inv, o0[4 * c4 + 2] * inv, o0[4 * c4 + 3] * inv);
                *reinterpret_cast<uint2 *>(dst + 32 + 8 * c4) =
                    round4<elem>(o1[4 * c4] * inv, o1[4 * c4 + 1] * inv, o1[4 * c4 + 2] * inv, o1[4 * c4 + 3] * inv);
            }
        } else if (q < rows) {
            uint2 *dst = reinterpret_cast<uint2 *>(Og + (int64_t)q * HD);
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i * 2 + g] = make_uint2(0u, 0u);
        }
    }   // query blocks of this wave
}

// One wave per row of dim = 256 * C elements; lane owns elements 4 * (64 c + lane) .. + 3 of every 256-element slice.
// DROP = true (ccr_add_layernorm_drop_half): v = x * keep * inv_keep + residual, one fp32 fma per element (the product is not rounded);
// the lane's four columns are one nibble of word (64 c + lane) >> 3 of its row of bits [rows][DIM / 32].
template <int C, int DT, bool DROP = false>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const uint16_t *__restrict__ x, const float *__restrict__ res,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           float eps, float *__restrict__ out_f32,
                                                           uint16_t *__restrict__ out_bf16, int64_t rows,
                                                           typename KeepArg<DROP>::type keep = {}) {
    constexpr int DIM = 256 * C;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[C][4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = 4 * (64 * c + lane);
        const uint2 xb = *reinterpret_cast<const uint2 *>(x + row * DIM + col);
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (res) r = *reinterpret_cast<const float4 *>(res + row * DIM + col);
        if constexpr (DROP) {
            float mk[4];
            keep_nibble(keep, row * (DIM / 32), 64 * c + lane, mk);
            v[c][0] = fmaf(Half16<DT>::lo(xb.x), mk[0], r.x);
            v[c][1] = fmaf(Half16<DT>::hi(xb.x), mk[1], r.y);
            v[c][2] = fmaf(Half16<DT>::lo(xb.y), mk[2], r.z);
            v[c][3] = fmaf(Half16<DT>::hi(xb.y), mk[3], r.w);
        } else {
            v[c][0] = Half16<DT>::lo(xb.x) + r.x;
            v[c][1] = Half16<DT>::hi(xb.x) + r.y;
            v[c][2] = Half16<DT>::lo(xb.y) + r.z;
            v[c][3] = Half16<DT>::hi(xb.y) + r.w;
        }
        sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
    float mean, rstd;
    row_mean_rstd<C>(v, sum, eps, mean, rstd);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = 4 * (64 * c + lane);
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + col);
        const float4 bt = *reinterpret_cast<const float4 *>(beta + col);
        float4 y = layernorm_row_out<C>(v, c, mean, rstd, gm, bt);
        if (out_f32) *reinterpret_cast<float4 *>(out_f32 + row * DIM + col) = y;
        if (out_bf16) *reinterpret_cast<uint2 *>(out_bf16 + row * DIM + col) = round4<typename Half16<DT>::elem>(y.x, y.y, y.z, y.w);
    }
}

// The embedding block of the encoder (transformers BertEmbeddings.forward): (word[id] + type[t]) + position[p] in that order, fp32,
// then LayerNorm -> the fp32 residual stream and its bf16 copy.  One wave per token; ids outside a table are clamped (memory safety).
// DROP = true (ccr_embed_layernorm_train_half with bits): the block's dropout on the way out, y * (keep ? inv_keep : 0) as
// dropout_apply_kernel forms it, from the lane's nibble of its row of bits [rows][DIM / 32].
template <int C, int DT, bool DROP = false>
__global__ __launch_bounds__(256) void embed_layernorm_kernel(const float *__restrict__ word, int64_t vocab,
                                                             const float *__restrict__ pos_tab, int64_t n_pos,
                                                             const float *__restrict__ type_tab, int64_t n_types,
                                                             const int64_t *__restrict__ ids, const int64_t *__restrict__ pos,
                                                             const int64_t *__restrict__ types, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, float eps, float *__restrict__ out_f32,
                                                             uint16_t *__restrict__ out_bf16, int64_t rows,
                                                             typename KeepArg<DROP>::type keep = {}) {
    constexpr int DIM = 256 * C;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    auto clamp = [](int64_t v, int64_t n) { return v < 0 ? (int64_t)0 : (v >= n ? n - 1 : v); };
    const float *w = word + clamp(ids[row], vocab) * DIM;
    const float *p = pos_tab + clamp(pos[row], n_pos) * DIM;
    const float *t = type_tab + clamp(types ? types[row] : 0, n_types) * DIM;
    float v[C][4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = 4 * (64 * c + lane);
        const float4 a = *reinterpret_cast<const float4 *>(w + col);
        const float4 b = *reinterpret_cast<const float4 *>(t + col);
        const float4 d = *reinterpret_cast<const float4 *>(p + col);
        v[c][0] = (a.x + b.x) + d.x;
        v[c][1] = (a.y + b.y) + d.y;
        v[c][2] = (a.z + b.z) + d.z;
        v[c][3] = (a.w + b.w) + d.w;
        sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
    float mean, rstd;
    row_mean_rstd<C>(v, sum, eps, mean, rstd);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int col = 4 * (64 * c + lane);
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + col);
        const float4 bt = *reinterpret_cast<const float4 *>(beta + col);
        float4 y = layernorm_row_out<C>(v, c, mean, rstd, gm, bt);
        if constexpr (DROP) {
            float mk[4];
            keep_nibble(keep, row * (DIM / 32), 64 * c + lane, mk);
            y.x *= mk[0], y.y *= mk[1], y.z *= mk[2], y.w *= mk[3];
        }
        if (out_f32) *reinterpret_cast<float4 *>(out_f32 + row * DIM + col) = y;
        if (out_bf16) *reinterpret_cast<uint2 *>(out_bf16 + row * DIM + col) = round4<typename Half16<DT>::elem>(y.x, y.y, y.z, y.w);
    }
}

// Exact (erf) GELU of a bf16 array, in place or out of place: 16 bytes per lane per access, grid-stride.  The same formula and fp32
// arithmetic as torch's GELU kernel (0.5 x (1 + erf(x / sqrt 2)), rounded to bf16 once): a pass of its own between the two FFN
// projections because the library's GEMM epilogue only offers the tanh form.
template <int DT>
__global__ __launch_bounds__(256) void gelu_kernel(const uint4 *__restrict__ x, uint4 *__restrict__ y, int64_t n16) {
    typedef Half16<DT> HT;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 v = x[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        float g[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = HT::lo(w[j]), b = HT::hi(w[j]);
            g[2 * j] = 0.5f * a * (1.f + erff(a * 0.70710678118654752440f));
            g[2 * j + 1] = 0.5f * b * (1.f + erff(b * 0.70710678118654752440f));
        }
        const uint2 r0 = round4<typename HT::elem>(g[0], g[1], g[2], g[3]), r1 = round4<typename HT::elem>(g[4], g[5], g[6], g[7]);
        y[i] = make_uint4(r0.x, r0.y, r1.x, r1.y);
    }
}

template <int DT, bool LSE = false, bool DROP = false, bool BIAS = false>
static int attention_any(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq, int n_heads,
                         int max_len, int pad_len, float scale, hipStream_t stream, typename LseArg<LSE>::type lse = {},
                         typename KeepArg<DROP>::type keep = {}, typename BiasArg<BIAS>::type rb = {}) {
    const int lk_pad = (max_len + ATT_KB - 1) / ATT_KB * ATT_KB;
    const size_t lds = attention_lds_bytes(lk_pad) + (BIAS ? attention_bias_lds_bytes(lk_pad) : 0);
    // the opt-in is cached per (kernel, device) whatever the size: ask for the kernel's maximum once (512 keys), not for this call's
    // image -- length-sorted batches start with the shortest texts
    static const bool tr = [] {
        const char *e = getenv("CCR_ATT_TR");      // A/B knob: 0 = the transposed-image kernel of rounds 3-5
        return !(e && atoi(e) == 0);
    }();
    if constexpr (BIAS) CCR_REQUIRE(tr, "ccr_attention_bias_half: the transposed-image kernel (CCR_ATT_TR=0) takes no bias");
    const void *kernel = nullptr;
    if constexpr (BIAS)
        kernel = reinterpret_cast<const void *>(&attention_kernel<DT, true, LSE, DROP, true>);
    else
        kernel = tr ? reinterpret_cast<const void *>(&attention_kernel<DT, true, LSE, DROP>) : reinterpret_cast<const void *>(&attention_kernel<DT, false, LSE, DROP>);
    const int rc = ensure_dynamic_lds(kernel, attention_lds_bytes(512) + (BIAS ? attention_bias_lds_bytes(512) : 0));
    if (rc != CCR_OK) return rc;
    int waves = (max_len + ATT_QW - 1) / ATT_QW;   // one wave per 32 query rows, at most 8 (longer sequences: the waves loop)
    if (waves > ATT_MAX_THREADS / 64) waves = ATT_MAX_THREADS / 64;
    // 129..192 tokens: the LDS image lets three workgroups share a CU, but workgroups of 5 or 6 waves do not pack three times into
    // its four SIMDs' wave slots (measured residency ~1.5 workgroups); 4 waves, the fifth / sixth query block on a second round
    // of a wave that rotates with the head: 134 -> 120 us at 136 tokens, 125 -> 111 at 160 (longer sequences: two workgroups
    // fit either way and 7-8 waves are faster)
    if (lk_pad == 192 && waves > 4) waves = 4;
    CCR_REQUIRE(lk_pad * 8 <= ATT_KMAX * 64 * waves && lk_pad * 4 <= ATT_VMAX * 64 * waves, "ccr_attention: staging bound (internal)");
    if constexpr (BIAS)
        hipLaunchKernelGGL((attention_kernel<DT, true, LSE, DROP, true>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, seq_start, seq_len,
                           out, n_heads, pad_len, max_len, lk_pad, scale * 1.4426950408889634f, lse, keep, rb);
    else if (tr)
        hipLaunchKernelGGL((attention_kernel<DT, true, LSE, DROP>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, seq_start, seq_len, out,
                           n_heads, pad_len, max_len, lk_pad, scale * 1.4426950408889634f, lse, keep);
    else
        hipLaunchKernelGGL((attention_kernel<DT, false, LSE, DROP>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, seq_start, seq_len, out,
                           n_heads, pad_len, max_len, lk_pad, scale * 1.4426950408889634f, lse, keep);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

template <int DT>
static int gelu_any(const uint16_t *x, uint16_t *y, int64_t n, hipStream_t stream) {
    const int64_t n16 = n / 8;
    int64_t blocks = (n16 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(gelu_kernel<DT>, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(x),
                       reinterpret_cast<uint4 *>(y), n16);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

}  // namespace ccr

using namespace ccr;

// ---- The implementations behind the exported pairs (plain / _drop_half, inference / _train_half): a null bits pointer means no dropout.
// Each reports its errors under the exported function's name `who`; every check runs before any launch.

static int attention_fwd_train(const char *who, const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, float *lse,
                               const uint32_t *keep_q, float inv_keep, int n_seq, int n_heads, int max_len, int pad_len, float scale,
                               int half_dtype, hipStream_t s) {
    if (const int rc = check_attention_shape(who, half_dtype, n_seq, n_heads, max_len, pad_len, scale)) return rc;
    if (keep_q)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    if (n_seq == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) {
        return dispatch_drop(keep_q != nullptr, [&](auto drop) {
            constexpr bool DROP = decltype(drop)::value;
            return attention_any<decltype(dt)::value, true, DROP>(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale, s, lse,
                                                                  keep_arg<DROP>(keep_q, inv_keep, (max_len + 31) / 32));
        });
    });
}

static int add_layernorm(const char *who, const uint16_t *x, const uint32_t *bits, float inv_keep, const float *res, const float *gamma,
                         const float *beta, float eps, float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype,
                         hipStream_t s) {
    if (const int rc = check_half(who, half_dtype)) return rc;
    if (const int rc = bits ? check_rows_dim(who, rows, dim) : check_rows_dim_infer(who, rows, dim)) return rc;
    if (bits)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    if (rows == 0) return CCR_OK;
    if (dim % 256) return add_layernorm_odd128(x, res, gamma, beta, eps, out_f32, out_half, rows, dim, half_dtype, s);   // (no bits: checked above)
    return dispatch_width(dim, [&](auto c) {
        return dispatch_half(half_dtype, [&](auto dt) {
            return dispatch_drop(bits != nullptr, [&](auto drop) {
                constexpr bool DROP = decltype(drop)::value;
                return launch_row_kernel(add_layernorm_kernel<decltype(c)::value, decltype(dt)::value, DROP>, (rows + 3) / 4, s, x, res, gamma, beta, eps,
                                   out_f32, out_half, rows, keep_arg<DROP>(bits, inv_keep, 0));
            });
        });
    });
}

static int embed_layernorm(const char *who, const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                           const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                           const int64_t *token_types, const float *gamma, const float *beta, float eps, const uint32_t *bits, float inv_keep,
                           float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype, hipStream_t s, bool odd_widths = false) {
    CCR_REQUIRE(word_table && position_table && type_table && token_ids && positions && gamma && beta && (out_f32 || out_half),
                "%s: null pointer", who);
    if (const int rc = check_half(who, half_dtype)) return rc;
    CCR_REQUIRE(vocab > 0 && n_positions > 0 && n_types > 0, "%s: empty table", who);
    // odd_widths: the inference entry points (no bits) also take the odd multiples of 128; the training block keeps 256 C with or without bits
    if (const int rc = odd_widths && !bits ? check_rows_dim_infer(who, rows, dim) : check_rows_dim(who, rows, dim)) return rc;
    if (bits)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    if (rows == 0) return CCR_OK;
    if (dim % 256)   // (an inference entry point without bits: checked above)
        return embed_layernorm_odd128(word_table, vocab, position_table, n_positions, type_table, n_types, token_ids, positions, token_types, gamma,
                                      beta, eps, out_f32, out_half, rows, dim, half_dtype, s);
    return dispatch_width(dim, [&](auto c) {
        return dispatch_half(half_dtype, [&](auto dt) {
            return dispatch_drop(bits != nullptr, [&](auto drop) {   // no bits: the inference kernel, no extra loads
                constexpr bool DROP = decltype(drop)::value;
                return launch_row_kernel(embed_layernorm_kernel<decltype(c)::value, decltype(dt)::value, DROP>, (rows + 3) / 4, s, word_table, vocab,
                                   position_table, n_positions, type_table, n_types, token_ids, positions, token_types, gamma, beta, eps,
                                   out_f32, out_half, rows, keep_arg<DROP>(bits, inv_keep, 0));
            });
        });
    });
}

extern "C" int ccr_attention_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq,
                                  int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *stream) {
    CCR_REQUIRE(qkv && seq_start && seq_len && out, "ccr_attention_half: null pointer");
    if (const int rc = check_attention_shape("ccr_attention_half", half_dtype, n_seq, n_heads, max_len, pad_len, scale)) return rc;
    if (n_seq == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) {
        return attention_any<decltype(dt)::value>(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale, (hipStream_t)stream);
    });
}

extern "C" int ccr_attention_bias_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, const float *rel_bias,
                                       int R, int n_seq, int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *stream) {
    CCR_REQUIRE(qkv && seq_start && seq_len && out, "ccr_attention_bias_half: null pointer");
    CCR_REQUIRE(rel_bias, "ccr_attention_bias_half: null bias table");
    if (const int rc = check_attention_shape("ccr_attention_bias_half", half_dtype, n_seq, n_heads, max_len, pad_len, scale)) return rc;
    CCR_REQUIRE(R >= max_len - 1 && R <= 511, "ccr_attention_bias_half: R=%d (max_len - 1 = %d <= R <= 511: the table holds every offset of a sequence)", R,
                max_len - 1);
    if (n_seq == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) {
        return attention_any<decltype(dt)::value, false, false, true>(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale,
                                                                      (hipStream_t)stream, NoLse{}, NoKeep{}, RelBias{rel_bias, R, 1.f / scale});
    });
}

extern "C" int ccr_attention_fwd_train_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, float *lse,
                                            int n_seq, int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *stream) {
    CCR_REQUIRE(qkv && seq_start && seq_len && out && lse, "ccr_attention_fwd_train_half: null pointer");
    return attention_fwd_train("ccr_attention_fwd_train_half", qkv, seq_start, seq_len, out, lse, nullptr, 1.f, n_seq, n_heads, max_len, pad_len,
                               scale, half_dtype, (hipStream_t)stream);
}

extern "C" int ccr_attention_fwd_train_drop_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out,
                                                 float *lse, const uint32_t *keep_q, float inv_keep, int n_seq, int n_heads, int max_len,
                                                 int pad_len, float scale, int half_dtype, void *stream) {
    CCR_REQUIRE(qkv && seq_start && seq_len && out && lse && keep_q, "ccr_attention_fwd_train_drop_half: null pointer");
    return attention_fwd_train("ccr_attention_fwd_train_drop_half", qkv, seq_start, seq_len, out, lse, keep_q, inv_keep, n_seq, n_heads, max_len,
                               pad_len, scale, half_dtype, (hipStream_t)stream);
}

extern "C" int ccr_attention_bf16(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out,
                                  int n_seq, int n_heads, int max_len, int pad_len, float scale, void *stream) {
    return ccr_attention_half(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale, CCR_DTYPE_BF16, stream);
}

extern "C" int ccr_add_layernorm_half(const uint16_t *x_half, const float *residual, const float *gamma, const float *beta, float eps,
                                      float *out_f32, uint16_t *out_half, int64_t rows, int dim, int half_dtype, void *stream) {
    CCR_REQUIRE(x_half && gamma && beta && (out_f32 || out_half), "ccr_add_layernorm_half: null pointer");
    return add_layernorm("ccr_add_layernorm_half", x_half, nullptr, 1.f, residual, gamma, beta, eps, out_f32, out_half, rows, dim, half_dtype,
                         (hipStream_t)stream);
}

extern "C" int ccr_add_layernorm_drop_half(const uint16_t *x_half, const uint32_t *bits, float inv_keep, const float *residual,
                                           const float *gamma, const float *beta, float eps, float *out_f32, uint16_t *out_half, int64_t rows,
                                           int dim, int half_dtype, void *stream) {
    CCR_REQUIRE(x_half && bits && gamma && beta && (out_f32 || out_half), "ccr_add_layernorm_drop_half: null pointer");
    return add_layernorm("ccr_add_layernorm_drop_half", x_half, bits, inv_keep, residual, gamma, beta, eps, out_f32, out_half, rows, dim,
                         half_dtype, (hipStream_t)stream);
}

extern "C" int ccr_add_layernorm(const uint16_t *x_bf16, const float *residual, const float *gamma, const float *beta, float eps,
                                 float *out_f32, uint16_t *out_bf16, int64_t rows, int dim, void *stream) {
    return ccr_add_layernorm_half(x_bf16, residual, gamma, beta, eps, out_f32, out_bf16, rows, dim, CCR_DTYPE_BF16, stream);
}

extern "C" int ccr_embed_layernorm_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                        const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                        const int64_t *token_types, const float *gamma, const float *beta, float eps, float *out_f32,
                                        uint16_t *out_half, int64_t rows, int dim, int half_dtype, void *stream) {
    return embed_layernorm("ccr_embed_layernorm_half", word_table, vocab, position_table, n_positions, type_table, n_types, token_ids, positions,
                           token_types, gamma, beta, eps, nullptr, 1.f, out_f32, out_half, rows, dim, half_dtype, (hipStream_t)stream, true);
}

extern "C" int ccr_embed_layernorm_train_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                              const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                              const int64_t *token_types, const float *gamma, const float *beta, float eps,
                                              const uint32_t *bits, float inv_keep, float *out_f32, uint16_t *out_half, int64_t rows, int dim,
                                              int half_dtype, void *stream) {
    return embed_layernorm("ccr_embed_layernorm_train_half", word_table, vocab, position_table, n_positions, type_table, n_types, token_ids,
                           positions, token_types, gamma, beta, eps, bits, inv_keep, out_f32, out_half, rows, dim, half_dtype,
                           (hipStream_t)stream);
}

extern "C" int ccr_embed_layernorm(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                   const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                   const int64_t *token_types, const float *gamma, const float *beta, float eps, float *out_f32,
                                   uint16_t *out_bf16, int64_t rows, int dim, void *stream) {
    return ccr_embed_layernorm_half(word_table, vocab, position_table, n_positions, type_table, n_types, token_ids, positions,
                                    token_types, gamma, beta, eps, out_f32, out_bf16, rows, dim, CCR_DTYPE_BF16, stream);
}

extern "C" int ccr_gelu_half(const uint16_t *x, uint16_t *y, int64_t n, int half_dtype, void *stream) {
    CCR_REQUIRE(x && y, "ccr_gelu_half: null pointer");
    if (const int rc = check_half("ccr_gelu_half", half_dtype)) return rc;
    CCR_REQUIRE(n >= 0 && n % 8 == 0, "ccr_gelu_half: n=%lld (a multiple of 8 elements)", (long long)n);
    CCR_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "ccr_gelu_half: 16-byte aligned arrays");
    if (n == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) { return gelu_any<decltype(dt)::value>(x, y, n, (hipStream_t)stream); });
}

extern "C" int ccr_gelu_bf16(const uint16_t *x, uint16_t *y, int64_t n, void *stream) {
    return ccr_gelu_half(x, y, n, CCR_DTYPE_BF16, stream);
}
