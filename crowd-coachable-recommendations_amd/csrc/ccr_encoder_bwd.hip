// ccr_encoder_bwd.hip -- the backward of the encoder layer kernels of ccr_encoder.hip, for fine-tuning through them: the reference's
// training steps run three encoder forwards and their backward per step (src/ccrec/models/bbpr.py:195-197, bert_mt.py:105-113).
//
//   attention_bwd_kernel       d(qkv) of softmax(Q K^T * scale + key mask) V from the saved output and log-sum-exp, two passes over one
//                              body: dQ per 32-query block with K, V in LDS; dK and dV per 32-key block with Q, dO in LDS.
//   add_layernorm_bwd_kernel   d(x + residual), d gamma, d beta of LayerNorm(x + residual); mean and rstd recomputed as the forward does.
//   gelu_bwd_kernel            d_y (Phi(x) + x phi(x)) from the pre-activation.
//
// Arithmetic: 16-bit MFMA operands, fp32 scores / probabilities / dS / reductions; no atomics anywhere, so every result is
// bit-identical from run to run.
#include "ccr_common.h"
#include "ccr_encoder_common.h"
#include "ccr_index.h"

namespace ccr {

constexpr int BWD_THREADS = 512;   // up to 8 waves per (sequence, head); wave w owns row blocks w, w + waves, ..
constexpr int BWD_TILE = 32;       // rows per MFMA tile on either side
constexpr int BWD_HEAD = 64;       // head width
constexpr int BWD_ROW = 144;       // bytes per row of an LDS image: 128 + 16 (distinct banks for the ds_read_b128 of a row fragment), 8-byte
                                   // aligned for ds_read_b64_tr_b16
constexpr int BWD_MAX_LEN = 512;

// LDS: two row-major images [lpad rows][144 B] | lse [lpad] fp32 | delta [lpad] fp32 (the last two in the dK / dV pass only)
__host__ __device__ inline size_t attention_bwd_lds_bytes(int lpad) { return 2 * (size_t)lpad * BWD_ROW + 2 * (size_t)lpad * 4; }

// One body, two passes.  A wave OWNS 32 rows (lane & 31; both 32-lane halves hold the same row, different head columns) whose two
// fragments stay in registers, and STREAMS the other side's rows from two LDS images X1 | X2 in tiles of 32:
//   KV = false (dQ):       own = queries (Q, dO),  streamed X1 = K, X2 = V;   acc  = dQ^T = K^T dS^T
//   KV = true  (dK, dV):   own = keys (K, V),      streamed X1 = Q, X2 = dO;  acc  = dK^T = Q^T dS,  accv = dV^T = dO^T P
// Per tile: s = X1 own1^T and dp = X2 own2^T on v_mfma_f32_32x32x16 (A = 16 contiguous bytes of a streamed row, B = the own fragment)
// land in the forward's C layout: lane -> own row, register e -> streamed row (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  Then
// P = exp2(s scale log2e - lse log2e) (no running maximum: lse is the forward's), dS = P (dp - delta) scale with lse and delta of
// the QUERY -- the lane's own in the dQ pass, the register's (from LDS) in the dK / dV pass.  Rounded to 16 bits, dS and P are B operands
// of the accumulating products, whose A operands X1^T / X2^T come out of the same row-major images by ds_read_b64_tr_b16 with the
// forward's row permutation (element j of lane half g <-> streamed row 16 s + 4 g + (j & 3) + 8 (j >> 2)).
// delta = sum_d dO O per query: computed in the dQ pass (a lane holds half of its query's columns: in-lane + one exchange), written to
// the workspace [n_seq][H][lpad], read back by the dK / dV pass that the launcher orders after it on the stream.
// DROP = true (ccr_attention_bwd_drop_half): with m = keep * inv_keep of (query, head, key), the P operand of dV is P m and
// dS = P (dp m - delta); delta = sum_d dO O stays as computed (sum_k P_k dP_k = dO . O holds with the dropped O).  Word t of the OWN
// row holds the 32 bits of streamed tile t: keep_q [query row][H][W] in the dQ pass, keep_k [key row][H][W] in the dK / dV pass.
template <int DT, bool KV, bool DROP = false>
__global__ __launch_bounds__(BWD_THREADS) void attention_bwd_kernel(const uint16_t *__restrict__ qkv, const uint16_t *__restrict__ out,
                                                                    const uint16_t *__restrict__ d_out, const float *__restrict__ lse,
                                                                    float *__restrict__ delta, const int32_t *__restrict__ seq_start,
                                                                    const int32_t *__restrict__ seq_len, uint16_t *__restrict__ d_qkv,
                                                                    int H, int pad_len, int max_len, int lpad, float scale,
                                                                    float scale_log2e, typename KeepArg<DROP>::type keep = {}) {
    typedef Half16<DT> HT;
    typedef typename HT::vec8 vec8;
    typedef typename HT::elem elem;
    typedef __attribute__((address_space(3))) es16x4 *lds_tr_ptr;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = nthreads >> 6;
    const int b = blockIdx.y, h = blockIdx.x;
    int len = seq_len[b];
    if (len > max_len) len = max_len;   // as the forward cuts it (the LDS images hold lpad >= max_len rows)
    if (len < 0) len = 0;
    const int rows = len > pad_len ? len : pad_len;
    const int HD = H * BWD_HEAD;
    const int64_t stride = 3 * (int64_t)HD;
    const int64_t row0 = seq_start[b];
    const uint16_t *Qg = qkv + row0 * stride + h * BWD_HEAD;
    const uint16_t *Kg = Qg + HD;
    const uint16_t *Vg = Qg + 2 * HD;
    const uint16_t *Og = out + row0 * HD + h * BWD_HEAD;
    const uint16_t *dOg = d_out + row0 * HD + h * BWD_HEAD;
    const float *lse_g = lse + row0 * H + h;                      // query q at lse_g[q * H]
    float *delta_g = delta + ((int64_t)b * H + h) * lpad;         // query q at delta_g[q]
    uint16_t *D1 = d_qkv + row0 * stride + h * BWD_HEAD + (KV ? HD : 0);   // dQ, or dK
    uint16_t *D2 = D1 + HD;                                                // dV (KV only)
    const int ql = lane & 31, g = lane >> 5;

    // zeros for the own rows r0 .. r0 + 31 that are padding (r >= len, r < rows): workgroup- or wave-uniform callers
    auto zero_rows = [&](int r) {
        if (r < rows) {
            uint2 *dst = reinterpret_cast<uint2 *>(D1 + (int64_t)r * stride);
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i * 2 + g] = make_uint2(0u, 0u);
            if constexpr (KV) {
                uint2 *dv = reinterpret_cast<uint2 *>(D2 + (int64_t)r * stride);
#pragma unroll
                for (int i = 0; i < 8; ++i) dv[i * 2 + g] = make_uint2(0u, 0u);
            }
        }
    };
    if (len == 0) {   // an empty sequence: its padding rows get zeros, nothing is read
        for (int r0 = wv * BWD_TILE; r0 < rows; r0 += nwaves * BWD_TILE) zero_rows(r0 + ql);
        return;
    }

    char *X1 = smem;
    char *X2 = smem + (size_t)lpad * BWD_ROW;
    float *lse_s = reinterpret_cast<float *>(smem + 2 * (size_t)lpad * BWD_ROW);
    float *delta_s = lse_s + lpad;
    const int ntile = (len + BWD_TILE - 1) / BWD_TILE;
    const int nstream = ntile * BWD_TILE;   // <= lpad

    // ---- stage the streamed side; rows len .. nstream - 1 are zeros (padding rows of the inputs are never read)
    {
        const uint16_t *S1 = KV ? Qg : Kg;
        const uint16_t *S2 = KV ? dOg : Vg;
        const int64_t st2 = KV ? (int64_t)HD : stride;
        for (int i = tid; i < nstream * 8; i += nthreads) {
            const int r = i >> 3, c = i & 7;
            uint4 a = make_uint4(0u, 0u, 0u, 0u), bb = a;
            if (r < len) {
                a = *reinterpret_cast<const uint4 *>(S1 + (int64_t)r * stride + c * 8);
                bb = *reinterpret_cast<const uint4 *>(S2 + (int64_t)r * st2 + c * 8);
            }
            *reinterpret_cast<uint4 *>(X1 + r * BWD_ROW + c * 16) = a;
            *reinterpret_cast<uint4 *>(X2 + r * BWD_ROW + c * 16) = bb;
        }
        if constexpr (KV) {
            for (int i = tid; i < nstream; i += nthreads) {
                lse_s[i] = i < len ? lse_g[(int64_t)i * H] * 1.4426950408889634f : 0.f;
                delta_s[i] = i < len ? delta_g[i] : 0.f;
            }
        }
    }
    __syncthreads();

    // this lane's part of every transposed read: a 16-lane group fetches 4 rows x 16 columns; lane 4 qq + pp of the group supplies the
    // address of row (base + qq), columns 4 pp .. + 3 (8 bytes) and receives column (lane & 15) of rows base .. + 3.  Groups 0 / 1 of a
    // 32-lane half take columns 0-15 / 16-31; row base = .. + 4 g.
    const int tr_qq = (lane & 15) >> 2, tr_pp = lane & 3;
    const int tr_off = (4 * g + tr_qq) * BWD_ROW + 32 * ((lane >> 4) & 1) + 8 * tr_pp;

    for (int r0 = wv * BWD_TILE; r0 < rows; r0 += nwaves * BWD_TILE) {   // wave-uniform; no barrier below
        const int r = r0 + ql;
        if (r0 >= len) {
            zero_rows(r);
            continue;
        }
        const int rr = r < len ? r : len - 1;   // lanes beyond the sequence repeat its last row: finite values nobody stores
        vec8 own1[4], own2[4];
        float my_lse = 0.f, my_delta = 0.f;
        if constexpr (KV) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                own1[s] = *reinterpret_cast<const vec8 *>(Kg + (int64_t)rr * stride + 16 * s + 8 * g);
                own2[s] = *reinterpret_cast<const vec8 *>(Vg + (int64_t)rr * stride + 16 * s + 8 * g);
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                own1[s] = *reinterpret_cast<const vec8 *>(Qg + (int64_t)rr * stride + 16 * s + 8 * g);
                own2[s] = *reinterpret_cast<const vec8 *>(dOg + (int64_t)rr * HD + 16 * s + 8 * g);
                const vec8 of = *reinterpret_cast<const vec8 *>(Og + (int64_t)rr * HD + 16 * s + 8 * g);
#pragma unroll
                for (int j = 0; j < 8; ++j) my_delta = fmaf((float)own2[s][j], (float)of[j], my_delta);
            }
            my_delta += __shfl_xor(my_delta, 32);
            my_lse = lse_g[(int64_t)rr * H] * 1.4426950408889634f;
            if (g == 0 && r < len) delta_g[r] = my_delta;
        }

        ef32x16 acc0, acc1, accv0, accv1;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc0[e] = acc1[e] = accv0[e] = accv1[e] = 0.f;
        // fp16 only: dS is rounded to 16 bits as 2^(DS_TOP - e_run) dS, e_run = the binary exponent of the largest |dS| this own row has met
        // (one per lane: a B-operand column and its accumulator column belong to one own row), and the accumulator follows when e_run grows
        // (a power of two: exact).  Unscaled fp16 gradients sit near 1e-6, where fp16's fixed spacing of 2^-24 would leave dS three or four
        // bits; with the factor it keeps its 11 whatever the magnitude.  `scale` is applied once, with 2^(e_run - DS_TOP), to the fp32 result.
        constexpr bool DS_SCALED = DT == CCR_DTYPE_F16;
        constexpr int DS_TOP = 8, DS_NONE = -1000, DS_MIN = -100;
        int e_run = DS_NONE;
        const uint32_t *keep_row = nullptr;   // DROP: the words of this lane's own row
        if constexpr (DROP) keep_row = keep.bits + ((row0 + rr) * H + h) * keep.W;

        for (int t = 0; t < ntile; ++t) {
            uint32_t kw = 0;   // DROP: bit (e & 3) + 8 (e >> 2) of kw <-> register e (ntile <= W: len <= max_len)
            if constexpr (DROP) kw = keep_row[t] >> (4 * g);
            ef32x16 sc, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[e] = dp[e] = 0.f;
            const char *p1 = X1 + (t * BWD_TILE + ql) * BWD_ROW + g * 16;
            const char *p2 = X2 + (t * BWD_TILE + ql) * BWD_ROW + g * 16;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                sc = HT::mfma(*reinterpret_cast<const vec8 *>(p1 + 32 * s), own1[s], sc);
                dp = HT::mfma(*reinterpret_cast<const vec8 *>(p2 + 32 * s), own2[s], dp);
            }
            float p[16], ds[16];
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                const int srow = t * BWD_TILE + 8 * c4 + 4 * g;   // streamed rows srow .. srow + 3 <-> registers 4 c4 .. 4 c4 + 3
                float l4[4] = {my_lse, my_lse, my_lse, my_lse}, d4[4] = {my_delta, my_delta, my_delta, my_delta};
                if constexpr (KV) {
                    const float4 lv = *reinterpret_cast<const float4 *>(lse_s + srow);
                    const float4 dv = *reinterpret_cast<const float4 *>(delta_s + srow);
                    l4[0] = lv.x, l4[1] = lv.y, l4[2] = lv.z, l4[3] = lv.w;
                    d4[0] = dv.x, d4[1] = dv.y, d4[2] = dv.z, d4[3] = dv.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * c4 + i;
                    const float pe = srow + i < len ? __builtin_amdgcn_exp2f(fmaf(sc[e], scale_log2e, -l4[i])) : 0.f;
                    if constexpr (DROP) {
                        const float mk = (kw >> (i + 8 * c4)) & 1u ? keep.inv_keep : 0.f;
                        p[e] = pe * mk;
                        ds[e] = pe * (dp[e] * mk - d4[i]);
                    } else {
                        p[e] = pe;
                        ds[e] = pe * (dp[e] - d4[i]);   // (without `scale`: the accumulator takes it at the end)
                    }
                }
            }
            if constexpr (DS_SCALED) {
                float amax = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(ds[e]));
                amax = fmaxf(amax, __shfl_xor(amax, 32));
                if (amax > 0.f) {
                    int ex = (int)(__float_as_uint(amax) >> 23) - 127;
                    if (ex < DS_MIN) ex = DS_MIN;
                    if (ex > e_run) {
                        const float shrink = e_run == DS_NONE ? 0.f : ldexpf(1.f, e_run - ex);   // (the accumulator is still zero at DS_NONE)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            acc0[e] *= shrink;
                            acc1[e] *= shrink;
                        }
                        e_run = ex;
                    }
                }
                const float f = e_run == DS_NONE ? 0.f : ldexpf(1.f, DS_TOP - e_run);
#pragma unroll
                for (int e = 0; e < 16; ++e) ds[e] *= f;
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                vec8 dsf, pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    dsf[j] = (elem)ds[s2 * 8 + j];
                    pf[j] = (elem)p[s2 * 8 + j];
                }
                // streamed rows base + 4 g .. + 3 and base + 4 g + 8 .. + 11 (base = 32 t + 16 s2) of this lane's column d (a0) and d + 32 (a1)
                const int off = (t * BWD_TILE + s2 * 16) * BWD_ROW + tr_off;
                union {
                    es16x4 hh[2];
                    vec8 v;
                } a0, a1;
                a0.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X1 + off));
                a0.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X1 + off + 8 * BWD_ROW));
                a1.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X1 + off + 64));
                a1.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X1 + off + 64 + 8 * BWD_ROW));
                acc0 = HT::mfma(a0.v, dsf, acc0);
                acc1 = HT::mfma(a1.v, dsf, acc1);
                if constexpr (KV) {
                    a0.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X2 + off));
                    a0.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X2 + off + 8 * BWD_ROW));
                    a1.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X2 + off + 64));
                    a1.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(X2 + off + 64 + 8 * BWD_ROW));
                    accv0 = HT::mfma(a0.v, pf, accv0);
                    accv1 = HT::mfma(a1.v, pf, accv1);
                }
            }
        }

        float unscale = scale;
        if constexpr (DS_SCALED) unscale = e_run == DS_NONE ? 0.f : scale * ldexpf(1.f, e_run - DS_TOP);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            acc0[e] *= unscale;
            acc1[e] *= unscale;
        }
        if (r < len) {
            // transposed tile: lane -> own row, register e -> head column 32 db + (e & 3) + 8 (e >> 2) + 4 g: four consecutive columns per store
            uint16_t *dst = D1 + (int64_t)r * stride + 4 * g;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                *reinterpret_cast<uint2 *>(dst + 8 * c4) = round4<elem>(acc0[4 * c4], acc0[4 * c4 + 1], acc0[4 * c4 + 2], acc0[4 * c4 + 3]);
                *reinterpret_cast<uint2 *>(dst + 32 + 8 * c4) = round4<elem>(acc1[4 * c4], acc1[4 * c4 + 1], acc1[4 * c4 + 2], acc1[4 * c4 + 3]);
            }
            if constexpr (KV) {
                uint16_t *dv = D2 + (int64_t)r * stride + 4 * g;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    *reinterpret_cast<uint2 *>(dv + 8 * c4) = round4<elem>(accv0[4 * c4], accv0[4 * c4 + 1], accv0[4 * c4 + 2], accv0[4 * c4 + 3]);
                    *reinterpret_cast<uint2 *>(dv + 32 + 8 * c4) =
                        round4<elem>(accv1[4 * c4], accv1[4 * c4 + 1], accv1[4 * c4 + 2], accv1[4 * c4 + 3]);
                }
            }
        } else {
            zero_rows(r);
        }
    }
}

// ---- LayerNorm(x + residual) backward.  One wave per row (lane owns elements 4 (64 c + lane) .. + 3 of every 256-element slice, as the
// forward), a workgroup of four waves walks rows blockIdx.x * 4 + wave, + 4 gridDim.x, ..  With xhat = (v - mean) rstd and g = d_y gamma:
// d_v = rstd (g - mean(g) - xhat mean(g xhat)).  d gamma = sum_rows d_y xhat and d beta = sum_rows d_y accumulate in registers over the
// workgroup's rows, the four waves add up through LDS in a fixed order, and the workgroup's sums go to partial [gridDim.x][2][DIM].
constexpr int LN_BWD_MAX_BLOCKS = 512;

// DROP = true (ccr_add_layernorm_bwd_drop_half): v is recomputed as x * keep * inv_keep + residual with the forward's bits and fma, so
// mean and rstd are the forward's; d_res = d_v as ever, d_x = d_v * keep * inv_keep rounded to x's type.
template <int C, int DT, bool DROP = false>
__global__ __launch_bounds__(256) void add_layernorm_bwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ res,
                                                               const float *__restrict__ gamma, float eps, const float *__restrict__ dy,
                                                               float *__restrict__ d_res, uint16_t *__restrict__ d_x,
                                                               float *__restrict__ partial, int64_t rows,
                                                               typename KeepArg<DROP>::type keep = {}) {
    constexpr int DIM = 256 * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // gamma and the zeroed column sums stay written out in the two backward kernels: as a shared function these eight lines cost every
    // instantiation two VGPRs (ccr_encoder_common.h holds the rest of the row body)
    float gm[C][4], ag[C][4], ab[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 t = *reinterpret_cast<const float4 *>(gamma + 4 * (64 * c + lane));
        gm[c][0] = t.x, gm[c][1] = t.y, gm[c][2] = t.z, gm[c][3] = t.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) ag[c][j] = ab[c][j] = 0.f;
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        float v[C][4], d[C][4];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int col = 4 * (64 * c + lane);
            const uint2 xb = *reinterpret_cast<const uint2 *>(x + row * DIM + col);
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (res) r = *reinterpret_cast<const float4 *>(res + row * DIM + col);
            const float4 t = *reinterpret_cast<const float4 *>(dy + row * DIM + col);
            d[c][0] = t.x, d[c][1] = t.y, d[c][2] = t.z, d[c][3] = t.w;
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
        float mean, rstd, m1, m2;
        row_mean_rstd<C>(v, sum, eps, mean, rstd);
        layernorm_bwd_row<C>(v, d, gm, mean, rstd, ag, ab, m1, m2);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int col = 4 * (64 * c + lane);
            const float4 y = layernorm_bwd_dv<C>(v, d, gm, c, rstd, m1, m2);
            if (d_res) *reinterpret_cast<float4 *>(d_res + row * DIM + col) = y;
            if constexpr (DROP) {
                if (d_x) {
                    float mk[4];
                    keep_nibble(keep, row * (DIM / 32), 64 * c + lane, mk);
                    *reinterpret_cast<uint2 *>(d_x + row * DIM + col) =
                        round4<typename Half16<DT>::elem>(y.x * mk[0], y.y * mk[1], y.z * mk[2], y.w * mk[3]);
                }
            } else {
                if (d_x) *reinterpret_cast<uint2 *>(d_x + row * DIM + col) = round4<typename Half16<DT>::elem>(y.x, y.y, y.z, y.w);
            }
        }
    }
    if (!partial) return;   // (workgroup-uniform)
    layernorm_bwd_flush<C>(ag, ab, partial, lane, wave);
}

// Second stage: column vc of partial [nblk][2 * dim] (gamma sums | beta sums) summed over the workgroups in a fixed order: four thread
// groups take a quarter of the workgroups each, then add up through LDS.
__global__ __launch_bounds__(256) void layernorm_bwd_reduce_kernel(const float *__restrict__ partial, int nblk, int dim,
                                                                  float *__restrict__ d_gamma, float *__restrict__ d_beta) {
    __shared__ float sh[4][64];
    const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int vc = blockIdx.x * 64 + c;   // < 2 * dim (the grid is 2 * dim / 64 workgroups)
    const int chunk = (nblk + 3) / 4;
    const int b0 = part * chunk, b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += partial[(int64_t)b * 2 * dim + vc];
    sh[part][c] = s;
    __syncthreads();
    if (part == 0) {
        const float t = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
        if (vc < dim) {
            if (d_gamma) d_gamma[vc] = t;
        } else if (d_beta) {
            d_beta[vc - dim] = t;
        }
    }
}

// ---- Embedding block backward (ccr_embed_layernorm_bwd_half): add_layernorm_bwd_kernel's row arithmetic on v = (word[id] + type[t]) +
// position[p], gathered and summed as embed_layernorm_kernel does, so mean and rstd are the forward's.  DROP = true: the block's dropout
// sits AFTER the LayerNorm, so the gradient that enters it is d_v = d_y * (keep ? inv_keep : 0); d gamma and d beta sum d_v.  d_x stays
// fp32 (it feeds ccr_embedding_grad).
template <int C, bool DROP = false>
__global__ __launch_bounds__(256) void embed_layernorm_bwd_kernel(const float *__restrict__ word, int64_t vocab,
                                                                 const float *__restrict__ pos_tab, int64_t n_pos,
                                                                 const float *__restrict__ type_tab, int64_t n_types,
                                                                 const int64_t *__restrict__ ids, const int64_t *__restrict__ pos,
                                                                 const int64_t *__restrict__ types, const float *__restrict__ gamma, float eps,
                                                                 const float *__restrict__ dy, float *__restrict__ d_x,
                                                                 float *__restrict__ partial, int64_t rows,
                                                                 typename KeepArg<DROP>::type keep = {}) {
    constexpr int DIM = 256 * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto clamp = [](int64_t v, int64_t n) { return v < 0 ? (int64_t)0 : (v >= n ? n - 1 : v); };
    float gm[C][4], ag[C][4], ab[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 t = *reinterpret_cast<const float4 *>(gamma + 4 * (64 * c + lane));
        gm[c][0] = t.x, gm[c][1] = t.y, gm[c][2] = t.z, gm[c][3] = t.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) ag[c][j] = ab[c][j] = 0.f;
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const float *w = word + clamp(ids[row], vocab) * DIM;
        const float *p = pos_tab + clamp(pos[row], n_pos) * DIM;
        const float *t = type_tab + clamp(types ? types[row] : 0, n_types) * DIM;
        float v[C][4], d[C][4];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int col = 4 * (64 * c + lane);
            const float4 a = *reinterpret_cast<const float4 *>(w + col);
            const float4 b = *reinterpret_cast<const float4 *>(t + col);
            const float4 e = *reinterpret_cast<const float4 *>(p + col);
            const float4 g = *reinterpret_cast<const float4 *>(dy + row * DIM + col);
            v[c][0] = (a.x + b.x) + e.x;
            v[c][1] = (a.y + b.y) + e.y;
            v[c][2] = (a.z + b.z) + e.z;
            v[c][3] = (a.w + b.w) + e.w;
            d[c][0] = g.x, d[c][1] = g.y, d[c][2] = g.z, d[c][3] = g.w;
            if constexpr (DROP) {
                float mk[4];
                keep_nibble(keep, row * (DIM / 32), 64 * c + lane, mk);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[c][j] *= mk[j];
            }
            sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
        }
        float mean, rstd, m1, m2;
        row_mean_rstd<C>(v, sum, eps, mean, rstd);
        layernorm_bwd_row<C>(v, d, gm, mean, rstd, ag, ab, m1, m2);
        if (d_x) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int col = 4 * (64 * c + lane);
                const float4 y = layernorm_bwd_dv<C>(v, d, gm, c, rstd, m1, m2);
                *reinterpret_cast<float4 *>(d_x + row * DIM + col) = y;
            }
        }
    }
    if (!partial) return;   // (workgroup-uniform)
    layernorm_bwd_flush<C>(ag, ab, partial, lane, wave);
}

// d_x = d_y (Phi(x) + x phi(x)) of the exact GELU, from the pre-activation: fp32, rounded once, 16 bytes per lane per access.
template <int DT>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const uint4 *__restrict__ x, const uint4 *__restrict__ dy, uint4 *__restrict__ dx,
                                                       int64_t n16) {
    typedef Half16<DT> HT;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const uint4 v = x[i], u = dy[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w}, q[4] = {u.x, u.y, u.z, u.w};
        float gr[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a[2] = {HT::lo(w[j]), HT::hi(w[j])}, ga[2] = {HT::lo(q[j]), HT::hi(q[j])};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float cdf = 0.5f * (1.f + erff(a[k] * 0.70710678118654752440f));
                const float pdf = 0.39894228040143267794f * expf(-0.5f * a[k] * a[k]);
                gr[2 * j + k] = ga[k] * fmaf(a[k], pdf, cdf);
            }
        }
        const uint2 r0 = round4<typename HT::elem>(gr[0], gr[1], gr[2], gr[3]), r1 = round4<typename HT::elem>(gr[4], gr[5], gr[6], gr[7]);
        dx[i] = make_uint4(r0.x, r0.y, r1.x, r1.y);
    }
}

static inline int bwd_lpad(int max_len) { return (max_len + BWD_TILE - 1) / BWD_TILE * BWD_TILE; }

template <int DT, bool DROP = false>
static int attention_bwd_any(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out, const int32_t *seq_start,
                             const int32_t *seq_len, uint16_t *d_qkv, int n_seq, int n_heads, int max_len, int pad_len, float scale,
                             float *delta, hipStream_t stream, typename KeepArg<DROP>::type keep_q = {},
                             typename KeepArg<DROP>::type keep_k = {}) {
    const int lpad = bwd_lpad(max_len);
    const size_t lds = attention_bwd_lds_bytes(lpad);
    // the opt-in is cached per (kernel, device): ask for the kernel's maximum (512 tokens) once
    int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&attention_bwd_kernel<DT, false, DROP>), attention_bwd_lds_bytes(BWD_MAX_LEN));
    if (rc != CCR_OK) return rc;
    rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&attention_bwd_kernel<DT, true, DROP>), attention_bwd_lds_bytes(BWD_MAX_LEN));
    if (rc != CCR_OK) return rc;
    int waves = lpad / BWD_TILE;
    if (waves > BWD_THREADS / 64) waves = BWD_THREADS / 64;
    const float scale_log2e = scale * 1.4426950408889634f;
    hipLaunchKernelGGL((attention_bwd_kernel<DT, false, DROP>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, out, d_out, lse, delta,
                       seq_start, seq_len, d_qkv, n_heads, pad_len, max_len, lpad, scale, scale_log2e, keep_q);
    CCR_LAUNCH_CHECK();
    hipLaunchKernelGGL((attention_bwd_kernel<DT, true, DROP>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, out, d_out, lse, delta,
                       seq_start, seq_len, d_qkv, n_heads, pad_len, max_len, lpad, scale, scale_log2e, keep_k);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

template <int DT>
static int gelu_bwd_any(const uint16_t *x, const uint16_t *dy, uint16_t *dx, int64_t n, hipStream_t stream) {
    const int64_t n16 = n / 8;
    int64_t blocks = (n16 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(gelu_bwd_kernel<DT>, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(x),
                       reinterpret_cast<const uint4 *>(dy), reinterpret_cast<uint4 *>(dx), n16);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

}  // namespace ccr

using namespace ccr;

extern "C" size_t ccr_attention_bwd_workspace_bytes(int n_seq, int n_heads, int max_len) {
    if (n_seq < 0 || n_seq > 65535 || n_heads <= 0 || n_heads > 1024 || max_len <= 0 || max_len > BWD_MAX_LEN) {
        set_error("ccr_attention_bwd_workspace_bytes: n_seq=%d n_heads=%d max_len=%d", n_seq, n_heads, max_len);
        return 0;
    }
    const size_t need = (size_t)n_seq * n_heads * bwd_lpad(max_len) * sizeof(float);
    return need ? need : sizeof(float);
}

// ---- The implementations behind the exported pairs: null bits pointers mean no dropout.  Each reports its errors under the exported
// function's name `who`; every check runs before any launch.

static int attention_bwd(const char *who, const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out,
                         const int32_t *seq_start, const int32_t *seq_len, const uint32_t *keep_q, const uint32_t *keep_k, float inv_keep,
                         uint16_t *d_qkv, int n_seq, int n_heads, int max_len, int pad_len, float scale, int half_dtype, void *workspace,
                         size_t workspace_bytes, hipStream_t s) {
    if (const int rc = check_attention_shape(who, half_dtype, n_seq, n_heads, max_len, pad_len, scale)) return rc;
    if (keep_q)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    const size_t need = ccr_attention_bwd_workspace_bytes(n_seq, n_heads, max_len);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
        return CCR_ERR_WORKSPACE;
    }
    CCR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: 4-byte aligned workspace", who);
    if (n_seq == 0) return CCR_OK;
    float *delta = static_cast<float *>(workspace);
    const int W = (max_len + 31) / 32;
    return dispatch_half(half_dtype, [&](auto dt) {
        return dispatch_drop(keep_q != nullptr, [&](auto drop) {
            constexpr bool DROP = decltype(drop)::value;
            return attention_bwd_any<decltype(dt)::value, DROP>(qkv, out, lse, d_out, seq_start, seq_len, d_qkv, n_seq, n_heads, max_len, pad_len,
                                                               scale, delta, s, keep_arg<DROP>(keep_q, inv_keep, W),
                                                               keep_arg<DROP>(keep_k, inv_keep, W));
        });
    });
}

// The plan of a LayerNorm backward, for its three entry points: at most LN_BWD_MAX_BLOCKS workgroups walk the rows; when d gamma or d beta
// is wanted, the workgroups' sums go through the workspace partial [nblk][2][dim] and layernorm_bwd_reduce_kernel adds them up.
// launch(partial, nblk) starts the row kernel (partial is null when no parameter gradient is wanted).
template <class Launch>
static int layernorm_bwd_run(const char *who, bool wants_dx, float *d_gamma, float *d_beta, int64_t rows, int dim, void *workspace,
                             size_t workspace_bytes, hipStream_t s, Launch &&launch) {
    const bool params = d_gamma || d_beta;
    int64_t nblk = (rows + 3) / 4;
    if (nblk > LN_BWD_MAX_BLOCKS) nblk = LN_BWD_MAX_BLOCKS;
    const size_t need = params ? (size_t)nblk * 2 * dim * sizeof(float) : 0;
    if (need && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
        return CCR_ERR_WORKSPACE;
    }
    CCR_REQUIRE(!need || (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: 16-byte aligned workspace", who);
    if (!wants_dx && !params) return CCR_OK;
    if (rows == 0) {   // sums over no rows
        if (d_gamma) CCR_HIP_CHECK(hipMemsetAsync(d_gamma, 0, (size_t)dim * sizeof(float), s));
        if (d_beta) CCR_HIP_CHECK(hipMemsetAsync(d_beta, 0, (size_t)dim * sizeof(float), s));
        return CCR_OK;
    }
    float *partial = params ? static_cast<float *>(workspace) : nullptr;
    const int rc = launch(partial, (int)nblk);
    if (rc != CCR_OK || !params) return rc;
    hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3((unsigned)(2 * dim / 64)), dim3(256), 0, s, partial, (int)nblk, dim, d_gamma, d_beta);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

static int add_layernorm_bwd(const char *who, const uint16_t *x, const uint32_t *bits, float inv_keep, const float *res, const float *gamma,
                             float eps, const float *dy, float *d_res, uint16_t *d_x, float *d_gamma, float *d_beta, int64_t rows, int dim,
                             int half_dtype, void *workspace, size_t workspace_bytes, hipStream_t s) {
    if (const int rc = check_half(who, half_dtype)) return rc;
    if (const int rc = check_rows_dim(who, rows, dim)) return rc;
    if (bits)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    return layernorm_bwd_run(who, d_res || d_x, d_gamma, d_beta, rows, dim, workspace, workspace_bytes, s, [&](float *partial, int nblk) {
        return dispatch_width(dim, [&](auto c) {
            return dispatch_half(half_dtype, [&](auto dt) {
                return dispatch_drop(bits != nullptr, [&](auto drop) {
                    constexpr bool DROP = decltype(drop)::value;
                    return launch_row_kernel(add_layernorm_bwd_kernel<decltype(c)::value, decltype(dt)::value, DROP>, nblk, s, x, res, gamma, eps, dy,
                                         d_res, d_x, partial, rows, keep_arg<DROP>(bits, inv_keep, 0));
                });
            });
        });
    });
}

extern "C" int ccr_attention_bwd_half(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out,
                                      const int32_t *seq_start, const int32_t *seq_len, uint16_t *d_qkv, int n_seq, int n_heads,
                                      int max_len, int pad_len, float scale, int half_dtype, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    CCR_REQUIRE(qkv && out && lse && d_out && seq_start && seq_len && d_qkv && workspace, "ccr_attention_bwd_half: null pointer");
    return attention_bwd("ccr_attention_bwd_half", qkv, out, lse, d_out, seq_start, seq_len, nullptr, nullptr, 1.f, d_qkv, n_seq, n_heads, max_len,
                         pad_len, scale, half_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ccr_attention_bwd_drop_half(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *d_out,
                                           const int32_t *seq_start, const int32_t *seq_len, const uint32_t *keep_q, const uint32_t *keep_k,
                                           float inv_keep, uint16_t *d_qkv, int n_seq, int n_heads, int max_len, int pad_len, float scale,
                                           int half_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    CCR_REQUIRE(qkv && out && lse && d_out && seq_start && seq_len && keep_q && keep_k && d_qkv && workspace,
                "ccr_attention_bwd_drop_half: null pointer");
    return attention_bwd("ccr_attention_bwd_drop_half", qkv, out, lse, d_out, seq_start, seq_len, keep_q, keep_k, inv_keep, d_qkv, n_seq, n_heads,
                         max_len, pad_len, scale, half_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ccr_add_layernorm_bwd_drop_half(const uint16_t *x_half, const uint32_t *bits, float inv_keep, const float *residual,
                                               const float *gamma, float eps, const float *d_y, float *d_res, uint16_t *d_x, float *d_gamma,
                                               float *d_beta, int64_t rows, int dim, int half_dtype, void *workspace, size_t workspace_bytes,
                                               void *stream) {
    CCR_REQUIRE(x_half && bits && gamma && d_y, "ccr_add_layernorm_bwd_drop_half: null pointer");
    return add_layernorm_bwd("ccr_add_layernorm_bwd_drop_half", x_half, bits, inv_keep, residual, gamma, eps, d_y, d_res, d_x, d_gamma, d_beta, rows,
                             dim, half_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ccr_add_layernorm_bwd_half(const uint16_t *x_half, const float *residual, const float *gamma, float eps, const float *d_y,
                                          float *d_res, uint16_t *d_x, float *d_gamma, float *d_beta, int64_t rows, int dim,
                                          int half_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    CCR_REQUIRE(x_half && gamma && d_y, "ccr_add_layernorm_bwd_half: null pointer");
    return add_layernorm_bwd("ccr_add_layernorm_bwd_half", x_half, nullptr, 1.f, residual, gamma, eps, d_y, d_res, d_x, d_gamma, d_beta, rows, dim,
                             half_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ccr_embed_layernorm_bwd_half(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions,
                                            const float *type_table, int64_t n_types, const int64_t *token_ids, const int64_t *positions,
                                            const int64_t *token_types, const float *gamma, float eps, const uint32_t *bits, float inv_keep,
                                            const float *d_y, float *d_x, float *d_gamma, float *d_beta, int64_t rows, int dim,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    static const char who[] = "ccr_embed_layernorm_bwd_half";
    CCR_REQUIRE(word_table && position_table && type_table && token_ids && positions && gamma && d_y,
                "ccr_embed_layernorm_bwd_half: null pointer");
    CCR_REQUIRE(vocab > 0 && n_positions > 0 && n_types > 0, "ccr_embed_layernorm_bwd_half: empty table");
    if (const int rc = check_rows_dim(who, rows, dim)) return rc;
    if (bits)
        if (const int rc = check_inv_keep(who, inv_keep)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return layernorm_bwd_run(who, d_x != nullptr, d_gamma, d_beta, rows, dim, workspace, workspace_bytes, s, [&](float *partial, int nblk) {
        return dispatch_width(dim, [&](auto c) {
            return dispatch_drop(bits != nullptr, [&](auto drop) {
                constexpr bool DROP = decltype(drop)::value;
                return launch_row_kernel(embed_layernorm_bwd_kernel<decltype(c)::value, DROP>, nblk, s, word_table, vocab, position_table, n_positions,
                                     type_table, n_types, token_ids, positions, token_types, gamma, eps, d_y, d_x, partial, rows,
                                     keep_arg<DROP>(bits, inv_keep, 0));
            });
        });
    });
}

extern "C" int ccr_gelu_bwd_half(const uint16_t *x, const uint16_t *d_y, uint16_t *d_x, int64_t n, int half_dtype, void *stream) {
    CCR_REQUIRE(x && d_y && d_x, "ccr_gelu_bwd_half: null pointer");
    if (const int rc = check_half("ccr_gelu_bwd_half", half_dtype)) return rc;
    CCR_REQUIRE(n >= 0 && n % 8 == 0, "ccr_gelu_bwd_half: n=%lld (a multiple of 8 elements)", (long long)n);
    CCR_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_x)) & 15) == 0,
                "ccr_gelu_bwd_half: 16-byte aligned arrays");
    if (n == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) { return gelu_bwd_any<decltype(dt)::value>(x, d_y, d_x, n, (hipStream_t)stream); });
}
