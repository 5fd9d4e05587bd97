// ccr_encoder_common.h -- what the encoder layer's forward (ccr_encoder.hip) and backward (ccr_encoder_bwd.hip) kernels share:
// the two 16-bit operand types, the rounding of four fp32 values, the LayerNorm row body (statistics, backward row step, partial-sum
// flush) that the add_ and embed_ kernels of both files run on a row held in registers, and the host side's dispatchers and checks.
#pragma once

#include <type_traits>

#include "ccr_common.h"

namespace ccr {

typedef __bf16 ebf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ef16x8 __attribute__((ext_vector_type(8)));
typedef float ef32x16 __attribute__((ext_vector_type(16)));

// The layer's 16-bit operand type: bf16 or fp16 -- whichever the caller's autocast context names (the reference's
// torch.cuda.amp.autocast() at scripts/al_0_rank.py:125 is fp16).  Same kernels, same MFMA rate (v_mfma_f32_32x32x16_f16 /
// _bf16), fp32 scores / softmax / residual stream / LayerNorm either way; only the rounding of the 16-bit operands differs.
template <int DT>
struct Half16;
template <>
struct Half16<CCR_DTYPE_BF16> {
    typedef __bf16 elem;
    typedef ebf16x8 vec8;
    static __device__ __forceinline__ ef32x16 mfma(vec8 a, vec8 b, ef32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float lo(uint32_t w) { return __uint_as_float(w << 16); }
    static __device__ __forceinline__ float hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
};
template <>
struct Half16<CCR_DTYPE_F16> {
    typedef _Float16 elem;
    typedef ef16x8 vec8;
    static __device__ __forceinline__ ef32x16 mfma(vec8 a, vec8 b, ef32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ float lo(uint32_t w) {
        union {
            uint32_t u;
            _Float16 h[2];
        } x;
        x.u = w;
        return (float)x.h[0];
    }
    static __device__ __forceinline__ float hi(uint32_t w) {
        union {
            uint32_t u;
            _Float16 h[2];
        } x;
        x.u = w;
        return (float)x.h[1];
    }
};
// four fp32 values -> four 16-bit values (round to nearest even; a NaN stays a NaN), 8 bytes
template <class E>
__device__ __forceinline__ uint2 round4(float a, float b, float c, float d) {
    union {
        E h[4];
        uint2 u;
    } w;
    w.h[0] = (E)a;
    w.h[1] = (E)b;
    w.h[2] = (E)c;
    w.h[3] = (E)d;
    return w.u;
}

typedef short es16x4 __attribute__((ext_vector_type(4)));

// The mean of a row held in registers (v[c][j] per lane), from a first estimate m0 = sum / DIM: one correction step m0 + mean(v - m0).
// The fp32 sum of DIM elements leaves m0 an ulp or so off, which is harmless next to a variance but IS the whole deviation of a row
// whose elements are all equal: there v - m0 is a few ulps, exactly, its sum is exact, and the corrected mean is v itself -- the row
// normalises to beta for every eps, where the uncorrected mean left gamma (v - m0) / sqrt(eps): 0.18 to 1.0 gamma at eps = 1e-12, by width.
template <int C>
__device__ __forceinline__ float refined_mean(const float (&v)[C][4], float m0) {
    float sd = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) sd += ((v[c][0] - m0) + (v[c][1] - m0)) + ((v[c][2] - m0) + (v[c][3] - m0));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    return m0 + sd * (1.f / (256 * C));
}

// ---- The LayerNorm row body.  A wave holds one row of DIM = 256 C elements, v[c][j] = element 4 (64 c + lane) + j.  Each kernel loads its
// own operands into v (and d = d_y), applies its own dropout and stores its own outputs; what lies between is the same arithmetic, in the
// same order, for all four row kernels -- written once here, so that the forward's and the backward's mean and rstd cannot drift apart.

// mean and rstd of the row from the lane's partial sum of its elements: butterfly sum, refined mean, squared deviations, rsqrt
template <int C>
__device__ __forceinline__ void row_mean_rstd(const float (&v)[C][4], float sum, float eps, float &mean, float &rstd) {
    constexpr int DIM = 256 * C;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    mean = refined_mean<C>(v, sum * (1.f / DIM));
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = v[c][j] - mean;
            sq = fmaf(d, d, sq);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    rstd = rsqrtf(sq * (1.f / DIM) + eps);
}

// slice c of y = xhat gamma + beta
template <int C>
__device__ __forceinline__ float4 layernorm_row_out(const float (&v)[C][4], int c, float mean, float rstd, float4 gm, float4 bt) {
    float4 y;
    y.x = fmaf((v[c][0] - mean) * rstd, gm.x, bt.x);
    y.y = fmaf((v[c][1] - mean) * rstd, gm.y, bt.y);
    y.z = fmaf((v[c][2] - mean) * rstd, gm.z, bt.z);
    y.w = fmaf((v[c][3] - mean) * rstd, gm.w, bt.w);
    return y;
}

// One row of the backward: v (the summed input) becomes xhat = (v - mean) rstd, the row's d_y (d) joins ag / ab, and m1 = mean(d gamma),
// m2 = mean(d gamma xhat) come back for layernorm_bwd_dv.
template <int C>
__device__ __forceinline__ void layernorm_bwd_row(float (&v)[C][4], const float (&d)[C][4], const float (&gm)[C][4], float mean, float rstd,
                                                  float (&ag)[C][4], float (&ab)[C][4], float &m1, float &m2) {
    constexpr int DIM = 256 * C;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (v[c][j] - mean) * rstd;
            const float gy = d[c][j] * gm[c][j];
            v[c][j] = xh;
            s1 += gy;
            s2 = fmaf(gy, xh, s2);
            ag[c][j] = fmaf(d[c][j], xh, ag[c][j]);
            ab[c][j] += d[c][j];
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    m1 = s1 * (1.f / DIM), m2 = s2 * (1.f / DIM);
}

// slice c of d_v = rstd (d gamma - m1 - xhat m2), xhat as layernorm_bwd_row left it
template <int C>
__device__ __forceinline__ float4 layernorm_bwd_dv(const float (&xhat)[C][4], const float (&d)[C][4], const float (&gm)[C][4], int c,
                                                   float rstd, float m1, float m2) {
    float4 y;
    y.x = rstd * ((d[c][0] * gm[c][0] - m1) - xhat[c][0] * m2);
    y.y = rstd * ((d[c][1] * gm[c][1] - m1) - xhat[c][1] * m2);
    y.z = rstd * ((d[c][2] * gm[c][2] - m1) - xhat[c][2] * m2);
    y.w = rstd * ((d[c][3] * gm[c][3] - m1) - xhat[c][3] * m2);
    return y;
}

// The workgroup's four waves add their ag, then their ab, through LDS in a fixed order (wave 0 adds waves 1, 2, 3), and the sums go to
// partial [gridDim.x][2][DIM].  Every wave of the workgroup calls this (it holds barriers).  red is declared here, not handed in by the
// kernel: with the array as a parameter add_layernorm_bwd_kernel<3, *, true> went from 128 to 130 VGPRs and lost an occupancy step.
template <int C>
__device__ __forceinline__ void layernorm_bwd_flush(const float (&ag)[C][4], const float (&ab)[C][4], float *partial, int lane, int wave) {
    constexpr int DIM = 256 * C;
    __shared__ float red[3][DIM];
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        if (which) __syncthreads();
        if (wave > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                *reinterpret_cast<float4 *>(&red[wave - 1][4 * (64 * c + lane)]) =
                    which ? make_float4(ab[c][0], ab[c][1], ab[c][2], ab[c][3]) : make_float4(ag[c][0], ag[c][1], ag[c][2], ag[c][3]);
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int col = 4 * (64 * c + lane);
                float4 t = which ? make_float4(ab[c][0], ab[c][1], ab[c][2], ab[c][3]) : make_float4(ag[c][0], ag[c][1], ag[c][2], ag[c][3]);
#pragma unroll
                for (int w = 0; w < 3; ++w) {
                    const float4 u = *reinterpret_cast<const float4 *>(&red[w][col]);
                    t.x += u.x, t.y += u.y, t.z += u.z, t.w += u.w;
                }
                *reinterpret_cast<float4 *>(partial + ((int64_t)blockIdx.x * 2 + which) * DIM + col) = t;
            }
        }
    }
}

// Training dropout (ccr_dropout.hip writes the bits): a kernel instantiated with DROP = true takes the packed keep bits of its site and
// the scale 1 / (1 - p_eff) of a kept element; DROP = false takes an empty struct in their place, as NoLse does for lse -- the
// dropout-free instantiations keep their argument layout and their code.
struct NoKeep {};
struct KeepBits {
    const uint32_t *bits;   // row-wise sites: [rows][dim / 32]; attention: keep_q (forward, dQ pass) or keep_k (dK / dV pass) [T][H][W]
    float inv_keep;
    int W;                  // attention only: words per (token row, head) = ceil(max_len / 32)
};
template <bool DROP>
struct KeepArg {
    typedef NoKeep type;
};
template <>
struct KeepArg<true> {
    typedef KeepBits type;
};

// row-wise sites: the factors of the four columns 4 u .. 4 u + 3 (u = 64 c + lane) of the row whose words start at bits[word0]
__device__ __forceinline__ void keep_nibble(const KeepBits &keep, int64_t word0, int u, float (&mk)[4]) {
    const uint32_t nib = keep.bits[word0 + (u >> 3)] >> (4 * (u & 7));
#pragma unroll
    for (int j = 0; j < 4; ++j) mk[j] = (nib >> j) & 1u ? keep.inv_keep : 0.f;
}

// the argument a <.., DROP> kernel takes for a site whose bits pointer may be null (DROP = false: nothing)
template <bool DROP>
inline typename KeepArg<DROP>::type keep_arg(const uint32_t *bits, float inv_keep, int W) {
    if constexpr (DROP)
        return KeepBits{bits, inv_keep, W};
    else
        return NoKeep{};
}

// (ccr_dropout.hip spells its 16-bit type check with this macro; the encoder files use check_half below: one text, two callers)
#define CCR_REQUIRE_HALF(dtype, who) \
    CCR_REQUIRE((dtype) == CCR_DTYPE_BF16 || (dtype) == CCR_DTYPE_F16, who ": half_dtype=%d (CCR_DTYPE_F16 or CCR_DTYPE_BF16)", (int)(dtype))

// ---- Host side: a run-time width, 16-bit type or dropout flag becomes a template argument in ONE place each.  f is a generic lambda
// whose parameter is a std::integral_constant (read its ::value); it returns the launch's status.
template <class F>
inline int dispatch_width(int dim, F &&f) {   // dim = 256 C, C = 1 .. 8 (the caller has checked)
    switch (dim / 256) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}
// (dispatch_half: ccr_common.h -- the search kernels resolve their element type with it too)
template <class F>
inline int dispatch_drop(bool drop, F &&f) {
    return drop ? f(std::true_type{}) : f(std::false_type{});
}

// the launch of a row kernel: nblk workgroups of four waves, one row per wave at a time
template <class K, class... A>
inline int launch_row_kernel(K kernel, int64_t nblk, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, s, args...);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

// The argument checks that entry points share, reported under the caller's name `who`.
// (check_half: ccr_common.h)
inline int check_inv_keep(const char *who, float inv_keep) {
    CCR_REQUIRE(inv_keep >= 1.f && inv_keep <= 65536.f, "%s: inv_keep=%g (1 .. 65536)", who, (double)inv_keep);
    return CCR_OK;
}
inline int check_rows_dim(const char *who, int64_t rows, int dim) {   // the row kernels: one wave per row of 256 C elements
    CCR_REQUIRE(rows >= 0 && dim > 0 && dim % 256 == 0 && dim <= 2048,
                "%s: rows=%lld dim=%d (dim %% 256 == 0, dim <= 2048: the rule of the keep-bit, training and backward row kernels)", who,
                (long long)rows, dim);
    return CCR_OK;
}
// the inference row kernels (no keep bits): also the odd multiples of 128 from 384 on, one wave per row of 128 P elements
// (ccr_encoder_h32.hip); a row of 128 stays refused, as it always was (tests/test_gpu_row_kernels.py pins that)
inline int check_rows_dim_infer(const char *who, int64_t rows, int dim) {
    CCR_REQUIRE(rows >= 0 && dim >= 256 && dim % 128 == 0 && dim <= 2048,
                "%s: rows=%lld dim=%d (dim %% 128 == 0, 256 <= dim <= 2048: the rule of the inference row kernels, no keep bits)", who,
                (long long)rows, dim);
    return CCR_OK;
}
// The inference row kernels at dim = 128 P, P = 3, 5 .. 15 (ccr_encoder_h32.hip); the callers (ccr_encoder.hip) have checked every argument.
int add_layernorm_odd128(const uint16_t *x, const float *res, const float *gamma, const float *beta, float eps, float *out_f32,
                         uint16_t *out_half, int64_t rows, int dim, int half_dtype, hipStream_t s);
int embed_layernorm_odd128(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions, const float *type_table,
                           int64_t n_types, const int64_t *token_ids, const int64_t *positions, const int64_t *token_types,
                           const float *gamma, const float *beta, float eps, float *out_f32, uint16_t *out_half, int64_t rows, int dim,
                           int half_dtype, hipStream_t s);
inline int check_attention_shape(const char *who, int half_dtype, int n_seq, int n_heads, int max_len, int pad_len, float scale) {
    if (const int rc = check_half(who, half_dtype)) return rc;
    CCR_REQUIRE(n_seq >= 0 && n_seq <= 65535 && n_heads > 0 && n_heads <= 1024, "%s: bad shape n_seq=%d n_heads=%d", who, n_seq, n_heads);
    CCR_REQUIRE(max_len > 0 && max_len <= 512 && pad_len >= 0 && pad_len <= 512, "%s: max_len=%d pad_len=%d (1..512 tokens per sequence)", who,
                max_len, pad_len);
    CCR_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
    return CCR_OK;
}

}  // namespace ccr
