// ccr_encoder_common.h -- what the encoder layer's forward (ccr_encoder.hip) and backward (ccr_encoder_bwd.hip) kernels share:
// the two 16-bit operand types, the rounding of four fp32 values, and the LayerNorm's two-step mean.
#pragma once

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

#define CCR_REQUIRE_HALF(dtype, who) \
    CCR_REQUIRE((dtype) == CCR_DTYPE_BF16 || (dtype) == CCR_DTYPE_F16, who ": half_dtype=%d (CCR_DTYPE_F16 or CCR_DTYPE_BF16)", (int)(dtype))

}  // namespace ccr
