// ccr_optim.hip -- the fine-tune step's optimizer: one multi-tensor AdamW pass over fp32 master weights that also writes the 16-bit
// copies the encoder's layer kernels read (FusedBertEncoder's wqkv / wo / wi / wo2 and their biases), so no forward casts a weight again.
// Replaces: torch.optim.AdamW in the reference's configure_optimizers (src/ccrec/models/bert_mt.py:115-146) and the per-forward
// torch.cat(...).to(half) / .to(half) of FusedBertEncoder._layers_forward_train.
//
//   adamw_kernel    one workgroup of 256 threads per 4096-element chunk of one segment (parameter tensor); the segments of a launch and the
//                   prefix of their chunk counts travel in the kernel arguments (ccr_optim_plan.h), the grid is capped at 2048 workgroups
//                   and strides over the remaining chunks.  28 bytes per element move (p, g, m, v read; p, m, v written) + 2 for a shadow.
//
// Arithmetic (restated in ccrec_amd/optim_ref.py bit for bit): every operation fp32, rounded to nearest, NOT contracted, the
// divide and the square root correctly rounded (hipcc's default for HIP; contraction is switched off below):
//   p1 = p * decay;  m' = m + w1 * (g - m);  v' = v * b2 + (w2 * g) * g;  d = sqrt(v') / bc2_sqrt + eps;  p' = p1 - step_size * (m' / d)
//   shadow = p' rounded to nearest even in bf16 / fp16
#pragma clang fp contract(off)
#include <hip/hip_fp16.h>
#include <math.h>

#include "ccr_common.h"
#include "ccr_optim_plan.h"

namespace ccr {
namespace optim {

struct Scalars {
    float decay, step_size, bc2_sqrt, w1, b2, w2, eps;
};

__device__ __forceinline__ void adamw_element(float &p, const float g, float &m, float &v, const Scalars &s) {
    const float p1 = p * s.decay;
    const float gm = g - m;
    const float m1 = m + s.w1 * gm;
    const float wg = s.w2 * g;
    const float v1 = v * s.b2 + wg * g;
    const float d = sqrtf(v1) / s.bc2_sqrt + s.eps;
    const float q = m1 / d;
    p = p1 - s.step_size * q;
    m = m1;
    v = v1;
}

// round to nearest even; a NaN stays a (quiet) NaN of its sign
__device__ __forceinline__ uint16_t bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ uint16_t fp16_rne(float f) { return __half_as_ushort(__float2half_rn(f)); }

template <int SHADOW>   // 0 none, SEG_SHADOW_BF16, SEG_SHADOW_FP16
__device__ __forceinline__ uint16_t shadow_bits(float f) {
    return SHADOW == SEG_SHADOW_BF16 ? bf16_rne(f) : fp16_rne(f);
}

// elements [begin, end) of one segment, one at a time (a segment on odd addresses, or the last n % 4 elements of an aligned one)
template <int SHADOW>
__device__ __forceinline__ void chunk_scalar(const SegArg &a, const Scalars &s, int64_t begin, int64_t end) {
    for (int64_t i = begin + threadIdx.x; i < end; i += THREADS) {
        float p = a.param[i], m = a.exp_avg[i], v = a.exp_avg_sq[i];
        adamw_element(p, a.grad[i], m, v, s);
        a.param[i] = p;
        a.exp_avg[i] = m;
        a.exp_avg_sq[i] = v;
        if (SHADOW) static_cast<uint16_t *>(a.shadow)[i] = shadow_bits<SHADOW>(p);
    }
}

// groups of four elements [begin / 4, end4) of a segment whose pointers allow 16-byte accesses (8-byte ones on the shadow)
template <int SHADOW>
__device__ __forceinline__ void chunk_vec4(const SegArg &a, const Scalars &s, int64_t begin4, int64_t end4) {
    float4 *__restrict__ P = reinterpret_cast<float4 *>(a.param);
    const float4 *__restrict__ G = reinterpret_cast<const float4 *>(a.grad);
    float4 *__restrict__ M = reinterpret_cast<float4 *>(a.exp_avg);
    float4 *__restrict__ V = reinterpret_cast<float4 *>(a.exp_avg_sq);
#pragma unroll 2
    for (int64_t i = begin4 + threadIdx.x; i < end4; i += THREADS) {
        float4 p = P[i], m = M[i], v = V[i];
        const float4 g = G[i];
        adamw_element(p.x, g.x, m.x, v.x, s);
        adamw_element(p.y, g.y, m.y, v.y, s);
        adamw_element(p.z, g.z, m.z, v.z, s);
        adamw_element(p.w, g.w, m.w, v.w, s);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (SHADOW) {
            uint2 h;
            h.x = (uint32_t)shadow_bits<SHADOW>(p.x) | ((uint32_t)shadow_bits<SHADOW>(p.y) << 16);
            h.y = (uint32_t)shadow_bits<SHADOW>(p.z) | ((uint32_t)shadow_bits<SHADOW>(p.w) << 16);
            static_cast<uint2 *>(a.shadow)[i] = h;
        }
    }
}

template <int SHADOW>
__device__ __forceinline__ void chunk(const SegArg &a, const Scalars &s, int64_t begin, int64_t end) {
    if (a.flags & SEG_VEC4) {      // (begin is a multiple of CHUNK: the 16-byte alignment of the bases carries over)
        const int64_t end4 = begin + ((end - begin) & ~(int64_t)3);
        chunk_vec4<SHADOW>(a, s, begin >> 2, end4 >> 2);
        chunk_scalar<SHADOW>(a, s, end4, end);
    } else {
        chunk_scalar<SHADOW>(a, s, begin, end);
    }
}

__global__ __launch_bounds__(THREADS) void adamw_kernel(const Batch b) {
    const uint32_t total = b.prefix[b.n_seg];
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int si = find_segment(b.prefix, b.n_seg, c);      // block-uniform
        const SegArg &a = b.seg[si];
        const int64_t begin = (int64_t)(c - b.prefix[si]) * CHUNK;
        const int64_t end = begin + CHUNK < a.n ? begin + CHUNK : a.n;
        const Scalars s = {a.decay, a.step_size, a.bc2_sqrt, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.eps};
        if (a.flags & SEG_SHADOW_BF16)
            chunk<SEG_SHADOW_BF16>(a, s, begin, end);
        else if (a.flags & SEG_SHADOW_FP16)
            chunk<SEG_SHADOW_FP16>(a, s, begin, end);
        else
            chunk<0>(a, s, begin, end);
    }
}

}  // namespace optim
}  // namespace ccr

using namespace ccr;

extern "C" int ccr_adamw_step(const ccr_adamw_segment *segments, int n_segments, float one_minus_beta1, float beta2, float one_minus_beta2,
                              float eps, void *stream) {
    CCR_REQUIRE(n_segments >= 0, "ccr_adamw_step: n_segments=%d", n_segments);
    if (n_segments == 0) return CCR_OK;
    CCR_REQUIRE(segments != nullptr, "ccr_adamw_step: segments is NULL (n_segments=%d)", n_segments);
    for (int i = 0; i < n_segments; ++i) {      // everything is checked before anything is launched: a refused call changes nothing
        const char *why = optim::segment_error(segments[i]);
        CCR_REQUIRE(why == nullptr, "ccr_adamw_step: segment %d (n=%lld): %s", i, (long long)segments[i].n, why);
    }
    optim::Batch batch = {};
    batch.one_minus_beta1 = one_minus_beta1, batch.beta2 = beta2, batch.one_minus_beta2 = one_minus_beta2, batch.eps = eps;
    int cursor = 0;
    while (const uint32_t chunks = optim::next_batch(segments, n_segments, cursor, batch)) {
        hipLaunchKernelGGL(optim::adamw_kernel, dim3(optim::grid_for(chunks)), dim3(optim::THREADS), 0, (hipStream_t)stream, batch);
        CCR_LAUNCH_CHECK();
    }
    return CCR_OK;
}
