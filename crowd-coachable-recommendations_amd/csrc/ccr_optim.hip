// ccr_optim.hip -- the fine-tune step's optimizer: one multi-tensor AdamW pass over fp32 master weights that also writes the 16-bit
// copies the encoder's layer kernels read (FusedBertEncoder's wqkv / wo / wi / wo2 and their biases), so no forward casts a weight again.
// Replaces: torch.optim.AdamW in the reference's configure_optimizers (src/ccrec/models/bert_mt.py:115-146) and the per-forward
// torch.cat(...).to(half) / .to(half) of FusedBertEncoder._layers_forward_train.
//
//   (ccr_adamw_step_scaled: the same pass under a control block in device memory -- loss scale, overflow skip, global-norm clip -- which
//    grad_stats_kernel's read-only pass and control_update_kernel's single workgroup fill first; include/ccr_retrieval.h has the definition.)
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

// SCALED: the gradient is multiplied by the control block's coef first (one fp32 multiply, rounded; contraction is off in this file)
template <bool SCALED>
__device__ __forceinline__ float scaled(const float g, const float coef) {
    return SCALED ? g * coef : g;
}

// elements [begin, end) of one segment, one at a time (a segment on odd addresses, or the last n % 4 elements of an aligned one)
template <int SHADOW, bool SCALED>
__device__ __forceinline__ void chunk_scalar(const SegArg &a, const Scalars &s, const float coef, int64_t begin, int64_t end) {
    for (int64_t i = begin + threadIdx.x; i < end; i += THREADS) {
        float p = a.param[i], m = a.exp_avg[i], v = a.exp_avg_sq[i];
        adamw_element(p, scaled<SCALED>(a.grad[i], coef), m, v, s);
        a.param[i] = p;
        a.exp_avg[i] = m;
        a.exp_avg_sq[i] = v;
        if (SHADOW) static_cast<uint16_t *>(a.shadow)[i] = shadow_bits<SHADOW>(p);
    }
}

// groups of four elements [begin / 4, end4) of a segment whose pointers allow 16-byte accesses (8-byte ones on the shadow)
template <int SHADOW, bool SCALED>
__device__ __forceinline__ void chunk_vec4(const SegArg &a, const Scalars &s, const float coef, int64_t begin4, int64_t end4) {
    float4 *__restrict__ P = reinterpret_cast<float4 *>(a.param);
    const float4 *__restrict__ G = reinterpret_cast<const float4 *>(a.grad);
    float4 *__restrict__ M = reinterpret_cast<float4 *>(a.exp_avg);
    float4 *__restrict__ V = reinterpret_cast<float4 *>(a.exp_avg_sq);
#pragma unroll 2
    for (int64_t i = begin4 + threadIdx.x; i < end4; i += THREADS) {
        float4 p = P[i], m = M[i], v = V[i];
        const float4 g = G[i];
        adamw_element(p.x, scaled<SCALED>(g.x, coef), m.x, v.x, s);
        adamw_element(p.y, scaled<SCALED>(g.y, coef), m.y, v.y, s);
        adamw_element(p.z, scaled<SCALED>(g.z, coef), m.z, v.z, s);
        adamw_element(p.w, scaled<SCALED>(g.w, coef), m.w, v.w, s);
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

template <int SHADOW, bool SCALED>
__device__ __forceinline__ void chunk(const SegArg &a, const Scalars &s, const float coef, int64_t begin, int64_t end) {
    if (a.flags & SEG_VEC4) {      // (begin is a multiple of CHUNK: the 16-byte alignment of the bases carries over)
        const int64_t end4 = begin + ((end - begin) & ~(int64_t)3);
        chunk_vec4<SHADOW, SCALED>(a, s, coef, begin >> 2, end4 >> 2);
        chunk_scalar<SHADOW, SCALED>(a, s, coef, end4, end);
    } else {
        chunk_scalar<SHADOW, SCALED>(a, s, coef, begin, end);
    }
}

// every chunk of a launch, a workgroup striding over them (the body of both step kernels: a macro, not a function, so that adamw_kernel
// compiles to the instructions it had before the scaled form existed)
#define CCR_ADAMW_CHUNKS(SCALED, coef)                                                                                   \
    const uint32_t total = b.prefix[b.n_seg];                                                                            \
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {                                                           \
        const int si = find_segment(b.prefix, b.n_seg, c); /* block-uniform */                                           \
        const SegArg &a = b.seg[si];                                                                                     \
        const int64_t begin = (int64_t)(c - b.prefix[si]) * CHUNK;                                                       \
        const int64_t end = begin + CHUNK < a.n ? begin + CHUNK : a.n;                                                   \
        const Scalars s = {a.decay, a.step_size, a.bc2_sqrt, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.eps};      \
        if (a.flags & SEG_SHADOW_BF16)                                                                                   \
            chunk<SEG_SHADOW_BF16, SCALED>(a, s, coef, begin, end);                                                      \
        else if (a.flags & SEG_SHADOW_FP16)                                                                              \
            chunk<SEG_SHADOW_FP16, SCALED>(a, s, coef, begin, end);                                                      \
        else                                                                                                             \
            chunk<0, SCALED>(a, s, coef, begin, end);                                                                    \
    }

__global__ __launch_bounds__(THREADS) void adamw_kernel(const Batch b) { CCR_ADAMW_CHUNKS(false, 1.0f) }

// ccr_adamw_step_scaled: the same pass under a control block.  skip is read by every workgroup before anything else; a skipped step
// stores nothing at all.
__global__ __launch_bounds__(THREADS) void adamw_scaled_kernel(const Batch b, const ccr_adamw_control *__restrict__ control) {
    if (control->skip != 0) return;
    const float coef = control->coef;
    CCR_ADAMW_CHUNKS(true, coef)
}
#undef CCR_ADAMW_CHUNKS

// ccr_grad_stats: the sum of squares of each chunk's gradients -> partials[chunk_base + c], in ONE order on both access paths (header):
// the element at offset j of its chunk is thread (j >> 2) & 255's, a thread adds its squares in increasing j.
__device__ __forceinline__ float add_square(const float acc, const float g) {
    const float sq = g * g;
    return acc + sq;
}

__global__ __launch_bounds__(THREADS) void grad_stats_kernel(const Batch b, float *__restrict__ partials, const int64_t chunk_base) {
    __shared__ float wave_sum[2][THREADS / 64];
    const uint32_t total = b.prefix[b.n_seg];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int parity = 0;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x, parity ^= 1) {
        const int si = find_segment(b.prefix, b.n_seg, c);      // block-uniform
        const SegArg &a = b.seg[si];
        const int64_t begin = (int64_t)(c - b.prefix[si]) * CHUNK;
        const int64_t end = begin + CHUNK < a.n ? begin + CHUNK : a.n;
        float acc = 0.0f;
        if (a.flags & SEG_VEC4) {
            const float4 *__restrict__ G = reinterpret_cast<const float4 *>(a.grad);
            const int64_t begin4 = begin >> 2, end4 = (begin + ((end - begin) & ~(int64_t)3)) >> 2;
            float4 g[CHUNK / 4 / THREADS];
#pragma unroll
            for (int k = 0; k < (int)(CHUNK / 4 / THREADS); ++k) {      // the loads first, the sums in order after them
                const int64_t i = begin4 + threadIdx.x + k * THREADS;
                g[k] = i < end4 ? G[i] : make_float4(0.f, 0.f, 0.f, 0.f);      // (+0 leaves a sum of squares as it is)
            }
#pragma unroll
            for (int k = 0; k < (int)(CHUNK / 4 / THREADS); ++k) {
                acc = add_square(acc, g[k].x);
                acc = add_square(acc, g[k].y);
                acc = add_square(acc, g[k].z);
                acc = add_square(acc, g[k].w);
            }
            // the last n % 4 elements: they follow every whole group of their thread, the one that would own the group
            if (end == a.n && ((end4 - begin4) & (THREADS - 1)) == (int64_t)threadIdx.x)
                for (int64_t i = end4 << 2; i < end; ++i) acc = add_square(acc, a.grad[i]);
        } else {
            for (int64_t i0 = begin + 4 * (int64_t)threadIdx.x; i0 < end; i0 += 4 * THREADS) {
                const int64_t i1 = i0 + 4 < end ? i0 + 4 : end;
                for (int64_t i = i0; i < i1; ++i) acc = add_square(acc, a.grad[i]);
            }
        }
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) acc = acc + __shfl_xor(acc, h, 64);      // lane i < h now holds x[i] + x[i + h]; lane 0 the wave's sum
        if (lane == 0) wave_sum[parity][wave] = acc;
        __syncthreads();      // (two buffers: the next chunk's writes cannot pass this chunk's read, one barrier per chunk)
        if (threadIdx.x == 0) {
            const float *w = wave_sum[parity];
            partials[chunk_base + c] = ((w[0] + w[1]) + w[2]) + w[3];
        }
    }
}

// ccr_adamw_control_update: one workgroup.  Thread t sums partials[t * slice, (t + 1) * slice) in index order in double, thread 0 the 256
// slice sums in slice order, and writes the block.
__global__ __launch_bounds__(CONTROL_THREADS) void control_update_kernel(ccr_adamw_control *__restrict__ control, const float *__restrict__ partials,
                                                                          const int64_t n_partials, const int64_t slice, const float max_norm,
                                                                          const int own_scale, const double growth, const double backoff,
                                                                          const int growth_interval, const float *__restrict__ ext_grad_scale,
                                                                          const float *__restrict__ ext_found_inf) {
    __shared__ double slice_sum[CONTROL_THREADS];
    const int64_t first = (int64_t)threadIdx.x * slice;
    const int64_t last = first + slice < n_partials ? first + slice : n_partials;
    double mine = 0.0;
    for (int64_t i = first; i < last; ++i) mine = mine + (double)partials[i];
    slice_sum[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int t = 0; t < CONTROL_THREADS; ++t) s = s + slice_sum[t];
    float scale = control->scale;
    int32_t tracker = control->growth_tracker, skipped = control->skipped_total;
    float inv = 1.0f;
    if (ext_grad_scale != nullptr)
        inv = (float)(1.0 / (double)*ext_grad_scale);
    else if (own_scale)
        inv = (float)(1.0 / (double)scale);
    const bool skip = !isfinite(s) || (ext_found_inf != nullptr && *ext_found_inf != 0.0f);
    const float norm = (float)sqrt(s) * inv;
    float clip = 1.0f;
    if (max_norm > 0.0f && !isinf(max_norm)) {
        const float denom = norm + 1e-6f;
        const float ratio = max_norm / denom;
        clip = ratio < 1.0f ? ratio : 1.0f;      // (a NaN ratio belongs to a skipped step)
    }
    if (skip) ++skipped;
    if (own_scale) {
        if (skip) {
            scale = (float)((double)scale * backoff);
            tracker = 0;
        } else if (++tracker == growth_interval) {
            const float grown = (float)((double)scale * growth);
            if (isfinite(grown)) scale = grown;
            tracker = 0;
        }
    }
    control->coef = inv * clip;
    control->skip = skip ? 1 : 0;
    control->norm = norm;
    control->scale = scale;
    control->growth_tracker = tracker;
    control->skipped_total = skipped;
}

}  // namespace optim
}  // namespace ccr

using namespace ccr;

// the list's checks, shared by the three entry points that take one: everything is checked before anything is launched, so a refused
// call changes nothing.  -> CCR_OK, or CCR_ERR_INVALID with the message set
static int check_segments(const char *who, const ccr_adamw_segment *segments, int n_segments) {
    CCR_REQUIRE(n_segments >= 0, "%s: n_segments=%d", who, n_segments);
    if (n_segments == 0) return CCR_OK;
    CCR_REQUIRE(segments != nullptr, "%s: segments is NULL (n_segments=%d)", who, n_segments);
    for (int i = 0; i < n_segments; ++i) {
        const char *why = optim::segment_error(segments[i]);
        CCR_REQUIRE(why == nullptr, "%s: segment %d (n=%lld): %s", who, i, (long long)segments[i].n, why);
    }
    return CCR_OK;
}

extern "C" int ccr_adamw_step(const ccr_adamw_segment *segments, int n_segments, float one_minus_beta1, float beta2, float one_minus_beta2,
                              float eps, void *stream) {
    if (const int rc = check_segments("ccr_adamw_step", segments, n_segments)) return rc;
    optim::Batch batch = {};
    batch.one_minus_beta1 = one_minus_beta1, batch.beta2 = beta2, batch.one_minus_beta2 = one_minus_beta2, batch.eps = eps;
    int cursor = 0;
    while (const uint32_t chunks = optim::next_batch(segments, n_segments, cursor, batch)) {
        hipLaunchKernelGGL(optim::adamw_kernel, dim3(optim::grid_for(chunks)), dim3(optim::THREADS), 0, (hipStream_t)stream, batch);
        CCR_LAUNCH_CHECK();
    }
    return CCR_OK;
}

extern "C" int ccr_adamw_step_scaled(const ccr_adamw_segment *segments, int n_segments, float one_minus_beta1, float beta2,
                                     float one_minus_beta2, float eps, const ccr_adamw_control *control, void *stream) {
    if (const int rc = check_segments("ccr_adamw_step_scaled", segments, n_segments)) return rc;
    CCR_REQUIRE(control != nullptr, "ccr_adamw_step_scaled: control is NULL");
    optim::Batch batch = {};
    batch.one_minus_beta1 = one_minus_beta1, batch.beta2 = beta2, batch.one_minus_beta2 = one_minus_beta2, batch.eps = eps;
    int cursor = 0;
    while (const uint32_t chunks = optim::next_batch(segments, n_segments, cursor, batch)) {
        hipLaunchKernelGGL(optim::adamw_scaled_kernel, dim3(optim::grid_for(chunks)), dim3(optim::THREADS), 0, (hipStream_t)stream, batch, control);
        CCR_LAUNCH_CHECK();
    }
    return CCR_OK;
}

extern "C" int64_t ccr_grad_stats_workspace_bytes(const ccr_adamw_segment *segments, int n_segments) {
    if (check_segments("ccr_grad_stats_workspace_bytes", segments, n_segments) != CCR_OK) return -1;
    return optim::stats_workspace_bytes(segments, n_segments);
}

extern "C" int ccr_grad_stats(const ccr_adamw_segment *segments, int n_segments, float *partials, void *stream) {
    if (const int rc = check_segments("ccr_grad_stats", segments, n_segments)) return rc;
    if (optim::list_chunks(segments, n_segments) == 0) return CCR_OK;
    CCR_REQUIRE(partials != nullptr, "ccr_grad_stats: partials is NULL (ccr_grad_stats_workspace_bytes)");
    optim::Batch batch = {};
    int cursor = 0;
    int64_t chunk_base = 0;      // the global index of the batch's first chunk
    while (const uint32_t chunks = optim::next_batch(segments, n_segments, cursor, batch)) {
        hipLaunchKernelGGL(optim::grad_stats_kernel, dim3(optim::grid_for(chunks)), dim3(optim::THREADS), 0, (hipStream_t)stream, batch, partials,
                           chunk_base);
        CCR_LAUNCH_CHECK();
        chunk_base += chunks;
    }
    return CCR_OK;
}

extern "C" int ccr_adamw_control_update(ccr_adamw_control *control, const float *partials, int64_t n_partials, float max_norm, int own_scale,
                                        double growth, double backoff, int growth_interval, const float *ext_grad_scale,
                                        const float *ext_found_inf, void *stream) {
    CCR_REQUIRE(control != nullptr, "ccr_adamw_control_update: control is NULL");
    CCR_REQUIRE(n_partials >= 0 && (n_partials == 0 || partials != nullptr), "ccr_adamw_control_update: n_partials=%lld, partials %s",
                (long long)n_partials, partials ? "given" : "NULL");
    CCR_REQUIRE(!(own_scale && ext_grad_scale != nullptr), "ccr_adamw_control_update: own_scale together with an external grad_scale");
    CCR_REQUIRE(!own_scale || growth_interval >= 1, "ccr_adamw_control_update: growth_interval=%d", growth_interval);
    hipLaunchKernelGGL(optim::control_update_kernel, dim3(1), dim3(optim::CONTROL_THREADS), 0, (hipStream_t)stream, control, partials, n_partials,
                       optim::control_slice(n_partials), max_norm, own_scale ? 1 : 0, growth, backoff, growth_interval, ext_grad_scale,
                       ext_found_inf);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}
