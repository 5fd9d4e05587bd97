// ccr_loss_common.h -- what the three training losses (ccr_inbatch.hip, ccr_poolce.hip, ccr_bpr.hip) share, each defined once:
// the bf16 pieces both backward GEMMs rest on, the 64 x 64 tile transpose, the wave and workgroup reductions, and the host's
// workspace arithmetic.  Everything is inlined into its caller: a kernel's operation order is the order written here.
#pragma once
#include "ccr_gemm_common.h"   // bf16x8, f32x16

namespace ccr {

// g = hi + mid + lo exactly to 2^-24 relative: three bf16 parts, so that a product with a bf16 embedding runs on
// v_mfma_f32_32x32x16_bf16 at fp32-product accuracy.
__device__ __forceinline__ void split3(float g, uint16_t &hi, uint16_t &mid, uint16_t &lo) {
    const __bf16 a = (__bf16)g;
    const float r1 = g - (float)a;
    const __bf16 b = (__bf16)r1;
    const __bf16 c = (__bf16)(r1 - (float)b);
    hi = __builtin_bit_cast(uint16_t, a);
    mid = __builtin_bit_cast(uint16_t, b);
    lo = __builtin_bit_cast(uint16_t, c);
}

// 8 consecutive floats (32-byte aligned pairs of float4) -> 8 bf16, round to nearest even: torch's .to(bfloat16) bits
__device__ __forceinline__ uint4 pack8_bf16(const float *__restrict__ src) {
    const float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 4);
    const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        w[e] = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f[2 * e]) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f[2 * e + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// C layout of v_mfma_f32_32x32x16: column = lane & 31, register e of lane half h = lane >> 5 -> this row of a tile that starts at row0
__device__ __forceinline__ int mfma32_row(int row0, int e, int h) { return row0 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// Butterflies over the 64 lanes: every lane ends with the wave's sum / maximum (float or double).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off, 64);
        if constexpr (std::is_same_v<T, double>) v = fmax(v, o); else v = fmaxf(v, o);
    }
    return v;
}

// sum_i a[i] and sum_i b[i] (i < count) over a workgroup of 256 threads in fp64: thread t adds the elements t, t + 256, ... in turn,
// then one fixed tree.  Thread 0 hands the two totals to done(numerator, denominator).  4 KiB of LDS.
template <typename F>
__device__ __forceinline__ void block256_sum2(const float *__restrict__ a, const float *__restrict__ b, int count, F done) {
    __shared__ double s_n[256], s_d[256];
    const int tid = threadIdx.x;
    double n = 0.0, d = 0.0;
    for (int i = tid; i < count; i += 256) n += (double)a[i], d += (double)b[i];
    s_n[tid] = n, s_d[tid] = d;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) s_n[tid] += s_n[tid + s], s_d[tid] += s_d[tid + s];
        __syncthreads();
    }
    if (tid == 0) done(s_n[0], s_d[0]);
}

// ---- transpose of a 64 x 64 bf16 tile through LDS, 256 threads: thread tid takes row tid >> 2, columns (tid & 3) * 16 .. + 15 of the
// tile on the way in and the same position of the TRANSPOSED tile on the way out (two 16-byte LDS reads: each kernel writes them
// where its own layout wants them).
constexpr int TILE64 = 64;
constexpr int TILE64_PITCH = TILE64 + 8;   // LDS pitch 72 bf16 = 144 B: 16-byte aligned rows, rows 4 banks apart

// v = the 16 elements at columns c .. c + 15 of a row of a [rows][dim] bf16 matrix; zeros at columns >= dim (dim % 8 == 0, c % 8 == 0:
// whole 16-byte vectors) and, with inside = false, for a row beyond the matrix (`row` is then not read)
__device__ __forceinline__ void tile64_load16(const uint16_t *__restrict__ row, bool inside, int c, int dim, uint16_t (&v)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0;
    if (inside) {
#pragma unroll
        for (int h8 = 0; h8 < 2; ++h8) {
            const int dc = c + 8 * h8;
            if (dc < dim) {
                const uint4 q = *reinterpret_cast<const uint4 *>(row + dc);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[8 * h8 + 2 * e] = (uint16_t)(w[e] & 0xffffu), v[8 * h8 + 2 * e + 1] = (uint16_t)(w[e] >> 16);
            }
        }
    }
}
// the thread's 16 elements (tile row r, columns c0 .. c0 + 15) go to column r of the rows c0 .. c0 + 15 of the LDS tile
__device__ __forceinline__ void tile64_scatter16(uint16_t (*s_t)[TILE64_PITCH], int r, int c0, const uint16_t (&v)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) s_t[c0 + e][r] = v[e];
}

// ---- host: workspaces are carved in 256-byte steps from a 256-byte aligned base
inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }
inline char *align256(void *p) { return (char *)p + (256 - (uintptr_t)p % 256) % 256; }

// Bump carver: take<T>(bytes) is the next block, the one after it starts up256(bytes) further on.  A null base only counts.
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T>
    T *take(size_t bytes) {
        T *p = (T *)(base + off);
        off += up256(bytes);
        return p;
    }
};

// CCR_OK, or CCR_ERR_WORKSPACE with the error text set, for a workspace that is missing or shorter than `need`
inline int check_workspace(const char *who, const void *workspace, size_t need, size_t got) {
    if (workspace && got >= need) return CCR_OK;
    set_error("%s: workspace %zu bytes required, got %zu", who, need, got);
    return CCR_ERR_WORKSPACE;
}

}  // namespace ccr
