// ccr_gemm_common.h -- definitions shared by the GEMM + top-k kernels (ccr_main_pass.hip, experimental/gemm4w_proto.hip)
// and, for its wait macros, the threshold kernels (ccr_threshold.hip).
#pragma once
#include "ccr_common.h"

namespace ccr {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// The two MFMA shapes on either element type ET (CCR_DTYPE_BF16 / CCR_DTYPE_F16).  v_mfma_f32_*_f16 has the operand layout and the rate
// of the bf16 form, so operand fragments stay 16 opaque bytes (held as bf16x8 whatever they mean) all the way from LDS or HBM; the type
// is named HERE only, and the fp16 form reinterprets the same registers.  The ET = bf16 instantiation is the plain bf16 builtin.
template <int ET>
__device__ __forceinline__ f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (ET == CCR_DTYPE_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <int ET>
__device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (ET == CCR_DTYPE_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// LDS-DMA of 16 bytes per lane: the LDS destination is the wave-uniform base + lane * 16
__device__ __forceinline__ void glds16(const void *gsrc, char *lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// K is walked in 32-element sub-stages through a ring of four 32-KiB LDS buffers:
// [256 corpus rows x 64 B][256 query rows x 64 B] per sub-stage
constexpr int SUB_K = 32;
constexpr int SUB_BYTES = (TILE_DOCS + TILE_Q) * SUB_K * 2;  // 32768
constexpr int SUB_Q_REGION = TILE_DOCS * SUB_K * 2;           // 16384
constexpr int RING = 4;

// hipcc neither waits for LDS-DMA in __syncthreads() nor counts it for us: every wait is explicit
#define CCR_BARRIER() asm volatile("s_barrier" ::: "memory")
#define CCR_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define CCR_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

}  // namespace ccr
