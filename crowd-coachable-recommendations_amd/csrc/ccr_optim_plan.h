// ccr_optim_plan.h -- host-only batching of ccr_adamw_step's segment list (no device header: tests/native/optim_plan_check.cpp
// compiles it with a plain C++ compiler).
//
// A segment (one parameter tensor) is cut into CHUNKs of 4096 elements; one workgroup of 256 threads updates one chunk at a time.  A launch
// carries up to BATCH_SEGMENTS segments BY VALUE in its kernel arguments together with the running prefix of their chunk counts, so the
// kernel finds (segment, offset) of chunk c with a short search over that prefix and no table ever lives in device memory.  Which segments
// share a launch depends on the list alone: the non-empty segments in order, BATCH_SEGMENTS at a time (a batch also closes before its
// chunk total would pass 2^31).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ccr_retrieval.h"

namespace ccr {
namespace optim {

constexpr int THREADS = 256;
constexpr int64_t CHUNK = 4096;          // elements per chunk: 256 threads x 4 iterations x one 16-byte access per stream
constexpr int BATCH_SEGMENTS = 48;       // segments per launch: 48 x 64 B + the prefix + the scalars = 3296 B of kernel arguments
constexpr int MAX_GRID = 2048;           // workgroups per launch; a workgroup strides over the chunks beyond
constexpr size_t MAX_ARG_BYTES = 4096;   // the kernel-argument segment the launches must stay under
constexpr uint32_t MAX_BATCH_CHUNKS = 1u << 31;

enum { SEG_VEC4 = 1, SEG_SHADOW_BF16 = 2, SEG_SHADOW_FP16 = 4 };

struct SegArg {      // 64 bytes
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    void *shadow;                 // NULL: none
    int64_t n;
    float decay, step_size, bc2_sqrt;
    uint32_t flags;               // SEG_VEC4: every pointer allows the 16-byte path; SEG_SHADOW_*: the shadow's type
};

struct Batch {       // one launch's kernel argument
    SegArg seg[BATCH_SEGMENTS];
    uint32_t prefix[BATCH_SEGMENTS + 1];   // prefix[i] = chunks of seg[0 .. i); prefix[n_seg] = the launch's chunk count
    int32_t n_seg;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
};
static_assert(sizeof(SegArg) == 64, "SegArg is laid out for 64 bytes");
static_assert(sizeof(Batch) <= MAX_ARG_BYTES, "a launch's arguments pass the kernel-argument limit");

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the 16-byte path: the four fp32 streams on 16-byte boundaries and the shadow (four 16-bit values per store) on an 8-byte one
inline bool segment_vec4(const ccr_adamw_segment &s) {
    const bool shadow = s.shadow != nullptr && s.shadow_dtype != 0;
    return aligned_to(s.param, 16) && aligned_to(s.grad, 16) && aligned_to(s.exp_avg, 16) && aligned_to(s.exp_avg_sq, 16) &&
           (!shadow || aligned_to(s.shadow, 8));
}

inline int64_t segment_chunks(int64_t n) { return (n + CHUNK - 1) / CHUNK; }

// NULL if the segment is well formed, else what is wrong with it (n == 0 asks for nothing and needs no pointers)
inline const char *segment_error(const ccr_adamw_segment &s) {
    if (s.n < 0) return "n < 0";
    if (s.shadow_dtype < 0 || s.shadow_dtype > 2) return "shadow_dtype is not 0 (none), 1 (bf16) or 2 (fp16)";
    if (s.n == 0) return nullptr;
    if (s.param == nullptr || s.grad == nullptr || s.exp_avg == nullptr || s.exp_avg_sq == nullptr)
        return "param, grad, exp_avg or exp_avg_sq is NULL";
    if (s.shadow_dtype != 0 && s.shadow == nullptr) return "shadow_dtype names a type and shadow is NULL";
    if (segment_chunks(s.n) >= (int64_t)MAX_BATCH_CHUNKS) return "n is beyond 2^43 elements";
    return nullptr;
}

// Fill `out` with the next batch of segments[cursor ...] (validated by segment_error) and move the cursor; -> the batch's chunk count, 0
// when the list is exhausted.  The scalars of `out` are the caller's to set.
inline uint32_t next_batch(const ccr_adamw_segment *segments, int n_segments, int &cursor, Batch &out) {
    out.n_seg = 0;
    out.prefix[0] = 0;
    uint32_t total = 0;
    while (cursor < n_segments && out.n_seg < BATCH_SEGMENTS) {
        const ccr_adamw_segment &s = segments[cursor];
        if (s.n == 0) {
            ++cursor;
            continue;
        }
        const uint64_t chunks = (uint64_t)segment_chunks(s.n);
        if (out.n_seg > 0 && (uint64_t)total + chunks > MAX_BATCH_CHUNKS) break;
        SegArg &a = out.seg[out.n_seg];
        a.param = s.param, a.grad = s.grad, a.exp_avg = s.exp_avg, a.exp_avg_sq = s.exp_avg_sq;
        const bool shadow = s.shadow != nullptr && s.shadow_dtype != 0;
        a.shadow = shadow ? s.shadow : nullptr;
        a.n = s.n;
        a.decay = s.decay, a.step_size = s.step_size, a.bc2_sqrt = s.bc2_sqrt;
        a.flags = (segment_vec4(s) ? SEG_VEC4 : 0) | (shadow ? (s.shadow_dtype == 1 ? SEG_SHADOW_BF16 : SEG_SHADOW_FP16) : 0);
        total += (uint32_t)chunks;
        out.prefix[++out.n_seg] = total;
        ++cursor;
    }
    for (int i = out.n_seg + 1; i <= BATCH_SEGMENTS; ++i) out.prefix[i] = total;   // (the search never reads past n_seg; no stale words travel)
    return total;
}

inline int grid_for(uint32_t chunks) { return (int)(chunks < (uint32_t)MAX_GRID ? chunks : (uint32_t)MAX_GRID); }

// ccr_grad_stats writes one fp32 partial per chunk at the chunk's GLOBAL index: the chunks of the list's non-empty segments counted in
// list order, whatever launch batch carries them.  A batch's first chunk sits at the chunk total of the batches before it, which the
// caller keeps while it walks the list:   base = 0;  while (chunks = next_batch(...)) { launch(batch, base);  base += chunks; }
// (the sum over the list of at most 2^31 segments of fewer than 2^31 chunks stays far inside int64)
inline int64_t list_chunks(const ccr_adamw_segment *segments, int n_segments) {
    int64_t total = 0;
    for (int i = 0; i < n_segments; ++i) total += segment_chunks(segments[i].n);
    return total;
}
inline int64_t stats_workspace_bytes(const ccr_adamw_segment *segments, int n_segments) {
    return list_chunks(segments, n_segments) * (int64_t)sizeof(float);
}

// ccr_adamw_control_update's slices: CONTROL_THREADS threads each sum ceil(n / CONTROL_THREADS) consecutive partials
constexpr int CONTROL_THREADS = 256;
inline int64_t control_slice(int64_t n_partials) { return (n_partials + CONTROL_THREADS - 1) / CONTROL_THREADS; }

// The segment of chunk c in a batch: the largest s with prefix[s] <= c (c < prefix[n_seg]).  Block-uniform in the kernel; the check program
// runs the same function.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int find_segment(const uint32_t *prefix, int n_seg, uint32_t c) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

}  // namespace optim
}  // namespace ccr
