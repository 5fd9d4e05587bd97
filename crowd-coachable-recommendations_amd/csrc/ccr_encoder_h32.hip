// ccr_encoder_h32.hip -- the encoder layer kernels of the MiniLM-class models (hidden 384, 12 heads of width 32), inference only:
//
//   attention_h32_kernel        the algorithm of attention_kernel<DT, TR = true> (ccr_encoder.hip) for head width 32
//   add_layernorm128_kernel     add_layernorm_kernel / embed_layernorm_kernel without keep bits for rows of 128 P elements, P = 3, 5 .. 15
//   embed_layernorm128_kernel   (384, 640 .. 1920): widths the 256 C kernels cannot hold (a row of 128 stays refused, as it always was)
//
// A head-32 model could run on the 64-wide kernel with every head's Q / K / V weight rows zero-padded: twice the QKV GEMM, twice the
// attention MFMA work, twice the K of the output projection.  Attention's share of the forward grows as the hidden size shrinks (the
// GEMMs scale with hidden^2, attention with hidden x L), so the narrow head has a kernel of its own.  Nothing of ccr_encoder.hip's
// device code is touched: the 64-wide and the 256 C instantiations keep their code and their bits.
#include "ccr_common.h"
#include "ccr_encoder_common.h"
#include "ccr_index.h"

namespace ccr {

constexpr int A32_MAX_THREADS = 512;   // up to 8 waves per (sequence, head), wave w takes query blocks w, w + waves, ..
constexpr int A32_QW = 32;             // query rows per wave step (the N side of one 32x32 MFMA tile)
constexpr int A32_KB = 64;             // keys per loop step (two 32-key score tiles per online-softmax rescaling)
constexpr int A32_HEAD = 32;           // head width
// A key / value row is 64 bytes = FOUR 16-byte pieces (the 64-wide kernel: eight): a thread stages at most A32_KMAX key pieces and
// A32_VMAX value pieces, all in flight at once (8 x 4 VGPRs).  The launcher's wave count keeps lk_pad * 4 <= 4 * 64 * waves.
constexpr int A32_KMAX = 4, A32_VMAX = 4;
// Bytes per key row in LDS: 64 + 16.  The score MFMA's A operand is a ds_read_b128 of 16 bytes at the SAME column offset of 32
// consecutive rows per lane half; that instruction is served in 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of a half) on
// 64 banks, i.e. sixteen 16-byte slots of a 256-byte bank row.  Slot of row r = (80 r / 16) mod 16 = 5 r mod 16: both groups hold 16 rows
// that are distinct mod 16, and 5 is odd, so each group covers all sixteen slots once -- conflict-free.  (64-byte rows unpadded: 4 r mod 16,
// 4-way.  The 64-wide kernel's 144 = 9 x 16 is the same rule at its row length.)
constexpr int A32_KROW = 80;
// V stays row-major as it arrives, [lk_pad keys][64 B].  A 16-lane group of ds_read_b64_tr_b16 fetches 4 key rows x 16 head columns
// (32 bytes of each row); the two groups of a 32-lane half take columns 0-15 and 16-31 of the SAME four consecutive rows, so a half reads
// 4 x 64 = 256 contiguous bytes starting at a multiple of 256: all 64 banks once.  No half swap (the 64-wide kernel's 128-byte rows put two
// of a half's four rows on the same banks; these do not).
constexpr int A32_VROW = 64;

// LDS image: K [lk_pad][80 B] | V [lk_pad][64 B], lk_pad = the longest sequence rounded up to 64: 144 bytes per key, 73 728 at 512 keys.
__host__ __device__ inline size_t attention_h32_lds_bytes(int lk_pad) { return (size_t)lk_pad * (A32_KROW + A32_VROW); }

// S^T = K Q^T on v_mfma_f32_32x32x16: the contraction runs over 32 head columns = TWO MFMAs per 32-key tile (qf[2]); C layout: lane -> query
// (lane & 31), register e -> key (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  The probabilities, rounded to the 16-bit type, are the B operand of
// O^T = V^T P^T, ONE accumulator tile (32 head columns x 32 queries): register e -> head column (e & 3) + 8 (e >> 2) + 4 (lane >> 5).
template <int DT>
__global__ __launch_bounds__(A32_MAX_THREADS) void attention_h32_kernel(const uint16_t *__restrict__ qkv, const int32_t *__restrict__ seq_start,
                                                                      const int32_t *__restrict__ seq_len, uint16_t *__restrict__ out, int H,
                                                                      int pad_len, int max_len, int lk_pad, float scale_log2e) {
    typedef Half16<DT> HT;
    typedef typename HT::vec8 vec8;
    typedef typename HT::elem elem;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int nthreads = blockDim.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = nthreads >> 6;
    const int wq = (wv + blockIdx.x) % nwaves;   // the wave's first query block rotates with the head, as in the 64-wide kernel
    const int b = blockIdx.y, h = blockIdx.x;
    int len = seq_len[b];
    if (len > max_len) len = max_len;   // the LDS image holds max_len keys: a longer entry is cut
    if (len < 0) len = 0;
    const int rows = len > pad_len ? len : pad_len;   // rows the sequence occupies in the token arrays (padding rows get zeros)
    const int HD = H * A32_HEAD;
    const int64_t stride = 3 * (int64_t)HD;
    const int64_t row0 = seq_start[b];
    const uint16_t *Qg = qkv + row0 * stride + h * A32_HEAD;   // a head starts every 64 bytes: 16-byte accesses stay aligned
    const uint16_t *Kg = Qg + HD;
    const uint16_t *Vg = Qg + 2 * HD;
    uint16_t *Og = out + row0 * HD + h * A32_HEAD;
    const int ql = lane & 31, g = lane >> 5;
    if (len == 0) {   // an empty sequence (workgroup-uniform): its padding rows get zeros, nothing is read
        for (int q = tid; q < rows; q += nthreads) {
            uint4 *dst = reinterpret_cast<uint4 *>(Og + (int64_t)q * HD);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }

    char *Ks = smem;
    char *Vs = smem + (size_t)lk_pad * A32_KROW;
    const int nkb = (len + A32_KB - 1) / A32_KB;
    const int nk = nkb * A32_KB;   // <= lk_pad: rows len .. nk - 1 of both images are zeros

    // ---- stage K and V of this (sequence, head): every load (and the wave's first query fragment) is issued before the first LDS store
    uint4 kreg[A32_KMAX], vreg[A32_VMAX];
#pragma unroll
    for (int u = 0; u < A32_KMAX; ++u) {
        const int i = tid + u * nthreads;
        const int r = i >> 2, c = i & 3;
        kreg[u] = make_uint4(0u, 0u, 0u, 0u);
        if (r < len) kreg[u] = *reinterpret_cast<const uint4 *>(Kg + (int64_t)r * stride + c * 8);
    }
#pragma unroll
    for (int u = 0; u < A32_VMAX; ++u) {
        const int i = tid + u * nthreads;
        const int r = i >> 2, c = i & 3;
        vreg[u] = make_uint4(0u, 0u, 0u, 0u);
        if (r < len) vreg[u] = *reinterpret_cast<const uint4 *>(Vg + (int64_t)r * stride + c * 8);
    }
    vec8 qf[2];
    {
        const int q = wq * A32_QW + ql;
        const int qr = q < len ? q : len - 1;
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const vec8 *>(Qg + (int64_t)qr * stride + 16 * s + 8 * g);
    }
#pragma unroll
    for (int u = 0; u < A32_KMAX; ++u) {
        const int i = tid + u * nthreads;
        if (i < nk * 4) *reinterpret_cast<uint4 *>(Ks + (i >> 2) * A32_KROW + (i & 3) * 16) = kreg[u];
    }
#pragma unroll
    for (int u = 0; u < A32_VMAX; ++u) {
        const int i = tid + u * nthreads;
        if (i < nk * 4) *reinterpret_cast<uint4 *>(Vs + (size_t)i * 16) = vreg[u];   // row i >> 2, piece i & 3 of 64-byte rows: i * 16
    }
    __syncthreads();
    // This lane's part of every transposed read: lane 4 qq + pp of a 16-lane group supplies key row (base + qq), columns 4 pp .. 4 pp + 3 of
    // the group's 16 (8 bytes) and receives column (lane & 15) of keys base .. base + 3.  Groups 0 / 1 of a half take columns 0-15 / 16-31:
    // the lane's own head column d = lane & 31.  Key base = .. + 4 g: element j of half g <-> key 16 s + 4 g + (j & 3) + 8 (j >> 2), the
    // permutation the score tile's registers have.
    const int tr_qq = (lane & 15) >> 2, tr_pp = lane & 3;
    const int tr_off = (4 * g + tr_qq) * A32_VROW + 32 * ((lane >> 4) & 1) + 8 * tr_pp;

    for (int q0w = wq * A32_QW; q0w < rows; q0w += nwaves * A32_QW) {   // wave-uniform; no barrier below
        const int q = q0w + ql;
        if (q0w >= len) {   // a block of padding rows only: zeros
            if (q < rows) {
                uint2 *dst = reinterpret_cast<uint2 *>(Og + (int64_t)q * HD);
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[i * 2 + g] = make_uint2(0u, 0u);
            }
            continue;
        }
        if (q0w != wq * A32_QW) {   // the wave's next query block (sequences beyond 32 x waves tokens)
            const int qr = q < len ? q : len - 1;
#pragma unroll
            for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const vec8 *>(Qg + (int64_t)qr * stride + 16 * s + 8 * g);
        }

        ef32x16 o;
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = 0.f;
        float m = -INFINITY, lsum = 0.f;

        for (int kb = 0; kb < nkb; ++kb) {
            ef32x16 s0, s1;
#pragma unroll
            for (int e = 0; e < 16; ++e) s0[e] = s1[e] = 0.f;
            const char *kp = Ks + (kb * A32_KB + ql) * A32_KROW + g * 16;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const vec8 k0 = *reinterpret_cast<const vec8 *>(kp + 32 * s);
                const vec8 k1 = *reinterpret_cast<const vec8 *>(kp + 32 * A32_KROW + 32 * s);
                s0 = HT::mfma(k0, qf[s], s0);
                s1 = HT::mfma(k1, qf[s], s1);
            }
            float x[32];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                x[e] = s0[e];
                x[16 + e] = s1[e];
            }
            if (kb * A32_KB + A32_KB > len) {   // the last step: keys beyond the sequence
#pragma unroll
                for (int e = 0; e < 32; ++e) {
                    const int key = kb * A32_KB + (e >> 4) * 32 + (e & 3) + 8 * ((e & 15) >> 2) + 4 * g;
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
            for (int e = 0; e < 16; ++e) o[e] *= alpha;
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    vec8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (elem)x[hb * 16 + s2 * 8 + j];
                    // keys kbase .. + 3 and kbase + 8 .. + 11 (kbase = kb * 64 + hb * 32 + s2 * 16 + 4 g) of this lane's head column
                    typedef __attribute__((address_space(3))) es16x4 *lds_tr_ptr;
                    const char *vp = Vs + (size_t)(kb * A32_KB + hb * 32 + s2 * 16) * A32_VROW + tr_off;
                    union {
                        es16x4 h[2];
                        vec8 v;
                    } a;
                    a.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vp));
                    a.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(vp + 8 * A32_VROW));
                    o = HT::mfma(a.v, pf, o);
                }
            }
        }

        const float inv = 1.f / (lsum + __shfl_xor(lsum, 32));
        if (q < len) {
            // O^T tile: lane -> query, register e -> head column (e & 3) + 8 (e >> 2) + 4 g: four consecutive columns per 8-byte store
            uint16_t *dst = Og + (int64_t)q * HD + 4 * g;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4)
                *reinterpret_cast<uint2 *>(dst + 8 * c4) = round4<elem>(o[4 * c4] * inv, o[4 * c4 + 1] * inv, o[4 * c4 + 2] * inv, o[4 * c4 + 3] * inv);
        } else if (q < rows) {
            uint2 *dst = reinterpret_cast<uint2 *>(Og + (int64_t)q * HD);
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i * 2 + g] = make_uint2(0u, 0u);
        }
    }   // query blocks of this wave
}

template <int DT>
static int attention_h32_any(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq, int n_heads,
                             int max_len, int pad_len, float scale, hipStream_t stream) {
    const int lk_pad = (max_len + A32_KB - 1) / A32_KB * A32_KB;
    const size_t lds = attention_h32_lds_bytes(lk_pad);
    // the opt-in is cached per (kernel, device): ask for the kernel's maximum once (512 keys: 72 KB, above the 64 KB a launch gets unasked)
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&attention_h32_kernel<DT>), attention_h32_lds_bytes(512));
    if (rc != CCR_OK) return rc;
    // One wave per 32 query rows, at most 8.  Residency: the kernel takes 88 VGPRs (no AGPRs, no scratch), i.e. 5 waves per SIMD, 20 per
    // CU; the image is 144 bytes per key, so by LDS a CU holds 17 workgroups at 64 keys, 8 at 128, 4 at 256 and 2 at 512.  With this rule
    // those workgroups are 2, 4, 8 and 8 waves: the registers, not the LDS, set the residency up to 256 keys (10, 5 and 2 workgroups = 20,
    // 20 and 16 waves per CU), and at 512 keys both allow two workgroups = 16 waves.  Fewer waves per workgroup would not raise that and
    // would leave the staging of K and V, which runs once per (sequence, head), to fewer loads in flight; a second wave per query block
    // has nothing to do.  The staging bound below holds for every max_len: waves = min(8, ceil(max_len / 32)) >= lk_pad / 64.
    int waves = (max_len + A32_QW - 1) / A32_QW;
    if (waves > A32_MAX_THREADS / 64) waves = A32_MAX_THREADS / 64;
    CCR_REQUIRE(lk_pad * 4 <= A32_KMAX * 64 * waves && lk_pad * 4 <= A32_VMAX * 64 * waves, "ccr_attention_head_half: staging bound (internal)");
    hipLaunchKernelGGL((attention_h32_kernel<DT>), dim3(n_heads, n_seq), dim3(64 * waves), lds, stream, qkv, seq_start, seq_len, out, n_heads,
                       pad_len, max_len, lk_pad, scale * 1.4426950408889634f);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

// ---- LayerNorm rows of DIM = 128 P elements, P = 3, 5 .. 15.  One wave per row; a lane owns elements 2 (64 p + lane), + 1 of every 128-element
// slice: v[p][j].  4-byte loads of the 16-bit operand, 8-byte loads and stores of fp32 (a wave: 256 / 512 contiguous bytes per slice).
// The statistics are row_mean_rstd's definition (ccr_encoder_common.h) restated for this register layout -- butterfly sum, first mean
// sum / DIM, ONE correction step m0 + mean(v - m0), squared deviations by fma, rsqrtf -- so a row of equal elements normalises to exactly
// beta for every eps here too: v - m0 is a few ulps, exactly, its sum is exact, and m0 + sum / DIM rounds to v itself.  (1 / DIM is not a
// power of two at any of these widths; neither is it at 768: the product's rounding is 2^-24 of a few ulps.)
template <int P>
__device__ __forceinline__ void row_mean_rstd128(const float (&v)[P][2], float sum, float eps, float &mean, float &rstd) {
    constexpr int DIM = 128 * P;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float m0 = sum * (1.f / DIM);
    float sd = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) sd += (v[p][0] - m0) + (v[p][1] - m0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sd += __shfl_xor(sd, o);
    mean = m0 + sd * (1.f / DIM);
    float sq = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float d = v[p][j] - mean;
            sq = fmaf(d, d, sq);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    rstd = rsqrtf(sq * (1.f / DIM) + eps);
}

// slice p of y = xhat gamma + beta -> the fp32 row and / or its 16-bit copy (the rounded fp32 value)
template <int P, int DT>
__device__ __forceinline__ void layernorm128_store(const float (&v)[P][2], float mean, float rstd, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, float *__restrict__ out_f32,
                                                   uint16_t *__restrict__ out_half, int64_t row, int lane) {
    constexpr int DIM = 128 * P;
    typedef typename Half16<DT>::elem elem;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int col = 2 * (64 * p + lane);
        const float2 gm = *reinterpret_cast<const float2 *>(gamma + col);
        const float2 bt = *reinterpret_cast<const float2 *>(beta + col);
        float2 y;
        y.x = fmaf((v[p][0] - mean) * rstd, gm.x, bt.x);
        y.y = fmaf((v[p][1] - mean) * rstd, gm.y, bt.y);
        if (out_f32) *reinterpret_cast<float2 *>(out_f32 + row * DIM + col) = y;
        if (out_half) {
            union {
                elem h[2];
                uint32_t u;
            } w;
            w.h[0] = (elem)y.x;
            w.h[1] = (elem)y.y;
            *reinterpret_cast<uint32_t *>(out_half + row * DIM + col) = w.u;
        }
    }
}

template <int P, int DT>
__global__ __launch_bounds__(256) void add_layernorm128_kernel(const uint16_t *__restrict__ x, const float *__restrict__ res,
                                                              const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                              float *__restrict__ out_f32, uint16_t *__restrict__ out_half, int64_t rows) {
    constexpr int DIM = 128 * P;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[P][2];
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int col = 2 * (64 * p + lane);
        const uint32_t xb = *reinterpret_cast<const uint32_t *>(x + row * DIM + col);
        float2 r = make_float2(0.f, 0.f);
        if (res) r = *reinterpret_cast<const float2 *>(res + row * DIM + col);
        v[p][0] = Half16<DT>::lo(xb) + r.x;
        v[p][1] = Half16<DT>::hi(xb) + r.y;
        sum += v[p][0] + v[p][1];
    }
    float mean, rstd;
    row_mean_rstd128<P>(v, sum, eps, mean, rstd);
    layernorm128_store<P, DT>(v, mean, rstd, gamma, beta, out_f32, out_half, row, lane);
}

// (word[id] + type[t]) + position[p] in that order, fp32, then LayerNorm; ids outside a table are clamped (memory safety)
template <int P, int DT>
__global__ __launch_bounds__(256) void embed_layernorm128_kernel(const float *__restrict__ word, int64_t vocab, const float *__restrict__ pos_tab,
                                                                int64_t n_pos, const float *__restrict__ type_tab, int64_t n_types,
                                                                const int64_t *__restrict__ ids, const int64_t *__restrict__ pos,
                                                                const int64_t *__restrict__ types, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float eps, float *__restrict__ out_f32,
                                                                uint16_t *__restrict__ out_half, int64_t rows) {
    constexpr int DIM = 128 * P;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    auto clamp = [](int64_t v, int64_t n) { return v < 0 ? (int64_t)0 : (v >= n ? n - 1 : v); };
    const float *w = word + clamp(ids[row], vocab) * DIM;
    const float *q = pos_tab + clamp(pos[row], n_pos) * DIM;
    const float *t = type_tab + clamp(types ? types[row] : 0, n_types) * DIM;
    float v[P][2];
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int col = 2 * (64 * p + lane);
        const float2 a = *reinterpret_cast<const float2 *>(w + col);
        const float2 bq = *reinterpret_cast<const float2 *>(t + col);
        const float2 d = *reinterpret_cast<const float2 *>(q + col);
        v[p][0] = (a.x + bq.x) + d.x;
        v[p][1] = (a.y + bq.y) + d.y;
        sum += v[p][0] + v[p][1];
    }
    float mean, rstd;
    row_mean_rstd128<P>(v, sum, eps, mean, rstd);
    layernorm128_store<P, DT>(v, mean, rstd, gamma, beta, out_f32, out_half, row, lane);
}

// dim = 128 P, P = 3, 5 .. 15 (the caller has checked) -> a template argument
template <class F>
static inline int dispatch_width_odd128(int dim, F &&f) {
    switch (dim / 128) {
        case 3: return f(std::integral_constant<int, 3>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 9: return f(std::integral_constant<int, 9>{});
        case 11: return f(std::integral_constant<int, 11>{});
        case 13: return f(std::integral_constant<int, 13>{});
        default: return f(std::integral_constant<int, 15>{});
    }
}

int add_layernorm_odd128(const uint16_t *x, const float *res, const float *gamma, const float *beta, float eps, float *out_f32,
                         uint16_t *out_half, int64_t rows, int dim, int half_dtype, hipStream_t s) {
    CCR_REQUIRE(dim >= 384 && dim <= 1920 && dim % 256 == 128, "add_layernorm_odd128: dim=%d (internal)", dim);
    return dispatch_width_odd128(dim, [&](auto p) {
        return dispatch_half(half_dtype, [&](auto dt) {
            return launch_row_kernel(add_layernorm128_kernel<decltype(p)::value, decltype(dt)::value>, (rows + 3) / 4, s, x, res, gamma, beta, eps,
                                     out_f32, out_half, rows);
        });
    });
}

int embed_layernorm_odd128(const float *word_table, int64_t vocab, const float *position_table, int64_t n_positions, const float *type_table,
                           int64_t n_types, const int64_t *token_ids, const int64_t *positions, const int64_t *token_types,
                           const float *gamma, const float *beta, float eps, float *out_f32, uint16_t *out_half, int64_t rows, int dim,
                           int half_dtype, hipStream_t s) {
    CCR_REQUIRE(dim >= 384 && dim <= 1920 && dim % 256 == 128, "embed_layernorm_odd128: dim=%d (internal)", dim);
    return dispatch_width_odd128(dim, [&](auto p) {
        return dispatch_half(half_dtype, [&](auto dt) {
            return launch_row_kernel(embed_layernorm128_kernel<decltype(p)::value, decltype(dt)::value>, (rows + 3) / 4, s, word_table, vocab,
                                     position_table, n_positions, type_table, n_types, token_ids, positions, token_types, gamma, beta, eps,
                                     out_f32, out_half, rows);
        });
    });
}

}  // namespace ccr

using namespace ccr;

extern "C" int ccr_attention_head_half(const uint16_t *qkv, const int32_t *seq_start, const int32_t *seq_len, uint16_t *out, int n_seq,
                                       int n_heads, int head_width, int max_len, int pad_len, float scale, int half_dtype, void *stream) {
    CCR_REQUIRE(qkv && seq_start && seq_len && out, "ccr_attention_head_half: null pointer");
    CCR_REQUIRE(head_width == 32 || head_width == 64, "ccr_attention_head_half: head_width=%d (32 or 64)", head_width);
    if (const int rc = check_attention_shape("ccr_attention_head_half", half_dtype, n_seq, n_heads, max_len, pad_len, scale)) return rc;
    if (head_width == 64) return ccr_attention_half(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale, half_dtype, stream);
    if (n_seq == 0) return CCR_OK;
    return dispatch_half(half_dtype, [&](auto dt) {
        return attention_h32_any<decltype(dt)::value>(qkv, seq_start, seq_len, out, n_seq, n_heads, max_len, pad_len, scale, (hipStream_t)stream);
    });
}
