// ccr_select.hip -- the select stage of the search (stages: ccr_index.h):
//   select_rescore_kernel      per query radix-select the k-th largest MFMA score among the candidates, keep everything whose error
//                              interval reaches it, re-score those canonically (fp64 ordered) and sort by (score desc, id asc)
//   partition_flags / underfilled_to_retry / scatter_thresholds / gather_queries   the lists of the queries it flagged, for the retry
#include <algorithm>

#include "ccr_index.h"
#include "ccr_topk_device.h"

namespace ccr {

// Stage-2: per query, candidates -> exact canonical top-k.  grid = n_q, block = THREADS (256; 1024 for large k).
// dyn LDS: [dim bf16 query row][sub-list counts][sub-list offsets][rescore_cap u64 keys][compact x 8-byte candidates]
//
// JOIN of the sampled tiles (gmax != null: the main pass left out the tiles j * sample_stride, j < sample_tiles, and gmax[group][query],
// pitch gmax_pitch, still holds the sample pass's maximum MFMA score of each of their 16-row groups).  Why the result is unchanged:
//   * L, the k-th largest lower bound of the recorded candidates, is the k-th largest lower bound of a SUBSET of the rows, so it is
//     at most the k-th largest exact score -- and it is still taken from the recorded candidates alone;
//   * an unsampled row whose exact score reaches L >= tau was recorded by the filter (the argument without the join);
//   * a sampled row's exact score is at most its sample-pass MFMA score + c ||d||, at most gmax + c * tile_norm of its group: the
//     margin holds for any fp32 summation order, the sample pass's 32x32 shape included;
//   * so a group with gmax + c * tile_norm < L holds no result row, and a group at or above L is re-scored WHOLE (its 16 rows
//     join the collected rows through the same counter and capacity check; an overflow takes the dense path);
//   * ties are settled by the sort on (score, ~row) as before.
template <int ET, int THREADS>
__global__ __launch_bounds__(THREADS) void select_rescore_kernel(const uint2 *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                            int ranges, int sp, int nq_pad, const CandLayout lay, int k, int rescore_cap, int compact,
                                                            int64_t n_rows, float *__restrict__ thr, const float *__restrict__ cq,
                                                            const float *__restrict__ tile_norm, const float *__restrict__ row_norm,
                                                            const uint32_t *__restrict__ dmax_bits,
                                                            const uint16_t *__restrict__ Q, const uint16_t *__restrict__ D,
                                                            int dim, int64_t id_offset, float *__restrict__ out_scores,
                                                            int64_t *__restrict__ out_ids, uint32_t *__restrict__ flag_count,
                                                            uint32_t *__restrict__ flag_list,
                                                            unsigned long long *__restrict__ stat_cand,
                                                            const uint32_t *__restrict__ out_rows, const float *__restrict__ gmax,
                                                            int sample_tiles, int sample_stride, int gmax_pitch,
                                                            const uint32_t *__restrict__ glist, int list_cap, int regular_cap) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const size_t cnt_bytes = ((size_t)(ranges + 1) * 4 + 15) & ~(size_t)15;
    uint16_t *s_q = reinterpret_cast<uint16_t *>(sm);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(sm + (((size_t)dim * 2 + 15) & ~(size_t)15));
    uint32_t *s_off = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(s_cnt) + cnt_bytes);
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(s_off) + cnt_bytes);
    uint2 *s_comp = reinterpret_cast<uint2 *>(s_keys + rescore_cap);   // [compact] gathered candidates
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_ctl[4];
    __shared__ uint32_t s_wsum[THREADS / 64];
    __shared__ int s_flag;
    __shared__ uint32_t s_total, s_maxc, s_fill;
    __shared__ uint32_t s_ncoll;

    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    if (tid == 0) {
        s_flag = 0;
        s_total = 0;
        s_ncoll = 0;
        s_maxc = 0;
        s_fill = 0;
    }
    __syncthreads();
    // `ranges` counts SUB-LISTS here (sp per (range, query)); thread t owns the contiguous sub-lists [t*per, t*per+per)
    // so that the exclusive scan of the counts below is a plain block scan of per-thread sums
    const int per = (ranges + THREADS - 1) / THREADS;
    uint32_t my = 0, mymax = 0;
    for (int j = tid * per; j < min(ranges, tid * per + per); ++j) {
        uint32_t c = cnt[((int64_t)(j / sp) * nq_pad + q) * sp + (j % sp)];
        int cap;
        (void)cand_sublist(lay, j / sp, q, j % sp, nq_pad, sp, cap);
        if (c > (uint32_t)cap) {
            s_flag = 1;  // overflow: some survivors were dropped
            c = (uint32_t)cap;
        }
        s_cnt[j] = c;
        my += c;
        mymax = c > mymax ? c : mymax;
    }
    {   // block exclusive scan of `my` -> s_off[]
        const int lane = tid & 63, wid = tid >> 6;
        uint32_t incl = my;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_wsum[wid] = incl;
        if (my) atomicMax(&s_maxc, mymax);
        for (int c = tid; c < dim / 8; c += THREADS)
            reinterpret_cast<uint4 *>(s_q)[c] = reinterpret_cast<const uint4 *>(Q + (int64_t)q * dim)[c];
        __syncthreads();
        uint32_t base = incl - my;
        for (int w = 0; w < wid; ++w) base += s_wsum[w];
        for (int j = tid * per; j < min(ranges, tid * per + per); ++j) {
            s_off[j] = base;
            base += s_cnt[j];
        }
        if (tid == THREADS - 1) s_total = base;
        __syncthreads();
    }
    if (tid == 0 && stat_cand) atomicAdd(stat_cand, (unsigned long long)s_total);
    // A query the fused path cannot finish is flagged.  Two kinds: candidates were DROPPED (a sub-list overflowed, or fewer
    // than k rows passed) -- the caller retries the main pass for it under the re-tightened threshold its truncated lists
    // still give (FLAG_RETRY); or the selection itself cannot be done here (mass ties around the cut, k beyond the LDS
    // budget) -- only the exact dense path helps (FLAG_DENSE, the top bit of the list entry).
    bool bad = (s_flag != 0) || (s_total < (uint32_t)k);
    bool dense_only = (s_flag == 0) && bad;   // nothing was dropped and still fewer than k rows passed: a retry cannot find more
    // (fewer than k rows passed an ESTIMATED threshold: it was too high, and no list gives a bound -- the exact path, without a hint)
    if (dense_only && thr && tid == 0) thr[q] = -INFINITY;

    // sub-list j = (range j / sp, wave-row / lane part j % sp): cand_sublist() gives its first record and capacity
    auto sub_base = [&](int j) -> int64_t {
        int cap;
        return cand_sublist(lay, j / sp, q, j % sp, nq_pad, sp, cap);
    };
    auto at = [&](int j, int sl) -> uint2 { return cand[sub_base(j) + (int64_t)sl * sp]; };
    const int coll_cap = rescore_cap;
    uint32_t kth = 0;
    int need_eq = 0;
    int n_lds = 0;   // candidates resident in s_comp
    // Every candidate (mfma score m, row d of tile t) has its exact score inside [m - c ||d||, m + c ||d||] (c = gamma ||q||), and
    // ||d|| <= nt.  The LDS records carry the lower bound m - c nt; the k-th largest of them, L, is a lower bound of the k-th
    // largest exact score, and only candidates whose UPPER bound m + c ||d|| -- the ROW's own norm here, so one huge row widens
    // nobody else's interval -- reaches L can be in the result.
    const float c = cq[q];
    bool row_lb = false;   // the records' lower bounds use the row's own norm (the rare overflow sweep) instead of its tile's

    if (!bad && s_total <= (uint32_t)compact) {
        // The sub-lists are sparse: one sweep over (sub-list, slot < longest list) gathers them into LDS at their
        // scanned offsets (independent loads, no atomics); the select then never touches global memory.
        // (1) the first FIRST slots of every cell -- whole 16-byte pairs (slot, parts 2p and 2p + 1), contiguous and
        //     independent of the counts: a cell's slots 0..3 are its first one (sp = 4) or two (sp = 8) lines (issuing these
        //     loads at kernel start, ahead of the count scan, was measured: 398 -> 488 us, the 32 live registers cost more);
        // (2) only lists longer than that are swept: (sub-list, slot FIRST + s), s < W = pow2 >= longest - FIRST.
        // (large k -- the 1 024-thread form -- has lists of three to six records: eight unconditional slots there)
        constexpr int FIRST = THREADS >= 1024 ? 8 : 4, MAXL = 8;   // ranges * FIRST / 2 <= MAXL * THREADS (1 024 / 2 048 sub-lists)
        {
            const int per_cell = FIRST * sp / 2;               // 16-byte pairs per cell
            const int nload = (ranges / sp) * per_cell;
            uint4 v[MAXL];
#pragma unroll
            for (int t = 0; t < MAXL; ++t) {
                const int x = tid + t * THREADS;
                if (x < nload) {
                    const int cell = x / per_cell, w = x - cell * per_cell;
                    int cap;
                    v[t] = *reinterpret_cast<const uint4 *>(cand + cand_sublist(lay, cell, q, 0, nq_pad, sp, cap) + 2 * w);
                }
            }
#pragma unroll
            for (int t = 0; t < MAXL; ++t) {
                const int x = tid + t * THREADS;
                if (x < nload) {
                    const int cell = x / per_cell, w = x - cell * per_cell;
                    const int slot = (2 * w) / sp, part = (2 * w) % sp;
                    const int j = cell * sp + part;
                    if ((uint32_t)slot < s_cnt[j]) s_comp[s_off[j] + slot] = make_uint2(v[t].x, v[t].y);
                    if ((uint32_t)slot < s_cnt[j + 1]) s_comp[s_off[j + 1] + slot] = make_uint2(v[t].z, v[t].w);
                }
            }
        }
        sweep_sublists<THREADS, 8>(tid, ranges, FIRST, (int)s_maxc, s_cnt, at, [](int, int) { return true; },
                                   [&](int j, int sl, uint2 e) { s_comp[s_off[j] + sl] = e; });
        __syncthreads();
        n_lds = (int)s_total;
        for (int i0 = tid; i0 < n_lds; i0 += 4 * THREADS) {   // lower bounds with the TILE's norm (a 42-KB table: cache hits)
            uint2 e[4];
            float rn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * THREADS;
                e[u] = s_comp[i < n_lds ? i : i0];
                rn[u] = tile_norm[e[u].y / TILE_DOCS];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * THREADS;
                if (i < n_lds) s_comp[i] = make_uint2(__float_as_uint(fmaf(-c, rn[u], __uint_as_float(e[u].x))), e[u].y);
            }
        }
        __syncthreads();
    } else if (!bad && compact < k) {
        bad = dense_only = true;   // the LDS budget cannot even hold k records (huge dim * k): exact dense path
    } else if (!bad) {
        // More candidates than the LDS holds.  The k-th largest lower bound of ANY `compact` of them is a valid lower bound of
        // the query's k-th largest, so: keep the first `compact` records whose upper bound passes the current bound (none at
        // first), and while more than that passed, tighten the bound to the k-th largest lower bound of the kept ones and sweep again.
        // Every sweep at least halves what passes (the kept ones are a random part of what passed); 4 sweeps cover
        // 16 x the LDS capacity, beyond that the exact dense path takes the query.
        float keep = -INFINITY;
        bool fits = false;
        row_lb = true;
        for (int round = 0; round < 4 && !fits; ++round) {
            __syncthreads();   // everybody is done with s_comp / s_fill of the previous round
            if (tid == 0) s_fill = 0u;
            __syncthreads();
            sweep_sublists<THREADS, 8>(tid, ranges, 0, (int)s_maxc, s_cnt, at, [](int, int) { return true; },
                                       [&](int, int, uint2 e) {
                                           // (the ROW's own norm on both sides here: records of a tile that holds one huge row
                                           // would otherwise pass every sweep and contribute nothing to the bound)
                                           const float cn = c * row_norm[e.y];
                                           if (__uint_as_float(e.x) + cn >= keep) {
                                               const uint32_t p = atomicAdd(&s_fill, 1u);
                                               if (p < (uint32_t)compact) s_comp[p] = make_uint2(__float_as_uint(__uint_as_float(e.x) - cn), e.y);
                                           }
                                       });
            __syncthreads();
            if (s_fill <= (uint32_t)compact) {
                fits = true;
            } else {
                uint32_t kth0 = 0;
                int eq0 = 0;
                block_radix_select(
                    [&](int64_t i, bool &skip) -> uint32_t {
                        (void)skip;
                        return f32_orderable(__uint_as_float(s_comp[i].x));
                    },
                    compact, k, s_hist, s_ctl, kth0, eq0);
                keep = orderable_to_f32(kth0);
            }
        }
        if (fits)
            n_lds = (int)s_fill;
        else
            bad = dense_only = true;   // (near-)constant scores or k close to the LDS capacity: the exact dense path takes the query
    }
    if (!bad) {
        const int M = n_lds;
        block_radix_select(
            [&](int64_t i, bool &skip) -> uint32_t {
                (void)skip;
                return f32_orderable(__uint_as_float(s_comp[i].x));
            },
            M, k, s_hist, s_ctl, kth, need_eq);
        const float low = orderable_to_f32(kth);                                  // L: the k-th largest lower bound
        // Verification of the threshold the main pass filtered with.  Every row whose exact score reaches tau was recorded; if k
        // candidates have lower bounds >= tau (L >= tau), the k-th largest exact score is >= tau and nothing is missing.  A valid
        // lower bound (conservative thresholds, re-tightened ones) always passes; an ESTIMATED threshold that came out too high
        // fails: the query is retried under L, which is a valid bound.
        if (thr && low < thr[q]) {
            __syncthreads();
            if (tid == 0) {
                thr[q] = low;
                const uint32_t p = atomicAdd(flag_count, 1u);
                flag_list[p] = (out_rows ? out_rows[q] : (uint32_t)q);
            }
            return;
        }
        const float loose = fmaf(-2.f * c, __uint_as_float(*dmax_bits), low);    // no row's upper bound is further above its lower one
        for (int i = tid; i < M; i += THREADS) {
            const uint2 e = s_comp[i];
            const float lb = __uint_as_float(e.x);
            // (the row's own norm only here, for the few records near the cut: 4-byte reads scattered over an n_rows table --
            // taken for every record they cost the k = 1001 select +0.25 ms)
            if (lb >= loose && fmaf(c, row_norm[e.y], fmaf(c, row_lb ? row_norm[e.y] : tile_norm[e.y / TILE_DOCS], lb)) >= low) {
                const uint32_t p = atomicAdd(&s_ncoll, 1u);
                if (p < (uint32_t)coll_cap) s_keys[p] = (unsigned long long)e.y;  // local row for now
            }
        }
        // INVARIANT: `bad` and `dense_only` are workgroup-uniform -- every thread takes the same returns and the same barriers.  So the
        // counter is read where nobody can be adding to it: behind the barrier that ends the collection, and (join) in front of the
        // barrier that starts the joiners.
        // The recorded candidates keep their own limit (regular_cap: what rescore_cap is without the join -- mass ties around the cut
        // take the dense path exactly as they do when every tile is scored, in the retry pass too); joined rows may fill the rest.
        __syncthreads();
        const uint32_t n_recorded = s_ncoll;
        if (n_recorded > (uint32_t)regular_cap) bad = dense_only = true;  // mass ties around the cut
        if (gmax && !bad) {
            __syncthreads();   // every thread has read n_recorded: the joiners may add
            // The groups to test: the threshold kernel's short list of this query (the groups whose upper bound reaches tau <= L: a
            // few dozen 4-byte reads) -- or, without a list or when it overflowed, the query's whole column of the group maxima
            // (one value per 128-byte line: 2.3 GB of line traffic at NQ, measured +0.12 ms of select and a slower pack beside it).
            // Group gi of a sampled tile (Mfma32::gmax): wave row gi >> 3, MFMA tile (gi >> 1) & 3, lane half gi & 1; register e of its
            // 16 holds row (e & 3) + 8 * (e >> 2) of the lane half's rows.
            const int ngroups = sample_tiles * GROUPS_PER_TILE;
            const uint32_t *const my_list = glist ? glist + (int64_t)q * (list_cap + 1) : nullptr;
            const int nlist = my_list ? (int)min(my_list[0], (uint32_t)list_cap + 1u) : list_cap + 1;
            const bool listed = nlist <= list_cap;
            for (int x = tid; x < (listed ? nlist : ngroups); x += THREADS) {
                const int g = listed ? (int)my_list[1 + x] : x;
                const int64_t tile = (int64_t)(g / GROUPS_PER_TILE) * sample_stride;
                if (fmaf(c, tile_norm[tile], gmax[(int64_t)g * gmax_pitch + q]) >= low) {
                    const int gi = g % GROUPS_PER_TILE;
                    const uint32_t row0 = (uint32_t)(tile * TILE_DOCS) + (uint32_t)((gi >> 3) * 128 + ((gi >> 1) & 3) * 32 + (gi & 1) * 4);
                    for (int e = 0; e < 16; ++e) {   // (one slot at a time, exactly as the recorded candidates above)
                        const uint32_t p = atomicAdd(&s_ncoll, 1u);
                        if (p < (uint32_t)coll_cap) s_keys[p] = (unsigned long long)(row0 + (uint32_t)((e & 3) + 8 * (e >> 2)));
                    }
                }
            }
            __syncthreads();   // (no thread adds behind this barrier: the read below is uniform)
            if (s_ncoll > (uint32_t)coll_cap) bad = dense_only = true;  // the joined rows do not fit beside the recorded ones
        }
    }
    if (bad) {
        if (tid == 0) {
            const uint32_t p = atomicAdd(flag_count, 1u);
            flag_list[p] = (out_rows ? out_rows[q] : (uint32_t)q) | (dense_only ? FLAG_DENSE : 0u);
        }
        return;
    }
    const int ncoll = (int)s_ncoll;
    const int np2 = pow2_ceil(ncoll);
    // Canonical re-score.  The candidate rows are scattered over the shard; a thread walking "its" row 16 bytes at a
    // time makes every wave-load touch 64 different cache lines (measured 1.5 TB/s at k = 1000).  Instead the rows are
    // staged through the (now free) candidate area of the LDS in K slices of SB bytes per row: lanes_per_row adjacent
    // lanes fetch one row's slice (whole 64/128-byte segments, all loads of a slice in flight), then every thread runs
    // the fp64 chain of its own row(s) over the slice from LDS.  Element order inside a row is unchanged.
    const size_t stage_bytes = (size_t)compact * 8;
    // (both variants: before the slices were software-pipelined the barriers cost the 256-thread form more than they saved;
    // with the pipeline the NQ select goes 405 -> 308 us -- its re-score 228 -> 130 us -- and a 1/8 shard, whose rows sit in the
    // Infinity Cache, is unchanged)
    int SB = (size_t)ncoll * 144 <= stage_bytes ? 128 : ((size_t)ncoll * 80 <= stage_bytes ? 64 : 0);
    constexpr int PRE = 8;                                               // 16-byte pieces a thread keeps in flight for the next slice
    if (SB == 128 && ncoll * 8 > PRE * THREADS) SB = 64;
    if (SB != 0 && ncoll <= 2 * THREADS && ncoll * (SB / 16) <= PRE * THREADS) {
        char *stage = reinterpret_cast<char *>(s_comp);
        const int stride = SB + 16;                 // +16: consecutive rows start 4 banks apart (conflict-free b128 reads)
        const int lpr = SB / 16;                    // lanes per row and slice (THREADS % lpr == 0: a thread's pieces share one column)
        const int row_bytes = dim * 2;
        const char *Dbytes = reinterpret_cast<const char *>(D);
        const int col = (tid % lpr) * 16;           // byte column of this thread's pieces inside a slice
        // Software pipeline: the pieces of slice s + 1 are loaded into registers while slice s is consumed from the LDS, so the
        // scattered row reads (the bulk of this stage: ~1.5 KB per re-scored row) overlap the fp64 chains instead of sitting
        // between two barriers 24 times per query.
        // (every piece is loaded unconditionally -- an unused slot reads row 0, a column past the row end re-reads column 0 --
        // so that the prefetched values stay in registers; only the store into the LDS is conditional)
        // piece j of this thread belongs to candidate (tid + j * THREADS) / lpr; only its row pointer is kept.  Eight named
        // values, not an array: hipcc leaves a uint4[8] in scratch memory under the 128-register budget of 1 024 threads.
#define CCR_PIECES(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
        // address column: a column past the row end (dim = 32 under a 128-byte slice) reads column 0 -- the FIRST load too, not only
        // the refills below: the last corpus row may end exactly at the end of the caller's allocation
        const int acol = col < row_bytes ? col : 0;
        const char *Dcol = Dbytes + acol;
        const int npiece = ncoll * lpr;
#define CCR_DECL(j)                                                                                              \
    const int idx##j = tid + j * THREADS;                                                                        \
    const char *src##j = Dcol + (int64_t)(uint32_t)s_keys[idx##j < npiece ? idx##j / lpr : 0] * row_bytes;      \
    uint4 pre##j = *reinterpret_cast<const uint4 *>(src##j);
        CCR_PIECES(CCR_DECL)
#undef CCR_DECL
        double acc[2] = {0.0, 0.0};
        for (int k0 = 0; k0 < row_bytes; k0 += SB) {
            __syncthreads();                        // the previous slice has been consumed (first pass: s_comp is free)
            const bool col_in = k0 + col < row_bytes;
#define CCR_PUT(j) \
    if (col_in && idx##j < npiece) *reinterpret_cast<uint4 *>(stage + (idx##j / lpr) * stride + col) = pre##j;
            CCR_PIECES(CCR_PUT)
#undef CCR_PUT
            __syncthreads();
            {   // next slice: in flight during the fp64 chains below
                const int kn = (k0 + SB + col < row_bytes) ? k0 + SB : -acol;
#define CCR_GET(j) pre##j = *reinterpret_cast<const uint4 *>(src##j + kn);
                CCR_PIECES(CCR_GET)
#undef CCR_GET
            }
#undef CCR_PIECES
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * THREADS;
                if (i < ncoll) {
                    double a = acc[j];
                    for (int c = 0; c < lpr && k0 + c * 16 < row_bytes; ++c) {
                        const uint4 dv = *reinterpret_cast<const uint4 *>(stage + (size_t)i * stride + c * 16);
                        const uint4 qv = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(s_q) + k0 + c * 16);
                        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w};
                        const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            a = fma((double)elem_lo<ET>(qw[e]), (double)elem_lo<ET>(dw[e]), a);
                            a = fma((double)elem_hi<ET>(qw[e]), (double)elem_hi<ET>(dw[e]), a);
                        }
                    }
                    acc[j] = a;
                }
            }
        }
        __syncthreads();                            // every loader is done reading the row ids in s_keys
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + j * THREADS;
            if (i < np2) s_keys[i] = i < ncoll ? make_key((float)acc[j], (uint32_t)s_keys[i]) : 0ull;
        }
    } else {
        // each thread reads and rewrites only its own key slots
        for (int i = tid; i < np2; i += blockDim.x) {
            unsigned long long key = 0ull;
            if (i < ncoll) {
                const uint32_t row = (uint32_t)s_keys[i];
                key = make_key(canonical_dot<ET>(s_q, D + (int64_t)row * dim, dim), row);
            }
            s_keys[i] = key;
        }
    }
    block_bitonic_sort_desc(s_keys, np2);
    const int64_t orow = out_rows ? (int64_t)out_rows[q] : (int64_t)q;   // retry pass: compacted query i -> original row
    for (int i = tid; i < k; i += blockDim.x) {
        const unsigned long long key = s_keys[i];
        out_scores[orow * k + i] = key_score(key);
        store_id(out_ids, orow * k + i, id_offset, key_idx(key));
    }
}

constexpr size_t SELECT_LDS_BUDGET = 150 * 1024;   // dynamic LDS the select kernel may ask for (160 KiB per CU)

static size_t select_fixed_lds(int dim, int ranges, int rescore_cap) {
    const size_t cnt_bytes = ((size_t)(ranges + 1) * 4 + 15) & ~(size_t)15;
    return (((size_t)dim * 2 + 15) & ~(size_t)15) + 2 * cnt_bytes + (size_t)rescore_cap * 8;
}

// Candidates per query the select kernel can gather into LDS: `want` (the planner's expectation with head room),
// at least 2048 (a smaller area lets more queries share a CU: the re-score is latency-bound, 0.39 -> 0.37 ms at NQ and
// 0.25 -> 0.21 ms on a 1/8 shard against a 4096 floor), never more than the LDS budget allows.
int select_compact_entries(int dim, int ranges, int rescore_cap, int64_t want) {
    const size_t fixed = select_fixed_lds(dim, ranges, rescore_cap);
    const int64_t fit = fixed + 2048 < SELECT_LDS_BUDGET ? (int64_t)((SELECT_LDS_BUDGET - fixed) / 8) : 256;
    return (int)std::min<int64_t>(std::max<int64_t>(want, 2048), fit) / 256 * 256;
}

int launch_select_rescore(const SelectArgs &a, hipStream_t s) {
    const int regular_cap = a.regular_cap <= 0 || a.regular_cap > a.rescore_cap ? a.rescore_cap : a.regular_cap;
    const size_t lds = select_fixed_lds(a.dim, a.ranges, a.rescore_cap) + (size_t)a.compact * 8;
    const bool wide = a.rescore_cap > 512 || a.compact > 8192 || a.ranges > 1024;   // 1024 threads: one re-scored row per thread at large k
    auto go = [&](auto kernel, int threads) -> int {
        if (lds > 48 * 1024) {
            const int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), SELECT_LDS_BUDGET + 8192);
            if (rc != CCR_OK) return rc;
        }
        hipLaunchKernelGGL(kernel, dim3(a.n_q), dim3(threads), lds, s, a.cand, a.cnt, a.ranges, a.sp, a.nq_pad, a.lay, a.k, a.rescore_cap, a.compact,
                           a.n_rows, a.thr, a.cq, a.tile_norm, a.row_norm, a.dmax_bits, a.Q, a.D, a.dim, a.id_offset, a.out_scores, a.out_ids,
                           a.flag_count, a.flag_list, a.stat_cand, a.out_rows, a.gmax, a.sample_tiles, a.sample_stride, a.gmax_pitch, a.glist,
                           a.list_cap, regular_cap);
        CCR_LAUNCH_CHECK();
        return CCR_OK;
    };
    return dispatch_half(a.dt, [&](auto et) {
        constexpr int ET = decltype(et)::value;
        if (wide) return go(&select_rescore_kernel<ET, 1024>, 1024);
        return go(&select_rescore_kernel<ET, 256>, 256);
    });
}

// Retry pass set-up: split the flagged list into the queries to retry and the ones that need the dense path, and gather
// the retried queries' rows, thresholds and margins into compact arrays.  One workgroup; counts[0] = retried, counts[1] = dense.
__global__ __launch_bounds__(256) void partition_flags_kernel(const uint32_t *__restrict__ flags, int begin, int n,
                                                             uint32_t *__restrict__ retry_list, uint32_t *__restrict__ dense_list,
                                                             uint32_t *__restrict__ counts) {   // dense_list: the caller's append position
    __shared__ uint32_t s_n[2];
    if (threadIdx.x == 0) s_n[0] = s_n[1] = 0;
    __syncthreads();
    // order inside the two lists does not matter (each entry is a whole query)
    for (int i = begin + threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t f = flags[i];
        if (f & FLAG_DENSE)
            dense_list[atomicAdd(&s_n[1], 1u)] = f & ~FLAG_DENSE;
        else
            retry_list[atomicAdd(&s_n[0], 1u)] = f;
    }
    __syncthreads();
    if (threadIdx.x < 2) counts[threadIdx.x] = s_n[threadIdx.x];
}

// Estimated thresholds: a query for which FEWER than k rows passed (the select left thr[q] = -inf and FLAG_DENSE) gets the conservative
// bound of the sample instead -- a valid lower bound of its k-th largest score -- and becomes an ordinary retry.
__global__ __launch_bounds__(256) void underfilled_to_retry_kernel(uint32_t *__restrict__ flags, int begin, int n,
                                                                  const float *__restrict__ thr_safe, float *__restrict__ thr) {
    const int i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    const uint32_t q = f & ~FLAG_DENSE;
    if ((f & FLAG_DENSE) && thr[q] == -INFINITY && thr_safe[q] > -INFINITY) {   // (a NaN bound -- non-finite embeddings -- stays on the exact path)
        thr[q] = thr_safe[q];
        flags[i] = q;
    }
}

// thr[list[i]] = thr2[i]: the re-tightened thresholds of a retry round go back to the original query order
__global__ __launch_bounds__(256) void scatter_thresholds_kernel(const uint32_t *__restrict__ list, int n, const float *__restrict__ thr2,
                                                                float *__restrict__ thr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) thr[list[i]] = thr2[i];
}

__global__ __launch_bounds__(256) void gather_queries_kernel(const uint16_t *__restrict__ Q, int dim, const uint32_t *__restrict__ list,
                                                            int n, const float *__restrict__ thr, const float *__restrict__ delta,
                                                            uint16_t *__restrict__ Q2, float *__restrict__ thr2,
                                                            float *__restrict__ delta2) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const uint32_t q = list[i];
    for (int c = threadIdx.x; c < dim / 8; c += blockDim.x)
        reinterpret_cast<uint4 *>(Q2 + (int64_t)i * dim)[c] = reinterpret_cast<const uint4 *>(Q + (int64_t)q * dim)[c];
    if (threadIdx.x == 0) {
        thr2[i] = thr[q];
        delta2[i] = delta[q];
    }
}

int launch_partition_flags(const uint32_t *flags, int begin, int n, uint32_t *retry_list, uint32_t *dense_list, uint32_t *counts,
                           hipStream_t s) {
    hipLaunchKernelGGL(partition_flags_kernel, dim3(1), dim3(256), 0, s, flags, begin, n, retry_list, dense_list, counts);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_underfilled_to_retry(uint32_t *flags, int begin, int n, const float *thr_safe, float *thr, hipStream_t s) {
    if (n <= begin) return CCR_OK;
    hipLaunchKernelGGL(underfilled_to_retry_kernel, dim3((n - begin + 255) / 256), dim3(256), 0, s, flags, begin, n, thr_safe, thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_scatter_thresholds(const uint32_t *list, int n, const float *thr2, float *thr, hipStream_t s) {
    if (n <= 0) return CCR_OK;
    hipLaunchKernelGGL(scatter_thresholds_kernel, dim3((n + 255) / 256), dim3(256), 0, s, list, n, thr2, thr);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

int launch_gather_queries(const uint16_t *Q, int dim, const uint32_t *list, int n, const float *thr, const float *delta, uint16_t *Q2,
                          float *thr2, float *delta2, hipStream_t s) {
    if (n <= 0) return CCR_OK;
    hipLaunchKernelGGL(gather_queries_kernel, dim3(n), dim3(256), 0, s, Q, dim, list, n, thr, delta, Q2, thr2, delta2);
    CCR_LAUNCH_CHECK();
    return CCR_OK;
}

}  // namespace ccr
