// optim_plan_check.cpp -- the host-side batching of ccr_adamw_step (csrc/ccr_optim_plan.h) without a device: walks segment lists the way
// the library and the kernel do (next_batch, the grid-stride loop over chunks, find_segment, the 16-byte / 4-byte split of a chunk) and
// checks that every element is covered exactly once, no chunk straddles a segment, the 16-byte path is taken only where every pointer
// allows it, the kernel arguments stay within 4096 bytes and BERT-base's 199 tensors need at most 16 launches.  Pointers are made-up
// addresses and never dereferenced.  Prints "<checks> checks, <violations> violations" last; exit status 1 on any violation.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "ccr_optim_plan.h"

using namespace ccr::optim;

static long long g_checks = 0, g_violations = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        ++g_checks;                       \
        if (!(cond)) {                    \
            ++g_violations;               \
            if (g_violations <= 20) {     \
                printf("VIOLATION: ");    \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}

// a segment of n elements whose arrays start `skew` floats past a 16-byte boundary (shadow: skew 16-bit values past an 8-byte one)
static ccr_adamw_segment make_segment(int64_t n, int skew_p, int skew_g, int skew_m, int skew_v, int shadow_dtype, int skew_s, uint64_t &next) {
    auto take = [&](int64_t bytes, int skew, int elem) {
        next = (next + 255) & ~(uint64_t)255;
        const uint64_t at = next + (uint64_t)skew * elem;
        next = at + (uint64_t)bytes;
        return at;
    };
    ccr_adamw_segment s;
    s.param = reinterpret_cast<float *>(take(n * 4, skew_p, 4));
    s.grad = reinterpret_cast<const float *>(take(n * 4, skew_g, 4));
    s.exp_avg = reinterpret_cast<float *>(take(n * 4, skew_m, 4));
    s.exp_avg_sq = reinterpret_cast<float *>(take(n * 4, skew_v, 4));
    s.shadow = shadow_dtype ? reinterpret_cast<void *>(take(n * 2, skew_s, 2)) : nullptr;
    s.n = n;
    s.decay = 1.f, s.step_size = 0.f, s.bc2_sqrt = 1.f;
    s.shadow_dtype = shadow_dtype;
    return s;
}

// Walk the list as ccr_adamw_step and adamw_kernel do; -> launches.  elementwise: mark every element (else: every chunk).
static int walk(const char *label, const std::vector<ccr_adamw_segment> &list, bool elementwise) {
    const int n_segments = (int)list.size();
    std::vector<std::vector<uint8_t>> seen(list.size());
    for (size_t i = 0; i < list.size(); ++i) {
        CHECK(segment_error(list[i]) == nullptr, "%s: segment %zu refused: %s", label, i, segment_error(list[i]));
        seen[i].assign((size_t)(elementwise ? list[i].n : segment_chunks(list[i].n)), 0);
    }
    Batch b = {};
    int cursor = 0, launches = 0, first_of_batch = 0;
    while (true) {
        first_of_batch = cursor;
        const uint32_t chunks = next_batch(list.data(), n_segments, cursor, b);
        if (chunks == 0) break;
        ++launches;
        CHECK(b.n_seg >= 1 && b.n_seg <= BATCH_SEGMENTS, "%s: launch %d carries %d segments", label, launches, b.n_seg);
        CHECK(b.prefix[0] == 0 && b.prefix[b.n_seg] == chunks, "%s: launch %d prefix ends %u / %u", label, launches, b.prefix[b.n_seg], chunks);
        // which list entries the batch's segments are (empty ones were skipped)
        std::vector<int> origin;
        for (int i = first_of_batch; i < cursor; ++i)
            if (list[i].n != 0) origin.push_back(i);
        CHECK((int)origin.size() == b.n_seg, "%s: launch %d has %d segments for %zu list entries", label, launches, b.n_seg, origin.size());
        if ((int)origin.size() != b.n_seg) return launches;
        for (int s = 0; s < b.n_seg; ++s) {
            const ccr_adamw_segment &src = list[origin[s]];
            const bool all_aligned = aligned_to(src.param, 16) && aligned_to(src.grad, 16) && aligned_to(src.exp_avg, 16) &&
                                     aligned_to(src.exp_avg_sq, 16) && (!(src.shadow && src.shadow_dtype) || aligned_to(src.shadow, 8));
            CHECK(((b.seg[s].flags & SEG_VEC4) != 0) == all_aligned, "%s: segment %d vec flag %u, aligned %d", label, origin[s], b.seg[s].flags, all_aligned);
            CHECK(b.seg[s].n == src.n && b.seg[s].param == src.param && b.seg[s].shadow == (src.shadow_dtype ? src.shadow : nullptr),
                  "%s: segment %d copied wrongly", label, origin[s]);
            CHECK(b.prefix[s + 1] - b.prefix[s] == (uint32_t)segment_chunks(src.n), "%s: segment %d has %u chunks for n=%lld", label, origin[s],
                  b.prefix[s + 1] - b.prefix[s], (long long)src.n);
        }
        const int grid = grid_for(chunks);
        CHECK(grid >= 1 && grid <= MAX_GRID, "%s: grid %d", label, grid);
        for (int block = 0; block < grid; ++block) {
            for (uint32_t c = (uint32_t)block; c < chunks; c += (uint32_t)grid) {
                const int si = find_segment(b.prefix, b.n_seg, c);
                CHECK(si >= 0 && si < b.n_seg && b.prefix[si] <= c && c < b.prefix[si + 1], "%s: chunk %u mapped to segment %d", label, c, si);
                const SegArg &a = b.seg[si];
                const int64_t begin = (int64_t)(c - b.prefix[si]) * CHUNK;
                const int64_t end = begin + CHUNK < a.n ? begin + CHUNK : a.n;
                CHECK(begin >= 0 && begin < end && end <= a.n, "%s: chunk %u covers [%lld, %lld) of n=%lld", label, c, (long long)begin, (long long)end,
                      (long long)a.n);      // no chunk straddles its segment
                std::vector<uint8_t> &mark = seen[origin[si]];
                if (!elementwise) {
                    ++mark[(size_t)(begin / CHUNK)];
                    continue;
                }
                int64_t end4 = begin;
                if (a.flags & SEG_VEC4) {      // the kernel's chunk(): groups of four on the 16-byte path, the rest one by one
                    end4 = begin + ((end - begin) & ~(int64_t)3);
                    CHECK((reinterpret_cast<uintptr_t>(a.param + begin) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.grad + begin) & 15) == 0 &&
                              (reinterpret_cast<uintptr_t>(a.exp_avg + begin) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.exp_avg_sq + begin) & 15) == 0,
                          "%s: 16-byte path on an odd address (chunk %u)", label, c);
                    CHECK(a.shadow == nullptr || ((reinterpret_cast<uintptr_t>(a.shadow) + 2 * (uintptr_t)begin) & 7) == 0,
                          "%s: 8-byte shadow store on an odd address (chunk %u)", label, c);
                    for (int64_t i4 = begin >> 2; i4 < (end4 >> 2); ++i4)
                        for (int j = 0; j < 4; ++j) ++mark[(size_t)(4 * i4 + j)];
                }
                for (int64_t i = end4; i < end; ++i) ++mark[(size_t)i];
            }
        }
    }
    for (size_t i = 0; i < list.size(); ++i) {
        size_t bad = 0;
        for (uint8_t m : seen[i]) bad += m != 1;
        CHECK(bad == 0, "%s: segment %zu (n=%lld): %zu %s not covered exactly once", label, i, (long long)list[i].n, bad, elementwise ? "elements" : "chunks");
    }
    return launches;
}

int main() {
    CHECK(sizeof(Batch) <= 4096 && sizeof(Batch) <= MAX_ARG_BYTES, "kernel arguments are %zu bytes", sizeof(Batch));
    CHECK(sizeof(SegArg) == 64, "SegArg is %zu bytes", sizeof(SegArg));
    uint64_t next = 1u << 20;

    // the empty list, and one segment of every size around the chunk and vector edges, on every alignment
    CHECK(walk("empty", {}, true) == 0, "the empty list launched something");
    const int64_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 1000003, 24000000};
    for (int64_t n : sizes)
        for (int skew = 0; skew < 4; ++skew)
            for (int which = 0; which < 6; ++which) {      // which array is off: none, p, g, m, v, the shadow
                if (skew == 0 && which > 0) continue;
                const int shadow = (int)(n % 3);
                std::vector<ccr_adamw_segment> one = {make_segment(n, which == 1 ? skew : 0, which == 2 ? skew : 0, which == 3 ? skew : 0,
                                                                   which == 4 ? skew : 0, shadow, which == 5 ? skew : 0, next)};
                char label[96];
                snprintf(label, sizeof label, "one n=%lld skew=%d which=%d", (long long)n, skew, which);
                const int launches = walk(label, one, n <= 1000003);
                CHECK(launches == 1, "%s: %d launches", label, launches);
                const bool expect_vec = which == 0 || skew == 0 || (which == 5 && shadow == 0);
                Batch b = {};
                int cursor = 0;
                next_batch(one.data(), 1, cursor, b);
                CHECK(((b.seg[0].flags & SEG_VEC4) != 0) == expect_vec, "%s: vec flag %u", label, b.seg[0].flags);
            }

    // 300 segments of n = 1 .. 300 (the GPU test's list) and with empty segments in between
    {
        std::vector<ccr_adamw_segment> list;
        for (int n = 1; n <= 300; ++n) list.push_back(make_segment(n, n % 4, 0, 0, 0, n % 3, 0, next));
        CHECK(walk("1..300", list, true) == (300 + BATCH_SEGMENTS - 1) / BATCH_SEGMENTS, "1..300: launch count");
        std::vector<ccr_adamw_segment> holes;
        for (int n = 0; n <= 100; ++n) holes.push_back(make_segment(n % 5 == 0 ? 0 : n, 0, 0, 0, 0, 0, 0, next));
        CHECK(walk("holes", holes, true) == 2, "holes: 80 non-empty segments are two launches");
    }

    // 1000 segments: mostly small, some of millions of elements, two of 24 M, every alignment
    {
        std::vector<ccr_adamw_segment> list;
        for (int i = 0; i < 1000; ++i) {
            int64_t n = 1 + (int64_t)(rnd() % 20000);
            if (i % 97 == 0) n = 1 + (int64_t)(rnd() % 3000000);
            if (i == 123 || i == 777) n = 24000000 - (i & 1);
            const uint64_t r = rnd();
            list.push_back(make_segment(n, (r & 8) ? (int)(r & 3) : 0, (r & 128) ? (int)((r >> 4) & 3) : 0, 0, (r >> 9) % 11 == 0 ? 1 : 0, (int)((r >> 16) % 3),
                                        (int)((r >> 20) & 3), next));
        }
        const int launches = walk("1000 segments", list, true);
        CHECK(launches == (1000 + BATCH_SEGMENTS - 1) / BATCH_SEGMENTS, "1000 segments: %d launches", launches);
    }

    // a list whose chunk count passes the capped grid (the stride loop), chunk level
    {
        std::vector<ccr_adamw_segment> list;
        for (int i = 0; i < 5; ++i) list.push_back(make_segment(2 * 1024 * 1024 + 17 * i, 0, 0, 0, 0, 1, 0, next));
        Batch b = {};
        int cursor = 0;
        const uint32_t chunks = next_batch(list.data(), 5, cursor, b);
        CHECK(chunks > (uint32_t)MAX_GRID && grid_for(chunks) == MAX_GRID, "stride list: %u chunks, grid %d", chunks, grid_for(chunks));
        CHECK(walk("stride", list, false) == 1, "stride list: launch count");
    }

    // BERT-base's parameter list: 5 embedding tensors, 12 x 16 layer tensors, the pooler's 2 = 199 tensors, 109.5 M elements
    {
        std::vector<int64_t> shape = {30522LL * 768, 512 * 768, 2 * 768, 768, 768};
        for (int l = 0; l < 12; ++l) {
            for (int j = 0; j < 4; ++j) shape.push_back(768 * 768), shape.push_back(768);      // q, k, v, attention output
            shape.push_back(768), shape.push_back(768);                                        // LayerNorm
            shape.push_back(3072 * 768), shape.push_back(3072), shape.push_back(768 * 3072), shape.push_back(768);
            shape.push_back(768), shape.push_back(768);
        }
        shape.push_back(768 * 768), shape.push_back(768);
        std::vector<ccr_adamw_segment> list;
        int64_t total = 0;
        for (int64_t n : shape) list.push_back(make_segment(n, 0, 0, 0, 0, n >= 768 * 768 && n < 30522LL * 768 ? 1 : 0, 0, next)), total += n;
        CHECK(list.size() == 199 && total == 109482240, "BERT-base list: %zu tensors, %lld elements", list.size(), (long long)total);
        const int launches = walk("BERT-base", list, false);
        CHECK(launches <= 16, "BERT-base needs %d launches", launches);
        printf("BERT-base: %zu tensors, %lld elements, %d launches, %zu argument bytes per launch\n", list.size(), (long long)total, launches, sizeof(Batch));
    }

    // what the entry point refuses
    {
        ccr_adamw_segment s = make_segment(10, 0, 0, 0, 0, 1, 0, next);
        ccr_adamw_segment bad = s;
        bad.n = -1;
        CHECK(segment_error(bad) != nullptr, "n < 0 accepted");
        bad = s, bad.grad = nullptr;
        CHECK(segment_error(bad) != nullptr, "NULL grad accepted");
        bad = s, bad.shadow = nullptr;
        CHECK(segment_error(bad) != nullptr, "NULL shadow with a type accepted");
        bad = s, bad.shadow_dtype = 3;
        CHECK(segment_error(bad) != nullptr, "shadow_dtype 3 accepted");
        bad = s, bad.n = 0, bad.param = nullptr;
        CHECK(segment_error(bad) == nullptr, "an empty segment needs no pointers");
    }

    printf("%lld checks, %lld violations\n", g_checks, g_violations);
    return g_violations ? 1 : 0;
}
