// optim_amp_plan_check.cpp -- the host-side logic that ccr_grad_stats and ccr_adamw_control_update add to csrc/ccr_optim_plan.h, without a
// device: the GLOBAL chunk index of a partial across launch batches (base = the chunk total of the batches before; partial = base + c), the
// workspace size, and the control kernel's slices.  Walks lists the way ccr_grad_stats and grad_stats_kernel do and checks that chunk k of
// the list (the chunks of the non-empty segments counted in list order) is written exactly once, at index k, by the workgroup that holds
// that segment and offset; that the workspace is exactly 4 bytes per chunk; and that the 256 slices cover [0, n) once, in order.  Pointers
// are made-up addresses and never dereferenced.  Prints "<checks> checks, <violations> violations" last; exit status 1 on any violation.
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

static ccr_adamw_segment make_segment(int64_t n, int skew, uint64_t &next) {
    auto take = [&](int64_t bytes, int sk) {
        next = (next + 255) & ~(uint64_t)255;
        const uint64_t at = next + (uint64_t)sk * 4;
        next = at + (uint64_t)bytes;
        return at;
    };
    ccr_adamw_segment s;
    s.param = reinterpret_cast<float *>(take(n * 4, 0));
    s.grad = reinterpret_cast<const float *>(take(n * 4, skew));
    s.exp_avg = reinterpret_cast<float *>(take(n * 4, 0));
    s.exp_avg_sq = reinterpret_cast<float *>(take(n * 4, 0));
    s.shadow = nullptr;
    s.n = n;
    s.decay = 1.f, s.step_size = 0.f, s.bc2_sqrt = 1.f;
    s.shadow_dtype = 0;
    return s;
}

// Walk the list as ccr_grad_stats does; -> launches
static int walk(const char *label, const std::vector<ccr_adamw_segment> &list) {
    const int n_segments = (int)list.size();
    // what the list says: chunk k belongs to (segment, first element)
    std::vector<int> want_segment;
    std::vector<int64_t> want_begin;
    for (int i = 0; i < n_segments; ++i)
        for (int64_t c = 0; c < segment_chunks(list[i].n); ++c) want_segment.push_back(i), want_begin.push_back(c * CHUNK);
    const int64_t total = list_chunks(list.data(), n_segments);
    CHECK(total == (int64_t)want_segment.size(), "%s: list_chunks %lld, counted %zu", label, (long long)total, want_segment.size());
    CHECK(stats_workspace_bytes(list.data(), n_segments) == 4 * total, "%s: workspace %lld bytes for %lld chunks", label,
          (long long)stats_workspace_bytes(list.data(), n_segments), (long long)total);
    std::vector<uint8_t> written((size_t)total, 0);
    Batch b = {};
    int cursor = 0, launches = 0;
    int64_t base = 0;
    while (true) {
        const int first_of_batch = cursor;
        const uint32_t chunks = next_batch(list.data(), n_segments, cursor, b);
        if (chunks == 0) break;
        ++launches;
        std::vector<int> origin;
        for (int i = first_of_batch; i < cursor; ++i)
            if (list[i].n != 0) origin.push_back(i);
        CHECK((int)origin.size() == b.n_seg, "%s: launch %d has %d segments for %zu list entries", label, launches, b.n_seg, origin.size());
        if ((int)origin.size() != b.n_seg) return launches;
        const int grid = grid_for(chunks);
        for (int block = 0; block < grid; ++block)
            for (uint32_t c = (uint32_t)block; c < chunks; c += (uint32_t)grid) {
                const int si = find_segment(b.prefix, b.n_seg, c);
                const int64_t begin = (int64_t)(c - b.prefix[si]) * CHUNK;
                const int64_t k = base + c;      // the partial's index
                CHECK(k >= 0 && k < total, "%s: launch %d chunk %u writes partial %lld of %lld", label, launches, c, (long long)k, (long long)total);
                if (k < 0 || k >= total) continue;
                ++written[(size_t)k];
                CHECK(want_segment[(size_t)k] == origin[si] && want_begin[(size_t)k] == begin, "%s: partial %lld is segment %d at %lld, the list says segment %d at %lld",
                      label, (long long)k, origin[si], (long long)begin, want_segment[(size_t)k], (long long)want_begin[(size_t)k]);
            }
        base += chunks;
    }
    CHECK(base == total, "%s: the batches carry %lld chunks of %lld", label, (long long)base, (long long)total);
    size_t bad = 0;
    for (uint8_t w : written) bad += w != 1;
    CHECK(bad == 0, "%s: %zu partials not written exactly once", label, bad);
    return launches;
}

static void slices(int64_t n) {
    const int64_t per = control_slice(n);
    CHECK(per * CONTROL_THREADS >= n && (n == 0 ? per == 0 : (per - 1) * CONTROL_THREADS < n), "slices of n=%lld: %lld each", (long long)n, (long long)per);
    int64_t next = 0;      // the control kernel's ranges, thread by thread: contiguous, in order, ending at n
    for (int t = 0; t < CONTROL_THREADS; ++t) {
        const int64_t first = (int64_t)t * per, last = first + per < n ? first + per : n;
        if (first >= last) continue;
        CHECK(first == next, "slices of n=%lld: thread %d starts at %lld, not %lld", (long long)n, t, (long long)first, (long long)next);
        next = last;
    }
    CHECK(next == n, "slices of n=%lld end at %lld", (long long)n, (long long)next);
}

int main() {
    uint64_t next = 1u << 20;
    CHECK(walk("empty", {}) == 0, "the empty list launched something");
    CHECK(sizeof(Batch) + sizeof(float *) + sizeof(int64_t) <= MAX_ARG_BYTES, "the statistics kernel's arguments are %zu bytes", sizeof(Batch) + 16);

    // the GPU test's lists: the edge sizes in one list; 100 segments (three batches); one segment with more chunks than the capped grid
    {
        std::vector<ccr_adamw_segment> list;
        for (int64_t n : {1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193}) list.push_back(make_segment(n, 0, next));
        CHECK(walk("edges", list) == 1, "edges: launch count");
        CHECK(list_chunks(list.data(), (int)list.size()) == 9 + 2 + 3, "edges: %lld chunks", (long long)list_chunks(list.data(), (int)list.size()));
    }
    {
        std::vector<ccr_adamw_segment> list;
        for (int i = 0; i < 100; ++i) list.push_back(make_segment(1 + (int64_t)(i * 977) % 9000, i % 4, next));
        CHECK(walk("100 segments", list) == 3, "100 segments: launch count");
    }
    {
        std::vector<ccr_adamw_segment> list = {make_segment(2049 * CHUNK + 5, 0, next)};
        CHECK(list_chunks(list.data(), 1) == 2050 && list_chunks(list.data(), 1) > MAX_GRID, "one long segment: %lld chunks", (long long)list_chunks(list.data(), 1));
        CHECK(walk("one long segment", list) == 1, "one long segment: launch count");
    }
    // empty segments between and at the ends of batches take no index
    {
        std::vector<ccr_adamw_segment> list;
        for (int i = 0; i <= 200; ++i) list.push_back(make_segment(i % 7 == 0 ? 0 : 1 + (int64_t)i * 131, 0, next));
        walk("holes", list);
    }
    // BERT-base's 199 tensors: 26 823 partials
    {
        std::vector<int64_t> shape = {30522LL * 768, 512 * 768, 2 * 768, 768, 768};
        for (int l = 0; l < 12; ++l) {
            for (int j = 0; j < 4; ++j) shape.push_back(768 * 768), shape.push_back(768);
            shape.push_back(768), shape.push_back(768);
            shape.push_back(3072 * 768), shape.push_back(3072), shape.push_back(768 * 3072), shape.push_back(768);
            shape.push_back(768), shape.push_back(768);
        }
        shape.push_back(768 * 768), shape.push_back(768);
        std::vector<ccr_adamw_segment> list;
        for (int64_t n : shape) list.push_back(make_segment(n, 0, next));
        const int launches = walk("BERT-base", list);
        printf("BERT-base: %zu tensors, %lld partials, %lld workspace bytes, %d launches\n", list.size(), (long long)list_chunks(list.data(), (int)list.size()),
               (long long)stats_workspace_bytes(list.data(), (int)list.size()), launches);
    }
    for (int64_t n : {0, 1, 2, 255, 256, 257, 511, 512, 513, 2050, 26823, 1000003}) slices(n);

    printf("%lld checks, %lld violations\n", g_checks, g_violations);
    return g_violations ? 1 : 0;
}
