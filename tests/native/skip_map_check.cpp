// Host-only check of the main pass's tile map (ccr::unsampled_tile in ccr_common.h) and of the plans that use it (ccr::make_plan
// in libccr_hip.so): no GPU call.  Built and run by tests/test_cpu_skip_map.py.  Exits non-zero on a violated property.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ccr_plan.h"

using namespace ccr;

// t(v), v in [0, tiles - n): strictly ascending, never a sampled tile j * s (j < n), every other tile below `tiles` exactly once
static int check_map(long long tiles, int s, int n) {
    std::vector<char> seen((size_t)tiles, 0);
    long long prev = -1;
    int bad = 0;
    for (long long v = 0; v < tiles - n; ++v) {
        const long long t = unsampled_tile(v, s, n);
        if (t <= prev) bad |= 1;
        if (t < 0 || t >= tiles) {
            bad |= 2;
            continue;
        }
        if (t % s == 0 && t / s < n) bad |= 4;
        if (seen[(size_t)t]) bad |= 8;
        seen[(size_t)t] = 1;
        prev = t;
    }
    for (long long t = 0; t < tiles; ++t) {
        const bool sampled = t % s == 0 && t / s < n;
        if (!sampled && !seen[(size_t)t]) bad |= 16;
    }
    if (bad) printf("FAIL map tiles=%lld s=%d n=%d: %s%s%s%s%s\n", tiles, s, n, bad & 1 ? "not ascending; " : "", bad & 2 ? "out of range; " : "",
                    bad & 4 ? "hits a sampled tile; " : "", bad & 8 ? "a tile twice; " : "", bad & 16 ? "an unsampled tile missed; " : "");
    return bad ? 1 : 0;
}

static int expect_skip(const char *what, const Plan &p, int want) {
    printf("%s: fused %d opt_rank %d phases %d/%d narrow %d sample %d x stride %lld of %lld tiles, rescore_cap %d, skip_sampled %d\n", what, p.fused,
           p.opt_rank, p.item_a, p.item_b, p.narrow, p.sample_tiles, (long long)p.sample_stride, (long long)p.tiles, p.rescore_cap, p.skip_sampled);
    int bad = 0;
    if (p.skip_sampled != want) bad = 1;
    if (p.skip_sampled) {
        // the conditions of the skip: one launch under estimated thresholds on a tile kernel, unsampled tiles between full sampled ones
        if (!p.fused || p.opt_rank <= 0 || p.item_a || p.item_b || p.narrow || p.sample_stride < 2 ||
            (long long)(p.sample_tiles - 1) * p.sample_stride >= p.full_tiles)
            bad = 1;
        if (p.rescore_cap < TILE_DOCS + 1 || (p.rescore_cap & (p.rescore_cap - 1))) bad = 1;
        bad |= check_map(p.tiles, (int)p.sample_stride, p.sample_tiles);
    }
    if (bad) printf("FAIL plan %s\n", what);
    return bad;
}

int main() {
    int bad = 0, maps = 0;
    // identity when nothing is left out
    for (long long v = 0; v < 100; ++v)
        if (unsampled_tile(v, 0, 0) != v) bad += 1;
    // sweep: s = 2, n = 1, n * s equal to and just below the tile count, NQ's (10475, 31, 328)
    const long long tile_counts[] = {2, 3, 4, 5, 7, 8, 16, 17, 31, 32, 33, 79, 100, 256, 257, 1000, 10475};
    const int strides[] = {2, 3, 4, 7, 8, 31, 32, 33, 64};
    for (long long tiles : tile_counts)
        for (int s : strides) {
            std::vector<int> ns = {1, 2, 3, (int)(tiles / s), (int)(tiles / s) - 1, (int)((tiles - 1) / s), (int)((tiles - 1) / s) + 1};
            for (int n : ns) {
                if (n < 1 || (long long)(n - 1) * s >= tiles) continue;   // the sampled tiles exist
                bad += check_map(tiles, s, n);
                ++maps;
            }
        }
    bad += check_map(10475, 31, 328);
    bad += check_map(79, 7, 10);
    bad += check_map(64, 2, 32);   // n * s == tiles at s = 2
    bad += check_map(63, 2, 32);
    maps += 4;

    // plans at the default knobs (default_knobs() in ccr_plan.h: what read_knobs() gives with an empty environment)
    const Knobs kn = default_knobs();
    bad += expect_skip("NQ k=100", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn), 1);
    // (k = 1001: measured, the 250 joined rows per query cost the select more than the main pass saves -- the planner's own choice
    // leaves it off; pinned on below)
    bad += expect_skip("NQ k=1001", make_plan(2681468, 768, 3452, 1001, CCR_SEARCH_DEFAULT, 256, kn), 0);
    {
        Knobs c = kn;
        c.optimistic = 0;   // conservative thresholds (phased at NQ)
        const Plan p = make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c);
        bad += expect_skip("NQ k=100 conservative (phased)", p, 0);
        if (p.opt_rank != 0 || p.item_a <= 0) bad += 1;
        c.progressive = 0;
        bad += expect_skip("NQ k=100 conservative, single launch", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 0);
    }
    {
        const Plan p = make_plan(2681468, 768, 40, 100, CCR_SEARCH_DEFAULT, 256, kn);   // small batch: the streaming kernel
        bad += expect_skip("NQ 40 queries (streaming)", p, 0);
        if (!p.narrow) bad += 1;
    }
    bad += expect_skip("NQ forced dense", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_FORCE_DENSE, 256, kn), 0);
    {
        Knobs c = kn;
        c.skip_sampled = 0;   // the A/B knob
        bad += expect_skip("NQ k=100, CCR_SKIP_SAMPLED=0", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 0);
    }
    {
        Knobs c = kn;
        c.skip_sampled = 1;   // pinned on: what the GPU tests run
        bad += expect_skip("NQ k=100, CCR_SKIP_SAMPLED=1", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 1);
        bad += expect_skip("NQ k=1001, CCR_SKIP_SAMPLED=1", make_plan(2681468, 768, 3452, 1001, CCR_SEARCH_DEFAULT, 256, c), 1);
        bad += expect_skip("NQ 40 queries, CCR_SKIP_SAMPLED=1 (streaming)", make_plan(2681468, 768, 40, 100, CCR_SEARCH_DEFAULT, 256, c), 0);
    }
    printf("%d maps, %d violations\n", maps, bad);
    return bad ? 1 : 0;
}
