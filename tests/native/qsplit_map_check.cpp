// Host-only check of the main pass's item map (ccr::main_item in ccr_common.h) with unequal query groups, and of the plans that
// choose them (ccr::make_plan in libccr_hip.so): no GPU call.  Built and run by tests/test_cpu_qsplit_map.py.  Exits non-zero on a
// violated property.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "ccr_plan.h"

using namespace ccr;

// the map of equal groups as the kernels' item walk spelled it before main_item() existed
static long long equal_item(int i, int xcd, int qblocks, int qgroups, int ranges, long long n_vt, int &r, int &qb) {
    const int qg = xcd % qgroups, rc = xcd / qgroups, nrc = NUM_XCD / qgroups, qb_per = qblocks / qgroups;
    const int rl = i / qb_per;
    qb = qg * qb_per + i % qb_per;
    r = rc + nrc * rl;
    return (n_vt - r + ranges - 1) / ranges;
}

// One launch: B blocks, G groups (split: G does not divide B; else equal groups of G), R ranges, n_vt virtual tiles, `grid` workgroups
// that walk the items the way the kernels do (workgroup w of XCD w % 8 takes items w / 8, w / 8 + grid / 8, ...).
static int check_launch(int B, int G, bool split, int R, long long n_vt, int grid) {
    const int count = R / NUM_XCD * B, base = B / G, rem = B % G;
    std::vector<int> cell((size_t)R * B, 0);
    int bad = 0;
    for (int xcd = 0; xcd < NUM_XCD; ++xcd) {
        std::vector<int> item_r((size_t)count, -1), item_b((size_t)count, -1);
        std::vector<char> taken((size_t)count, 0);
        for (int w = xcd; w < grid; w += NUM_XCD)
            for (int i = w / NUM_XCD; i < count; i += grid / NUM_XCD) {   // every XCD set walks the same `count` items
                int r = -1, qb = -1;
                const long long nt = main_item(i, xcd, B, split ? 1 : G, split ? G : 0, R, n_vt, r, qb);
                if (taken[(size_t)i]++) bad |= 1;
                if (r < 0 || r >= R || qb < 0 || qb >= B) {
                    bad |= 2;
                    continue;
                }
                if (nt != (n_vt - r + R - 1) / R || (nt > 0) != (r < n_vt)) bad |= 4;
                cell[(size_t)r * B + qb]++;
                item_r[(size_t)i] = r;
                item_b[(size_t)i] = qb;
                if (!split) {
                    int r0, b0;
                    const long long nt0 = equal_item(i, xcd, B, G, R, n_vt, r0, b0);
                    if (r0 != r || b0 != qb || nt0 != nt) bad |= 8;
                }
            }
        for (int i = 0; i < count; ++i)
            if (!taken[(size_t)i]) bad |= 1;
        if (bad & 3) continue;
        std::set<int> blocks(item_b.begin(), item_b.end());
        if ((int)blocks.size() > base + rem) bad |= 16;                           // what an XCD's L2 has to hold
        for (int i = 1; i < count; ++i)
            if (item_r[(size_t)i] < item_r[(size_t)i - 1]) bad |= 32;             // consecutive items share a range: ranges never go back
        if (split && base >= 1) {
            std::set<int> whole_ranges;   // ranges this XCD walks for a block of its own
            for (int i = 0; i < count; ++i)
                if (item_b[(size_t)i] < G * base) whole_ranges.insert(item_r[(size_t)i]);
            for (int i = 0; i < count; ++i) {
                if (item_b[(size_t)i] >= G * base && !whole_ranges.count(item_r[(size_t)i])) bad |= 64;
                if (item_b[(size_t)i] < G * base && item_b[(size_t)i] / base != xcd % G) bad |= 128;   // whole blocks stay with their group
            }
        }
    }
    for (int c : cell)
        if (c != 1) bad |= 256;
    if (bad)
        printf("FAIL map B=%d G=%d split=%d R=%d n_vt=%lld grid=%d: %s%s%s%s%s%s%s%s%s\n", B, G, (int)split, R, n_vt, grid, bad & 1 ? "an item not walked once; " : "",
               bad & 2 ? "out of range; " : "", bad & 4 ? "tile count; " : "", bad & 8 ? "differs from the equal-group formula; " : "",
               bad & 16 ? "more than base + rem blocks on an XCD; " : "", bad & 32 ? "ranges go back; " : "",
               bad & 64 ? "a shared block in a range the XCD does not walk; " : "", bad & 128 ? "a whole block off its group; " : "",
               bad & 256 ? "a (range, block) cell not exactly once; " : "");
    return bad ? 1 : 0;
}

static int expect_plan(const char *what, const Plan &p, int want_split, int want_tile) {
    printf("%s: fused %d tile_q %d blocks %d groups %d opt_rank %d phases %d/%d narrow %d ranges %d, split %d\n", what, p.fused, p.tile_q, p.main_qblocks,
           p.main_qgroups, p.opt_rank, p.item_a, p.item_b, p.narrow, p.ranges, p.main_qsplit);
    int bad = 0;
    if (p.main_qsplit != want_split) bad = 1;
    if (want_tile && p.tile_q != want_tile) bad = 1;
    if (p.main_qsplit) {
        // the conditions of a split: one launch of a tile kernel, G in {2, 4, 8} that does not divide the blocks; the equal groups keep their value
        const int G = p.main_qsplit;
        if (!p.fused || p.item_a || p.item_b || p.narrow || !(G == 2 || G == 4 || G == 8) || p.main_qblocks % G == 0) bad = 1;
        if (p.main_qgroups < 1 || p.main_qblocks % p.main_qgroups) bad = 1;
        if (!bad) bad |= check_launch(p.main_qblocks, G, true, p.ranges, p.skip_sampled ? p.tiles - p.sample_tiles : p.tiles, p.grid);
    }
    if (bad) printf("FAIL plan %s\n", what);
    return bad;
}

int main() {
    int bad = 0, maps = 0;
    const int grids[] = {8, 256};
    for (int B = 1; B <= 40; ++B)
        for (int R = NUM_XCD; R <= 128; R += NUM_XCD) {
            const long long n_vts[] = {1, R / 2 + 1, R - 1, R, R + 1, 3LL * R + 5, 10475};
            for (long long n_vt : n_vts)
                for (int grid : grids) {
                    for (int G = 2; G <= NUM_XCD; G *= 2) {
                        bad += check_launch(B, G, B % G != 0, R, n_vt, grid);   // a split where G leaves blocks over, else equal groups of G
                        ++maps;
                    }
                    bad += check_launch(B, 1, false, R, n_vt, grid);
                    ++maps;
                }
        }

    // plans at the default knobs (default_knobs() in ccr_plan.h: what read_knobs() gives with an empty environment)
    const Knobs kn = default_knobs();
    bad += expect_plan("NQ k=100", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn), 2, WIDE_Q);
    bad += expect_plan("NQ k=1001", make_plan(2681468, 768, 3452, 1001, CCR_SEARCH_DEFAULT, 256, kn), 2, WIDE_Q);
    bad += expect_plan("dim 768, 6980 queries", make_plan(8841823, 768, 6980, 100, CCR_SEARCH_DEFAULT, 256, kn), 0, TILE_Q);
    bad += expect_plan("NQ shape, 6980 queries", make_plan(2681468, 768, 6980, 100, CCR_SEARCH_DEFAULT, 256, kn), 0, TILE_Q);
    {
        Knobs c = kn;
        c.optimistic = 0;   // conservative thresholds: phased at NQ
        const Plan p = make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c);
        bad += expect_plan("NQ k=100 conservative (phased)", p, 0, WIDE_Q);
        if (p.opt_rank != 0 || p.item_a <= 0) bad += 1;
    }
    {
        const Plan p = make_plan(2681468, 768, 40, 100, CCR_SEARCH_DEFAULT, 256, kn);   // small batch: the streaming kernel
        bad += expect_plan("NQ 40 queries (streaming)", p, 0, 0);
        if (!p.narrow) bad += 1;
        Knobs c = kn;
        c.qsplit = 1;
        bad += expect_plan("NQ 40 queries, CCR_QSPLIT=1 (streaming)", make_plan(2681468, 768, 40, 100, CCR_SEARCH_DEFAULT, 256, c), 0, 0);
    }
    bad += expect_plan("NQ forced dense", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_FORCE_DENSE, 256, kn), 0, 0);
    {
        Knobs c = kn;
        c.qsplit = 0;   // the A/B knob
        bad += expect_plan("NQ k=100, CCR_QSPLIT=0", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 0, WIDE_Q);
        bad += expect_plan("NQ k=1001, CCR_QSPLIT=0", make_plan(2681468, 768, 3452, 1001, CCR_SEARCH_DEFAULT, 256, c), 0, WIDE_Q);
        c.qgroups = 2;
        bad += expect_plan("NQ k=100, CCR_QSPLIT=0 CCR_QGROUPS=2", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 0, WIDE_Q);
        c.qsplit = 1;
        c.optimistic = 0;
        bad += expect_plan("NQ k=100 conservative (phased), CCR_QSPLIT=1 CCR_QGROUPS=2", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 0, WIDE_Q);
    }
    {
        Knobs c = kn;
        c.qsplit = 1;   // pinned on: what the GPU tests run
        c.qgroups = 8;
        bad += expect_plan("NQ k=100, CCR_QSPLIT=1 CCR_QGROUPS=8", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, c), 8, WIDE_Q);
        c.qgroups = 0;
        c.wide = 0;
        c.progressive = 0;
        bad += expect_plan("70 000 x 64, 1 025 queries on the 256-tile, CCR_QSPLIT=1", make_plan(70000, 64, 1025, 10, CCR_SEARCH_FORCE_FUSED, 256, c), 2, TILE_Q);
    }
    printf("%d maps, %d violations\n", maps, bad);
    return bad ? 1 : 0;
}
