// Host-only check of the plans that leave CUs to side work (ccr::make_plan with the side hint, CCR_SIDE_CUS; libccr_hip.so): no GPU
// call.  Built and run by tests/test_cpu_side_cus_plan.py.  Walks the shapes of planner_check.cpp at 256 CUs with every pinned count
// 0, 8 .. 64 and with the planner's own choice; prints the choice for three named shapes; exits non-zero on a violated invariant.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ccr_plan.h"

using namespace ccr;

static int fail(const char *what, long long n, int d, int nq, int k, int side) {
    printf("FAIL %s at n=%lld dim=%d nq=%d k=%d side=%d\n", what, n, d, nq, k, side);
    return 1;
}

static size_t at(const void *p) { return (size_t)(uintptr_t)p; }   // search_ws without a base: the pointers are byte offsets

// the planner's invariants that involve the main pass's grid, and the walk of its items on main_grid workgroups
static int check_plan(const Plan &p, long long n, int d, int nq, int k, int side) {
    int bad = 0;
    const SearchWs w = search_ws(p, n, d, nq, k, nullptr);
    if (p.total != w.total || p.total == 0) bad += fail("workspace total", n, d, nq, k, side);
    if (at(w.arrive) != at(w.flag_count) + 16 || at(w.arrive) + 4 > at(w.flag_list)) bad += fail("arrival counter outside the cleared flag line", n, d, nq, k, side);
    if (p.grid != 256) bad += fail("grid", n, d, nq, k, side);
    if (p.main_grid != p.grid - p.side_cus || p.main_grid % NUM_XCD || p.main_grid < NUM_XCD || p.side_cus < 0) bad += fail("main_grid", n, d, nq, k, side);
    if (p.side_cus && (!p.fused || p.narrow || p.item_a || p.item_b)) bad += fail("side CUs on a plan that is not one launch of a tile kernel", n, d, nq, k, side);
    if (!p.fused) return bad;
    if (p.ranges % NUM_XCD || p.ranges < NUM_XCD || p.ranges * p.sublists > 2048) bad += fail("ranges", n, d, nq, k, side);
    if (p.main_qblocks % p.main_qgroups || NUM_XCD % p.main_qgroups) bad += fail("main-pass query groups", n, d, nq, k, side);
    if (p.main_qsplit && (p.main_qblocks % p.main_qsplit == 0 || p.item_a)) bad += fail("unequal groups", n, d, nq, k, side);
    if (p.narrow || p.item_a) return bad;   // (phased plans walk [item_begin, item_end) per launch: planner_check.cpp)
    // the single launch: workgroup j of XCD x walks the items j, j + main_grid / 8, ... of its XCD set (ItemWalk in ccr_main_pass.hip)
    const int64_t n_vt = p.tiles - (p.skip_sampled ? p.sample_tiles : 0);
    const int count_x = p.ranges / NUM_XCD * p.main_qblocks, step = p.main_grid / NUM_XCD;
    std::vector<int> seen((size_t)p.ranges * p.main_qblocks, 0);
    int64_t tiles_walked = 0;
    for (int x = 0; x < NUM_XCD; ++x)
        for (int j = 0; j < step; ++j)
            for (int i = j; i < count_x; i += step) {
                int r = -1, qb = -1;
                const int64_t ntile = main_item(i, x, p.main_qblocks, p.main_qgroups, p.main_qsplit, p.ranges, n_vt, r, qb);
                if (r < 0 || r >= p.ranges || qb < 0 || qb >= p.main_qblocks) {
                    bad += fail("item outside the (range, block) table", n, d, nq, k, side);
                    continue;
                }
                ++seen[(size_t)r * p.main_qblocks + qb];
                if (qb == 0 && ntile > 0) tiles_walked += ntile;
            }
    for (int c : seen)
        if (c != 1) {
            bad += fail("a (range, block) cell is not covered exactly once", n, d, nq, k, side);
            break;
        }
    if (tiles_walked != n_vt) bad += fail("the ranges do not hold every tile once", n, d, nq, k, side);
    return bad;
}

static void show(const char *what, long long n, int d, int nq, int k) {
    const Knobs kn = default_knobs();
    const Plan whole = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, false), p = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, true);
    printf("%s: side_cus %d main_grid %d ranges %d (on every CU: %d), main pass %.2f ms (on every CU: %.2f), pack %.2f ms\n", what, p.side_cus, p.main_grid,
           p.ranges, whole.ranges, side_main_pass_ms(p, d), side_main_pass_ms(whole, d), side_pack_ms(n, d));
}

int main() {
    const long long rows[] = {300, 9862, 70000, 335184, 1105228, 2681468, 8841823, 6250000};
    const int dims[] = {64, 768, 1024};
    const int nqs[] = {1, 40, 300, 3452, 6980, 10000};
    const int ks[] = {1, 10, 100, 300, 1001, 4096};
    int bad = 0, total = 0, carved = 0, chosen = 0;
    for (long long n : rows)
        for (int d : dims)
            for (int nq : nqs)
                for (int k : ks) {
                    if (k > n) continue;
                    Knobs kn = default_knobs();
                    kn.side_cus = 0;
                    const Plan off = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, true);
                    bad += check_plan(off, n, d, nq, k, 0);
                    if (off.side_cus) bad += fail("CCR_SIDE_CUS=0 leaves CUs free", n, d, nq, k, 0);
                    for (int side = 8; side <= 64; side += 8) {
                        kn.side_cus = side;
                        // without the hint: the plan of CCR_SIDE_CUS=0, field for field
                        const Plan unhinted = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, false);
                        if (memcmp(&unhinted, &off, sizeof(Plan))) bad += fail("a plan without the hint differs from the plan on every CU", n, d, nq, k, side);
                        const Plan p = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, true);
                        ++total;
                        bad += check_plan(p, n, d, nq, k, side);
                        if (p.side_cus != 0 && p.side_cus != side) bad += fail("pinned count not honoured", n, d, nq, k, side);
                        // the pin applies wherever the plan on every CU is one launch of a tile kernel and stays one on fewer
                        if (p.side_cus == 0 && memcmp(&p, &off, sizeof(Plan))) bad += fail("a plan that keeps every CU differs from CCR_SIDE_CUS=0", n, d, nq, k, side);
                        carved += p.side_cus != 0;
                    }
                    // the planner's own choice
                    kn.side_cus = -1;
                    const Plan p = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn, true);
                    bad += check_plan(p, n, d, nq, k, -1);
                    if (p.side_cus % NUM_XCD) bad += fail("chosen count is no multiple of 8", n, d, nq, k, -1);
                    if (p.main_grid * SIDE_CUS_MAX_DIV < p.grid * (SIDE_CUS_MAX_DIV - 1)) bad += fail("the choice leaves the main pass fewer than 3/4 of the CUs", n, d, nq, k, -1);
                    if (off.fused && !off.narrow && !off.item_a && side_main_pass_ms(off, d) < side_pack_ms(n, d) && p.side_cus)
                        bad += fail("CUs left free although the main pass is shorter than the pack", n, d, nq, k, -1);
                    if (p.side_cus == 0 && memcmp(&p, &off, sizeof(Plan))) bad += fail("a plan that keeps every CU differs from CCR_SIDE_CUS=0", n, d, nq, k, -1);
                    chosen += p.side_cus != 0;
                }
    show("NQ k=100", 2681468, 768, 3452, 100);
    show("NQ k=1001", 2681468, 768, 3452, 1001);
    show("MS-MARCO scale", 8841823, 768, 6980, 100);
    show("one query", 2681468, 768, 1, 100);
    printf("%d pinned plans (%d with side CUs), %d chosen by the planner, %d violations\n", total, carved, chosen, bad);
    return bad ? 1 : 0;
}
