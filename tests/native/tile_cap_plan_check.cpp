// Host-only check of the rank and the tile cap of estimated thresholds (ccr::make_plan in libccr_hip.so): no GPU call.  Built and run by
// tests/test_cpu_tile_cap_plan.py.  Prints the plans the test reads; exits non-zero on a violated invariant.
#include <stdio.h>

#include "ccr_plan.h"

using namespace ccr;

static int fail(const char *what, long long n, int d, int nq, int k) {
    printf("FAIL %s at n=%lld dim=%d nq=%d k=%d\n", what, n, d, nq, k);
    return 1;
}

static void show(const char *what, const Plan &p) {
    printf("%s: fused %d rank %d cap %d sample %d skip_sampled %d phases %d/%d\n", what, p.fused, p.opt_rank, p.tile_cap, p.sample_tiles, p.skip_sampled,
           p.item_a, p.item_b);
}

int main() {
    int bad = 0, estimated = 0, total = 0;
    // the planner's own choices over a grid of shapes, at the default knobs and with estimated thresholds wherever the sample allows
    const long long rows[] = {9862, 16640, 70000, 335184, 1105228, 2681468, 8841823};
    const int dims[] = {64, 768}, nqs[] = {1, 40, 300, 3452, 6980}, ks[] = {1, 10, 100, 300, 1001, 4096};
    for (int optimistic : {-1, 1})
        for (long long n : rows)
            for (int d : dims)
                for (int nq : nqs)
                    for (int k : ks) {
                        if (k > n) continue;
                        Knobs kn = default_knobs();
                        kn.optimistic = optimistic;
                        const Plan p = make_plan(n, d, nq, k, CCR_SEARCH_DEFAULT, 256, kn);
                        ++total;
                        if (!p.fused) continue;
                        if (!p.opt_rank) {
                            if (p.tile_cap != GROUPS_PER_TILE) bad += fail("a cap without estimated thresholds", n, d, nq, k);
                            continue;
                        }
                        ++estimated;
                        if (p.opt_rank < 17) bad += fail("rank below 17", n, d, nq, k);
                        // below the earlier floor only where the sampled tiles are left out and the sample holds forty tiles at least
                        if (p.opt_rank < 40 && (!p.skip_sampled || p.sample_tiles < 40)) bad += fail("rank below 40 outside the skip plan of a large sample", n, d, nq, k);
                        if (p.cap_rank < p.opt_rank || p.cap_rank < 40) bad += fail("capacities sized below the rank or the floor", n, d, nq, k);
                        if (p.tile_cap < 4 || p.tile_cap > GROUPS_PER_TILE) bad += fail("cap outside 4 .. 16", n, d, nq, k);
                        if (p.tile_cap < GROUPS_PER_TILE && p.tile_cap * 5 < p.opt_rank) bad += fail("cap x 5 below the rank", n, d, nq, k);
                        if (p.opt_rank <= 4 * p.tile_cap) bad += fail("four tiles can settle the rank", n, d, nq, k);
                        if (p.sample_tiles < 10) bad += fail("estimated on fewer than ten sampled tiles", n, d, nq, k);
                        if ((long long)p.tile_cap * p.sample_tiles < p.opt_rank) bad += fail("the capped groups do not hold the rank", n, d, nq, k);
                    }
    const Knobs dflt = default_knobs();
    show("NQ k=100", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, dflt));
    show("NQ k=1001", make_plan(2681468, 768, 3452, 1001, CCR_SEARCH_DEFAULT, 256, dflt));
    {
        Knobs kn = dflt;   // every tile scored: the plan and the rank of before
        kn.skip_sampled = 0;
        show("NQ k=100, CCR_SKIP_SAMPLED=0", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn));
        kn = dflt;
        kn.tile_cap = 16;
        show("NQ k=100, CCR_TILE_CAP=16", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn));
        kn.opt_rank = 13;
        show("NQ k=100, CCR_OPT_RANK=13 CCR_TILE_CAP=16", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn));
        kn.opt_rank = 40, kn.tile_cap = 0;
        show("NQ k=100, CCR_OPT_RANK=40", make_plan(2681468, 768, 3452, 100, CCR_SEARCH_DEFAULT, 256, kn));
        // small samples (forced fused searches of 65 and 40 tiles, a quarter of them sampled, every estimate the sample allows)
        kn = dflt;
        kn.narrow = 0, kn.optimistic = 1, kn.skip_sampled = 0, kn.sample_div = 4, kn.opt_rank = 17, kn.tile_cap = 1;
        show("17 sampled tiles, CCR_TILE_CAP=1", make_plan(16640, 64, 144, 10, CCR_SEARCH_FORCE_FUSED, 256, kn));
        show("10 sampled tiles, CCR_TILE_CAP=1", make_plan(10240, 256, 144, 10, CCR_SEARCH_FORCE_FUSED, 256, kn));   // rank 17 needs two groups of each
        kn.opt_rank = 0, kn.tile_cap = 0;
        show("17 sampled tiles", make_plan(16640, 64, 144, 10, CCR_SEARCH_FORCE_FUSED, 256, kn));                    // a small sample keeps the floor
        kn.sample_div = 0;
        show("4 sampled tiles", make_plan(16640, 64, 300, 10, CCR_SEARCH_FORCE_FUSED, 256, kn));                      // too few to estimate from
    }
    printf("%d plans (%d with estimated thresholds), %d violations\n", total, estimated, bad);
    return bad ? 1 : 0;
}
