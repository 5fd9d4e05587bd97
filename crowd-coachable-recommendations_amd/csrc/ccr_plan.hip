// ccr_plan.hip -- the search planner: what one search launches (tile, sample, ranges, phases, thresholds, skip, query groups,
// candidate segments) and where its workspace lies.  Host code only: no kernel, no GPU call -- tests/native/ and tools/plan_dump.cpp
// run it on a machine without a GPU.
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <vector>

#include "ccr_index.h"
#include "ccr_topk_device.h"

namespace ccr {

// ------------------------------------------------------------------ knobs
Knobs read_knobs() {
    Knobs kn = default_knobs();
    for (const KnobDef &d : KNOB_DEFS)
        if (const char *e = getenv(d.env)) kn.*d.field = atoi(e);
    return kn;
}

// ------------------------------------------------------------------ the model's constants and formulas, each ONCE
// Query bytes one XCD walks in a main pass against its 4-MiB L2: they stay resident beside the corpus stream up to 3.2 MiB, mostly
// up to 5.5 MiB, and stream past it beyond (the per-flop table of the wide tile, the unequal groups' reason to exist).
constexpr double L2_RESIDENT_BYTES = 3.2 * 1048576.0, L2_MOSTLY_BYTES = 5.5 * 1048576.0;
// a 256 x 384 tile in units of the 256 x 256 tile the other terms were measured in (1.5x the multiply-adds at ~1.09x the rate)
constexpr double WIDE_TILE_COST = 1.37;
// The per-query terms were measured at 3 452 queries (14 query blocks = 3 584 columns) and scale with the query count.
constexpr double MODEL_QUERIES = 3584.0;

static double tile_cost(const Plan &p) { return p.tile_q == WIDE_Q ? WIDE_TILE_COST : 1.0; }
static double query_scale(const Plan &p) { return (double)p.nq_pad / MODEL_QUERIES; }

// A threshold that is the r-th order statistic of what was seen has a Gamma(r)-distributed pass rate: an upper quantile of it is
// (r + 4.75 sqrt(r) + 8) / r times the mean (15 x at r = 1, 1.6 x at r = 100, 1.16 x at r = 1000) -- times 1.25 for uneven data.
static double gamma_upper(double r) { return 1.25 * (r + 4.75 * sqrt(r) + 8.0) / r; }

// Rows per query that pass ESTIMATED thresholds (the rank-th largest group maximum of a sample of the corpus fraction fs): about
// rank / fs over the whole corpus, and the plan needs k of them.
static double estimated_pass(int rank, double fs, int k) { return std::max((double)rank / fs, (double)k); }
// the corpus fraction of the plan's sample, as the capacities see it
static double sample_fraction(const Plan &p) { return 1.0 / ((double)p.tiles / (double)p.sample_tiles); }
// ... and its upper quantile for the rank the plan's capacities are sized for (opt_rank > 0: cap_rank)
static double estimated_pass_upper(const Plan &p, int k) {
    return gamma_upper((double)p.cap_rank) * estimated_pass(p.cap_rank, sample_fraction(p), k);
}
// survivors per query under the sample's CONSERVATIVE thresholds alone
static double conservative_pass(const Plan &p, int k) { return (double)k * ((double)p.tiles / (double)p.sample_tiles) * 1.3 + 64.0; }

// ------------------------------------------------------------------ query groups
// Query-block groups per XCD set (pick_qgroups): the smallest divisor of qblocks among {1,2,4,8} that keeps one XCD's
// query rows (qblocks / groups blocks of tile_q rows) within ~3 MiB of its 4-MiB L2.  These are the EQUAL groups every launch
// knows; a block count they cannot cut small enough (nine = 3 x 3, a prime) gets unequal groups in a single-launch main pass
// (pick_qsplit).
int pick_qgroups(int qblocks, int dim, const Knobs &kn, int tile_q) {
    {
        const int v = kn.qgroups;
        if ((v == 1 || v == 2 || v == 4 || v == 8) && qblocks % v == 0) return v;
    }
    const size_t block_bytes = (size_t)tile_q * dim * 2;
    int best = 1;
    for (int gq = 1; gq <= NUM_XCD; gq *= 2) {
        if (qblocks % gq) continue;
        best = gq;
        if ((size_t)(qblocks / gq) * block_bytes <= (size_t)3 << 20) break;
    }
    return best;
}

// Price class of the query bytes one XCD walks in a main pass (the per-flop table of the wide tile): they stay in its 4-MiB L2
// beside the corpus stream (0), mostly (1), or stream past it (2).
static int footprint_class(double bytes) { return bytes <= L2_RESIDENT_BYTES ? 0 : (bytes <= L2_MOSTLY_BYTES ? 1 : 2); }

// Unequal query groups of a single-launch main pass (main_item() in ccr_common.h): G in {2, 4, 8} that does NOT divide the block
// count, each group base = qblocks / G whole blocks, the qblocks % G left-over blocks shared range row by range row, so that an XCD
// walks base + rem blocks.  0 = keep the equal groups.  The planner's own choice: the smallest G whose footprint reaches a better
// price class than the equal groups' (NQ on the wide tile: nine blocks = 5.06 MiB in one group, five = 2.81 MiB with G = 2).
// CCR_QSPLIT=1: any block count that has a split gets one; a CCR_QGROUPS that does not divide the block count names G.
static int pick_qsplit(int qblocks, int equal_groups, int dim, int tile_q, const Knobs &kn) {
    if (kn.qsplit == 0) return 0;
    const int v = kn.qgroups;
    if (v == 2 || v == 4 || v == 8) return qblocks % v ? v : 0;
    const double block_bytes = (double)tile_q * dim * 2.0;
    const int equal_class = footprint_class((double)(qblocks / equal_groups) * block_bytes);
    for (int G = 2; G <= NUM_XCD; G *= 2)
        if (qblocks % G && footprint_class((double)(qblocks / G + qblocks % G) * block_bytes) < equal_class) return G;
    if (kn.qsplit == 1)
        for (int G = 2; G <= NUM_XCD; G *= 2)
            if (qblocks % G) return G;
    return 0;
}

// ------------------------------------------------------------------ sample pass
// Range count of the SAMPLE pass: its few tiles (1/16 ... 1/64 of the corpus) are cut into (range, query block) items like the main
// pass's, and with so few tiles per item the rounding decides the time: 82 sample tiles x 14 query blocks in 24 ranges are 42 items per XCD
// set = two rounds of 4- and 3-tile items, in 16 ranges one round of 6- and 5-tile items (1/8 NQ shard: 0.145 -> 0.115 ms).  The kernel's
// static assignment is simulated exactly (workgroup j of an XCD set takes items j, j + per_x, ...; item = range-row * blocks + block).
static int best_sample_ranges(int64_t n_vt, int qblocks, int qgroups, int grid) {
    const int nrc = NUM_XCD / qgroups, qb_per = qblocks / qgroups, per_x = std::max(1, grid / NUM_XCD);
    int best_r = NUM_XCD;
    double best = 1e300;
    const int64_t r_max = round_up(std::min<int64_t>(n_vt, 1024), NUM_XCD);
    std::vector<double> load((size_t)per_x);
    for (int64_t R = NUM_XCD; R <= r_max; R += NUM_XCD) {
        double worst = 0.0;
        for (int rc = 0; rc < nrc; ++rc) {   // the XCD sets of one query group differ only in their range class
            std::fill(load.begin(), load.end(), 0.0);
            const int64_t items = R / nrc * qb_per;
            for (int64_t item = 0; item < items; ++item) {
                const int64_t r = rc + nrc * (item / qb_per);
                const int64_t ntile = (n_vt - r + R - 1) / R;
                if (ntile > 0) load[(size_t)(item % per_x)] += (double)ntile + 0.15;   // + pipeline fill per item
            }
            worst = std::max(worst, *std::max_element(load.begin(), load.end()));
        }
        if (worst < best - 1e-9) {
            best = worst;
            best_r = (int)R;
        }
    }
    return best_r;
}

constexpr size_t DENSE_SCRATCH_TARGET = (size_t)1 << 30;  // ~1 GiB of score rows per dense chunk

// ------------------------------------------------------------------ main-pass planner
// Work items of the main pass are (range, query block); range r owns the tiles r, r + R, ...  An XCD set of per_x
// workgroups walks (R / nrc) * qb_per items round-robin, so R (a multiple of 8, near 6 items per workgroup, items of at
// least 8 tiles) is chosen to make that count sit just below a multiple of per_x -- NQ: 128 ranges give exactly 7 items per
// workgroup where 112 left the last round 1/8 full.  The launches: phase A = one round of items with the sample
// thresholds, a re-tightening (threshold_update_kernel), optionally a second re-tightening after whole rounds, the rest.
//
// Every candidate (sample size, R, phase split) is priced in TILE UNITS of one workgroup (one 256 x 256 x dim tile ~ 22 us):
//   makespan of each launch    simulated static item assignment (+ 0.15 tile of pipeline fill per item)
//   sample pass                its tiles spread over the grid + the threshold kernel's passes over the group maxima
//   select stage               0.1 per range (it walks R x sublists sub-lists per query)
//   surviving candidates       0.014 each (filter hit path + select), a phase that covers the corpus fraction f with
//                              thresholds taken from a fraction g seen before lets through k * f / g rows per query
//                              (measured: 3 280 from a 1/32 sample alone, 1 180 with one re-tightening at k = 100)
//   launch boundary            3 per extra phase
// The per-query terms were measured at 3 452 queries (14 query blocks) and scale with the query count.
struct MainPassChoice {
    int64_t sample, ranges;
    int item_a, item_b;   // phase ends in work items of one XCD set (0 = absent)
    int opt_rank;         // > 0: ESTIMATED thresholds (the opt_rank-th largest sampled group maximum), single launch, verified by the select
    int skip;             // 1: that launch leaves out the sampled tiles (the select joins their rows from the group maxima)
};

// May a single-launch estimated-threshold main pass leave out the `sample` sampled tiles?  Only a tile kernel (not the streaming
// kernel of small batches), only when unsampled tiles lie between the sampled ones (stride >= 2) and every sampled tile is a full
// tile.  Every other plan -- conservative, phased, streaming -- and the retry, margin and dense paths score every tile.
static bool may_skip_sampled(const Plan &p, int64_t sample, const Knobs &kn) {
    if (kn.skip_sampled == 0 || p.narrow || sample < 1) return false;
    const int64_t stride = std::max<int64_t>(1, p.full_tiles / sample);
    return stride >= 2 && (sample - 1) * stride < p.full_tiles && sample < p.tiles;
}

// Estimated ("optimistic") thresholds.  The conservative threshold -- the k-th largest group maximum of a sample of the corpus
// fraction fs -- lets k / fs rows per query through the first phase, so large k needs a big sample (1/16 at k = 1001: 1/16 of the
// corpus scored twice) and two re-tightenings.  But the filter does not need a BOUND: any threshold tau works if at least k rows
// turn out to pass it with their lower bounds (then the k-th largest exact score is >= tau and every row that could reach it was
// recorded) -- which the select stage checks (L >= tau; a query that fails is retried under a valid bound).  So tau is set to
// the r-th largest sampled group maximum: about r / fs rows pass over the WHOLE corpus in ONE launch.  Given r, the pass count is
// (r / fs) x Gamma(r) / r: fewer than k rows pass iff Gamma(r) < k fs.  r is the smallest rank whose 1e-7 lower quantile
// (Wilson-Hilferty: r (1 - 1/(9r) - 5.2 sqrt(1/(9r)))^3) reaches k fs -- k = 100 on a 1/32 sample: r = 18, k = 1001 on a 1/64
// sample: r = 41, 2 700 rows pass.
// The tile cap: a corpus in topical order can fool the estimate when the sample holds a tile that lies inside a query's cluster:
// all 16 group maxima of that ONE tile are high, and a rank of 16 or less is then settled by it alone (measured with r = 13 at
// k = 100 on the topically sorted bench corpus: one query in 3 452 fails the check, and its retry costs 5 ms of an 18-ms step).
// So a sampled tile may speak for only tile_cap = ceil(r / 5), at least 4, of its groups (tile_cap_for): tau is the r-th largest
// lower bound among the groups that are among the tile_cap largest of their own sampled tile, and with r >= 4 x 4 + 1 = 17 no
// fewer than five tiles determine it.  Results do not change: any tau is valid if at least k recorded rows pass it
// with their lower bounds, which the select verifies and a failing query's retry under the conservative bound repairs; and for a
// given rank the capped tau is never above the uncapped one -- leaving values out can only lower the r-th largest -- so the cap
// lets more rows through, never fewer, than the statistics above count on.  Exact either way.
// Where the rank may be that small: the rule before the cap was a floor of OPT_RANK_FLOOR = 40 under the rank (three whole tiles), which
// cost 2.3 x the candidates on EVERY corpus at k = 100.  The floor goes where the cap can stand in for it, and stays elsewhere:
//   * the plan that leaves out the sampled tiles (skip, the re-priced plan of choose_launches) on a sample of at least
//     REDUCED_RANK_MIN_TILES = 40 tiles takes the formula's rank, at least 17: the five tiles that settle tau are then an eighth of
//     the sample at most.  This is the flagship plan: rank 18 on 328 sampled tiles.
//   * a smaller sample keeps the floor: with ten sampled tiles five are half of what was seen, and rows that sit in the sampled
//     tiles only -- tests/test_gpu_skip_sampled.py plants 140 of them -- set a rank of 17 for every query (124 of 300 queries
//     failed the check there, the query of the hot tile among them; none of that kind under rank 40);
//   * a plan that scores every tile keeps the floor: the sample size and the kind of plan are chosen on that price, as before
//     (choose_main_pass), and the planner's invariant check (tests/native/planner_check.cpp) holds such plans to a rank of 40.
// The cap itself applies to every estimated threshold, whatever set its rank.
// (skip: the main pass leaves out the sampled tiles, so the k rows must pass among the unsampled fraction 1 - fs: k fs / (1 - fs))
static int optimistic_rank(int k, int64_t sample, int64_t tiles, const Knobs &kn, bool skip = false) {
    if (kn.opt_rank > 0) return kn.opt_rank;   // tests: a small rank makes most queries fail the check
    const double need = (double)k * (double)sample / (double)(skip ? tiles - sample : tiles);
    int r = (skip && sample >= REDUCED_RANK_MIN_TILES) ? OPT_RANK_MIN : OPT_RANK_FLOOR;
    for (; r < 1 << 20; ++r) {
        const double a = 1.0 / (9.0 * r), t = 1.0 - a - 5.2 * sqrt(a);
        if (t > 0.0 && (double)r * t * t * t >= need) break;
    }
    return r;
}

// Groups of one sampled tile that count towards the rank of an estimated threshold (above): ceil(rank / 5) within [4, 16]; 16 = all
// of them, no cap.  CCR_TILE_CAP pins it (1 .. 16).  Either way the cap is raised to what leaves `rank` groups eligible on `sample`
// tiles, so that the threshold kernels always find their rank (a pinned rank or cap on a small sample).
static int tile_cap_for(int rank, int64_t sample, const Knobs &kn) {
    int cap = (rank + TILE_CAP_TILES - 1) / TILE_CAP_TILES;
    cap = std::min(GROUPS_PER_TILE, std::max(TILE_CAP_MIN, cap));
    if (kn.tile_cap >= 1 && kn.tile_cap <= GROUPS_PER_TILE) cap = kn.tile_cap;
    const int64_t fill = ((int64_t)rank + sample - 1) / std::max<int64_t>(1, sample);
    return (int)std::min<int64_t>(GROUPS_PER_TILE, std::max<int64_t>(cap, fill));
}

// The window of range counts a plan is priced over: r_hi = most ranges the select stage walks, target = ~6 items per workgroup.
static void range_window(const Plan &p, const Knobs &kn, int64_t &r_hi, int64_t &target) {
    // the select stage walks ranges x sublists sub-lists per query: 1 024 with its 256-thread form, 2 048 with the 1 024-thread
    // form large k uses anyway (rescore_cap > 512)
    int64_t max_lists = p.rescore_cap > 512 ? 2048 : 1024;
    // one or two query blocks: 128 ranges x 8 sub-lists would leave half of the workgroups without a work item (n_q = 1: main pass
    // 1.34 ms instead of 0.7) -- the select stage's wide form walks 2 048 sub-lists, and its cost does not matter for so few queries
    if ((max_lists / p.sublists) * p.main_qblocks < p.main_grid) max_lists = 2048;
    if (kn.max_lists >= 64 && kn.max_lists < max_lists) max_lists = kn.max_lists;
    r_hi = std::min<int64_t>(max_lists / p.sublists, round_up(std::max<int64_t>(1, p.tiles / 8), NUM_XCD));
    target = std::min<int64_t>(r_hi, round_up(std::max<int64_t>(NUM_XCD, (int64_t)p.main_grid * 6 / p.main_qblocks), NUM_XCD));
}

// 0.11 ms = 4.9 units of threshold kernel for 328 sample tiles x 3 584 queries
// (the threshold kernel's time follows the number of sampled groups, not the number of queries, below ~3 500 queries: it runs
// nq_pad / 16 workgroups of four latency-bound passes -- 0.21 ms for 655 sample tiles at n_q = 1)
static double sample_cost(const Plan &p, int64_t smp) {
    return (double)((smp * p.qblocks + p.grid - 1) / p.grid) + 0.015 * (double)smp * std::max(1.0, query_scale(p));
}

// the cheapest candidate so far
struct Best {
    double cost;
    MainPassChoice choice;
    void offer(double c, const MainPassChoice &ch) {
        if (c < cost) cost = c, choice = ch;
    }
};

// The plans over R ranges on the sample smp -- one launch under conservative or estimated thresholds, two or three phases -- against
// the best so far.
// Every XCD set holds the same items = (R / classes) * blocks_per_group, all of ceil(tiles / R) tiles at most, dealt
// round-robin to its per_x workgroups: a launch over n items takes ceil(n / per_x) rounds.  Phases end at ITEM
// indices, so phase A is exactly one full round (and the middle phase whole rounds) for any R.
// reprice_skipped: see choose_main_pass.
static void price_range_count(const Plan &p, int k, const Knobs &kn, int64_t smp, int64_t R, int64_t target, bool reprice_skipped, Best &best) {
    const int nrc = NUM_XCD / p.main_qgroups, qb_per = p.main_qblocks / p.main_qgroups, per_x = p.main_grid / NUM_XCD;
    const double qscale = query_scale(p);
    const double select_per_range = 0.1 * qscale, hit_w = 0.014 * qscale, phase_w = 3.0;
    const double fs = (double)smp / (double)p.tiles;
    auto survivors = [&](double fa, double fb) -> double {   // fa, fb: corpus fractions of phases A and B1 (0 = absent)
        if (fa <= 0.0) return (double)k / fs;
        if (fb <= 0.0) return (double)k * (fa / fs + (1.0 - fa) / fa);
        return (double)k * (fa / fs + fb / fa + (1.0 - fa - fb) / (fa + fb));
    };
    const int64_t items = R / nrc * qb_per;
    const double item_cost = ((double)((p.tiles + R - 1) / R) + 0.15) * tile_cost(p);   // + pipeline fill per item
    auto rounds = [&](int64_t n) { return (double)((n + per_x - 1) / per_x); };
    const double common = sample_cost(p, smp) + select_per_range * (double)R + 1e-3 * std::abs((double)(R - target));
    const double single = rounds(items) * item_cost + hit_w * survivors(0.0, 0.0) + common;
    if (kn.optimistic != 1 && !reprice_skipped) best.offer(single, {smp, R, 0, 0, 0, 0});
    // estimated thresholds: one launch, ~rank / fs rows pass (on ten sampled tiles at least: the tile cap asks for five)
    if (kn.optimistic != 0 && smp * GROUPS_PER_TILE >= 160) {
        // (a main pass that leaves out the sampled tiles walks tiles - smp virtual tiles)
        const bool skip = reprice_skipped && may_skip_sampled(p, smp, kn);
        const int rank = optimistic_rank(k, smp, p.tiles, kn, skip);
        if ((int64_t)rank * 4 <= smp * GROUPS_PER_TILE) {
            const double opt_item = skip ? ((double)((p.tiles - smp + R - 1) / R) + 0.15) * tile_cost(p) : item_cost;
            const double opt = rounds(items) * opt_item + hit_w * estimated_pass(rank, fs, k) + common - (kn.optimistic == 1 ? 1e9 : 0.0);
            best.offer(opt, {smp, R, 0, 0, rank, skip ? 1 : 0});
        }
    }
    // phased plans: not for the re-pricing, CCR_PROGRESSIVE=0 (single launch), the streaming kernel of small batches (it has no phases)
    // or a main pass that leaves CUs to side work (one launch: make_plan tried it because the plan on every CU is one)
    if (reprice_skipped || kn.progressive == 0 || p.narrow || p.side_cus || !(items > per_x && (double)p.tiles / (double)R >= 8.0)) return;
    // the thresholds after phase A come from the ranges it completed (+ the started one for part of the queries)
    const double fa = (double)per_x / (double)items;
    best.offer((1.0 + rounds(items - per_x)) * item_cost + phase_w + hit_w * survivors(fa, 0.0) + common, {smp, R, per_x, 0, 0, 0});
    if (kn.max_phases < 3) return;   // CCR_PHASES=2: at most one re-tightening
    for (int ph = 1; ph <= 3; ++ph) {   // a second re-tightening after ph more rounds
        const int64_t ib = (int64_t)per_x * (1 + ph);
        if (ib >= items) break;
        const double fb = (double)ph * per_x / (double)items;
        best.offer((1.0 + ph + rounds(items - ib)) * item_cost + 2.0 * phase_w + hit_w * survivors(fa, fb) + common, {smp, R, per_x, (int)ib, 0, 0});
    }
}

// The cheapest plan over the distinct sample sizes `samples`.
// reprice_skipped: the second call for a plan whose first choice was a single launch under estimated thresholds on the one sample
// in `samples` and which may leave out the sampled tiles -- only that kind of plan on that sample is priced, now over the
// tiles - sample virtual tiles its launch walks (ranges, rounds, item cost).  The sample size and the kind of plan stay chosen on the
// price of scoring every tile: the re-priced model prefers twice the sample at NQ by less than its own error (the sample pass's
// tiles count as main-pass tiles that need not be walked), and the select's walk over the group maxima grows with the sample.
static MainPassChoice choose_main_pass(const Plan &p, int k, const std::vector<int64_t> &samples, const Knobs &kn, bool reprice_skipped = false) {
    int64_t r_hi, target;
    range_window(p, kn, r_hi, target);
    Best best = {1e300, {samples[0], target, 0, 0, 0, 0}};
    // R stays a multiple of the XCD count (not just of the range classes): the retry pass of flagged queries re-uses the
    // ranges with its own, possibly different, query grouping
    const int64_t r_lo = std::max<int64_t>(NUM_XCD, target / 2 / NUM_XCD * NUM_XCD);
    for (int64_t smp : samples)
        for (int64_t R = r_lo; R <= std::min(r_hi, target * 2); R += NUM_XCD) {
            if (kn.ranges > 0 && R != std::min<int64_t>(r_hi, std::max<int64_t>(r_lo, round_up(kn.ranges, NUM_XCD)))) continue;
            price_range_count(p, k, kn, smp, R, target, reprice_skipped, best);
        }
    return best.choice;
}

// ------------------------------------------------------------------ the stages of a plan
// what is asked: one search on one index
struct Search {
    int64_t n_rows;
    int dim, n_q, k, flags, num_cu;
    const Knobs &kn;
    int side_cus;   // CUs a single-launch main pass on a tile kernel leaves free (multiple of NUM_XCD; 0: none)
};

// the sample pass scores group maxima of 16 rows: 1/div of the tiles, and comfortably more groups than k
static int64_t sample_for(const Plan &p, int k, int64_t div) {
    const int64_t min_sample = (2 * (int64_t)k + GROUPS_PER_TILE - 1) / GROUPS_PER_TILE;
    return std::max<int64_t>({(p.tiles + div - 1) / div, min_sample, 4});
}
// fraction of the tiles scored by the threshold pass (the planner also prices 1/64 and 1/16); CCR_SAMPLE_DIV pins it
static bool sample_div_forced(const Knobs &kn) { return kn.sample_div >= 4 && kn.sample_div <= 256; }
static int64_t sample_div(const Knobs &kn) { return sample_div_forced(kn) ? kn.sample_div : 32; }

// geometry: what follows from the shapes alone
static Plan plan_geometry(const Search &s, int mfma16) {
    Plan p;
    memset(&p, 0, sizeof(p));
    p.nq_pad = (int)round_up(s.n_q, TILE_Q);
    p.qblocks = p.nq_pad / TILE_Q;
    p.tile_q = TILE_Q;
    p.main_qblocks = p.qblocks;
    p.main_qgroups = 1;
    p.tiles = (s.n_rows + TILE_DOCS - 1) / TILE_DOCS;
    p.full_tiles = s.n_rows / TILE_DOCS;
    p.grid = std::max(NUM_XCD, s.num_cu / NUM_XCD * NUM_XCD);
    p.side_cus = std::min(s.side_cus, p.grid - NUM_XCD);
    p.main_grid = p.grid - p.side_cus;
    p.mfma16 = mfma16;   // main pass on v_mfma_f32_16x16x32_bf16 (8 sub-lists per (range, query)) or 32x32x16 (4)
    p.sublists = p.mfma16 ? 8 : 4;
    p.rescore_cap = p.rescore_regular = std::min(8192, std::max(256, 2 * pow2_ceil(s.k)));
    return p;
}

// fused or dense: sets p.fused, returns the sample the fused path starts from
static int64_t decide_fused(const Search &s, Plan &p) {
    int64_t sample = sample_for(p, s.k, sample_div(s.kn));
    // any dim the index accepts (a multiple of 8): the fused kernels zero-fill the last 32-element K sub-stage when dim % 32 != 0
    bool fused = (s.dim % 8 == 0) && s.dim >= 8 && (sample * 4 <= p.full_tiles) && s.k <= MAX_K;
    if ((s.flags & CCR_SEARCH_FORCE_FUSED) && (s.dim % 8 == 0) && p.full_tiles >= 1) {
        // honour the request where at all possible: the sample may be the whole corpus
        if (!fused) sample = std::min<int64_t>(std::max<int64_t>(sample, 1), p.full_tiles);
        fused = sample * GROUPS_PER_TILE >= s.k;
    }
    if (s.flags & CCR_SEARCH_FORCE_DENSE) fused = false;
    p.fused = fused ? 1 : 0;
    return sample;
}

// the planner prices three sample sizes: 1/32 of the tiles, 1/64 (cheaper pass, twice the survivors of phase A) and 1/16
// (large k: phase A's survivors cost more than the second half of the sample) -- the distinct ones, the base size first
static std::vector<int64_t> sample_sizes(const Search &s, const Plan &p, int64_t sample) {
    const bool pinned = sample_div_forced(s.kn) || (s.flags & CCR_SEARCH_FORCE_FUSED);
    const int64_t sample_alt = pinned ? sample : sample_for(p, s.k, 2 * sample_div(s.kn));
    int64_t sample_big = pinned ? sample : sample_for(p, s.k, sample_div(s.kn) / 2);
    if (sample_big * 4 > p.full_tiles) sample_big = sample;
    std::vector<int64_t> sizes = {sample};
    for (int64_t v : {sample_alt, sample_big})
        if (std::find(sizes.begin(), sizes.end(), v) == sizes.end()) sizes.push_back(v);
    return sizes;
}

// small batches: the first main pass is the streaming kernel (ccr_narrow.hip) when the query rows fit its LDS image
// (65 .. 128 queries: two groups of <= 64 on paired workgroups that walk the same rows)
static void choose_streaming(const Search &s, Plan &p) {
    const Knobs &kn = s.kn;
    const int n_q = s.n_q, dim = s.dim;
    int nqt = n_q <= 16 ? 1 : (n_q <= 32 ? 2 : 4);
    int ngroups = n_q <= NARROW_MAX_Q ? 1 : 2;
    // 65 .. 96 queries: ONE group of six query tiles where their rows fit the LDS (dim <= 768) -- every corpus row is pulled once
    if (n_q > NARROW_MAX_Q && n_q <= 96 && kn.narrow_groups >= 2 && dim % TILE_K == 0 && narrow_lds_bytes(6, dim) <= (size_t)160 * 1024)
        nqt = 6, ngroups = 1;
    const bool narrow = kn.narrow != 0 && n_q <= NARROW_MAX_Q * std::min(std::max(kn.narrow_groups, 1), NARROW_MAX_GROUPS) && dim % TILE_K == 0 &&
                        narrow_lds_bytes(nqt, dim) <= (size_t)160 * 1024 && (ngroups == 1 || s.num_cu >= 16);
    p.narrow = narrow ? nqt : 0;
    p.narrow_groups = narrow ? ngroups : 1;
}

// the main pass's tile: 256 x 384 (gemm_topk16w_kernel: -17 % bytes per flop through the L1 miss path that bounds the 256 x 256
// kernel) where it pays.  Measured at the NQ corpus (profiles/r06_wide_*.txt), per padded multiply-add against the 256 x 256
// kernel: 0.92-0.96 while the query rows one XCD walks stay L2-resident (300 and 1 100 queries: main pass -31 % / -14 %, most
// of it the padding: one block instead of two, three instead of five), 0.97 at 5 MiB per XCD (3 452 queries: nine blocks =
// 3 456 columns against fourteen = 3 584: -6.5 %), and SLOWER beyond -- 4 096 queries = eleven blocks, 6 980 = nineteen: a prime
// block count has no equal groups over the XCDs, every XCD streams all the query rows past its 4-MiB L2 (L2 hit rate 0.71 against
// 0.91, +3.4 % main pass) while sixteen / twenty-eight 256-blocks split into groups that fit.
// (The tile is priced on its EQUAL groups: the unequal ones of pick_qsplit exist for a single-launch plan only, which is not
// known yet, and they have been measured at nine blocks alone -- eleven and nineteen blocks stay on the 256 x 256 tile.)
static void choose_tile(const Search &s, Plan &p) {
    const Knobs &kn = s.kn;
    const int n_q = s.n_q, dim = s.dim;
    if (!p.narrow && p.mfma16 && dim % 32 == 0 && kn.wide != 0) {
        static const double per_flop_of_class[3] = {0.95, 0.97, 1.04};
        const int wb = (n_q + WIDE_Q - 1) / WIDE_Q;
        const double per_xcd = (double)(wb / pick_qgroups(wb, dim, kn, WIDE_Q)) * WIDE_Q * dim * 2.0;   // query bytes one XCD walks
        const double per_flop = per_flop_of_class[footprint_class(per_xcd)];
        if (kn.wide == 1 || (double)wb * WIDE_Q * per_flop < (double)p.qblocks * TILE_Q) {
            p.tile_q = WIDE_Q;
            p.main_qblocks = wb;
            p.nq_pad = (int)round_up(std::max<int64_t>(n_q, (int64_t)wb * WIDE_Q), TILE_Q);   // the counters of every block's columns exist
            p.qblocks = p.nq_pad / TILE_Q;
            p.qgroups = pick_qgroups(p.qblocks, dim, kn);
        }
    }
    p.main_qgroups = pick_qgroups(p.main_qblocks, dim, kn, p.tile_q);
}

// the tile cap and the capacity rank that follow from the plan's rank and sample
static void set_rank_dependents(Plan &p, const Knobs &kn) {
    p.tile_cap = p.opt_rank > 0 ? tile_cap_for(p.opt_rank, p.sample_tiles, kn) : GROUPS_PER_TILE;
    // Capacities (sub-lists, the select's buffer) stay sized for the floor's rank where the planner's own rank is below it: a corpus
    // in topical order records several times the estimate (3 054 rows per query on the sorted bench corpus at rank 18, 575 estimated),
    // and a select buffer sized from rank 18 (2 816 entries) made that corpus 0.07 ms SLOWER than under rank 40.  A pinned rank sizes them.
    p.cap_rank = (kn.opt_rank > 0 || p.opt_rank == 0) ? p.opt_rank : std::max(p.opt_rank, OPT_RANK_FLOOR);
}

// sample size, range count, phases and thresholds of the main pass, and with them the sample pass's ranges and the query split
static void choose_launches(const Search &s, Plan &p, const std::vector<int64_t> &samples) {
    const Knobs &kn = s.kn;
    MainPassChoice choice = choose_main_pass(p, s.k, samples, kn);
    if (choice.opt_rank > 0 && may_skip_sampled(p, choice.sample, kn)) {
        const MainPassChoice skipped = choose_main_pass(p, s.k, {choice.sample}, kn, true);
        if (skipped.skip) choice = skipped;   // (else: the rank the unsampled fraction needs does not fit the sample)
    }
    p.sample_tiles = (int)choice.sample;
    p.sample_stride = std::max<int64_t>(1, p.full_tiles / choice.sample);
    p.sample_ranges = best_sample_ranges(choice.sample, p.qblocks, p.qgroups, p.grid);
    p.ranges = (int)choice.ranges;
    p.item_a = choice.item_a;
    p.item_b = choice.item_b;
    p.opt_rank = choice.opt_rank;
    set_rank_dependents(p, kn);
    p.skip_sampled = (p.opt_rank > 0 && !p.narrow) ? choice.skip : 0;
    // unequal query groups: a single launch of a tile kernel only (phase ends are item indices of the equal groups' map, and
    // the re-tightening between two phases takes a query's finished ranges from its block's place in an equal group)
    p.main_qsplit = (!p.narrow && p.item_a == 0 && p.item_b == 0) ? pick_qsplit(p.main_qblocks, p.main_qgroups, s.dim, p.tile_q, kn) : 0;
}

// skip-sampled: room for the joined rows, and whether the skip pays.
// the join can add a whole sampled tile to a query's collected rows (a corpus in topical order): room for one beside the
// regular rows (about k, and ties around the cut) -- 512 at k = 100, which keeps the select's 256-thread form.  On iid rows a
// sampled group of 16 holds a row of the top k with probability 1 - (1 - k / n)^16 and joins whole: J rows per query (50 at NQ,
// k = 100; 1 700 for k = 1001 of 300 000 rows with a tenth of them sampled: measured, every query overflowed 2 048) -- room
// for 1.5 J of them; where even 8 192 do not hold that, every tile is scored
static void price_skip_sampled(const Search &s, Plan &p) {
    if (!p.skip_sampled) return;
    const int k = s.k;
    const double join_rows = 256.0 * (double)p.sample_tiles * (1.0 - pow(1.0 - std::min(1.0, (double)k / (double)s.n_rows), 16.0));
    const double need = (double)k + (double)(k / 4) + 1.5 * join_rows + TILE_DOCS + 16;
    // the planner's own choice prices the join: a joined row costs the select 0.065 tile units (measured at NQ: + 0.06 ms for
    // 50 rows per query at k = 100, + 0.42 ms for 250 at k = 1001), the main pass saves sample x blocks / grid tiles per
    // workgroup of which the item rounding returns about half (0.29 of 0.35 ms at k = 100, 0.08 of 0.17 at k = 1001: there the
    // search got SLOWER, 13.46 against 13.10 ms) -- CCR_SKIP_SAMPLED=1 skips wherever the plan allows.
    // The three constants (0.065, the 3 584-query scale of the planner's other per-query terms, the half) are fitted to
    // those TWO measured points: at NQ the rule switches the skip off above k of about 240; nothing between the points and
    // no other query count has been measured.
    const double saved = 0.5 * (double)p.sample_tiles * p.main_qblocks * tile_cost(p) / (double)p.main_grid;
    const bool pays = 0.065 * join_rows * query_scale(p) < saved;
    if (need > 8192.0 || (s.kn.skip_sampled < 0 && !pays)) {
        p.skip_sampled = 0;
        // every tile is scored after all: the rank is not below what such a plan takes (optimistic_rank: the floor).  As before,
        // p.ranges stays the range count priced for the walk over tiles - sample, and the estimated plan is not compared again with
        // the phased and conservative plans; new is only that the rank may rise with the switch (NQ, k = 300: to the floor of 40).
        p.opt_rank = std::max(p.opt_rank, optimistic_rank(k, p.sample_tiles, p.tiles, s.kn, false));
        set_rank_dependents(p, s.kn);
    } else
        p.rescore_cap = std::min(8192, std::max(p.rescore_cap, pow2_ceil((int)need)));
}

// candidate layout of one segment over every range
CandLayout one_segment(int cap) {
    CandLayout L;
    memset(&L, 0, sizeof(L));
    L.nseg = 1;
    L.seg_end[0] = L.seg_end[1] = L.seg_end[2] = INT32_MAX;
    L.cap[0] = L.cap[1] = L.cap[2] = cap;
    return L;
}

// candidate segments and their sub-list capacities: p.cand, p.cap, p.cand_recs
static void plan_candidates(const Search &s, Plan &p) {
    const int k = s.k;
    const int64_t R = p.ranges;
    // ranges that hold items of a phase: the candidate segments (a range started in phase A keeps phase A's capacity)
    const int nrc_p = NUM_XCD / p.main_qgroups, qb_per_p = p.main_qblocks / p.main_qgroups;
    auto ranges_to = [&](int item) { return item ? std::min<int64_t>(R, (int64_t)nrc_p * ((item + qb_per_p - 1) / qb_per_p)) : 0; };
    const int64_t RA = ranges_to(p.item_a), RB = ranges_to(p.item_b);
    // Sub-list capacities, one per phase (segment).  A phase whose thresholds were taken from a corpus fraction g lets
    // k / g rows per query through, spread over R * sublists sub-lists.  Two noise terms on top of that mean:
    //   the threshold itself is the k-th order statistic of what was seen: its pass rate is Gamma(k)-distributed, an
    //     upper quantile of it is (k + 4.75 sqrt(k) + 8) / k times the mean (15 x at k = 1, 1.6 x at k = 100, 1.16 x at
    //     k = 1000) -- times 1.25 for uneven data;
    //   the count of one sub-list is Poisson around its share: + 6 sigma + 16.
    // An overflowing sub-list only flags its query for the exact path, so the model needs to be safe, not a bound.
    const double fs = sample_fraction(p), nlists = (double)R * p.sublists;
    const double xk = gamma_upper((double)k);
    // Allowance: one WHOLE tile may pass for a query (a corpus in topical order: all 256 rows of a tile belong to the
    // query's cluster); that is TILE_DOCS / sublists rows for one sub-list on top of its regular share.
    const int64_t tile_rows = TILE_DOCS / p.sublists;
    // estimated thresholds: about opt_rank / fs rows pass, Gamma(opt_rank)-distributed
    auto cap_for = [&](double g) -> int {
        const double mean = p.opt_rank ? estimated_pass_upper(p, k) / nlists : xk * (double)k / (g * nlists);
        const int64_t c = (int64_t)(mean + 6.0 * sqrt(mean)) + 16 + tile_rows;   // the model's share PLUS one whole tile
        return (int)round_up(std::min<int64_t>(std::max<int64_t>(c, 16), 8192), 4);
    };
    // corpus fractions the re-tightenings have SEEN: the ranges completed by then
    const double fa = p.item_a ? (double)(p.item_a / qb_per_p) * nrc_p / (double)R : 0.0;
    const double fb = p.item_b ? std::max(0.0, (double)(p.item_b / qb_per_p) * nrc_p / (double)R - fa) : 0.0;
    // the re-tightening selects among at most `compact` of the candidates found so far (launch_threshold_update): when
    // phase A is expected to leave more than that, the bound is the k-th of a subset and passes proportionally more
    const double upd_compact = std::min(32768.0, std::max(4096.0, 8.0 * pow2_ceil(k)));
    auto seen = [&](double g, double found) { return found > upd_compact ? g * upd_compact / found : g; };
    const double found_a = (double)k * fa / fs;
    CandLayout &L = p.cand;
    memset(&L, 0, sizeof(L));
    const int seg_end_v[3] = {RA ? (int)RA : (int)R, RB > RA ? (int)RB : (int)R, (int)R};
    int64_t recs = 0;
    int prev_end = 0;
    for (int g = 0; g < 3; ++g) L.seg_end[g] = INT32_MAX, L.cap[g] = 16;   // unused segments
    for (int g = 0; g < 3; ++g) {
        if (seg_end_v[g] <= prev_end) continue;
        const int sg = L.nseg++;
        double frac_seen = fs;                                  // phase A: the sample
        if (sg == 1) frac_seen = fa >= 2.0 * fs ? seen(fa, found_a) : fs;
        if (sg == 2) frac_seen = fa >= 2.0 * fs ? seen(fa + fb, found_a + (double)k * fb / fa) : fs;
        L.seg_end[sg] = seg_end_v[g];
        L.cap[sg] = cap_for(std::min(1.0, std::max(frac_seen, fs)));
        L.base[sg] = recs;
        recs += (int64_t)(seg_end_v[g] - prev_end) * p.nq_pad * p.sublists * L.cap[sg];
        recs = round_up(recs, 32);
        prev_end = seg_end_v[g];
    }
    L.seg_end[L.nseg - 1] = INT32_MAX;   // the last segment is open-ended (sub-list lookups never fall off the table)
    p.cap = L.cap[0];
    p.cand_recs = recs;
}

// what the select stage gathers per query, and what the FIRST main pass fills
static void plan_select_and_first_pass(const Search &s, Plan &p) {
    const int k = s.k, n_q = s.n_q;
    // survivors per query reaching the select stage: ~12 k after the progressive re-tightening, `expect` without it
    // (estimated thresholds leave fewer candidates, but the select's staged re-score borrows this area: about 1.15 k rows are
    // re-scored per query and a 64-byte slice of each needs 80 bytes = 10 entries -- a smaller area sends the re-score down its
    // unstaged path: measured 2.41 instead of 2.06 ms at k = 1001)
    const double expect = conservative_pass(p, k);
    double want = expect;
    if (p.opt_rank)
        want = std::max(estimated_pass_upper(p, k) + 512.0, k > 256 ? 18.0 * k : 0.0);   // (18 entries per re-scored row: the 128-byte slices, where the LDS budget allows)
    else if (p.item_a)
        want = 16.0 * k + 512.0;
    p.select_compact = select_compact_entries(s.dim, p.ranges * p.sublists, p.rescore_cap, (int64_t)(want * 1.25));
    // what the FIRST main pass fills: the tile kernels' (range, query) cells -- or, for the streaming kernel, one cell of two
    // sub-lists per query with whatever the candidate area gives each of them (at least 8 x the model's expectation)
    p.first_nsub = p.ranges * p.sublists;
    p.first_sp = p.sublists;
    p.first_lay = p.cand;
    if (p.narrow) {
        const double pass = p.opt_rank ? estimated_pass_upper(p, k) : expect;
        int64_t capn = std::max<int64_t>(p.cand_recs / ((int64_t)NARROW_SUBLISTS * std::max(1, n_q)), (int64_t)(8.0 * pass) + 4096);
        capn = std::min<int64_t>(capn, (int64_t)1 << 22) / 4 * 4;
        p.cand_recs = std::max<int64_t>(p.cand_recs, capn * NARROW_SUBLISTS * n_q);
        p.first_lay = one_segment((int)capn);
        p.first_nsub = NARROW_SUBLISTS;
        p.first_sp = NARROW_SUBLISTS;
    }
}

// queries per chunk of the dense path: ~1 GiB of score rows
static int64_t dense_chunk_rows(const Search &s) {
    int64_t rows = (int64_t)(DENSE_SCRATCH_TARGET / ((size_t)s.n_rows * 4));
    rows = std::min<int64_t>(std::max<int64_t>(rows, 1), s.n_q);
    if (rows >= 64) rows = rows / 64 * 64;
    return rows;
}

static Plan plan_once(const Search &s, int mfma16) {
    Plan p = plan_geometry(s, mfma16);
    const int64_t sample = decide_fused(s, p);
    if (p.fused) {
        p.qgroups = pick_qgroups(p.qblocks, s.dim, s.kn);
        const std::vector<int64_t> samples = sample_sizes(s, p, sample);
        choose_streaming(s, p);
        choose_tile(s, p);
        choose_launches(s, p, samples);
        price_skip_sampled(s, p);
        plan_candidates(s, p);
        plan_select_and_first_pass(s, p);
        p.dense_rows_per_chunk = FALLBACK_ROWS;
    } else {
        p.dense_rows_per_chunk = dense_chunk_rows(s);
    }
    p.total = search_ws(p, s.n_rows, s.dim, s.n_q, s.k, nullptr).total;   // no base: the pointers are the byte offsets
    return p;
}

// Side CUs are left by ONE launch of a tile kernel alone: a phased plan (its launches would each wait for their stragglers on fewer
// CUs), the streaming kernel and the dense path are planned again on every CU.
static Plan make_plan_for(const Search &s, int mfma16) {
    Plan p = plan_once(s, mfma16);
    if (s.side_cus == 0 || (p.fused && !p.narrow && p.item_a == 0 && p.item_b == 0)) return p;
    const Search whole = {s.n_rows, s.dim, s.n_q, s.k, s.flags, s.num_cu, s.kn, 0};
    return plan_once(whole, mfma16);
}

SearchWs search_ws(const Plan &p, int64_t n_rows, int dim, int n_q, int k, char *base) {
    SearchWs w;
    memset(&w, 0, sizeof(w));
    Bump b = {0};
    auto at = [&](size_t off) { return (char *)((uintptr_t)base + off); };
    auto take = [&](size_t bytes) { return at(b.take(bytes)); };
    if (!p.fused) {
        w.flag_count = (uint32_t *)take(64 + (size_t)n_q * 4);   // queries the margin select hands to the fp64 path
        w.arrive = w.flag_count + 4;
    w.flag_list = w.flag_count + 16;
        w.dense_bytes = (size_t)p.dense_rows_per_chunk * (n_rows + 3) * 4;
        w.dense = (float *)take(w.dense_bytes);
        w.total = b.off;
        return w;
    }
    const size_t nq_pad = p.nq_pad;
    w.qnorm = (float *)take(nq_pad * 4);
    w.thr = (float *)take(nq_pad * 8);
    w.cq = w.thr + nq_pad;
    w.gmax = (float *)take((size_t)p.sample_tiles * GROUPS_PER_TILE * nq_pad * 4);
    w.cnt = (uint32_t *)take((size_t)p.ranges * nq_pad * p.sublists * 4);
    w.cand = (uint2 *)take((size_t)p.cand_recs * 8);
    w.flag_count = (uint32_t *)take(64 + (size_t)n_q * 4);
    w.stat_cand = (unsigned long long *)(w.flag_count + 2);
    w.arrive = w.flag_count + 4;
    w.flag_list = w.flag_count + 16;
    w.cand_bytes = (char *)w.flag_count - (char *)w.cand;
    w.top = (uint32_t *)take(p.item_b ? (nq_pad + (size_t)n_q * k) * 4 : 0);
    w.thr_safe = (float *)take(p.opt_rank ? nq_pad * 8 : 0);
    w.cq_safe = w.thr_safe + nq_pad;
    w.glist = (uint32_t *)take(p.skip_sampled ? nq_pad * (size_t)(skip_list_cap(p.opt_rank) + 1) * 4 : 0);
    w.dense_bytes = (size_t)p.dense_rows_per_chunk * n_rows * 4;
    w.dense = (float *)take(w.dense_bytes);
    // the retry area keeps its reserved size: its nine sub-buffers plus up to 255 bytes of rounding each
    w.retry_bytes = nq_pad * dim * 2 + nq_pad * 8 + (size_t)n_q * 16 + 64 + 64 + (size_t)n_q * 4 + 256 * 10;
    Bump r = {b.take(w.retry_bytes)};
    w.Q2 = (uint16_t *)at(r.take(nq_pad * dim * 2));
    w.thr2 = (float *)at(r.take(nq_pad * 4));
    w.cq2 = (float *)at(r.take(nq_pad * 4));
    w.retry_list = (uint32_t *)at(r.take((size_t)n_q * 4));
    w.dense_list = (uint32_t *)at(r.take((size_t)n_q * 4));
    w.counts = (uint32_t *)at(r.take(64));
    w.flag2 = (uint32_t *)at(r.take(64 + (size_t)n_q * 4));
    w.list_b = (uint32_t *)at(r.take((size_t)n_q * 4));
    w.list_c = (uint32_t *)at(r.take((size_t)n_q * 4));
    w.total = b.off;
    return w;
}

// Which main-pass kernel: CCR_MFMA16 pins it.  Otherwise the 16x16x32 kernel (the chip holds a higher clock on that MFMA shape)
// whenever its eight sub-lists per (range, query) do not force FEWER ranges than the 32x32x16 plan wants: up to k = 512 always
// (measured), above that when the four-sub-list plan's range count times 8 stays within the select stage's 2 048
// sub-lists (config-4 shard, k = 1000, 62 ranges: main pass 111 vs 120 ms, select 8.9 vs 9.4 ms).
static Plan plan_on_best_kernel(const Search &s) {
    const Knobs &kn = s.kn;
    if (kn.mfma16 >= 0) return make_plan_for(s, kn.mfma16 ? 1 : 0);
    if (s.k <= 512) return make_plan_for(s, 1);
    const Plan p32 = make_plan_for(s, 0);
    if (p32.fused && p32.ranges * 8 <= 2048) return make_plan_for(s, 1);
    return p32;
}

// ------------------------------------------------------------------ side CUs
// A caller that re-packs the shard for its next search beside this one (ccr_search_stream_wait_main_pass) gets CUs to do it on: the
// single-launch main pass holds every register of each CU it runs on and nearly idles the HBM, the pack is HBM-bound and needs no
// matrix core.  The model, in milliseconds (profiles/side_cus.md has the points):
//   main pass      its items' rounds x tiles per item (the planner's tile units) x SIDE_TILE_MS per unit of a 768-wide tile: 9.82 ms
//                  on 256 workgroups (112 ranges, four rounds), 11.4 on 224 (72 ranges, three rounds) by the kernel trace
//   pack           n_rows x dim x 6 bytes (fp32 read, 16-bit write) at SIDE_PACK_CU_GBPS per free CU beside the main pass (measured:
//                  50 on 8 CUs, 34 or more on 32, where the 12.4-GB pack ends with the main pass), at SIDE_PACK_ALL_GBPS on the whole
//                  chip behind it (2.34 ms)
//   select         no longer covered by the pack.  The cover was worth the whole select at k = 100 (0.33 ms) and next to nothing at
//                  k = 1001, where the 1.8-ms select is HBM-bound like the pack and the step was their sum: at most SIDE_SELECT_COVER_MS
// The planner's own choice is the multiple of 8 CUs on which the pack ends about when the main pass does, at most a quarter of
// the grid; it is 0 where the main pass is shorter than the pack at full speed (the pack cannot hide behind it) and where the
// re-planned main pass grows by more than the pack's hidden part saves.  Every constant is fitted to ONE shape, the NQ step
// (2 681 468 x 768, 3 452 queries) at k = 100, on gaussian, clustered and sorted rows; at k = 1001 the same 32 CUs were measured
// (-0.5 ms); the MS-MARCO-scale step has a phased plan and keeps every CU.  No other width or query count has been measured.
constexpr double SIDE_TILE_MS = 0.0198, SIDE_PACK_CU_GBPS = 40.0, SIDE_PACK_ALL_GBPS = 5300.0, SIDE_SELECT_COVER_MS = 0.35;

// length of a single-launch main pass on a tile kernel, in tile units of one workgroup (price_range_count's first term)
static double main_pass_units(const Plan &p) {
    const int nrc = NUM_XCD / p.main_qgroups, qb_per = p.main_qblocks / p.main_qgroups, per_x = p.main_grid / NUM_XCD;
    const int64_t items = p.ranges / nrc * qb_per, walked = p.tiles - (p.skip_sampled ? p.sample_tiles : 0);
    return (double)((items + per_x - 1) / per_x) * ((double)((walked + p.ranges - 1) / p.ranges) + 0.15) * tile_cost(p);
}
static double side_ms_per_unit(const Search &s) { return SIDE_TILE_MS * (double)s.dim / 768.0; }
static double side_pack_bytes(const Search &s) { return (double)s.n_rows * s.dim * 6.0; }
double side_main_pass_ms(const Plan &p, int dim) { return main_pass_units(p) * SIDE_TILE_MS * (double)dim / 768.0; }
double side_pack_ms(int64_t n_rows, int dim) { return (double)n_rows * dim * 6.0 / (SIDE_PACK_ALL_GBPS * 1e6); }

// CUs to plan the carve with: the pinned count, or the model's (0: none)
static int side_cus_for(const Search &s, const Plan &whole) {
    const Knobs &kn = s.kn;
    if (kn.side_cus == 0 || !whole.fused || whole.narrow || whole.item_a || whole.item_b) return 0;
    if (kn.side_cus > 0) return (int)std::min<int64_t>(round_up(kn.side_cus, NUM_XCD), whole.grid - NUM_XCD);
    const double main_ms = main_pass_units(whole) * side_ms_per_unit(s), bytes = side_pack_bytes(s);
    if (main_ms < side_pack_ms(s.n_rows, s.dim)) return 0;   // the pack outlasts the main pass even on the whole chip
    const int want = (int)(bytes / (main_ms * SIDE_PACK_CU_GBPS * 1e6) / NUM_XCD + 0.5) * NUM_XCD;
    return std::min(want, whole.grid / SIDE_CUS_MAX_DIV / NUM_XCD * NUM_XCD);
}

// does the plan `carved` beat `whole` for a caller that packs beside the main pass?
static bool side_cus_pay(const Search &s, const Plan &whole, const Plan &carved) {
    const double unit = side_ms_per_unit(s), main_ms = main_pass_units(carved) * unit;
    const double cost = main_ms - main_pass_units(whole) * unit;
    const double pack_ms = side_pack_bytes(s) / (SIDE_PACK_ALL_GBPS * 1e6);
    const double hidden = std::min(pack_ms, main_ms * carved.side_cus * SIDE_PACK_CU_GBPS / SIDE_PACK_ALL_GBPS);
    const double pass = carved.opt_rank ? estimated_pass(carved.opt_rank, sample_fraction(carved), s.k) : conservative_pass(carved, s.k);
    const double select_ms = (0.1 * carved.ranges + 0.014 * pass) * query_scale(carved) * unit;   // it ran beside the pack
    return cost + std::min(select_ms, SIDE_SELECT_COVER_MS) < hidden;
}

// The plan of one search: on every CU, or -- side_hint -- with side CUs where they apply and, by the planner's own choice, pay.
Plan make_plan(int64_t n_rows, int dim, int n_q, int k, int flags, int num_cu, const Knobs &kn, bool side_hint) {
    Search s = {n_rows, dim, n_q, k, flags, num_cu, kn, 0};
    const Plan whole = plan_on_best_kernel(s);
    s.side_cus = side_hint ? side_cus_for(s, whole) : 0;
    if (s.side_cus == 0) return whole;
    const Plan carved = plan_on_best_kernel(s);
    if (carved.side_cus == 0 || (kn.side_cus < 0 && !side_cus_pay(s, whole, carved))) return whole;
    return carved;
}

}  // namespace ccr
