// plan_dump -- what the search planner (ccr::make_plan in libccr_hip.so) decides, host-only: no GPU call.
//   hipcc -O1 -std=c++17 -I include -I crowd-coachable-recommendations_amd/csrc tools/plan_dump.cpp -o plan_dump -L crowd-coachable-recommendations_amd/lib -lccr_hip -Wl,-rpath,$PWD/crowd-coachable-recommendations_amd/lib
//
//   plan_dump n_rows dim n_q k [flags] [num_cu] [side_hint]
//                                                 every field of that search's plan and the workspace offsets (knobs from the CCR_*
//                                                 environment, flags as in ccr_retrieval.h, 256 CUs; side_hint 1: the plan of a search
//                                                 that may leave CUs to side work): what one wants beside a profile
//   plan_dump --grid                              a fixed grid of shapes under a dozen knob variants: per variant the plan count, the
//                                                 fused count and a 64-bit FNV-1a hash over every field of every plan.  A change of
//                                                 the planner that is meant to keep every plan prints the same lines before and after
//                                                 -- on ONE machine: pow() is not correctly rounded, so no hash is kept as a golden value.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ccr_plan.h"

using namespace ccr;

// THE list of what a plan holds: the printer and the hash both walk it.  f(name, value as long long).
template <class F>
static void plan_fields(const Plan &p, const SearchWs &w, F f) {
    auto off = [](const void *ptr) { return (long long)(uintptr_t)ptr; };   // search_ws without a base: the pointers are byte offsets
    f("fused", p.fused);
    f("nq_pad", p.nq_pad);
    f("qblocks", p.qblocks);
    f("tile_q", p.tile_q);
    f("main_qblocks", p.main_qblocks);
    f("main_qgroups", p.main_qgroups);
    f("main_qsplit", p.main_qsplit);
    f("tiles", p.tiles);
    f("full_tiles", p.full_tiles);
    f("sample_tiles", p.sample_tiles);
    f("sample_stride", p.sample_stride);
    f("sample_ranges", p.sample_ranges);
    f("ranges", p.ranges);
    f("item_a", p.item_a);
    f("item_b", p.item_b);
    f("opt_rank", p.opt_rank);
    f("tile_cap", p.tile_cap);
    f("cap_rank", p.cap_rank);
    f("skip_sampled", p.skip_sampled);
    f("qgroups", p.qgroups);
    f("cap", p.cap);
    f("cand.nseg", p.cand.nseg);
    f("cand.seg_end[0]", p.cand.seg_end[0]);
    f("cand.seg_end[1]", p.cand.seg_end[1]);
    f("cand.seg_end[2]", p.cand.seg_end[2]);
    f("cand.cap[0]", p.cand.cap[0]);
    f("cand.cap[1]", p.cand.cap[1]);
    f("cand.cap[2]", p.cand.cap[2]);
    f("cand.base[0]", p.cand.base[0]);
    f("cand.base[1]", p.cand.base[1]);
    f("cand.base[2]", p.cand.base[2]);
    f("grid", p.grid);
    f("main_grid", p.main_grid);
    f("side_cus", p.side_cus);
    f("rescore_cap", p.rescore_cap);
    f("rescore_regular", p.rescore_regular);
    f("select_compact", p.select_compact);
    f("mfma16", p.mfma16);
    f("sublists", p.sublists);
    f("narrow", p.narrow);
    f("narrow_groups", p.narrow_groups);
    f("first_nsub", p.first_nsub);
    f("first_sp", p.first_sp);
    f("first_lay.nseg", p.first_lay.nseg);
    f("first_lay.seg_end[0]", p.first_lay.seg_end[0]);
    f("first_lay.seg_end[1]", p.first_lay.seg_end[1]);
    f("first_lay.seg_end[2]", p.first_lay.seg_end[2]);
    f("first_lay.cap[0]", p.first_lay.cap[0]);
    f("first_lay.cap[1]", p.first_lay.cap[1]);
    f("first_lay.cap[2]", p.first_lay.cap[2]);
    f("first_lay.base[0]", p.first_lay.base[0]);
    f("first_lay.base[1]", p.first_lay.base[1]);
    f("first_lay.base[2]", p.first_lay.base[2]);
    f("cand_recs", p.cand_recs);
    f("dense_rows_per_chunk", p.dense_rows_per_chunk);
    f("total", (long long)p.total);
    // where search_ws() puts the buffers of this plan
    f("ws.qnorm", off(w.qnorm));
    f("ws.thr", off(w.thr));
    f("ws.gmax", off(w.gmax));
    f("ws.cnt", off(w.cnt));
    f("ws.cand", off(w.cand));
    f("ws.flag", off(w.flag_count));
    f("ws.top", off(w.top));
    f("ws.thr_safe", off(w.thr_safe));
    f("ws.glist", off(w.glist));
    f("ws.dense", off(w.dense));
    f("ws.retry", off(w.Q2));
    f("ws.cand_bytes", (long long)w.cand_bytes);
    f("ws.dense_bytes", (long long)w.dense_bytes);
    f("ws.retry_bytes", (long long)w.retry_bytes);
    f("ws.total", (long long)w.total);
}

static int dump_one(long long n, int dim, int nq, int k, int flags, int num_cu, bool side_hint) {
    const Plan p = make_plan(n, dim, nq, k, flags, num_cu, read_knobs(), side_hint);
    printf("n_rows %lld dim %d n_q %d k %d flags %d num_cu %d side_hint %d\n", n, dim, nq, k, flags, num_cu, (int)side_hint);
    plan_fields(p, search_ws(p, n, dim, nq, k, nullptr), [](const char *name, long long v) { printf("  %-22s %lld\n", name, v); });
    return 0;
}

struct Variant {
    const char *name;
    Knobs kn;
    int num_cu;
    int stride;   // every stride-th point of the grid's cross product
};

static Variant variant(const char *name, int num_cu, int stride) { return {name, default_knobs(), num_cu, stride}; }

static int dump_grid() {
    // the shapes of tests/native/planner_check.cpp, plus widths that are no multiple of 32, the query counts at which the streaming
    // kernel, the tile and the block count change, and ks on both sides of the skip rule and of the 16x16 / 32x32 choice
    const long long rows[] = {300, 9862, 70000, 335184, 1105228, 2681468, 8841823, 6250000};
    const int dims[] = {64, 768, 1024, 8, 200};
    const int nqs[] = {1, 40, 300, 3452, 6980, 10000, 16, 17, 64, 65, 96, 97, 128, 129, 1025, 4096, 16384};
    const int ks[] = {1, 10, 100, 300, 1001, 4096, 240, 513};
    const int flag_set[] = {CCR_SEARCH_DEFAULT, CCR_SEARCH_FORCE_DENSE, CCR_SEARCH_FORCE_FUSED};
    // Together the variants touch every knob the planner reads.  The cross product (16 320 points) is thinned per variant: half of it
    // at the defaults, every 17th point elsewhere (another residue per variant) -- about 24 000 plans, 10 s.
    Variant vs[] = {variant("default", 256, 2),          variant("default", 64, 7),          variant("planner_check legs", 256, 17),
                    variant("optimistic=0", 256, 17),    variant("optimistic=1", 256, 17),   variant("progressive=0", 256, 17),
                    variant("phases=2 optimistic=0", 256, 17), variant("mfma16=0", 256, 17), variant("mfma16=1 max_lists=512", 256, 17),
                    variant("sample_div=16", 256, 17),   variant("ranges=64 qgroups=2", 256, 17), variant("opt_rank=13", 256, 17),
                    variant("wide=0 qsplit=1", 256, 17), variant("wide=1 qgroups=8 qsplit=1", 256, 17), variant("skip_sampled=1", 256, 17),
                    variant("narrow_groups=1 skip_sampled=0", 256, 17), variant("side hint", 256, 17), variant("side hint side_cus=24", 256, 17)};
    int v = 2;
    vs[v].kn.narrow = vs[v].kn.skip_sampled = vs[v].kn.skip_list = vs[v].kn.qsplit = vs[v].kn.narrow_groups = 0, ++v;
    vs[v++].kn.optimistic = 0;
    vs[v++].kn.optimistic = 1;
    vs[v++].kn.progressive = 0;
    vs[v].kn.max_phases = 2, vs[v].kn.optimistic = 0, ++v;
    vs[v++].kn.mfma16 = 0;
    vs[v].kn.mfma16 = 1, vs[v].kn.max_lists = 512, ++v;
    vs[v++].kn.sample_div = 16;
    vs[v].kn.ranges = 64, vs[v].kn.qgroups = 2, ++v;
    vs[v++].kn.opt_rank = 13;
    vs[v].kn.wide = 0, vs[v].kn.qsplit = 1, ++v;
    vs[v].kn.wide = 1, vs[v].kn.qgroups = 8, vs[v].kn.qsplit = 1, ++v;
    vs[v++].kn.skip_sampled = 1;
    vs[v].kn.narrow_groups = 1, vs[v].kn.skip_sampled = 0, ++v;
    const int first_hinted = v++;   // the last two variants plan with the side hint
    vs[v++].kn.side_cus = 24;

    long long all_plans = 0;
    unsigned long long all_hash = 0xcbf29ce484222325ull;
    int vi = 0;
    for (const Variant &var : vs) {
        unsigned long long h = 0xcbf29ce484222325ull;
        auto mix = [&h](const char *, long long val) {
            for (int b = 0; b < 8; ++b) h = (h ^ (unsigned char)((unsigned long long)val >> (8 * b))) * 0x100000001b3ull;
        };
        long long point = 0, plans = 0, fused = 0;
        for (long long n : rows)
            for (int d : dims)
                for (int nq : nqs)
                    for (int k : ks)
                        for (int flags : flag_set) {
                            if (point++ % var.stride != vi % var.stride || k > n) continue;
                            const Plan p = make_plan(n, d, nq, k, flags, var.num_cu, var.kn, vi >= first_hinted);
                            plan_fields(p, search_ws(p, n, d, nq, k, nullptr), mix);
                            ++plans;
                            fused += p.fused;
                        }
        printf("%-32s num_cu %3d: %5lld plans (%5lld fused), hash %016llx\n", var.name, var.num_cu, plans, fused, h);
        all_plans += plans;
        for (int b = 0; b < 8; ++b) all_hash = (all_hash ^ (unsigned char)(h >> (8 * b))) * 0x100000001b3ull;
        ++vi;
    }
    printf("%lld plans in all, hash of the hashes %016llx\n", all_plans, all_hash);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--grid")) return dump_grid();
    if (argc < 5 || argc > 8) {
        fprintf(stderr, "usage: %s n_rows dim n_q k [flags] [num_cu] [side_hint]   |   %s --grid\n", argv[0], argv[0]);
        return 2;
    }
    return dump_one(atoll(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argc > 5 ? atoi(argv[5]) : CCR_SEARCH_DEFAULT,
                    argc > 6 ? atoi(argv[6]) : 256, argc > 7 && atoi(argv[7]) != 0);
}
