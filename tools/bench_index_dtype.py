#!/usr/bin/env python3
"""Same-process A/B of the search on a bf16 and on an fp16 index (CCREC_INDEX_DTYPE), alternating the two types round by round, at the
NQ shape (2 681 468 x 768, 3 452 queries, k = 100: the 256 x 384 main pass) and with the streaming pass of a 64-query batch over the
same rows.  Both indices are resident at once (two 4.1 GB shards of one seeded fp32 stream, packed by ops.pack_half); every shape is
warmed up on both types before the timed rounds; a timed search is one CorpusIndex.search between two device synchronises, next to the
library's own HIP-event times of that search.  Prints one JSON line and, with an output path, writes it there too.

  python3 tools/bench_index_dtype.py [out.json] [--rows N --queries Q --dim D --k K --rounds R --warmup W]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]


def arg(name, dflt):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    import torch
    from ccrec_amd import ops
    n, nq, d, k = arg("--rows", 2681468), arg("--queries", 3452), arg("--dim", 768), arg("--k", 100)
    rounds, warmup, small = arg("--rounds", 20), arg("--warmup", 3), 64
    types = {"bf16": torch.bfloat16, "fp16": torch.float16}
    g = torch.Generator(device="cuda").manual_seed(1234)
    shards = {name: torch.empty(n, d, dtype=dt, device="cuda") for name, dt in types.items()}
    bounds = {name: torch.empty(n, device="cuda") for name in types}
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    pack_ms = {name: [] for name in types}
    for lo in range(0, n, 1 << 19):
        hi = min(n, lo + (1 << 19))
        x = torch.randn(hi - lo, d, generator=g, device="cuda") / d ** 0.5
        for name, dt in types.items():          # the same fp32 rows into both shards
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.pack_half(x, dt, out=shards[name][lo:hi], norm_bounds=bounds[name][lo:hi], overflow=overflow if dt == torch.float16 else None)
            torch.cuda.synchronize()
            if hi - lo == 1 << 19 and lo:       # whole chunks, the first (cold) one left out
                pack_ms[name].append((time.perf_counter() - t0) * 1e3)
    q32 = torch.randn(nq, d, generator=torch.Generator(device="cuda").manual_seed(4321), device="cuda") / d ** 0.5
    queries = {name: ops.pack_half(q32, dt) for name, dt in types.items()}
    index = {name: ops.CorpusIndex(shards[name], norm_bounds=bounds[name]) for name in types}
    assert int(overflow.item()) == 0
    result = {"rows": n, "dim": d, "k": k, "rounds": rounds, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "pack_ms_per_524288_rows": {name: spread(v) for name, v in pack_ms.items() if v}}
    for label, m in (("nq%d" % nq, nq), ("nq%d" % small, small)):
        wall = {name: [] for name in types}
        total = {name: [] for name in types}
        main_ms = {name: [] for name in types}
        last = {}
        for it in range(warmup + rounds):
            for name in (("bf16", "fp16") if it % 2 == 0 else ("fp16", "bf16")):       # alternate, and alternate who goes first
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s, i = index[name].search(queries[name][:m], k)
                torch.cuda.synchronize()
                dt_ms = (time.perf_counter() - t0) * 1e3
                st = index[name].last_stats()
                if it >= warmup:
                    wall[name].append(dt_ms)
                    total[name].append(st["ms_total"])
                    main_ms[name].append(st["ms_main"])
                last[name] = (st, i)
        # the two types rank different roundings of the same rows: how much of the top-k they share is reported, not asserted
        same_pos = float((last["bf16"][1] == last["fp16"][1]).float().mean())
        result[label] = {name: {"wall_ms": spread(wall[name]), "library_total_ms": spread(total[name]), "main_pass_ms": spread(main_ms[name]),
                                "main_tile_queries": last[name][0]["main_tile_queries"], "n_fallback": last[name][0]["n_fallback"],
                                "queries_per_s": round(m / (statistics.median(wall[name]) * 1e-3))} for name in types}
        result[label]["rank_positions_equal_between_types"] = round(same_pos, 4)
    line = json.dumps(result)
    print(line)
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
