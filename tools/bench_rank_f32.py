#!/usr/bin/env python3
"""Same-process A/B of the plain k = 100 search on a bf16 index and the fp32-exact search on top of it (ops.ExactF32Index), alternating
the two round by round, at the NQ shape (2 681 468 x 768, 3 452 queries: the 256 x 384 main pass) and with the streaming pass of a
64-query batch over the same rows.  One seeded fp32 stream is packed (ops.pack_half) and kept (ops.keep_f32) chunk by chunk, both
timed; every shape is warmed up on both variants before the timed rounds; a timed call sits between two device events.  The exact
search's three parts are timed on their own as well: the wider 16-bit search (2 k + 32 rows), the re-score kernel, the keep pass at
index build.  Recorded beside the times: the rung statistics of the exact search, and the rank positions that the plain and the exact
search share with the fp32 ranking of 16 sampled queries computed on the CPU (rank_f32_ref).  Prints one JSON line and, with an output
path, writes it there too.

  python3 tools/bench_rank_f32.py [out.json] [--rows N --queries Q --dim D --k K --rounds R --warmup W --check C]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]


def arg(name, dflt):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn):
    """(result, device ms) of fn() between two events on the current stream."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    import numpy as np
    import torch
    from ccrec_amd import index_ref, ops, rank_f32_ref
    n, nq, d, k = arg("--rows", 2681468), arg("--queries", 3452), arg("--dim", 768), arg("--k", 100)
    rounds, warmup, small, n_check = arg("--rounds", 20), arg("--warmup", 3), 64, arg("--check", 16)
    chunk = 1 << 19
    g = torch.Generator(device="cuda").manual_seed(1234)
    shard = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    kept = torch.empty(n, d, dtype=torch.float32, device="cuda")
    bounds, res = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    pack_ms, keep_ms = [], []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        x = torch.randn(hi - lo, d, generator=g, device="cuda") / d ** 0.5
        _, t_pack = timed(lambda: ops.pack_half(x, torch.bfloat16, out=shard[lo:hi], norm_bounds=bounds[lo:hi]))
        _, t_keep = timed(lambda: ops.keep_f32(x, shard[lo:hi], out=kept[lo:hi], res_bounds=res[lo:hi]))
        if hi - lo == chunk and lo:             # whole chunks, the first (cold) one left out
            pack_ms.append(t_pack)
            keep_ms.append(t_keep)
    q32 = torch.randn(nq, d, generator=torch.Generator(device="cuda").manual_seed(4321), device="cuda") / d ** 0.5
    hq = ops.pack_half(q32, torch.bfloat16)
    exact = ops.ExactF32Index(shard, kept, bounds, res)
    plain = exact.index
    n1 = min(n, exact.max_candidates, 2 * k + 32)
    result = {"rows": n, "dim": d, "k": k, "first_rung": n1, "rounds": rounds, "warmup": warmup, "device": torch.cuda.get_device_name(0),
              "build_ms_per_%d_rows" % chunk: {"pack": spread(pack_ms), "keep_f32": spread(keep_ms)} if pack_ms else None}
    for label, m in (("nq%d" % nq, nq), ("nq%d" % small, small)):
        ms = {name: [] for name in ("plain", "exact", "wider_search", "rescore")}
        stats, last = None, {}
        for it in range(warmup + rounds):
            for name in (("plain", "exact") if it % 2 == 0 else ("exact", "plain")):        # alternate, and alternate who goes first
                if name == "plain":
                    (s, i), t = timed(lambda: plain.search(hq[:m], k))
                else:
                    (s, i), t = timed(lambda: exact.search(q32[:m], k))
                    stats = exact.last_stats()
                if it >= warmup:
                    ms[name].append(t)
                last[name] = i
            # the exact search's parts on their own: the wider 16-bit search, then the re-score of its lists
            (s16, i16), t_wide = timed(lambda: plain.search(hq[:m], n1))
            nbq = torch.empty(m, device="cuda")
            hm = ops.pack_half(q32[:m], torch.bfloat16, norm_bounds=nbq)
            ym, rm = ops.keep_f32(q32[:m], hm)
            A = torch.nextafter(nbq + rm, torch.full_like(nbq, float("inf")))
            out, t_resc = timed(lambda: ops.rescore_f32(ym, kept, i16, s16, k, A, rm, exact.corpus_max))
            if it >= warmup:
                ms["wider_search"].append(t_wide)
                ms["rescore"].append(t_resc)
        diag = out[3].double()
        room = (diag[:, 0] - (diag[:, 1] + diag[:, 2] + diag[:, 3]))                          # tau - (cut + E + slack): > 0 = verified
        extra = [e - p for e, p in zip(ms["exact"], ms["plain"])]
        result[label] = {name: spread(v) for name, v in ms.items()}
        result[label]["exact_minus_plain_ms"] = spread(extra)
        result[label]["exact_over_plain"] = round(statistics.median(ms["exact"]) / statistics.median(ms["plain"]), 4)
        result[label]["rungs"] = stats
        result[label]["first_rung_margin"] = {"min": float(room.min()), "median": float(room.median()), "unverified": int((room <= 0).sum())}
        result[label]["rank_positions_equal_plain_vs_exact"] = round(float((last["plain"] == last["exact"]).float().mean()), 4)
        if label.startswith("nq%d" % nq) and n_check:
            # fidelity: the fp32 ranking of a few queries on the CPU (no normalisation: the kept rows are the embeddings)
            pick = np.linspace(0, m - 1, min(n_check, m)).astype(np.int64)
            qn = q32[pick].cpu().numpy()
            cols = [rank_f32_ref.scores(qn, kept[lo:lo + (1 << 18)].cpu().numpy()) for lo in range(0, n, 1 << 18)]   # 0.8 GB of rows at a time
            ref_i, _ = index_ref.rank(np.concatenate(cols, 1), k)
            result["fidelity"] = {"queries": int(pick.size), "positions": int(pick.size * k),
                                  "plain_bf16_equal": int((last["plain"][pick].cpu().numpy() == ref_i).sum()),
                                  "exact_f32_equal": int((last["exact"][pick].cpu().numpy() == ref_i).sum())}
    line = json.dumps(result)
    print(line)
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
