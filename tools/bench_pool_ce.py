#!/usr/bin/env python3
"""Pool contrastive loss: forward + backward time of ccrec_amd.ops.pool_ce (ccr_pool_ce_*) next to the torch formulation a user
runs in its place (mm, scale, cross_entropy, autograd), in fp32 as the reference runs it and under bf16 autocast, on the same
operands in one process.  The candidates are ALTERNATED round by round (device events around each call, after a warm-up of
every shape); the interquartile range of the torch fp32 rounds is the margin below which a difference is a tie.  Shapes (width 768):
(1024, 8192) seven negatives on one rank, (1024, 16384) eight ranks' pool, (1024, 2048) and (30, 150) beside the square
kernel (its shape; host-bound).  One JSON document (stdout, and --out).  Kernel times come from a separate run of this script
with --only ours under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]

SHAPES = [(1024, 8192, 768), (1024, 16384, 768), (1024, 2048, 768), (30, 150, 768)]
INV_T = 20.0


def candidates(n_q, n_c, dim):
    from ccrec_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n_c)
    q = torch.randn(n_q, dim, device="cuda", generator=g) * dim ** -0.5
    c = torch.randn(n_c, dim, device="cuda", generator=g) * dim ** -0.5
    labels = torch.arange(n_q, device="cuda", dtype=torch.int32) % n_c
    labels64 = labels.long()

    def ours():
        a, b = q.clone().requires_grad_(True), c.clone().requires_grad_(True)
        loss = ops.pool_ce(a, b, labels, INV_T)
        loss.backward()
        return loss

    def ref(dtype):
        a, b = q.clone().requires_grad_(True), c.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            scores = (a @ b.T) * INV_T
            loss = torch.nn.functional.cross_entropy(scores.float(), labels64)
        loss.backward()
        return loss

    fns = {"ccr_pool_ce": ours, "torch_fp32": lambda: ref(torch.float32), "torch_bf16_autocast": lambda: ref(torch.bfloat16)}
    if n_c == 2 * n_q:   # the square kernel's shape: C = [P ; N], labels arange(B)
        def square():
            a, p, n = q.clone().requires_grad_(True), c[:n_q].clone().requires_grad_(True), c[n_q:].clone().requires_grad_(True)
            loss = ops.inbatch_ce(a, p, n, INV_T)
            loss.backward()
            return loss
        fns["ccr_inbatch_ce"] = square
    return fns


def measure(fns, rounds, inner):
    """rounds x (every candidate once, `inner` calls between two device events): ms per call, per round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                loss = fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / inner)
    return times, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default=None, help="ours: time ccr_pool_ce alone (the run to profile)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pool_ce.py needs the GPU"
    doc = {"inv_temperature": INV_T, "rounds": args.rounds, "calls_per_round": args.inner, "unit": "ms per forward + backward", "shapes": []}
    for n_q, n_c, dim in SHAPES:
        fns = candidates(n_q, n_c, dim)
        if args.only == "ours":
            fns = {"ccr_pool_ce": fns["ccr_pool_ce"]}
        times, _ = measure(fns, args.rounds, args.inner)
        row = {"n_q": n_q, "n_c": n_c, "dim": dim, "flops_fwd_bwd": 3 * 2 * n_q * n_c * dim}
        for name, t in times.items():
            row[name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        if "torch_fp32" in times:
            t = times["torch_fp32"]
            # repeated measurements of the same thing.  The tie margin is the interquartile range of the rounds (one slow round,
            # another tenant's burst, does not widen it); the full range is recorded beside it.
            qs = statistics.quantiles(t, n=4)
            row["torch_fp32_spread_ms"] = round(qs[2] - qs[0], 4)
            row["torch_fp32_range_ms"] = round(max(t) - min(t), 4)
            diff = statistics.median(times["ccr_pool_ce"]) - statistics.median(t)
            row["ccr_minus_torch_fp32_ms"] = round(diff, 4)
            row["verdict_vs_torch_fp32"] = "faster" if diff < -row["torch_fp32_spread_ms"] else ("tie" if diff <= row["torch_fp32_spread_ms"] else "slower")
        doc["shapes"].append(row)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
