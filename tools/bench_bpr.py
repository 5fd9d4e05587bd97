#!/usr/bin/env python3
"""The bpr objective with a frozen tower: time of one step -- negative sampling + loss forward + backward -- of
ccrec_amd.BprStep (ccr_bpr_sample, ccr_bpr_frozen_*) next to the torch fp32 formulation of the same reference lines
(src/ccrec/models/bbpr.py:153-185: index_select().to_dense(), softmax, multinomial, gather, LayerNorm, products, logsigmoid,
autograd) on the same GPU, the same cached rows and the same prior, in one process.  The candidates are ALTERNATED round by
round (device events around each call, after a warm-up of every shape); the interquartile range of the torch rounds is the
margin below which a difference is a tie.  Shapes: the reference's frozen default (B = 10 000, 10 negatives, width 768, the
10 812 items of Prime-Pantry, about 4 prior entries per user) and B = 1 024.  The sampling halves are timed on their own too.
One JSON document (stdout, and --out).  Kernel times come from a separate run of this script with --only ours under
`rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]

# (B, n_negatives, dim, n_items, n_users, prior entries per user)
SHAPES = [(10000, 10, 768, 10812, 20000, 4), (1024, 10, 768, 10812, 20000, 4)]


def candidates(B, n_neg, dim, n_items, n_users, per_user):
    from ccrec_amd import BprStep, item_proposal
    g = torch.Generator().manual_seed(B)
    all_cls = torch.randn(n_items, dim, generator=g).cuda()
    item_freq = torch.randint(0, 200, (n_items,), generator=g)
    idx = torch.stack([torch.arange(n_users).repeat_interleave(per_user), torch.randint(0, n_items, (n_users * per_user,), generator=g)])
    prior = torch.sparse_coo_tensor(idx, torch.rand(n_users * per_user, generator=g) * 5, (n_users, n_items)).coalesce()
    i_to_ptr = torch.randint(0, n_items, (n_users,), generator=g)     # a user's row of the table: the item the session ends with
    j_to_ptr = torch.arange(n_items)
    batch = torch.stack([torch.randint(0, n_users, (B,), generator=g).float(), torch.randint(0, n_items, (B,), generator=g).float(),
                         torch.rand(B, generator=g) + 0.1], 1).cuda()
    ln_ours, ln_ref = torch.nn.LayerNorm(dim).cuda(), torch.nn.LayerNorm(dim).cuda()
    step = BprStep(None, i_to_ptr, j_to_ptr, item_freq.numpy(), tr_prior_score=prior, n_negatives=n_neg, all_cls=all_cls, layer_norm=ln_ours)
    prior_dev, i_dev, j_dev = prior.cuda(), i_to_ptr.cuda(), j_to_ptr.cuda()
    proposal = item_proposal(item_freq.numpy()).float().cuda()

    def ours():
        ln_ours.zero_grad(set_to_none=True)
        loss = step(batch)
        loss.backward()
        return loss

    def ours_sample():
        return step.sample_negatives(batch[:, 0].to(int), n_neg)

    def ref_sample(i):
        prior_score = prior_dev.index_select(0, i).to_dense()
        return torch.multinomial((prior_score + proposal.log()).softmax(1), n_neg, True).T

    def ref():
        ln_ref.zero_grad(set_to_none=True)
        i, j, w = batch.T
        i, j = i.to(int), j.to(int)
        pairwise = lambda a, b: (ln_ref(all_cls[i_dev[a.ravel()]]).reshape([*a.shape, -1]) * ln_ref(all_cls[j_dev[b.ravel()]]).reshape([*b.shape, -1])).sum(-1)
        pos_score = pairwise(i, j)
        with torch.no_grad():
            nj = ref_sample(i)
        loglik = torch.nn.functional.logsigmoid(pos_score - pairwise(i, nj))
        loss = (-loglik * w).sum() / (n_neg * w.sum())
        loss.backward()
        return loss

    return {"ccr_bpr_step": ours, "torch_fp32_step": ref, "ccr_bpr_sample": ours_sample, "torch_fp32_sample": lambda: ref_sample(batch[:, 0].to(int))}


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
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / inner)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default=None, help="ours: time ccr_bpr_step alone (the run to profile)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bpr.py needs the GPU"
    doc = {"rounds": args.rounds, "calls_per_round": args.inner, "unit": "ms per call (step = sampling + forward + backward)", "shapes": []}
    for B, n_neg, dim, n_items, n_users, per_user in SHAPES:
        fns = candidates(B, n_neg, dim, n_items, n_users, per_user)
        if args.only == "ours":
            fns = {"ccr_bpr_step": fns["ccr_bpr_step"]}
        times = measure(fns, args.rounds, args.inner)
        row = {"B": B, "n_negatives": n_neg, "dim": dim, "n_items": n_items, "n_users": n_users, "prior_entries_per_user": per_user,
               "gathered_bytes_per_pass": (2 + n_neg) * B * dim * 4, "dense_prior_bytes": B * n_items * 4}
        for name, t in times.items():
            row[name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
        if "torch_fp32_step" in times:
            t = times["torch_fp32_step"]
            # repeated measurements of the same thing.  The tie margin is the interquartile range of the rounds (one slow round,
            # another tenant's burst, does not widen it); the full range is recorded beside it.
            qs = statistics.quantiles(t, n=4)
            row["torch_fp32_spread_ms"] = round(qs[2] - qs[0], 4)
            row["torch_fp32_range_ms"] = round(max(t) - min(t), 4)
            diff = statistics.median(times["ccr_bpr_step"]) - statistics.median(t)
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
