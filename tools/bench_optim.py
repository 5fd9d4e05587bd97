#!/usr/bin/env python
"""The optimizer step of the fine-tune loop: optim.FusedAdamW (csrc/ccr_optim.hip) against torch.optim.AdamW, alone and inside the
whole step.

(a) step() alone on the real parameter lists of BERT-base and DistilBERT (models built from their default configs, random init, every
    parameter with a gradient): FusedAdamW without and with the maintained 16-bit weight set, torch.optim.AdamW default, foreach=True
    and fused=True.  ms per step and bytes/s, counting 28 B per parameter (p, g, exp_avg, exp_avg_sq read; p, exp_avg, exp_avg_sq written)
    plus 2 B per parameter that has a 16-bit copy.  Beside it: ccr_pack_bf16's rate on this device, measured as bench.py --full does
    (one corpus pack, 6 B per element).
(b) the whole fine-tune step -- three training forwards of 30 texts on the layer kernels, one backward, the optimizer step,
    zero_grad(set_to_none=True) -- at tools/bench_encoder_train.py's 90 x 128 ragged batch: torch.optim.AdamW + the per-forward casts
    (what ran before FusedAdamW), FusedAdamW + casts, FusedAdamW + the maintained weight set.

Timing: device events around each run, 5 warm-up rounds, the median of 20 rounds; the variants ALTERNATE inside every round, in one
process, so drift of the device hits them alike.  Writes <out>/optim_step.json and <out>/optim_step.md and prints the JSON.

    python tools/bench_optim.py [--out profiles] [--runs 20] [--warmup 5] [--dtype bf16]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd"), os.path.join(ROOT, "tools")]

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def alternate(variants, runs, warmup):
    """variants: {name: fn}.  Every round runs each fn once between two device events; -> {name: {median_ms, min_ms, max_ms, runs}}."""
    ms = {name: [] for name in variants}
    for r in range(warmup + runs):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "runs": runs}
            for name, v in ms.items()}


def build(kind, dropout=0.0):
    if kind == "bert-base":
        from transformers import BertConfig, BertModel
        return BertModel(BertConfig(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout))
    from transformers import DistilBertConfig, DistilBertModel
    return DistilBertModel(DistilBertConfig(dropout=dropout, attention_dropout=dropout))


def give_gradients(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3


def pack_rate(runs, warmup):
    """ccr_pack_bf16 over a 2 M x 768 fp32 corpus with its norm bounds, as bench.py --full times it: 6 B per element."""
    from ccrec_amd import ops
    rows, dim = 2_000_000, 768
    corpus = torch.randn(rows, dim, device="cuda")
    out = torch.empty(rows, dim, dtype=torch.bfloat16, device="cuda")
    bounds = torch.empty(rows, dtype=torch.float32, device="cuda")
    t = alternate({"pack": lambda: ops.pack_bf16(corpus, out=out, norm_bounds=bounds)}, runs, warmup)["pack"]
    t["gb_per_s"] = round(rows * dim * 6 / t["median_ms"] / 1e6, 1)
    return t


def bench_step_alone(kind, dtype, runs, warmup):
    from ccrec_amd import _lib, optim
    torch.manual_seed(0)
    shared, shadowed = build(kind).cuda(), build(kind).cuda()      # the shadow variant's weight set must see no other optimizer
    give_gradients(shared, 1)
    give_gradients(shadowed, 1)
    n = sum(p.numel() for p in shared.parameters())
    lr = 1e-6
    opts = {
        "FusedAdamW": optim.FusedAdamW(shared.parameters(), lr=lr),
        "FusedAdamW + 16-bit weight set": optim.FusedAdamW(shadowed.parameters(), lr=lr, shadow_for=shadowed, shadow_dtype=dtype),
        "torch AdamW (default)": torch.optim.AdamW(shared.parameters(), lr=lr),
        "torch AdamW foreach=True": torch.optim.AdamW(shared.parameters(), lr=lr, foreach=True),
        "torch AdamW fused=True": torch.optim.AdamW(shared.parameters(), lr=lr, fused=True),
    }
    n_shadow = sum(p.numel() for p in shadowed.parameters() if id(p) in opts["FusedAdamW + 16-bit weight set"]._shadow)
    t = alternate({name: o.step for name, o in opts.items()}, runs, warmup)
    # the device time of the library call alone: the segment list of the last step again, ten calls back to back between two events
    # (the host runs ahead of the device), per call
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    replay = {}
    for name in ("FusedAdamW", "FusedAdamW + 16-bit weight set"):
        seg, count = opts[name]._segments, opts[name]._n_segments

        def ten(seg=seg, count=count):
            for _ in range(10):
                _lib.check(lib.ccr_adamw_step(ctypes.c_void_p(seg.ctypes.data), count, 0.1, 0.999, 0.001, 1e-8, stream), "ccr_adamw_step")
        replay[name + ": ccr_adamw_step alone (device time per call)"] = ten
    for name, rec in alternate(replay, runs, warmup).items():
        t[name] = {k: (round(v / 10, 4) if k.endswith("_ms") else v) for k, v in rec.items()}
    for name, rec in t.items():
        nbytes = 28 * n + (2 * n_shadow if "weight set" in name else 0)
        rec["bytes"] = nbytes
        rec["gb_per_s"] = round(nbytes / rec["median_ms"] / 1e6, 1)
    return {"model": kind, "tensors": len(list(shared.parameters())), "parameters": n, "parameters_with_16_bit_copy": n_shadow, "variants": t}


def bench_whole_step(dtype, runs, warmup):
    """Three forwards of 30 texts + backward + optimizer + zero_grad on BERT-base (dropout 0, train())."""
    from bench_encoder_train import ragged_batch
    from ccrec_amd import fused_bert, optim
    from transformers import BertConfig, BertModel
    ids, mask, lengths = ragged_batch(90, 128, 0.4, seed=128 + 90)
    parts = [(ids[i:i + 30].contiguous(), lengths[i:i + 30].contiguous(), mask[i:i + 30].unsqueeze(-1).float()) for i in (0, 30, 60)]

    def variant(make_opt):
        torch.manual_seed(0)
        model = BertModel(BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False).cuda().train()
        enc = fused_bert.for_model(model)      # (the encoder whose weight set the optimizer adopts)
        opt = make_opt(model)

        def step():
            with torch.autocast("cuda", dtype=dtype):
                loss = sum((enc.forward_train(i, l, dtype=dtype) * w).sum() for i, l, w in parts)
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return step

    lr = 1e-6
    variants = {
        "torch AdamW + casts in every forward": variant(lambda m: torch.optim.AdamW(m.parameters(), lr=lr)),
        "FusedAdamW + casts in every forward": variant(lambda m: optim.FusedAdamW(m.parameters(), lr=lr)),
        "FusedAdamW + 16-bit weight set": variant(lambda m: optim.FusedAdamW(m.parameters(), lr=lr, shadow_for=m, shadow_dtype=dtype)),
    }
    t = alternate(variants, runs, warmup)
    return {"batch": "3 x (30 x 128 ragged)", "real_tokens": int(lengths.sum()), "model": "BERT-base (random init, dropout 0, no pooler)", "variants": t}


def to_markdown(result):
    lines = [f"# Optimizer step: FusedAdamW against torch.optim.AdamW ({result['device']})", "",
             f"`{result['tool']}`: device events, {result['warmup']} warm-up rounds, median of {result['runs']} rounds, the variants alternating in one "
             f"process.  16-bit type: {result['dtype']}.", "",
             f"`ccr_pack_bf16` on the same device in the same process (2 M x 768, 6 B per element, as `bench.py --full` times it): "
             f"**{result['pack']['gb_per_s']} GB/s** ({result['pack']['median_ms']} ms).", ""]
    for rec in result["step_alone"]:
        lines += [f"## step() alone: {rec['model']} ({rec['tensors']} tensors, {rec['parameters'] / 1e6:.1f} M parameters, "
                  f"{rec['parameters_with_16_bit_copy'] / 1e6:.1f} M with a 16-bit copy)", "",
                  "| variant | median ms | min | max | GB/s (28 B, +2 B per copied parameter) | of the pack rate |", "|---|---|---|---|---|---|"]
        for name, t in rec["variants"].items():
            lines.append(f"| {name} | {t['median_ms']} | {t['min_ms']} | {t['max_ms']} | {t['gb_per_s']} | {t['gb_per_s'] / result['pack']['gb_per_s']:.2f} |")
        lines.append("")
    w = result["whole_step"]
    lines += [f"## the whole fine-tune step: {w['batch']}, {w['real_tokens']} real tokens, {w['model']}", "",
              "three training forwards on the layer kernels, one backward, the optimizer step, zero_grad(set_to_none=True)", "",
              "| variant | median ms | min | max |", "|---|---|---|---|"]
    for name, t in w["variants"].items():
        lines.append(f"| {name} | {t['median_ms']} | {t['min_ms']} | {t['max_ms']} |")
    lines.append("")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    args = ap.parse_args(argv)
    assert args.runs >= 20, "a median of at least 20 runs"
    from ccrec_amd import ops
    ops.require_gpu()
    os.environ["CCREC_FUSED_ENCODER_TRAIN"] = "1"
    dtype = DTYPES[args.dtype]
    result = {"tool": "tools/bench_optim.py", "device": torch.cuda.get_device_name(0), "dtype": args.dtype, "runs": args.runs, "warmup": args.warmup}
    result["pack"] = pack_rate(args.runs, args.warmup)
    print(json.dumps(result["pack"]), flush=True)
    torch.cuda.empty_cache()
    result["step_alone"] = []
    for kind in ("bert-base", "distilbert"):
        result["step_alone"].append(bench_step_alone(kind, dtype, args.runs, args.warmup))
        print(json.dumps(result["step_alone"][-1]), flush=True)
        torch.cuda.empty_cache()
    result["whole_step"] = bench_whole_step(dtype, args.runs, args.warmup)
    print(json.dumps(result["whole_step"]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "optim_step.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "optim_step.md"), "w") as f:
        f.write(to_markdown(result))


if __name__ == "__main__":
    main()
