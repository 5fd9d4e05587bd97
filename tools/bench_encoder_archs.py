#!/usr/bin/env python3
"""Timing of what the RoBERTa / XLM-R / MPNet support adds (profiles/encoder_archs.md), at DESIGN 4.8's corpus shape: 482 sequences of
129-136 tokens, 12 heads of 64.  Device events around every call, warm-up first, the variants of a part alternating inside one process;
every figure is the median of the timed calls with their min-max band.

  --part attention   ops.attention without and with a relative bias table (span 511, as the encoder passes it), packed, fp16 and bf16
  --part models      a random-init MPNet-base and RoBERTa-base forward over the same passages under fp16 autocast: FusedBertEncoder.forward
                     (packed) against the torch module
  --part plain       the plain ops.attention alone, one JSON line: run it in fresh processes on two checkouts (--pkg names the other
                     checkout's package directory) to compare their builds of the same kernel

  --part head32      the MiniLM-class shapes behind CCREC_FUSED_ENCODER_HEAD32=1 (profiles/encoder_head32.md): a random-init BertModel of
                     6 and of 12 layers x 384, 12 heads of 32, FFN 1536 over the same passages under fp16 autocast.  Per shape, alternating
                     in one process: FusedBertEncoder.forward (packed), the torch module, and the attention call alone at head width 32
                     against the 64-wide call on the same tokens and head count

A GPU is required; nothing here falls back."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L_LO, L_HI, HEADS = 482, 129, 136, 12


def timed_alternating(variants, warmup, reps):
    """variants: {name: callable}.  -> {name: [ms per call]}: reps rounds, every round runs each variant once (in turn) between events."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        marks = []
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in marks:
            times[name].append(e0.elapsed_time(e1))
    return times


def band(ms, per_ms=1e3, digits=1):
    """Median and min-max band of a list of milliseconds, in units of 1 / per_ms ms (default: microseconds)."""
    return {"median": round(statistics.median(ms) * per_ms, digits), "min": round(min(ms) * per_ms, digits),
            "max": round(max(ms) * per_ms, digits), "n": len(ms)}


def corpus_lengths():
    g = torch.Generator().manual_seed(0)
    return torch.randint(L_LO, L_HI + 1, (B,), generator=g, dtype=torch.int32)


def attention_inputs(half):
    lens = corpus_lengths()
    torch.manual_seed(0)
    start = (torch.cumsum(lens, 0, dtype=torch.int32) - lens).cuda()
    T = int(lens.sum())
    qkv = torch.randn(T, 3 * HEADS * 64, device="cuda").to(half)
    out = torch.empty(T, HEADS * 64, dtype=half, device="cuda")
    return qkv, start, lens.cuda(), out, T


def part_attention(ops, args):
    for half in (torch.float16, torch.bfloat16):
        qkv, start, lens, out, T = attention_inputs(half)
        table = torch.randn(HEADS, 1023, device="cuda")
        variants = {"plain": lambda: ops.attention(qkv, start, lens, HEADS, max_len=L_HI, out=out),
                    "biased": lambda: ops.attention(qkv, start, lens, HEADS, max_len=L_HI, out=out, rel_bias=table, rel_span=511)}
        times = timed_alternating(variants, args.warmup, args.reps)
        print(json.dumps({"part": "attention", "dtype": str(half)[6:], "tokens": T, "unit": "us", **{k: band(v) for k, v in times.items()}}),
              flush=True)


def part_plain(ops, args):
    qkv, start, lens, out, T = attention_inputs(torch.float16)
    times = timed_alternating({"plain": lambda: ops.attention(qkv, start, lens, HEADS, max_len=L_HI, out=out)}, args.warmup, args.reps)
    print(json.dumps({"part": "plain", "pkg": args.pkg or "this tree", "version": int(ops.require_gpu().ccr_version()), "unit": "us",
                      **band(times["plain"])}), flush=True)


def part_models(ops, args):
    import transformers
    from ccrec_amd import fused_bert
    lens = corpus_lengths()
    g = torch.Generator().manual_seed(1)
    ids = torch.full((B, L_HI), 1, dtype=torch.int64)
    mask = torch.zeros(B, L_HI, dtype=torch.int64)
    for r, n in enumerate(lens.tolist()):
        ids[r, :n] = torch.randint(2, 30000, (n,), generator=g)
        mask[r, :n] = 1
    ids, mask, lens_dev = ids.cuda(), mask.cuda(), lens.cuda()
    for name, cfg_cls, cls in (("mpnet-base", transformers.MPNetConfig, transformers.MPNetModel),
                               ("roberta-base", transformers.RobertaConfig, transformers.RobertaModel)):
        torch.manual_seed(0)
        model = cls(cfg_cls(vocab_size=30527, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                            max_position_embeddings=514, pad_token_id=1)).cuda().eval()
        enc = fused_bert.for_model(model)
        assert enc is not None, fused_bert.unsupported_reason(model)
        enc.refresh(torch.float16)

        def kernels():
            return enc.forward(ids, lens_dev, packed=True, lengths_host=lens, dtype=torch.float16)

        def module():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return model(input_ids=ids, attention_mask=mask).last_hidden_state

        times = timed_alternating({"kernels": kernels, "module": module}, args.warmup, args.reps)
        live = mask.bool()
        diff = (kernels()[live] - module().float()[live]).abs().max().item()
        print(json.dumps({"part": "models", "model": name, "passages": B, "tokens": int(lens.sum()), "max_abs_diff": round(diff, 5), "unit": "ms",
                          **{k: band(v, 1.0, 2) for k, v in times.items()}}), flush=True)


def part_head32(ops, args):
    import transformers
    from ccrec_amd import fused_bert
    os.environ["CCREC_FUSED_ENCODER_HEAD32"] = "1"      # (read at call time)
    lens = corpus_lengths()
    g = torch.Generator().manual_seed(1)
    ids = torch.zeros(B, L_HI, dtype=torch.int64)
    mask = torch.zeros(B, L_HI, dtype=torch.int64)
    for r, n in enumerate(lens.tolist()):
        ids[r, :n] = torch.randint(2, 30000, (n,), generator=g)
        mask[r, :n] = 1
    ids, mask, lens_dev = ids.cuda(), mask.cuda(), lens.cuda()
    start = (torch.cumsum(lens, 0, dtype=torch.int32) - lens).cuda()
    T = int(lens.sum())
    torch.manual_seed(0)
    qkv32 = torch.randn(T, 3 * HEADS * 32, device="cuda").to(torch.float16)
    qkv64 = torch.randn(T, 3 * HEADS * 64, device="cuda").to(torch.float16)
    out32 = torch.empty(T, HEADS * 32, dtype=torch.float16, device="cuda")
    out64 = torch.empty(T, HEADS * 64, dtype=torch.float16, device="cuda")
    for name, layers in (("MiniLM-L6", 6), ("MiniLM-L12", 12)):
        torch.manual_seed(0)
        model = transformers.BertModel(transformers.BertConfig(vocab_size=30522, hidden_size=384, num_hidden_layers=layers, num_attention_heads=HEADS,
                                                               intermediate_size=1536, max_position_embeddings=512)).cuda().eval()
        enc = fused_bert.for_model(model)
        assert enc is not None, fused_bert.unsupported_reason(model)
        enc.refresh(torch.float16)

        def kernels():
            return enc.forward(ids, lens_dev, packed=True, lengths_host=lens, dtype=torch.float16)

        def module():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return model(input_ids=ids, attention_mask=mask).last_hidden_state

        variants = {"kernels": kernels, "module": module,
                    "attention32": lambda: ops.attention(qkv32, start, lens_dev, HEADS, max_len=L_HI, scale=32 ** -0.5, out=out32, head_width=32),
                    "attention64": lambda: ops.attention(qkv64, start, lens_dev, HEADS, max_len=L_HI, out=out64)}
        times = timed_alternating(variants, args.warmup, args.reps)
        live = mask.bool()
        diff = (kernels()[live] - module().float()[live]).abs().max().item()
        print(json.dumps({"part": "head32", "model": name, "passages": B, "tokens": T, "max_abs_diff": round(diff, 5), "unit": "ms",
                          **{k: band(v, 1.0, 3) for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["attention", "models", "plain", "head32"], required=True)
    ap.add_argument("--pkg", default=None, help="package directory of another checkout (the directory that holds ccrec_amd/)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    pkg = os.path.abspath(args.pkg) if args.pkg else os.path.join(ROOT, "crowd-coachable-recommendations_amd")
    sys.path[:0] = [pkg]
    from ccrec_amd import ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__))) == pkg, ops.__file__
    assert torch.cuda.is_available(), "a GPU is required"
    {"attention": part_attention, "models": part_models, "plain": part_plain, "head32": part_head32}[args.part](ops, args)


if __name__ == "__main__":
    main()
