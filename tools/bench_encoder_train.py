#!/usr/bin/env python
"""Forward + backward of a BERT-base encoder on training batches shaped like the reference's fine-tune step: the layer kernels'
training path (FusedBertEncoder.forward_train: packed tokens, ccr_attention_fwd_train_half / ccr_*_bwd_half) against the torch
module under the same autocast, plus every new kernel on its own.

The reference's step encodes 30 x 3 texts with padding="max_length" (src/ccrec/models/bbpr.py:360, bert_mt.py:243); real texts fill
about 40 % of it.  Shapes: 90 x 128, 90 x 256 (ragged, mean real length ~ 40 %), and a 16 K-token batch without padding (128 x 128).
The module path is code this tool does not change (transformers' BertModel under torch.autocast), so its time here is its time at any
commit of this repository.

Timing: warm-up runs, then HIP events around each of >= 20 runs, median (and min / max).  Writes <out>/encoder_train_bench.json and
<out>/encoder_train_kernel_stats.csv and prints the JSON.

    python tools/bench_encoder_train.py [--out profiles] [--runs 20] [--warmup 5] [--dtypes bf16,fp16]

--dropout P (0.1: the checkpoints' own): the model is built with dropout P and stays in train(); three columns per shape -- the module
with dropout under autocast, the kernels with dropout from keep bits (CCREC_FUSED_ENCODER_TRAIN_DROPOUT=1), and the kernels with every
Dropout module's p set to 0 (the dropout-free instantiations, measured twice: the distance between the two is the run-to-run spread) --
plus the generator's time per layer and every kernel with and without bits.  Writes <out>/encoder_train_dropout_bench.json and
<out>/encoder_train_dropout_kernel_stats.csv instead.

--ab-tree DIR (with --dropout): DIR is a checkout of the PARENT commit with its library built.  Before anything else runs here, the
dropout-free step is timed by DIR's own copy of this tool and by this tree's, in fresh child processes, parent / this / parent / this; the
medians of all four runs, the difference of the two trees and the run-to-run spread of each go into the JSON ("dropout_off_ab")."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def timed(fn, runs, warmup):
    """-> {median, min, max} ms over `runs` runs of fn(), HIP events around each, after `warmup` untimed runs."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": runs}


def ragged_batch(n, L, fill, seed):
    """n right-padded rows of L tokens; real lengths uniform in [fill / 4, 7 fill / 4] x L (mean fill x L); fill 1.0 = no padding."""
    g = torch.Generator().manual_seed(seed)
    if fill >= 1.0:
        lens = torch.full((n,), L, dtype=torch.int64)
    else:
        lens = torch.randint(max(1, int(L * fill / 4)), int(L * fill * 7 / 4) + 1, (n,), generator=g)
    ids = torch.zeros(n, L, dtype=torch.int64)
    mask = torch.zeros(n, L, dtype=torch.int64)
    for r, ln in enumerate(lens.tolist()):
        ids[r, :ln] = torch.randint(1000, 30000, (ln,), generator=g)
        mask[r, :ln] = 1
    return ids.cuda(), mask.cuda(), lens.to(torch.int32).cuda()


def bench_step(model, enc, ids, mask, lengths, dtype, runs, warmup):
    w = mask.unsqueeze(-1).float()

    def module_step():
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            h = model(input_ids=ids, attention_mask=mask).last_hidden_state
        (h.float() * w).sum().backward()

    def kernel_step():
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            h = enc.forward_train(ids, lengths, dtype=dtype)
        (h * w).sum().backward()

    out = {"module": timed(module_step, runs, warmup), "kernels": timed(kernel_step, runs, warmup)}
    out["speedup"] = round(out["module"]["median_ms"] / out["kernels"]["median_ms"], 3)
    return out


def bench_step_dropout(model, enc, ids, mask, lengths, dtype, runs, warmup):
    """module with dropout | kernels with dropout | kernels with dropout off (twice: run-to-run spread) on a train() model."""
    w = mask.unsqueeze(-1).float()
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    ps = [m.p for m in drops]

    def module_step():
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            h = model(input_ids=ids, attention_mask=mask).last_hidden_state
        (h.float() * w).sum().backward()

    def kernel_step():
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype):
            h = enc.forward_train(ids, lengths, dtype=dtype)
        (h * w).sum().backward()

    out = {"module_dropout": timed(module_step, runs, warmup), "kernels_dropout": timed(kernel_step, runs, warmup)}
    for m in drops:
        m.p = 0.0
    try:
        out["kernels_dropout_off"] = timed(kernel_step, runs, warmup)
        out["kernels_dropout_off_again"] = timed(kernel_step, runs, warmup)
    finally:
        for m, p in zip(drops, ps):
            m.p = p
    out["speedup_with_dropout"] = round(out["module_dropout"]["median_ms"] / out["kernels_dropout"]["median_ms"], 3)
    out["dropout_cost_ms"] = round(out["kernels_dropout"]["median_ms"] - out["kernels_dropout_off"]["median_ms"], 4)
    out["dropout_off_spread_ms"] = round(abs(out["kernels_dropout_off"]["median_ms"] - out["kernels_dropout_off_again"]["median_ms"]), 4)
    return out


def bench_kernels_dropout(dtype, p, runs, warmup, rows):
    """The generator per layer and every layer kernel with and without bits, on bench_kernels' shapes."""
    from ccrec_amd import dropout_ref, ops
    n_seq, L, H, hidden = 128, 128, 12, 768
    T = n_seq * L
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(T, 3 * hidden, device="cuda", generator=g).to(dtype)
    d_out = torch.randn(T, hidden, device="cuda", generator=g).to(dtype)
    seq_len = torch.full((n_seq,), L, dtype=torch.int32, device="cuda")
    seq_start = torch.arange(n_seq, dtype=torch.int32, device="cuda") * L
    x = torch.randn(T, hidden, device="cuda", generator=g).to(dtype)
    res = torch.randn(T, hidden, device="cuda", generator=g)
    gamma, beta = torch.ones(hidden, device="cuda"), torch.zeros(hidden, device="cuda")
    d_y = torch.randn(T, hidden, device="cuda", generator=g)
    inv = dropout_ref.inv_keep(p)
    keep_q, keep_k = ops.dropout_bits_attention(seq_start, seq_len, T, H, L, 1, 1, p)
    bits = ops.dropout_bits_rows(T, hidden, 1, 2, p)
    out, lse = ops.attention_fwd_train(qkv, seq_start, seq_len, H, L)
    out_d, lse_d = ops.attention_fwd_train(qkv, seq_start, seq_len, H, L, keep_q=keep_q, inv_keep=inv)
    cases = [
        ("ccr_dropout_bits_attention", lambda: ops.dropout_bits_attention(seq_start, seq_len, T, H, L, 1, 1, p)),
        ("ccr_dropout_bits_rows", lambda: ops.dropout_bits_rows(T, hidden, 1, 2, p)),
        ("ccr_attention_fwd_train_half", lambda: ops.attention_fwd_train(qkv, seq_start, seq_len, H, L)),
        ("ccr_attention_fwd_train_drop_half", lambda: ops.attention_fwd_train(qkv, seq_start, seq_len, H, L, keep_q=keep_q, inv_keep=inv)),
        ("ccr_attention_bwd_half", lambda: ops.attention_bwd(qkv, out, lse, d_out, seq_start, seq_len, H, L)),
        ("ccr_attention_bwd_drop_half", lambda: ops.attention_bwd(qkv, out_d, lse_d, d_out, seq_start, seq_len, H, L, keep_q=keep_q, keep_k=keep_k, inv_keep=inv)),
        ("ccr_add_layernorm_half", lambda: ops.add_layernorm(x, res, gamma, beta, 1e-12)),
        ("ccr_add_layernorm_drop_half", lambda: ops.add_layernorm(x, res, gamma, beta, 1e-12, keep_bits=bits, inv_keep=inv)),
        ("ccr_add_layernorm_bwd_half", lambda: ops.add_layernorm_bwd(x, res, gamma, 1e-12, d_y)),
        ("ccr_add_layernorm_bwd_drop_half", lambda: ops.add_layernorm_bwd(x, res, gamma, 1e-12, d_y, keep_bits=bits, inv_keep=inv)),
        ("ccr_dropout_apply", lambda: ops.dropout_apply(res, bits, inv, dtype)),
    ]
    for name, fn in cases:
        rows.append({"kernel": name, "dtype": str(dtype)[6:], "shape": f"{n_seq}x{L} tokens, {H} heads", **timed(fn, runs, warmup), "tflops": "",
                     "gb_per_s": ""})


def dropout_off_ab(args):
    """The dropout-free kernels column of the plain mode at the parent (args.ab_tree) and at this tree, two rounds each, one child process per run."""
    import subprocess
    import tempfile
    runs = {"parent": [], "this": []}
    for _ in range(2):
        for which, tree in (("parent", os.path.abspath(args.ab_tree)), ("this", ROOT)):
            with tempfile.TemporaryDirectory() as tmp:
                subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_encoder_train.py"), "--out", tmp, "--runs", str(args.runs), "--warmup",
                                str(args.warmup), "--dtypes", args.dtypes], check=True, cwd=tree, stdout=subprocess.DEVNULL, timeout=600)
                with open(os.path.join(tmp, "encoder_train_bench.json")) as f:
                    runs[which].append({(r["batch"], r["dtype"]): r["kernels"]["median_ms"] for r in json.load(f)["steps"]})
    out = []
    for key in runs["this"][0]:
        parent, this = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        out.append({"batch": key[0], "dtype": key[1], "parent_ms": parent, "this_ms": this,
                    "difference_ms": round(sum(this) / 2 - sum(parent) / 2, 4),
                    "run_to_run_spread_ms": round(max(abs(parent[0] - parent[1]), abs(this[0] - this[1])), 4)})
    return out


def main_dropout(args):
    ab = dropout_off_ab(args) if args.ab_tree else None
    from transformers import BertConfig, BertModel
    from ccrec_amd import ops
    from ccrec_amd.fused_bert import FusedBertEncoder
    ops.require_gpu()
    os.environ["CCREC_FUSED_ENCODER_TRAIN"] = os.environ["CCREC_FUSED_ENCODER_TRAIN_DROPOUT"] = "1"
    torch.manual_seed(0)
    p = args.dropout
    model = BertModel(BertConfig(hidden_dropout_prob=p, attention_probs_dropout_prob=p), add_pooling_layer=False).cuda().train()
    enc = FusedBertEncoder(model)
    shapes = [("90x128 ragged", 90, 128, 0.4), ("90x256 ragged", 90, 256, 0.4), ("128x128 full (16K tokens)", 128, 128, 1.0)]
    result = {"tool": "tools/bench_encoder_train.py --dropout", "device": torch.cuda.get_device_name(0),
              "model": f"BERT-base (random init, dropout {p}, train())", "what": "forward + backward of the encoder, ms per step (median)",
              "steps": [], "kernels": []}
    if ab is not None:
        result["dropout_off_ab"] = ab
        print(json.dumps(ab), flush=True)
    for name in args.dtypes.split(","):
        dtype = DTYPES[name]
        for label, n, L, fill in shapes:
            ids, mask, lengths = ragged_batch(n, L, fill, seed=L + n)
            rec = {"batch": label, "dtype": name, "real_tokens": int(lengths.sum()), "padded_tokens": n * L}
            rec.update(bench_step_dropout(model, enc, ids, mask, lengths, dtype, args.runs, args.warmup))
            result["steps"].append(rec)
            print(json.dumps(rec), flush=True)
        bench_kernels_dropout(dtype, p, args.runs, args.warmup, result["kernels"])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "encoder_train_dropout_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    cols = ["kernel", "dtype", "shape", "median_ms", "min_ms", "max_ms", "runs"]
    with open(os.path.join(args.out, "encoder_train_dropout_kernel_stats.csv"), "w") as f:
        f.write(",".join(cols) + "\n")
        for r in result["kernels"]:
            f.write(",".join(f'"{r[c]}"' if isinstance(r[c], str) and "," in r[c] else str(r[c]) for c in cols) + "\n")
    print(json.dumps(result["kernels"]))


def bench_kernels(dtype, runs, warmup, rows):
    """Each new kernel alone on the 16 K-token packed batch's shapes (128 sequences x 128 tokens, 12 heads, hidden 768, FFN 3072)."""
    from ccrec_amd import ops
    n_seq, L, H, hidden, inter = 128, 128, 12, 768, 3072
    T = n_seq * L
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn(T, 3 * hidden, device="cuda", generator=g).to(dtype)
    d_out = torch.randn(T, hidden, device="cuda", generator=g).to(dtype)
    seq_len = torch.full((n_seq,), L, dtype=torch.int32, device="cuda")
    seq_start = torch.arange(n_seq, dtype=torch.int32, device="cuda") * L
    out, lse = ops.attention_fwd_train(qkv, seq_start, seq_len, H, L)
    x = torch.randn(T, hidden, device="cuda", generator=g).to(dtype)
    res = torch.randn(T, hidden, device="cuda", generator=g)
    gamma = torch.ones(hidden, device="cuda")
    d_y = torch.randn(T, hidden, device="cuda", generator=g)
    mid = torch.randn(T, inter, device="cuda", generator=g).to(dtype)
    d_mid = torch.randn(T, inter, device="cuda", generator=g).to(dtype)
    att_flop = 4.0 * n_seq * H * L * L * 64        # forward: Q K^T and P V
    cases = [
        ("ccr_attention_half (inference forward, for scale)", lambda: ops.attention(qkv, seq_start, seq_len, H, L), att_flop, None),
        ("ccr_attention_fwd_train_half", lambda: ops.attention_fwd_train(qkv, seq_start, seq_len, H, L), att_flop, None),
        ("ccr_attention_bwd_half", lambda: ops.attention_bwd(qkv, out, lse, d_out, seq_start, seq_len, H, L), 3.5 * att_flop, None),
        ("ccr_add_layernorm_bwd_half", lambda: ops.add_layernorm_bwd(x, res, gamma, 1e-12, d_y), None, T * hidden * (2 + 4 + 4 + 4 + 2)),
        ("ccr_gelu_bwd_half", lambda: ops.gelu_bwd(mid, d_mid), None, T * inter * 6),
    ]
    for name, fn, flop, nbytes in cases:
        t = timed(fn, runs, warmup)
        rows.append({"kernel": name, "dtype": str(dtype)[6:], "shape": f"{n_seq}x{L} tokens, {H} heads", **t,
                     "tflops": round(flop / t["median_ms"] / 1e9, 2) if flop else "", "gb_per_s": round(nbytes / t["median_ms"] / 1e6, 1) if nbytes else ""})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--dropout", type=float, default=0.0, help="> 0: the dropout mode (three columns, see above)")
    ap.add_argument("--ab-tree", default=None, help="with --dropout: a checkout of the parent commit, library built (see above)")
    args = ap.parse_args(argv)
    assert args.runs >= 20, "a median of at least 20 runs"
    if args.dropout > 0:
        return main_dropout(args)
    from transformers import BertConfig, BertModel
    from ccrec_amd import ops
    from ccrec_amd.fused_bert import FusedBertEncoder
    ops.require_gpu()
    torch.manual_seed(0)
    model = BertModel(BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False).cuda().train()
    enc = FusedBertEncoder(model)
    shapes = [("90x128 ragged", 90, 128, 0.4), ("90x256 ragged", 90, 256, 0.4), ("128x128 full (16K tokens)", 128, 128, 1.0)]
    result = {"tool": "tools/bench_encoder_train.py", "device": torch.cuda.get_device_name(0), "model": "BERT-base (random init, dropout 0)",
              "what": "forward + backward of the encoder, ms per step (median)", "steps": [], "kernels": []}
    for name in args.dtypes.split(","):
        dtype = DTYPES[name]
        for label, n, L, fill in shapes:
            ids, mask, lengths = ragged_batch(n, L, fill, seed=L + n)
            rec = {"batch": label, "dtype": name, "real_tokens": int(lengths.sum()), "padded_tokens": n * L}
            rec.update(bench_step(model, enc, ids, mask, lengths, dtype, args.runs, args.warmup))
            result["steps"].append(rec)
            print(json.dumps(rec), flush=True)
        bench_kernels(dtype, args.runs, args.warmup, result["kernels"])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "encoder_train_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    cols = ["kernel", "dtype", "shape", "median_ms", "min_ms", "max_ms", "runs", "tflops", "gb_per_s"]
    with open(os.path.join(args.out, "encoder_train_kernel_stats.csv"), "w") as f:
        f.write(",".join(cols) + "\n")
        for r in result["kernels"]:
            f.write(",".join(f'"{r[c]}"' if isinstance(r[c], str) and "," in r[c] else str(r[c]) for c in cols) + "\n")
    print(json.dumps(result["kernels"]))


if __name__ == "__main__":
    main()
