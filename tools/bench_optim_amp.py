#!/usr/bin/env python
"""The fp16 fine-tune step's optimizer work under loss scaling and gradient clipping, on BERT-base's real parameter list (default config,
random init, every parameter with a gradient that was multiplied by the loss scale):

(a) torch.amp.GradScaler + clip_grad_norm_ + FusedAdamW.step() as they ran before the optimizer knew about scaling: unscale_ (a pass
    over every gradient), clip_grad_norm_ (two more), GradScaler.step's host read of found_inf, then the plain step
(b) torch.amp.GradScaler through torch's _step_supports_amp_scaling protocol + FusedAdamW(max_grad_norm=1): torch's own inf check
    (one pass) + statistics + control + scaled step
(c) optim.LossScaler + FusedAdamW(max_grad_norm=1): statistics + control + scaled step, nothing else
and the plain FusedAdamW.step() beside them.  Every variant owns its model (unscale_ rewrites the gradients of (a) in place).

Also the device time of each library call alone (ten calls back to back between two events): ccr_grad_stats (4 B per parameter)
against ccr_pack_bf16's rate measured in the same process, ccr_adamw_control_update, ccr_adamw_step_scaled and ccr_adamw_step (28 B per
parameter); with --parent-lib, ccr_adamw_step of that library (a build of the parent commit) alternates with this one's.

Timing: device events around each run, 5 warm-up rounds, the median of 20 rounds, the variants ALTERNATING inside every round in one
process; the whole table is measured twice (two passes), and the larger of the two passes' differences is the run-to-run spread the
file reports.  Writes <out>/optim_amp.json and <out>/optim_amp.md and prints the JSON.

    python tools/bench_optim_amp.py [--out profiles] [--runs 20] [--warmup 5] [--parent-lib path/to/libccr_hip.so]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd"), os.path.join(ROOT, "tools")]

from bench_optim import alternate, build, pack_rate      # noqa: E402

SCALE, MAX_NORM, LR = 65536.0, 1.0, 1e-6


def scaled_gradients(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * (1e-3 * SCALE)


def variants():
    from ccrec_amd import optim
    models = {}
    for key in ("a", "b", "c", "plain"):
        torch.manual_seed(0)
        models[key] = build("bert-base").cuda()
        scaled_gradients(models[key], 1)
    params = {key: list(m.parameters()) for key, m in models.items()}
    opt_a = optim.FusedAdamW(params["a"], lr=LR)
    opt_a._step_supports_amp_scaling = False      # as before this optimizer spoke the protocol: GradScaler unscales and reads found_inf itself
    opt_b = optim.FusedAdamW(params["b"], lr=LR, max_grad_norm=MAX_NORM)
    opt_c = optim.FusedAdamW(params["c"], lr=LR, max_grad_norm=MAX_NORM)
    opt_plain = optim.FusedAdamW(params["plain"], lr=LR)
    # a growth interval beyond the run: the scale stays at 65536 (unscale_ shrinks (a)'s gradients in place, which costs the same passes)
    scaler_a = torch.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=10 ** 9)
    scaler_b = torch.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=10 ** 9)
    for s in (scaler_a, scaler_b):
        s.scale(torch.zeros((), device="cuda"))
    scaler_c = optim.LossScaler(init_scale=SCALE, growth_interval=10 ** 9)

    def a():
        scaler_a.unscale_(opt_a)
        torch.nn.utils.clip_grad_norm_(params["a"], MAX_NORM)
        scaler_a.step(opt_a)
        scaler_a.update()

    def b():
        scaler_b.step(opt_b)
        scaler_b.update()

    def c():
        scaler_c.step(opt_c)
        scaler_c.update()

    fns = {"(a) GradScaler.unscale_ + clip_grad_norm_ + GradScaler.step(plain FusedAdamW)": a,
           "(b) GradScaler.step through the protocol, FusedAdamW(max_grad_norm)": b,
           "(c) LossScaler.step, FusedAdamW(max_grad_norm)": c,
           "plain FusedAdamW.step() (no scaling, no clipping)": opt_plain.step}
    return fns, opt_c, opt_plain, sum(p.numel() for p in params["c"]), (models, scaler_a, scaler_b, scaler_c)


def library_calls(opt_c, opt_plain, n, parent_lib, runs, warmup):
    """Device time per call: ten calls back to back between two events (the host runs ahead of the device)."""
    from ccrec_amd import _lib
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    seg, count = opt_c._segments, opt_c._n_segments
    segments = ctypes.c_void_p(seg.ctypes.data)
    partials, control = opt_c._partials, torch.zeros(16, dtype=torch.float32, device="cuda")
    n_partials = lib.ccr_grad_stats_workspace_bytes(segments, count) // 4
    control[0] = 1.0      # coef 1, skip 0: the scaled step does the plain step's work
    cptr, pptr = ctypes.c_void_p(control.data_ptr()), ctypes.c_void_p(partials.data_ptr())
    plain_seg = ctypes.c_void_p(opt_plain._segments.ctypes.data)

    def ten(call):
        def run():
            for _ in range(10):
                _lib.check(call(), "library call")
        return run

    calls = {"ccr_grad_stats": (ten(lambda: lib.ccr_grad_stats(segments, count, pptr, stream)), 4 * n),
             "ccr_adamw_step_scaled (coef 1)": (ten(lambda: lib.ccr_adamw_step_scaled(segments, count, 0.1, 0.999, 0.001, 1e-8, cptr, stream)), 28 * n),
             "ccr_adamw_step": (ten(lambda: lib.ccr_adamw_step(plain_seg, opt_plain._n_segments, 0.1, 0.999, 0.001, 1e-8, stream)), 28 * n)}
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        parent.ccr_adamw_step.argtypes = lib.ccr_adamw_step.argtypes
        parent.ccr_version.restype = ctypes.c_int
        name = f"ccr_adamw_step of the parent commit's library (version {parent.ccr_version()})"
        calls[name] = (ten(lambda: parent.ccr_adamw_step(plain_seg, opt_plain._n_segments, 0.1, 0.999, 0.001, 1e-8, stream)), 28 * n)
    t = alternate({k: fn for k, (fn, _) in calls.items()}, runs, warmup)
    out = {}
    for k, rec in t.items():
        out[k] = {key: (round(v / 10, 4) if key.endswith("_ms") else v) for key, v in rec.items()}
        out[k]["bytes"] = calls[k][1]
        out[k]["gb_per_s"] = round(calls[k][1] / out[k]["median_ms"] / 1e6, 1)

    # the control kernel reads its own output (the scale): time it apart, on a block of its own
    own = torch.zeros(16, dtype=torch.float32, device="cuda")
    optr = ctypes.c_void_p(own.data_ptr())
    t = alternate({"ccr_adamw_control_update": ten(lambda: lib.ccr_adamw_control_update(optr, pptr, n_partials, MAX_NORM, 0, 2.0, 0.5, 2000, None, None, stream))},
                  runs, warmup)["ccr_adamw_control_update"]
    out[f"ccr_adamw_control_update ({n_partials} partials)"] = {key: (round(v / 10, 4) if key.endswith("_ms") else v) for key, v in t.items()}
    return out


def to_markdown(r):
    lines = [f"# Loss scaling and clipping inside the optimizer step ({r['device']})", "",
             f"`{r['tool']}`: BERT-base, {r['tensors']} tensors, {r['parameters'] / 1e6:.1f} M parameters; device events, {r['warmup']} warm-up rounds, "
             f"median of {r['runs']} rounds, the variants alternating in one process; two passes.  All numbers measured by this run.", "",
             "## one optimizer step under loss scaling (scale 65536) and clipping (max_norm 1), host work included", "",
             "| variant | pass 1 median ms | min | max | pass 2 median ms | min | max |", "|---|---|---|---|---|---|---|"]
    for name in r["passes"][0]:
        p1, p2 = r["passes"][0][name], r["passes"][1][name]
        lines.append(f"| {name} | {p1['median_ms']} | {p1['min_ms']} | {p1['max_ms']} | {p2['median_ms']} | {p2['min_ms']} | {p2['max_ms']} |")
    lines += ["", f"Run-to-run spread (the largest difference between the two passes' medians): **{r['spread_ms']} ms**.", "",
              "## the library calls alone (device time per call, ten calls back to back)", "",
              f"`ccr_pack_bf16` in the same process (2 M x 768, 6 B per element): **{r['pack']['gb_per_s']} GB/s**.", "",
              "| call | median ms | min | max | bytes per parameter | GB/s | of the pack rate |", "|---|---|---|---|---|---|---|"]
    for name, t in r["library_calls"].items():
        if "gb_per_s" in t:
            lines.append(f"| {name} | {t['median_ms']} | {t['min_ms']} | {t['max_ms']} | {t['bytes'] // r['parameters']} | {t['gb_per_s']} | "
                         f"{t['gb_per_s'] / r['pack']['gb_per_s']:.2f} |")
        else:
            lines.append(f"| {name} | {t['median_ms']} | {t['min_ms']} | {t['max_ms']} | | | |")
    lines.append("")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libccr_hip.so built from the parent commit: its ccr_adamw_step alternates with this one's")
    args = ap.parse_args(argv)
    assert args.runs >= 20, "a median of at least 20 runs"
    from ccrec_amd import ops
    ops._require_optim_amp()
    result = {"tool": "tools/bench_optim_amp.py", "device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup}
    result["pack"] = pack_rate(args.runs, args.warmup)
    print(json.dumps(result["pack"]), flush=True)
    torch.cuda.empty_cache()
    fns, opt_c, opt_plain, n, keep = variants()
    result["tensors"], result["parameters"] = len(opt_c.param_groups[0]["params"]), n
    result["passes"] = [alternate(fns, args.runs, args.warmup) for _ in range(2)]
    result["spread_ms"] = round(max(abs(result["passes"][0][k]["median_ms"] - result["passes"][1][k]["median_ms"]) for k in fns), 4)
    print(json.dumps(result["passes"]), flush=True)
    result["library_calls"] = library_calls(opt_c, opt_plain, n, args.parent_lib, args.runs, args.warmup)
    print(json.dumps(result["library_calls"]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "optim_amp.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    with open(os.path.join(args.out, "optim_amp.md"), "w") as f:
        f.write(to_markdown(result))


if __name__ == "__main__":
    main()
