"""The encoder layer kernels' training forward and backward (csrc/ccr_encoder_bwd.hip, ops.attention_train / add_layernorm_train /
gelu_train, FusedBertEncoder.forward_train) on the GPU, in both 16-bit operand types.

Bars.  Every kernel is compared with a high-precision reference (fp32 autograd for the attention, fp64 for LayerNorm and GELU) and
must be no further from it than a stated multiple of a YARDSTICK's own error, measured in the same test on the same inputs: torch's
own path in the precision the reference's training runs in (16-bit matmul operands + fp32 softmax for the attention -- what autocast
does; torch's fp32 F.layer_norm backward for the LayerNorm).  Floors are written in units of the number format's spacing.  The measured
ratios are printed (pytest -s)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, PKG  # noqa: F401
from helpers import (ATT_CASES, DTYPES, LN_EPS, MANTISSA, att_inputs as _att_inputs, att_reference as _att_reference,
                     ln_inputs as _ln_inputs, ln_torch_backward as _ln_torch_backward, run_att as _run_att, spacing as _spacing)  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- attention backward
# (cases, inputs and references: tests/helpers.py, shared with test_gpu_encoder_train_edges.py)
_ATT_REF = {}


def _att_case(name, dtype):
    """Inputs, fp32 reference and yardstick of one case, computed once and shared (never modified)."""
    key = (name, dtype)
    if key not in _ATT_REF:
        kind, lens, H = ATT_CASES[name]
        case = _att_inputs(kind, lens, H, dtype, seed=len(name) + 7 * H)
        case["ref"], case["lse_ref"] = _att_reference(case, None)
        case["yard"], _ = _att_reference(case, dtype)
        _ATT_REF[key] = case
    return _ATT_REF[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(ATT_CASES))
def test_attention_backward_is_as_close_to_fp32_as_the_16_bit_torch_path(name, dtype):
    """dQ, dK, dV vs fp32 autograd: max |err| / max |ref| and mean |err| / mean |ref| are at most 1.5 x those of torch autograd with
    16-bit matmuls and an fp32 softmax (the margin of test_gpu_encoder_fp16.py's "no further from fp32 than torch's own 16-bit path");
    the max has a floor of one spacing of the type at max |ref|.  Plus: lse, out == ops.attention bit for bit, zeros on padding rows,
    nothing non-finite, run-to-run determinism, and (bf16) exact linearity in d_out under a power-of-two factor."""
    from ccrec_amd import ops
    case = _att_case(name, dtype)
    H, live = case["H"], case["live"]
    out, lse, d_qkv = _run_att(case)
    assert d_qkv.dtype == dtype and d_qkv.shape == case["qkv"].shape
    assert torch.isfinite(d_qkv).all() and torch.isfinite(lse).all()
    assert (d_qkv[~live] == 0).all() and (lse[~live] == 0).all()
    assert torch.equal(out.view(torch.int16), ops.attention(case["qkv"], case["seq_start"], case["seq_len"], H, case["max_len"], case["pad_len"]).view(torch.int16))
    assert torch.allclose(lse[live], case["lse_ref"][live], atol=2e-5, rtol=2e-5), (lse - case["lse_ref"])[live].abs().max().item()
    got = d_qkv.float()
    for part, label in enumerate(("dQ", "dK", "dV")):
        cols = slice(part * H * 64, (part + 1) * H * 64)
        ref, yard, mine = case["ref"][live][:, cols], case["yard"][live][:, cols], got[live][:, cols]
        ref_max, ref_mean = ref.abs().max().item(), ref.abs().mean().item()
        k_max, y_max = (mine - ref).abs().max().item(), (yard - ref).abs().max().item()
        k_mean, y_mean = (mine - ref).abs().mean().item(), (yard - ref).abs().mean().item()
        print(f"attention_bwd {name} {str(dtype)[6:]} {label}: max err/max ref kernel {k_max / ref_max:.3e} torch {y_max / ref_max:.3e} "
              f"(ratio {k_max / max(y_max, 1e-30):.2f}); mean err/mean ref kernel {k_mean / ref_mean:.3e} torch {y_mean / ref_mean:.3e} "
              f"(ratio {k_mean / max(y_mean, 1e-30):.2f})")
        assert k_max <= max(1.5 * y_max, _spacing(ref_max, dtype)), (label, k_max, y_max, ref_max)
        assert k_mean <= 1.5 * y_mean, (label, k_mean, y_mean, ref_mean)
    _, _, again = _run_att(case)
    assert torch.equal(again.view(torch.int16), d_qkv.view(torch.int16))
    if dtype == torch.bfloat16:      # the backward is linear in d_out and a power-of-two factor commutes with every rounding
        _, _, scaled = _run_att(case, d_out=case["d_out"] * 4)
        assert torch.equal(scaled.view(torch.int16), (d_qkv * 4).view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_attention_train_autograd_function(dtype):
    """ops.attention_train: attention()'s bits forward, the kernel's d_qkv through autograd (a non-contiguous, fp32 upstream gradient)."""
    from ccrec_amd import ops
    case = _att_case("packed_12_heads", dtype)
    qkv = case["qkv"].clone().requires_grad_(True)
    out = ops.attention_train(qkv, case["seq_start"], case["seq_len"], case["H"], case["max_len"], case["pad_len"])
    assert torch.equal(out.detach().view(torch.int16), ops.attention(case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"]).view(torch.int16))
    (out.float() * case["d_out"].float()).sum().backward()
    _, _, want = _run_att(case)
    assert qkv.grad.dtype == dtype and torch.equal(qkv.grad.view(torch.int16), want.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
LN_SHAPES = [(1, 256), (5, 768), (1031, 768), (4, 2048)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("with_res", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("rows,dim", LN_SHAPES)
def test_layernorm_backward_against_fp64(rows, dim, with_res, dtype):
    """d_res, d_gamma, d_beta vs fp64 torch: at most 2 x the error of torch's fp32 F.layer_norm backward (max and mean; floor
    1e-6 max |ref|).  d_x == d_res rounded once; any output may be left out; two runs agree bit for bit."""
    from ccrec_amd import ops
    x, res, gamma, d_y = _ln_inputs(rows, dim, dtype, with_res, seed=rows + dim)
    v = x.float() if res is None else x.float() + res      # the fp32 sum both the kernel and the yardstick normalise
    ref = _ln_torch_backward(v, gamma, d_y, torch.float64)
    yard = _ln_torch_backward(v, gamma, d_y, torch.float32)
    d_res, d_x, d_gamma, d_beta = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y)
    for label, mine, r, y in zip(("d_res", "d_gamma", "d_beta"), (d_res, d_gamma, d_beta), ref, yard):
        assert mine.dtype == torch.float32 and torch.isfinite(mine).all()
        e_k, e_y = (mine.double() - r).abs(), (y.double() - r).abs()
        floor = 1e-6 * r.abs().max().item()
        print(f"layernorm_bwd {rows}x{dim} {'res' if with_res else 'nores'} {str(dtype)[6:]} {label}: max err kernel {e_k.max().item():.3e} torch "
              f"{e_y.max().item():.3e}; mean err kernel {e_k.mean().item():.3e} torch {e_y.mean().item():.3e}; max |ref| {r.abs().max().item():.3e}")
        assert e_k.max().item() <= 2 * e_y.max().item() + floor, (label, e_k.max().item(), e_y.max().item(), floor)
        assert e_k.mean().item() <= 2 * e_y.mean().item() + floor, (label, e_k.mean().item(), e_y.mean().item(), floor)
    assert d_x.dtype == dtype and torch.equal(d_x.view(torch.int16), d_res.to(dtype).view(torch.int16))
    # null-output combinations: what is asked for has the same bits
    for want in [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (True, False, True, True), (False, True, False, True)]:
        outs = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y, *want)
        for w, o, full in zip(want, outs, (d_res, d_x, d_gamma, d_beta)):
            assert (o is None) == (not w)
            if w:
                assert torch.equal(o.view(torch.int32 if o.dtype == torch.float32 else torch.int16),
                                   full.view(torch.int32 if full.dtype == torch.float32 else torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_add_layernorm_train_sums_the_gradients_of_both_outputs(dtype):
    """ops.add_layernorm_train: add_layernorm()'s bits forward; the fp32 and the 16-bit output both carry gradient, summed in fp32
    before the kernel runs; x, residual, gamma and beta receive theirs."""
    from ccrec_amd import ops
    x, res, gamma, d_y = _ln_inputs(5, 768, dtype, True, seed=3)
    beta = torch.linspace(-1, 1, 768, device="cuda")
    g16 = torch.randn(5, 768, device="cuda").to(dtype)
    xs, rs, gs, bs = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    f32, b16 = ops.add_layernorm_train(xs, rs, gs, bs, LN_EPS)
    w32, w16 = ops.add_layernorm(x, res, gamma, beta, LN_EPS)
    assert torch.equal(f32.detach(), w32) and torch.equal(b16.detach().view(torch.int16), w16.view(torch.int16))
    ((f32 * d_y).sum() + (b16.float() * g16.float()).sum()).backward()
    want = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y + g16.float())
    assert torch.equal(rs.grad, want[0]) and torch.equal(xs.grad.view(torch.int16), want[1].view(torch.int16))
    assert torch.equal(gs.grad, want[2]) and torch.equal(bs.grad, want[3])


# ---------------------------------------------------------------------------------------------------------------------- GELU backward
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_gelu_backward_against_fp64(dtype):
    """2^20 values, x ~ 3 N(0, 1), d_y ~ N(0, 1): |err| <= one spacing of the type at |ref| (at least 2^-24 for fp16, its subnormal
    spacing; bf16's normal range covers every value here down to 2^-126) + 1e-6 |d_y| (the zero crossing of Phi + x phi near -0.75)."""
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(1 << 20, generator=g)).to(dtype).cuda()
    d_y = torch.randn(1 << 20, generator=g).to(dtype).cuda()
    got = ops.gelu_bwd(x, d_y)
    assert got.dtype == dtype
    xd, dd = x.double(), d_y.double()
    ref = dd * (0.5 * (1 + torch.erf(xd / math.sqrt(2))) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi))
    exponent = torch.floor(torch.log2(ref.abs().clamp_min(1e-300)))
    floor_exp = -24.0 if dtype == torch.float16 else -126.0 - MANTISSA[dtype]
    spacing = torch.exp2(torch.clamp(exponent - MANTISSA[dtype], min=floor_exp))
    err = (got.double() - ref).abs()
    bad = err > spacing + 1e-6 * dd.abs()
    print(f"gelu_bwd {str(dtype)[6:]}: max err / spacing {(err / spacing).max().item():.3f}, violations {int(bad.sum())}")
    assert not bad.any(), (int(bad.sum()), x[bad][:4], got[bad][:4], ref[bad][:4])
    # ... and through autograd, out of place: gelu_'s bits forward, the pre-activation untouched
    xs = x.clone().requires_grad_(True)
    y = ops.gelu_train(xs)
    assert torch.equal(xs.detach().view(torch.int16), x.view(torch.int16))
    assert torch.equal(y.detach().view(torch.int16), ops.gelu_(x.clone()).view(torch.int16))
    y.backward(d_y)
    assert torch.equal(xs.grad.view(torch.int16), got.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------- whole layer stack
def _tiny_model(kind, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    if kind == "bert":
        from transformers import BertConfig, BertModel
        m = BertModel(BertConfig(vocab_size=600, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                 max_position_embeddings=128, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout))
        attn = [(l.attention.self.query, l.attention.self.key) for l in m.encoder.layer]
    else:
        from transformers import DistilBertConfig, DistilBertModel
        m = DistilBertModel(DistilBertConfig(vocab_size=600, dim=256, n_layers=2, n_heads=4, hidden_dim=512, max_position_embeddings=128,
                                             dropout=dropout, attention_dropout=dropout))
        attn = [(l.attention.q_lin, l.attention.k_lin) for l in m.transformer.layer]
    with torch.no_grad():      # the default init (std 0.02) leaves every softmax uniform: widen the attention projections
        for q, k in attn:
            q.weight.mul_(20.0)
            k.weight.mul_(20.0)
    return m.cuda()


_KEY_BIAS = ("attention.self.key.bias", "attention.k_lin.bias")

STACK_LENS = [1, 70, 17, 33, 64, 65, 9, 40, 2]


def _stack_batch():
    g = torch.Generator().manual_seed(11)
    L = max(STACK_LENS)
    ids = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    mask = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    for r, n in enumerate(STACK_LENS):
        ids[r, :n] = torch.randint(1, 600, (n,), generator=g)
        mask[r, :n] = 1
    return ids.cuda(), mask.cuda()


def _step_loss(tower, ids, mask, autocast_dtype):
    """One MultipleNrlStep loss (three tower forwards with gradients on: queries, positives, hard negatives) over the nine texts."""
    import contextlib
    from ccrec_amd.bbpr_loss import MultipleNrlStep

    def forward(ptr):
        ptr = torch.as_tensor(ptr, device=ids.device)
        return tower(input_ids=ids[ptr], attention_mask=mask[ptr], input_step="inputs", output_step="mean_pooling")

    step = MultipleNrlStep(forward, torch.tensor([0, 1, 2]), torch.arange(9), {0: [6, 7], 1: [7, 8], 2: [8, 6]})
    batch = torch.tensor([[0, 3, 1.0], [1, 4, 1.0], [2, 5, 1.0]])
    ctx = contextlib.nullcontext() if autocast_dtype is None else torch.autocast("cuda", dtype=autocast_dtype)
    with ctx:
        return step(batch)


def _grads(tower, ids, mask, autocast_dtype):
    tower.zero_grad(set_to_none=True)
    loss = _step_loss(tower, ids, mask, autocast_dtype)
    loss.backward()
    return loss.item(), {n: p.grad.detach().clone() for n, p in tower.cls_model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_fine_tune_step_through_the_layer_kernels(kind, dtype, monkeypatch):
    """Parameter gradients of one MultipleNrlStep through the tower on the kernels' training path (CCREC_FUSED_ENCODER_TRAIN=1, under
    autocast) vs the fp32 module's; yardstick: the module under the same autocast.  Per parameter: relative L2 error <= 1.5 x the
    module's (floor 2^-8 bf16 / 2^-11 fp16), cosine >= the module's - 1e-3.  The loss agrees with the fp32 loss as the forward tests ask of
    hidden states: within 1.5 x the autocast module's own deviation, floor one spacing of the type at the loss.  After an AdamW step the
    next training forward uses the new weights."""
    from ccrec_amd import ops
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    model = _tiny_model(kind)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()
    ids, mask = _stack_batch()
    calls = []
    real = ops.attention_train
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN", raising=False)
    loss32, g32 = _grads(tower, ids, mask, None)
    loss_m, g_m = _grads(tower, ids, mask, dtype)
    assert not calls                                         # the variable is unset: the module ran, under autocast too
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    loss_k, g_k = _grads(tower, ids, mask, dtype)
    assert len(calls) == 3 * 2                               # three tower forwards x two layers
    pooler = {n for n in g32 if n.startswith("pooler.")}
    assert set(g_k) == set(g32) - pooler and set(g_m) - pooler == set(g_k)      # the same parameters train (the pooler never does)
    floor = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    worst = (0.0, None)
    for name in sorted(g_k):
        ref = g32[name].double()
        assert torch.isfinite(g_k[name]).all() and g_k[name].dtype == torch.float32
        if name.endswith(_KEY_BIAS):
            # The key projection's bias adds the same q . b_k to every score of a query's row and the softmax is invariant to that shift:
            # its gradient is identically zero, and what any path returns is the rounding residue of sum_tokens dK -- there is no
            # direction to compare.  The check that is left: the residue is negligible, no larger than 1.5 x the module's or the floor
            # x the gradient of the same layer's query bias (the sum of the same number of dQ rows).
            scale = g32[name.replace("key.bias", "query.bias").replace("k_lin.bias", "q_lin.bias")].double().norm().item()
            assert g_k[name].double().norm().item() <= max(1.5 * g_m[name].double().norm().item(), floor * scale), (name, g_k[name].norm().item(), scale)
            assert ref.norm().item() <= 1e-3 * scale, (name, ref.norm().item(), scale)      # (zero in fp32 as well)
            continue
        rel_k = ((g_k[name].double() - ref).norm() / ref.norm()).item()
        rel_m = ((g_m[name].double() - ref).norm() / ref.norm()).item()
        cos_k = F.cosine_similarity(g_k[name].double().flatten(), ref.flatten(), dim=0).item()
        cos_m = F.cosine_similarity(g_m[name].double().flatten(), ref.flatten(), dim=0).item()
        worst = max(worst, (rel_k / max(rel_m, floor), name))
        assert rel_k <= max(1.5 * rel_m, floor), (name, rel_k, rel_m)
        assert cos_k >= cos_m - 1e-3, (name, cos_k, cos_m)
    print(f"fine-tune step {kind} {str(dtype)[6:]}: loss fp32 {loss32:.6f} module {loss_m:.6f} kernels {loss_k:.6f}; "
          f"worst relative-L2 ratio kernel / max(module, floor) {worst[0]:.2f} ({worst[1]})")
    assert abs(loss_k - loss32) <= max(1.5 * abs(loss_m - loss32), _spacing(loss32, dtype)), (loss_k, loss_m, loss32)

    # one optimizer step on the kernel path's gradients: the next training forward reads the new weights (no stale 16-bit copy)
    opt = torch.optim.AdamW(tower.parameters(), lr=5e-3)
    opt.step()
    loss_next = _step_loss(tower, ids, mask, dtype).item()
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN")
    loss_next_m = _step_loss(tower, ids, mask, dtype).item()
    loss_next32 = _step_loss(tower, ids, mask, None).item()
    tol = max(1.5 * abs(loss_next_m - loss_next32), _spacing(loss_next32, dtype))
    assert abs(loss_next32 - loss32) > 4 * tol, (loss_next32, loss32, tol)      # the step moved the loss by more than the tolerance ...
    assert abs(loss_next - loss_next32) <= tol, (loss_next, loss_next_m, loss_next32)      # ... and the kernel path followed it


def test_training_path_gating(monkeypatch):
    """Opt-in only: without CCREC_FUSED_ENCODER_TRAIN=1 the module runs; with it, a model in training mode with dropout 0.1 is refused
    with the dropout reason and the tower falls back to the module; outside autocast the module runs; eval mode is accepted."""
    from ccrec_amd import fused_bert, ops
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    ids, mask = _stack_batch()
    calls = []
    real = ops.attention_train
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    wet = _tiny_model("bert", dropout=0.1)
    tower = NaiveItemTower(wet, torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    assert "dropout" in fused_bert.train_unsupported_reason(wet)
    assert torch.isfinite(_step_loss(tower, ids, mask, torch.bfloat16)) and not calls       # refused: the module trained
    with pytest.raises(AssertionError, match="dropout"):
        fused_bert.for_model(wet).forward_train(ids, mask.sum(1).to(torch.int32))
    tower.eval()                                            # dropout is inactive in eval mode: accepted
    assert fused_bert.train_unsupported_reason(wet) is None
    _step_loss(tower, ids, mask, torch.bfloat16)
    assert len(calls) == 6
    del calls[:]
    _step_loss(tower, ids, mask, None)                      # no autocast: the caller asked for an fp32 step
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():      # no gradients: the inference path, as ever
        tower(input_ids=ids, attention_mask=mask, input_step="inputs", output_step="mean_pooling")
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN")
    _step_loss(tower, ids, mask, torch.bfloat16)
    assert not calls


# ----------------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_return_an_error_code_and_launch_nothing():
    """Null pointers, max_len > 512, an unsupported dim and a too-small workspace: an error code, the outputs keep their bytes."""
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    case = _att_case("packed_12_heads", torch.bfloat16)
    H, n_seq = case["H"], len(case["lens"])
    out, lse = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], H, case["max_len"])
    d_qkv = torch.full_like(case["qkv"], 7.0)
    need = lib.ccr_attention_bwd_workspace_bytes(n_seq, H, case["max_len"])
    assert need == n_seq * H * 224 * 4 and lib.ccr_attention_bwd_workspace_bytes(n_seq, H, 513) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p, st = ops._ptr, ops._stream(d_qkv)
    code = _lib.DTYPE_BF16

    def bwd(qkv=case["qkv"], max_len=case["max_len"], ws_bytes=need, dtype=code):
        return lib.ccr_attention_bwd_half(p(qkv), p(out), p(lse), p(case["d_out"]), p(case["seq_start"]), p(case["seq_len"]), p(d_qkv), n_seq, H,
                                          max_len, 0, 0.125, dtype, p(ws), ws_bytes, st)

    assert bwd(qkv=None) == _lib.CCR_ERR_INVALID and bwd(max_len=513) == _lib.CCR_ERR_INVALID and bwd(dtype=_lib.DTYPE_F32) == _lib.CCR_ERR_INVALID
    assert bwd(ws_bytes=need - 1) == _lib.CCR_ERR_WORKSPACE and b"workspace" in lib.ccr_last_error()
    lse2 = torch.full_like(lse, 7.0)
    assert lib.ccr_attention_fwd_train_half(p(case["qkv"]), p(case["seq_start"]), p(case["seq_len"]), p(out), None, n_seq, H, case["max_len"], 0,
                                            0.125, code, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_attention_fwd_train_half(p(case["qkv"]), p(case["seq_start"]), p(case["seq_len"]), p(out), p(lse2), n_seq, H, 513, 0,
                                            0.125, code, st) == _lib.CCR_ERR_INVALID
    x = torch.zeros(8, 320, dtype=torch.bfloat16, device="cuda")
    gamma, d_y = torch.ones(320, device="cuda"), torch.ones(8, 320, device="cuda")
    d_res, d_gamma = torch.full((8, 320), 7.0, device="cuda"), torch.full((320,), 7.0, device="cuda")
    big = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def ln(x=x, gamma=gamma, dim=320, ws=big, ws_bytes=1 << 16):
        return lib.ccr_add_layernorm_bwd_half(p(x), None, p(gamma), 1e-12, p(d_y), p(d_res), None, p(d_gamma), None, 8, dim, code, p(ws), ws_bytes, st)

    assert ln() == _lib.CCR_ERR_INVALID and ln(dim=2304) == _lib.CCR_ERR_INVALID and ln(x=None, dim=256) == _lib.CCR_ERR_INVALID
    assert ln(dim=256, ws_bytes=2 * 2 * 256 * 4 - 1) == _lib.CCR_ERR_WORKSPACE and ln(dim=256, ws=None, ws_bytes=0) == _lib.CCR_ERR_WORKSPACE
    h = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    d_h = torch.full((64,), 7.0, dtype=torch.bfloat16, device="cuda")
    assert lib.ccr_gelu_bwd_half(p(h), None, p(d_h), 64, code, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_gelu_bwd_half(p(h), p(h), p(d_h), 60, code, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_gelu_bwd_half(p(h), p(h), ctypes.c_void_p(d_h.data_ptr() + 2), 56, code, st) == _lib.CCR_ERR_INVALID
    torch.cuda.synchronize()
    assert (d_qkv == 7).all() and (lse2 == 7).all() and (d_res == 7).all() and (d_gamma == 7).all() and (d_h == 7).all()
