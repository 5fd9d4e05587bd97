"""The encoder backward kernels (csrc/ccr_encoder_bwd.hip) with probes whose expected value is exact, and at every launch path.

tests/test_gpu_encoder_train.py holds the kernels to an aggregate error on random inputs; here
  1. the SELECTOR PROBE (builder and its contract: tests/helpers.py, tests/test_cpu_encoder_probe.py) makes every element of dQ, dK, dV a sum
     of a few exactly representable products, so a streamed row that is dropped, doubled or misplaced moves elements by whole units;
  2. the fp16 row factor of dS runs at the magnitudes it exists for: exact linearity under 2^-k, magnitudes that rise and fall by 2^12
     along a sequence, a peaked softmax, a query whose dS are all zero;
  3. the attention backward writes a canary-filled d_qkv: live rows written, padding rows zero, every other row untouched;
  4. the LayerNorm backward runs every width C = 1 .. 8 and every workgroup count of both stages, with integer d_y whose column sums are exact;
  5. the GELU backward runs one vector, the workgroup edges, past the grid cap, and every 16-bit pattern of x.
Figures are printed (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401
from helpers import (ATT_CASES, DTYPES, ENC_PROBE_HEADS, ENC_PROBE_LENS, LN_EPS, MANTISSA, att_inputs, att_reference, encoder_probe,
                     encoder_probe_leak_bound, ln_inputs, ln_torch_backward, run_att, spacing)

pytestmark = pytest.mark.gpu

IDS = ["bf16", "fp16"]
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


# ------------------------------------------------------------------------------------------------------- 1. the selector probe
_PROBE = {}


def _probe_reference():
    """fp64 autograd of plain softmax attention on the probe's inputs, once per process: per sequence (grad [len, 3, H, 64], out [len, H, 64],
    lse [len, H]) as fp64 CPU tensors."""
    if "ref" not in _PROBE:
        ref = []
        for seq in encoder_probe():
            rows = torch.from_numpy(seq["qkv"]).permute(1, 2, 0, 3)                       # [3, H, len, 64] fp64
            q, k, v = (rows[i].clone().requires_grad_(True) for i in range(3))
            scores = q @ k.transpose(1, 2) * 0.125
            out = torch.softmax(scores, dim=-1) @ v
            out.backward(torch.from_numpy(seq["d_out"]).permute(1, 0, 2))
            grad = torch.stack([q.grad, k.grad, v.grad]).permute(2, 0, 1, 3).contiguous()  # [len, 3, H, 64]
            half = []                                                                      # the closed form of O: (V_a + V_b) / 2
            for head in seq["heads"]:
                sel = np.stack([np.isin(np.arange(seq["length"]), head["groups"][g]) for g in head["select"]]).astype(np.float64)
                half.append(torch.from_numpy(sel / sel.sum(1, keepdims=True) @ head["v"]))
            ref.append(dict(grad=grad, out=out.detach().permute(1, 0, 2).contiguous(), lse=torch.logsumexp(scores.detach(), dim=-1).T.contiguous(),
                            out_exact=torch.stack(half, dim=1)))
        _PROBE["ref"] = ref
    return _PROBE["ref"]


def _probe_case(kind, dtype):
    """The probe's sequences in one launch, padded (NaN in the padding rows) or packed."""
    seqs, H = encoder_probe(), ENC_PROBE_HEADS
    lens = ENC_PROBE_LENS
    if kind == "padded":
        L = max(lens)
        starts, pad_len, T = [s * L for s in range(len(lens))], L, len(lens) * L
    else:
        starts, pad_len, T = [sum(lens[:s]) for s in range(len(lens))], 0, sum(lens)
    qkv = torch.full((T, 3 * H * 64), float("nan"), dtype=torch.float64)
    d_out = torch.full((T, H * 64), float("nan"), dtype=torch.float64)
    live = torch.zeros(T, dtype=torch.bool)
    for s, seq in zip(starts, seqs):
        n = seq["length"]
        qkv[s:s + n] = torch.from_numpy(seq["qkv"]).reshape(n, -1)
        d_out[s:s + n] = torch.from_numpy(seq["d_out"]).reshape(n, -1)
        live[s:s + n] = True
    assert torch.equal(qkv[live].to(dtype).double(), qkv[live])                           # small integers: values of the type
    dev = "cuda"
    return dict(qkv=qkv.to(dtype).to(dev), d_out=d_out.to(dtype).to(dev), live=live.to(dev), starts=starts, lens=lens, H=H, pad_len=pad_len,
                max_len=max(lens), seq_start=torch.tensor(starts, dtype=torch.int32, device=dev),
                seq_len=torch.tensor(lens, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["padded", "packed"])
def test_selector_probe_places_every_streamed_row(kind, dtype):
    """Against fp64 autograd of plain softmax attention on the same inputs.  Preconditions: the forward's out is (V_a + V_b) / 2 to 1e-6 and
    lse passes at 2e-5; the exact gradients (fp64 snapped to multiples of 1/64, the rest being the e^-24 leak) are values of the type.
    Where the exact value is non-zero, d_qkv is within ONE spacing of the type at |exact| -- a misplaced row moves elements by whole
    multiples of 1/64 x 8 significant bits, far beyond that; the arithmetic (tests/test_cpu_encoder_probe.py) says that NO element differs
    at all, and the count is printed.  Where it is zero, |d_qkv| <= len e^-24 64 4, the leak bound.  Padding rows are zero; two runs agree
    bit for bit.  Measured on the MI355X: 0 elements differ, in both types and both layouts."""
    case, ref = _probe_case(kind, dtype), _probe_reference()
    H = case["H"]
    out, lse, d_qkv = run_att(case)
    assert d_qkv.dtype == dtype and torch.isfinite(d_qkv).all()
    assert (d_qkv[~case["live"]] == 0).all()
    got_all, out_all, lse_all = d_qkv.double().cpu(), out.double().cpu(), lse.double().cpu()
    differ = total = 0
    worst_zero = 0.0
    for s, n, r in zip(case["starts"], case["lens"], ref):
        assert (out_all[s:s + n].view(n, H, 64) - r["out_exact"]).abs().max().item() <= 1e-6
        assert (r["out"] - r["out_exact"]).abs().max().item() <= 1e-8                     # (the reference agrees with the closed form)
        assert torch.allclose(lse_all[s:s + n], r["lse"], atol=2e-5, rtol=2e-5), (lse_all[s:s + n] - r["lse"]).abs().max().item()
        exact = torch.round(r["grad"] * 64) / 64
        leak = encoder_probe_leak_bound(n)
        assert (r["grad"] - exact).abs().max().item() <= leak
        assert torch.equal(exact.to(dtype).double(), exact), "an exact gradient is not a value of the type"
        got = got_all[s:s + n].view(n, 3, H, 64)
        nz = exact != 0
        assert torch.equal(r["grad"].to(dtype).double()[nz], exact[nz])                    # = the reference rounded once
        assert n < 31 or all(nz[:, part].any(0).any(0).all() for part in range(3))        # every column, in some head
        one = torch.exp2(torch.floor(torch.log2(exact[nz].abs())) - MANTISSA[dtype])
        err = (got[nz] - exact[nz]).abs()
        assert (err <= one).all(), (n, int((err > one).sum()), err.max().item())
        differ += int((err != 0).sum())
        total += int(nz.sum())
        worst_zero = max(worst_zero, got[~nz].abs().max().item())
        assert got[~nz].abs().max().item() <= leak, (n, got[~nz].abs().max().item(), leak)
    print(f"selector probe {kind} {str(dtype)[6:]}: {differ} of {total} non-zero elements differ from the exact value; largest |value| where the "
          f"exact value is 0: {worst_zero:.2e}")
    _, _, again = run_att(case)
    assert _same_bits(again, d_qkv)


# ------------------------------------------------------------------------------------------------------- 2. the fp16 row factor
_LINEAR = {}


@pytest.mark.parametrize("k", [-4, 6, 10])
@pytest.mark.parametrize("name", ["packed_blocks", "padded_edges"])
def test_fp16_backward_is_exactly_linear_under_a_power_of_two(name, k):
    """d_out snapped to multiples of 2^-6, |d_out| <= 4, then times 2^-k (exact in fp16 down to 2^-16).  Every intermediate scales by the exact
    power of two and the row factor makes the rounded dS bits identical, so the fp32 result is base 2^-k exactly: bit for bit wherever the
    rounding of neither run falls on fp16's fixed subnormal spacing (|base| >= 2^-14 and |base| 2^-k >= 2^-14; for k > 0 the second implies
    the first, which is the condition as the issue states it; with k = -4 a base below 2^-14 was itself rounded at 2^-24, which 2^4 magnifies).
    Elsewhere: within one subnormal spacing, 2^-24 (k > 0) or 2^-24 2^-k (k < 0).  Without the factor dS of the k = 10 run falls to a few bits."""
    dtype = torch.float16
    if name not in _LINEAR:
        kind, lens, H = ATT_CASES[name]
        case = att_inputs(kind, lens, H, dtype, seed=len(name) + 7 * H)
        d_out = (torch.round(case["d_out"].float() * 64) / 64).clamp(-4, 4).to(dtype)
        _LINEAR[name] = (case, d_out, run_att(case, d_out=d_out)[2])
    case, d_out, base = _LINEAR[name]
    scaled_in = (d_out.float() * 2.0 ** -k).to(dtype)
    live = case["live"]
    assert torch.equal(scaled_in[live].float() * 2.0 ** k, d_out[live].float())          # the scaled input is exact
    got = run_att(case, d_out=scaled_in)[2][live].double()
    want = base[live].double() * 2.0 ** -k
    assert want.abs().max().item() < 65504
    normal = (base[live].double().abs() >= 2.0 ** -14) & (want.abs() >= 2.0 ** -14)
    wrong = int((got[normal] != want[normal]).sum())
    rest = (got[~normal] - want[~normal]).abs().max().item() if (~normal).any() else 0.0
    print(f"fp16 linearity {name} 2^{-k}: {int(normal.sum())} elements in the normal range, {wrong} differ; {int((~normal).sum())} below it, "
          f"largest deviation {rest:.3e} (bound {2.0 ** -24 * max(1.0, 2.0 ** -k):.3e}); max |base| {base[live].float().abs().max().item():.3f}")
    assert normal.float().mean().item() > (0.9 if k < 10 else 0.2)                       # the bit-exact part is most of the tensor
    assert wrong == 0
    assert rest <= 2.0 ** -24 * max(1.0, 2.0 ** -k)


def _bar_check(label, mine, ref, yard, dtype):
    """The bar of tests/test_gpu_encoder_train.py: max |err| <= max(1.5 x the 16-bit torch path's, one spacing at max |ref|); mean <= 1.5 x."""
    ref_max = ref.abs().max().item()
    k_max, y_max = (mine - ref).abs().max().item(), (yard - ref).abs().max().item()
    k_mean, y_mean = (mine - ref).abs().mean().item(), (yard - ref).abs().mean().item()
    print(f"{label}: max err / max ref kernel {k_max / ref_max:.3e} torch {y_max / ref_max:.3e} (ratio {k_max / max(y_max, 1e-30):.2f}); "
          f"mean ratio {k_mean / max(y_mean, 1e-30):.2f}")
    bar = max(1.5 * y_max, spacing(ref_max, dtype))
    assert k_max <= bar, (label, k_max, y_max, ref_max)
    assert k_mean <= 1.5 * y_mean, (label, k_mean, y_mean)
    return bar


def _flipped(case):
    """The same sequence (one, packed) with its rows in reversed order: attention commutes with that."""
    out = dict(case)
    out["qkv"], out["d_out"] = case["qkv"].flip(0).contiguous(), case["d_out"].flip(0).contiguous()
    return out


def _ds_tile_medians(case, own_keys):
    """log2 of the largest |dS| of an own row within each streamed tile of 32 rows (fp32, from the case's inputs: one packed sequence), its
    median over the own rows and heads -> one value per streamed tile.  own_keys False: the dQ pass (own = queries, streamed = keys)."""
    n, H = case["lens"][0], case["H"]
    r = case["qkv"].float().view(n, 3, H, 64).permute(1, 2, 0, 3)
    do = case["d_out"].float().view(n, H, 64).permute(1, 0, 2)
    p = torch.softmax(r[0] @ r[1].transpose(1, 2) * 0.125, dim=-1)
    ds = (p * (do @ r[2].transpose(1, 2) - (do * (p @ r[2])).sum(-1, keepdim=True))).abs()
    if own_keys:
        ds = ds.transpose(1, 2)
    tile = torch.arange(n, device=ds.device) // 32
    per = torch.stack([ds[:, :, tile == t].amax(-1) for t in range(int(tile[-1]) + 1)], dim=-1)
    return torch.log2(per.clamp_min(1e-38)).reshape(-1, per.shape[-1]).median(0).values.tolist()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["scores", "d_out"])
def test_ds_magnitudes_that_rise_and_fall_by_2_to_the_12(which, dtype):
    """One sequence of 129 keys, 2 heads, in which the largest |dS| of every own row arrives LAST, so that the fp16 accumulator is rescaled
    by 2^-3 or so at every streamed tile; the same rows in reversed order put it FIRST.
      "d_out" (the dK / dV pass streams queries): the rows of tile t of d_out carry the factor 2^(3 t - 10), t = 0 .. 4.
      "scores" (the dQ pass streams keys): a magnitude on the rows of V does NOT do it there -- delta_i = d_out_i . out_i is dominated by the
         large rows of V, so |dS| = P |dP - delta| is as large on the early keys as on the late ones -- so P itself rises: Q and K are halved,
         every query carries 4 in the head's first column and the keys of tile t carry 6 t ln 2 there, which adds 3 t ln 2 to their scores.
    The test asserts on the fp32 dS of the inputs that the median over the own rows of the per-tile largest |dS| rises (falls) from full
    tile to full tile and spans at least 2^9.  Both runs vs fp32 autograd at the bar of tests/test_gpu_encoder_train.py, and the two runs
    agree with each other (one reversed back) within that bar."""
    H, n = 2, 129
    case = att_inputs("packed", [n], H, dtype, seed=40 + (which == "scores"))
    tile = torch.arange(n, device="cuda") // 32
    if which == "scores":
        qkv = case["qkv"].float()
        qkv[:, :2 * H * 64] *= 0.5
        for h in range(H):
            qkv[:, h * 64] = 4.0
            qkv[:, H * 64 + h * 64] = 6 * math.log(2) * tile
        case["qkv"] = qkv.to(dtype)
    else:
        case["d_out"] = (case["d_out"].float() * torch.exp2(3.0 * tile - 10.0)[:, None]).to(dtype)
    for order, c in (("rising", case), ("falling", _flipped(case))):
        med = _ds_tile_medians(c, own_keys=which == "d_out")
        print(f"{which} {order} {str(dtype)[6:]}: median log2 of the per-tile largest |dS| {[round(m, 1) for m in med]}")
        steps = [b - a for a, b in zip(med[:3], med[1:4])]                                # between the four full tiles
        assert all(d > 1 for d in steps) if order == "rising" else all(d < -1 for d in steps), med
        assert max(med) - min(med) >= 9 and (med.index(min(med)) == 0 if order == "rising" else med.index(max(med)) == 0), med
    results = {}
    for order, c in (("rising", case), ("falling", _flipped(case))):
        ref, _ = att_reference(c, None)
        yard, _ = att_reference(c, dtype)
        got = run_att(c)[2].float()
        assert torch.isfinite(got).all()
        bars = []
        for part, label in enumerate(("dQ", "dK", "dV")):
            cols = slice(part * H * 64, (part + 1) * H * 64)
            bars.append(_bar_check(f"{which} {order} {str(dtype)[6:]} {label}", got[:, cols], ref[:, cols], yard[:, cols], dtype))
        results[order] = (got, bars)
    back = results["falling"][0].flip(0)
    for part, label in enumerate(("dQ", "dK", "dV")):
        cols = slice(part * H * 64, (part + 1) * H * 64)
        gap = (results["rising"][0][:, cols] - back[:, cols]).abs().max().item()
        bar = max(results["rising"][1][part], results["falling"][1][part])
        print(f"{which} {str(dtype)[6:]} {label}: rising vs falling max gap {gap:.3e}, bar {bar:.3e}")
        assert gap <= bar, (label, gap, bar)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_peaked_softmax_and_a_query_without_gradient(dtype):
    """qkv ~ 6 N(0, 1), lengths 33, 129, 300 (packed, 2 heads): near one-hot softmaxes, tiny gradients with a wide spread, at the bar of
    tests/test_gpu_encoder_train.py.  One query row per sequence has d_out = 0 in every head: all its dS are zero (the fp16 factor never
    finds an exponent) and its dQ must be exactly zero."""
    H, lens = 2, [33, 129, 300]
    case = att_inputs("packed", lens, H, dtype, seed=77)
    case["qkv"] = (case["qkv"].float() * 4).to(dtype)                                     # 1.5 N(0, 1) x 4
    dead = [case["starts"][0] + 7, case["starts"][1] + 128, case["starts"][2] + 150]
    case["d_out"][dead] = 0
    ref, lse_ref = att_reference(case, None)
    yard, _ = att_reference(case, dtype)
    out, lse, d_qkv = run_att(case)
    got = d_qkv.float()
    assert torch.isfinite(got).all()
    assert torch.allclose(lse, lse_ref, atol=2e-5, rtol=2e-5)
    for part, label in enumerate(("dQ", "dK", "dV")):
        cols = slice(part * H * 64, (part + 1) * H * 64)
        _bar_check(f"peaked {str(dtype)[6:]} {label}", got[:, cols], ref[:, cols], yard[:, cols], dtype)
    assert (ref[dead][:, :H * 64] == 0).all()
    assert (d_qkv[dead][:, :H * 64].view(torch.int16) == 0).all()                         # exactly (+)zero


# ------------------------------------------------------------------------------------------------------- 3. what the kernel writes
CANARY = 7.0


def _canary_run(dtype, starts, lens, pad_len, max_len, T, H=12):
    """ccr_attention_bwd_half through ctypes into a d_qkv filled with CANARY; the workspace has exactly the required size and sits in front of
    guard bytes.  Rows outside the live ranges hold NaN in every input.  -> (d_qkv, the live mask after the cut at max_len)."""
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    g = torch.Generator().manual_seed(sum(lens) + pad_len)
    qkv = (1.5 * torch.randn(T, 3 * H * 64, generator=g)).to(dtype)
    d_out = torch.randn(T, H * 64, generator=g).to(dtype)
    live = torch.zeros(T, dtype=torch.bool)
    for s, n in zip(starts, lens):
        live[s:s + min(n, max_len)] = True
    qkv[~live], d_out[~live] = float("nan"), float("nan")
    qkv, d_out, live = qkv.cuda(), d_out.cuda(), live.cuda()
    n_seq = len(lens)
    seq_start = torch.tensor(starts or [0], dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens or [0], dtype=torch.int32, device="cuda")
    p, st = ops._ptr, ops._stream(qkv)
    code = _lib.DTYPE_BF16 if dtype == torch.bfloat16 else _lib.DTYPE_F16
    out = torch.full((T, H * 64), float("nan"), dtype=dtype, device="cuda")
    lse = torch.full((T, H), float("nan"), dtype=torch.float32, device="cuda")
    if n_seq:
        _lib.check(lib.ccr_attention_fwd_train_half(p(qkv), p(seq_start), p(seq_len), p(out), p(lse), n_seq, H, max_len, pad_len, 0.125, code, st),
                   "ccr_attention_fwd_train_half")
        out[~live], lse[~live] = float("nan"), float("nan")
    need = int(lib.ccr_attention_bwd_workspace_bytes(n_seq, H, max_len))
    assert need == max(n_seq * H * ((max_len + 31) // 32 * 32) * 4, 4)
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    d_qkv = torch.full((T, 3 * H * 64), CANARY, dtype=dtype, device="cuda")
    _lib.check(lib.ccr_attention_bwd_half(p(qkv), p(out), p(lse), p(d_out), p(seq_start), p(seq_len), p(d_qkv), n_seq, H, max_len, pad_len, 0.125,
                                          code, p(ws), need, st), "ccr_attention_bwd_half")
    torch.cuda.synchronize()
    assert (ws[need:] == 0x5A).all()                       # nothing past the workspace's required size
    return dict(d_qkv=d_qkv, live=live, qkv=qkv, out=out, lse=lse, d_out=d_out, seq_start=seq_start, seq_len=seq_len)


def _expect_rows(d_qkv, live, zero, label):
    """Live rows: written (finite, not the canary in any (part, head) block).  `zero` rows: +0 everywhere.  Every other row: the canary."""
    T = d_qkv.shape[0]
    zero_mask = torch.zeros(T, dtype=torch.bool, device="cuda")
    for a, b in zero:
        zero_mask[a:b] = True
    assert not (zero_mask & live).any()
    assert torch.isfinite(d_qkv[live]).all(), label
    blocks = d_qkv[live].view(int(live.sum()), -1, 64)     # [rows, 3 * H, 64]: both passes' outputs, every head
    assert not (blocks == CANARY).all(dim=-1).any(), label
    assert (d_qkv[zero_mask].view(torch.int16) == 0).all(), label
    assert (d_qkv[~(zero_mask | live)] == CANARY).all(), label


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_attention_backward_writes_its_rows_and_no_others(dtype):
    """Lengths 1, 32, 33 and 0 at 12 heads, with rows between and after the sequences that belong to none.  Padded (pad_len 40): live rows
    written, rows len .. 39 of every sequence zero -- the empty one's too -- the gaps untouched.  Packed with holes: nothing but the live
    rows is written.  A seq_len beyond max_len: rows past the cut untouched, the rest bit-identical to the run with seq_len = max_len.
    n_seq = 0: nothing is written.  The workspace has exactly the required size throughout."""
    from ccrec_amd import ops
    starts, lens, T = [5, 50, 100, 150], [1, 32, 33, 0], 200
    run = _canary_run(dtype, starts, lens, pad_len=40, max_len=33, T=T)
    _expect_rows(run["d_qkv"], run["live"], [(s + n, s + 40) for s, n in zip(starts, lens)], "padded")
    via_ops = ops.attention_bwd(run["qkv"], run["out"], run["lse"], run["d_out"], run["seq_start"], run["seq_len"], 12, 33, 40)
    assert _same_bits(via_ops[run["live"]], run["d_qkv"][run["live"]])

    starts = [3, 4, 40, 90]                                # packed: 1 row at 3, 32 rows from 4, a hole 36 .. 39, 33 rows from 40, hole, empty
    run = _canary_run(dtype, starts, lens, pad_len=0, max_len=33, T=T)
    _expect_rows(run["d_qkv"], run["live"], [], "packed with holes")
    via_ops = ops.attention_bwd(run["qkv"], run["out"], run["lse"], run["d_out"], run["seq_start"], run["seq_len"], 12, 33, 0)
    assert _same_bits(via_ops[run["live"]], run["d_qkv"][run["live"]])

    cut = _canary_run(dtype, [2, 60], [40, 33], pad_len=0, max_len=33, T=100)      # the first sequence claims 40 rows, 33 are processed
    _expect_rows(cut["d_qkv"], cut["live"], [], "seq_len beyond max_len")
    assert int(cut["live"].sum()) == 66 and (cut["d_qkv"][35:60] == CANARY).all()
    honest = ops.attention_bwd(cut["qkv"], cut["out"], cut["lse"], cut["d_out"], cut["seq_start"], torch.full_like(cut["seq_len"], 33), 12, 33, 0)
    assert _same_bits(honest[cut["live"]], cut["d_qkv"][cut["live"]])

    none = _canary_run(dtype, [], [], pad_len=16, max_len=33, T=8)
    assert (none["d_qkv"] == CANARY).all()


# ------------------------------------------------------------------------------------------------------- 4. LayerNorm backward
def _ln_check(label, mine, ref, yard):
    """The bar of tests/test_gpu_encoder_train.py: max and mean error <= 2 x torch fp32's + 1e-6 max |ref|."""
    e_k, e_y = (mine.double() - ref).abs(), (yard.double() - ref).abs()
    floor = 1e-6 * ref.abs().max().item()
    assert mine.dtype == torch.float32 and torch.isfinite(mine).all()
    assert e_k.max().item() <= 2 * e_y.max().item() + floor, (label, e_k.max().item(), e_y.max().item(), floor)
    assert e_k.mean().item() <= 2 * e_y.mean().item() + floor, (label, e_k.mean().item(), e_y.mean().item(), floor)
    return e_k.max().item() / (2 * e_y.max().item() + floor), 2 * e_y.max().item() + floor


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_res", [True, False], ids=["residual", "no_residual"])
@pytest.mark.parametrize("C", range(1, 9))
def test_layernorm_backward_at_every_width(C, with_res, dtype):
    """dim = 256 C for every instantiated C, 7 rows (two workgroups, the second one short), against fp64 at the existing bar."""
    from ccrec_amd import ops
    rows, dim = 7, 256 * C
    x, res, gamma, d_y = ln_inputs(rows, dim, dtype, with_res, seed=rows + dim)
    v = x.float() if res is None else x.float() + res
    ref, yard = ln_torch_backward(v, gamma, d_y, torch.float64), ln_torch_backward(v, gamma, d_y, torch.float32)
    d_res, d_x, d_gamma, d_beta = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y)
    ratios = [_ln_check(label, mine, r, y)[0] for label, mine, r, y in zip(("d_res", "d_gamma", "d_beta"), (d_res, d_gamma, d_beta), ref, yard)]
    print(f"layernorm_bwd width {dim} {'res' if with_res else 'nores'} {str(dtype)[6:]}: max err / bar d_res {ratios[0]:.2f} d_gamma {ratios[1]:.2f} "
          f"d_beta {ratios[2]:.2f}")
    assert d_x.dtype == dtype and _same_bits(d_x, d_res.to(dtype))


LN_ROWS = [1, 2, 3, 4, 5, 9, 13, 17, 21, 25, 29,          # 1 .. 8 first-stage workgroups: every quartering of the second stage, empty parts included
           2047, 2048, 2049, 2051, 4100]                  # around and past the cap of 512 workgroups (rows > 2048: more than one row per wave)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_backward_at_every_launch_path(rows, dtype):
    """dim 256, d_y integers in [-8, 8]: d_beta must be the integer column sums BIT FOR BIT (fp32 adds of integers below 2^24 are exact in
    any order, so a dropped, doubled or mis-striped row shows in either stage); d_res and d_gamma against fp64 at the existing bar; and with
    the LAST row's d_y set to zero d_gamma changes by that row's fp64 contribution d_y xhat, to within the bar, d_beta by its d_y exactly."""
    from ccrec_amd import ops
    dim = 256
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, dim, generator=g).to(dtype).cuda()
    res = torch.randn(rows, dim, generator=g).cuda()
    gamma = (1.0 + 0.2 * torch.randn(dim, generator=g)).cuda()
    d_y = torch.randint(-8, 9, (rows, dim), generator=g).float().cuda()
    v = x.float() + res
    ref, yard = ln_torch_backward(v, gamma, d_y, torch.float64), ln_torch_backward(v, gamma, d_y, torch.float32)
    d_res, d_x, d_gamma, d_beta = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y)
    assert torch.equal(d_beta.double(), d_y.double().sum(0)), (rows, (d_beta.double() - d_y.double().sum(0)).abs().max().item())
    r_res, _ = _ln_check("d_res", d_res, ref[0], yard[0])
    r_gamma, bar = _ln_check("d_gamma", d_gamma, ref[1], yard[1])
    assert _same_bits(d_x, d_res.to(dtype))
    d_y0 = d_y.clone()
    d_y0[rows - 1] = 0
    _, _, d_gamma0, d_beta0 = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y0)
    vd = v[rows - 1].double()
    xhat = (vd - vd.mean()) / torch.sqrt(vd.var(unbiased=False) + LN_EPS)
    miss = ((d_gamma.double() - d_gamma0.double()) - d_y[rows - 1].double() * xhat).abs().max().item()
    print(f"layernorm_bwd {rows} rows {str(dtype)[6:]}: max err / bar d_res {r_res:.2f} d_gamma {r_gamma:.2f}; last row's share of d_gamma off by "
          f"{miss:.3e} (bar {bar:.3e})")
    assert miss <= bar, (rows, miss, bar)
    assert torch.equal(d_beta0.double(), d_y0.double().sum(0))
    if rows == 2051:      # the null-output combinations past the cap: what is asked for has the same bits
        for want in [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                     (True, False, True, True), (False, True, False, True)]:
            outs = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y, *want)
            for w, o, full in zip(want, outs, (d_res, d_x, d_gamma, d_beta)):
                assert (o is None) == (not w)
                assert not w or _same_bits(o, full)


# ------------------------------------------------------------------------------------------------------- 5. GELU backward
def _gelu_check(x, d_y, got, label):
    """|got - fp64| <= one spacing of the type at |ref| (fp16: at least its subnormal spacing 2^-24) + 1e-6 |d_y|: the bound of
    tests/test_gpu_encoder_train.py.  x, d_y finite."""
    dtype = x.dtype
    xd, dd = x.double(), d_y.double()
    ref = dd * (0.5 * (1 + torch.erf(xd / math.sqrt(2))) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi))
    exponent = torch.floor(torch.log2(ref.abs().clamp_min(1e-300)))
    floor_exp = -24.0 if dtype == torch.float16 else -126.0 - MANTISSA[dtype]
    one = torch.exp2(torch.clamp(exponent - MANTISSA[dtype], min=floor_exp))
    err = (got.double() - ref).abs()
    bad = ~(err <= one + 1e-6 * dd.abs())                  # (a NaN is bad)
    print(f"gelu_bwd {label} {str(dtype)[6:]}: {x.numel()} values, max err / spacing {(err / one).max().item():.3f}, violations {int(bad.sum())}")
    assert not bad.any(), (label, int(bad.sum()), x[bad][:4], d_y[bad][:4], got[bad][:4], ref[bad][:4])


GELU_SIZES = [8, 8 * 255, 8 * 256, 8 * 257, 8 * (256 * 4096 + 3)]      # one vector; around one workgroup; three vectors past 4096 full workgroups


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", GELU_SIZES)
def test_gelu_backward_at_every_launch_path(n, dtype):
    """x ~ 3 N(0, 1), d_y ~ N(0, 1) against fp64.  The last size runs the grid-stride loop: 4096 workgroups, three vectors in a second lap."""
    from ccrec_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    x = (3 * torch.randn(n, generator=g, device="cuda")).to(dtype)
    d_y = torch.randn(n, generator=g, device="cuda").to(dtype)
    guard = torch.full((n + 64,), CANARY, dtype=dtype, device="cuda")
    got = ops.gelu_bwd(x, d_y)
    assert got.dtype == dtype and got.shape == x.shape
    _gelu_check(x, d_y, got, f"n = {n}")
    # the same through the entry point into the middle of a canary-filled array: nothing before or after the n elements is written
    from ccrec_amd import _lib
    lib = ops.require_gpu()
    code = _lib.DTYPE_BF16 if dtype == torch.bfloat16 else _lib.DTYPE_F16
    inner = guard[32:32 + n]
    _lib.check(lib.ccr_gelu_bwd_half(ops._ptr(x), ops._ptr(d_y), ctypes.c_void_p(inner.data_ptr()), n, code, ops._stream(x)), "ccr_gelu_bwd_half")
    torch.cuda.synchronize()
    assert _same_bits(inner, got) and (guard[:32] == CANARY).all() and (guard[32 + n:] == CANARY).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gelu_backward_on_every_pattern_of_x(dtype):
    """All 65,536 patterns of x, each with d_y = 1, -3 and 2^-10.  Finite x: the fp64 bound.  x = +-inf and NaN: what torch's own GELU backward
    returns in the same type is all that is asked -- NaN where it returns NaN, and a zero of the same sign where it returns zero.  (Both
    return NaN at +-inf: inf x phi(inf) = inf x 0.)"""
    from ccrec_amd import ops
    x = torch.arange(65536, dtype=torch.int32, device="cuda").to(torch.int16).view(dtype)      # (wraps: every 16-bit pattern once)
    finite = torch.isfinite(x)
    assert int(finite.sum()) == (65536 - 2 * 128 if dtype == torch.bfloat16 else 65536 - 2 * 1024)
    for value in (1.0, -3.0, 2.0 ** -10):
        d_y = torch.full_like(x, value)
        got = ops.gelu_bwd(x, d_y)
        _gelu_check(x[finite], d_y[finite], got[finite], f"every pattern, d_y = {value}")
        xs = x.clone().requires_grad_(True)
        torch.nn.functional.gelu(xs).backward(d_y)
        theirs, mine = xs.grad[~finite], got[~finite]
        assert torch.equal(torch.isnan(mine), torch.isnan(theirs))
        zero = theirs == 0
        assert (mine[zero] == 0).all() and torch.equal(torch.signbit(mine[zero]), torch.signbit(theirs[zero]))
        at_inf = torch.isinf(x[~finite])
        print(f"gelu_bwd non-finite x {str(dtype)[6:]} d_y = {value}: torch returns NaN at {int(torch.isnan(theirs[at_inf]).sum())} of "
              f"{int(at_inf.sum())} infinities, the kernel at {int(torch.isnan(mine[at_inf]).sum())}")
