"""Training dropout from explicit keep bits on the GPU (csrc/ccr_dropout.hip and the DROP instantiations of the layer kernels), in both
16-bit operand types: the generator against its CPU restatement bit for bit, identity and exact-structure probes with hand-made masks,
random masks against fp64 with the dropout-free tests' bars, and one fine-tune step of the whole stack against a pure-torch restatement
that takes the masks dropout_ref rebuilds from the seeds the encoder drew.  The measured ratios are printed (pytest -s)."""
import contextlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, PKG  # noqa: F401
from helpers import ATT_CASES, DTYPES, LN_EPS, MANTISSA, att_inputs, ln_inputs, ln_torch_backward, run_att, spacing

pytestmark = pytest.mark.gpu

_IDS = ["bf16", "fp16"]


def _host_bits(t):
    return t.cpu().numpy().view(np.uint32)


def _bits32(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("dim", [256, 768, 2048])
@pytest.mark.parametrize("rows", [1, 5, 1031])
def test_row_wise_bits_equal_the_cpu_restatement(rows, dim):
    from ccrec_amd import dropout_ref, ops
    seed, stream = 0x9e3779b97f4a7c15 + rows, 4 * dim + 1
    for p in (0.1, 0.5):
        got = _host_bits(ops.dropout_bits_rows(rows, dim, seed, stream, p))
        assert got.shape == (rows, dim // 32)
        assert np.array_equal(got, dropout_ref.rows_bits(seed, stream, p, rows, dim)), (rows, dim, p)
    if rows == 1031 and dim == 2048:      # the largest case: the kept fraction is within 4 sigma of 1 - p_eff
        n, q = rows * dim, dropout_ref.p_eff(0.5)
        kept = int(dropout_ref.unpack_bits(got, dim).sum())
        print(f"row-wise bits {rows}x{dim} p=0.5: kept {kept / n:.6f}, expected {1 - q:.6f}, sigma {math.sqrt(q * (1 - q) / n):.2e}")
        assert abs(kept / n - (1 - q)) <= 4 * math.sqrt(q * (1 - q) / n)


GEN_LENS = [1, 31, 33, 64, 65, 257, 512]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("heads", [3, 12])
def test_attention_bits_equal_the_cpu_restatement_below_each_length(heads, p):
    """One packed launch over lengths 1 .. 512: keep_q and keep_k against dropout_ref on every (query, key) below the length."""
    from ccrec_amd import dropout_ref, ops
    starts = [sum(GEN_LENS[:i]) for i in range(len(GEN_LENS))]
    T, seed, stream = sum(GEN_LENS), 0xfedcba9876543210, 7 + heads
    seq_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(GEN_LENS, dtype=torch.int32, device="cuda")
    keep_q, keep_k = ops.dropout_bits_attention(seq_start, seq_len, T, heads, 512, seed, stream, p)
    assert keep_q.shape == keep_k.shape == (T, heads, 16)
    uq, uk = dropout_ref.unpack_bits(_host_bits(keep_q), 512), dropout_ref.unpack_bits(_host_bits(keep_k), 512)      # [T, H, 512]
    masks = dropout_ref.attention_mask(seed, stream, p, starts, GEN_LENS, heads)
    kept = total = 0
    for s, n, m in zip(starts, GEN_LENS, masks):
        assert np.array_equal(uq[s:s + n, :, :n].transpose(1, 0, 2), m), ("keep_q", n)       # [H, query, key]
        assert np.array_equal(uk[s:s + n, :, :n].transpose(1, 2, 0), m), ("keep_k", n)       # [key, H, query] -> [H, query, key]
        kept, total = kept + int(m.sum()), total + m.size
    q = dropout_ref.p_eff(p)
    print(f"attention bits H={heads} p={p}: kept {kept / total:.6f}, expected {1 - q:.6f}, sigma {math.sqrt(q * (1 - q) / total):.2e}")
    assert abs(kept / total - (1 - q)) <= 4 * math.sqrt(q * (1 - q) / total)
    # a second launch repeats the bits
    again_q, again_k = ops.dropout_bits_attention(seq_start, seq_len, T, heads, 512, seed, stream, p)
    assert torch.equal(again_q, keep_q) and torch.equal(again_k, keep_k)


def test_generator_writes_nothing_outside_its_arrays():
    from ccrec_amd import _lib, ops
    lib = ops._require_encoder_dropout()
    pad = 4096
    rows_buf = torch.full((5 * 8 + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    _lib.check(lib.ccr_dropout_bits_rows(ops._ptr(rows_buf), 5, 256, 3, 1, 0.1, ops._stream(rows_buf)))
    assert (rows_buf[40:] == 0x5a5a5a5a).all() and not (rows_buf[:40] == 0x5a5a5a5a).all()
    lens = [33, 65, 7]
    T, H, W = sum(lens), 3, 3
    seq_start = torch.tensor([0, 33, 98], dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    bufs = [torch.full((T * H * W + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for _ in range(2)]
    _lib.check(lib.ccr_dropout_bits_attention(ops._ptr(bufs[0]), ops._ptr(bufs[1]), ops._ptr(seq_start), ops._ptr(seq_len), T, 3, H, 65, 3, 1, 0.5,
                                              ops._stream(bufs[0])))
    for b in bufs:
        assert (b[T * H * W:] == 0x5a5a5a5a).all() and not (b[:T * H * W] == 0x5a5a5a5a).all()
    # a sequence that claims rows beyond n_tokens writes nothing there
    before = [b.clone() for b in bufs]
    for b in bufs:
        b[(T - 7) * H * W:] = 0x5a5a5a5a
    _lib.check(lib.ccr_dropout_bits_attention(ops._ptr(bufs[0]), ops._ptr(bufs[1]), ops._ptr(seq_start), ops._ptr(seq_len), T - 7, 3, H, 65, 3, 1, 0.5,
                                              ops._stream(bufs[0])))
    for b, was in zip(bufs, before):
        assert (b[(T - 7) * H * W:] == 0x5a5a5a5a).all() and torch.equal(b[:(T - 7) * H * W], was[:(T - 7) * H * W])


# --------------------------------------------------------------------------------------------------- attention: cases, masks, references
_CASES = {}


def _case(name, dtype):
    """Inputs of one helpers.ATT_CASES entry (the dropout-free tests' seeds), computed once and shared (never modified)."""
    key = (name, dtype)
    if key not in _CASES:
        kind, lens, H = ATT_CASES[name]
        case = att_inputs(kind, lens, H, dtype, seed=len(name) + 7 * H)
        case["T"], case["W"] = case["qkv"].shape[0], (case["max_len"] + 31) // 32
        _CASES[key] = case
    return _CASES[key]


def _ones_bits(case):
    return torch.full((case["T"], case["H"], case["W"]), -1, dtype=torch.int32, device="cuda")


def _run_drop(case, keep_q, keep_k, inv_keep, d_out=None):
    from ccrec_amd import ops
    out, lse = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"], case["pad_len"],
                                       keep_q=keep_q, inv_keep=inv_keep)
    out_nan = out.clone()
    out_nan[~case["live"]] = float("nan")                 # the backward must not read the forward's padding rows
    d_qkv = ops.attention_bwd(case["qkv"], out_nan, lse, case["d_out"] if d_out is None else d_out, case["seq_start"], case["seq_len"],
                              case["H"], case["max_len"], case["pad_len"], keep_q=keep_q, keep_k=keep_k, inv_keep=inv_keep)
    return out, lse, d_qkv


_MASKED = {}


def _masked_case(name, dtype, p):
    """The case with a random mask of probability p: device bits from the generator (checked against dropout_ref above), the unpacked
    per-sequence masks, the fp64 reference and the 16-bit yardstick of out and d_qkv -- computed once and shared."""
    from ccrec_amd import dropout_ref, ops
    key = (name, dtype, p)
    if key not in _MASKED:
        case = _case(name, dtype)
        seed, stream = 1234 + len(name), 3
        keep_q, keep_k = ops.dropout_bits_attention(case["seq_start"], case["seq_len"], case["T"], case["H"], case["max_len"], seed, stream, p)
        masks = [torch.from_numpy(m).cuda() for m in dropout_ref.attention_mask(seed, stream, p, case["starts"], case["lens"], case["H"])]
        inv_keep = dropout_ref.inv_keep(p)
        m = dict(keep_q=keep_q, keep_k=keep_k, masks=masks, inv_keep=inv_keep)
        m["ref"] = _att_reference_masked(case, masks, inv_keep, None)
        m["yard"] = _att_reference_masked(case, masks, inv_keep, dtype)
        _MASKED[key] = m
    return _MASKED[key]


def _att_reference_masked(case, masks, inv_keep, half):
    """helpers.att_reference with dropout: per (sequence, head) autograd of (softmax(Q K^T / 8) * M * inv_keep) V on the rounded operands.
    half None: everything fp64 (the reference).  half = a 16-bit type: the matmul operands and results are 16-bit, softmax and mask fp32
    -- autocast's arithmetic (the yardstick).  -> (out [T, H 64], d_qkv [T, 3 H 64]) fp64, zeros on padding rows."""
    qkv, d_out, H = case["qkv"], case["d_out"], case["H"]
    T = qkv.shape[0]
    grad = torch.zeros(T, 3 * H * 64, dtype=torch.float64, device=qkv.device)
    out = torch.zeros(T, H * 64, dtype=torch.float64, device=qkv.device)
    for s, ln, mask in zip(case["starts"], case["lens"], masks):
        if ln == 0:
            continue
        rows = qkv[s:s + ln].view(ln, 3, H, 64).permute(1, 2, 0, 3)          # [3, H, len, 64]
        dt = torch.float64 if half is None else half
        st = torch.float64 if half is None else torch.float32
        q, k, v = (rows[i].to(dt).detach().clone().requires_grad_(True) for i in range(3))
        scores = (q @ k.transpose(1, 2)).to(st) * 0.125
        p = torch.softmax(scores, dim=-1) * (mask.to(st) * inv_keep)
        o = p.to(dt) @ v
        do = d_out[s:s + ln].view(ln, H, 64).permute(1, 0, 2).to(dt)
        o.backward(do)
        g3 = torch.stack([q.grad, k.grad, v.grad]).double()                   # [3, H, len, 64]
        grad[s:s + ln] = g3.permute(2, 0, 1, 3).reshape(ln, 3 * H * 64)
        out[s:s + ln] = o.detach().double().permute(1, 0, 2).reshape(ln, H * 64)
    return out, grad


def _errors(mine, ref, yard):
    return ((mine - ref).abs().max().item(), (yard - ref).abs().max().item(), (mine - ref).abs().mean().item(), (yard - ref).abs().mean().item(),
            ref.abs().max().item())


# ----------------------------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", list(ATT_CASES))
def test_all_ones_bits_and_scale_one_are_the_dropout_free_attention(name, dtype):
    case = _case(name, dtype)
    out0, lse0, d0 = run_att(case)
    ones = _ones_bits(case)
    out, lse, d = _run_drop(case, ones, ones, 1.0)
    assert torch.equal(_bits32(out), _bits32(out0)) and torch.equal(_bits32(lse), _bits32(lse0)) and torch.equal(_bits32(d), _bits32(d0))


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("rows,dim", [(1, 256), (7, 768), (1031, 768), (4, 2048)] + [(7, 256 * C) for C in (2, 4, 5, 6, 7)])
def test_all_ones_bits_and_scale_one_are_the_dropout_free_layernorm_and_cast(rows, dim, dtype):
    from ccrec_amd import ops
    x, res, gamma, d_y = ln_inputs(rows, dim, dtype, True, seed=rows + dim)
    beta = torch.linspace(-1, 1, dim, device="cuda")
    ones = torch.full((rows, dim // 32), -1, dtype=torch.int32, device="cuda")
    for r in (res, None):
        want, got = ops.add_layernorm(x, r, gamma, beta, LN_EPS), ops.add_layernorm(x, r, gamma, beta, LN_EPS, keep_bits=ones, inv_keep=1.0)
        assert torch.equal(got[0], want[0]) and torch.equal(_bits32(got[1]), _bits32(want[1]))
        want, got = ops.add_layernorm_bwd(x, r, gamma, LN_EPS, d_y), ops.add_layernorm_bwd(x, r, gamma, LN_EPS, d_y, keep_bits=ones, inv_keep=1.0)
        for w, g in zip(want, got):
            assert (w is None) == (g is None)
            if w is not None:
                assert torch.equal(_bits32(g), _bits32(w))
    f32, b16 = ops.dropout_apply(res, ones, 1.0, dtype)
    assert torch.equal(_bits32(f32), _bits32(res)) and torch.equal(_bits32(b16), _bits32(res.to(dtype)))


def test_the_earlier_drop_names_are_the_keyword_form():
    """ops.*_drop (the spelling before each op became one function with optional bits) forward to the keyword form: the same bits out of
    both, at one small shape per op, random bits."""
    from ccrec_amd import dropout_ref, ops
    dtype, p = torch.bfloat16, 0.1
    inv = dropout_ref.inv_keep(p)
    case = _case("padded_edges", dtype)
    a = (case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"])
    kq, kk = ops.dropout_bits_attention(case["seq_start"], case["seq_len"], case["T"], case["H"], case["max_len"], 7, 3, p)
    out, lse = ops.attention_fwd_train(*a, case["pad_len"], keep_q=kq, inv_keep=inv)
    old = ops.attention_fwd_train_drop(*a, kq, inv, case["pad_len"])
    assert torch.equal(_bits32(old[0]), _bits32(out)) and torch.equal(_bits32(old[1]), _bits32(lse))
    out = torch.where(case["live"][:, None], out, torch.zeros_like(out))
    b = (case["qkv"], out, lse, case["d_out"], case["seq_start"], case["seq_len"], case["H"], case["max_len"])
    assert torch.equal(_bits32(ops.attention_bwd_drop(*b, kq, kk, inv, case["pad_len"])),
                       _bits32(ops.attention_bwd(*b, case["pad_len"], keep_q=kq, keep_k=kk, inv_keep=inv)))
    x, res, gamma, d_y = ln_inputs(7, 256, dtype, True, seed=5)
    beta = torch.linspace(-1, 1, 256, device="cuda")
    bits = ops.dropout_bits_rows(7, 256, 7, 4, p)
    pairs = list(zip(ops.add_layernorm_drop(x, bits, inv, res, gamma, beta, LN_EPS), ops.add_layernorm(x, res, gamma, beta, LN_EPS, keep_bits=bits, inv_keep=inv)))
    pairs += zip(ops.add_layernorm_bwd_drop(x, bits, inv, res, gamma, LN_EPS, d_y), ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y, keep_bits=bits, inv_keep=inv))
    g = torch.Generator().manual_seed(6)
    word, pos, typ = (torch.randn(n, 256, generator=g).cuda() for n in (50, 16, 2))
    ids, ps = (torch.randint(0, n, (7,), generator=g).cuda() for n in (50, 16))
    e = (word, pos, typ, ids, ps, None, gamma, beta, LN_EPS)
    pairs += zip(ops.embed_layernorm_drop(*e, keep_bits=bits, inv_keep=inv, dtype=dtype), ops.embed_layernorm(*e, dtype=dtype, keep_bits=bits, inv_keep=inv))
    pairs += zip(ops.embed_layernorm_drop(*e, dtype=dtype), ops.embed_layernorm(*e, dtype=dtype))
    assert len(pairs) == 10
    for was, now in pairs:
        assert torch.equal(_bits32(was), _bits32(now))


# ---------------------------------------------------------------------------------------------------------------------- exact structure
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["padded_edges", "packed_12_heads"])
def test_scale_two_doubles_the_output_exactly_and_leaves_lse(name, dtype):
    """All-ones bits, inv_keep = 2: a power of two commutes with every rounding, so out is exactly 2 x the dropout-free out wherever
    that stays in the type's normal range, and lse (of the undropped scores) keeps its bits."""
    from ccrec_amd import ops
    case = dict(_case(name, dtype))
    if dtype == torch.float16:
        # fp16's normal range ends at 6e-5: a probability below it is rounded on a fixed grid and does not double exactly.  Quarter the
        # queries and keys (a power of two: exact) so that every probability of these <= 200-token rows stays far above that.
        case["qkv"] = case["qkv"].clone()
        case["qkv"][:, :2 * case["H"] * 64] *= 0.25
    out0, lse0 = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"], case["pad_len"])
    ones = _ones_bits(case)
    out, lse = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"], case["pad_len"], keep_q=ones, inv_keep=2.0)
    assert torch.equal(_bits32(lse), _bits32(lse0))
    tiny = torch.finfo(dtype).tiny
    normal = (out0.float().abs() >= tiny) | (out0 == 0)
    assert normal.float().mean().item() > 0.99
    assert torch.equal(_bits32((out0.float() * 2).to(dtype))[normal], _bits32(out)[normal])
    assert (out[~case["live"]] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_a_fully_dropped_query_row_gives_exact_zeros(dtype):
    """Every bit of one query cleared (in keep_q's row and in the query's bit of every keep_k row): its out row and its dQ row are +0
    exactly and its lse is unchanged; the other rows of out keep the all-ones bits."""
    case = _case("padded_edges", dtype)
    H, W = case["H"], case["W"]
    ones = _ones_bits(case)
    out1, lse1, _ = _run_drop(case, ones, ones, 1.0)
    s, n = case["starts"][7], case["lens"][7]      # the 65-token sequence
    for q in (0, 33, 64):
        keep_q, keep_k = ones.clone(), ones.clone()
        keep_q[s + q] = 0
        keep_k[s:s + n, :, q >> 5] &= ~(1 << (q & 31)) if (q & 31) < 31 else 0x7fffffff
        out, lse, d_qkv = _run_drop(case, keep_q, keep_k, 1.0)
        assert (_bits32(out[s + q]) == 0).all() and (_bits32(d_qkv[s + q, :H * 64]) == 0).all()
        assert torch.equal(_bits32(lse), _bits32(lse1))
        others = torch.ones(case["T"], dtype=torch.bool, device="cuda")
        others[s + q] = False
        assert torch.equal(_bits32(out[others]), _bits32(out1[others]))
        assert torch.isfinite(d_qkv).all() and (d_qkv[~case["live"]] == 0).all()
    assert W == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["padded_edges", "padded_512_empty", "packed_blocks"])
def test_bits_beyond_the_length_change_no_output_bit(name, dtype):
    """Random bits at every position >= the sequence's length (and in rows of no sequence): out, lse and d_qkv keep their bits."""
    case = _case(name, dtype)
    m = _masked_case(name, dtype, 0.5)
    want = _run_drop(case, m["keep_q"], m["keep_k"], m["inv_keep"])
    g = torch.Generator().manual_seed(3)
    noise = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, case["T"], case["H"], case["W"] * 32 // 32), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    valid = torch.zeros(case["T"], case["W"] * 32, dtype=torch.bool, device="cuda")      # (token row, position) below the length
    for s, n in zip(case["starts"], case["lens"]):
        valid[s:s + n, :n] = True
    weights = (1 << torch.arange(32, dtype=torch.int64, device="cuda"))
    vmask = (valid.view(case["T"], case["W"], 32).long() * weights).sum(-1)
    vmask = torch.where(vmask >= 2 ** 31, vmask - 2 ** 32, vmask).to(torch.int32)[:, None, :]      # 1 = a meaningful bit
    dirty_q = (m["keep_q"] & vmask) | (noise[0] & ~vmask)
    dirty_k = (m["keep_k"] & vmask) | (noise[1] & ~vmask)
    assert not torch.equal(dirty_q, m["keep_q"])
    got = _run_drop(case, dirty_q, dirty_k, m["inv_keep"])
    for w, g_ in zip(want, got):
        assert torch.equal(_bits32(w), _bits32(g_))


def test_canaries_behind_the_gradient_and_the_workspace_survive():
    from ccrec_amd import _lib, ops
    lib = ops._require_encoder_dropout()
    dtype = torch.bfloat16
    case = _case("packed_12_heads", dtype)
    m = _masked_case("packed_12_heads", dtype, 0.1)
    H, T, n_seq = case["H"], case["T"], len(case["lens"])
    out, lse = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], H, case["max_len"], keep_q=m["keep_q"], inv_keep=m["inv_keep"])
    need = lib.ccr_attention_bwd_workspace_bytes(n_seq, H, case["max_len"])
    pad = 4096
    ws = torch.full((need + pad,), 0x5a, dtype=torch.uint8, device="cuda")
    d_buf = torch.full((T * 3 * H * 64 + pad,), 7.0, dtype=dtype, device="cuda")
    p = ops._ptr
    _lib.check(lib.ccr_attention_bwd_drop_half(p(case["qkv"]), p(out), p(lse), p(case["d_out"]), p(case["seq_start"]), p(case["seq_len"]),
                                               p(m["keep_q"]), p(m["keep_k"]), m["inv_keep"], p(d_buf), n_seq, H, case["max_len"], 0, 0.125,
                                               _lib.DTYPE_BF16, p(ws), need, ops._stream(ws)))
    assert (ws[need:] == 0x5a).all() and (d_buf[T * 3 * H * 64:] == 7).all()
    want = ops.attention_bwd(case["qkv"], out, lse, case["d_out"], case["seq_start"], case["seq_len"], H, case["max_len"], keep_q=m["keep_q"],
                             keep_k=m["keep_k"], inv_keep=m["inv_keep"])
    assert torch.equal(_bits32(d_buf[:T * 3 * H * 64].view(T, 3 * H * 64)), _bits32(want))
    # bad arguments launch nothing
    d_buf.fill_(7.0)
    assert lib.ccr_attention_bwd_drop_half(p(case["qkv"]), p(out), p(lse), p(case["d_out"]), p(case["seq_start"]), p(case["seq_len"]), p(m["keep_q"]),
                                           None, m["inv_keep"], p(d_buf), n_seq, H, case["max_len"], 0, 0.125, _lib.DTYPE_BF16, p(ws), need,
                                           ops._stream(ws)) == _lib.CCR_ERR_INVALID
    assert lib.ccr_attention_bwd_drop_half(p(case["qkv"]), p(out), p(lse), p(case["d_out"]), p(case["seq_start"]), p(case["seq_len"]), p(m["keep_q"]),
                                           p(m["keep_k"]), m["inv_keep"], p(d_buf), n_seq, H, case["max_len"], 0, 0.125, _lib.DTYPE_BF16, p(ws),
                                           need - 1, ops._stream(ws)) == _lib.CCR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (d_buf == 7).all()


# ------------------------------------------------------------------------------------------------------------ random masks against fp64
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", list(ATT_CASES))
def test_attention_with_random_masks_is_as_close_to_fp64_as_the_16_bit_torch_path(name, dtype, p):
    """out, dQ, dK, dV vs fp64 autograd of (softmax(S) * M * inv_keep) V with the same unpacked mask: max |err| and mean |err| at most
    1.5 x those of the same formula with 16-bit matmuls and an fp32 softmax; the max has a floor of one spacing of the type at max |ref|
    (the bars of test_gpu_encoder_train.py)."""
    case, m = _case(name, dtype), _masked_case(name, dtype, p)
    H, live = case["H"], case["live"]
    out, lse, d_qkv = _run_drop(case, m["keep_q"], m["keep_k"], m["inv_keep"])
    assert torch.isfinite(d_qkv).all() and torch.isfinite(out).all() and (d_qkv[~live] == 0).all() and (out[~live] == 0).all()
    pieces = [("out", out.double()[live], m["ref"][0][live], m["yard"][0][live])]
    for part, label in enumerate(("dQ", "dK", "dV")):
        cols = slice(part * H * 64, (part + 1) * H * 64)
        pieces.append((label, d_qkv.double()[live][:, cols], m["ref"][1][live][:, cols], m["yard"][1][live][:, cols]))
    for label, mine, ref, yard in pieces:
        k_max, y_max, k_mean, y_mean, ref_max = _errors(mine, ref, yard)
        print(f"attention_drop {name} {str(dtype)[6:]} p={p} {label}: max err/max ref kernel {k_max / ref_max:.3e} torch {y_max / ref_max:.3e} "
              f"(ratio {k_max / max(y_max, 1e-30):.2f}); mean err kernel {k_mean:.3e} torch {y_mean:.3e} (ratio {k_mean / max(y_mean, 1e-30):.2f})")
        assert k_max <= max(1.5 * y_max, spacing(ref_max, dtype)), (label, k_max, y_max, ref_max)
        assert k_mean <= 1.5 * y_mean, (label, k_mean, y_mean)
    again = _run_drop(case, m["keep_q"], m["keep_k"], m["inv_keep"])
    assert torch.equal(_bits32(again[2]), _bits32(d_qkv)) and torch.equal(_bits32(again[0]), _bits32(out))


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_one_flipped_bit_of_keep_k_alone_fails_the_comparison(dtype):
    """The two views must agree: with ONE bit of keep_k flipped (keep_q untouched) on the 65-token sequence, dK or dV moves away from the
    fp64 reference by more than the bar of the test above.  The bit is the (query, key) of head 0 with the largest probability."""
    case, m = _case("padded_edges", dtype), _masked_case("padded_edges", dtype, 0.5)
    H, live = case["H"], case["live"]
    s, n = case["starts"][7], case["lens"][7]
    rows = case["qkv"][s:s + n].view(n, 3, H, 64).double()
    prob = torch.softmax(rows[:, 0, 0] @ rows[:, 1, 0].T * 0.125, dim=-1) * case["d_out"][s:s + n, :64].double().abs().amax(1, keepdim=True)
    q, k = divmod(int(prob.argmax()), n)
    keep_k = m["keep_k"].clone()
    keep_k[s + k, 0, q >> 5] ^= (1 << (q & 31)) if (q & 31) < 31 else -2 ** 31
    _, _, d_qkv = _run_drop(case, m["keep_q"], keep_k, m["inv_keep"])
    moved = False
    for part, label in ((1, "dK"), (2, "dV")):
        cols = slice(part * H * 64, (part + 1) * H * 64)
        k_max, y_max, _, _, ref_max = _errors(d_qkv.double()[live][:, cols], m["ref"][1][live][:, cols], m["yard"][1][live][:, cols])
        print(f"one flipped keep_k bit {str(dtype)[6:]} {label}: max err {k_max:.3e}, bar {max(1.5 * y_max, spacing(ref_max, dtype)):.3e}")
        moved |= k_max > max(1.5 * y_max, spacing(ref_max, dtype))
    assert moved


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,dim", [(1, 256), (7, 256), (1031, 256), (1, 768), (7, 768), (1031, 768)] + [(7, 256 * C) for C in (2, 4, 5, 6, 7, 8)])
def test_layernorm_with_bits_against_fp64(rows, dim, p, dtype):
    """d_res, d_x, d_gamma, d_beta of LayerNorm(x * M * inv_keep + residual) vs fp64 torch: at most 2 x the error of torch's fp32 path
    (the same formula in fp32, F.layer_norm backward; d_x rounded to the type), floor 1e-6 max |ref| -- test_gpu_encoder_train.py's bar.
    The forward's two outputs against the same fp64 reference under the same bar."""
    from ccrec_amd import dropout_ref, ops
    x, res, gamma, d_y = ln_inputs(rows, dim, dtype, True, seed=rows + dim)
    beta = torch.linspace(-1, 1, dim, device="cuda")
    seed, stream = 99 + rows, 6
    bits = ops.dropout_bits_rows(rows, dim, seed, stream, p)
    mask = torch.from_numpy(dropout_ref.rows_mask(seed, stream, p, rows, dim)).cuda()
    inv_keep = dropout_ref.inv_keep(p)
    m64, m32 = mask.double() * inv_keep, mask.float() * inv_keep
    v64, v32 = x.double() * m64 + res.double(), x.float() * m32 + res
    ref = ln_torch_backward(v64, gamma, d_y, torch.float64)
    yard = ln_torch_backward(v32, gamma, d_y, torch.float32)
    d_res, d_x, d_gamma, d_beta = ops.add_layernorm_bwd(x, res, gamma, LN_EPS, d_y, keep_bits=bits, inv_keep=inv_keep)
    pieces = [("d_res", d_res, ref[0], yard[0]), ("d_x", d_x, ref[0] * m64, (yard[0] * m32).to(dtype)), ("d_gamma", d_gamma, ref[1], yard[1]),
              ("d_beta", d_beta, ref[2], yard[2])]
    y64 = F.layer_norm(v64, (dim,), gamma.double(), beta.double(), LN_EPS)
    y32 = F.layer_norm(v32, (dim,), gamma, beta, LN_EPS)
    f32, b16 = ops.add_layernorm(x, res, gamma, beta, LN_EPS, keep_bits=bits, inv_keep=inv_keep)
    pieces += [("y_f32", f32, y64, y32), ("y_half", b16, y64, y32.to(dtype))]
    for label, mine, r, y in pieces:
        assert torch.isfinite(mine).all()
        e_k, e_y = (mine.double() - r).abs(), (y.double() - r).abs()
        floor = 1e-6 * r.abs().max().item()
        print(f"layernorm_drop {rows}x{dim} p={p} {str(dtype)[6:]} {label}: max err kernel {e_k.max().item():.3e} torch {e_y.max().item():.3e}; "
              f"mean err kernel {e_k.mean().item():.3e} torch {e_y.mean().item():.3e}")
        assert e_k.max().item() <= 2 * e_y.max().item() + floor, (label, e_k.max().item(), e_y.max().item(), floor)
        assert e_k.mean().item() <= 2 * e_y.mean().item() + floor, (label, e_k.mean().item(), e_y.mean().item(), floor)
    assert d_x.dtype == dtype and torch.equal(_bits32(d_x), _bits32((d_res * m32).to(dtype)))
    assert (d_x[~mask] == 0).all()
    # the embeddings' site: x * M * inv_keep exactly (one fp32 product), its 16-bit copy rounded once
    a32, a16 = ops.dropout_apply(res, bits, inv_keep, dtype)
    assert torch.equal(_bits32(a32), _bits32(res * m32)) and torch.equal(_bits32(a16), _bits32((res * m32).to(dtype)))


# ------------------------------------------------------------------------------------------------------------------- whole layer stack
def _tiny_model(kind, dropout=0.0, seed=0):
    """test_gpu_encoder_train._tiny_model: a 2-layer BERT / DistilBERT, hidden 256, 4 heads, with widened attention projections."""
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
HEADS, HIDDEN = 4, 256


def _stack_batch():
    g = torch.Generator().manual_seed(11)
    L = max(STACK_LENS)
    ids = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    mask = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    for r, n in enumerate(STACK_LENS):
        ids[r, :n] = torch.randint(1, 600, (n,), generator=g)
        mask[r, :n] = 1
    return ids.cuda(), mask.cuda()


def _restate(model, ids, mask, seed=None, cls_only=False):
    """The layer stack in plain torch (fp32, or autocast's arithmetic inside an autocast context) -> last hidden state [B, L, hidden]
    with zeros on padding (cls_only: [B, 1, hidden]).  seed None: no dropout.  Otherwise every site multiplies by the mask dropout_ref
    rebuilds from (seed, the site's stream id, the site module's p) for the token rows FusedBertEncoder.forward_train uses: a packed
    array when more than a tenth of the batch is padding, else the padded [B, L] batch."""
    from ccrec_amd import dropout_ref, fused_bert
    bert = type(model).__name__ == "BertModel"
    e = model.embeddings
    layers = list(model.encoder.layer if bert else model.transformer.layer)
    B, L = ids.shape
    lens = mask.sum(1).tolist()
    packed = sum(lens) < 0.9 * B * L
    starts = [sum(lens[:b]) for b in range(B)] if packed else [b * L for b in range(B)]
    T = sum(lens) if packed else B * L
    flat = torch.cat([torch.arange(L, device=ids.device)[:n] + b * L for b, n in enumerate(lens)])      # real tokens in the [B, L] batch
    rows = torch.cat([torch.arange(n, device=ids.device) + s for s, n in zip(starts, lens)])            # ... and their kernel token rows
    own = [sum(lens[:b]) for b in range(B)]                                                              # ... and in this function's arrays

    def row_mask(module, stream, n_rows, pick):
        if seed is None or module is None or module.p <= 0:
            return None
        m = torch.from_numpy(dropout_ref.rows_mask(seed, stream, module.p, n_rows, HIDDEN)).to(ids.device)[pick]
        return m.float() * dropout_ref.inv_keep(module.p)

    x = e.word_embeddings(ids.flatten()[flat])
    if bert:
        x = x + e.token_type_embeddings(torch.zeros_like(flat))
    x = x + e.position_embeddings(flat % L)
    h = F.layer_norm(x.float(), (HIDDEN,), e.LayerNorm.weight, e.LayerNorm.bias, e.LayerNorm.eps)
    m = row_mask(e.dropout, fused_bert.EMBEDDINGS_STREAM, T, rows)
    if m is not None:
        h = h * m
    for i, mod in enumerate(layers):
        if bert:
            q, k, v, so, ln1, ff, out, ln2 = (mod.attention.self.query, mod.attention.self.key, mod.attention.self.value, mod.attention.output.dense,
                                              mod.attention.output.LayerNorm, mod.intermediate.dense, mod.output.dense, mod.output.LayerNorm)
            d_prob, d_attn, d_ffn = mod.attention.self.dropout, mod.attention.output.dropout, mod.output.dropout
        else:
            q, k, v, so, ln1, ff, out, ln2 = (mod.attention.q_lin, mod.attention.k_lin, mod.attention.v_lin, mod.attention.out_lin,
                                              mod.sa_layer_norm, mod.ffn.lin1, mod.ffn.lin2, mod.output_layer_norm)
            d_prob, d_attn, d_ffn = mod.attention.dropout, None, mod.ffn.dropout
        Q, K, V = q(h), k(h), v(h)
        amasks = None
        if seed is not None and d_prob.p > 0:
            amasks = dropout_ref.attention_mask(seed, fused_bert.dropout_stream(i, fused_bert.SITE_PROBABILITIES), d_prob.p, starts, lens, HEADS)
        ctx = []
        for b, n in enumerate(lens):
            sl = slice(own[b], own[b] + n)
            qs, ks, vs = (t[sl].view(n, HEADS, 64).transpose(0, 1) for t in (Q, K, V))
            prob = torch.softmax((qs @ ks.transpose(1, 2)) * 0.125, dim=-1)
            if amasks is not None:
                prob = prob * (torch.from_numpy(amasks[b]).to(ids.device).float() * dropout_ref.inv_keep(d_prob.p))
            ctx.append((prob.to(vs.dtype) @ vs).transpose(0, 1).reshape(n, HIDDEN))
        ctx = torch.cat(ctx)
        li, n_rows, pick = i, T, rows
        if cls_only and i == len(layers) - 1:      # the last layer runs on the first tokens' rows only: one row per sequence, own streams
            first = torch.tensor(own, device=ids.device)
            ctx, h = ctx[first], h[first]
            li, n_rows, pick = len(layers), B, torch.arange(B, device=ids.device)
        a = so(ctx)
        m = row_mask(d_attn, fused_bert.dropout_stream(li, fused_bert.SITE_ATTENTION_OUTPUT), n_rows, pick)
        h = F.layer_norm((a * m if m is not None else a) + h, (HIDDEN,), ln1.weight, ln1.bias, ln1.eps)
        f = out(F.gelu(ff(h)))
        m = row_mask(d_ffn, fused_bert.dropout_stream(li, fused_bert.SITE_FFN_OUTPUT), n_rows, pick)
        h = F.layer_norm((f * m if m is not None else f) + h, (HIDDEN,), ln2.weight, ln2.bias, ln2.eps)
    h = h.float()
    if cls_only:
        return h.view(B, 1, HIDDEN)
    return torch.zeros(B * L, HIDDEN, device=ids.device).index_copy(0, flat, h).view(B, L, HIDDEN)


def _step_loss(tower, ids, mask, autocast_dtype):
    """One MultipleNrlStep loss (three tower forwards with gradients on: queries, positives, hard negatives) over the nine texts."""
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


@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_the_restatement_is_the_module_in_eval_mode(kind):
    """The reference of the test below, pinned to transformers' own module first: without dropout its hidden states are the module's
    fp32 forward to fp32 rounding: 32 fp32 spacings (32 x 2^-23 = 3.8e-6) of the largest hidden state, a few times the 0.5e-6 / 1.2e-6 that
    two layers of fp32 sums in another order were measured to leave.  The measured figure is printed."""
    model = _tiny_model(kind, dropout=0.1).eval()
    ids, mask = _stack_batch()
    with torch.no_grad():
        want = model(input_ids=ids, attention_mask=mask).last_hidden_state
        got = _restate(model, ids, mask)
        cls = _restate(model, ids, mask, cls_only=True)
    live = mask.bool()
    err = (got[live] - want[live]).abs().max().item()
    print(f"restatement vs module ({kind}, eval, fp32): max |diff| {err:.2e}, max |hidden| {want[live].abs().max().item():.2f}")
    assert err <= 32 * 2.0 ** -23 * want[live].abs().max().item()
    assert (cls[:, 0] - want[:, 0]).abs().max().item() <= 32 * 2.0 ** -23 * want[live].abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_fine_tune_step_with_dropout_through_the_layer_kernels(kind, dtype, monkeypatch):
    """One MultipleNrlStep of a train() tower with dropout 0.1 under autocast, both opt-ins set, torch.manual_seed(s): every parameter's
    gradient against the fp32 restatement fed the masks of the seeds the encoder drew; yardstick = the restatement under the same
    autocast.  Per parameter: relative L2 <= max(1.5 x the yardstick's, 2^-8 bf16 / 2^-11 fp16), cosine >= the yardstick's - 1e-3 (the
    bars of test_gpu_encoder_train.py).  The same seed repeats loss and gradients bit for bit, another seed moves the loss; with the new
    variable unset the module trains; in eval() both variables give the dropout-free path's bits."""
    from ccrec_amd import fused_bert, ops
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    model = _tiny_model(kind, dropout=0.1)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()
    ids, mask = _stack_batch()
    calls, seeds = [], []
    real_att, real_seed = ops.attention_train, fused_bert.draw_seed
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (calls.append(k.get("keep_bits") is not None), real_att(*a, **k))[1])
    monkeypatch.setattr(fused_bert, "draw_seed", lambda: (seeds.append(real_seed()), seeds[-1])[1])
    variance = []      # per attention backward call: the modelled variance of the key bias's rounding residue (see the key-bias branch below)
    real_bwd = ops.attention_bwd
    ebits = MANTISSA[dtype]

    def bwd_spy(qkv, out, lse, d_out, seq_start, seq_len, n_heads, max_len, pad_len=0, scale=0.125, keep_q=None, keep_k=None, inv_keep=1.0):
        T = qkv.shape[0]
        q2 = qkv[:, :n_heads * 64].double().view(T, n_heads, 64).pow(2).sum(-1)                       # ||Q_qh||^2
        vmax = qkv[:, 2 * n_heads * 64:].double().view(T, n_heads, 64).abs().amax(0)                  # max_k |V_khd| (over all rows: an upper estimate)
        o = out.double().view(T, n_heads, 64).abs()
        ulp = torch.where(o > 0, torch.exp2(torch.floor(torch.log2(o.clamp_min(1e-300))) - ebits), torch.zeros_like(o))   # spacing of the stored O
        var_o = ulp.pow(2) / 12 + (2.0 ** -ebits * inv_keep * vmax).pow(2) / 12                          # O's own rounding + its P m operands'
        var_r = (d_out.double().view(T, n_heads, 64).pow(2) * var_o).sum(-1)                            # of dO . (O_stored - O)
        variance.append((scale ** 2 * (q2 * var_r).sum()).item())
        return real_bwd(qkv, out, lse, d_out, seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q, keep_k, inv_keep)

    monkeypatch.setattr(ops, "attention_bwd", bwd_spy)

    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", raising=False)
    assert "dropout" in fused_bert.train_unsupported_reason(model)
    assert torch.isfinite(_step_loss(tower, ids, mask, dtype)) and not calls and not seeds      # the new variable is unset: the module trained

    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")
    assert fused_bert.train_unsupported_reason(model) is None
    torch.manual_seed(123)
    loss_k, g_k = _grads(tower, ids, mask, dtype)
    residue_bound = 4 * math.sqrt(sum(variance))
    assert len(variance) == 6 and calls == [True] * 6 and len(seeds) == 3 and len(set(seeds)) == 3       # three tower forwards x two layers, one seed per forward
    assert fused_bert.for_model(model).last_seed == seeds[-1]
    drawn = list(seeds)
    torch.manual_seed(123)
    loss_again, g_again = _grads(tower, ids, mask, dtype)
    assert seeds[3:] == drawn and loss_again == loss_k and set(g_again) == set(g_k)
    assert all(torch.equal(g_again[n], g_k[n]) for n in g_k)
    torch.manual_seed(124)
    loss_other, _ = _grads(tower, ids, mask, dtype)
    assert loss_other != loss_k and seeds[6:] != drawn

    # the restatement, fed the masks of the three seeds of the first step, in the tower's place
    turn = []
    monkeypatch.setattr(tower, "_encode", lambda inputs, cls_only=False: (turn.append(1), _restate(model, inputs["input_ids"], inputs["attention_mask"],
                                                                                                  drawn[len(turn) - 1]))[1])
    loss32, g32 = _grads(tower, ids, mask, None)
    del turn[:]
    loss_m, g_m = _grads(tower, ids, mask, dtype)
    monkeypatch.undo()
    pooler = {n for n in g32 if n.startswith("pooler.")}
    assert set(g_k) == set(g32) - pooler == set(g_m) - pooler
    floor = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    worst = (0.0, None)
    for name in sorted(g_k):
        ref = g32[name].double()
        assert torch.isfinite(g_k[name]).all() and g_k[name].dtype == torch.float32
        if name.endswith(_KEY_BIAS):
            # Softmax is invariant to the shift the key bias adds to a query's row, with or without a mask on the probabilities: the
            # gradient is identically zero (sum_k dS_qk = sum_k P_k m_k dP_k - Delta_q = 0) and what any path returns is a rounding residue;
            # there is no direction to compare, and the relative-L2 bar has no meaning against a zero reference.  The dropout-free test holds
            # this residue under max(1.5 x the module's, floor x the query bias's gradient); its module runs a fused attention that takes
            # Delta = dO . O from a 16-bit O just as the kernels do.  The yardstick HERE is a restatement whose softmax backward forms
            # sum_k P_k m_k dP_k itself, so it lacks the one term that dominates the kernels' residue and 1.5 x it says nothing about that
            # term; the issue prescribes Delta = dO . O of the stored output.  What is asserted instead is the size that term must have
            # from the number format alone, at 4 sigma.  r_q = sum_k dS_qk = dO_q . (O_stored - O)_q, where each component of O_stored
            # carries its own rounding (uniform within half a spacing: variance ulp(O_d)^2 / 12) and those of its 16-bit P m operands
            # (at most (2^-e inv_keep max_k |V_kd|)^2 / 12 when one key holds the probability, as these widened projections make it);
            # d b_k = scale sum_q r_q Q_q sums independent errors, so E ||d b_k||^2 = scale^2 sum_{q,h} ||Q_qh||^2 Var r_qh, summed by
            # the spy over all six backward calls (both layers together: sqrt 2 too wide for one).  A mask that disagreed between the
            # passes would leave sum_k dS_qk of the order of P dP itself, 2^e times this.
            scale = g32[name.replace("key.bias", "query.bias").replace("k_lin.bias", "q_lin.bias")].double().norm().item()
            print(f"key-bias residue {name}: kernels {g_k[name].double().norm().item():.3e}, restatement under autocast "
                  f"{g_m[name].double().norm().item():.3e}, 4 sigma of the modelled residue {residue_bound:.3e}, floor x query-bias gradient "
                  f"{floor * scale:.3e}")
            assert g_k[name].double().norm().item() <= max(1.5 * g_m[name].double().norm().item(), residue_bound), (name, g_k[name].norm().item(), residue_bound)
            assert ref.norm().item() <= 1e-3 * scale, (name, ref.norm().item(), scale)
            continue
        rel_k = ((g_k[name].double() - ref).norm() / ref.norm()).item()
        rel_m = ((g_m[name].double() - ref).norm() / ref.norm()).item()
        cos_k = F.cosine_similarity(g_k[name].double().flatten(), ref.flatten(), dim=0).item()
        cos_m = F.cosine_similarity(g_m[name].double().flatten(), ref.flatten(), dim=0).item()
        worst = max(worst, (rel_k / max(rel_m, floor), name))
        assert rel_k <= max(1.5 * rel_m, floor), (name, rel_k, rel_m)
        assert cos_k >= cos_m - 1e-3, (name, cos_k, cos_m)
    print(f"fine-tune step with dropout {kind} {str(dtype)[6:]}: loss restatement fp32 {loss32:.6f} autocast {loss_m:.6f} kernels {loss_k:.6f}; "
          f"worst relative-L2 ratio kernel / max(restatement under autocast, floor) {worst[0]:.2f} ({worst[1]})")
    assert abs(loss_k - loss32) <= max(1.5 * abs(loss_m - loss32), spacing(loss32, dtype)), (loss_k, loss_m, loss32)

    # eval(): dropout is inactive, both variables set give the bits of the dropout-free path
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    tower.eval()
    loss_dry, g_dry = _grads(tower, ids, mask, dtype)
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")
    loss_both, g_both = _grads(tower, ids, mask, dtype)
    assert loss_both == loss_dry and all(torch.equal(g_both[n], g_dry[n]) for n in g_dry)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_cls_only_forward_with_dropout(kind, dtype, monkeypatch):
    """forward_train(cls_only=True) in train() with dropout: the last layer draws its row-wise bits for the one row per sequence it runs
    on (its own stream ids).  Against the fp32 restatement with the same masks: max |err| <= max(1.5 x the restatement's under autocast,
    one spacing of the type at max |ref|); the same seed repeats the bits."""
    from ccrec_amd import fused_bert
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")
    model = _tiny_model(kind, dropout=0.1).train()
    ids, mask = _stack_batch()
    enc = fused_bert.for_model(model)
    lengths = mask.sum(1).to(torch.int32)
    with torch.no_grad():
        torch.manual_seed(9)
        got = enc.forward_train(ids, lengths, cls_only=True, dtype=dtype)
        seed = enc.last_seed
        torch.manual_seed(9)
        again = enc.forward_train(ids, lengths, cls_only=True, dtype=dtype)
        assert enc.last_seed == seed and torch.equal(got, again) and got.shape == (len(STACK_LENS), 1, HIDDEN)
        ref = _restate(model, ids, mask, seed, cls_only=True)
        with torch.autocast("cuda", dtype=dtype):
            yard = _restate(model, ids, mask, seed, cls_only=True)
        full = enc.forward_train(ids, lengths, cls_only=False, dtype=dtype)      # (another seed: only the shape and the padding are checked)
    assert full.shape == (len(STACK_LENS), max(STACK_LENS), HIDDEN) and (full[~mask.bool()] == 0).all()
    e_k, e_y, ref_max = (got - ref).abs().max().item(), (yard - ref).abs().max().item(), ref.abs().max().item()
    print(f"cls_only with dropout {kind} {str(dtype)[6:]}: max err kernels {e_k:.3e} restatement under autocast {e_y:.3e}, max |ref| {ref_max:.2f}")
    assert e_k <= max(1.5 * e_y, spacing(ref_max, dtype)), (e_k, e_y)


PADDED_LENS = [64, 63, 64, 60, 64]      # 315 of 320 tokens: forward_train keeps the padded [B, L] batch (pad_len = L)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_near_full_batch_takes_the_padded_branch_with_dropout(kind, dtype, monkeypatch):
    """Less than a tenth of the batch is padding, so forward_train runs the layers on all B x L rows (seq_start = b L, pad_len = L): the
    padding rows get row-wise bits too and the attention bit arrays keep zero words on them.  Hidden states of the real tokens and the
    gradient of their sum against the fp32 restatement with the same masks (token row = b L + t): max |err| <= max(1.5 x the restatement's
    under autocast, one spacing of the type at max |ref|); padding rows of a padded forward carry no gradient into the parameters."""
    from ccrec_amd import fused_bert, ops
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")
    model = _tiny_model(kind, dropout=0.1).train()
    g = torch.Generator().manual_seed(13)
    L = max(PADDED_LENS)
    ids = torch.zeros(len(PADDED_LENS), L, dtype=torch.int64)
    mask = torch.zeros(len(PADDED_LENS), L, dtype=torch.int64)
    for r, n in enumerate(PADDED_LENS):
        ids[r, :n] = torch.randint(1, 600, (n,), generator=g)
        mask[r, :n] = 1
    ids, mask = ids.cuda(), mask.cuda()
    live = mask.bool()
    weight = torch.randn(len(PADDED_LENS), L, HIDDEN, generator=g).cuda() * live[..., None]
    enc = fused_bert.for_model(model)
    pads = []
    real = ops.attention_train
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (pads.append(k["pad_len"]), real(*a, **k))[1])

    def grads(fn):
        model.zero_grad(set_to_none=True)
        h = fn()
        (h.float() * weight).sum().backward()
        return h.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    torch.manual_seed(21)
    h_k, g_k = grads(lambda: enc.forward_train(ids, mask.sum(1).to(torch.int32), dtype=dtype))
    assert pads == [L, L]
    seed = enc.last_seed
    h32, g32 = grads(lambda: _restate(model, ids, mask, seed))
    with torch.autocast("cuda", dtype=dtype):
        h_m, g_m = grads(lambda: _restate(model, ids, mask, seed))
    e_k, e_y, ref_max = (h_k[live] - h32[live]).abs().max().item(), (h_m[live] - h32[live]).abs().max().item(), h32[live].abs().max().item()
    print(f"padded branch with dropout {kind} {str(dtype)[6:]}: hidden max err kernels {e_k:.3e} restatement under autocast {e_y:.3e}")
    assert torch.isfinite(h_k).all() and e_k <= max(1.5 * e_y, spacing(ref_max, dtype)), (e_k, e_y)
    floor = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for name in sorted(g_k):
        if name.endswith(_KEY_BIAS) or name.startswith("pooler."):
            continue
        ref = g32[name].double()
        rel_k = ((g_k[name].double() - ref).norm() / ref.norm()).item()
        rel_m = ((g_m[name].double() - ref).norm() / ref.norm()).item()
        assert rel_k <= max(1.5 * rel_m, floor), (name, rel_k, rel_m)
