"""The MiniLM-class encoders on the layer kernels (csrc/ccr_encoder_h32.hip): the attention forward for head width 32, the inference
LayerNorm rows at the odd multiples of 128 from 384 on, and the whole encoder behind CCREC_FUSED_ENCODER_HEAD32=1 (ccrec_amd/fused_bert.py).

The references, tolerances and length sets are those of tests/test_gpu_encoder_kernels.py, restated for width 32 and scale 32 ** -0.5: the
attention tolerance is the rounding of the probabilities plus two ulps of the 16-bit type, which does not depend on the head width; the
LayerNorm bound is fp32 reduction order; the whole encoder is held to "no further from the fp32 module forward than the module's own
forward under the same autocast".

Value-only mutants of the new kernels that this file catches: scale 0.125 in place of 32 ** -0.5 (every attention case: the
scores carry a spread of several units, so the softmax moves by far more than the tolerance); the head offset computed with 64 (every case
with more than one head: head h would read head 2 h's columns, and the H = 3 and H = 12 cases cover odd heads); the key mask off by one at
len (key len - 1 dropped: every sequence loses a key, and at lengths 2, 31 .. 33 that key carries a visible share of the softmax; key len
admitted: the staged image holds a zero row there, whose score 0 joins the denominator of every sequence whose length is no multiple of
64); the LayerNorm divisor 256 C at an odd width (the mean and variance of a 384-wide row scale by 384 / 512: far outside 2e-5).  DESIGN
4.8 holds the counts of one run of each on an MI355X.

A row of 128 elements stays refused (tests/test_gpu_row_kernels.py pins ops.add_layernorm and ops.embed_layernorm at dim 128 as errors), so
the cases the feature's request named at 128 -- add_layernorm (1, 128), the embedding block at 128, BertModel 128 / 2 heads -- are not run:
(1, 384) and (2, 640), the embedding block at 384 and 640, and BertModel 384 / 6 heads (64-wide heads at a new width, no switch) stand in."""

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

pytestmark = pytest.mark.gpu

SWITCH = "CCREC_FUSED_ENCODER_HEAD32"
ATT_TOL = {torch.bfloat16: (1.5e-2, 1.6e-2), torch.float16: (2e-3, 2e-3)}      # (atol, rtol): test_gpu_encoder_kernels.ATT_TOL
ATT_CAP = {torch.bfloat16: 5e-2, torch.float16: 8e-3}                          # ... and its caps on the largest error
HALVES = [torch.bfloat16, torch.float16]
W = 32
SCALE = 32 ** -0.5


def _attention_reference(qkv, starts, lens, H, width=W, scale=SCALE):
    """fp32 softmax(Q K^T * scale) V per (sequence, head) on the 16-bit operands."""
    T = qkv.shape[0]
    out = torch.zeros(T, H * width, dtype=torch.float32, device=qkv.device)
    x = qkv.float().view(T, 3, H, width)
    for s0, n in zip(starts, lens):
        q, k, v = (x[s0:s0 + n, i].transpose(0, 1) for i in range(3))          # [H, n, width]
        p = torch.softmax(q @ k.transpose(1, 2) * scale, dim=-1)
        out[s0:s0 + n] = (p @ v).transpose(0, 1).reshape(n, H * width)
    return out


def _layout(lens, padded):
    L = max(lens)
    if padded:
        pad = (L + 7) // 8 * 8
        return pad, [i * pad for i in range(len(lens))], pad * len(lens)
    return 0, [int(v) for v in np.cumsum([0] + lens[:-1])], sum(lens)


@pytest.mark.parametrize("lens,H,padded", [
    ([1, 2, 31, 32, 33], 2, True),
    ([63, 64, 65, 127, 128, 129], 3, True),
    ([200, 17, 136, 136, 5], 12, True),
    ([512, 300, 257, 1], 2, True),
    ([1, 2, 31, 32, 33, 64, 65, 100], 4, False),
    ([129, 255, 256, 384], 2, False),
])
@pytest.mark.parametrize("half", HALVES)
def test_attention_head32_matches_fp32_reference(lens, H, padded, half):
    from ccrec_amd import ops
    atol, rtol = ATT_TOL[half]
    torch.manual_seed(sum(lens) + H)
    L = max(lens)
    pad, starts, T = _layout(lens, padded)
    qkv = (torch.randn(T, 3 * H * W, device="cuda") * 1.5).to(half)
    if padded:      # padding rows hold NaN: nothing reads them as keys
        live = torch.zeros(T, dtype=torch.bool, device="cuda")
        for s0, n in zip(starts, lens):
            live[s0:s0 + n] = True
        qkv[~live] = float("nan")
    seq_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = torch.full((T, H * W), 7.0, dtype=half, device="cuda")
    got = ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, scale=SCALE, out=out, head_width=32)
    assert got is out
    ref = _attention_reference(torch.nan_to_num(qkv.float()).to(half), starts, lens, H)
    got = out.float()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    print(f"head32 attention {half} lens={lens} H={H}: max |err| = {err:.3e}")
    for s0, n in zip(starts, lens):
        torch.testing.assert_close(got[s0:s0 + n], ref[s0:s0 + n], atol=atol, rtol=rtol)
        if padded:
            assert (got[s0 + n:s0 + pad] == 0).all(), "padding rows must be zeros"
    assert err < ATT_CAP[half]
    fresh = ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, scale=SCALE, head_width=32)      # out allocated by the op
    assert fresh.shape == (T, H * W) and fresh.dtype == half
    for s0, n in zip(starts, lens):
        assert torch.equal(fresh[s0:s0 + n], out[s0:s0 + n])


def test_attention_head32_empty_and_overlong_entries_are_memory_safe():
    """seq_len lives in device memory, so the kernel guards it itself: 0 (or negative) = an empty sequence whose padding rows get zeros and
    whose row range is never read; an entry above max_len is cut to max_len (the LDS image holds max_len keys)."""
    from ccrec_amd import ops
    H, pad = 3, 40
    torch.manual_seed(0)
    qkv = torch.randn(4 * pad, 3 * H * W, device="cuda").to(torch.bfloat16)
    start = torch.arange(4, dtype=torch.int32, device="cuda") * pad
    lens = torch.tensor([0, 17, -3, 40], dtype=torch.int32, device="cuda")
    out = torch.full((4 * pad, H * W), 5.0, dtype=torch.bfloat16, device="cuda")
    ops.attention(qkv, start, lens, H, max_len=40, pad_len=pad, scale=SCALE, out=out, head_width=32)
    ref = _attention_reference(qkv, [pad, 3 * pad], [17, 40], H)
    got = out.float()
    assert (got[:pad] == 0).all() and (got[2 * pad:3 * pad] == 0).all()
    torch.testing.assert_close(got[pad:pad + 17], ref[pad:pad + 17], atol=1.5e-2, rtol=1.6e-2)
    assert (got[pad + 17:2 * pad] == 0).all()
    torch.testing.assert_close(got[3 * pad:], ref[3 * pad:], atol=1.5e-2, rtol=1.6e-2)
    # an entry longer than max_len: attended as its first max_len tokens, no access beyond them
    lens2 = torch.tensor([40, 17, 40, 40], dtype=torch.int32, device="cuda")
    out2 = torch.full((4 * pad, H * W), 5.0, dtype=torch.bfloat16, device="cuda")
    ops.attention(qkv, start, lens2, H, max_len=24, pad_len=pad, scale=SCALE, out=out2, head_width=32)
    ref2 = _attention_reference(qkv, [0, pad, 2 * pad, 3 * pad], [24, 17, 24, 24], H)
    torch.testing.assert_close(out2.float()[:24], ref2[:24], atol=1.5e-2, rtol=1.6e-2)
    torch.testing.assert_close(out2.float()[pad:pad + 17], ref2[pad:pad + 17], atol=1.5e-2, rtol=1.6e-2)
    assert (out2.float()[24:pad] == 0).all()


@pytest.mark.parametrize("lens,H,padded", [([63, 64, 65, 127, 128, 129], 3, True), ([1, 2, 31, 32, 33, 64, 65, 100], 4, False)])
@pytest.mark.parametrize("half", HALVES)
def test_head_width_64_through_the_new_entry_point_is_the_old_call(lens, H, padded, half):
    """ccr_attention_head_half(head_width = 64) runs what ccr_attention_half runs: the same bits; so does ops.attention(head_width=64)."""
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    torch.manual_seed(5)
    L = max(lens)
    pad, starts, T = _layout(lens, padded)
    qkv = (torch.randn(T, 3 * H * 64, device="cuda") * 1.5).to(half)
    seq_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    want = torch.full((T, H * 64), 7.0, dtype=half, device="cuda")
    ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, out=want)
    got = torch.full((T, H * 64), 7.0, dtype=half, device="cuda")
    _lib.check(lib.ccr_attention_head_half(ops._ptr(qkv), ops._ptr(seq_start), ops._ptr(seq_len), ops._ptr(got), len(lens), H, 64, L, pad,
                                           0.125, ops._half_code(half), ops._stream(qkv)), "ccr_attention_head_half")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    named = torch.full((T, H * 64), 7.0, dtype=half, device="cuda")
    ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, out=named, head_width=64)
    assert torch.equal(named.view(torch.int16), want.view(torch.int16))


def test_attention_head32_refusals():
    from ccrec_amd import ops, _lib
    qkv = torch.zeros(16, 3 * 2 * 32, dtype=torch.bfloat16, device="cuda")
    s = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = torch.full((1,), 16, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.attention(qkv, s, n, 2, max_len=16, head_width=32, rel_bias=torch.zeros(2, 31, device="cuda"))
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 3, max_len=16, head_width=32)      # rows are 192 wide, not 3 x 3 x 32
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 2, max_len=16)                      # ... and not 3 x 2 x 64
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 2, max_len=16, head_width=32, out=torch.zeros(16, 2 * 64, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(_lib.CcrError):
        ops.attention(qkv, s, n, 2, max_len=513, head_width=32)
    with pytest.raises(_lib.CcrError):
        ops.attention(qkv, s, n, 2, max_len=0, head_width=32)


@pytest.mark.parametrize("rows,dim", [(1, 384), (2, 640), (7, 384), (1000, 384), (333, 640), (5, 1920), (3, 1152)])
@pytest.mark.parametrize("half", HALVES)
def test_add_layernorm_at_the_odd_multiples_of_128(rows, dim, half):
    from ccrec_amd import ops
    torch.manual_seed(rows + dim)
    x = torch.randn(rows, dim, device="cuda").to(half)
    res = torch.randn(rows, dim, device="cuda") * 3 + 0.5
    gamma = torch.rand(dim, device="cuda") + 0.5
    beta = torch.randn(dim, device="cuda")
    f32, b16 = ops.add_layernorm(x, res, gamma, beta, 1e-12)
    ref = torch.nn.functional.layer_norm(x.float() + res, (dim,), gamma, beta, 1e-12)
    print(f"add_layernorm {half} {rows}x{dim}: max |err| = {(f32 - ref).abs().max().item():.3e}")
    torch.testing.assert_close(f32, ref, atol=2e-5, rtol=2e-5)       # fp32 reduction order only
    assert b16.dtype == half and torch.equal(b16, f32.to(half))      # the 16-bit copy is the rounded fp32 row, bit for bit
    f32_nores, b16_nores = ops.add_layernorm(x, None, gamma, beta, 1e-12)
    torch.testing.assert_close(f32_nores, torch.nn.functional.layer_norm(x.float(), (dim,), gamma, beta, 1e-12), atol=2e-5, rtol=2e-5)
    assert torch.equal(b16_nores, f32_nores.to(half))
    only_b16 = ops.add_layernorm(x, None, gamma, beta, 1e-5, want_f32=False)
    assert only_b16[0] is None
    ref2 = torch.nn.functional.layer_norm(x.float(), (dim,), gamma, beta, 1e-5)
    assert torch.equal(only_b16[1], ops.add_layernorm(x, None, gamma, beta, 1e-5)[0].to(half))
    torch.testing.assert_close(only_b16[1].float(), ref2, atol=2e-2, rtol=8e-3)
    only_f32 = ops.add_layernorm(x, res, gamma, beta, 1e-12, want_bf16=False)
    assert only_f32[1] is None and torch.equal(only_f32[0], f32)


@pytest.mark.parametrize("dim", [384, 640])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("half", HALVES)
def test_a_row_of_equal_elements_normalises_to_exactly_beta(dim, eps, half):
    """The refined mean (one correction step) makes the deviations of an all-equal row exactly zero, whatever eps: y = beta, bit for bit."""
    from ccrec_amd import ops
    torch.manual_seed(dim)
    values = torch.tensor([0.0, 1.0, -3.0, 0.3, 1e-3, 7.77, -123.4, 1e4, 0.1, 2.0 ** -20, 33.3], device="cuda")
    x = values[:, None].expand(-1, dim).to(half).contiguous()
    gamma = torch.rand(dim, device="cuda") + 0.5
    beta = torch.randn(dim, device="cuda")
    for res in (None, torch.full((len(values), dim), 0.7, device="cuda"), values.flip(0)[:, None].expand(-1, dim).contiguous() * 1.37):
        f32, b16 = ops.add_layernorm(x, res, gamma, beta, eps)
        assert torch.equal(f32, beta[None].expand_as(f32)), (f32 - beta).abs().max().item()
        assert torch.equal(b16, beta.to(half)[None].expand_as(b16))


def _bert(hidden, heads, layers=2, inter=768, seed=0, scale=1.0, vocab=600):
    from transformers import BertConfig, BertModel
    torch.manual_seed(seed)
    m = BertModel(BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                             max_position_embeddings=512)).cuda().eval()
    with torch.no_grad():      # the default init (std 0.02) leaves every softmax near uniform: widen the attention projections
        for layer in m.encoder.layer:
            layer.attention.self.query.weight.mul_(scale)
            layer.attention.self.key.weight.mul_(scale)
    return m


def _roberta(hidden, heads, layers=2, inter=768, seed=0, scale=1.0):
    from transformers import RobertaConfig, RobertaModel
    torch.manual_seed(seed)
    m = RobertaModel(RobertaConfig(vocab_size=600, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                                   intermediate_size=inter, max_position_embeddings=514)).cuda().eval()
    with torch.no_grad():
        for layer in m.encoder.layer:
            layer.attention.self.query.weight.mul_(scale)
            layer.attention.self.key.weight.mul_(scale)
    return m


def _distil(hidden, heads, layers=2, inter=768, seed=0, scale=1.0):
    from transformers import DistilBertConfig, DistilBertModel
    torch.manual_seed(seed)
    m = DistilBertModel(DistilBertConfig(vocab_size=600, dim=hidden, n_layers=layers, n_heads=heads, hidden_dim=inter,
                                         max_position_embeddings=512)).cuda().eval()
    with torch.no_grad():
        for layer in m.transformer.layer:
            layer.attention.q_lin.weight.mul_(scale)
            layer.attention.k_lin.weight.mul_(scale)
    return m


def _batch(lens, L, vocab=600, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), L, dtype=torch.int64)
    mask = torch.zeros(len(lens), L, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.randint(2, vocab, (n,), generator=g)
        mask[r, :n] = 1
    return ids.cuda(), mask.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("dim", [384, 640])
def test_embed_layernorm_at_the_new_widths_gives_the_module_bits(dim, half):
    """ccr_embed_layernorm == transformers' BertEmbeddings.forward in eval mode at hidden 384 and 640: the same fp32 sum order, LayerNorm to
    fp32 reduction order (2e-5); the 16-bit copy is the rounded fp32 row; an index outside its table is clamped, not read."""
    from ccrec_amd import ops
    model = _bert(dim, dim // 64, layers=1, inter=2 * dim, seed=2)
    e = model.embeddings
    g = torch.Generator().manual_seed(1)
    T = 3000
    ids = torch.randint(0, 600, (T,), generator=g).cuda()
    pos = torch.randint(0, 512, (T,), generator=g).cuda()
    types = torch.randint(0, 2, (T,), generator=g).cuda()
    with torch.no_grad():
        e.LayerNorm.weight.uniform_(0.5, 1.5)
        e.LayerNorm.bias.normal_()
        for tt in (types, None):
            ref = e(input_ids=ids[None], token_type_ids=(types if tt is not None else torch.zeros_like(ids))[None], position_ids=pos[None])[0]
            f32, b16 = ops.embed_layernorm(e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
                                           ids, pos, tt, e.LayerNorm.weight, e.LayerNorm.bias, e.LayerNorm.eps, dtype=half)
            torch.testing.assert_close(f32, ref, atol=2e-5, rtol=2e-5)
            assert b16.dtype == half and torch.equal(b16, f32.to(half))
        bad = ids.clone()
        bad[0], bad[1] = 10 ** 9, -5
        f32, _ = ops.embed_layernorm(e.word_embeddings.weight, e.position_embeddings.weight, e.token_type_embeddings.weight,
                                     bad, pos, None, e.LayerNorm.weight, e.LayerNorm.bias, e.LayerNorm.eps)
        assert torch.isfinite(f32).all()


LENS = [40, 1, 17, 33, 64, 65, 128, 130, 97, 200]


def _check_against_the_autocast_module(model, enc, lens=LENS):
    """The criterion of test_fused_forward_is_as_close_to_fp32_as_the_autocast_module; -> (the padded forward, ids, mask, lengths)."""
    ids, mask, lengths = _batch(lens, max(lens))
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).last_hidden_state                       # fp32 module forward
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = model(input_ids=ids, attention_mask=mask).last_hidden_state.float()           # what the reference's layer computes
    got = enc.forward(ids, lengths, packed=False)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    live = mask.bool()
    e_amp = (amp - ref)[live].abs()
    e_got = (got - ref)[live].abs()
    print(f"{type(model).__name__}: max {e_got.max().item():.3e} (autocast module {e_amp.max().item():.3e}), "
          f"mean {e_got.mean().item():.3e} ({e_amp.mean().item():.3e})")
    assert e_got.max().item() <= 1.5 * e_amp.max().item() + 1e-3, (e_got.max().item(), e_amp.max().item())
    assert e_got.mean().item() <= 1.5 * e_amp.mean().item() + 1e-4, (e_got.mean().item(), e_amp.mean().item())
    cos = torch.nn.functional.cosine_similarity(got[live], ref[live], dim=-1)
    cos_amp = torch.nn.functional.cosine_similarity(amp[live], ref[live], dim=-1)
    assert cos.min().item() > cos_amp.min().item() - 1e-3 and cos.min().item() > 0.995, (cos.min().item(), cos_amp.min().item())
    assert torch.isfinite(got).all()
    return got, ids, mask, lengths


@pytest.mark.parametrize("kind", ["bert", "distil", "roberta"])
def test_whole_encoder_at_384_with_12_heads_behind_the_switch(monkeypatch, kind):
    from ccrec_amd.fused_bert import FusedBertEncoder, unsupported_reason
    make = {"bert": _bert, "distil": _distil, "roberta": _roberta}[kind]
    model = make(384, 12, layers=2, inter=768, seed=384 + 2, scale=12.0)
    monkeypatch.delenv(SWITCH, raising=False)
    assert "head width" in unsupported_reason(model)
    monkeypatch.setenv(SWITCH, "1")
    assert unsupported_reason(model) is None
    enc = FusedBertEncoder(model)
    got, ids, mask, lengths = _check_against_the_autocast_module(model, enc)
    live = mask.bool()
    again = enc.forward(ids, lengths, packed=False)
    assert torch.equal(got, again)                                                 # two runs: the same bits
    packed = enc.forward(ids, lengths, packed=True)                                # forward_packed on the real tokens, scattered back
    torch.testing.assert_close(packed[live], got[live], atol=3e-2, rtol=2e-2)
    assert torch.nn.functional.cosine_similarity(packed[live], got[live], dim=-1).min().item() > 0.9995
    assert (packed[~live] == 0).all() and torch.equal(packed, enc.forward(ids, lengths, packed=True))
    for form in (False, True):
        cls = enc.forward(ids, lengths, packed=form, cls_only=True)                # cls_rows: the last layer on the first tokens only
        assert cls.shape == (len(LENS), 1, 384)
        torch.testing.assert_close(cls[:, 0], got[:, 0], atol=3e-2, rtol=2e-2)
        assert torch.nn.functional.cosine_similarity(cls[:, 0], got[:, 0], dim=-1).min().item() > 0.9995


def test_bert_384_with_6_heads_needs_no_switch(monkeypatch):
    """Width-64 heads with a new LayerNorm width: accepted as it stands, same criterion; hidden 128 stays refused."""
    from ccrec_amd.fused_bert import FusedBertEncoder, unsupported_reason
    monkeypatch.delenv(SWITCH, raising=False)
    model = _bert(384, 6, layers=2, inter=768, seed=128, scale=12.0)
    assert unsupported_reason(model) is None and "hidden size" in unsupported_reason(_bert(128, 2, layers=1, inter=256))
    _check_against_the_autocast_module(model, FusedBertEncoder(model))


class _WordTokenizer:
    """Whitespace tokenizer with the HF call shape (padding=False -> lists)."""
    pad_token_id = 0

    def __call__(self, texts, truncation=True, padding=True, max_length=64, return_tensors="pt"):
        ids = [[1] + [2 + (sum(map(ord, w)) * 7 % 500) for w in t.split()][: max_length - 2] + [3] for t in texts]
        assert padding is False
        return {"input_ids": ids, "attention_mask": [[1] * len(r) for r in ids]}


def test_length_sorted_encoder_routes_by_the_switch(monkeypatch):
    from ccrec_amd.encode import LengthSortedEncoder
    from ccrec_amd.item_tower import NaiveItemTower
    tok = _WordTokenizer()
    rs = np.random.RandomState(0)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rs.choice(words, rs.randint(1, 60))) for _ in range(200)]
    monkeypatch.delenv(SWITCH, raising=False)
    tower = NaiveItemTower(_bert(384, 12, 2, 768, seed=3, scale=10.0), torch.nn.LayerNorm(384, elementwise_affine=False)).cuda()
    off = LengthSortedEncoder(tower, tok, max_length=64, max_tokens=4096, fused="auto")
    assert off._fused is None
    with pytest.raises(ValueError, match="head width"):
        LengthSortedEncoder(tower, tok, max_length=64, fused=True)
    monkeypatch.setenv(SWITCH, "1")
    on = LengthSortedEncoder(tower, tok, max_length=64, max_tokens=4096, fused="auto")
    assert on._fused is not None
    fa = torch.zeros(200, 384, device="cuda")
    fb = torch.zeros(200, 384, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        on.encode(texts, out_f32=fa)
        off.encode(texts, out_f32=fb)
    assert on.stats["fused_layers"] is True and off.stats["fused_layers"] is False
    assert torch.nn.functional.cosine_similarity(fa, fb, dim=1).min().item() >= 0.9995


def test_item_tower_routes_by_the_switch_and_trains_as_its_module(monkeypatch):
    from ccrec_amd import fused_bert, optim
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.delenv("CCREC_FUSED_ENCODER", raising=False)
    monkeypatch.delenv(SWITCH, raising=False)
    model = _bert(384, 12, 2, 768, seed=5, scale=8.0)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(384, elementwise_affine=False)).cuda().eval()
    ids, mask, _ = _batch([12, 40, 1, 33, 64], 64)
    calls, train_calls = [], []
    real, real_train = fused_bert.FusedBertEncoder.forward, fused_bert.FusedBertEncoder.forward_train
    monkeypatch.setattr(fused_bert.FusedBertEncoder, "forward", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(fused_bert.FusedBertEncoder, "forward_train", lambda self, *a, **k: (train_calls.append(1), real_train(self, *a, **k))[1])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        amp = tower(input_ids=ids, attention_mask=mask, output_step="mean_pooling")            # switch off: the module under autocast
        assert not calls
        monkeypatch.setenv(SWITCH, "1")
        fast = tower(input_ids=ids, attention_mask=mask, output_step="mean_pooling")
        assert len(calls) == 1
        cls = tower(input_ids=ids, attention_mask=mask, output_step="cls")
        assert len(calls) == 2 and cls.shape == (5, 384)
        monkeypatch.delenv(SWITCH)
        tower(input_ids=ids, attention_mask=mask, output_step="mean_pooling")                  # read at call time: the module again
        assert len(calls) == 2
    assert torch.nn.functional.cosine_similarity(fast.float(), amp.float(), dim=1).min().item() > 0.9995
    # training: both opt-ins set, the tower still runs the torch module, and the optimizer refuses to shadow its weights
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = tower(input_ids=ids, attention_mask=mask, output_step="mean_pooling")
    assert out.requires_grad and not train_calls and len(calls) == 2
    out.float().square().mean().backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(torch.isfinite(g).all() for g in grads)
    assert "head width" in fused_bert.shadow_unsupported_reason(model)
    with pytest.raises(ValueError, match="head width"):
        optim.FusedAdamW(tower.parameters(), lr=1e-4, shadow_for=tower, shadow_dtype=torch.bfloat16)
