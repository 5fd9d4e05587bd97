"""RoBERTa, XLM-R and MPNet on the layer kernels: the attention kernel's additive relative position bias (csrc/ccr_encoder.hip,
ccr_attention_bias_half, ops.attention(rel_bias=...)) and the three classes through every inference path of ccrec_amd/fused_bert.py.

Tolerances.  The kernel against an fp32 torch reference on the same 16-bit qkv: ATT_TOL of tests/test_gpu_encoder_kernels.py -- the bias
is one more fp32 addition in front of a softmax whose probabilities are rounded to 16 bits, so the bound of the plain kernel applies.  A
zero table: the plain kernel's bits.  The selector probe is exact by construction (below).  Whole models: the convention of
test_fused_forward_is_as_close_to_fp32_as_the_autocast_module -- at most 1.5 x the autocast module's own distance from the fp32 module,
with the same floors.  RoBERTa's training step: the comparison and bounds of tests/test_gpu_encoder_train.py's BERT case."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, PKG  # noqa: F401
from helpers import spacing as _spacing
from test_gpu_encoder_kernels import ATT_TOL, HALVES

pytestmark = pytest.mark.gpu

LENGTHS = [1, 31, 32, 33, 63, 64, 65, 128, 129, 200, 257, 512]


# ------------------------------------------------------------------------------------------------------------------- the kernel
def _layout(lens, padded):
    L = max(lens)
    if padded:
        pad = min(512, (L + 7) // 8 * 8)
        return [i * pad for i in range(len(lens))], pad * len(lens), pad
    return [int(v) for v in np.cumsum([0] + lens[:-1])], sum(lens), 0


def _reference(qkv, starts, lens, H, table, R):
    """fp32 softmax(Q K^T / 8 + table[h, R + key - query]) V per (sequence, head) on the 16-bit operands."""
    T = qkv.shape[0]
    out = torch.zeros(T, H * 64, dtype=torch.float32, device=qkv.device)
    x = qkv.float().view(T, 3, H, 64)
    for s0, n in zip(starts, lens):
        q, k, v = (x[s0:s0 + n, i].transpose(0, 1) for i in range(3))          # [H, n, 64]
        i, j = torch.arange(n, device=qkv.device)[:, None], torch.arange(n, device=qkv.device)[None, :]
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125 + table[:, (j - i) + R], dim=-1)
        out[s0:s0 + n] = (p @ v).transpose(0, 1).reshape(n, H * 64)
    return out


def _widen(table, R, seed):
    """The table of span R(table) inside a random table of span R: the same bias, other numbers around it."""
    r = table.shape[1] // 2
    g = torch.Generator().manual_seed(seed)
    wide = (torch.randn(table.shape[0], 2 * R + 1, generator=g) * 2.0).to(table.device)
    wide[:, R - r:R + r + 1] = table
    return wide.contiguous()


def _companions(L):
    """A batch whose longest sequence has L tokens: L first, then shorter ones from both sides of the 32- and 64-key steps."""
    return [L] + [n for n in (1, 33, 64, 97) if n < L][-2:] + ([L - 1] if L > 1 else [])


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "packed"])
@pytest.mark.parametrize("H", [1, 2, 12])
@pytest.mark.parametrize("L", LENGTHS)
def test_biased_attention_matches_the_fp32_reference(L, H, padded, half):
    from ccrec_amd import ops
    atol, rtol = ATT_TOL[half]
    lens = _companions(L)
    starts, T, pad = _layout(lens, padded)
    torch.manual_seed(1000 * L + 10 * H + padded)
    qkv = (torch.randn(T, 3 * H * 64, device="cuda") * 1.5).to(half)
    if padded:      # padding rows hold NaN: nothing reads them as keys, and their output rows are zeros
        live = torch.zeros(T, dtype=torch.bool, device="cuda")
        for s0, n in zip(starts, lens):
            live[s0:s0 + n] = True
        qkv[~live] = float("nan")
    table = (torch.randn(H, 2 * L - 1, device="cuda") * 2.0).contiguous()      # N(0, 2^2): no symmetry between +d and -d
    seq_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ref = _reference(torch.nan_to_num(qkv.float()).to(half), starts, lens, H, table, L - 1)
    plain = ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad).float()
    for R, tab in ((L - 1, table), (511, _widen(table, 511, L))):
        out = torch.full((T, H * 64), 7.0, dtype=half, device="cuda")
        ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, out=out, rel_bias=tab, rel_span=R)
        got = out.float()
        assert torch.isfinite(got).all()
        for s0, n in zip(starts, lens):
            err = (got[s0:s0 + n] - ref[s0:s0 + n]).abs().max().item()
            print(f"L={L} H={H} {'padded' if padded else 'packed'} {str(half)[6:]} R={R} len={n}: max |err| {err:.3e}")
            torch.testing.assert_close(got[s0:s0 + n], ref[s0:s0 + n], atol=atol, rtol=rtol)
            if padded:
                assert (got[s0 + n:s0 + pad] == 0).all(), "padding rows must be zeros"
    if L > 1:      # (the bias matters: the plain kernel's output is far outside the tolerance)
        assert (plain - ref)[starts[0]:starts[0] + L].abs().max().item() > 10 * atol


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("lens,H,padded", [([1, 31, 65], 2, True), ([200, 129, 64, 5], 12, False), ([512, 257], 1, True)])
def test_zero_table_gives_the_plain_kernel_bits(lens, H, padded, half):
    from ccrec_amd import ops
    L = max(lens)
    starts, T, pad = _layout(lens, padded)
    torch.manual_seed(L + H)
    qkv = (torch.randn(T, 3 * H * 64, device="cuda") * 1.5).to(half)
    seq_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    plain = ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad)
    for R in (L - 1, 511):
        zero = torch.zeros(H, 2 * R + 1, device="cuda")
        got = ops.attention(qkv, seq_start, seq_len, H, max_len=L, pad_len=pad, rel_bias=zero)      # (rel_span from the table's width)
        rows = torch.cat([torch.arange(s0, s0 + max(n, pad), device="cuda") for s0, n in zip(starts, lens)])
        assert torch.equal(got[rows].view(torch.int16), plain[rows].view(torch.int16))


def _probe_offsets(L):
    return sorted({d for d in (-(L - 1), -64, -33, -32, -1, 0, 1, 31, 32, 63, 64, L - 1) if abs(d) <= L - 1})


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("L", [65, 200])
def test_exact_selector_probe(L, half):
    """q = k = 0: every score is the bias alone.  Head 0's table is +30 at offset d0 and 0 elsewhere, head 1's +30 at -d0.  Where query i
    has a key at i + d0 that key's probability is 1 / (1 + (L - 1) e^-30) = 1 - 2e-11 and the L - 1 others hold 1e-13 each: the output row
    is V[i + d0] -- every entry 0 or a small integer, exact in both 16-bit types -- to one rounding of the type.  Elsewhere every bias is 0,
    the softmax is uniform and the row is the mean of V's rows (ATT_TOL).  V row r is (1 + r // 64) at column r % 64 and 0 elsewhere: no
    two rows are equal.  One launch per (d0, table span)."""
    from ccrec_amd import ops
    offsets = _probe_offsets(L)
    assert {-(L - 1), L - 1, 0, -1, 1, 32, -32}.issubset(offsets)
    H = 2
    V = torch.zeros(L, 64)
    V[torch.arange(L), torch.arange(L) % 64] = 1.0 + (torch.arange(L) // 64).float()
    qkv = torch.zeros(L, 3, H, 64)
    qkv[:, 2] = V[:, None, :]
    qkv = qkv.view(L, 3 * H * 64).to(half).cuda().contiguous()
    start = torch.zeros(1, dtype=torch.int32, device="cuda")
    length = torch.full((1,), L, dtype=torch.int32, device="cuda")
    mean = V.mean(0)
    ulp = 2.0 ** -8 if half == torch.bfloat16 else 2.0 ** -11
    for d0 in offsets:
        for R in (L - 1, 511):
            table = torch.zeros(H, 2 * R + 1)
            table[0, R + d0] = 30.0
            table[1, R - d0] = 30.0
            got = ops.attention(qkv, start, length, H, max_len=L, rel_bias=table.cuda(), rel_span=R).float().cpu().view(L, H, 64)
            for h, d in ((0, d0), (1, -d0)):
                i = torch.arange(L)
                hit = (i + d >= 0) & (i + d < L)
                want = V[(i + d).clamp(0, L - 1)]
                worst = (got[hit, h] - want[hit]).abs().max().item()
                assert worst <= 4 * ulp, (L, d0, R, h, worst)      # (V's largest entry is 4)
                if (~hit).any():
                    torch.testing.assert_close(got[~hit, h], mean.expand(int((~hit).sum()), 64), atol=ATT_TOL[half][0], rtol=ATT_TOL[half][1])


def test_bias_arguments_are_checked():
    from ccrec_amd import ops, _lib
    qkv = torch.zeros(16, 3 * 64, dtype=torch.bfloat16, device="cuda")
    s = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = torch.full((1,), 16, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.CcrError, match="R=14"):
        ops.attention(qkv, s, n, 1, max_len=16, rel_bias=torch.zeros(1, 29, device="cuda"))      # R = 14 < max_len - 1
    with pytest.raises(_lib.CcrError, match="R=512"):
        ops.attention(qkv, s, n, 1, max_len=16, rel_bias=torch.zeros(1, 1025, device="cuda"))
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 1, max_len=16, rel_bias=torch.zeros(2, 31, device="cuda"))      # a row per head
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 1, max_len=16, rel_bias=torch.zeros(1, 31, device="cuda"), rel_span=16)
    with pytest.raises(AssertionError):
        ops.attention(qkv, s, n, 1, max_len=16, rel_span=15)
    ops.attention(qkv, s, n, 1, max_len=16, rel_bias=torch.zeros(1, 31, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------- whole models
MODEL_LENS = [40, 1, 17, 33, 64, 65, 128, 130, 97, 200]      # (the list of test_fused_forward_is_as_close_to_fp32_as_the_autocast_module)
PAD = 1
VOCAB = 600
MODELS = {"mpnet-256": ("mpnet", 256, 4, 25.0), "mpnet-768": ("mpnet", 768, 12, 12.0), "roberta-256": ("roberta", 256, 4, 25.0),
          "xlmr-256": ("xlmr", 256, 4, 25.0)}


def _build(kind, hidden, heads, scale, layers=2, seed=0, train_dropout=None):
    import transformers
    cfg_cls, cls = {"roberta": (transformers.RobertaConfig, transformers.RobertaModel),
                    "xlmr": (transformers.XLMRobertaConfig, transformers.XLMRobertaModel),
                    "mpnet": (transformers.MPNetConfig, transformers.MPNetModel)}[kind]
    extra = {} if train_dropout is None else {"hidden_dropout_prob": train_dropout, "attention_probs_dropout_prob": train_dropout}
    if kind != "mpnet":
        extra["type_vocab_size"] = 1      # (what the RoBERTa and XLM-R checkpoints ship: a one-row type table)
    torch.manual_seed(seed + hidden)
    m = cls(cfg_cls(vocab_size=VOCAB, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                    max_position_embeddings=514, pad_token_id=PAD, **extra)).cuda().eval()
    with torch.no_grad():      # the default init (std 0.02) leaves every softmax near uniform and the bias invisible
        for layer in m.encoder.layer:
            att = layer.attention.attn if kind == "mpnet" else layer.attention.self
            q, k = (att.q, att.k) if kind == "mpnet" else (att.query, att.key)
            q.weight.mul_(scale)
            k.weight.mul_(scale)
        if kind == "mpnet":
            m.encoder.relative_attention_bias.weight.normal_(0.0, 1.0)
    return m


def _ids(lens, L, seed=0):
    """Right-padded ids from [2, vocab), padding = the pad id; the row of 33 tokens holds a pad-id token inside its live part."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), L), PAD, dtype=torch.int64)
    mask = torch.zeros(len(lens), L, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.randint(2, VOCAB, (n,), generator=g)
        mask[r, :n] = 1
    ids[lens.index(33), 7] = PAD
    return ids.cuda(), mask.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")


_CASES = {}


def _case(name):
    """(model, ids, mask, lengths, fp32 hidden states, {half: the autocast module's hidden states}) -- built once per model, read-only."""
    if name not in _CASES:
        model = _build(*MODELS[name])
        ids, mask, lengths = _ids(MODEL_LENS, 200)
        with torch.no_grad():
            ref = model(input_ids=ids, attention_mask=mask).last_hidden_state
            amp = {}
            for half in HALVES:
                with torch.autocast("cuda", dtype=half):
                    amp[half] = model(input_ids=ids, attention_mask=mask).last_hidden_state.float()
        _CASES[name] = (model, ids, mask, lengths, ref, amp)
    return _CASES[name]


def _assert_as_close_as_the_autocast_module(got, amp, ref, what):
    """Rows [n, hidden] each: at most 1.5 x the autocast module's own distance from fp32 (max and mean) plus the floors 1e-3 / 1e-4, and
    the cosine convention of the BERT test."""
    assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all()
    e_amp, e_got = (amp - ref).abs(), (got - ref).abs()
    cos = F.cosine_similarity(got, ref, dim=-1).min().item()
    cos_amp = F.cosine_similarity(amp, ref, dim=-1).min().item()
    print(f"{what}: max |err| kernels {e_got.max().item():.3e} module {e_amp.max().item():.3e}; mean {e_got.mean().item():.3e} "
          f"{e_amp.mean().item():.3e}; min cos {cos:.6f} {cos_amp:.6f}")
    assert e_got.max().item() <= 1.5 * e_amp.max().item() + 1e-3, (what, e_got.max().item(), e_amp.max().item())
    assert e_got.mean().item() <= 1.5 * e_amp.mean().item() + 1e-4, (what, e_got.mean().item(), e_amp.mean().item())
    assert cos > cos_amp - 1e-3 and cos > 0.995, (what, cos, cos_amp)


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_forward_paths_are_as_close_to_fp32_as_the_autocast_module(name, half):
    """forward (right-padded rows and packed), forward_packed on a packed array of its own, and cls_only."""
    from ccrec_amd.fused_bert import FusedBertEncoder, unsupported_reason
    model, ids, mask, lengths, ref, amp = _case(name)
    assert unsupported_reason(model) is None
    live = mask.bool()
    enc = FusedBertEncoder(model)
    padded = enc.forward(ids, lengths, packed=False, dtype=half)
    _assert_as_close_as_the_autocast_module(padded[live], amp[half][live], ref[live], f"{name} forward padded")
    packed = enc.forward(ids, lengths, packed=True, dtype=half)
    _assert_as_close_as_the_autocast_module(packed[live], amp[half][live], ref[live], f"{name} forward packed")
    assert (packed[~live] == 0).all()
    B, L = ids.shape
    c_of = torch.arange(L, device="cuda").repeat(B)[live.flatten()]      # 0-based in-sequence positions: forward_packed's contract
    seq_start = (torch.cumsum(lengths, 0, dtype=torch.int32) - lengths).contiguous()
    rows = enc.forward_packed(ids[live], c_of, seq_start, lengths, max(MODEL_LENS), dtype=half)
    _assert_as_close_as_the_autocast_module(rows, amp[half][live], ref[live], f"{name} forward_packed")
    first = enc.forward(ids, lengths, cls_only=True, dtype=half)
    assert tuple(first.shape) == (B, 1, ref.shape[-1])
    _assert_as_close_as_the_autocast_module(first[:, 0], amp[half][:, 0], ref[:, 0], f"{name} cls_only")
    first_packed = enc.forward_packed(ids[live], c_of, seq_start, lengths, max(MODEL_LENS), cls_only=True, dtype=half)
    _assert_as_close_as_the_autocast_module(first_packed, amp[half][:, 0], ref[:, 0], f"{name} forward_packed cls_only")


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_tower_under_autocast_takes_the_kernels(name, half, monkeypatch):
    from ccrec_amd import fused_bert
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.delenv("CCREC_FUSED_ENCODER", raising=False)
    model, ids, mask, lengths, _, _ = _case(name)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(model.config.hidden_size, elementwise_affine=False)).cuda().eval()
    calls = []
    real = fused_bert.FusedBertEncoder.forward
    monkeypatch.setattr(fused_bert.FusedBertEncoder, "forward", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for step in ("mean_pooling", "cls"):
        del calls[:]
        with torch.no_grad():
            ref = tower(input_ids=ids, attention_mask=mask, output_step=step).float()
            assert not calls                                   # fp32, no autocast: the module
            with torch.autocast("cuda", dtype=half):
                got = tower(input_ids=ids, attention_mask=mask, output_step=step).float()
                assert len(calls) == 1
                monkeypatch.setenv("CCREC_FUSED_ENCODER", "0")
                amp = tower(input_ids=ids, attention_mask=mask, output_step=step).float()
                monkeypatch.delenv("CCREC_FUSED_ENCODER")
                assert len(calls) == 1
        _assert_as_close_as_the_autocast_module(got, amp, ref, f"{name} tower {step}")


class _Tokenizer:
    """Whitespace tokenizer with the HF call shape (padding=False -> lists): <s> = 0, </s> = 2, pad = 1, word w<i> -> 4 + i, and the word
    <pad> -> the pad id (a pad-id token inside a live text)."""
    pad_token_id = PAD

    def __call__(self, texts, truncation=True, padding=True, max_length=64, return_tensors="pt"):
        assert padding is False
        ids = [[0] + [PAD if w == "<pad>" else 4 + int(w[1:]) for w in t.split()][: max_length - 2] + [2] for t in texts]
        return {"input_ids": ids, "attention_mask": [[1] * len(r) for r in ids]}


@pytest.mark.parametrize("name", ["mpnet-256", "roberta-256", "xlmr-256"])
def test_length_sorted_encoder_on_the_kernels(name):
    """LengthSortedEncoder(fused=True): packed, length-sorted batches through forward_packed (mean pooling) and its cls_only form."""
    from ccrec_amd.encode import LengthSortedEncoder
    from ccrec_amd.item_tower import NaiveItemTower
    model = _case(name)[0]
    hidden = model.config.hidden_size
    tower = NaiveItemTower(model, torch.nn.LayerNorm(hidden, elementwise_affine=False)).cuda()
    rs = np.random.RandomState(0)
    texts = [" ".join(f"w{i}" for i in rs.randint(0, VOCAB - 4, max(n - 2, 0))) for n in MODEL_LENS * 3 if n >= 2]
    texts[3] = "w5 <pad> w9 " + texts[3]
    tok = _Tokenizer()
    for step in ("mean_pooling", "cls"):
        kw = dict(max_length=200, max_tokens=2048, output_step=step)
        fused = LengthSortedEncoder(tower, tok, fused=True, **kw)
        plain = LengthSortedEncoder(tower, tok, fused=False, **kw)
        ref, amp, got = (torch.zeros(len(texts), hidden, device="cuda") for _ in range(3))
        plain.encode(texts, out_f32=ref)                       # fp32 module
        with torch.autocast("cuda", dtype=torch.float16):
            plain.encode(texts, out_f32=amp)
            fused.encode(texts, out_f32=got)
        assert fused.stats["fused_layers"] is True and plain.stats["fused_layers"] is False and fused.stats["batches"] > 1
        _assert_as_close_as_the_autocast_module(got, amp, ref, f"{name} LengthSortedEncoder {step}")


def test_refresh_follows_the_bias_parameter():
    from ccrec_amd.fused_bert import FusedBertEncoder
    model = _build("mpnet", 256, 4, 25.0, seed=7)
    ids, mask, lengths = _ids([9, 33, 30], 40)
    enc = FusedBertEncoder(model)
    a = enc.forward(ids, lengths).clone()
    assert enc.refresh() is False
    with torch.no_grad():
        model.encoder.relative_attention_bias.weight.add_(torch.randn_like(model.encoder.relative_attention_bias.weight))
    assert enc.refresh() is True
    b = enc.forward(ids, lengths)
    live = mask.bool()
    assert (a - b)[live].abs().max().item() > 1e-2
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).last_hidden_state
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = model(input_ids=ids, attention_mask=mask).last_hidden_state.float()
    _assert_as_close_as_the_autocast_module(b[live], amp[live], ref[live], "mpnet after the bias changed")
    assert (a - ref)[live].abs().max().item() > 1.5 * (amp - ref)[live].abs().max().item() + 1e-3      # (the old table would not pass)


# ------------------------------------------------------------------------------------------------------------------------ training
_KEY_BIAS = ("attention.self.key.bias",)


def _train_batch():
    from test_gpu_encoder_train import STACK_LENS
    ids, mask, _ = _ids(STACK_LENS, max(STACK_LENS), seed=11)
    return ids, mask


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("packed", [False, True], ids=["forward_train", "forward_train_pooled"])
@pytest.mark.parametrize("kind", ["roberta", "xlmr"])
def test_roberta_fine_tune_step_through_the_layer_kernels(kind, packed, dtype, monkeypatch):
    """test_fine_tune_step_through_the_layer_kernels (tests/test_gpu_encoder_train.py) for a RoBERTa-family encoder: the parameter gradients
    of one MultipleNrlStep on the kernels' training path vs the fp32 module's, yardstick the module under the same autocast.  Per parameter:
    relative L2 error <= 1.5 x the module's (floor 2^-8 bf16 / 2^-11 fp16), cosine >= the module's - 1e-3; the loss within 1.5 x the
    autocast module's deviation (floor one spacing of the type at the loss).  packed: with CCREC_FUSED_ENCODER_TRAIN_PACKED=1 on top, the
    embedding block and the pooling on kernels (forward_train_pooled).  The batch holds a live pad-id token: like the module's
    Embedding(padding_idx), neither path gives the pad rows of the word and position tables a gradient."""
    from ccrec_amd import ops
    from ccrec_amd.item_tower import NaiveItemTower
    from test_gpu_encoder_train import _grads
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    model = _build(kind, 256, 4, 20.0, seed=1, train_dropout=0.0)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()
    ids, mask = _train_batch()
    calls = []
    real = ops.attention_train
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN", raising=False)
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN_PACKED", raising=False)
    loss32, g32 = _grads(tower, ids, mask, None)
    loss_m, g_m = _grads(tower, ids, mask, dtype)
    assert not calls
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    if packed:
        monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_PACKED", "1")
    loss_k, g_k = _grads(tower, ids, mask, dtype)
    assert len(calls) == 3 * 2                               # three tower forwards x two layers
    for table in ("word_embeddings", "position_embeddings"):
        assert (g_k[f"embeddings.{table}.weight"][PAD] == 0).all() and (g32[f"embeddings.{table}.weight"][PAD] == 0).all()
    pooler = {n for n in g32 if n.startswith("pooler.")}
    assert set(g_k) == set(g32) - pooler and set(g_m) - pooler == set(g_k)
    floor = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for name in sorted(g_k):
        ref = g32[name].double()
        assert torch.isfinite(g_k[name]).all() and g_k[name].dtype == torch.float32
        if name.endswith(_KEY_BIAS):      # identically zero (the softmax ignores a shift of a row): only its rounding residue is left
            scale = g32[name.replace("key.bias", "query.bias")].double().norm().item()
            assert g_k[name].double().norm().item() <= max(1.5 * g_m[name].double().norm().item(), floor * scale), name
            continue
        rel_k = ((g_k[name].double() - ref).norm() / ref.norm()).item()
        rel_m = ((g_m[name].double() - ref).norm() / ref.norm()).item()
        cos_k = F.cosine_similarity(g_k[name].double().flatten(), ref.flatten(), dim=0).item()
        cos_m = F.cosine_similarity(g_m[name].double().flatten(), ref.flatten(), dim=0).item()
        print(f"{kind} {str(dtype)[6:]} {name}: relative L2 kernels {rel_k:.3e} module {rel_m:.3e}; cos {cos_k:.6f} {cos_m:.6f}")
        assert rel_k <= max(1.5 * rel_m, floor), (name, rel_k, rel_m)
        assert cos_k >= cos_m - 1e-3, (name, cos_k, cos_m)
    assert abs(loss_k - loss32) <= max(1.5 * abs(loss_m - loss32), _spacing(loss32, dtype)), (loss_k, loss_m, loss32)
    assert "embeddings.position_embeddings.weight" in g_k and "embeddings.token_type_embeddings.weight" in g_k


def test_mpnet_with_the_training_opt_in_trains_as_its_module(monkeypatch):
    """CCREC_FUSED_ENCODER_TRAIN=1 and an MPNet tower: train_unsupported_reason names the bias, no training kernel runs, and the step is
    the module's own -- the same loss, and gradients equal to those of the run without the variable up to the order of the fp32 atomic
    additions in torch's embedding backward (relative 1e-5 of each tensor's largest entry).  The shadow set refuses the model."""
    from ccrec_amd import fused_bert, ops, optim
    from ccrec_amd.item_tower import NaiveItemTower
    from test_gpu_encoder_train import _grads
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    model = _build("mpnet", 256, 4, 20.0, seed=2, train_dropout=0.0)
    tower = NaiveItemTower(model, torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()
    ids, mask = _train_batch()
    calls = []
    real = ops.attention_train
    monkeypatch.setattr(ops, "attention_train", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN", raising=False)
    loss_m, g_m = _grads(tower, ids, mask, torch.bfloat16)
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    assert "relative position bias" in fused_bert.train_unsupported_reason(model)
    loss_k, g_k = _grads(tower, ids, mask, torch.bfloat16)
    assert not calls
    assert abs(loss_k - loss_m) <= 1e-6 * abs(loss_m) and set(g_k) == set(g_m) and "encoder.relative_attention_bias.weight" in g_k
    for name in g_k:
        assert (g_k[name] - g_m[name]).abs().max().item() <= 1e-5 * g_m[name].abs().max().item() + 1e-12, name
    with pytest.raises(AssertionError, match="relative position bias"):
        fused_bert.for_model(model).forward_train(ids, mask.sum(1).to(torch.int32))
    with pytest.raises(ValueError, match="no encoder under the module"):
        optim.FusedAdamW(tower.parameters(), lr=1e-3, shadow_for=tower)
