"""Training dropout from explicit keep bits (library version 104) without a GPU: the CPU restatement of the generator against Philox's
known answers, the packed layouts, the second opt-in's gating on CPU-built models, and the argument checks of every new entry point."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

DROPOUT_EXPORTS = ["ccr_dropout_bits_rows", "ccr_dropout_bits_attention", "ccr_dropout_apply", "ccr_attention_fwd_train_drop_half",
                   "ccr_attention_bwd_drop_half", "ccr_add_layernorm_drop_half", "ccr_add_layernorm_bwd_drop_half"]


def test_philox_known_answers():
    from ccrec_amd import dropout_ref
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        got = dropout_ref.philox4x32_10(counter, key)
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert " ".join(f"{int(w):08x}" for w in got) == want
    # vectorised over counters: the same words as one call each
    many = dropout_ref.philox4x32_10((np.arange(5)[:, None], np.arange(3)[None, :], 7, 2), (11, 13))
    assert many.shape == (5, 3, 4)
    assert np.array_equal(many[4, 2], dropout_ref.philox4x32_10((4, 2, 7, 2), (11, 13)))


def test_threshold_effective_probability_and_scale():
    from ccrec_amd import dropout_ref
    assert dropout_ref.threshold(0.1) == 6554 and dropout_ref.threshold(0.5) == 32768 and dropout_ref.threshold(0.0) == 0
    assert dropout_ref.p_eff(0.1) == 6554 / 65536 and abs(dropout_ref.p_eff(0.1) - 0.100006) < 5e-7 and dropout_ref.p_eff(0.5) == 0.5
    assert dropout_ref.inv_keep(0.5) == 2.0
    assert dropout_ref.inv_keep(0.1) == float(np.float32(65536.0 / (65536 - 6554)))
    assert abs(dropout_ref.inv_keep(0.1) * (1 - dropout_ref.p_eff(0.1)) - 1) < 2.0 ** -23      # E[keep * inv_keep] = 1 to fp32 rounding
    for bad in (1.0, 1.5, -0.1, float("nan"), 1 - 2.0 ** -18):                                  # (the last one rounds to thr = 65536)
        with pytest.raises(ValueError):
            dropout_ref.threshold(bad)


def test_row_wise_bits_layout():
    """3 x 256: bit i of word w is column 32 w + i; lane j of the call with counter (row, group, stream, 0) decides column 8 group + j."""
    from ccrec_amd import dropout_ref
    seed, stream, p = 0x0123456789abcdef, 5, 0.1
    mask, bits = dropout_ref.rows_mask(seed, stream, p, 3, 256), dropout_ref.rows_bits(seed, stream, p, 3, 256)
    assert mask.shape == (3, 256) and mask.dtype == bool and bits.shape == (3, 8) and bits.dtype == np.uint32
    thr = dropout_ref.threshold(p)
    for row, col in [(0, 0), (0, 1), (1, 31), (1, 32), (2, 255), (2, 137)]:
        words = dropout_ref.philox4x32_10((row, col >> 3, stream, 0), (seed & 0xffffffff, seed >> 32))
        j = col & 7
        lane = (int(words[j >> 1]) >> (16 * (j & 1))) & 0xffff
        assert bool(mask[row, col]) == (lane >= thr)
        assert (int(bits[row, col >> 5]) >> (col & 31)) & 1 == int(mask[row, col])
    assert np.array_equal(dropout_ref.unpack_bits(bits, 256), mask)
    assert 0.8 < mask.mean() < 0.97 and not np.array_equal(mask[0], mask[1])
    assert not np.array_equal(dropout_ref.rows_mask(seed, stream + 1, p, 3, 256), mask)          # another stream, other decisions
    assert not np.array_equal(dropout_ref.rows_mask(seed + (1 << 32), stream, p, 3, 256), mask)   # the seed's high word is part of the key
    assert dropout_ref.rows_mask(seed, stream, 0.0, 3, 256).all()


def test_attention_bits_layout_and_the_two_views_agree():
    """Two sequences (40 and 7 tokens at rows 0 and 40), 3 heads: counter (query's token row, key >> 3, stream, head); keep_q and keep_k
    hold the same decision for every (query, key) below the length."""
    from ccrec_amd import dropout_ref
    seed, stream, p, H = 77, 9, 0.5, 3
    starts, lens = [0, 40], [40, 7]
    masks = dropout_ref.attention_mask(seed, stream, p, starts, lens, H)
    keep_q, keep_k = dropout_ref.attention_bits(seed, stream, p, starts, lens, H, max_len=40, n_tokens=47)
    assert keep_q.shape == keep_k.shape == (47, H, 2) and keep_q.dtype == np.uint32
    thr = dropout_ref.threshold(p)
    for s, (start, n) in enumerate(zip(starts, lens)):
        assert masks[s].shape == (H, n, n)
        for h in range(H):
            for q in range(n):
                for k in range(n):
                    a = (int(keep_q[start + q, h, k >> 5]) >> (k & 31)) & 1
                    b = (int(keep_k[start + k, h, q >> 5]) >> (q & 31)) & 1
                    assert a == b == int(masks[s][h, q, k]), (s, h, q, k)
    for s, h, q, k in [(0, 0, 0, 0), (0, 2, 39, 33), (1, 1, 6, 5)]:
        words = dropout_ref.philox4x32_10((starts[s] + q, k >> 3, stream, h), (seed, 0))
        j = k & 7
        assert bool(masks[s][h, q, k]) == (((int(words[j >> 1]) >> (16 * (j & 1))) & 0xffff) >= thr)
    assert 0.4 < masks[0].mean() < 0.6


def test_the_seven_entry_points_are_declared_bound_and_exported():
    from ccrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    lib = _lib.load()
    for name in DROPOUT_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name
        assert re.search(name + r" \((?:bbpr\.py:195-197|bert_mt\.py:105-113)", header), name
    assert _lib.ENCODER_DROPOUT_VERSION == 104 and lib.ccr_version() >= 104
    assert _lib.MIN_VERSION == 101 and _lib.BPR_VERSION == 102 and _lib.ENCODER_TRAIN_VERSION == 103


def test_require_encoder_dropout_rejects_an_older_library(monkeypatch):
    from ccrec_amd import _lib, ops
    lib = _lib.load()

    class Old:
        def ccr_version(self):
            return 103

    monkeypatch.setattr(ops, "_ENCODER_DROPOUT_CHECKED", False)
    monkeypatch.setattr(ops, "require_gpu", lambda: Old())
    with pytest.raises(_lib.CcrError, match="version 103.*need 104"):
        ops._require_encoder_dropout()
    assert ops._ENCODER_DROPOUT_CHECKED is False
    monkeypatch.setattr(ops, "require_gpu", lambda: lib)
    assert ops._require_encoder_dropout() is lib and ops._ENCODER_DROPOUT_CHECKED is True


def test_dropout_gating_truth_table(monkeypatch):
    from transformers import BertConfig, BertModel, DistilBertConfig, DistilBertModel
    from ccrec_amd import fused_bert

    def bert(p):
        return BertModel(BertConfig(vocab_size=50, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                    max_position_embeddings=32, hidden_dropout_prob=p, attention_probs_dropout_prob=p))

    def distil(p):
        return DistilBertModel(DistilBertConfig(vocab_size=50, dim=256, n_layers=2, n_heads=4, hidden_dim=512, dropout=p, attention_dropout=p))

    wet, dry, dwet = bert(0.1).train(), bert(0.0).train(), distil(0.1).train()
    extra = bert(0.1).train()
    extra.encoder.layer[1].intermediate.extra_dropout = torch.nn.Dropout(0.2)      # a live Dropout module that is no known site
    for name in ("CCREC_FUSED_ENCODER_TRAIN", "CCREC_FUSED_ENCODER_TRAIN_DROPOUT"):
        monkeypatch.delenv(name, raising=False)
    assert fused_bert.train_dropout_wanted() is False
    today = fused_bert.train_unsupported_reason(wet)
    assert "dropout" in today and "hidden_dropout_prob=0.1" in today

    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")                    # the new variable alone does nothing
    assert fused_bert.train_dropout_wanted() is True and fused_bert.train_wanted() is False
    assert fused_bert.train_unsupported_reason(wet) == today and "dropout" in fused_bert.train_unsupported_reason(dwet)

    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")                            # the training opt-in alone refuses wet models, as today
    assert fused_bert.train_unsupported_reason(wet) == today and "dropout" in fused_bert.train_unsupported_reason(dwet)
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "0")
    assert fused_bert.train_dropout_wanted() is False and fused_bert.train_unsupported_reason(wet) == today

    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")                    # both: wet BERT and wet DistilBERT are accepted
    assert fused_bert.train_unsupported_reason(wet) is None and fused_bert.train_unsupported_reason(dwet) is None
    assert fused_bert.train_unsupported_reason(dry) is None and fused_bert.train_unsupported_reason(wet.eval()) is None
    wet.train()
    reason = fused_bert.train_unsupported_reason(extra)
    assert reason is not None and "encoder.layer.1.intermediate.extra_dropout" in reason and "0.2" in reason
    extra.encoder.layer[1].intermediate.extra_dropout.p = 0.0                       # ... a dead one is no obstacle
    assert fused_bert.train_unsupported_reason(extra) is None
    extra.encoder.layer[1].intermediate.extra_dropout.p = 0.2                       # ... nor is one in eval() inside the train() model:
    extra.encoder.layer[1].intermediate.extra_dropout.eval()                        # torch would not apply it either
    assert fused_bert.train_unsupported_reason(extra) is None
    wet.encoder.layer[0].output.dropout.p = 1.0                                     # p is read from the modules at call time
    assert "p=1" in fused_bert.train_unsupported_reason(wet)
    wet.encoder.layer[0].output.dropout.p = 0.3
    assert fused_bert.train_unsupported_reason(wet) is None
    assert "head width" in fused_bert.train_unsupported_reason(BertModel(BertConfig(vocab_size=50, hidden_size=256, num_hidden_layers=1,
                                                                                    num_attention_heads=8, intermediate_size=512)).train())
    # stream ids: one per (layer, site), none equal to the embeddings'
    ids = {fused_bert.dropout_stream(layer, site) for layer in range(13) for site in range(3)}
    assert len(ids) == 39 and fused_bert.EMBEDDINGS_STREAM not in ids
    torch.manual_seed(5)
    a, b = fused_bert.draw_seed(), fused_bert.draw_seed()
    torch.manual_seed(5)
    assert fused_bert.draw_seed() == a and a != b and 0 <= a < 1 << 64


def test_new_entry_points_reject_bad_arguments_before_any_device_call():
    """The argument checks come first: with no GPU in the machine these return their error code instead of a HIP error."""
    from ccrec_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * (4096 + 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 4096 bytes of host memory, 16-byte aligned: never dereferenced
    bf16, f16, f32 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32
    inv, wsp = _lib.CCR_ERR_INVALID, _lib.CCR_ERR_WORKSPACE

    def rows(bits=p, n=8, dim=256, prob=0.1):
        return lib.ccr_dropout_bits_rows(bits, n, dim, 1, 2, prob, None)

    assert rows(bits=None) == inv and b"null pointer" in lib.ccr_last_error()
    assert rows(dim=320) == inv and rows(dim=2304) == inv and rows(dim=0) == inv and rows(n=-1) == inv
    assert rows(prob=1.0) == inv and b"p=1" in lib.ccr_last_error() and rows(prob=1.5) == inv and rows(prob=-0.5) == inv
    assert rows(prob=float("nan")) == inv and rows(n=0) == _lib.CCR_OK

    def att(keep_q=p, keep_k=p, start=p, lens=p, n_heads=2, max_len=64, prob=0.1):
        return lib.ccr_dropout_bits_attention(keep_q, keep_k, start, lens, 64, 1, n_heads, max_len, 1, 2, prob, None)

    assert att(keep_q=None) == inv and att(keep_k=None) == inv and att(start=None) == inv and att(lens=None) == inv
    assert att(max_len=0) == inv and att(max_len=513) == inv and b"max_len=513" in lib.ccr_last_error()
    assert att(n_heads=0) == inv and att(prob=1.0) == inv and att(prob=2.0) == inv

    def apply(x=p, bits=p, out=p, inv_keep=1.25, n=8, dim=256, dtype=bf16):
        return lib.ccr_dropout_apply(x, bits, inv_keep, out, None, n, dim, dtype, None)

    assert apply(x=None) == inv and apply(bits=None) == inv and apply(out=None) == inv
    assert apply(dim=320) == inv and apply(dtype=f32) == inv and b"half_dtype" in lib.ccr_last_error()
    assert apply(inv_keep=0.5) == inv and apply(inv_keep=float("inf")) == inv and apply(n=0) == _lib.CCR_OK

    def fwd(lse=p, keep_q=p, n_heads=2, max_len=64, pad_len=0, scale=0.125, dtype=bf16, qkv=p, inv_keep=2.0):
        return lib.ccr_attention_fwd_train_drop_half(qkv, p, p, p, lse, keep_q, inv_keep, 1, n_heads, max_len, pad_len, scale, dtype, None)

    assert fwd(lse=None) == inv and fwd(keep_q=None) == inv and fwd(qkv=None) == inv
    assert fwd(max_len=513) == inv and fwd(max_len=0) == inv and fwd(pad_len=513) == inv and fwd(n_heads=0) == inv
    assert fwd(scale=0.0) == inv and fwd(dtype=f32) == inv and fwd(inv_keep=0.0) == inv and fwd(inv_keep=float("nan")) == inv

    def bwd(qkv=p, keep_q=p, keep_k=p, d_qkv=p, ws=p, max_len=64, dtype=f16, ws_bytes=4096, inv_keep=2.0):
        return lib.ccr_attention_bwd_drop_half(qkv, p, p, p, p, p, keep_q, keep_k, inv_keep, d_qkv, 1, 2, max_len, 0, 0.125, dtype, ws, ws_bytes, None)

    assert bwd(qkv=None) == inv and bwd(keep_q=None) == inv and bwd(keep_k=None) == inv and bwd(d_qkv=None) == inv and bwd(ws=None) == inv
    assert bwd(max_len=513) == inv and bwd(max_len=0) == inv and bwd(dtype=f32) == inv and bwd(inv_keep=0.9) == inv
    assert bwd(ws_bytes=2 * 64 * 4 - 1) == wsp and b"workspace" in lib.ccr_last_error()

    def ln(x=p, bits=p, gamma=p, dim=256, dtype=bf16, inv_keep=1.5, n=8):
        return lib.ccr_add_layernorm_drop_half(x, bits, inv_keep, None, gamma, p, 1e-12, p, None, n, dim, dtype, None)

    assert ln(x=None) == inv and ln(bits=None) == inv and ln(gamma=None) == inv
    assert ln(dim=320) == inv and ln(dim=2304) == inv and ln(dtype=f32) == inv and ln(inv_keep=0.0) == inv and ln(n=0) == _lib.CCR_OK

    def lnb(x=p, bits=p, gamma=p, d_y=p, dim=256, dtype=bf16, ws=p, ws_bytes=4096, d_gamma=p, n=8, inv_keep=1.5):
        return lib.ccr_add_layernorm_bwd_drop_half(x, bits, inv_keep, None, gamma, 1e-12, d_y, p, None, d_gamma, None, n, dim, dtype, ws, ws_bytes, None)

    assert lnb(x=None) == inv and lnb(bits=None) == inv and lnb(gamma=None) == inv and lnb(d_y=None) == inv
    assert lnb(dim=320) == inv and lnb(dim=0) == inv and lnb(n=-1) == inv and lnb(dtype=f32) == inv and lnb(inv_keep=0.5) == inv
    assert lnb(ws_bytes=2 * 2 * 256 * 4 - 1) == wsp and lnb(ws=None, ws_bytes=0) == wsp
    assert lnb(n=0, d_gamma=None, ws=None, ws_bytes=0) == _lib.CCR_OK
