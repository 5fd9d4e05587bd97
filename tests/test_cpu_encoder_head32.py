"""The MiniLM-class encoders on the layer kernels (hidden 384, 12 heads of width 32; CCREC_FUSED_ENCODER_HEAD32=1, default off), as far as it
can be checked without a GPU: which models fused_bert accepts and refuses with the switch off and on, that training and the 16-bit shadow
set stay refused for them, that a 64-wide-head model at a new LayerNorm width (hidden 384 with 6 heads, 640 with 10) needs no switch, and the
argument checks of ccr_attention_head_half and of the LayerNorm entry points at the new widths, which all run before any launch.  The GPU
side is tests/test_gpu_encoder_head32.py.

A row of 128 elements (bert-tiny's hidden size) stays refused at every level: tests/test_gpu_row_kernels.py pins ops.add_layernorm and
ops.embed_layernorm at dim 128 as errors, so the new widths start at 384 and the cases the feature's request named at 128 are not here."""

import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

SWITCH = "CCREC_FUSED_ENCODER_HEAD32"


def _model(kind, hidden, heads, layers=1):
    import transformers as tf
    torch.manual_seed(0)
    if kind == "distil":
        return tf.DistilBertModel(tf.DistilBertConfig(vocab_size=120, dim=hidden, n_layers=layers, n_heads=heads, hidden_dim=2 * hidden,
                                                      max_position_embeddings=514))
    cfg_cls, cls = {"bert": (tf.BertConfig, tf.BertModel), "roberta": (tf.RobertaConfig, tf.RobertaModel),
                    "mpnet": (tf.MPNetConfig, tf.MPNetModel)}[kind]
    return cls(cfg_cls(vocab_size=120, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                       max_position_embeddings=514))


def test_switch_unset_keeps_every_refusal(monkeypatch):
    from ccrec_amd import fused_bert
    monkeypatch.delenv(SWITCH, raising=False)
    assert fused_bert.head32_wanted() is False
    assert "head width" in fused_bert.unsupported_reason(_model("bert", 256, 8))
    assert fused_bert.unsupported_reason(_model("bert", 256, 8)) == "head width 32 (the attention kernel is built for 64)"
    assert "head width" in fused_bert.unsupported_reason(_model("distil", 256, 2))
    assert "hidden size" in fused_bert.unsupported_reason(_model("bert", 192, 3))
    assert "head width" in fused_bert.unsupported_reason(_model("bert", 384, 12))
    monkeypatch.setenv(SWITCH, "0")      # only "1" switches it on
    assert "head width" in fused_bert.unsupported_reason(_model("bert", 384, 12))
    with pytest.raises(ValueError):
        fused_bert.FusedBertEncoder(_model("bert", 384, 12))


@pytest.mark.parametrize("kind", ["bert", "roberta", "distil"])
def test_switch_on_accepts_head_width_32(monkeypatch, kind):
    from ccrec_amd import fused_bert
    monkeypatch.setenv(SWITCH, "1")
    assert fused_bert.head32_wanted() is True
    assert fused_bert.unsupported_reason(_model(kind, 384, 12)) is None
    assert fused_bert.unsupported_reason(_model(kind, 256, 8)) is None
    enc = fused_bert.FusedBertEncoder(_model(kind, 384, 12))
    assert enc.heads == 12 and enc.hidden == 384
    monkeypatch.delenv(SWITCH)                                   # read at call time: the same process refuses again
    assert "head width" in fused_bert.unsupported_reason(_model(kind, 384, 12))


def test_switch_on_keeps_the_other_refusals(monkeypatch):
    from ccrec_amd import fused_bert
    monkeypatch.setenv(SWITCH, "1")
    reason = fused_bert.unsupported_reason(_model("mpnet", 256, 8))      # no bias form at width 32: the reason names both
    assert "head width" in reason and "relative position bias" in reason
    assert fused_bert.unsupported_reason(_model("mpnet", 256, 4)) is None
    assert "hidden size" in fused_bert.unsupported_reason(_model("bert", 192, 3))
    assert "head width" in fused_bert.unsupported_reason(_model("bert", 256, 2))       # head width 128
    assert "head width" in fused_bert.unsupported_reason(_model("bert", 256, 16))      # head width 16
    assert "hidden size" in fused_bert.unsupported_reason(_model("bert", 96, 3))       # head width 32, hidden no multiple of 128


@pytest.mark.parametrize("switch", [None, "1"])
def test_training_and_the_shadow_set_stay_refused_at_head_width_32(monkeypatch, switch):
    from ccrec_amd import fused_bert
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", raising=False)
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    model = _model("bert", 384, 12)
    for m in (model.train(), model.eval()):
        assert "head width" in fused_bert.train_unsupported_reason(m)
        assert "head width" in fused_bert.shadow_unsupported_reason(m)
    mp = fused_bert.train_unsupported_reason(_model("mpnet", 256, 8).eval())
    assert "head width" in mp


def test_new_layernorm_widths_need_no_switch(monkeypatch):
    """Width-64 heads at hidden 384 and 640: inference accepted, training refused with the width rule of the training kernels; a 256 C model
    trains as before; hidden 128 stays refused (an existing test pins that width as an error of the row kernels)."""
    from ccrec_amd import fused_bert
    monkeypatch.delenv(SWITCH, raising=False)
    for hidden, heads in ((384, 6), (640, 10), (1920, 30)):
        model = _model("bert", hidden, heads).eval()
        assert fused_bert.unsupported_reason(model) is None
        assert "hidden size" in fused_bert.train_unsupported_reason(model)
        assert "multiples of 256" in fused_bert.train_unsupported_reason(model)
        assert "hidden size" in fused_bert.shadow_unsupported_reason(model)
    assert fused_bert.train_unsupported_reason(_model("bert", 256, 4).eval()) is None
    assert "hidden size" in fused_bert.unsupported_reason(_model("bert", 2176, 34))
    assert "hidden size" in fused_bert.unsupported_reason(_model("bert", 128, 2))


def test_ops_refuses_the_bias_form_and_other_widths_before_it_needs_a_gpu():
    from ccrec_amd import ops
    qkv = torch.zeros(8, 3 * 2 * 32, dtype=torch.bfloat16)
    s = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="rel_bias"):
        ops.attention(qkv, s, s, 2, max_len=8, head_width=32, rel_bias=torch.zeros(2, 15))
    with pytest.raises(ValueError, match="head_width"):
        ops.attention(qkv, s, s, 2, max_len=8, head_width=48)


def test_binding_declares_the_entry_point():
    from ccrec_amd import _lib, ops
    assert "ccr_attention_head_half" in _lib.EXPORTS and _lib.HEAD32_VERSION == 114
    lib = _lib.load()
    assert lib.ccr_version() >= 114 and len(lib.ccr_attention_head_half.argtypes) == 12
    assert callable(ops._require_head32)
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    m = re.search(r"int ccr_attention_head_half\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 12 and "int head_width" in m.group(1)
    args = [a.strip() for a in m.group(1).split(",")]
    assert args.index("int head_width") == args.index("int n_heads") + 1 == args.index("int max_len") - 1


def test_entry_points_check_their_arguments_before_any_device_call():
    """With no GPU in the machine these return their code instead of a HIP error: every check runs before any launch."""
    from ccrec_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * (4096 + 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 4096 bytes of host memory, 16-byte aligned: never dereferenced
    bf16, f16, f32 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32
    inv, ok = _lib.CCR_ERR_INVALID, _lib.CCR_OK

    def att(qkv=p, start=p, lens=p, out=p, n_seq=1, n_heads=2, width=32, max_len=64, pad_len=0, scale=32 ** -0.5, dtype=bf16):
        return lib.ccr_attention_head_half(qkv, start, lens, out, n_seq, n_heads, width, max_len, pad_len, scale, dtype, None)

    for width in (48, 0, 128, -32, 16):
        assert att(width=width) == inv and b"head_width" in lib.ccr_last_error(), width
    assert att(width=48, n_seq=0) == inv      # (the width is checked before the empty batch is waved through)
    assert att(qkv=None) == inv and b"null pointer" in lib.ccr_last_error()
    assert att(start=None) == inv and att(lens=None) == inv and att(out=None) == inv
    for width in (32, 64):
        assert att(width=width, max_len=0) == inv and att(width=width, max_len=513) == inv and att(width=width, n_heads=0) == inv
        assert att(width=width, pad_len=513) == inv and att(width=width, scale=0.0) == inv and att(width=width, dtype=f32) == inv
        assert att(width=width, n_seq=-1) == inv
        assert att(width=width, n_seq=0) == ok and att(width=width, n_seq=0, dtype=f16) == ok

    def ln(dim, rows=0, dtype=bf16):
        return lib.ccr_add_layernorm_half(p, None, p, p, 1e-12, p, None, rows, dim, dtype, None)

    for dim in (256, 384, 640, 1920, 2048):
        assert ln(dim) == ok, dim
    for dim in (320, 2176, 2304, 0, 64, 128, -128):
        assert ln(dim) == inv and b"128" in lib.ccr_last_error(), dim
    assert ln(384, rows=-1) == inv and ln(384, dtype=f32) == inv
    assert lib.ccr_add_layernorm(p, None, p, p, 1e-12, p, None, 0, 384, None) == ok
    assert lib.ccr_add_layernorm(p, None, p, p, 1e-12, p, None, 0, 320, None) == inv

    def emb(dim, rows=0):
        return lib.ccr_embed_layernorm_half(p, 10, p, 10, p, 2, p, p, None, p, p, 1e-12, p, None, rows, dim, bf16, None)

    assert emb(384) == ok and emb(640) == ok and emb(1920) == ok and emb(768) == ok
    assert emb(320) == inv and emb(2176) == inv and emb(0) == inv and emb(128) == inv
    assert lib.ccr_embed_layernorm(p, 10, p, 10, p, 2, p, p, None, p, p, 1e-12, p, None, 0, 384, None) == ok

    # the entry points that read keep bits, and the training block, keep dim % 256 == 0 and say so
    assert lib.ccr_add_layernorm_drop_half(p, p, 1.5, None, p, p, 1e-12, p, None, 0, 384, bf16, None) == inv
    assert b"256" in lib.ccr_last_error() and b"keep-bit" in lib.ccr_last_error()
    assert lib.ccr_add_layernorm_drop_half(p, p, 1.5, None, p, p, 1e-12, p, None, 0, 256, bf16, None) == ok
    assert lib.ccr_embed_layernorm_train_half(p, 10, p, 10, p, 2, p, p, None, p, p, 1e-12, p, 1.5, p, None, 0, 384, bf16, None) == inv
    assert lib.ccr_embed_layernorm_train_half(p, 10, p, 10, p, 2, p, p, None, p, p, 1e-12, None, 1.0, p, None, 0, 384, bf16, None) == inv
    assert lib.ccr_embed_layernorm_train_half(p, 10, p, 10, p, 2, p, p, None, p, p, 1e-12, None, 1.0, p, None, 0, 256, bf16, None) == ok
    assert lib.ccr_add_layernorm_bwd_half(p, None, p, 1e-12, p, p, None, None, None, 0, 384, bf16, None, 0, None) == inv
