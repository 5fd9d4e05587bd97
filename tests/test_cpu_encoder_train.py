"""The encoder layer kernels' training entry points (library version 103) without a GPU: the C ABI and its binding agree, the version
gate of ops works, the training path's gating logic runs on CPU-built models, and every entry point rejects bad arguments before it
makes a device call."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

TRAIN_EXPORTS = ["ccr_attention_fwd_train_half", "ccr_attention_bwd_workspace_bytes", "ccr_attention_bwd_half", "ccr_add_layernorm_bwd_half",
                 "ccr_gelu_bwd_half"]


def test_the_five_entry_points_are_declared_bound_and_exported():
    from ccrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    declared = set(re.findall(r"\b(ccr_[a-z0-9_]+)\s*\(", header)) - {"ccr_index", "ccr_search_stats"}
    assert declared == set(_lib.EXPORTS)
    lib = _lib.load()
    for name in TRAIN_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name      # one ctypes type per C parameter
        assert re.search(name + r" \((?:bbpr\.py:195-197|bert_mt\.py:105-113)", header), name   # each cites the reference lines it serves
    assert lib.ccr_attention_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert lib.ccr_version() >= _lib.ENCODER_TRAIN_VERSION == 103
    assert _lib.MIN_VERSION == 101 and _lib.BPR_VERSION == 102


def test_require_encoder_train_rejects_an_older_library(monkeypatch):
    from ccrec_amd import _lib, ops
    lib = _lib.load()

    class Old:
        def ccr_version(self):
            return 102

    monkeypatch.setattr(ops, "_ENCODER_TRAIN_CHECKED", False)
    monkeypatch.setattr(ops, "require_gpu", lambda: Old())
    with pytest.raises(_lib.CcrError, match="version 102.*need 103"):
        ops._require_encoder_train()
    assert ops._ENCODER_TRAIN_CHECKED is False
    monkeypatch.setattr(ops, "require_gpu", lambda: lib)
    assert ops._require_encoder_train() is lib and ops._ENCODER_TRAIN_CHECKED is True


def test_training_path_gating_on_cpu_models(monkeypatch):
    """fused_bert.train_unsupported_reason / train_wanted / train_dtype, and the tower's hook, on CPU-built models."""
    from transformers import BertConfig, BertModel, DistilBertConfig, DistilBertModel
    from ccrec_amd import fused_bert
    from ccrec_amd.item_tower import NaiveItemTower

    def bert(hidden=256, heads=4, p=0.0):
        return BertModel(BertConfig(vocab_size=50, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=heads, intermediate_size=512,
                                    max_position_embeddings=32, hidden_dropout_prob=p, attention_probs_dropout_prob=p))

    dry, wet = bert(), bert(p=0.1)
    assert fused_bert.train_unsupported_reason(dry.train()) is None and fused_bert.train_unsupported_reason(dry.eval()) is None
    assert "dropout" in fused_bert.train_unsupported_reason(wet.train())
    assert fused_bert.train_unsupported_reason(wet.eval()) is None                       # dropout is inactive in eval mode
    assert fused_bert.unsupported_reason(wet.train()) is None                            # the inference check is unchanged
    assert "head width" in fused_bert.train_unsupported_reason(bert(256, 8))            # ... and its reasons carry over
    half_wet = bert()
    half_wet.encoder.layer[0].output.dropout.p = 0.3                                     # one live Dropout module is enough
    assert "dropout" in fused_bert.train_unsupported_reason(half_wet.train())
    dist_wet = DistilBertModel(DistilBertConfig(vocab_size=50, dim=256, n_layers=1, n_heads=4, hidden_dim=512, dropout=0.0, attention_dropout=0.1))
    assert "attention_dropout" in fused_bert.train_unsupported_reason(dist_wet.train())
    dist_dry = DistilBertModel(DistilBertConfig(vocab_size=50, dim=256, n_layers=1, n_heads=4, hidden_dim=512, dropout=0.0, attention_dropout=0.0))
    assert fused_bert.train_unsupported_reason(dist_dry.train()) is None

    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN", raising=False)
    assert fused_bert.train_wanted() is False
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "0")
    assert fused_bert.train_wanted() is False
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    assert fused_bert.train_wanted() is True
    assert fused_bert.train_dtype() is None                                              # no CUDA autocast context here
    monkeypatch.setenv("CCREC_FUSED_ENCODER", "1")                                       # the inference knob does not name a training type
    assert fused_bert.train_dtype() is None
    assert fused_bert.kernel_dtype("auto") is torch.bfloat16                             # ... and the training knob leaves kernel_dtype alone
    monkeypatch.delenv("CCREC_FUSED_ENCODER")

    # the tower: gradients on -> the module, whatever the variable says on a machine without an autocast context
    tower = NaiveItemTower(dry.train(), torch.nn.LayerNorm(256, elementwise_affine=False))
    inputs = {"input_ids": torch.tensor([[1, 2, 3, 0]]), "attention_mask": torch.tensor([[1, 1, 1, 0]])}
    for value in (None, "1"):
        if value is None:
            monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN")
        else:
            monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", value)
        assert torch.is_grad_enabled() and tower._encode_on_kernels(inputs) is None
    out = tower(**inputs, input_step="inputs", output_step="cls")
    assert out.requires_grad and out.shape == (1, 256)


def test_entry_points_reject_bad_arguments_before_any_device_call():
    """The argument checks come first: with no GPU in the machine these return their error code instead of a HIP error."""
    from ccrec_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * (4096 + 16))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 4096 bytes of host memory, 16-byte aligned: never dereferenced
    bf16, f16, f32 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32
    inv, wsp = _lib.CCR_ERR_INVALID, _lib.CCR_ERR_WORKSPACE

    def fwd(lse=p, n_heads=2, max_len=64, pad_len=0, scale=0.125, dtype=bf16, qkv=p):
        return lib.ccr_attention_fwd_train_half(qkv, p, p, p, lse, 1, n_heads, max_len, pad_len, scale, dtype, None)

    assert fwd(lse=None) == inv and b"null pointer" in lib.ccr_last_error()
    assert fwd(qkv=None) == inv and fwd(max_len=513) == inv and fwd(max_len=0) == inv and fwd(pad_len=513) == inv
    assert fwd(n_heads=0) == inv and fwd(scale=0.0) == inv and fwd(dtype=f32) == inv and b"half_dtype" in lib.ccr_last_error()

    assert lib.ccr_attention_bwd_workspace_bytes(3, 12, 200) == 3 * 12 * 224 * 4        # one fp32 per query (rounded up to 32) and head
    assert lib.ccr_attention_bwd_workspace_bytes(1, 1, 512) == 2048 and lib.ccr_attention_bwd_workspace_bytes(0, 1, 1) > 0
    assert lib.ccr_attention_bwd_workspace_bytes(1, 1, 513) == 0 and b"max_len=513" in lib.ccr_last_error()
    assert lib.ccr_attention_bwd_workspace_bytes(1, 0, 64) == 0 and lib.ccr_attention_bwd_workspace_bytes(-1, 1, 64) == 0

    def bwd(qkv=p, d_qkv=p, ws=p, n_heads=2, max_len=64, pad_len=0, scale=0.125, dtype=f16, ws_bytes=4096):
        return lib.ccr_attention_bwd_half(qkv, p, p, p, p, p, d_qkv, 1, n_heads, max_len, pad_len, scale, dtype, ws, ws_bytes, None)

    assert bwd(qkv=None) == inv and bwd(d_qkv=None) == inv and bwd(ws=None) == inv
    assert bwd(max_len=513) == inv and bwd(pad_len=-1) == inv and bwd(n_heads=2000) == inv and bwd(scale=-1.0) == inv and bwd(dtype=f32) == inv
    assert bwd(ws_bytes=2 * 64 * 4 - 1) == wsp and b"workspace" in lib.ccr_last_error()

    def ln(x=p, gamma=p, d_y=p, rows=8, dim=256, dtype=bf16, ws=p, ws_bytes=4096, d_gamma=p):
        return lib.ccr_add_layernorm_bwd_half(x, None, gamma, 1e-12, d_y, p, None, d_gamma, None, rows, dim, dtype, ws, ws_bytes, None)

    assert ln(x=None) == inv and ln(gamma=None) == inv and ln(d_y=None) == inv
    assert ln(dim=320) == inv and ln(dim=2304) == inv and ln(dim=0) == inv and ln(rows=-1) == inv and ln(dtype=f32) == inv
    assert ln(ws_bytes=2 * 2 * 256 * 4 - 1) == wsp and ln(ws=None, ws_bytes=0) == wsp      # d_gamma asked for: two workgroups' column sums
    assert ln(rows=0, d_gamma=None, ws=None, ws_bytes=0) == _lib.CCR_OK                    # nothing to do needs no workspace

    def gelu(x=p, d_y=p, d_x=p, n=64, dtype=bf16):
        return lib.ccr_gelu_bwd_half(x, d_y, d_x, n, dtype, None)

    assert gelu(x=None) == inv and gelu(d_y=None) == inv and gelu(d_x=None) == inv and gelu(n=60) == inv and gelu(n=-8) == inv
    assert gelu(dtype=f32) == inv and gelu(d_x=ctypes.c_void_p(p.value + 8)) == inv and gelu(n=0) == _lib.CCR_OK
