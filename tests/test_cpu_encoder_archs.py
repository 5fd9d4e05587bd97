"""The encoder classes beyond BERT that the layer kernels cover (ccrec_amd/fused_bert.py): RobertaModel and XLMRobertaModel (BERT's
layers under another position rule) and MPNetModel (that rule plus one shared relative position bias).  What can be checked without a GPU:
which models are accepted and refused, that the bias table restates the module's compute_position_bias bit for bit, and that the position
rule restates the module's create_position_ids_from_input_ids on right-padded batches and on their packed form.  The GPU side is
tests/test_gpu_encoder_archs.py."""

import re

import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401


def _model(kind, hidden=256, heads=4, layers=1, **extra):
    import transformers
    cfg_cls, cls = {"roberta": (transformers.RobertaConfig, transformers.RobertaModel),
                    "xlmr": (transformers.XLMRobertaConfig, transformers.XLMRobertaModel),
                    "mpnet": (transformers.MPNetConfig, transformers.MPNetModel)}[kind]
    torch.manual_seed(0)
    return cls(cfg_cls(vocab_size=120, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=2 * hidden,
                       max_position_embeddings=514, **extra))


KINDS = ["roberta", "xlmr", "mpnet"]


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_classes_are_accepted_and_the_old_refusals_still_hold(kind):
    from ccrec_amd import fused_bert
    assert fused_bert.unsupported_reason(_model(kind, 256, 4)) is None
    assert fused_bert.unsupported_reason(_model(kind, 768, 12)) is None
    assert "head width" in fused_bert.unsupported_reason(_model(kind, 256, 8))       # head width 32
    assert "hidden size" in fused_bert.unsupported_reason(_model(kind, 192, 3))
    assert "activation" in fused_bert.unsupported_reason(_model(kind, 256, 4, hidden_act="relu"))
    assert "not a BertModel" in fused_bert.unsupported_reason(torch.nn.Linear(4, 4))
    arch = fused_bert._describe(_model(kind, 256, 4, layers=2))
    assert arch.padding_idx == 1 and len(arch.layer_parts(arch.stack.layer[1])) == 8
    assert (arch.bias_source is not None) == (kind == "mpnet") and (arch.type_table is None) == (kind == "mpnet")


@pytest.mark.parametrize("kind", ["roberta", "xlmr"])
def test_decoder_variants_are_refused(kind):
    from ccrec_amd import fused_bert
    assert "decoder" in fused_bert.unsupported_reason(_model(kind, 256, 4, is_decoder=True))


def test_training_is_refused_for_the_relative_bias_and_open_for_roberta(monkeypatch):
    """MPNet: the reason names the bias, in eval mode too, and the 16-bit shadow set refuses the model.  RoBERTa: as BERT -- eval mode or
    zero dropout is accepted, live dropout in training mode is refused with the dropout reason."""
    from ccrec_amd import fused_bert
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN", raising=False)
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", raising=False)
    mp = _model("mpnet").eval()
    assert "relative position bias" in fused_bert.train_unsupported_reason(mp)
    assert "relative position bias" in fused_bert.train_unsupported_reason(mp.train())
    assert "relative position bias" in fused_bert.shadow_unsupported_reason(mp)
    assert "head width" in fused_bert.train_unsupported_reason(_model("mpnet", 256, 8))      # (the inference refusal comes first)
    for kind in ("roberta", "xlmr"):
        wet = _model(kind)
        assert fused_bert.train_unsupported_reason(wet.eval()) is None
        assert "dropout" in fused_bert.train_unsupported_reason(wet.train())
        dry = _model(kind, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0).train()
        assert fused_bert.train_unsupported_reason(dry) is None and fused_bert.shadow_unsupported_reason(dry) is None


@pytest.mark.parametrize("L", [1, 9, 130, 512])
def test_relative_bias_table_is_compute_position_bias_bit_for_bit(L):
    from ccrec_amd import fused_bert
    model = _model("mpnet", 256, 4)
    with torch.no_grad():
        model.encoder.relative_attention_bias.weight.normal_(0.0, 1.0)
        want = model.encoder.compute_position_bias(torch.zeros(1, L, 256))[0]      # [heads, L, L], query x key
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    for R in (L - 1, 511):
        table = fused_bert.relative_bias_table(model, R)
        assert table.dtype == torch.float32 and tuple(table.shape) == (4, 2 * R + 1) and table.is_contiguous()
        window = table[:, R - (L - 1):R + L]
        assert torch.equal(window[:, (j - i) + L - 1], want)
    if L == 512:      # the rule has 32 buckets, 31 of them reachable inside 512 tokens
        buckets = model.encoder.relative_position_bucket(torch.arange(-511, 512))
        assert buckets.unique().numel() == 31
    assert fused_bert.relative_bias_table(model).shape[1] == 2 * fused_bert.REL_SPAN + 1 == 1023


def _padded_batch(pad):
    """Right-padded ids [5, 12]: padding holds the pad id; row 1's live part holds a pad-id token, row 2 has length 1, row 3 is full and
    starts with the pad id."""
    lens = [7, 9, 1, 12, 4]
    g = torch.Generator().manual_seed(3)
    ids = torch.full((len(lens), 12), pad, dtype=torch.int64)
    for r, n in enumerate(lens):
        ids[r, :n] = torch.randint(pad + 1, 120, (n,), generator=g)
    ids[1, 4] = pad
    ids[3, 0] = pad
    return ids, lens


@pytest.mark.parametrize("kind", KINDS)
def test_position_rule_equals_the_module_function_padded_and_packed(kind):
    from ccrec_amd import fused_bert
    model = _model(kind)
    pad = fused_bert._describe(model).padding_idx
    if kind == "mpnet":
        from transformers.models.mpnet.modeling_mpnet import create_position_ids_from_input_ids as module_rule
    else:
        module_rule = model.embeddings.create_position_ids_from_input_ids
    ids, lens = _padded_batch(pad)
    want = module_rule(ids, pad)
    B, L = ids.shape
    got = fused_bert.position_rows(ids.flatten(), torch.arange(L).repeat(B), pad).view(B, L)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert want[1, 4] == pad and want[1, 5] == pad + 5 and want[2, 0] == pad + 1 and want[3, 0] == pad and want[3, 1] == pad + 1
    live = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    c_of = torch.arange(L).repeat(B)[live.flatten()]      # the packed form: only the real tokens, their in-sequence positions
    packed = fused_bert.position_rows(ids[live], c_of, pad)
    assert torch.equal(packed, want[live])
    # a mutant that starts at padding_idx instead of padding_idx + 1 differs on every live token
    assert not torch.equal(packed - 1, want[live])


def test_bert_keeps_in_sequence_positions():
    from transformers import BertConfig, BertModel
    from ccrec_amd import fused_bert
    arch = fused_bert._describe(BertModel(BertConfig(vocab_size=50, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                                                     intermediate_size=512)))
    assert arch.padding_idx is None and arch.bias_source is None


def test_one_row_type_table_leaves_token_type_ids_to_the_module():
    """RoBERTa checkpoints ship a one-row type table: its row is added as the module adds it, and a batch that carries token_type_ids
    keeps the module (item_tower reads has_token_types), which raises on a nonzero id where a kernel could only clamp it."""
    from transformers import BertConfig, BertModel
    from ccrec_amd.fused_bert import FusedBertEncoder
    assert FusedBertEncoder(_model("roberta", type_vocab_size=1)).has_token_types is False
    assert FusedBertEncoder(_model("xlmr", type_vocab_size=2)).has_token_types is True
    assert FusedBertEncoder(_model("mpnet")).has_token_types is False
    assert FusedBertEncoder(BertModel(BertConfig(vocab_size=50, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                                                 intermediate_size=512))).has_token_types is True


def test_binding_declares_the_entry_point():
    import os
    from ccrec_amd import _lib, ops
    assert "ccr_attention_bias_half" in _lib.EXPORTS and _lib.ATTENTION_BIAS_VERSION == 112
    lib = _lib.load()
    assert lib.ccr_version() >= 112 and len(lib.ccr_attention_bias_half.argtypes) == 13
    assert callable(ops._require_attention_bias)
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    m = re.search(r"int ccr_attention_bias_half\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 13 and "const float *rel_bias" in m.group(1) and "int R" in m.group(1)
