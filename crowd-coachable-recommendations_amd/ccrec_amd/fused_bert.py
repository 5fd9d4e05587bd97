"""The item tower's encoder forward, layer by layer on this library's kernels (encoder-side fusion).

The reference encodes with transformers' BertModel under autocast (src/ccrec/models/item_tower.py:122
`cls_model(**inputs).last_hidden_state`; scripts/al_0_rank.py:92-101,125).  Run as torch modules on one MI355X that forward
spends 38 % of its GPU time in the projections (hipBLASLt, already at library speed), 22 % in the attention call (57 TFLOP/s at
these sequence lengths) and 30 % in separate residual-add / LayerNorm / dtype-cast passes (profiles/r03_encode_kernel_stats.csv).
FusedBertEncoder keeps the projections as library GEMMs (torch.nn.functional.linear on 16-bit weights: one stacked Q|K|V
projection instead of three) and replaces the rest with ccr_attention_half and ccr_add_layernorm_half (csrc/ccr_encoder.hip).

Arithmetic: what autocast does in the reference's layer -- 16-bit projection operands and outputs, fp32 attention scores and
softmax, fp32 residual stream and LayerNorm -- IN THE AUTOCAST CONTEXT'S OWN 16-BIT TYPE (kernel_dtype): fp16 under the reference's
`torch.cuda.amp.autocast()` (scripts/al_0_rank.py:8,125: the CUDA default), bf16 under autocast(dtype=torch.bfloat16).  The hidden
states agree with the module forward under the same autocast to that type's rounding (the tests compare both with the fp32 forward).
forward / forward_packed are inference forwards (eval mode, no autograd); forward_train / forward_train_packed run the same layers with
gradients on, on the kernels' backward (ops.attention_train, add_layernorm_train, gelu_train).  Dropout there is a second opt-in
(CCREC_FUSED_ENCODER_TRAIN_DROPOUT=1, train_dropout_wanted): a model in train() with live dropout then runs on the same kernels reading
packed keep bits that a generator kernel writes from one 64-bit seed per call (ops.dropout_bits_rows / dropout_bits_attention, restated on
the CPU in dropout_ref); without that opt-in such a model is refused and keeps training as its torch module.

Only what the kernels cover is accepted (unsupported_reason): post-LayerNorm layers with exact GELU, head width 64 (32 as well with
CCREC_FUSED_ENCODER_HEAD32=1, head32_wanted: the MiniLM-class encoders, inference only), hidden size a multiple of 128 from 256 on (the training
kernels: of 256), at most 512 tokens, right-padded batches, in one of these transformers classes:

  BertModel, DistilBertModel       absolute positions: the position row of a token is its index inside its sequence;
  RobertaModel, XLMRobertaModel    BERT's layers; the position row is padding_idx + the number of non-pad ids up to and including the
                                   token, and padding_idx itself for a pad-id token (position_rows); the module's own type table;
  MPNetModel                       the same position rule, no token types, and one relative position bias shared by every layer, added to
                                   the scaled attention scores (relative_bias_table, ops.attention(rel_bias=...)).  Inference only: the
                                   bias table's gradient has no kernel, so MPNet trains as its torch module (train_unsupported_reason).

The reference builds its tower with AutoModel.from_pretrained(MODEL_NAME) (src/ccrec/models/bbpr.py:30, bert_mt.py:74), so any of them
can arrive.  Every other encoder keeps running as its own torch module -- LengthSortedEncoder picks per model."""
import collections
import os
import threading

import torch
import torch.nn.functional as F

from . import ops


class _Arch:
    """Where a supported architecture keeps the pieces of its (post-LayerNorm, GELU) encoder layer."""

    def __init__(self, heads, hidden, activation, stack, embeddings, type_table, layer_parts, dropout_parts, padding_idx=None,
                 bias_source=None):
        self.heads, self.hidden, self.activation = heads, hidden, activation
        self.stack = stack                    # the module whose parameters are the layers' weights
        self.embeddings, self.type_table = embeddings, type_table
        self.layer_parts = layer_parts        # layer module -> (q, k, v, attention out, LayerNorm 1, ffn in, ffn out, LayerNorm 2)
        self.dropout_parts = dropout_parts    # layer module -> the Dropout modules on (probabilities, attention output or None, ffn output)
        self.padding_idx = padding_idx        # the position rule: None = a token's position row is its in-sequence index; an int = position_rows
        self.bias_source = bias_source        # None, or the module with relative_attention_bias / relative_position_bucket (relative_bias_table)


_BERT_LAYER_PARTS = (lambda m: (m.attention.self.query, m.attention.self.key, m.attention.self.value, m.attention.output.dense,
                                m.attention.output.LayerNorm, m.intermediate.dense, m.output.dense, m.output.LayerNorm),
                     lambda m: (m.attention.self.dropout, m.attention.output.dropout, m.output.dropout))


def _describe(model):
    """-> _Arch for a transformers BertModel or DistilBertModel (the reference's encoders: facebook/contriever and bert-base-uncased are
    BertModels, src/ccrec/models/bbpr.py:334, scripts/al_0_rank.py:120; distilbert-base-uncased is its default model_name,
    bbpr.py:50, bert_mt.py:35), a RobertaModel, XLMRobertaModel or MPNetModel (what --MODEL_NAME brings in: bbpr.py:30, bert_mt.py:74), or a
    string saying why the class is not covered."""
    name, cfg = type(model).__name__, getattr(model, "config", None)
    if name in ("BertModel", "RobertaModel", "XLMRobertaModel") and hasattr(model, "embeddings") and hasattr(model, "encoder"):
        if getattr(cfg, "position_embedding_type", None) not in (None, "absolute"):
            return f"position_embedding_type {cfg.position_embedding_type!r}"
        if getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False):
            return "decoder / cross-attention layers"
        e = model.embeddings
        return _Arch(int(cfg.num_attention_heads), int(cfg.hidden_size), getattr(cfg, "hidden_act", "gelu"), model.encoder, e,
                     e.token_type_embeddings.weight, *_BERT_LAYER_PARTS,
                     padding_idx=None if name == "BertModel" else int(e.padding_idx))
    if name == "MPNetModel" and hasattr(model, "embeddings") and hasattr(model, "encoder"):
        e = model.embeddings
        return _Arch(int(cfg.num_attention_heads), int(cfg.hidden_size), getattr(cfg, "hidden_act", "gelu"), model.encoder, e, None,
                     lambda m: (m.attention.attn.q, m.attention.attn.k, m.attention.attn.v, m.attention.attn.o, m.attention.LayerNorm,
                                m.intermediate.dense, m.output.dense, m.output.LayerNorm),
                     lambda m: (m.attention.attn.dropout, m.attention.dropout, m.output.dropout),
                     padding_idx=int(e.padding_idx), bias_source=model.encoder)
    if name == "DistilBertModel" and hasattr(model, "embeddings") and hasattr(model, "transformer"):
        return _Arch(int(cfg.n_heads), int(cfg.dim), getattr(cfg, "activation", "gelu"), model.transformer, model.embeddings, None,
                     lambda m: (m.attention.q_lin, m.attention.k_lin, m.attention.v_lin, m.attention.out_lin, m.sa_layer_norm,
                                m.ffn.lin1, m.ffn.lin2, m.output_layer_norm),
                     lambda m: (m.attention.dropout, None, m.ffn.dropout))      # (nothing between out_lin and sa_layer_norm)
    return f"{name} is not a BertModel, DistilBertModel, RobertaModel, XLMRobertaModel or MPNetModel"


def position_rows(token_ids, positions, padding_idx):
    """The position-table rows of a flat token array under RoBERTa's rule (transformers' create_position_ids_from_input_ids, restated for
    arrays whose sequences lie one after another): padding_idx + the number of non-pad ids among the tokens of the same sequence up to and
    including this one, and padding_idx itself where the id is padding_idx.  token_ids, positions: int64 [T]; positions = each token's
    0-based index inside its sequence, so row - position is the row of its sequence's first token -- true of a flattened right-padded
    batch (positions = 0 .. L-1 per row) and of a packed array alike."""
    live = token_ids.ne(padding_idx).to(torch.int64)
    upto = torch.cumsum(live, 0)
    before = upto - live      # non-pad ids in front of each row, over the whole array
    first = torch.arange(token_ids.numel(), device=token_ids.device) - positions
    return (upto - before[first]) * live + padding_idx


REL_SPAN = 511      # the span the encoder's bias table is built for: every offset of a 512-token sequence, one table for every batch


def relative_bias_table(model, R=REL_SPAN):
    """MPNetEncoder.compute_position_bias as a table: fp32 [heads, 2 R + 1] on the parameters' device, entry [h, R + d] = the bias of head h
    for key - query = d, from the model's own relative_position_bucket and relative_attention_bias.  The bias of a (query, key) pair depends
    on nothing else, so table[:, R - (L-1) : R + L][:, (j - i) + L - 1] is compute_position_bias for L tokens, bit for bit."""
    arch = _describe(model)
    assert not isinstance(arch, str) and arch.bias_source is not None, "the model has no relative position bias"
    src = arch.bias_source
    with torch.no_grad():
        offsets = torch.arange(-int(R), int(R) + 1, dtype=torch.long)      # (on the CPU, where compute_position_bias takes its buckets)
        buckets = src.relative_position_bucket(offsets).to(src.relative_attention_bias.weight.device)
        return src.relative_attention_bias(buckets).t().float().contiguous()


def _bias_train_reason(arch):
    if arch.bias_source is not None:
        return ("the relative position bias (relative_attention_bias) has no gradient on the layer kernels: "
                "the attention backward takes no bias, so this encoder trains as its torch module")
    return None


def _train_shape_reason(arch):
    """Why the TRAINING kernels (forward with a backward, keep bits) cannot take an architecture the inference kernels can: they are built
    for head width 64 and for rows of 256 C elements only."""
    heads, hidden = arch.heads, arch.hidden
    if hidden % heads or hidden // heads != 64:
        return f"head width {hidden / heads:g} (the training attention kernels are built for 64: this encoder trains as its torch module)"
    if hidden % 256 or hidden > 2048:
        return f"hidden size {hidden} (the training kernels take multiples of 256 up to 2048: this encoder trains as its torch module)"
    return None


def _train_reason(model):
    """unsupported_reason, then what only the training kernels refuse."""
    reason = unsupported_reason(model)
    if reason is not None:
        return reason
    arch = _describe(model)
    return _train_shape_reason(arch) or _bias_train_reason(arch)


def shadow_unsupported_reason(model):
    """None when an optimizer may keep a 16-bit weight set of `model` current for the training forward (optim.FusedAdamW(shadow_for=...)):
    what unsupported_reason asks, and an encoder the kernels can train."""
    return _train_reason(model)


def head32_wanted():
    """The opt-in of the head-width-32 attention kernel: CCREC_FUSED_ENCODER_HEAD32=1, read at call time (default off: a model with
    32-wide heads -- the MiniLM-class encoders, hidden 384 with 12 heads -- keeps running as its torch module)."""
    return os.environ.get("CCREC_FUSED_ENCODER_HEAD32", "").strip() == "1"


def unsupported_reason(model):
    """None when FusedBertEncoder can run `model` (one of the transformers classes _describe knows); otherwise why not."""
    arch = _describe(model)
    if isinstance(arch, str):
        return arch
    heads, hidden = arch.heads, arch.hidden
    width = hidden // heads if hidden % heads == 0 else None
    if width == 32 and head32_wanted():
        if arch.bias_source is not None:
            return "head width 32 with a relative position bias (the bias form of the attention kernel is built for head width 64 only)"
    elif width != 64:
        return f"head width {hidden / heads:g} (the attention kernel is built for 64)"
    if hidden % 128 or hidden < 256 or hidden > 2048:
        return f"hidden size {hidden} (the LayerNorm kernel takes multiples of 128 from 256 to 2048)"
    if arch.activation != "gelu":
        return f"activation {arch.activation!r} (exact GELU only)"
    return None


_DROPOUT_FIELDS = ("hidden_dropout_prob", "attention_probs_dropout_prob", "dropout", "attention_dropout")


def _dropout_sites(model):
    """The Dropout modules the kernels' training path knows how to replace: the one after the embedding LayerNorm and, per layer, those on
    the attention probabilities, the attention output (BERT only) and the FFN output.  -> the set of their ids."""
    arch = _describe(model)
    known = [getattr(arch.embeddings, "dropout", None)]
    for mod in arch.stack.layer:
        known.extend(arch.dropout_parts(mod))
    return {id(m) for m in known if m is not None}


def _live(m):
    """Is this module a dropout torch would apply right now?  (Its own training flag counts: a Dropout put in eval() inside a train() model
    is inactive.)"""
    return isinstance(m, torch.nn.Dropout) and m.training and m.p > 0


def _dropout_refusal(model):
    """With both opt-ins set: None if every live Dropout module of a model in training mode is a known site with p < 1; else why not."""
    known = _dropout_sites(model)
    for name, m in model.named_modules():
        if _live(m):
            if id(m) not in known:
                return f"dropout module {name or 'model'} (p={m.p:g}) is active in training mode and is not a site the layer kernels cover"
            if not m.p < 1:
                return f"dropout module {name} has p={m.p:g}: the keep bits take 0 <= p < 1"
    return None


def train_unsupported_reason(model):
    """None when FusedBertEncoder can run a TRAINING forward of `model`: what unsupported_reason asks, and no active dropout: a model in
    training mode with any dropout probability above 0 is refused; eval mode or all-zero dropout is fine.  With the second opt-in
    (train_wanted() and train_dropout_wanted()) active dropout is accepted where every live torch.nn.Dropout module is one of the known
    sites (_dropout_sites: their p is read from the modules at call time); any other live Dropout module is refused by name."""
    reason = _train_reason(model)
    if reason is not None:
        return reason
    if getattr(model, "training", False) and train_wanted() and train_dropout_wanted():
        return _dropout_refusal(model)
    if getattr(model, "training", False):
        cfg = getattr(model, "config", None)
        active = [f"{name}={float(getattr(cfg, name)):g}" for name in _DROPOUT_FIELDS if float(getattr(cfg, name, 0.0) or 0.0) > 0.0]
        active += [f"{name or 'model'}.p={m.p:g}" for name, m in model.named_modules() if isinstance(m, torch.nn.Dropout) and m.p > 0]
        if active:
            return f"dropout is active in training mode ({', '.join(active[:3])}): the layer kernels have no dropout"
    return None


def train_wanted():
    """The opt-in of the training path: CCREC_FUSED_ENCODER_TRAIN=1 (default off: the torch module trains)."""
    return os.environ.get("CCREC_FUSED_ENCODER_TRAIN", "").strip() == "1"


def train_dropout_wanted():
    """The opt-in of dropout on the training path: CCREC_FUSED_ENCODER_TRAIN_DROPOUT=1, read at call time (default off: a model with
    active dropout trains as its torch module).  Honoured only together with CCREC_FUSED_ENCODER_TRAIN=1."""
    return os.environ.get("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "").strip() == "1"


def train_packed_wanted():
    """The opt-in of the training path's embedding block and packed pooling on kernels: CCREC_FUSED_ENCODER_TRAIN_PACKED=1, read at call
    time (default off: _embed_train is the torch sum, the tower pools a padded tensor).  Honoured only together with
    CCREC_FUSED_ENCODER_TRAIN=1."""
    return train_wanted() and os.environ.get("CCREC_FUSED_ENCODER_TRAIN_PACKED", "").strip() == "1"


SITE_PROBABILITIES, SITE_ATTENTION_OUTPUT, SITE_FFN_OUTPUT = 0, 1, 2
EMBEDDINGS_STREAM = 0


def dropout_stream(layer, site):
    """The generator's stream id of a layer's dropout site: 4 * layer + site, plus one for the embeddings' (EMBEDDINGS_STREAM = 0).  The
    cls_only last layer draws its row-wise bits for the rows it runs on (one per sequence) under layer = the number of layers."""
    return 4 * int(layer) + int(site) + 1


def draw_seed():
    """One 64-bit seed from torch's default CPU generator (torch.manual_seed makes a step reproducible; no device sync)."""
    lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


class _DropoutDraw:
    """The dropout decisions of one training forward: every site's keep bits come from (seed, the site's stream id)."""

    def __init__(self, seed):
        from . import dropout_ref
        self.seed, self._ref = seed, dropout_ref

    def rows(self, module, stream, rows, dim, device):
        """-> (bits, inv_keep) of a row-wise site, or (None, 1.0) when its module is absent or has p = 0 (not a dropout site)."""
        p = float(module.p) if module is not None and _live(module) else 0.0
        if p <= 0.0:
            return None, 1.0
        return ops.dropout_bits_rows(rows, dim, self.seed, stream, p, device=device), self._ref.inv_keep(p)

    def attention(self, module, stream, seq_start, lengths, n_tokens, heads, max_len):
        p = float(module.p) if module is not None and _live(module) else 0.0
        if p <= 0.0:
            return None, 1.0
        return ops.dropout_bits_attention(seq_start, lengths, n_tokens, heads, max_len, self.seed, stream, p), self._ref.inv_keep(p)


def _autocast_dtype():
    """Inside a CUDA autocast context: the context's own type; outside one: None."""
    if torch.cuda.is_available() and torch.is_autocast_enabled("cuda"):
        return torch.get_autocast_dtype("cuda")
    return None


def train_dtype():
    """The 16-bit operand type of a training forward on the kernels = the CUDA autocast context's own type when that is fp16 or bf16;
    None (the module trains) outside autocast or under any other type."""
    dtype = _autocast_dtype()
    return dtype if dtype in (torch.float16, torch.bfloat16) else None


_ENV_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16, "half": torch.float16}


def kernel_dtype(explicit="auto"):
    """The 16-bit operand type an inference forward should run the layer kernels in, or None = run the torch module.

    Inside a CUDA autocast context it is the context's own type (torch.get_autocast_dtype): torch.float16 under the reference's
    `with torch.cuda.amp.autocast():` (scripts/al_0_rank.py:125), torch.bfloat16 under autocast(dtype=torch.bfloat16); any other
    autocast type keeps the module.  Outside autocast the caller asked for an fp32 forward and gets the fp32 module -- unless
    explicit is True or CCREC_FUSED_ENCODER=1 demands the kernels, which then run in CCREC_FUSED_ENCODER_DTYPE (bf16 | fp16, default bf16).
    explicit False or CCREC_FUSED_ENCODER=0: always None."""
    env = os.environ.get("CCREC_FUSED_ENCODER", "").strip()
    if explicit is False or (explicit is not True and env == "0"):
        return None
    dtype = _autocast_dtype()
    if dtype is not None:
        return dtype if dtype in (torch.float16, torch.bfloat16) else None
    if explicit is True or env == "1":
        name = os.environ.get("CCREC_FUSED_ENCODER_DTYPE", "bf16").strip().lower()
        assert name in _ENV_DTYPES, f"CCREC_FUSED_ENCODER_DTYPE={name!r}: bf16 or fp16"
        return _ENV_DTYPES[name]
    return None


def wanted(explicit="auto"):
    """Should an inference forward take the kernel path?  (kernel_dtype says in which 16-bit type.)"""
    return kernel_dtype(explicit) is not None


_SLOT = "_ccr_fused_encoder"        # the encoder lives in its model's __dict__: model <-> encoder is an ordinary cycle the GC collects
_SLOT_LOCK = threading.Lock()      # DataParallel runs its replicas' forwards on threads


def for_model(model):
    """The FusedBertEncoder of `model` (one per module object, built on first use), or None if the kernels do not cover it.
    torch's replicate() copies a module's __dict__ shallowly, so a DataParallel replica arrives holding its ORIGINAL's encoder:
    an encoder that belongs to another module object is replaced by one of the replica's own (its weights sit on the replica's device)."""
    if not isinstance(model, torch.nn.Module):      # a stand-in encoder (tests, wrappers): never covered
        return None
    with _SLOT_LOCK:
        enc = model.__dict__.get(_SLOT, False)
        if enc is False or (enc is not None and enc.model is not model):
            enc = FusedBertEncoder(model) if unsupported_reason(model) is None else None
            model.__dict__[_SLOT] = enc
        elif _head_width_32(model):      # the one answer that a switch read at call time can change (head32_wanted): asked again per call
            if unsupported_reason(model) is not None:
                return None      # (an encoder built while the switch was on stays in its slot, unused)
            if enc is None:
                enc = model.__dict__[_SLOT] = FusedBertEncoder(model)
        return enc


def _head_width_32(model):
    arch = _describe(model)
    return not isinstance(arch, str) and arch.heads > 0 and arch.hidden == 32 * arch.heads


def prefix_lengths(attention_mask):
    """int32 [B] token counts if every row of the 0/1 mask is ones followed by zeros with at least one token (right padding: what
    the tokenizers of the reference's models produce); None otherwise.  One small reduction + a host read per batch."""
    m = attention_mask
    if m.dim() != 2 or m.shape[1] == 0 or m.shape[1] > 512:
        return None
    lengths = m.sum(dim=1)
    L = m.shape[1]
    ok = ((m != 0) == (torch.arange(L, device=m.device)[None, :] < lengths[:, None])).all() & (lengths > 0).all()
    return lengths.to(torch.int32) if bool(ok) else None


_Batch = collections.namedtuple("_Batch", "B L ids positions types seq_start max_len pad_len keep")      # FusedBertEncoder._layout


class _Layer:
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "g1", "b1", "eps1", "wi", "bi", "wo2", "bo2", "g2", "b2", "eps2")


_LAYER_16BIT = ("wqkv", "bqkv", "wo", "bo", "wi", "bi", "wo2", "bo2")      # a layer's 16-bit copies (the LayerNorm tensors are the fp32 masters)
_LAYER_FP32 = ("g1", "b1", "eps1", "g2", "b2", "eps2")


_DEFERRED = object()      # FusedBertEncoder._signature after a maintained step: taken at the next refresh() (adopted_stepped)


class _NoGradRow(torch.autograd.Function):
    """A table one of whose rows receives no gradient, as torch.nn.Embedding(padding_idx=row) trains it: forward hands out the table
    itself, backward clears that row of the incoming gradient."""

    @staticmethod
    def forward(ctx, table, row):
        ctx.row = int(row)
        return table.view_as(table)

    @staticmethod
    def backward(ctx, grad):
        grad = grad.clone()
        grad[ctx.row] = 0
        return grad, None


def _padding_rows(arch):
    """(word table's, position table's) padding_idx where the training forward honours it (the architectures with a position rule: a
    pad-id token can be a live one there, and the module gives its rows no gradient), else (None, None)."""
    if arch.padding_idx is None:
        return None, None
    return arch.embeddings.word_embeddings.padding_idx, arch.embeddings.position_embeddings.padding_idx


class _ShadowWeights(torch.autograd.Function):
    """A layer's maintained 16-bit weights in the place of cat(q, k, v).to(half) and the seven other casts: forward hands out the eight
    copies an optimizer keeps current (optim.FusedAdamW), backward returns each incoming 16-bit gradient as fp32 to its masters -- wqkv's
    and bqkv's row-sliced into the three projections' -- the values the cast graph gives.  One node per layer."""

    @staticmethod
    def forward(ctx, layer, *masters):      # masters: the layer's twelve weights and biases in _live_masters' order
        ctx.rows = masters[0].shape[0]
        return tuple(getattr(layer, name).detach() for name in _LAYER_16BIT)

    @staticmethod
    def backward(ctx, g_wqkv, g_bqkv, g_wo, g_bo, g_wi, g_bi, g_wo2, g_bo2):
        r = ctx.rows
        w = None if g_wqkv is None else g_wqkv.float()
        b = None if g_bqkv is None else g_bqkv.float()
        qkv_w = (None, None, None) if w is None else (w[:r], w[r:2 * r], w[2 * r:])
        qkv_b = (None, None, None) if b is None else (b[:r], b[r:2 * r], b[2 * r:])
        rest = tuple(None if g is None else g.float() for g in (g_wo, g_bo, g_wi, g_bi, g_wo2, g_bo2))
        return (None, *qkv_w, *qkv_b, *rest)


class FusedBertEncoder:
    """16-bit (bf16 or fp16: the `dtype` of each call) forward of a transformers BertModel / DistilBertModel / RobertaModel /
    XLMRobertaModel / MPNetModel: forward(input_ids [B, L]
    right-padded, lengths [B]) -> last hidden state fp32 [B, L, hidden]; forward_packed(...) over a packed token array.  Holds 16-bit
    copies of the projection weights, one set per type used (rebuilt when the model's parameters change: fine-tuning between two
    ranking steps, load_state_dict, .to(device))."""

    def __init__(self, model):
        reason = unsupported_reason(model)
        if reason is not None:
            raise ValueError(f"FusedBertEncoder: {reason}")
        self.model = model
        arch = _describe(model)
        self.heads, self.hidden = arch.heads, arch.hidden
        # (a RoBERTa-family type table usually has ONE row: row 0 is added as the module adds it, and a caller that hands over
        # token_type_ids keeps the module, which alone can say that a nonzero id has no row)
        self.has_token_types = arch.type_table is not None and (arch.padding_idx is None or arch.type_table.shape[0] > 1)
        self._layers, self._signature, self._no_types = {}, None, None
        self._rel_bias = None      # relative_bias_table(model, REL_SPAN) of an encoder with a bias source: made and dropped with the weight copies
        self._adopted = self._adopted_stamp = None      # (dtype, layers): a weight set an optimizer keeps current (adopt_weights), and its stamp
        self.last_seed = None      # the seed of the latest training forward that ran with dropout (dropout_ref rebuilds its masks from it)

    def __getstate__(self):      # pickled with its model (torch.save(model)): without the 16-bit weight copies
        return {"model": self.model, "heads": self.heads, "hidden": self.hidden, "has_token_types": self.has_token_types}

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._layers, self._signature, self._no_types = {}, None, None
        self._rel_bias = None
        self._adopted = self._adopted_stamp = None
        self.last_seed = None

    def _params_signature(self):
        return tuple((p.data_ptr(), p._version, p.device) for p in _describe(self.model).stack.parameters())

    def refresh(self, dtype=None):
        """Drop the 16-bit weight copies if the module's parameters changed since they were made (-> True), and build the set of
        `dtype` (torch.bfloat16 / torch.float16) if one is named and missing."""
        sig = self._params_signature()
        if self._signature is _DEFERRED:      # a maintained step left its set as the only copies: current iff its stamp still holds
            changed = not self.adopted_current()
            self._signature = sig
            if changed:
                self._layers, self._rel_bias = {}, None
        else:
            changed = sig != self._signature
            if changed:
                self._layers, self._signature, self._rel_bias = {}, sig, None
        if dtype is not None and self._rel_bias is None and _describe(self.model).bias_source is not None:
            self._rel_bias = relative_bias_table(self.model, REL_SPAN)      # (its parameter is one of the stack's: the signature covers it)
        if dtype is not None and dtype not in self._layers:
            if self._adopted is not None and self._adopted[0] == dtype:
                self._rebuild_adopted()      # (in place: the optimizer that maintains the set holds its addresses)
            else:
                self._layers[dtype] = self._build_layers(dtype)
        return changed

    # ---- a weight set that an optimizer maintains (optim.FusedAdamW(shadow_for=...)): the set of `dtype` is built once from the masters;
    # every step of that optimizer writes the new 16-bit values into it and calls adopted_stepped.  Whether it may be read is decided by
    # its STAMP: (address, _version) of every tensor of every layer's parts, taken from the live module when the set was last made
    # current.  A parameter that changed any other way -- load_state_dict, an in-place operation, another optimizer, .to() -- has another
    # stamp: the set is stale, and a stale set is never read.  (Like _params_signature, the stamp sees what autograd's version counter sees.)
    def _live_masters(self):
        """Per layer the sixteen tensors the set derives from: q, k, v weight; q, k, v bias; attention output, FFN in, FFN out weight and
        bias; both LayerNorms' weight and bias."""
        arch = _describe(self.model)
        out = []
        for mod in arch.stack.layer:
            q, k, v, so, ln1, ff, fo, ln2 = arch.layer_parts(mod)
            out.append((q.weight, k.weight, v.weight, q.bias, k.bias, v.bias, so.weight, so.bias, ff.weight, ff.bias, fo.weight, fo.bias,
                        ln1.weight, ln1.bias, ln2.weight, ln2.bias))
        return out

    @staticmethod
    def _stamp(masters):
        return tuple((t.data_ptr(), t._version) for layer in masters for t in layer)

    def adopt_weights(self, dtype):
        """Build the weight set of `dtype` from the masters and keep it as the maintained one -> its layers (exactly _build_layers'
        tensors: the caller writes into wqkv / bqkv / wo / bo / wi / bi / wo2 / bo2)."""
        reason = shadow_unsupported_reason(self.model)
        assert reason is None, f"FusedBertEncoder.adopt_weights: {reason}"
        self.refresh()
        layers = self._build_layers(dtype)
        self._layers[dtype] = layers
        self._adopted, self._adopted_stamp = (dtype, layers), self._stamp(self._live_masters())
        return layers

    def adopted_masters(self):
        """The tensors the stamp is taken over, for a caller that checks it every step (it holds the same parameters)."""
        return self._live_masters()

    def adopted_current(self, dtype=None, masters=None):
        """Is there a maintained set (of `dtype`, if named) that matches the parameters as they are now?"""
        a = self._adopted
        return (a is not None and (dtype is None or a[0] == dtype) and self._layers.get(a[0]) is a[1]
                and self._adopted_stamp == self._stamp(self._live_masters() if masters is None else masters))

    def adopted_stepped(self, was_current, masters=None):
        """The maintaining optimizer has just updated the parameters and written their 16-bit values into the set.  was_current (taken
        before the update): the set is current at the new stamp and the copies of any other type are dropped; the signature that
        refresh() compares is taken at the next refresh() -- which trusts the stamp.  Otherwise something else had moved the
        parameters first, and the whole set is rebuilt from the masters."""
        if self._adopted is None:
            return
        dtype, layers = self._adopted
        if was_current:
            self._layers, self._signature = {dtype: layers}, _DEFERRED
            self._adopted_stamp = self._stamp(self._live_masters() if masters is None else masters)
        else:
            self._layers = {}
            self._rebuild_adopted()

    def _rebuild_adopted(self):
        """Fill the maintained set from the masters IN PLACE (the optimizer holds its addresses) and stamp it.  If the parameters have
        moved to another device or changed shape the set is given up: the next forwards cast, as without one."""
        dtype, layers = self._adopted
        sig = self._params_signature()
        if sig != self._signature:
            self._layers, self._signature = {}, sig
        fresh = self._build_layers(dtype)
        if len(fresh) != len(layers) or any(f.wqkv.device != l.wqkv.device or f.wqkv.shape != l.wqkv.shape for f, l in zip(fresh, layers)):
            self._adopted = self._adopted_stamp = None
            self._layers[dtype] = fresh
            return
        with torch.no_grad():
            for l, f in zip(layers, fresh):
                for name in _LAYER_16BIT:
                    getattr(l, name).copy_(getattr(f, name))
                for name in _LAYER_FP32:
                    setattr(l, name, getattr(f, name))
        self._layers[dtype] = layers
        self._adopted_stamp = self._stamp(self._live_masters())

    def _train_weights(self, half, masters):
        """The maintained set's layers when a training forward in `half` over the live `masters` may read them, else None = cast the
        live parameters for this call (no set, the other 16-bit type, or a stale set -- which is rebuilt from the masters here)."""
        a = self._adopted
        if a is None:
            return None
        if self._layers.get(a[0]) is a[1] and self._adopted_stamp == self._stamp(masters):
            return a[1] if a[0] == half else None
        self._rebuild_adopted()
        return None

    def _build_layers(self, half):
        assert half in (torch.bfloat16, torch.float16), half
        layers = []
        with torch.no_grad():
            arch = _describe(self.model)
            for mod in arch.stack.layer:
                q, k, v, so, ln1, ff, out, ln2 = arch.layer_parts(mod)
                l = _Layer()
                l.wqkv = torch.cat([q.weight, k.weight, v.weight]).to(half).contiguous()
                l.bqkv = torch.cat([q.bias, k.bias, v.bias]).to(half).contiguous()
                l.wo, l.bo = so.weight.to(half).contiguous(), so.bias.to(half).contiguous()
                l.g1, l.b1, l.eps1 = ln1.weight.float().contiguous(), ln1.bias.float().contiguous(), ln1.eps
                l.wi, l.bi = ff.weight.to(half).contiguous(), ff.bias.to(half).contiguous()
                l.wo2, l.bo2 = out.weight.to(half).contiguous(), out.bias.to(half).contiguous()
                l.g2, l.b2, l.eps2 = ln2.weight.float().contiguous(), ln2.bias.float().contiguous(), ln2.eps
                layers.append(l)
        return layers

    def _embedding_tables(self, token_types):
        """-> (word table, position table, type table, the block's LayerNorm, plain): the module's own tables, an all-zero type row
        standing in where the architecture has no token types; plain = all of them (and the LayerNorm's parameters) are contiguous fp32,
        what the embedding kernels read (a half-precision checkpoint is not)."""
        arch = _describe(self.model)
        e = arch.embeddings
        word, pos, ln, types = e.word_embeddings.weight, e.position_embeddings.weight, e.LayerNorm, arch.type_table
        if types is None:
            assert token_types is None, "this architecture has no token types"
            if self._no_types is None or self._no_types.device != word.device:
                self._no_types = torch.zeros(1, self.hidden, dtype=torch.float32, device=word.device)
            types = self._no_types
        plain = all(t.dtype == torch.float32 and t.is_contiguous() for t in (word, pos, types, ln.weight, ln.bias))
        return word, pos, types, ln, plain

    def _position_rows(self, token_ids, positions):
        """In-sequence positions (what every forward takes) -> rows of the architecture's position table."""
        padding_idx = _describe(self.model).padding_idx
        return positions if padding_idx is None else position_rows(token_ids, positions, padding_idx)

    def _embed(self, token_ids, positions, token_types, dtype):
        """The embedding block (BertEmbeddings.forward: (word + type) + position, LayerNorm; DistilBERT's Embeddings: word + position,
        LayerNorm) over flat int64 index vectors [T] -> (fp32 [T, hidden], its copy in `dtype`): one kernel on the module's own fp32
        tables (ccr_embed_layernorm; an all-zero type row stands in where the architecture has no token types), or the same sum
        in torch when the tables are not plain fp32 (a half-precision checkpoint)."""
        token_ids, positions = token_ids.long(), positions.long()          # (tokenizers may hand over int32 ids)
        token_types = None if token_types is None else token_types.long()
        positions = self._position_rows(token_ids, positions)
        word, pos, types, ln, plain = self._embedding_tables(token_types)
        if plain:
            return ops.embed_layernorm(word, pos, types, token_ids.contiguous(), positions.contiguous(),
                                       None if token_types is None else token_types.contiguous(), ln.weight, ln.bias, ln.eps, dtype=dtype)
        x = word[token_ids].float() + types[token_types if token_types is not None else torch.zeros_like(token_ids)].float()
        h = F.layer_norm(x + pos[positions].float(), (self.hidden,), ln.weight.float(), ln.bias.float(), ln.eps).contiguous()
        return h, h.to(dtype)

    def _layers_forward(self, h, hb, seq_start, lengths, max_len, pad_len, cls_rows=None):
        """The encoder layers over token rows h [T, hidden] fp32 / hb (its 16-bit copy, whose dtype selects the weight set); sequence s = rows seq_start[s] .. -> last
        hidden state [T, hidden] fp32.

        cls_rows ([n_seq] int64 rows of the sequences' first tokens): the caller reads only those rows of the last hidden state (the
        tower's cls | mu | mean | mean_layer_norm output steps, src/ccrec/models/item_tower.py:133-136 -- mean_layer_norm is the
        reference's CCREC_EMBEDDING_TYPE default).  The LAST layer then needs every token's keys and values but only the first
        tokens' attention output, so its output projection, both LayerNorms, the FFN and the GELU run on n_seq rows instead of T
        (same values: every one of those operations is row-wise) -> [n_seq, hidden]."""
        layers = self._layers[hb.dtype]
        last = len(layers) - 1
        bias = self._rel_bias
        assert (bias is not None) == (_describe(self.model).bias_source is not None), "refresh() keeps the bias table with the weight copies"
        width = self.hidden // self.heads      # 64, or 32 (unsupported_reason let it in: head32_wanted)
        scale = width ** -0.5
        for i, l in enumerate(layers):
            qkv = F.linear(hb, l.wqkv, l.bqkv)
            if bias is None:
                ctx = ops.attention(qkv, seq_start, lengths, self.heads, max_len=max_len, pad_len=pad_len, scale=scale, head_width=width)
            else:      # one table for every layer, as the module shares one position_bias
                ctx = ops.attention(qkv, seq_start, lengths, self.heads, max_len=max_len, pad_len=pad_len, scale=scale, rel_bias=bias,
                                    rel_span=REL_SPAN, head_width=width)
            if i == last and cls_rows is not None:
                ctx, h = ctx[cls_rows].contiguous(), h[cls_rows].contiguous()
            h, hb = ops.add_layernorm(F.linear(ctx, l.wo, l.bo), h, l.g1, l.b1, l.eps1)
            mid = ops.gelu_(F.linear(hb, l.wi, l.bi))      # exact GELU, in place (torch's bits)
            h, hb = ops.add_layernorm(F.linear(mid, l.wo2, l.bo2), h, l.g2, l.b2, l.eps2, want_bf16=i != last)
        if last < 0 and cls_rows is not None:
            h = h[cls_rows].contiguous()
        return h

    def _embed_train(self, token_ids, positions, token_types, dtype, drop=None):
        """_embed with gradients: F.embedding + F.layer_norm on the live tables (not a hot spot: one pass over T rows); drop (a
        _DropoutDraw): then the embeddings' dropout from its keep bits (ops.dropout_train).
        With CCREC_FUSED_ENCODER_TRAIN_PACKED=1 (train_packed_wanted) and plain contiguous fp32 tables: ops.embed_layernorm_train, the
        block and its dropout in one kernel with the backward on kernels (no atomics in the table gradients); the same keep bits."""
        arch = _describe(self.model)
        e = arch.embeddings
        token_ids, positions = token_ids.long(), positions.long()
        positions = self._position_rows(token_ids, positions)
        word_pad, pos_pad = _padding_rows(arch)
        if train_packed_wanted():
            word, pos, types, ln, plain = self._embedding_tables(token_types)
            if plain:
                word = word if word_pad is None else _NoGradRow.apply(word, word_pad)
                pos = pos if pos_pad is None else _NoGradRow.apply(pos, pos_pad)
                bits, inv_keep = (None, 1.0) if drop is None else drop.rows(getattr(e, "dropout", None), EMBEDDINGS_STREAM,
                                                                            token_ids.numel(), self.hidden, word.device)
                return ops.embed_layernorm_train(word, pos, types, token_ids, positions, None if token_types is None else token_types.long(),
                                                 ln.weight, ln.bias, ln.eps, keep_bits=bits, inv_keep=inv_keep, dtype=dtype)
        x = F.embedding(token_ids, e.word_embeddings.weight, padding_idx=word_pad).float()
        if arch.type_table is not None:
            types = torch.zeros_like(token_ids) if token_types is None else token_types.long()
            x = x + F.embedding(types, arch.type_table).float()
        else:
            assert token_types is None, "this architecture has no token types"
        x = x + F.embedding(positions, e.position_embeddings.weight, padding_idx=pos_pad).float()
        ln = e.LayerNorm
        h = F.layer_norm(x, (self.hidden,), ln.weight.float(), ln.bias.float(), ln.eps).contiguous()
        if drop is not None:
            bits, inv_keep = drop.rows(getattr(e, "dropout", None), EMBEDDINGS_STREAM, h.shape[0], self.hidden, h.device)
            if bits is not None:
                return ops.dropout_train(h, bits, inv_keep, dtype)
        return h, h.to(dtype)

    def _layers_forward_train(self, h, hb, seq_start, lengths, max_len, pad_len, cls_rows=None, drop=None):
        """_layers_forward with gradients.  The projections are F.linear on the LIVE parameters cast to hb's dtype: the gradients reach
        the fp32 master weights and no 16-bit copy can go stale between optimizer steps; autograd keeps the layer activations.  Where an
        optimizer maintains a weight set in hb's dtype and it is current (_train_weights), the projections read that set through
        _ShadowWeights instead of casting: the same operand bits, the same gradients.
        drop (a _DropoutDraw, a model in train() with live dropout): every site reads keep bits generated for its own stream id; the
        cls_only last layer generates its row-wise bits for the n_seq rows it runs on."""
        arch = _describe(self.model)
        half = hb.dtype
        mods = list(arch.stack.layer)
        last = len(mods) - 1
        masters = self._live_masters() if self._adopted is not None else None
        kept = None if masters is None else self._train_weights(half, masters)      # a current maintained weight set (optim.FusedAdamW): no cast, no cat
        for i, mod in enumerate(mods):
            q, k, v, so, ln1, ff, out, ln2 = arch.layer_parts(mod)
            if kept is not None:
                wqkv, bqkv, w_so, b_so, w_ff, b_ff, w_out, b_out = _ShadowWeights.apply(kept[i], *masters[i][:12])
            else:
                wqkv = torch.cat([q.weight, k.weight, v.weight]).to(half)
                bqkv = torch.cat([q.bias, k.bias, v.bias]).to(half)
                w_so, b_so, w_ff, b_ff = so.weight.to(half), so.bias.to(half), ff.weight.to(half), ff.bias.to(half)
                w_out, b_out = out.weight.to(half), out.bias.to(half)
            qkv = F.linear(hb, wqkv, bqkv)
            bits_a = bits_o = bits_f = None
            inv_a = inv_o = inv_f = 1.0
            if drop is not None:
                d_prob, d_attn, d_ffn = arch.dropout_parts(mod)
                bits_a, inv_a = drop.attention(d_prob, dropout_stream(i, SITE_PROBABILITIES), seq_start, lengths, hb.shape[0], self.heads, max_len)
            ctx = ops.attention_train(qkv, seq_start, lengths, self.heads, max_len=max_len, pad_len=pad_len, scale=0.125, keep_bits=bits_a,
                                      inv_keep=inv_a)
            if i == last and cls_rows is not None:
                ctx, h = ctx[cls_rows], h[cls_rows]
            if drop is not None:
                li = len(mods) if (i == last and cls_rows is not None) else i      # the rows it runs on are another index space: own streams
                bits_o, inv_o = drop.rows(d_attn, dropout_stream(li, SITE_ATTENTION_OUTPUT), ctx.shape[0], self.hidden, ctx.device)
                bits_f, inv_f = drop.rows(d_ffn, dropout_stream(li, SITE_FFN_OUTPUT), ctx.shape[0], self.hidden, ctx.device)
            h, hb = ops.add_layernorm_train(F.linear(ctx, w_so, b_so), h, ln1.weight.float(), ln1.bias.float(), ln1.eps,
                                            keep_bits=bits_o, inv_keep=inv_o)
            mid = ops.gelu_train(F.linear(hb, w_ff, b_ff))
            h, hb = ops.add_layernorm_train(F.linear(mid, w_out, b_out), h, ln2.weight.float(), ln2.bias.float(), ln2.eps,
                                            keep_bits=bits_f, inv_keep=inv_f)
        if last < 0 and cls_rows is not None:
            h = h[cls_rows]
        return h

    @staticmethod
    def _check_batch(input_ids, lengths):
        """What every forward over a right-padded batch asks of its arguments, before anything else runs."""
        assert input_ids.is_cuda and input_ids.dim() == 2
        B, L = input_ids.shape
        assert L <= 512 and lengths.dtype == torch.int32 and lengths.is_cuda and lengths.numel() == B

    def _layout(self, input_ids, lengths, token_type_ids, packed, lengths_host):
        """The token array of a right-padded batch input_ids [B, L] with lengths [B] int32 -> a _Batch: the flat token ids, positions and
        types, seq_start, max_len and pad_len as the layer kernels take them, and keep.
        packed: only the real tokens (keep = their int64 rows of the flattened batch; pad_len 0, max_len = the longest sequence); not
        packed: every row of the batch (keep None; pad_len = max_len = L).  packed None: packed when more than a tenth of the batch is
        padding.  A packed layout needs the lengths on the host: `lengths_host`, or one device read.  (The caller has run _check_batch.)"""
        B, L = input_ids.shape
        dev = input_ids.device
        if packed is None or packed:
            lens_h = lengths.cpu() if lengths_host is None else torch.as_tensor(lengths_host)
            total, longest = int(lens_h.sum()), int(lens_h.max()) if B else 0
            if packed is None:
                packed = total < 0.9 * B * L
        if packed:
            keep = (torch.arange(L, device=dev)[None, :] < lengths[:, None]).flatten().nonzero().squeeze(1)   # rows of the real tokens
            assert keep.numel() == total, "lengths_host does not match lengths"
            return _Batch(B, L, input_ids.flatten()[keep], keep % L, None if token_type_ids is None else token_type_ids.flatten()[keep],
                          (torch.cumsum(lengths, 0, dtype=torch.int32) - lengths).contiguous(), max(longest, 1), 0, keep)
        return _Batch(B, L, input_ids.flatten(), torch.arange(L, device=dev).repeat(B), None if token_type_ids is None else token_type_ids.flatten(),
                      torch.arange(B, dtype=torch.int32, device=dev) * L, L, L, None)

    def _padded(self, h, batch):
        """The layers' result h over batch's token rows -> [B, L, hidden]: a packed result goes back to its rows of a zero-filled batch
        (written in place into the fresh tensor; autograd follows index_copy_, padding rows carry no gradient)."""
        if batch.keep is not None:
            h = torch.zeros(batch.B * batch.L, self.hidden, dtype=torch.float32, device=h.device).index_copy_(0, batch.keep, h)
        return h.view(batch.B, batch.L, self.hidden)

    def _check_train(self):
        """Refuse what train_unsupported_reason refuses; -> the call's _DropoutDraw (one fresh seed, kept in last_seed) when the model is
        in training mode with live dropout, else None (the dropout-free kernels run)."""
        reason = train_unsupported_reason(self.model)
        assert reason is None, f"FusedBertEncoder training forward: {reason}"
        if not self.model.training or not any(_live(m) for m in self.model.modules()):
            return None
        self.last_seed = draw_seed()
        return _DropoutDraw(self.last_seed)

    def forward_train_packed(self, token_ids, positions, seq_start, lengths, max_len, token_type_ids=None, cls_only=False, dtype=torch.bfloat16):
        """forward_packed with gradients (same arguments, same result to the kernels' rounding): the parameters of the model receive
        gradients through the layer kernels' backward.  The model is in eval mode or has all-zero dropout, or CCREC_FUSED_ENCODER_TRAIN_DROPOUT=1
        opted into dropout from keep bits (train_unsupported_reason)."""
        ops.require_gpu()
        drop = self._check_train()
        assert token_ids.is_cuda and token_ids.dim() == 1 and positions.shape == token_ids.shape and 1 <= int(max_len) <= 512
        with torch.autocast("cuda", enabled=False):
            h, hb = self._embed_train(token_ids, positions, token_type_ids, dtype, drop)
            return self._layers_forward_train(h, hb, seq_start, lengths, int(max_len), 0, seq_start.long() if cls_only else None, drop)

    def forward_train(self, input_ids, lengths, token_type_ids=None, packed=None, lengths_host=None, cls_only=False, dtype=torch.bfloat16):
        """forward with gradients: the same arguments and the same [B, L, hidden] (or [B, 1, hidden]) fp32 result; padding rows are zeros
        (packed) or finite values nobody reads, and carry no gradient into the parameters."""
        ops.require_gpu()
        drop = self._check_train()
        self._check_batch(input_ids, lengths)
        with torch.autocast("cuda", enabled=False):
            b = self._layout(input_ids, lengths, token_type_ids, packed, lengths_host)
            h, hb = self._embed_train(b.ids, b.positions, b.types, dtype, drop)
            h = self._layers_forward_train(h, hb, b.seq_start, lengths, b.max_len, b.pad_len, b.seq_start.long() if cls_only else None, drop)
            return h.view(b.B, 1, self.hidden) if cls_only else self._padded(h, b)

    def forward_train_pooled(self, input_ids, lengths, token_type_ids=None, lengths_host=None, dtype=torch.bfloat16):
        """forward_train followed by the tower's masked mean pooling (src/ccrec/models/item_tower.py:141-146), without the padded tensor in
        between: the packed layers, then ops.meanpool_packed on the packed last hidden state -> [B, hidden] fp32 with gradients.  The
        pooled rows have the bits ops.meanpool gives on forward_train(packed=True)'s [B, L, hidden]; no [B, L, hidden] tensor is built
        and the backward writes no padding.  Same arguments as forward_train; the batch always runs packed."""
        ops.require_gpu()
        drop = self._check_train()
        self._check_batch(input_ids, lengths)
        with torch.autocast("cuda", enabled=False):
            b = self._layout(input_ids, lengths, token_type_ids, True, lengths_host)
            h, hb = self._embed_train(b.ids, b.positions, b.types, dtype, drop)
            h = self._layers_forward_train(h, hb, b.seq_start, lengths, b.max_len, 0, None, drop)
            return ops.meanpool_packed(h, b.seq_start, lengths.contiguous(), covers_all=True)

    @torch.no_grad()
    def forward_packed(self, token_ids, positions, seq_start, lengths, max_len, token_type_ids=None, cls_only=False, dtype=torch.bfloat16):
        """The forward over a packed token array that the caller built itself (no padded batch ever exists): token_ids / positions
        [T] int64 (position of each token inside its sequence), seq_start / lengths [n_seq] int32 (cuda), max_len = the longest
        sequence (host int).  -> fp32 [T, hidden]; pool it with ops.meanpool_pack_packed.  cls_only: -> [n_seq, hidden], the last
        hidden state of every sequence's first token only (_layers_forward).  dtype: the layer's 16-bit operand type (kernel_dtype())."""
        ops.require_gpu()
        assert not self.model.training, "FusedBertEncoder is an inference forward: call model.eval() first"
        assert token_ids.is_cuda and token_ids.dim() == 1 and positions.shape == token_ids.shape and 1 <= int(max_len) <= 512
        if dtype not in self._layers:      # (the per-batch caller, LengthSortedEncoder.encode, refreshes once per corpus)
            self.refresh(dtype)
        with torch.autocast("cuda", enabled=False):
            h, hb = self._embed(token_ids, positions, token_type_ids, dtype)
            return self._layers_forward(h, hb, seq_start, lengths, int(max_len), 0, seq_start.long() if cls_only else None)

    @torch.no_grad()
    def forward(self, input_ids, lengths, token_type_ids=None, packed=None, lengths_host=None, cls_only=False, dtype=torch.bfloat16):
        """input_ids [B, L] int64 (cuda, right-padded), lengths [B] int32 (cuda): real tokens per row, 1 .. L.
        -> fp32 [B, L, hidden]; rows of padding tokens hold finite values nobody reads (the pooling masks them).

        packed: run the layers on the REAL tokens only (a packed token array: the projections, LayerNorms and GELU skip the
        padding, the attention kernel takes row offsets + lengths) and scatter the result back into a zero-filled [B, L, hidden].
        That is what makes the reference-style batches cheap -- corpus-order batches padded to their longest text
        (scripts/al_0_rank.py:76-81) or to max_length (src/ccrec/models/item_tower.py:27-33) are 30-90 % padding.  None: packed
        when more than a tenth of the batch is padding (needs the lengths on the host: `lengths_host`, or one device read).
        cls_only: the caller reads only hidden[:, 0] -> fp32 [B, 1, hidden] (the last layer runs on the first tokens' rows only).
        dtype: the layer's 16-bit operand type (kernel_dtype(): the caller's autocast type)."""
        ops.require_gpu()
        model = self.model
        assert not model.training, "FusedBertEncoder is an inference forward: call model.eval() first"
        self._check_batch(input_ids, lengths)
        if dtype not in self._layers:
            self.refresh(dtype)
        with torch.autocast("cuda", enabled=False):
            b = self._layout(input_ids, lengths, token_type_ids, packed, lengths_host)
            h, hb = self._embed(b.ids, b.positions, b.types, dtype)
            h = self._layers_forward(h, hb, b.seq_start, lengths, b.max_len, b.pad_len, b.seq_start.long() if cls_only else None)
            return h.view(b.B, 1, self.hidden) if cls_only else self._padded(h, b)
