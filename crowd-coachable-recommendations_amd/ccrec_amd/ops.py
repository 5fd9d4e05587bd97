"""Tensor-level wrappers over the C ABI.  torch is plumbing here (device memory, streams); every
arithmetic step runs in libccr_hip.so.  All ops raise if there is no ROCm device."""
import contextlib
import ctypes
import os

import torch

from . import _lib

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.CcrError("ccrec_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return _lib.load()


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_NO_SWITCH = contextlib.nullcontext()


def _on(t):
    """Run the call with t's device current (HIP kernels launch on the current device).  The usual case -- it already
    is -- costs one integer compare instead of a device-guard round trip (the calls sit between a stream sync and the
    next kernel: host time here is GPU idle time)."""
    if t.device.index == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(t.device)


def _check_bounds(norm_bounds, rows):
    assert norm_bounds.is_cuda and norm_bounds.dtype == torch.float32 and norm_bounds.is_contiguous()
    assert norm_bounds.dim() == 1 and norm_bounds.numel() >= rows, "norm_bounds: one fp32 per (destination) row"


def padded_dim(dim):
    """Width of the packed rows: embeddings of any width are stored zero-padded to a multiple of 8 (16-byte chunks)."""
    return (int(dim) + 7) // 8 * 8


# ---- the 16-bit element type of a search index: bf16 (the default) or fp16 (opt-in)
INDEX_DTYPES = {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
_INDEX_DTYPE_NAMES = {"bf16": torch.bfloat16, "fp16": torch.float16}
_HALF_INDEX_CHECKED = False


def _require_half_index():
    """require_gpu() + once: the loaded library packs, indexes and searches either 16-bit type (ccr_version() >= 109)."""
    global _HALF_INDEX_CHECKED
    lib = require_gpu()
    if not _HALF_INDEX_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.HALF_INDEX_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, an fp16 index needs {_lib.HALF_INDEX_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _HALF_INDEX_CHECKED = True
    return lib


def index_dtype():
    """The element type the ranking paths pack and index with: os.environ["CCREC_INDEX_DTYPE"] = "bf16" (the default when unset) or
    "fp16", read at call time like CCREC_SIM_TYPE.  fp16 is what the reference's autocast hands its `Q @ chunk.T`
    (ms_marco_eval.py:215): unit roundoff 2^-11 instead of 2^-8, but a range that ends at 65 504 (see IndexOverflow)."""
    name = os.environ.get("CCREC_INDEX_DTYPE", "bf16")
    if name not in _INDEX_DTYPE_NAMES:
        raise ValueError(f"CCREC_INDEX_DTYPE={name!r}: expected 'bf16' or 'fp16'")
    return _INDEX_DTYPE_NAMES[name]


def _check_index_dtype(dtype):
    if dtype not in INDEX_DTYPES:
        raise TypeError(f"{dtype}: an index holds torch.bfloat16 or torch.float16 rows")
    return INDEX_DTYPES[dtype]


class IndexOverflow:
    """The overflow counter of ONE index build: every pack of the build adds the elements that were finite in fp32 and left fp16's
    range (-> +-inf) to one device int32; check() reads it once -- before the first search, not per batch -- and raises OverflowError.
    With bf16 there is nothing to count: `counter` is None and check() returns at once."""

    def __init__(self, dtype, device):
        self.dtype = dtype
        self.counter = torch.zeros(1, dtype=torch.int32, device=device) if dtype == torch.float16 else None

    def check(self):
        if self.counter is None:
            return
        n = int(self.counter.item())
        if n:
            raise OverflowError(f"{n} embedding element(s) left fp16's range (|x| >= 65520 became inf) while the index was packed: use "
                                f"CCREC_INDEX_DTYPE=bf16, or CCREC_SIM_TYPE=cos (normalised rows fit any type)")


def _check_overflow(overflow, dev):
    assert overflow.is_cuda and overflow.dtype == torch.int32 and overflow.numel() >= 1 and overflow.device == dev, \
        "overflow: an int32 cuda counter on the packed tensor's device"


def pack_half(x, dtype=torch.bfloat16, normalize=False, out=None, return_norms=False, norm_bounds=None, overflow=None):
    """pack_bf16 into either 16-bit element type of an index: fp32 [rows, dim] (cuda) -> dtype [rows, padded_dim(dim)], round to nearest
    even -- the bits of x.to(dtype), fp16 subnormals included; a finite value beyond +-65 504 becomes +-inf in fp16, as in torch.
    overflow: optional int32 cuda counter (zeroed by the caller, shared by any number of packs) that receives the number of such
    elements (fp16 only).  normalize / out / return_norms / norm_bounds: as pack_bf16."""
    lib = _require_half_index()
    code = _check_index_dtype(dtype)
    assert x.is_cuda and x.dim() == 2, "pack_half expects a 2-d cuda tensor"
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    rows, dim = x.shape
    pdim = padded_dim(dim)
    if out is None:
        out = torch.empty(rows, pdim, dtype=dtype, device=x.device)
    assert out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == (rows, pdim)
    norms = torch.empty(rows, dtype=torch.float32, device=x.device) if return_norms else None
    if norm_bounds is not None:
        _check_bounds(norm_bounds, rows)
    if overflow is not None:
        _check_overflow(overflow, x.device)
    with _on(x):
        if pdim != dim:
            _lib.check(lib.ccr_pack_half_padded(_ptr(x), rows, dim, _ptr(out), pdim, _ptr(norms), _ptr(norm_bounds),
                                                int(bool(normalize)), code, _ptr(overflow), _stream(x)), "ccr_pack_half_padded")
        else:
            _lib.check(lib.ccr_pack_half_ex(_ptr(x), _ptr(out), _ptr(norms), _ptr(norm_bounds), rows, dim, int(bool(normalize)), code,
                                            _ptr(overflow), _stream(x)), "ccr_pack_half")
    return (out, norms) if return_norms else out


def pack_bf16(x, normalize=False, out=None, return_norms=False, norm_bounds=None):
    """fp32 [rows, dim] (cuda) -> bf16 [rows, padded_dim(dim)]; normalize=True applies x / max(||x||, 1e-12) first
    (the cos_sim rule, ms_marco_eval.py:160-161).  `out` may be a slice of a preallocated shard.
    A width that is not a multiple of 8 (the reference takes any factor width, score_array.py:320-339) is zero-padded to the
    next one: scores, norms and cosines are unchanged, queries and corpus pad alike.
    norm_bounds: optional [rows] fp32 cuda tensor (the matching slice of a shard-sized one; no initialisation needed) that
    receives an upper bound of every packed row's norm; hand the whole array to CorpusIndex(norm_bounds=...) and the
    index build needs no pass over the shard (the search uses the bounds, per 256-row tile, in its filter margins)."""
    lib = require_gpu()
    assert x.is_cuda and x.dim() == 2, "pack_bf16 expects a 2-d cuda tensor"
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()  # autocast may hand over fp16 encoder outputs (al_0_rank.py:125)
    rows, dim = x.shape
    pdim = padded_dim(dim)
    if out is None:
        out = torch.empty(rows, pdim, dtype=torch.bfloat16, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.bfloat16 and tuple(out.shape) == (rows, pdim)
    norms = torch.empty(rows, dtype=torch.float32, device=x.device) if return_norms else None
    if norm_bounds is not None:
        _check_bounds(norm_bounds, rows)
    with _on(x):
        if pdim != dim:
            _lib.check(lib.ccr_pack_bf16_padded(_ptr(x), rows, dim, _ptr(out), pdim, _ptr(norms), _ptr(norm_bounds),
                                                int(bool(normalize)), _stream(x)), "ccr_pack_bf16_padded")
        else:
            _lib.check(lib.ccr_pack_bf16_ex(_ptr(x), _ptr(out), _ptr(norms), _ptr(norm_bounds), rows, dim, int(bool(normalize)),
                                            _stream(x)), "ccr_pack_bf16")
    return (out, norms) if return_norms else out


def meanpool_pack(hidden, mask, normalize=False, want_f32=True, want_bf16=True, out_bf16=None, out_f32=None, dst_rows=None,
                  norm_bounds=None, dtype=torch.bfloat16, overflow=None):
    """Fused masked mean pooling (item_tower.py:141-146) + bf16 pack of [B, L, dim] hidden states.
    Returns (pooled_f32 or None, packed_bf16 or None).

    out_bf16 / out_f32: write into these [rows, dim] tensors (e.g. the resident shard) instead of fresh [B, dim] ones;
    dst_rows: [B] int64 destination rows inside them (length-sorted batches scatter back to corpus order);
    norm_bounds: fp32 cuda tensor indexed like the destination rows: bound of each packed row's norm (see pack_bf16);
    dtype: element type of the packed rows (`out_bf16` keeps its name): torch.bfloat16, or torch.float16 with `overflow` as pack_half."""
    half = dtype != torch.bfloat16 or overflow is not None
    lib = _require_half_index() if half else require_gpu()
    code = _check_index_dtype(dtype)
    assert hidden.is_cuda and hidden.dim() == 3 and hidden.dtype in _DTYPES
    hidden = hidden.contiguous()
    mask = mask.to(device=hidden.device, dtype=torch.int64).contiguous()
    B, L, dim = hidden.shape
    assert tuple(mask.shape) == (B, L)
    f32 = out_f32 if out_f32 is not None else (torch.empty(B, dim, dtype=torch.float32, device=hidden.device) if want_f32 else None)
    b16 = out_bf16 if out_bf16 is not None else (torch.empty(B, dim, dtype=dtype, device=hidden.device) if want_bf16 else None)
    for t, dt in ((f32, torch.float32), (b16, dtype)):
        if t is not None:
            assert t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[1] == dim and t.is_contiguous()
            assert dst_rows is not None or t.shape[0] >= B
    if dst_rows is not None:
        dst_rows = dst_rows.to(device=hidden.device, dtype=torch.int64).contiguous()
        assert dst_rows.numel() == B
    if norm_bounds is not None:
        _check_bounds(norm_bounds, b16.shape[0] if (b16 is not None and dst_rows is not None) else B)
    if overflow is not None:
        _check_overflow(overflow, hidden.device)
    with _on(hidden):
        if half:
            _lib.check(lib.ccr_meanpool_pack_half_ex(_ptr(hidden), _DTYPES[hidden.dtype], _ptr(mask), _ptr(b16), _ptr(f32),
                                                     _ptr(dst_rows), _ptr(norm_bounds), B, L, dim, int(bool(normalize)), code,
                                                     _ptr(overflow), _stream(hidden)), "ccr_meanpool_pack_half")
        else:
            _lib.check(lib.ccr_meanpool_pack_bf16_ex(_ptr(hidden), _DTYPES[hidden.dtype], _ptr(mask), _ptr(b16), _ptr(f32),
                                                     _ptr(dst_rows), _ptr(norm_bounds), B, L, dim, int(bool(normalize)),
                                                     _stream(hidden)), "ccr_meanpool_pack_bf16")
    return f32, b16


def meanpool_pack_packed(hidden, seq_start, seq_len, normalize=False, out_bf16=None, out_f32=None, dst_rows=None, norm_bounds=None,
                         dtype=torch.bfloat16, overflow=None):
    """meanpool_pack for a packed token array: hidden [T, dim], sequence s = rows seq_start[s] .. + seq_len[s] - 1 (int32 cuda
    tensors).  Writes into out_bf16 / out_f32 ([rows, dim], at dst_rows or rows 0 .. n_seq - 1); returns (out_f32, out_bf16).
    dtype / overflow: as meanpool_pack."""
    half = dtype != torch.bfloat16 or overflow is not None
    lib = _require_half_index() if half else require_gpu()
    code = _check_index_dtype(dtype)
    assert hidden.is_cuda and hidden.dim() == 2 and hidden.dtype in _DTYPES and hidden.is_contiguous()
    n_seq, dim = seq_len.numel(), hidden.shape[1]
    for t in (seq_start, seq_len):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n_seq
    if out_bf16 is None and out_f32 is None:
        out_bf16 = torch.empty(n_seq, dim, dtype=dtype, device=hidden.device)
    for t, dt in ((out_f32, torch.float32), (out_bf16, dtype)):
        if t is not None:
            assert t.is_cuda and t.dtype == dt and t.dim() == 2 and t.shape[1] == dim and t.is_contiguous()
            assert dst_rows is not None or t.shape[0] >= n_seq
    if dst_rows is not None:
        dst_rows = dst_rows.to(device=hidden.device, dtype=torch.int64).contiguous()
        assert dst_rows.numel() == n_seq
    if norm_bounds is not None:
        _check_bounds(norm_bounds, out_bf16.shape[0] if (out_bf16 is not None and dst_rows is not None) else n_seq)
    if overflow is not None:
        _check_overflow(overflow, hidden.device)
    with _on(hidden):
        if half:
            _lib.check(lib.ccr_meanpool_pack_half_packed(_ptr(hidden), _DTYPES[hidden.dtype], _ptr(seq_start), _ptr(seq_len), _ptr(out_bf16),
                                                         _ptr(out_f32), _ptr(dst_rows), _ptr(norm_bounds), n_seq, dim, int(bool(normalize)),
                                                         code, _ptr(overflow), _stream(hidden)), "ccr_meanpool_pack_half_packed")
        else:
            _lib.check(lib.ccr_meanpool_pack_bf16_packed(_ptr(hidden), _DTYPES[hidden.dtype], _ptr(seq_start), _ptr(seq_len), _ptr(out_bf16),
                                                         _ptr(out_f32), _ptr(dst_rows), _ptr(norm_bounds), n_seq, dim, int(bool(normalize)),
                                                         _stream(hidden)), "ccr_meanpool_pack_bf16_packed")
    return out_f32, out_bf16


class _MeanPool(torch.autograd.Function):
    """Differentiable masked mean pooling (item_tower.py:141-146): forward = the fused pooling kernel (fp32 rows),
    backward = ccr_meanpool_bwd (grad / count broadcast over the unmasked tokens)."""

    @staticmethod
    def forward(ctx, hidden, mask):
        pooled, _ = meanpool_pack(hidden.detach(), mask, normalize=False, want_f32=True, want_bf16=False)
        ctx.save_for_backward(mask.to(device=hidden.device, dtype=torch.int64).contiguous())
        ctx.shape, ctx.dtype = tuple(hidden.shape), hidden.dtype
        return pooled

    @staticmethod
    def backward(ctx, grad):
        lib = require_gpu()
        (mask,) = ctx.saved_tensors
        B, L, dim = ctx.shape
        g = grad.detach().to(torch.float32).contiguous()
        dh = torch.empty(B, L, dim, dtype=ctx.dtype, device=g.device)
        with _on(g):
            _lib.check(lib.ccr_meanpool_bwd(_ptr(g), _ptr(mask), _ptr(dh), _DTYPES[ctx.dtype], B, L, dim, _stream(g)),
                       "ccr_meanpool_bwd")
        return dh, None


def meanpool(hidden, mask):
    """Masked mean pooling [B, L, dim] -> fp32 [B, dim] that autograd can differentiate (the training forward)."""
    return _MeanPool.apply(hidden, mask)


MAX_K = 4096   # the most results per query of a search (csrc/ccr_common.h)
MAX_QUERIES_PER_SEARCH = 16384   # larger batches are searched in pieces (last_stats() then describes the last piece)


_HALF_DTYPES = {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def _half_code(dtype):
    """CCR_DTYPE_* of one of the two 16-bit operand types of the encoder layer kernels."""
    assert dtype in _HALF_DTYPES, f"{dtype}: the encoder layer kernels take torch.bfloat16 or torch.float16 operands"
    return _HALF_DTYPES[dtype]


def _check_qkv(qkv, seq_start, seq_len, n_heads, head_width=64):
    """The token array and sequence table every attention op takes: qkv [T, 3 * n_heads * head_width] contiguous on the GPU, seq_start /
    seq_len [n_seq] contiguous int32 on the GPU.  -> T"""
    assert qkv.is_cuda and qkv.dim() == 2 and qkv.is_contiguous()
    T, width = qkv.shape
    assert width == 3 * n_heads * head_width, f"qkv rows are {width} wide, expected 3 x {n_heads} heads x {head_width}"
    assert seq_start.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_start.is_cuda and seq_len.is_cuda
    assert seq_start.is_contiguous() and seq_len.is_contiguous() and seq_start.numel() == seq_len.numel()
    return T


def _check_rows(x, residual, *vectors, keep_bits=None):
    """The operands of a row kernel: x [rows, dim] contiguous on the GPU, residual fp32 [rows, dim] or None, fp32 [dim] vectors (gamma,
    beta), keep bits int32 [rows, dim / 32] or None.  -> (rows, dim)"""
    assert x.is_cuda and x.dim() == 2 and x.is_contiguous()
    rows, dim = x.shape
    if keep_bits is not None:
        _check_bits(keep_bits, (rows, dim // 32))
    if residual is not None:
        assert residual.is_cuda and residual.dtype == torch.float32 and tuple(residual.shape) == (rows, dim) and residual.is_contiguous()
    for t in vectors:
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (dim,) and t.is_contiguous()
    return rows, dim


_ATTENTION_BIAS_CHECKED = False


def _require_attention_bias():
    """require_gpu() + once: the loaded library has the attention forward with a relative position bias (ccr_version() >= 112)."""
    global _ATTENTION_BIAS_CHECKED
    lib = require_gpu()
    if not _ATTENTION_BIAS_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.ATTENTION_BIAS_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, attention with a relative bias needs {_lib.ATTENTION_BIAS_VERSION}: "
                                f"rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        _ATTENTION_BIAS_CHECKED = True
    return lib


_HEAD32_CHECKED = False


def _require_head32():
    """require_gpu() + once: the loaded library has the attention forward for head width 32 (ccr_version() >= 114)."""
    global _HEAD32_CHECKED
    lib = require_gpu()
    if not _HEAD32_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.HEAD32_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, attention at head width 32 needs {_lib.HEAD32_VERSION}: "
                                f"rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        _HEAD32_CHECKED = True
    return lib


def attention(qkv, seq_start, seq_len, n_heads, max_len, pad_len=0, scale=0.125, out=None, rel_bias=None, rel_span=None, head_width=64):
    """Multi-head self-attention of a token array (ccr_attention_half; head width 64): qkv [T, 3 * n_heads * 64] bf16 or fp16 = the
    stacked query | key | value projection of every token, seq_start / seq_len [n_seq] int32 = each sequence's first row and real tokens,
    max_len = the longest seq_len (host int, <= 512), pad_len = L for a right-padded [n_seq, L] batch (its padding rows get
    zeros) or 0 for a packed array.  -> context rows [T, n_heads * 64] of qkv's dtype.
    rel_bias (ccr_attention_bias_half): fp32 [n_heads, 2 * R + 1] on qkv's device, one additive bias per (head, key - query) shared by
    every sequence: probability ~ exp(scale * q.k + rel_bias[head, R + key - query]).  rel_span = R (default: what the table's width
    says), max_len - 1 <= R <= 511.  An all-zero table gives the bits of the call without one.
    head_width = 32 (ccr_attention_head_half; the MiniLM-class encoders): qkv [T, 3 * n_heads * 32] -> [T, n_heads * 32], the caller's
    scale (32 ** -0.5 for BERT's layers), no rel_bias.  head_width = 64 is the call above, whichever entry point carries it."""
    if head_width not in (32, 64):
        raise ValueError(f"head_width={head_width}: the attention kernels are built for 32 and 64")
    if head_width == 32 and rel_bias is not None:
        raise ValueError("head_width=32 with rel_bias: the relative-bias attention kernel is built for head width 64 only")
    if head_width == 32:
        lib = _require_head32()
    else:
        lib = require_gpu() if rel_bias is None else _require_attention_bias()
    code = _half_code(qkv.dtype)
    T = _check_qkv(qkv, seq_start, seq_len, n_heads, head_width)
    if out is None:
        out = torch.empty(T, n_heads * head_width, dtype=qkv.dtype, device=qkv.device)
    assert out.is_cuda and out.dtype == qkv.dtype and tuple(out.shape) == (T, n_heads * head_width) and out.is_contiguous()
    if rel_bias is None:
        assert rel_span is None, "rel_span without rel_bias"
        with _on(qkv):
            if head_width == 32:
                _lib.check(lib.ccr_attention_head_half(_ptr(qkv), _ptr(seq_start), _ptr(seq_len), _ptr(out), seq_len.numel(), int(n_heads), 32,
                                                       int(max_len), int(pad_len), float(scale), code, _stream(qkv)), "ccr_attention_head_half")
            else:
                _lib.check(lib.ccr_attention_half(_ptr(qkv), _ptr(seq_start), _ptr(seq_len), _ptr(out), seq_len.numel(), int(n_heads),
                                                  int(max_len), int(pad_len), float(scale), code, _stream(qkv)), "ccr_attention_half")
        return out
    assert rel_bias.is_cuda and rel_bias.device == qkv.device and rel_bias.dtype == torch.float32 and rel_bias.is_contiguous()
    assert rel_bias.dim() == 2 and rel_bias.shape[0] == n_heads and rel_bias.shape[1] % 2 == 1, tuple(rel_bias.shape)
    R = rel_bias.shape[1] // 2 if rel_span is None else int(rel_span)
    assert rel_bias.shape[1] == 2 * R + 1, f"rel_bias has {rel_bias.shape[1]} columns, rel_span={R} needs {2 * R + 1}"
    with _on(qkv):
        _lib.check(lib.ccr_attention_bias_half(_ptr(qkv), _ptr(seq_start), _ptr(seq_len), _ptr(out), _ptr(rel_bias), R, seq_len.numel(),
                                               int(n_heads), int(max_len), int(pad_len), float(scale), code, _stream(qkv)),
                   "ccr_attention_bias_half")
    return out


def _check_embed_args(word_table, position_table, type_table, token_ids, positions, token_types, gamma):
    dim = word_table.shape[1]
    for t in (word_table, position_table, type_table):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == dim and t.is_contiguous()
    assert gamma.is_cuda and gamma.dtype == torch.float32 and tuple(gamma.shape) == (dim,) and gamma.is_contiguous()
    T = token_ids.numel()
    for t in (token_ids, positions) + ((token_types,) if token_types is not None else ()):
        assert t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.numel() == T and t.is_contiguous()
    return T, dim


def embed_layernorm(word_table, position_table, type_table, token_ids, positions, token_types, gamma, beta, eps, dtype=torch.bfloat16,
                    keep_bits=None, inv_keep=1.0):
    """LayerNorm((word_table[ids] + type_table[types]) + position_table[positions]) per token (ccr_embed_layernorm_half): fp32 tables
    [n, dim], int64 index vectors [T] (token_types may be None = type 0).  -> (fp32 [T, dim], its copy in `dtype` (bf16 / fp16) [T, dim]).
    keep_bits [T, dim / 32] (dropout_bits_rows): the block's dropout follows in the same kernel (ccr_embed_layernorm_train_half), with the
    bits of dropout_apply(embed_layernorm(...))."""
    lib = require_gpu() if keep_bits is None else _require_encoder_packed_train()
    code = _half_code(dtype)
    T, dim = _check_embed_args(word_table, position_table, type_table, token_ids, positions, token_types, gamma)
    assert beta.is_cuda and beta.dtype == torch.float32 and tuple(beta.shape) == (dim,) and beta.is_contiguous()
    if keep_bits is not None:
        _check_bits(keep_bits, (T, dim // 32))
    f32 = torch.empty(T, dim, dtype=torch.float32, device=word_table.device)
    b16 = torch.empty(T, dim, dtype=dtype, device=word_table.device)
    tables = (_ptr(word_table), word_table.shape[0], _ptr(position_table), position_table.shape[0], _ptr(type_table), type_table.shape[0],
              _ptr(token_ids), _ptr(positions), _ptr(token_types), _ptr(gamma), _ptr(beta), float(eps))
    with _on(word_table):
        if keep_bits is None:
            _lib.check(lib.ccr_embed_layernorm_half(*tables, _ptr(f32), _ptr(b16), T, dim, code, _stream(word_table)), "ccr_embed_layernorm_half")
        else:
            _lib.check(lib.ccr_embed_layernorm_train_half(*tables, _ptr(keep_bits), float(inv_keep), _ptr(f32), _ptr(b16), T, dim, code,
                                                          _stream(word_table)), "ccr_embed_layernorm_train_half")
    return f32, b16


def gelu_(x):
    """Exact (erf) GELU of a contiguous bf16 or fp16 cuda tensor, IN PLACE (ccr_gelu_half); returns x."""
    lib = require_gpu()
    code = _half_code(x.dtype)
    assert x.is_cuda and x.is_contiguous() and x.numel() % 8 == 0
    with _on(x):
        _lib.check(lib.ccr_gelu_half(_ptr(x), _ptr(x), x.numel(), code, _stream(x)), "ccr_gelu_half")
    return x


def add_layernorm(x, residual, gamma, beta, eps, want_f32=True, want_bf16=True, keep_bits=None, inv_keep=1.0):
    """LayerNorm(x + residual) * gamma + beta per row (ccr_add_layernorm_half): x [rows, dim] bf16 or fp16, residual [rows, dim] fp32 or
    None, gamma / beta [dim] fp32, dim a multiple of 128 (256 .. 2048; with keep_bits: of 256).  -> (fp32 rows or None, their copy in x's dtype or None:
    want_bf16 asks for that 16-bit copy whichever of the two types x has).
    keep_bits int32 [rows, dim / 32] (dropout_bits_rows): LayerNorm(x * keep * inv_keep + residual) (ccr_add_layernorm_drop_half)."""
    lib = require_gpu() if keep_bits is None else _require_encoder_dropout()
    code = _half_code(x.dtype)
    rows, dim = _check_rows(x, residual, gamma, beta, keep_bits=keep_bits)
    assert want_f32 or want_bf16
    f32 = torch.empty(rows, dim, dtype=torch.float32, device=x.device) if want_f32 else None
    b16 = torch.empty(rows, dim, dtype=x.dtype, device=x.device) if want_bf16 else None
    tail = (_ptr(residual), _ptr(gamma), _ptr(beta), float(eps), _ptr(f32), _ptr(b16), rows, dim, code, _stream(x))
    with _on(x):
        if keep_bits is None:
            _lib.check(lib.ccr_add_layernorm_half(_ptr(x), *tail), "ccr_add_layernorm_half")
        else:
            _lib.check(lib.ccr_add_layernorm_drop_half(_ptr(x), _ptr(keep_bits), float(inv_keep), *tail), "ccr_add_layernorm_drop_half")
    return f32, b16


# ---- the layer kernels with a backward (ccr_attention_fwd_train_half / ccr_*_bwd_half): fine-tuning through the encoder, the three
# encoder forwards + backward of a training step (src/ccrec/models/bbpr.py:195-197, bert_mt.py:105-113) ---------------------------------
_ENCODER_TRAIN_CHECKED = False


def _require_encoder_train():
    """require_gpu() + once: the loaded library has the encoder layer backward entry points (ccr_version() >= 103)."""
    global _ENCODER_TRAIN_CHECKED
    lib = require_gpu()
    if not _ENCODER_TRAIN_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.ENCODER_TRAIN_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the encoder training ops need {_lib.ENCODER_TRAIN_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _ENCODER_TRAIN_CHECKED = True
    return lib


def attention_fwd_train(qkv, seq_start, seq_len, n_heads, max_len, pad_len=0, scale=0.125, keep_q=None, inv_keep=1.0):
    """attention() that also returns lse [T, n_heads] fp32, the log-sum-exp of every real query row's scaled scores (0 on padding
    rows): what attention_bwd rebuilds the probabilities from (ccr_attention_fwd_train_half).  -> (out, lse); out has attention()'s bits.
    keep_q (dropout_bits_attention): dropout on the probabilities (ccr_attention_fwd_train_drop_half): the value rounded for the P V
    product is p * keep * inv_keep; lse stays that of the undropped scores."""
    lib = _require_encoder_train() if keep_q is None else _require_encoder_dropout()
    code = _half_code(qkv.dtype)
    T = _check_qkv(qkv, seq_start, seq_len, n_heads)
    if keep_q is not None:
        _check_bits(keep_q, (T, n_heads, (int(max_len) + 31) // 32))
    out = torch.empty(T, n_heads * 64, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(T, n_heads, dtype=torch.float32, device=qkv.device)
    shape = (seq_len.numel(), int(n_heads), int(max_len), int(pad_len), float(scale), code, _stream(qkv))
    with _on(qkv):
        if keep_q is None:
            _lib.check(lib.ccr_attention_fwd_train_half(_ptr(qkv), _ptr(seq_start), _ptr(seq_len), _ptr(out), _ptr(lse), *shape),
                       "ccr_attention_fwd_train_half")
        else:
            _lib.check(lib.ccr_attention_fwd_train_drop_half(_ptr(qkv), _ptr(seq_start), _ptr(seq_len), _ptr(out), _ptr(lse), _ptr(keep_q),
                                                             float(inv_keep), *shape), "ccr_attention_fwd_train_drop_half")
    return out, lse


def attention_bwd(qkv, out, lse, d_out, seq_start, seq_len, n_heads, max_len, pad_len=0, scale=0.125, keep_q=None, keep_k=None, inv_keep=1.0):
    """d_qkv [T, 3 * n_heads * 64] (qkv's dtype and layout) from attention_fwd_train's (out, lse) and d_out [T, n_heads * 64]
    (ccr_attention_bwd_half).  Rows of the sequences' padding get zeros; so do rows that belong to no sequence.
    keep_q, keep_k: the forward's bits, both or neither (ccr_attention_bwd_drop_half)."""
    assert (keep_q is None) == (keep_k is None), "attention_bwd: keep_q and keep_k come together"
    lib = _require_encoder_train() if keep_q is None else _require_encoder_dropout()
    code = _half_code(qkv.dtype)
    T = _check_qkv(qkv, seq_start, seq_len, n_heads)
    for t in (out, d_out):
        assert t.is_cuda and t.dtype == qkv.dtype and tuple(t.shape) == (T, n_heads * 64) and t.is_contiguous()
    assert lse.is_cuda and lse.dtype == torch.float32 and tuple(lse.shape) == (T, n_heads) and lse.is_contiguous()
    if keep_q is not None:
        for bits in (keep_q, keep_k):
            _check_bits(bits, (T, n_heads, (int(max_len) + 31) // 32))
    n_seq = seq_len.numel()
    need = int(lib.ccr_attention_bwd_workspace_bytes(n_seq, int(n_heads), int(max_len)))
    if need == 0:
        _lib.check(_lib.CCR_ERR_INVALID, "ccr_attention_bwd_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    d_qkv = torch.zeros_like(qkv)
    head = (_ptr(qkv), _ptr(out), _ptr(lse), _ptr(d_out), _ptr(seq_start), _ptr(seq_len))
    tail = (_ptr(d_qkv), n_seq, int(n_heads), int(max_len), int(pad_len), float(scale), code, _ptr(ws), need, _stream(qkv))
    with _on(qkv):
        if keep_q is None:
            _lib.check(lib.ccr_attention_bwd_half(*head, *tail), "ccr_attention_bwd_half")
        else:
            _lib.check(lib.ccr_attention_bwd_drop_half(*head, _ptr(keep_q), _ptr(keep_k), float(inv_keep), *tail), "ccr_attention_bwd_drop_half")
    return d_qkv


def _layernorm_bwd_workspace(rows, dim, want_params, device):
    """(workspace, its bytes) of a LayerNorm backward that returns d_gamma or d_beta: the per-workgroup column sums of at most 512
    workgroups of four rows (include/ccr_retrieval.h); (None, 0) when neither is wanted."""
    need = min((rows + 3) // 4, 512) * 2 * dim * 4 if want_params else 0
    return (torch.empty(need, dtype=torch.uint8, device=device) if need else None), need


def add_layernorm_bwd(x, residual, gamma, eps, d_y, want_res=True, want_x=True, want_gamma=True, want_beta=True, keep_bits=None, inv_keep=1.0):
    """The backward of add_layernorm (ccr_add_layernorm_bwd_half): d_y [rows, dim] fp32 = the summed gradient of the LayerNorm output
    -> (d_res fp32 = the gradient of x + residual, d_x = the same rounded to x's dtype, d_gamma, d_beta [dim] fp32); None where not wanted.
    keep_bits: the forward's (ccr_add_layernorm_bwd_drop_half): d_res is the gradient of the summed input, d_x = d_res * keep * inv_keep."""
    lib = _require_encoder_train() if keep_bits is None else _require_encoder_dropout()
    code = _half_code(x.dtype)
    rows, dim = _check_rows(x, residual, gamma, keep_bits=keep_bits)
    assert d_y.is_cuda and d_y.dtype == torch.float32 and tuple(d_y.shape) == (rows, dim) and d_y.is_contiguous()
    dev = x.device
    d_res = torch.empty(rows, dim, dtype=torch.float32, device=dev) if want_res else None
    d_x = torch.empty(rows, dim, dtype=x.dtype, device=dev) if want_x else None
    d_gamma = torch.empty(dim, dtype=torch.float32, device=dev) if want_gamma else None
    d_beta = torch.empty(dim, dtype=torch.float32, device=dev) if want_beta else None
    ws, need = _layernorm_bwd_workspace(rows, dim, want_gamma or want_beta, dev)
    tail = (_ptr(residual), _ptr(gamma), float(eps), _ptr(d_y), _ptr(d_res), _ptr(d_x), _ptr(d_gamma), _ptr(d_beta), rows, dim, code, _ptr(ws),
            need, _stream(x))
    with _on(x):
        if keep_bits is None:
            _lib.check(lib.ccr_add_layernorm_bwd_half(_ptr(x), *tail), "ccr_add_layernorm_bwd_half")
        else:
            _lib.check(lib.ccr_add_layernorm_bwd_drop_half(_ptr(x), _ptr(keep_bits), float(inv_keep), *tail), "ccr_add_layernorm_bwd_drop_half")
    return d_res, d_x, d_gamma, d_beta


def gelu_bwd(x, d_y):
    """d_x = d_y (Phi(x) + x phi(x)) of the exact GELU from its pre-activation x (ccr_gelu_bwd_half); x's dtype."""
    lib = _require_encoder_train()
    code = _half_code(x.dtype)
    assert x.is_cuda and x.is_contiguous() and x.numel() % 8 == 0
    assert d_y.is_cuda and d_y.dtype == x.dtype and d_y.shape == x.shape and d_y.is_contiguous()
    d_x = torch.empty_like(x)
    with _on(x):
        _lib.check(lib.ccr_gelu_bwd_half(_ptr(x), _ptr(d_y), _ptr(d_x), x.numel(), code, _stream(x)), "ccr_gelu_bwd_half")
    return d_x


def _sum_output_grads(d_f32, d_b16):
    """A row op returns one value in two precisions: the gradients of the two outputs add up (fp32) before the backward kernel runs."""
    if d_f32 is None:
        return d_b16.float()
    if d_b16 is None:
        return d_f32.float()
    return d_f32.float() + d_b16


class _AttentionTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q, keep_k, inv_keep):
        out, lse = attention_fwd_train(qkv, seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q, inv_keep)
        ctx.save_for_backward(qkv, out, lse, seq_start, seq_len, keep_q, keep_k)
        ctx.shape = (int(n_heads), int(max_len), int(pad_len), float(scale), float(inv_keep))
        return out

    @staticmethod
    def backward(ctx, d_out):
        qkv, out, lse, seq_start, seq_len, keep_q, keep_k = ctx.saved_tensors
        n_heads, max_len, pad_len, scale, inv_keep = ctx.shape
        d_qkv = attention_bwd(qkv, out, lse, d_out.to(qkv.dtype).contiguous(), seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q,
                              keep_k, inv_keep)
        return (d_qkv,) + (None,) * 9


def attention_train(qkv, seq_start, seq_len, n_heads, max_len, pad_len=0, scale=0.125, keep_bits=None, inv_keep=1.0):
    """attention() with a backward: the same context rows, bit for bit; the gradient reaches qkv (the stacked projection's output).
    keep_bits = (keep_q, keep_k) of dropout_bits_attention: dropout on the probabilities, scaled by inv_keep, the bits saved for the backward."""
    keep_q, keep_k = (None, None) if keep_bits is None else keep_bits
    return _AttentionTrain.apply(qkv.contiguous(), seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q, keep_k, inv_keep)


class _AddLayerNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps, bits, inv_keep):
        f32, b16 = add_layernorm(x, residual, gamma, beta, eps, keep_bits=bits, inv_keep=inv_keep)
        ctx.save_for_backward(x, residual, gamma, bits)
        ctx.eps, ctx.inv_keep = float(eps), float(inv_keep)
        return f32, b16

    @staticmethod
    def backward(ctx, d_f32, d_b16):
        x, residual, gamma, bits = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_res, d_x, d_gamma, d_beta = add_layernorm_bwd(x, residual, gamma, ctx.eps, _sum_output_grads(d_f32, d_b16).contiguous(),
                                                        want_res=residual is not None and need[1], want_x=need[0], want_gamma=need[2],
                                                        want_beta=need[3], keep_bits=bits, inv_keep=ctx.inv_keep)
        return d_x, d_res, d_gamma, d_beta, None, None, None


def add_layernorm_train(x, residual, gamma, beta, eps, keep_bits=None, inv_keep=1.0):
    """add_layernorm() with a backward -> (fp32 rows, their copy in x's dtype).  Both outputs are differentiable; the gradient reaches x
    (in its dtype), residual, gamma and beta.  keep_bits (dropout_bits_rows): LayerNorm(x * keep * inv_keep + residual)."""
    return _AddLayerNormTrain.apply(x.contiguous(), None if residual is None else residual.contiguous(), gamma.contiguous(), beta.contiguous(),
                                    eps, keep_bits, inv_keep)


class _GeluTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        lib = require_gpu()
        y = torch.empty_like(x)
        with _on(x):
            _lib.check(lib.ccr_gelu_half(_ptr(x), _ptr(y), x.numel(), _half_code(x.dtype), _stream(x)), "ccr_gelu_half")
        return y

    @staticmethod
    def backward(ctx, d_y):
        (x,) = ctx.saved_tensors
        return gelu_bwd(x, d_y.to(x.dtype).contiguous())


def gelu_train(x):
    """Exact GELU, out of place, with a backward (gelu_() overwrites the pre-activation the backward needs)."""
    assert x.is_cuda and x.numel() % 8 == 0
    return _GeluTrain.apply(x.contiguous())


# ---- training dropout from explicit keep bits (library version 104, csrc/ccr_dropout.hip): the reference's towers train in train() mode
# with dropout 0.1 (src/ccrec/models/bbpr.py:195-197, bert_mt.py:105-113).  A generator kernel writes packed keep bits; the layer kernels
# read them with one scale factor.  ccrec_amd/dropout_ref.py restates the generator on the CPU ---------------------------------------------
_ENCODER_DROPOUT_CHECKED = False


def _require_encoder_dropout():
    """require_gpu() + once: the loaded library has the keep-bit entry points (ccr_version() >= 104)."""
    global _ENCODER_DROPOUT_CHECKED
    lib = require_gpu()
    if not _ENCODER_DROPOUT_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.ENCODER_DROPOUT_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the encoder dropout ops need {_lib.ENCODER_DROPOUT_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _ENCODER_DROPOUT_CHECKED = True
    return lib


_OPTIM_CHECKED = False


def _require_optim():
    """require_gpu() + once: the loaded library has the multi-tensor AdamW step (ccr_version() >= 107; ccrec_amd/optim.py calls it)."""
    global _OPTIM_CHECKED
    lib = require_gpu()
    if not _OPTIM_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.OPTIM_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the fused optimizer step needs {_lib.OPTIM_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _OPTIM_CHECKED = True
    return lib


_OPTIM_AMP_CHECKED = False


def _require_optim_amp():
    """require_gpu() + once: the loaded library has the scaled AdamW step with its statistics and control kernels (ccr_version() >= 110;
    FusedAdamW(max_grad_norm=...), the GradScaler protocol and optim.LossScaler call them)."""
    global _OPTIM_AMP_CHECKED
    lib = require_gpu()
    if not _OPTIM_AMP_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.AMP_OPTIM_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, loss scaling and clipping in the optimizer step need "
                                f"{_lib.AMP_OPTIM_VERSION}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        _OPTIM_AMP_CHECKED = True
    return lib


def dropout_bits_rows(rows, dim, seed, stream_id, p, device="cuda"):
    """Packed keep bits uint32 (stored as int32) [rows, dim / 32] of a row-wise dropout site (ccr_dropout_bits_rows): bit i of word w <->
    column 32 w + i, 1 = keep; a pure function of (seed, stream_id, p, row, column) -- dropout_ref.rows_bits gives the same words."""
    lib = _require_encoder_dropout()
    bits = torch.empty(int(rows), int(dim) // 32, dtype=torch.int32, device=device)
    with _on(bits):
        _lib.check(lib.ccr_dropout_bits_rows(_ptr(bits), int(rows), int(dim), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                                             float(p), _stream(bits)), "ccr_dropout_bits_rows")
    return bits


def dropout_bits_attention(seq_start, seq_len, n_tokens, n_heads, max_len, seed, stream_id, p):
    """(keep_q, keep_k) int32 [n_tokens, n_heads, ceil(max_len / 32)] of an attention dropout site (ccr_dropout_bits_attention): the same
    decisions by query row (bit = key position) and by key row (bit = query position).  Zero-filled first: words of rows outside every
    sequence and bits beyond a length carry no meaning, and no kernel reads them into a result."""
    lib = _require_encoder_dropout()
    assert seq_start.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_start.is_cuda and seq_len.is_cuda
    assert seq_start.is_contiguous() and seq_len.is_contiguous() and seq_start.numel() == seq_len.numel()
    W = (int(max_len) + 31) // 32
    both = torch.zeros(2, int(n_tokens), int(n_heads), W, dtype=torch.int32, device=seq_start.device)
    with _on(both):
        _lib.check(lib.ccr_dropout_bits_attention(_ptr(both[0]), _ptr(both[1]), _ptr(seq_start), _ptr(seq_len), int(n_tokens), seq_len.numel(),
                                                  int(n_heads), int(max_len), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                                                  float(p), _stream(both)), "ccr_dropout_bits_attention")
    return both[0], both[1]


def _check_bits(bits, shape):
    assert bits.is_cuda and bits.dtype == torch.int32 and tuple(bits.shape) == tuple(shape) and bits.is_contiguous(), \
        f"keep bits: contiguous int32 {tuple(shape)}, got {bits.dtype} {tuple(bits.shape)}"


def dropout_apply(x, bits, inv_keep, dtype=torch.bfloat16, want_f32=True, want_half=True):
    """x * keep * inv_keep of fp32 rows [rows, dim] (ccr_dropout_apply; dim % 256 == 0) -> (fp32 or None, its copy in `dtype` or None)."""
    lib = _require_encoder_dropout()
    code = _half_code(dtype)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and (want_f32 or want_half)
    rows, dim = x.shape
    _check_bits(bits, (rows, dim // 32))
    f32 = torch.empty_like(x) if want_f32 else None
    b16 = torch.empty(rows, dim, dtype=dtype, device=x.device) if want_half else None
    with _on(x):
        _lib.check(lib.ccr_dropout_apply(_ptr(x), _ptr(bits), float(inv_keep), _ptr(f32), _ptr(b16), rows, dim, code, _stream(x)),
                   "ccr_dropout_apply")
    return f32, b16


class _DropoutTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bits, inv_keep, dtype):
        f32, b16 = dropout_apply(x, bits, inv_keep, dtype)
        ctx.save_for_backward(bits)
        ctx.inv_keep, ctx.dtype = float(inv_keep), dtype
        return f32, b16

    @staticmethod
    def backward(ctx, d_f32, d_b16):
        (bits,) = ctx.saved_tensors
        d_x, _ = dropout_apply(_sum_output_grads(d_f32, d_b16).contiguous(), bits, ctx.inv_keep, ctx.dtype, want_half=False)
        return d_x, None, None, None


def dropout_train(x, bits, inv_keep, dtype=torch.bfloat16):
    """Dropout of fp32 rows [rows, dim] from explicit keep bits, with a backward (the same operation on the gradient) -> (fp32 rows, their
    copy in `dtype`); both outputs are differentiable.  The site after the embedding LayerNorm."""
    return _DropoutTrain.apply(x.contiguous(), bits, inv_keep, dtype)


# ---- the earlier spelling of the ops with keep bits, for callers written against it: each forwards to the one function of its op (the
# positional order of these differs from the keyword form's, so they stay functions of their own) --------------------------------------
def attention_fwd_train_drop(qkv, seq_start, seq_len, n_heads, max_len, keep_q, inv_keep, pad_len=0, scale=0.125):
    return attention_fwd_train(qkv, seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q=keep_q, inv_keep=inv_keep)


def attention_bwd_drop(qkv, out, lse, d_out, seq_start, seq_len, n_heads, max_len, keep_q, keep_k, inv_keep, pad_len=0, scale=0.125):
    return attention_bwd(qkv, out, lse, d_out, seq_start, seq_len, n_heads, max_len, pad_len, scale, keep_q=keep_q, keep_k=keep_k, inv_keep=inv_keep)


def add_layernorm_drop(x, bits, inv_keep, residual, gamma, beta, eps, want_f32=True, want_bf16=True):
    return add_layernorm(x, residual, gamma, beta, eps, want_f32, want_bf16, keep_bits=bits, inv_keep=inv_keep)


def add_layernorm_bwd_drop(x, bits, inv_keep, residual, gamma, eps, d_y, want_res=True, want_x=True, want_gamma=True, want_beta=True):
    return add_layernorm_bwd(x, residual, gamma, eps, d_y, want_res, want_x, want_gamma, want_beta, keep_bits=bits, inv_keep=inv_keep)


def embed_layernorm_drop(word_table, position_table, type_table, token_ids, positions, token_types, gamma, beta, eps, keep_bits=None,
                         inv_keep=1.0, dtype=torch.bfloat16):
    _require_encoder_packed_train()      # (as it always asked, with or without bits)
    return embed_layernorm(word_table, position_table, type_table, token_ids, positions, token_types, gamma, beta, eps, dtype, keep_bits, inv_keep)


# ---- the fine-tune step in one packed pass (library version 108): the embedding block with a backward (csrc/ccr_encoder.hip,
# ccr_encoder_bwd.hip, ccr_embed_train.hip) and mean pooling of a packed token array with a backward (csrc/ccr_pack.hip).  The reference
# encodes three times per step (src/ccrec/models/bbpr.py:195-197) and pools under the mask (item_tower.py:141-146) ------------------------
_ENCODER_PACKED_TRAIN_CHECKED = False


def _require_encoder_packed_train():
    """require_gpu() + once: the loaded library has the embedding block's and the packed pooling's backward (ccr_version() >= 108)."""
    global _ENCODER_PACKED_TRAIN_CHECKED
    lib = require_gpu()
    if not _ENCODER_PACKED_TRAIN_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.ENCODER_PACKED_TRAIN_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the packed training ops need {_lib.ENCODER_PACKED_TRAIN_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _ENCODER_PACKED_TRAIN_CHECKED = True
    return lib


def embed_layernorm_bwd(word_table, position_table, type_table, token_ids, positions, token_types, gamma, eps, d_y, keep_bits=None,
                        inv_keep=1.0, want_x=True, want_gamma=True, want_beta=True):
    """The backward of embed_layernorm, with or without keep bits (ccr_embed_layernorm_bwd_half): d_y [T, dim] fp32 = the summed gradient of both outputs ->
    (d_x fp32 [T, dim] = the gradient of every gathered table row, d_gamma, d_beta [dim] fp32); None where not wanted."""
    lib = _require_encoder_packed_train()
    T, dim = _check_embed_args(word_table, position_table, type_table, token_ids, positions, token_types, gamma)
    assert d_y.is_cuda and d_y.dtype == torch.float32 and tuple(d_y.shape) == (T, dim) and d_y.is_contiguous()
    if keep_bits is not None:
        _check_bits(keep_bits, (T, dim // 32))
    dev = word_table.device
    d_x = torch.empty(T, dim, dtype=torch.float32, device=dev) if want_x else None
    d_gamma = torch.empty(dim, dtype=torch.float32, device=dev) if want_gamma else None
    d_beta = torch.empty(dim, dtype=torch.float32, device=dev) if want_beta else None
    ws, need = _layernorm_bwd_workspace(T, dim, want_gamma or want_beta, dev)
    with _on(word_table):
        _lib.check(lib.ccr_embed_layernorm_bwd_half(_ptr(word_table), word_table.shape[0], _ptr(position_table), position_table.shape[0],
                                                    _ptr(type_table), type_table.shape[0], _ptr(token_ids), _ptr(positions), _ptr(token_types),
                                                    _ptr(gamma), float(eps), _ptr(keep_bits), float(inv_keep), _ptr(d_y), _ptr(d_x),
                                                    _ptr(d_gamma), _ptr(d_beta), T, dim, _ptr(ws), need, _stream(word_table)),
                   "ccr_embed_layernorm_bwd_half")
    return d_x, d_gamma, d_beta


def embedding_order(idx, n_rows):
    """The permutation ccr_embedding_grad walks: token rows sorted by (clamped id, row) ascending.  One torch.sort of the unique keys
    clamp(idx) * T + row on the device: no host wait, and the result does not depend on the sort being stable."""
    T = idx.numel()
    keys = idx.clamp(0, int(n_rows) - 1) * T + torch.arange(T, dtype=torch.int64, device=idx.device)
    return torch.sort(keys)[1]


def embedding_grad(idx, d_x, n_rows, order=None, out=None):
    """The gradient [n_rows, dim] fp32 of an embedding table from d_x [T, dim] fp32, the gradient of its gathered rows table[idx]
    (ccr_embedding_grad): no atomics, every row written (+0 where an id does not occur), the summation order of embed_grad_ref."""
    lib = _require_encoder_packed_train()
    assert idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous()
    T = idx.numel()
    assert d_x.is_cuda and d_x.dtype == torch.float32 and d_x.dim() == 2 and d_x.shape[0] == T and d_x.is_contiguous()
    dim = d_x.shape[1]
    if order is None:
        order = embedding_order(idx, n_rows)
    assert order.is_cuda and order.dtype == torch.int64 and tuple(order.shape) == (T,) and order.is_contiguous()
    if out is None:
        out = torch.empty(int(n_rows), dim, dtype=torch.float32, device=d_x.device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (int(n_rows), dim) and out.is_contiguous()
    with _on(d_x):
        _lib.check(lib.ccr_embedding_grad(_ptr(idx), _ptr(order), _ptr(d_x), T, dim, _ptr(out), int(n_rows), _stream(d_x)), "ccr_embedding_grad")
    return out


class _EmbedLayerNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, word, pos, types, token_ids, positions, token_types, gamma, beta, eps, bits, inv_keep, dtype):
        _require_encoder_packed_train()      # (its backward needs it: fail before the forward runs, not in the middle of a step)
        f32, b16 = embed_layernorm(word, pos, types, token_ids, positions, token_types, gamma, beta, eps, dtype, bits, inv_keep)
        ctx.save_for_backward(word, pos, types, token_ids, positions, token_types, gamma, bits)
        ctx.eps, ctx.inv_keep = float(eps), float(inv_keep)
        return f32, b16

    @staticmethod
    def backward(ctx, d_f32, d_b16):
        word, pos, types, token_ids, positions, token_types, gamma, bits = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_x, d_gamma, d_beta = embed_layernorm_bwd(word, pos, types, token_ids, positions, token_types, gamma, ctx.eps,
                                                   _sum_output_grads(d_f32, d_b16).contiguous(), bits, ctx.inv_keep, want_x=any(need[:3]), want_gamma=need[6], want_beta=need[7])
        d_word = embedding_grad(token_ids, d_x, word.shape[0]) if need[0] else None
        d_pos = embedding_grad(positions, d_x, pos.shape[0]) if need[1] else None
        d_types = None
        if need[2] and token_types is not None:
            d_types = embedding_grad(token_types, d_x, types.shape[0])
        elif need[2]:      # every token is type 0: one run in row order, nothing to sort
            rows = torch.arange(token_ids.numel(), dtype=torch.int64, device=token_ids.device)
            d_types = embedding_grad(torch.zeros_like(token_ids), d_x, types.shape[0], order=rows)
        return d_word, d_pos, d_types, None, None, None, d_gamma, d_beta, None, None, None, None


def embed_layernorm_train(word_table, position_table, type_table, token_ids, positions, token_types, gamma, beta, eps, keep_bits=None,
                          inv_keep=1.0, dtype=torch.bfloat16):
    """The embedding block with a backward: dropout(LayerNorm((word[ids] + type[types]) + position[positions])) -> (fp32 [T, dim], its copy
    in `dtype`), both differentiable.  Forward = embed_layernorm (the inference kernel's bits without keep_bits); backward =
    embed_layernorm_bwd, then one embedding_grad per table that needs a gradient (needs_input_grad is honoured: a frozen table costs
    nothing).  Tables, gamma, beta: contiguous fp32; index vectors int64 [T], token_types may be None = type 0."""
    return _EmbedLayerNormTrain.apply(word_table, position_table, type_table, token_ids.contiguous(), positions.contiguous(),
                                      None if token_types is None else token_types.contiguous(), gamma, beta, eps, keep_bits, inv_keep, dtype)


def meanpool_bwd_packed(grad, seq_start, seq_len, out):
    """Rows seq_start[s] .. + seq_len[s] - 1 of out [T, dim] receive grad[s] / len (ccr_meanpool_bwd_packed); every other row of out
    keeps its bytes.  Returns out."""
    lib = _require_encoder_packed_train()
    assert grad.is_cuda and grad.dtype == torch.float32 and grad.dim() == 2 and grad.is_contiguous()
    n_seq, dim = grad.shape
    for t in (seq_start, seq_len):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n_seq
    assert out.is_cuda and out.dtype in _DTYPES and out.dim() == 2 and out.shape[1] == dim and out.is_contiguous()
    with _on(grad):
        _lib.check(lib.ccr_meanpool_bwd_packed(_ptr(grad), _ptr(seq_start), _ptr(seq_len), _ptr(out), _DTYPES[out.dtype], n_seq, dim,
                                               _stream(grad)), "ccr_meanpool_bwd_packed")
    return out


class _MeanPoolPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, seq_start, seq_len, covers_all):
        pooled = torch.empty(seq_len.numel(), hidden.shape[1], dtype=torch.float32, device=hidden.device)
        meanpool_pack_packed(hidden.detach(), seq_start, seq_len, out_f32=pooled)
        ctx.save_for_backward(seq_start, seq_len)
        ctx.shape, ctx.dtype, ctx.covers_all = tuple(hidden.shape), hidden.dtype, bool(covers_all)
        return pooled

    @staticmethod
    def backward(ctx, grad):
        seq_start, seq_len = ctx.saved_tensors
        make = torch.empty if ctx.covers_all else torch.zeros      # rows of no sequence carry no gradient
        dh = make(ctx.shape, dtype=ctx.dtype, device=grad.device)
        meanpool_bwd_packed(grad.detach().to(torch.float32).contiguous(), seq_start, seq_len, dh)
        return dh, None, None, None


def meanpool_packed(hidden, seq_start, seq_len, covers_all=False):
    """Mean pooling of a packed token array that autograd can differentiate: hidden [T, dim], sequence s = rows seq_start[s] .. +
    seq_len[s] - 1 (int32 cuda) -> fp32 [n_seq, dim], with the bits of meanpool() on the zero-padded form of the same rows, forward and
    backward; no [B, L, dim] tensor exists.  covers_all: the caller vouches that every row of hidden belongs to a sequence (the gradient
    buffer then needs no zero fill)."""
    _require_encoder_packed_train()
    return _MeanPoolPacked.apply(hidden.contiguous(), seq_start, seq_len, covers_all)


class CorpusIndex:
    """A resident 16-bit corpus shard + its search state (ccr_index).  Build once per AL step, query many.

    corpus_bf16: [n_rows, dim] bf16 -- or fp16: the argument keeps its name -- cuda tensor (kept alive by this object; the C index
    borrows it).  `.dtype` is its element type; every search takes queries of that type (TypeError otherwise).
    global_row_offset: id of row 0 in the whole corpus (row-sharded multi-GPU search).
    norm_bounds: [n_rows] fp32 cuda tensor written by pack_bf16 / meanpool_pack(norm_bounds=...) for THESE rows (optional;
    kept alive by this object and not to be rewritten while the index is in use).
    workspace: optional uint8 cuda tensor to search in (not to be shared by two indices that are in use at the same time).
    """

    def __init__(self, corpus_bf16, global_row_offset=0, norm_bounds=None, workspace=None):
        assert corpus_bf16.is_cuda and corpus_bf16.dim() == 2
        code = _check_index_dtype(corpus_bf16.dtype)
        self.dtype = corpus_bf16.dtype
        half = self.dtype != torch.bfloat16
        self._lib = _require_half_index() if half else require_gpu()
        self.corpus = corpus_bf16.contiguous()
        self.n_rows, self.dim = self.corpus.shape
        self.offset = int(global_row_offset)
        self._h = ctypes.c_void_p()
        # workspace: a uint8 cuda tensor to adopt (e.g. the previous step's `index.workspace`: an index built per step then
        # allocates nothing in steady state); replaced by a larger one when a search needs more
        assert workspace is None or (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.device == corpus_bf16.device)
        self._ws = workspace
        self._ws_need = {}
        self._deferred = None
        with _on(self.corpus):
            if norm_bounds is not None:
                _check_bounds(norm_bounds, self.n_rows)
                self._norm_bounds = norm_bounds   # borrowed by the C index, like the corpus
            if half and norm_bounds is None:
                _lib.check(self._lib.ccr_index_create_half(_ptr(self.corpus), self.n_rows, self.dim, code, self.offset,
                                                           _stream(self.corpus), ctypes.byref(self._h)), "ccr_index_create_half")
            elif half:
                _lib.check(self._lib.ccr_index_create_with_norms_half(_ptr(self.corpus), self.n_rows, self.dim, code, self.offset,
                                                                      _ptr(norm_bounds), _stream(self.corpus),
                                                                      ctypes.byref(self._h)), "ccr_index_create_with_norms_half")
            elif norm_bounds is None:
                _lib.check(self._lib.ccr_index_create(_ptr(self.corpus), self.n_rows, self.dim, self.offset,
                                                      _stream(self.corpus), ctypes.byref(self._h)), "ccr_index_create")
            else:  # row-norm bounds from ccr_pack_bf16_ex: no extra pass over the shard, no synchronisation
                _lib.check(self._lib.ccr_index_create_with_norms(_ptr(self.corpus), self.n_rows, self.dim, self.offset,
                                                                 _ptr(norm_bounds), _stream(self.corpus),
                                                                 ctypes.byref(self._h)), "ccr_index_create_with_norms")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            # a deferred search nobody finished: ccr_index_destroy waits for that search's own event before the index's
            # arrays go back to the block cache (the workspace tensor is released after this call returns)
            self._lib.ccr_index_destroy(h)

    @property
    def workspace(self):
        return self._ws

    def _check_queries(self, q):
        """The query matrix of a search: [n_q, dim] cuda rows of the index's element type."""
        if q.dtype != self.dtype:
            raise TypeError(f"queries are {q.dtype} but the index holds {self.dtype} rows: pack the queries with "
                            f"pack_half(dtype={self.dtype})")
        assert q.is_cuda and q.dim() == 2 and q.shape[1] == self.dim

    def library_dtype(self):
        """ccr_index_dtype of the C index, as a torch dtype."""
        _require_half_index()
        code = int(self._lib.ccr_index_dtype(self._h))
        return {v: k for k, v in INDEX_DTYPES.items()}[code]

    def _grow_ws(self, need):
        """The workspace, at least `need` bytes.  A deferred search still owns the current one: complete it before the
        tensor is replaced (or handed to another search)."""
        if getattr(self, "_deferred", None) is not None:
            self.finish()
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.corpus.device)
        return self._ws

    def _workspace(self, n_q, k):
        need = self._ws_need.get((n_q, k))
        if need is None:   # the planner runs three times in there: once per (n_q, k) is enough
            need = self._ws_need[(n_q, k)] = int(self._lib.ccr_search_workspace_bytes(self._h, n_q, k))
        return self._grow_ws(need)

    def search(self, queries_bf16, k, flags=_lib.SEARCH_DEFAULT, out=None, defer=False):
        """-> (scores [n_q, k] fp32, ids [n_q, k] int64 global), canonical order.
        out=(scores, ids): contiguous [n_q, k] destinations (e.g. views of a packed all-gather message).
        defer=True: CCR_SEARCH_ASYNC -- the call returns without synchronising the stream; call finish() before trusting
        the result (it completes the -- rare -- flagged queries and fills last_stats())."""
        q = queries_bf16
        self._check_queries(q)
        q = q.contiguous()
        n_q = q.shape[0]
        if out is None:
            scores = torch.empty(n_q, k, dtype=torch.float32, device=q.device)
            ids = torch.empty(n_q, k, dtype=torch.int64, device=q.device)
        else:
            scores, ids = out
            assert scores.shape == (n_q, k) and ids.shape == (n_q, k) and scores.is_contiguous() and ids.is_contiguous()
            assert scores.dtype == torch.float32 and ids.dtype == torch.int64 and scores.device == q.device == ids.device
        if n_q == 0:
            return scores, ids
        if n_q > MAX_QUERIES_PER_SEARCH:   # the workspace grows with the query count (~0.4 MB per query at k = 100): bounded batches
            assert not defer, "a deferred search takes at most MAX_QUERIES_PER_SEARCH queries"
            for lo in range(0, n_q, MAX_QUERIES_PER_SEARCH):
                hi = min(n_q, lo + MAX_QUERIES_PER_SEARCH)
                self.search(q[lo:hi], k, flags, out=(scores[lo:hi], ids[lo:hi]))
            return scores, ids
        ws = self._workspace(n_q, k)
        if defer:
            flags = int(flags) | _lib.SEARCH_ASYNC
            self._deferred = (q, scores, ids)   # keep the operands alive until finish()
        with _on(q):
            _lib.check(self._lib.ccr_search(self._h, _ptr(q), n_q, k, _ptr(scores), _ptr(ids), _ptr(ws), ws.numel(),
                                            int(flags), _stream(q)), "ccr_search")
        return scores, ids

    def finish(self):
        """Complete a deferred search: waits for THAT search's stream work (its own event -- not for work enqueued after it),
        fills last_stats(), and re-does the queries the search flagged (only then does it synchronise the stream)."""
        with _on(self.corpus):
            _lib.check(self._lib.ccr_search_finish(self._h), "ccr_search_finish")
        self._deferred = None

    def stream_wait_main_pass(self, stream):
        """ccr_search_stream_wait_main_pass: `stream` (a torch.cuda.Stream) is released when side work can usefully start beside this
        index's last search -- deferred or not.  That is when its main pass is done (the side work runs beside the select stage), or, when
        that main pass left CUs free (last_stats()["side_cus"] > 0), as soon as its workgroups are resident: the side work then runs on
        the free CUs beside it.  The call is also the hint that lets the NEXT fused search on the device leave CUs free.  Either way the
        side work must not touch any buffer of the search -- inputs included: the select stage reads them all."""
        _lib.check(self._lib.ccr_search_stream_wait_main_pass(self._h, ctypes.c_void_p(stream.cuda_stream)), "ccr_search_stream_wait_main_pass")

    def search_shard(self, queries_bf16, k, message, defer=False, flags=_lib.SEARCH_DEFAULT):
        """ccr_search_shard: the search writes the packed shard message (header | scores | u32 local rows) that ONE all-gather
        moves (dist.ShardMessage.send).  `message`: uint8 cuda tensor of ccr_shard_message_bytes(n_q, k).  defer=True: no host
        synchronisation; the header's n_flagged is written on the stream, finish() completes the search."""
        q = queries_bf16
        self._check_queries(q)
        q = q.contiguous()
        n_q = q.shape[0]
        assert 0 < n_q <= MAX_QUERIES_PER_SEARCH and 1 <= k <= self.n_rows
        assert message.is_cuda and message.dtype == torch.uint8 and message.is_contiguous() and message.device == q.device
        assert message.numel() >= shard_message_bytes(n_q, k)
        ws = self._workspace(n_q, k)
        if defer:
            flags = int(flags) | _lib.SEARCH_ASYNC
            self._deferred = (q, message)
        with _on(q):
            _lib.check(self._lib.ccr_search_shard(self._h, _ptr(q), n_q, k, _ptr(message), _ptr(ws), ws.numel(), int(flags),
                                                  _stream(q)), "ccr_search_shard")
        return message

    def _special_args(self, queries_bf16, ptr, idx):
        q = queries_bf16
        self._check_queries(q)
        q = q.contiguous()
        ptr = torch.as_tensor(ptr, dtype=torch.int64).cpu().contiguous()
        assert ptr.numel() == q.shape[0] + 1
        idx = torch.as_tensor(idx, dtype=torch.int64).to(q.device).contiguous()
        assert idx.numel() == int(ptr[-1])
        return q, ptr, idx

    def _special_ws(self, need):
        return self._grow_ws(need)

    def search_blocked(self, queries_bf16, k, block_ptr, block_idx, flags=_lib.SEARCH_DEFAULT):
        """Search with per-query blocked GLOBAL ids (CSR: block_ptr [n_q + 1] on the host, block_idx ascending and unique
        inside a query; any length -- ms_marco_eval.py:224-227): blocked columns score -1e6, they are kept not removed.
        Ids outside this shard are ignored.  -> (scores [n_q, k], ids [n_q, k])."""
        q, ptr, idx = self._special_args(queries_bf16, block_ptr, block_idx)
        n_q = q.shape[0]
        scores = torch.empty(n_q, k, dtype=torch.float32, device=q.device)
        ids = torch.empty(n_q, k, dtype=torch.int64, device=q.device)
        if n_q == 0:
            return scores, ids
        if n_q > MAX_QUERIES_PER_SEARCH:
            for lo in range(0, n_q, MAX_QUERIES_PER_SEARCH):
                hi = min(n_q, lo + MAX_QUERIES_PER_SEARCH)
                a, b = int(ptr[lo]), int(ptr[hi])
                s_part, i_part = self.search_blocked(q[lo:hi], k, ptr[lo:hi + 1] - a, idx[a:b], flags)
                scores[lo:hi], ids[lo:hi] = s_part, i_part
            return scores, ids
        pp = ctypes.c_void_p(ptr.data_ptr())
        need = int(self._lib.ccr_search_blocked_workspace_bytes(self._h, n_q, k, pp))
        if need == 0:
            raise _lib.CcrError("ccr_search_blocked: " + self._lib.ccr_last_error().decode("utf-8", "replace"))
        ws = self._special_ws(need)
        with _on(q):
            _lib.check(self._lib.ccr_search_blocked(self._h, _ptr(q), n_q, k, pp, _ptr(idx), _ptr(scores), _ptr(ids), _ptr(ws),
                                                    ws.numel(), int(flags), _stream(q)), "ccr_search_blocked")
        return scores, ids

    def search_sparse_prior(self, queries_bf16, k, prior_ptr, prior_idx, prior_val, flags=_lib.SEARCH_DEFAULT):
        """Top-k of (low-rank score + sparse prior) (bbpr.py:592-595).  CSR prior over GLOBAL column ids (ascending, unique
        per row, <= 4096 per row), fp64 values.  -> (final scores [n_q, k] fp64, ids [n_q, k]) by (final desc, id asc)."""
        require_index_rank("CorpusIndex.search_sparse_prior")
        q, ptr, idx = self._special_args(queries_bf16, prior_ptr, prior_idx)
        val = torch.as_tensor(prior_val, dtype=torch.float64).to(q.device).contiguous()
        assert val.numel() == idx.numel()
        n_q = q.shape[0]
        scores = torch.empty(n_q, k, dtype=torch.float64, device=q.device)
        ids = torch.empty(n_q, k, dtype=torch.int64, device=q.device)
        if n_q == 0:
            return scores, ids
        if n_q > MAX_QUERIES_PER_SEARCH:
            for lo in range(0, n_q, MAX_QUERIES_PER_SEARCH):
                hi = min(n_q, lo + MAX_QUERIES_PER_SEARCH)
                a, b = int(ptr[lo]), int(ptr[hi])
                s_part, i_part = self.search_sparse_prior(q[lo:hi], k, ptr[lo:hi + 1] - a, idx[a:b], val[a:b], flags)
                scores[lo:hi], ids[lo:hi] = s_part, i_part
            return scores, ids
        pp = ctypes.c_void_p(ptr.data_ptr())
        need = int(self._lib.ccr_search_sparse_prior_workspace_bytes(self._h, n_q, k, pp))
        if need == 0:
            raise _lib.CcrError("ccr_search_sparse_prior: " + self._lib.ccr_last_error().decode("utf-8", "replace"))
        ws = self._special_ws(need)
        with _on(q):
            _lib.check(self._lib.ccr_search_sparse_prior(self._h, _ptr(q), n_q, k, pp, _ptr(idx), _ptr(val), _ptr(scores),
                                                         _ptr(ids), _ptr(ws), ws.numel(), int(flags), _stream(q)),
                       "ccr_search_sparse_prior")
        return scores, ids

    def last_stats(self):
        st = _lib.SearchStats()
        _lib.check(self._lib.ccr_search_last_stats(self._h, ctypes.byref(st)), "ccr_search_last_stats")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def last_main_split(self):
        """Unequal query groups (2, 4, 8) of the last search's main pass; 0: equal groups (ccr_search_last_main_split)."""
        return int(self._lib.ccr_search_last_main_split(self._h))

    def last_threshold_phases(self):
        """Group phases per query (16 / 64) of the last search's threshold kernel; 0: small-batch kernel or dense path
        (ccr_search_last_threshold_phases)."""
        return int(self._lib.ccr_search_last_threshold_phases(self._h))

    def scores(self, queries_bf16, mode="canonical"):
        """Dense score matrix [n_q, n_rows] fp32 (ccr_scores).  mode "canonical": the fp64-ordered values the ranking
        reports; "mfma": the same bf16 rows through the MFMA tile kernel (fp32 accumulation)."""
        q = queries_bf16.contiguous()
        self._check_queries(q)
        out = torch.empty(q.shape[0], self.n_rows, dtype=torch.float32, device=q.device)
        if q.shape[0] == 0:
            return out
        m = {"canonical": _lib.SCORES_CANONICAL, "mfma": _lib.SCORES_MFMA}[mode]
        with _on(q):
            _lib.check(self._lib.ccr_scores(self._h, _ptr(q), q.shape[0], m, _ptr(out), _stream(q)), "ccr_scores")
        return out


# ---- ranking on the fp32 embeddings (library version 111, csrc/ccr_rank_f32.hip): the 16-bit search fetches somewhat more than k rows,
# they are re-scored on the kept fp32 rows, and one inequality per query proves that no other row belongs to the fp32 top-k.  The
# reference's CPU path ranks fp32 scores (scripts/ms_marco_eval.py:204-230); ccrec_amd/rank_f32_ref.py restates all of it in numpy ------
_RANK_F32_CHECKED = False
_RANK_PRECISIONS = ("index", "fp32")


def _require_rank_f32():
    """require_gpu() + once: the loaded library keeps and re-scores fp32 rows (ccr_version() >= 111)."""
    global _RANK_F32_CHECKED
    lib = _require_half_index()
    if not _RANK_F32_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.RANK_F32_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the fp32 ranking needs {_lib.RANK_F32_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _RANK_F32_CHECKED = True
    return lib


def rank_precision():
    """What the ranking paths rank: os.environ["CCREC_RANK_PRECISION"] = "index" (the default when unset: the embeddings as the index
    holds them, rounded to CCREC_INDEX_DTYPE) or "fp32" (the fp32 embeddings, through ExactF32Index), read at call time."""
    name = os.environ.get("CCREC_RANK_PRECISION", "index")
    if name not in _RANK_PRECISIONS:
        raise ValueError(f"CCREC_RANK_PRECISION={name!r}: expected 'index' or 'fp32'")
    return name


def require_index_rank(what):
    """Called by the entry points that rank the index's 16-bit rows only: NotImplementedError under CCREC_RANK_PRECISION=fp32."""
    if rank_precision() == "fp32":
        raise NotImplementedError(f"{what} ranks the index's 16-bit rows; CCREC_RANK_PRECISION=fp32 is implemented for "
                                  f"ms_marco_eval.ranking / Retriever / ExactF32Index only: unset CCREC_RANK_PRECISION for this call")


def keep_f32(x, packed, normalize=False, out=None, res_bounds=None):
    """Beside rows that are already packed, keep the fp32 rows the pack rounded (ccr_keep_f32): x fp32 [rows, dim] (cuda), packed
    [rows, padded_dim(dim)] bf16 or fp16 = pack_half(x, normalize=normalize) -> (kept fp32 [rows, padded_dim(dim)], zero-padded, with
    normalize the normalised value the pack rounded; res_bounds [rows] fp32 >= ||kept row - packed row||).  out / res_bounds: write
    into these (slices of shard-sized tensors)."""
    lib = _require_rank_f32()
    code = _check_index_dtype(packed.dtype)
    assert x.is_cuda and x.dim() == 2, "keep_f32 expects a 2-d cuda tensor"
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    rows, dim = x.shape
    pdim = padded_dim(dim)
    assert packed.is_cuda and packed.is_contiguous() and tuple(packed.shape) == (rows, pdim) and packed.device == x.device
    if out is None:
        out = torch.empty(rows, pdim, dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (rows, pdim)
    if res_bounds is None:
        res_bounds = torch.empty(rows, dtype=torch.float32, device=x.device)
    _check_bounds(res_bounds, rows)
    with _on(x):
        _lib.check(lib.ccr_keep_f32(_ptr(x), _ptr(packed), code, int(bool(normalize)), _ptr(out), _ptr(res_bounds), rows, dim, _stream(x)),
                   "ccr_keep_f32")
    return out, res_bounds


class KeptF32:
    """The fp32 side of ONE index build under CCREC_RANK_PRECISION=fp32: `rows` [num, padded_dim(dim)] fp32 (allocated with the first
    batch, when the width is known) and `res_bounds` [num] fp32; generate_embeddings(kept=...) fills both batch by batch."""

    def __init__(self, num, device="cuda"):
        self.num, self.device = int(num), torch.device(device)
        self.rows = None
        self.res_bounds = torch.empty(self.num, dtype=torch.float32, device=self.device)

    def keep(self, emb, packed, lo, normalize):
        if self.rows is None:
            self.rows = torch.empty(self.num, packed.shape[1], dtype=torch.float32, device=self.device)
        hi = lo + emb.shape[0]
        keep_f32(emb, packed, normalize, out=self.rows[lo:hi], res_bounds=self.res_bounds[lo:hi])


def rescore_f32(queries_f32, corpus_f32, cand_ids, cand_s16, k, q_norm_bounds, q_res_bounds, corpus_max, id_offset=0):
    """ccr_rescore_f32: kept fp32 queries [n_q, pdim] and corpus [n_rows, pdim], cand_ids / cand_s16 [n_q, n_cand] = the first n_cand
    results of the 16-bit search (global ids, scores) -> (scores [n_q, k] fp32, ids [n_q, k] int64 by (fp32 score desc, id asc),
    flags [n_q] int32: 0 = no row outside the list can belong to the fp32 top-k, diag [n_q, 4] fp32 = {tau, cut, E, slack})."""
    lib = _require_rank_f32()
    q, d = queries_f32, corpus_f32
    assert q.is_cuda and q.dtype == torch.float32 and q.dim() == 2 and q.is_contiguous()
    assert d.is_cuda and d.dtype == torch.float32 and d.dim() == 2 and d.is_contiguous() and d.shape[1] == q.shape[1] and d.device == q.device
    n_q, pdim = q.shape
    cand_ids, cand_s16 = cand_ids.contiguous(), cand_s16.contiguous()
    assert cand_ids.dtype == torch.int64 and cand_s16.dtype == torch.float32 and cand_ids.shape == cand_s16.shape and cand_ids.dim() == 2
    assert cand_ids.shape[0] == n_q and cand_ids.device == q.device == cand_s16.device
    n_cand = cand_ids.shape[1]
    for t in (q_norm_bounds, q_res_bounds):
        _check_bounds(t, n_q)
    assert corpus_max.is_cuda and corpus_max.dtype == torch.float32 and corpus_max.numel() == 2 and corpus_max.is_contiguous()
    need = _workspace_bytes(lib, "ccr_rescore_f32_workspace_bytes", n_q, n_cand, int(k), pdim)
    diag = torch.empty(need // 4, dtype=torch.float32, device=q.device)
    scores = torch.empty(n_q, k, dtype=torch.float32, device=q.device)
    ids = torch.empty(n_q, k, dtype=torch.int64, device=q.device)
    flags = torch.empty(n_q, dtype=torch.int32, device=q.device)
    with _on(q):
        _lib.check(lib.ccr_rescore_f32(_ptr(q), _ptr(d), d.shape[0], pdim, _ptr(cand_ids), _ptr(cand_s16), n_q, n_cand, int(k), int(id_offset),
                                       _ptr(q_norm_bounds), _ptr(q_res_bounds), _ptr(corpus_max), _ptr(scores), _ptr(ids), _ptr(flags),
                                       _ptr(diag), need, _stream(q)), "ccr_rescore_f32")
    return scores, ids, flags, diag[:4 * n_q].view(n_q, 4)


DENSE_SCORE_BYTES = 1 << 30   # the dense path of ExactF32Index takes index.scores() in query chunks of at most this many bytes


class ExactF32Index:
    """The fp32 ranking of a shard: a CorpusIndex over the 16-bit rows (`.index`) plus the kept fp32 rows and the bounds that tie the two
    together.  search() returns exactly the ranking of the fp32 rows by (s32 desc, id asc) -- rank_f32_ref.ranking.

    corpus_half [n_rows, pdim] bf16 or fp16, corpus_f32 [n_rows, pdim] fp32 and res_bounds [n_rows] = keep_f32's outputs for those rows,
    norm_bounds [n_rows] = the pack's bound of every packed row's norm.  ValueError when a bound is not finite (NaN / inf embeddings,
    or an element that left fp16's range): such a corpus stays on the 16-bit paths.
    max_candidates: the most rows the 16-bit search is asked for per query before the dense path takes over (<= MAX_K)."""

    def __init__(self, corpus_half, corpus_f32, norm_bounds, res_bounds, global_row_offset=0, max_candidates=MAX_K):
        _require_rank_f32()
        max_candidates = int(max_candidates)
        assert 1 <= max_candidates <= MAX_K
        self.index = CorpusIndex(corpus_half, global_row_offset, norm_bounds=norm_bounds)
        self.n_rows, self.dim, self.dtype, self.offset = self.index.n_rows, self.index.dim, self.index.dtype, self.index.offset
        assert corpus_f32.is_cuda and corpus_f32.dtype == torch.float32 and tuple(corpus_f32.shape) == (self.n_rows, self.dim)
        assert corpus_f32.is_contiguous() and corpus_f32.device == self.index.corpus.device
        _check_bounds(norm_bounds, self.n_rows)
        _check_bounds(res_bounds, self.n_rows)
        self.corpus_f32, self.norm_bounds, self.res_bounds = corpus_f32, norm_bounds[:self.n_rows], res_bounds[:self.n_rows]
        self.max_candidates = max_candidates
        self.corpus_max = torch.stack([self.res_bounds.max(), self.norm_bounds.max()])   # {Rmax, Nmax}: read on the device
        if not bool(torch.isfinite(self.corpus_max).all()):
            raise ValueError("ExactF32Index: a row's norm or residual bound is not finite (NaN / inf embeddings, or fp16 overflow): "
                             "rank this corpus on the 16-bit paths (CCREC_RANK_PRECISION=index)")
        self._stats = {"rungs": [], "flagged": [], "dense": 0, "dense_rows": []}

    def last_stats(self):
        """Of the last search(): {"rungs": candidates per rung that ran, "flagged": queries still unverified after each,
        "dense": queries the dense path finished, "dense_rows": rows its filter kept per such query}."""
        return {k: (list(v) if isinstance(v, list) else v) for k, v in self._stats.items()}

    def _search16(self, hq, n, ptr, idx_cpu, rows):
        """The 16-bit search for n rows of the queries `rows` (None: all) of hq, with their block lists."""
        q = hq if rows is None else hq[rows]
        if ptr is None:
            return self.index.search(q, n)
        if rows is None:
            return self.index.search_blocked(q, n, ptr, idx_cpu)
        parts = [idx_cpu[int(ptr[r]):int(ptr[r + 1])] for r in rows.tolist()]
        sub = torch.zeros(len(parts) + 1, dtype=torch.int64)
        sub[1:] = torch.cumsum(torch.tensor([p.numel() for p in parts], dtype=torch.int64), 0)
        return self.index.search_blocked(q, n, sub, torch.cat(parts) if parts else idx_cpu[:0])

    def search(self, queries_f32, k, block_ptr=None, block_idx=None, normalize=False):
        """queries_f32 [n_q, dim] fp32 (cuda; the width before padding), normalize = the corpus was packed with normalize (cos) ->
        (scores [n_q, k] fp32, ids [n_q, k] int64 global).  block_ptr / block_idx: CorpusIndex.search_blocked's CSR of GLOBAL ids
        (blocked rows score -1e6 and stay in the ranking)."""
        q = queries_f32
        assert q.is_cuda and q.dim() == 2 and padded_dim(q.shape[1]) == self.dim, "queries: fp32 [n_q, dim] of the corpus's width"
        k = int(k)
        top = min(self.n_rows, self.max_candidates)
        if not 1 <= k <= top:
            raise ValueError(f"ExactF32Index.search: k={k} outside [1, min(n_rows, max_candidates) = {top}]")
        n_q = q.shape[0]
        dev = q.device
        scores = torch.empty(n_q, k, dtype=torch.float32, device=dev)
        ids = torch.empty(n_q, k, dtype=torch.int64, device=dev)
        stats = self._stats = {"rungs": [], "flagged": [], "dense": 0, "dense_rows": []}
        if n_q == 0:
            return scores, ids
        ptr = idx_cpu = None
        if block_ptr is not None:
            ptr = torch.as_tensor(block_ptr, dtype=torch.int64).cpu().contiguous()
            idx_cpu = torch.as_tensor(block_idx, dtype=torch.int64).cpu().contiguous()
            assert ptr.numel() == n_q + 1 and idx_cpu.numel() == int(ptr[-1])
        # 1. the queries as the index takes them, their kept fp32 rows and their two bounds
        nbq = torch.empty(n_q, dtype=torch.float32, device=dev)
        hq = pack_half(q, self.dtype, normalize=normalize, norm_bounds=nbq)
        yq, rq = keep_f32(q, hq, normalize)
        A = torch.nextafter(nbq + rq, torch.full_like(nbq, float("inf")))   # >= ||kept row||: triangle inequality, one fp32 step up
        if not bool((torch.isfinite(A) & torch.isfinite(rq)).all()):
            raise ValueError("ExactF32Index.search: a query's norm or residual bound is not finite (NaN / inf embeddings): rank these "
                             "queries on the 16-bit paths (CCREC_RANK_PRECISION=index)")
        # 2./3. the rungs: 2 k + 32 rows first, doubled for the queries still unverified
        n = min(top, 2 * k + 32)
        rows = None   # queries still to do (None: all)
        while True:
            s16, i16 = self._search16(hq, n, ptr, idx_cpu, rows)
            sub = slice(None) if rows is None else rows
            s, i, flags, _ = rescore_f32(yq[sub], self.corpus_f32, i16, s16, k, A[sub], rq[sub], self.corpus_max, self.offset)
            scores[sub], ids[sub] = s, i
            bad = flags.nonzero().flatten()          # (the one host read of a rung)
            rows = bad if rows is None else rows[bad]
            stats["rungs"].append(n)
            stats["flagged"].append(int(rows.numel()))
            if rows.numel() == 0 or n == top:
                break
            n = min(top, 2 * n)
        # 4. still unverified: the dense path
        if rows.numel():
            self._dense(hq, yq, A, rq, rows, k, ptr, idx_cpu, scores, ids)
        return scores, ids

    def _dense(self, hq, yq, A, rq, rows, k, ptr, idx_cpu, scores, ids):
        """The queries `rows`: every row whose 16-bit score, raised by the row's own bounds, reaches the last rung's tau (a lower bound of
        the true k-th fp32 score, so the true top-k is among them) is re-scored on the fp32 rows; chunks of MAX_K, merged."""
        stats = self._stats
        Rmax, Nmax = (float(v) for v in self.corpus_max.double().tolist())
        res64, norm64 = self.res_bounds.double(), self.norm_bounds.double()
        per = max(1, DENSE_SCORE_BYTES // (self.n_rows * 4))
        row_list = rows.tolist()
        for lo in range(0, len(row_list), per):
            part = row_list[lo:lo + per]
            s16_all = self.index.scores(hq[rows[lo:lo + per]], "canonical")
            for j, r in enumerate(part):
                s16 = s16_all[j]
                if ptr is not None:
                    blocked = idx_cpu[int(ptr[r]):int(ptr[r + 1])] - self.offset
                    blocked = blocked[(blocked >= 0) & (blocked < self.n_rows)]
                    s16[blocked.to(s16.device)] = -1e6
                tau = scores[r, k - 1].double()
                a, rr = A[r].double(), rq[r].double()
                s64 = s16.double()
                slack = 2.0 ** -21 * (s64.abs() + tau.abs()) + 2.0 ** -40 * (a * (Nmax + Rmax))
                keep = ((s64 + (a * res64 + rr * norm64)) + slack >= tau).nonzero().flatten()
                m = int(keep.numel())
                assert m >= k, "the dense filter keeps the last rung's own top-k"
                parts_s, parts_i = [], []
                for c in range(0, m, MAX_K):
                    rows_c = keep[c:c + MAX_K]
                    n_c = int(rows_c.numel())
                    s, i, _, _ = rescore_f32(yq[r:r + 1], self.corpus_f32, (rows_c + self.offset)[None, :], s16[rows_c][None, :], n_c,
                                             A[r:r + 1], rq[r:r + 1], self.corpus_max, self.offset)
                    if n_c < k:   # a short last chunk: entries below every real one fill its list
                        s = torch.cat([s, torch.full((1, k - n_c), float("-inf"), device=s.device)], 1)
                        i = torch.cat([i, torch.full((1, k - n_c), 1 << 62, dtype=torch.int64, device=i.device)], 1)
                    parts_s.append(s[:, :k])
                    parts_i.append(i[:, :k])
                if len(parts_s) == 1:
                    scores[r], ids[r] = parts_s[0][0], parts_i[0][0]
                else:
                    ms, mi = merge_topk(torch.stack(parts_s), torch.stack(parts_i))
                    scores[r], ids[r] = ms[0], mi[0]
                stats["dense"] += 1
                stats["dense_rows"].append(m)


def _rank_strided(t):
    """[R, n_q, k] tensor whose [n_q, k] lists are dense; only the rank stride is free (a view of a gathered message)."""
    return t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2] and t.stride(0) >= t.shape[1] * t.shape[2]


def merge_topk(scores, ids):
    """[R, n_q, k] per-shard canonical lists -> global ([n_q, k], [n_q, k]).  Rank-strided views are merged in place."""
    lib = require_gpu()
    assert scores.is_cuda and scores.dtype == torch.float32 and ids.dtype == torch.int64 and scores.shape == ids.shape
    if not _rank_strided(scores):
        scores = scores.contiguous()
    if not _rank_strided(ids):
        ids = ids.contiguous()
    R, n_q, k = scores.shape
    os_ = torch.empty(n_q, k, dtype=torch.float32, device=scores.device)
    oi = torch.empty(n_q, k, dtype=torch.int64, device=scores.device)
    with _on(scores):
        _lib.check(lib.ccr_merge_topk_strided(_ptr(scores), _ptr(ids), scores.stride(0), ids.stride(0), R, n_q, k, _ptr(os_),
                                              _ptr(oi), _stream(scores)), "ccr_merge_topk")
    return os_, oi


def shard_message_bytes(n_q, k):
    """Bytes of one packed shard message (ccr_shard_message_bytes): 32-byte header | fp32 scores | u32 local rows."""
    rows_at = (_lib.SHARD_HEADER_BYTES + n_q * k * 4 + 15) // 16 * 16
    return (rows_at + n_q * k * 4 + 15) // 16 * 16


def shard_message_fill(message, n_q, k, scores, ids, row_offset, n_rows):
    """Ordinary results ([n_q, k_valid] fp32 scores, int64 GLOBAL ids; k_valid <= k) -> packed shard message."""
    lib = require_gpu()
    k_valid = scores.shape[1] if scores is not None and scores.dim() == 2 else 0
    assert message.is_cuda and message.dtype == torch.uint8 and message.numel() >= shard_message_bytes(n_q, k)
    if k_valid:
        scores, ids = scores.contiguous(), ids.contiguous()
        assert scores.dtype == torch.float32 and ids.dtype == torch.int64 and scores.shape == ids.shape == (n_q, k_valid)
    with _on(message):
        _lib.check(lib.ccr_shard_message_fill(_ptr(message), n_q, k, k_valid, _ptr(scores) if k_valid else None,
                                              _ptr(ids) if k_valid else None, int(row_offset), int(n_rows), _stream(message)),
                   "ccr_shard_message_fill")
    return message


def merge_shard_messages(gathered, world, n_q, k):
    """R gathered shard messages (uint8 [R * stride]) -> global ([n_q, k] fp32, [n_q, k] int64 global ids)."""
    lib = require_gpu()
    assert gathered.is_cuda and gathered.dtype == torch.uint8 and gathered.is_contiguous() and gathered.numel() % world == 0
    stride = gathered.numel() // world
    os_ = torch.empty(n_q, k, dtype=torch.float32, device=gathered.device)
    oi = torch.empty(n_q, k, dtype=torch.int64, device=gathered.device)
    with _on(gathered):
        _lib.check(lib.ccr_merge_shard_messages(_ptr(gathered), stride, world, n_q, k, _ptr(os_), _ptr(oi), _stream(gathered)),
                   "ccr_merge_shard_messages")
    return os_, oi


SHORT_LIST_LDS_BYTES = 96 * 1024   # ccr_merge_short_lists merges a query's R lists in LDS: R * k_list * 12 bytes must fit


def merge_short_lists(gathered, world, n_q, k_list, k_out, out=None):
    """R gathered SHORT shard messages (k_list entries per query each) -> the k_out best of every query plus the verification of the
    shortcut (ccr_merge_short_lists): ([n_q, k_out] fp32, [n_q, k_out] int64 global ids, flags [n_q] int32 -- 1 where a shard's list
    was consumed to its end although the shard holds more rows: that query must be repeated with full lists --, n_flagged [1] int32)."""
    lib = require_gpu()
    assert gathered.is_cuda and gathered.dtype == torch.uint8 and gathered.is_contiguous() and gathered.numel() % world == 0
    assert 1 <= k_list <= k_out <= world * k_list and world * k_list * 12 <= SHORT_LIST_LDS_BYTES
    stride = gathered.numel() // world
    dev = gathered.device
    if out is not None:      # (scores, ids, zeroed flags, zeroed count) allocated by the caller (dist.ShardExchange: on another stream)
        os_, oi, flags, count = out
    else:
        os_ = torch.empty(n_q, k_out, dtype=torch.float32, device=dev)
        oi = torch.empty(n_q, k_out, dtype=torch.int64, device=dev)
        flags = torch.zeros(max(1, n_q), dtype=torch.int32, device=dev)[:n_q]
        count = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(gathered):
        _lib.check(lib.ccr_merge_short_lists(_ptr(gathered), stride, world, n_q, k_list, k_out, _ptr(os_), _ptr(oi), _ptr(flags) if n_q else _ptr(count),
                                             _ptr(count), _stream(gathered)), "ccr_merge_short_lists")
    return os_, oi, flags, count


def apply_block(scores, ids, block_ptr, block_idx, k_out, n_rows_total):
    """Post-filter an over-fetched canonical list with per-query blocked ids (ms_marco_eval.py:224-227)."""
    lib = require_gpu()
    n_q, k_in = scores.shape
    os_ = torch.empty(n_q, k_out, dtype=torch.float32, device=scores.device)
    oi = torch.empty(n_q, k_out, dtype=torch.int64, device=scores.device)
    block_ptr = block_ptr.to(device=scores.device, dtype=torch.int64).contiguous()
    block_idx = block_idx.to(device=scores.device, dtype=torch.int64).contiguous()
    if block_idx.numel() == 0:
        block_idx = torch.zeros(1, dtype=torch.int64, device=scores.device)
    with _on(scores):
        _lib.check(lib.ccr_apply_block(_ptr(scores.contiguous()), _ptr(ids.contiguous()), n_q, k_in, _ptr(block_ptr),
                                       _ptr(block_idx), int(n_rows_total), _ptr(os_), _ptr(oi), k_out, _stream(scores)),
                   "ccr_apply_block")
    return os_, oi


def colsum_bf16(x):
    """Column sums of a bf16 -- or fp16: it follows the tensor it is given -- [rows, dim] cuda matrix in fp64 (ccr_colsum_bf16 /
    ccr_colsum_half) -> [dim] float64."""
    assert x.is_cuda and x.dim() == 2
    code = _check_index_dtype(x.dtype)
    lib = require_gpu() if x.dtype == torch.bfloat16 else _require_half_index()
    x = x.contiguous()
    out = torch.empty(x.shape[1], dtype=torch.float64, device=x.device)
    with _on(x):
        if x.dtype == torch.bfloat16:
            _lib.check(lib.ccr_colsum_bf16(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _stream(x)), "ccr_colsum_bf16")
        else:
            _lib.check(lib.ccr_colsum_half(_ptr(x), x.shape[0], x.shape[1], code, _ptr(out), _stream(x)), "ccr_colsum_half")
    return out


def _f32_on(t, dev):   # t (or None) as a contiguous fp32 tensor on dev: a value the library reads on the device
    if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()   # stays on the device either way
    return t


def _grad_as(g, dtype):   # an fp32 gradient in its input's dtype
    return g if dtype == torch.float32 else g.to(dtype)


def _workspace_bytes(lib, name, *shape):   # lib.<name>(*shape): host arithmetic only; 0 = the shape was refused, the library says why
    ws_bytes = int(getattr(lib, name)(*shape))
    if ws_bytes == 0:
        raise _lib.CcrError(name + ": " + lib.ccr_last_error().decode("utf-8", "replace"))
    return ws_bytes


def _one_buffer(packed_bytes, ws_bytes, n_lse):
    """A forward's single uint8 buffer [packed operands | workspace | lse: n_lse floats at the tail]
    -> (bytes of the packed operands padded to 256 = the workspace's offset, workspace bytes, total bytes)."""
    head = (packed_bytes + 255) // 256 * 256
    return head, ws_bytes, head + (ws_bytes + 255) // 256 * 256 + n_lse * 4


_INBATCH_LAYOUT = {}   # (B, dim) -> _one_buffer(...): (bytes of the packed blocks padded to 256, workspace bytes, total bytes)


class _InBatchCE(torch.autograd.Function):
    """loss = CE([Q P^T | Q N^T] * inv_T, arange(B)).mean()   (bbpr.py:205-212), bf16 operands, fp32 accumulate.

    The step is ~0.12 ms of kernels, so the host path is kept to a handful of Python operations: ONE allocation per forward holds the
    packed bf16 operands, the library's workspace and lse (addresses by integer arithmetic, no tensor views), ONE library call rounds
    the three fp32 blocks to bf16 (torch's .to(bfloat16) bits) and runs the forward; the backward is one allocation and one call.
    The buffer belongs to THIS forward until its backward has run (the backward reads the forward's logits there; the library checks
    the workspace's stamp on the device)."""

    @staticmethod
    def forward(ctx, q, p, n, inv_temperature):
        lib = require_gpu()
        B, dim = q.shape
        assert q.is_cuda and p.shape == q.shape == n.shape and p.device == q.device == n.device, "three [B, dim] blocks on one device"
        lay = _INBATCH_LAYOUT.get((B, dim))
        if lay is None:
            lay = _INBATCH_LAYOUT[(B, dim)] = _one_buffer(3 * B * dim * 2, int(lib.ccr_inbatch_ce_workspace_bytes(B, dim)), B)
        head, ws_bytes, total = lay
        dev = q.device
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        base = buf.data_ptr()
        lse_ptr = base + total - B * 4
        stream = torch.cuda.current_stream(dev).cuda_stream
        fast = (q.dtype == p.dtype == n.dtype == torch.float32 and q.is_contiguous() and p.is_contiguous() and n.is_contiguous()
                and (q.data_ptr() | p.data_ptr() | n.data_ptr()) % 16 == 0)   # (dim % 16 == 0: inbatch_ce sends no other width here)
        with _on(q):
            if fast:
                _lib.check(lib.ccr_inbatch_ce_fwd_f32(q.data_ptr(), p.data_ptr(), n.data_ptr(), B, dim, float(inv_temperature), base,
                                                      loss.data_ptr(), lse_ptr, base + head, ws_bytes, stream), "ccr_inbatch_ce_fwd_f32")
            else:   # other dtypes / strided inputs: torch copies round to bf16, then the forward on the packed blocks
                packed = buf[:3 * B * dim * 2].view(torch.bfloat16).view(3, B, dim)
                for dst, t in zip(packed, (q, p, n)):
                    dst.copy_(t.detach())
                blk = B * dim * 2
                _lib.check(lib.ccr_inbatch_ce_fwd(base, base + blk, base + 2 * blk, B, dim, float(inv_temperature), loss.data_ptr(), lse_ptr,
                                                  base + head, ws_bytes, stream), "ccr_inbatch_ce_fwd")
        ctx.save_for_backward(buf)
        ctx.lay = (B, dim, head, ws_bytes, total, float(inv_temperature), q.dtype, p.dtype, n.dtype)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        lib = require_gpu()
        (buf,) = ctx.saved_tensors
        B, dim, head, ws_bytes, total, inv_t, tq, tp, tn = ctx.lay
        dev = buf.device
        grads = torch.empty(3, B, dim, dtype=torch.float32, device=dev)
        g = _f32_on(grad_out, dev)
        base, gp, blk = buf.data_ptr(), grads.data_ptr(), B * dim
        with _on(buf):
            _lib.check(lib.ccr_inbatch_ce_bwd_dev(base, base + 2 * blk, base + 4 * blk, base + total - B * 4, B, dim, inv_t, g.data_ptr(),
                                                  gp, gp + 4 * blk, gp + 8 * blk, base + head, ws_bytes, torch.cuda.current_stream(dev).cuda_stream),
                       "ccr_inbatch_ce_bwd")
        dq, dp, dn = grads.unbind(0)
        return _grad_as(dq, tq), _grad_as(dp, tp), _grad_as(dn, tn), None


def inbatch_ce(q, p, n, inv_temperature):
    """The square loss of three [B, dim] blocks.  The square kernels take widths that are multiples of 16; any other width >= 1 is
    the same loss in the pool form (pool = [p ; n], labels arange(B)), which zero-pads the width."""
    assert q.dim() == 2 and p.shape == q.shape == n.shape, "three [B, dim] blocks"
    if q.shape[1] % 16 != 0:
        labels = torch.arange(q.shape[0], dtype=torch.int32, device=q.device)
        return pool_ce(q, torch.cat([p, n]), labels, inv_temperature)
    return _InBatchCE.apply(q, p, n, inv_temperature)


def pool_ce_forward(q, c, labels, inv_temperature, weights=None):
    """The forward half of pool_ce without autograd (dist.gathered_pool_ce builds its own graph node on it):
    -> (out3, state).  out3 = [loss, numerator sum w ce, denominator sum w] fp32 on the device; state goes to pool_ce_backward.
    ONE allocation holds the packed bf16 operands, the library's workspace (the scaled logits stay there for the backward) and lse.
    fp32 contiguous operands of a width that is a multiple of 8 are rounded by the library in the same call (torch's
    .to(bfloat16) bits); anything else (other dtypes, strides, widths zero-padded to a multiple of 8 as pack_bf16 does) goes
    through torch copies into the packed block first."""
    lib = require_gpu()
    assert q.is_cuda and q.dim() == 2 and c.dim() == 2 and q.shape[1] == c.shape[1] and c.device == q.device, "q [n_q, dim], c [n_c, dim] on one device"
    n_q, dim = q.shape
    n_c = c.shape[0]
    assert n_q >= 1 and n_c >= 1 and dim >= 1, "pool_ce needs at least one query, one candidate and one column"
    dev = q.device
    labels = labels.detach().to(device=dev, dtype=torch.int32).contiguous()
    assert labels.shape == (n_q,), "one label per query"
    if weights is not None:
        weights = weights.detach().to(device=dev, dtype=torch.float32).contiguous()
        assert weights.shape == (n_q,), "one weight per query"
    pdim = padded_dim(dim)
    head, ws_bytes, total = _one_buffer((n_q + n_c) * pdim * 2, _workspace_bytes(lib, "ccr_pool_ce_workspace_bytes", n_q, n_c, pdim), n_q)
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    base = buf.data_ptr()
    lse_ptr = base + total - n_q * 4
    stream = torch.cuda.current_stream(dev).cuda_stream
    fast = (q.dtype == c.dtype == torch.float32 and q.is_contiguous() and c.is_contiguous() and pdim == dim
            and (q.data_ptr() | c.data_ptr()) % 16 == 0)
    wp = weights.data_ptr() if weights is not None else None
    with _on(q):
        if fast:
            _lib.check(lib.ccr_pool_ce_fwd_f32(q.data_ptr(), c.data_ptr(), labels.data_ptr(), wp, n_q, n_c, dim, float(inv_temperature), base,
                                               out3.data_ptr(), lse_ptr, base + head, ws_bytes, stream), "ccr_pool_ce_fwd_f32")
        else:
            packed = buf[:(n_q + n_c) * pdim * 2].view(torch.bfloat16).view(n_q + n_c, pdim)
            if pdim != dim:
                packed[:, dim:].zero_()
            packed[:n_q, :dim].copy_(q.detach())
            packed[n_q:, :dim].copy_(c.detach())
            _lib.check(lib.ccr_pool_ce_fwd(base, base + n_q * pdim * 2, labels.data_ptr(), wp, n_q, n_c, pdim, float(inv_temperature),
                                           out3.data_ptr(), lse_ptr, base + head, ws_bytes, stream), "ccr_pool_ce_fwd")
    return out3, (buf, labels, weights, (n_q, n_c, dim, pdim, head, ws_bytes, total, float(inv_temperature)))


def pool_ce_backward(state, grad_out, W=None):
    """-> (dq [n_q, dim], dc [n_c, dim]) fp32: grad_out times the gradient of numerator / W.  W: None = the forward's own
    denominator, or a 1-element fp32 device tensor (the denominator summed over all ranks).  One allocation, one library call;
    grad_out and W are read on the device."""
    lib = require_gpu()
    buf, labels, weights, (n_q, n_c, dim, pdim, head, ws_bytes, total, inv_t) = state
    dev = buf.device
    grads = torch.empty(n_q + n_c, pdim, dtype=torch.float32, device=dev)
    g, W = _f32_on(grad_out, dev), _f32_on(W, dev)
    base, gp = buf.data_ptr(), grads.data_ptr()
    with _on(buf):
        _lib.check(lib.ccr_pool_ce_bwd_dev(base, base + n_q * pdim * 2, labels.data_ptr(), weights.data_ptr() if weights is not None else None,
                                           base + total - n_q * 4, n_q, n_c, pdim, inv_t, g.data_ptr(), W.data_ptr() if W is not None else None,
                                           gp, gp + n_q * pdim * 4, base + head, ws_bytes, torch.cuda.current_stream(dev).cuda_stream),
                   "ccr_pool_ce_bwd_dev")
    return grads[:n_q, :dim], grads[n_q:, :dim]


class _PoolCE(torch.autograd.Function):
    """loss = sum_i w_i (logsumexp_j s_ij - s_{i,label_i}) / sum_i w_i,  s = inv_T q c^T: bf16 operands, fp32 accumulate.
    The buffer belongs to THIS forward until its backward has run (the backward reads the forward's logits there; the library
    checks the workspace's stamp on the device)."""

    @staticmethod
    def forward(ctx, q, c, labels, weights, inv_temperature):
        out3, state = pool_ce_forward(q, c, labels, inv_temperature, weights)
        ctx.state, ctx.dtypes = state, (q.dtype, c.dtype)
        return out3[0]

    @staticmethod
    def backward(ctx, grad_out):
        dq, dc = pool_ce_backward(ctx.state, grad_out)
        tq, tc = ctx.dtypes
        return _grad_as(dq, tq), _grad_as(dc, tc), None, None, None


def pool_ce(q, c, labels, inv_temperature, weights=None):
    """Weighted cross-entropy of n_q queries over a pool of n_c candidates (ccr_pool_ce_*): several hard negatives per query,
    per-sample weights, or a pool gathered from other ranks.  labels [n_q] index the pool; labels and weights get no gradient;
    gradients come back in the inputs' dtypes.  A label outside the pool gives a NaN loss and NaN gradients (checked on the
    device, no read-back)."""
    return _PoolCE.apply(q, c, labels, weights, inv_temperature)


# ---- the "bpr" objective (ccr_bpr_*; src/ccrec/models/bbpr.py:153-185) ------------------------------------------------------------
_BPR_CHECKED = False


def _require_bpr():
    """require_gpu() + once: the loaded library has the ccr_bpr_* entry points (ccr_version() >= 102)."""
    global _BPR_CHECKED
    lib = require_gpu()
    if not _BPR_CHECKED:
        have = int(lib.ccr_version())
        if have < _lib.BPR_VERSION:
            raise _lib.CcrError(f"{_lib.LIB_PATH} is version {have}, the bpr ops need {_lib.BPR_VERSION}: rebuild it "
                                f"(python -c 'import __graft_entry__ as g; g.build()')")
        _BPR_CHECKED = True
    return lib


def bpr_frozen_supported(dim):
    """Widths the fused frozen-tower loss takes (ccr_bpr_frozen_*); BprStep runs its torch formulation at any other."""
    return dim % 64 == 0 and 64 <= dim <= 2048


def bpr_proposal_cdf(proposal):
    """Inclusive fp64 prefix sums of the item proposal (once per training set): the second input of bpr_sample_negatives."""
    return torch.cumsum(proposal.detach().to(torch.float64), 0)


def bpr_sample_negatives(users, n_negatives, proposal, proposal_cdf, prior=None, t0=0.0, uniforms=None, generator=None):
    """Negatives of bbpr.py:160-179 -> [n_negatives, B] int64, as multinomial(softmax(f(prior[users]) + log proposal), n, True).T
    draws them, by inverse CDF over the sparse row (ccr_bpr_sample): no [B, n_items] matrix.
    users [B] int64; proposal [n_items] fp32 > 0 and proposal_cdf = bpr_proposal_cdf(proposal); prior = None (draw from the
    proposal alone, bbpr.py:176-179) or (ptr [n_users + 1] int64, idx int64 ascending and unique per row, t fp32 =
    training_prior_fcn(value), max_row_nnz) on the device, with t0 = training_prior_fcn(0).  uniforms [n_negatives, B] fp64 in
    [0, 1): drawn here with torch.rand (generator) when None.  With replacement only."""
    lib = _require_bpr()
    dev = proposal.device
    users = users.detach().to(device=dev, dtype=torch.int64).contiguous()
    B, n_neg, n_items = users.numel(), int(n_negatives), proposal.numel()
    assert users.dim() == 1 and B >= 1 and n_neg >= 1, "users [B], n_negatives >= 1"
    assert proposal.is_cuda and proposal.dtype == torch.float32 and proposal.is_contiguous(), "proposal: fp32 [n_items] on the device"
    assert proposal_cdf.device == dev and proposal_cdf.dtype == torch.float64 and proposal_cdf.is_contiguous() and proposal_cdf.numel() == n_items, \
        "proposal_cdf: bpr_proposal_cdf(proposal)"
    if uniforms is None:
        uniforms = torch.rand(n_neg, B, dtype=torch.float64, device=dev, generator=generator)
    assert uniforms.device == dev and uniforms.dtype == torch.float64 and uniforms.is_contiguous() and uniforms.shape == (n_neg, B), \
        "uniforms: fp64 [n_negatives, B] on the device"
    if prior is not None:
        ptr, idx, t, max_row_nnz = prior
        assert ptr.device == idx.device == t.device == dev and ptr.dtype == idx.dtype == torch.int64 and t.dtype == torch.float32
        assert ptr.is_contiguous() and idx.is_contiguous() and t.is_contiguous() and idx.numel() == t.numel()
        n_users = ptr.numel() - 1
    else:
        ptr = idx = t = None
        n_users, max_row_nnz = 0, 0
    out = torch.empty(n_neg, B, dtype=torch.int64, device=dev)
    with _on(proposal):
        _lib.check(lib.ccr_bpr_sample(_ptr(users), B, n_neg, n_users, _ptr(ptr), _ptr(idx), _ptr(t), float(t0), _ptr(proposal), _ptr(proposal_cdf),
                                      n_items, _ptr(uniforms), int(max_row_nnz), _ptr(out), _stream(proposal)), "ccr_bpr_sample")
    return out


def _bpr_frozen_args(table, ptr_i, ptr_j, ptr_nj, w):
    assert table.is_cuda and table.dtype == torch.float32 and table.dim() == 2 and table.is_contiguous(), "table: fp32 [n_rows, dim] on the device"
    dev = table.device
    ptr_i, ptr_j, ptr_nj = (p.detach().to(device=dev, dtype=torch.int64).contiguous() for p in (ptr_i, ptr_j, ptr_nj))
    w = w.detach().to(device=dev, dtype=torch.float32).contiguous()
    B = ptr_i.numel()
    assert ptr_i.dim() == 1 and ptr_j.shape == (B,) and w.shape == (B,) and ptr_nj.dim() == 2 and ptr_nj.shape[1] == B, \
        "ptr_i, ptr_j, w [B] and ptr_nj [n_negatives, B]"
    return ptr_i, ptr_j, ptr_nj, w, B, ptr_nj.shape[0]


class _BprFrozen(torch.autograd.Function):
    """loss = sum_nb w_b softplus(-(e_i . e_j - e_i . e_nb)) / (n_neg sum_b w_b),  e = LayerNorm(table[ptr]); gradients with respect to
    the LayerNorm's weight and bias only (the table is a frozen buffer).  Nothing is saved but the inputs: the backward reads and
    normalises the rows again."""

    @staticmethod
    def forward(ctx, table, weight, bias, eps, ptr_i, ptr_j, ptr_nj, w):
        lib = _require_bpr()
        ptr_i, ptr_j, ptr_nj, w, B, n_neg = _bpr_frozen_args(table, ptr_i, ptr_j, ptr_nj, w)
        n_rows, dim = table.shape
        dev = table.device
        assert (weight is None) == (bias is None), "LayerNorm weight and bias: both or neither"
        gb = None
        if weight is not None:   # one [2, dim] block: gamma and beta 16-byte aligned whatever views the module holds
            gb = torch.stack([weight.detach().to(device=dev, dtype=torch.float32), bias.detach().to(device=dev, dtype=torch.float32)])
            assert gb.shape == (2, dim), "LayerNorm weight and bias [dim]"
        ws_bytes = _workspace_bytes(lib, "ccr_bpr_frozen_workspace_bytes", B, n_neg, dim)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        with _on(table):
            _lib.check(lib.ccr_bpr_frozen_fwd(_ptr(table), n_rows, dim, gb.data_ptr() if gb is not None else None,
                                              gb.data_ptr() + dim * 4 if gb is not None else None, float(eps), _ptr(ptr_i), _ptr(ptr_j), _ptr(ptr_nj),
                                              _ptr(w), B, n_neg, _ptr(out3), _ptr(ws), ws_bytes, _stream(table)), "ccr_bpr_frozen_fwd")
        ctx.save_for_backward(table, gb, ptr_i, ptr_j, ptr_nj, w, out3)
        ctx.lay = (float(eps), weight.dtype if weight is not None else None, bias.dtype if bias is not None else None)
        return out3[0]

    @staticmethod
    def backward(ctx, grad_out):
        lib = _require_bpr()
        table, gb, ptr_i, ptr_j, ptr_nj, w, out3 = ctx.saved_tensors
        eps, tw, tb = ctx.lay
        if gb is None:
            raise _lib.CcrError("bpr_frozen_loss: no gradient without a LayerNorm weight and bias (elementwise_affine=False)")
        n_rows, dim = table.shape
        B, n_neg = ptr_i.numel(), ptr_nj.shape[0]
        dev = table.device
        g = _f32_on(grad_out, dev)
        grads = torch.empty(2, dim, dtype=torch.float32, device=dev)
        ws_bytes = _workspace_bytes(lib, "ccr_bpr_frozen_workspace_bytes", B, n_neg, dim)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with _on(table):
            _lib.check(lib.ccr_bpr_frozen_bwd_dev(_ptr(table), n_rows, dim, gb.data_ptr(), gb.data_ptr() + dim * 4, eps, _ptr(ptr_i), _ptr(ptr_j),
                                                  _ptr(ptr_nj), _ptr(w), B, n_neg, out3.data_ptr() + 8, _ptr(g), grads.data_ptr(),
                                                  grads.data_ptr() + dim * 4, _ptr(ws), ws_bytes, _stream(table)), "ccr_bpr_frozen_bwd_dev")
        dw, db = grads.unbind(0)
        return None, _grad_as(dw, tw), _grad_as(db, tb), None, None, None, None, None


def bpr_frozen_loss(table, layer_norm_weight, layer_norm_bias, eps, ptr_i, ptr_j, ptr_nj, w):
    """The bpr loss of one step over cached CLS rows (bbpr.py:144-147, 180-185 with forward = LayerNorm(all_cls[ptr])), fused
    (ccr_bpr_frozen_*): table [n_rows, dim] fp32, dim a multiple of 64 up to 2048; ptr_i, ptr_j [B], ptr_nj [n_negatives, B] rows
    of the table; w [B].  Autograd with respect to layer_norm_weight and layer_norm_bias (both None: forward only).  A pointer
    outside the table gives a NaN loss and NaN gradients, all-zero weights NaN (checked on the device, no read-back)."""
    return _BprFrozen.apply(table, layer_norm_weight, layer_norm_bias, eps, ptr_i, ptr_j, ptr_nj, w)
