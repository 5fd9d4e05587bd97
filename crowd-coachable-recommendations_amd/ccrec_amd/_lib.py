"""ctypes binding of libccr_hip.so (include/ccr_retrieval.h).  No CPU fallback: if the library or a
ROCm device is missing, every op raises -- the product path never routes through oracle/ or torch math."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libccr_hip.so")

CCR_OK = 0
CCR_ERR_INVALID, CCR_ERR_HIP, CCR_ERR_WORKSPACE, CCR_ERR_BLOCK_ID = -1, -2, -3, -4
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
SEARCH_DEFAULT, SEARCH_FORCE_DENSE, SEARCH_FORCE_FUSED, SEARCH_ASYNC = 0, 1, 2, 4
SCORES_CANONICAL, SCORES_MFMA = 0, 1

EXPORTS = [
    "ccr_last_error", "ccr_version", "ccr_pack_bf16", "ccr_pack_bf16_ex", "ccr_meanpool_pack_bf16", "ccr_meanpool_pack_bf16_ex", "ccr_index_create",
    "ccr_index_create_with_norms", "ccr_index_destroy",
    "ccr_index_rows", "ccr_index_dim", "ccr_search_workspace_bytes", "ccr_search", "ccr_search_last_stats",
    "ccr_merge_topk", "ccr_merge_topk_strided", "ccr_apply_block", "ccr_inbatch_ce_workspace_bytes", "ccr_inbatch_ce_fwd", "ccr_inbatch_ce_bwd", "ccr_inbatch_ce_bwd_dev", "ccr_rank_metrics",
    "ccr_search_finish", "ccr_scores", "ccr_search_blocked_workspace_bytes", "ccr_search_blocked",
    "ccr_search_sparse_prior_workspace_bytes", "ccr_search_sparse_prior", "ccr_colsum_bf16", "ccr_meanpool_bwd", "ccr_bm25_index_create", "ccr_bm25_index_destroy", "ccr_bm25_search_workspace_bytes",
    "ccr_bm25_search", "ccr_pack_bf16_padded", "ccr_shard_message_bytes", "ccr_search_shard", "ccr_shard_message_fill", "ccr_merge_shard_messages",
    "ccr_attention_bf16", "ccr_add_layernorm", "ccr_meanpool_pack_bf16_packed", "ccr_embed_layernorm", "ccr_gelu_bf16",
    "ccr_attention_half", "ccr_add_layernorm_half", "ccr_embed_layernorm_half", "ccr_gelu_half", "ccr_merge_short_lists",
    "ccr_bm25_search_workspace_bytes_k", "ccr_bm25_search_last_stats", "ccr_bm25_index_set_idf", "ccr_inbatch_pack3_bf16", "ccr_inbatch_ce_fwd_f32",
    "ccr_search_stream_wait_main_pass", "ccr_pool_ce_workspace_bytes", "ccr_pool_ce_fwd", "ccr_pool_ce_fwd_f32", "ccr_pool_ce_bwd_dev",
    "ccr_bpr_sample", "ccr_bpr_frozen_workspace_bytes", "ccr_bpr_frozen_fwd", "ccr_bpr_frozen_bwd_dev",
    "ccr_attention_fwd_train_half", "ccr_attention_bwd_workspace_bytes", "ccr_attention_bwd_half", "ccr_add_layernorm_bwd_half", "ccr_gelu_bwd_half",
    "ccr_dropout_bits_rows", "ccr_dropout_bits_attention", "ccr_dropout_apply", "ccr_attention_fwd_train_drop_half", "ccr_attention_bwd_drop_half",
    "ccr_add_layernorm_drop_half", "ccr_add_layernorm_bwd_drop_half", "ccr_search_last_main_split",
    "ccr_search_last_threshold_phases", "ccr_adamw_step",
    "ccr_embed_layernorm_train_half", "ccr_embed_layernorm_bwd_half", "ccr_embedding_grad", "ccr_meanpool_bwd_packed",
    "ccr_pack_half_ex", "ccr_pack_half_padded", "ccr_meanpool_pack_half_ex", "ccr_meanpool_pack_half_packed", "ccr_index_create_half",
    "ccr_index_create_with_norms_half", "ccr_index_dtype", "ccr_colsum_half",
    "ccr_grad_stats_workspace_bytes", "ccr_grad_stats", "ccr_adamw_control_update", "ccr_adamw_step_scaled",
    "ccr_keep_f32", "ccr_rescore_f32_workspace_bytes", "ccr_rescore_f32",
    "ccr_attention_bias_half",
    "ccr_attention_head_half",
]

MIN_VERSION = 101   # ccr_version() of the oldest library load() accepts (101: the ccr_pool_ce_* entry points)
BPR_VERSION = 102   # ... and the one the ccr_bpr_* entry points came with (ops checks it on their first use)
ENCODER_TRAIN_VERSION = 103   # ... and the encoder layer kernels' training forward and backward (ccr_attention_bwd_half and its kin)
ENCODER_DROPOUT_VERSION = 104   # ... and the keep-bit generators and the layer kernels that read the bits (ccr_dropout_bits_rows and its kin)
QSPLIT_VERSION = 105   # ... and the main pass's unequal query groups with their getter (ccr_search_last_main_split)
THR_PHASES_VERSION = 106   # ... and the threshold kernel's 64-phase form with its getter (ccr_search_last_threshold_phases)
OPTIM_VERSION = 107   # ... and the multi-tensor AdamW step that keeps the encoder's 16-bit weights current (ccr_adamw_step)
ENCODER_PACKED_TRAIN_VERSION = 108   # ... and the embedding block's and the packed pooling's backward (ccr_embed_layernorm_bwd_half and its kin)
HALF_INDEX_VERSION = 109   # ... and the pack, index and search on either 16-bit element type (ccr_index_create_half and its kin)
AMP_OPTIM_VERSION = 110   # ... and loss scaling, overflow skip and norm clipping inside the AdamW step (ccr_adamw_step_scaled and its kin)
RANK_F32_VERSION = 111   # ... and the kept fp32 rows with the verified re-score of a 16-bit search on them (ccr_keep_f32, ccr_rescore_f32)
ATTENTION_BIAS_VERSION = 112   # ... and the attention forward with a shared relative position bias (ccr_attention_bias_half)
SIDE_CUS_VERSION = 113   # ... and the main pass that leaves CUs to the caller's side work (CCR_SIDE_CUS; main_grid and side_cus in the search statistics: an older library leaves them 0)
HEAD32_VERSION = 114   # ... and the attention forward with the head width as an argument, 32 or 64 (ccr_attention_head_half), with the inference LayerNorm rows at every multiple of 128

SHARD_HEADER_BYTES = 32
SHARD_MAGIC = 0x4D524343


class ShardHeader(ctypes.Structure):
    """ccr_shard_header (include/ccr_retrieval.h)."""
    _fields_ = [("magic", ctypes.c_uint32), ("n_flagged", ctypes.c_uint32), ("k_valid", ctypes.c_uint32),
                ("n_covered", ctypes.c_uint32), ("row_offset", ctypes.c_int64), ("n_rows", ctypes.c_int64)]


class SearchStats(ctypes.Structure):
    _fields_ = [("path", ctypes.c_int32), ("n_fallback", ctypes.c_int32), ("sample_tiles", ctypes.c_int32),
                ("ranges", ctypes.c_int32), ("cap", ctypes.c_int32), ("sublists", ctypes.c_int32),
                ("n_candidates", ctypes.c_int64), ("ms_sample", ctypes.c_float), ("ms_threshold", ctypes.c_float),
                ("ms_main", ctypes.c_float), ("ms_select", ctypes.c_float), ("ms_fallback", ctypes.c_float),
                ("ms_total", ctypes.c_float), ("n_retried", ctypes.c_int32), ("n_dense", ctypes.c_int32),
                ("main_launches", ctypes.c_int32), ("opt_rank", ctypes.c_int32), ("main_tile_queries", ctypes.c_int32),
                ("skipped_tiles", ctypes.c_int32), ("tile_cap", ctypes.c_int32), ("main_grid", ctypes.c_int32), ("side_cus", ctypes.c_int32)]


class AdamwSegment(ctypes.Structure):
    """ccr_adamw_segment (include/ccr_retrieval.h)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("shadow", ctypes.c_void_p), ("n", ctypes.c_int64), ("decay", ctypes.c_float), ("step_size", ctypes.c_float),
                ("bc2_sqrt", ctypes.c_float), ("shadow_dtype", ctypes.c_int32)]


class AdamwControl(ctypes.Structure):
    """ccr_adamw_control (include/ccr_retrieval.h): 64 bytes of device memory; CONTROL_WORDS names its 4-byte words."""
    _fields_ = [("coef", ctypes.c_float), ("skip", ctypes.c_int32), ("norm", ctypes.c_float), ("scale", ctypes.c_float),
                ("growth_tracker", ctypes.c_int32), ("skipped_total", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 10)]


CONTROL_WORDS = {name: i for i, (name, _) in enumerate(AdamwControl._fields_[:6])}


class CcrError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen the in-tree library and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise CcrError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"(or make -C crowd-coachable-recommendations_amd/csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    lib.ccr_version.restype = ctypes.c_int
    have = int(lib.ccr_version())
    if have < MIN_VERSION:   # a stale build would fail later, at the first missing symbol or with another argument list
        raise CcrError(f"{LIB_PATH} is version {have}, this binding needs {MIN_VERSION}: rebuild it "
                       f"(python -c 'import __graft_entry__ as g; g.build()')")
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:   # same version number, other entry points: a build from another tree
        raise CcrError(f"{LIB_PATH} lacks {', '.join(missing)}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    vp, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    lib.ccr_last_error.restype = ctypes.c_char_p
    lib.ccr_last_error.argtypes = []
    lib.ccr_version.restype = i32
    lib.ccr_pack_bf16.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    lib.ccr_pack_bf16_ex.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp]
    lib.ccr_index_create_with_norms.argtypes = [vp, i64, i32, i64, vp, vp, ctypes.POINTER(vp)]
    lib.ccr_meanpool_pack_bf16.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ccr_meanpool_pack_bf16_ex.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ccr_index_create.argtypes = [vp, i64, i32, i64, vp, ctypes.POINTER(vp)]
    lib.ccr_index_destroy.argtypes = [vp]
    lib.ccr_index_rows.argtypes = [vp]
    lib.ccr_index_rows.restype = i64
    lib.ccr_index_dim.argtypes = [vp]
    lib.ccr_search_workspace_bytes.argtypes = [vp, i32, i32]
    lib.ccr_search_workspace_bytes.restype = sz
    lib.ccr_search.argtypes = [vp, vp, i32, i32, vp, vp, vp, sz, i32, vp]
    lib.ccr_search_last_stats.argtypes = [vp, ctypes.POINTER(SearchStats)]
    lib.ccr_merge_topk.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.ccr_merge_topk_strided.argtypes = [vp, vp, i64, i64, i32, i32, i32, vp, vp, vp]
    lib.ccr_apply_block.argtypes = [vp, vp, i32, i32, vp, vp, i64, vp, vp, i32, vp]
    lib.ccr_inbatch_ce_workspace_bytes.argtypes = [i32, i32]
    lib.ccr_inbatch_ce_workspace_bytes.restype = sz
    lib.ccr_inbatch_ce_fwd.argtypes = [vp, vp, vp, i32, i32, f32, vp, vp, vp, sz, vp]
    lib.ccr_inbatch_ce_bwd.argtypes = [vp, vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp, sz, vp]
    lib.ccr_inbatch_ce_bwd_dev.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp, sz, vp]
    lib.ccr_inbatch_pack3_bf16.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.ccr_inbatch_ce_fwd_f32.argtypes = [vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, sz, vp]
    lib.ccr_pool_ce_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ccr_pool_ce_workspace_bytes.restype = sz
    lib.ccr_pool_ce_fwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, sz, vp]
    lib.ccr_pool_ce_fwd_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]
    lib.ccr_pool_ce_bwd_dev.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, sz, vp]
    lib.ccr_bpr_sample.argtypes = [vp, i32, i32, i64, vp, vp, vp, f32, vp, vp, i32, vp, i32, vp, vp]
    lib.ccr_bpr_frozen_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ccr_bpr_frozen_workspace_bytes.restype = sz
    lib.ccr_bpr_frozen_fwd.argtypes = [vp, i64, i32, vp, vp, f32, vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]
    lib.ccr_bpr_frozen_bwd_dev.argtypes = [vp, i64, i32, vp, vp, f32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.ccr_rank_metrics.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.ccr_search_finish.argtypes = [vp]
    lib.ccr_search_stream_wait_main_pass.argtypes = [vp, vp]
    lib.ccr_search_last_main_split.argtypes = [vp]
    lib.ccr_search_last_threshold_phases.argtypes = [vp]
    lib.ccr_scores.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.ccr_search_blocked_workspace_bytes.argtypes = [vp, i32, i32, vp]
    lib.ccr_search_blocked_workspace_bytes.restype = sz
    lib.ccr_search_blocked.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, i32, vp]
    lib.ccr_search_sparse_prior_workspace_bytes.argtypes = [vp, i32, i32, vp]
    lib.ccr_search_sparse_prior_workspace_bytes.restype = sz
    lib.ccr_search_sparse_prior.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, sz, i32, vp]
    lib.ccr_colsum_bf16.argtypes = [vp, i64, i32, vp, vp]
    lib.ccr_meanpool_bwd.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.ccr_bm25_index_create.argtypes = [vp, vp, vp, vp, i64, i64, ctypes.c_double, ctypes.POINTER(vp)]
    lib.ccr_bm25_index_destroy.argtypes = [vp]
    lib.ccr_bm25_search_workspace_bytes.argtypes = [vp, i32, i32]
    lib.ccr_bm25_search_workspace_bytes.restype = sz
    lib.ccr_bm25_search_workspace_bytes_k.argtypes = [vp, i32, i32, i32]
    lib.ccr_bm25_search_workspace_bytes_k.restype = sz
    lib.ccr_bm25_search_last_stats.argtypes = [vp, vp]
    lib.ccr_bm25_index_set_idf.argtypes = [vp, vp, vp, vp]
    lib.ccr_bm25_search.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]
    lib.ccr_pack_bf16_padded.argtypes = [vp, i64, i32, vp, i32, vp, vp, i32, vp]
    lib.ccr_attention_bf16.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_float, vp]
    lib.ccr_add_layernorm.argtypes = [vp, vp, vp, vp, ctypes.c_float, vp, vp, i64, i32, vp]
    lib.ccr_embed_layernorm.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, i64, i32, vp]
    lib.ccr_gelu_bf16.argtypes = [vp, vp, i64, vp]
    lib.ccr_attention_half.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    lib.ccr_attention_bias_half.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    lib.ccr_attention_head_half.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    lib.ccr_add_layernorm_half.argtypes = [vp, vp, vp, vp, ctypes.c_float, vp, vp, i64, i32, i32, vp]
    lib.ccr_embed_layernorm_half.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, i64, i32, i32, vp]
    lib.ccr_gelu_half.argtypes = [vp, vp, i64, i32, vp]
    lib.ccr_attention_fwd_train_half.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, vp]
    lib.ccr_attention_bwd_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ccr_attention_bwd_workspace_bytes.restype = sz
    lib.ccr_attention_bwd_half.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, ctypes.c_float, i32, vp, sz, vp]
    lib.ccr_add_layernorm_bwd_half.argtypes = [vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, i64, i32, i32, vp, sz, vp]
    lib.ccr_gelu_bwd_half.argtypes = [vp, vp, vp, i64, i32, vp]
    u64, u32, f64 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
    lib.ccr_dropout_bits_rows.argtypes = [vp, i64, i32, u64, u32, f64, vp]
    lib.ccr_dropout_bits_attention.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, u64, u32, f64, vp]
    lib.ccr_dropout_apply.argtypes = [vp, vp, f32, vp, vp, i64, i32, i32, vp]
    lib.ccr_attention_fwd_train_drop_half.argtypes = [vp, vp, vp, vp, vp, vp, f32, i32, i32, i32, i32, f32, i32, vp]
    lib.ccr_attention_bwd_drop_half.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, i32, i32, i32, i32, f32, i32, vp, sz, vp]
    lib.ccr_add_layernorm_drop_half.argtypes = [vp, vp, f32, vp, vp, vp, f32, vp, vp, i64, i32, i32, vp]
    lib.ccr_add_layernorm_bwd_drop_half.argtypes = [vp, vp, f32, vp, vp, f32, vp, vp, vp, vp, vp, i64, i32, i32, vp, sz, vp]
    lib.ccr_adamw_step.argtypes = [vp, i32, f32, f32, f32, f32, vp]
    lib.ccr_grad_stats_workspace_bytes.argtypes = [vp, i32]
    lib.ccr_grad_stats_workspace_bytes.restype = i64
    lib.ccr_grad_stats.argtypes = [vp, i32, vp, vp]
    lib.ccr_adamw_control_update.argtypes = [vp, vp, i64, f32, i32, ctypes.c_double, ctypes.c_double, i32, vp, vp, vp]
    lib.ccr_adamw_step_scaled.argtypes = [vp, i32, f32, f32, f32, f32, vp, vp]
    lib.ccr_embed_layernorm_train_half.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, f32, vp, f32, vp, vp, i64, i32, i32, vp]
    lib.ccr_embed_layernorm_bwd_half.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, f32, vp, f32, vp, vp, vp, vp, i64, i32, vp, sz, vp]
    lib.ccr_embedding_grad.argtypes = [vp, vp, vp, i64, i32, vp, i64, vp]
    lib.ccr_meanpool_bwd_packed.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.ccr_meanpool_pack_bf16_packed.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.ccr_pack_half_ex.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp]
    lib.ccr_pack_half_padded.argtypes = [vp, i64, i32, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.ccr_meanpool_pack_half_ex.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.ccr_meanpool_pack_half_packed.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    lib.ccr_index_create_half.argtypes = [vp, i64, i32, i32, i64, vp, ctypes.POINTER(vp)]
    lib.ccr_index_create_with_norms_half.argtypes = [vp, i64, i32, i32, i64, vp, vp, ctypes.POINTER(vp)]
    lib.ccr_index_dtype.argtypes = [vp]
    lib.ccr_colsum_half.argtypes = [vp, i64, i32, i32, vp, vp]
    lib.ccr_keep_f32.argtypes = [vp, vp, i32, i32, vp, vp, i64, i32, vp]
    lib.ccr_rescore_f32_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.ccr_rescore_f32_workspace_bytes.restype = sz
    lib.ccr_rescore_f32.argtypes = [vp, vp, i64, i32, vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.ccr_shard_message_bytes.argtypes = [i32, i32]
    lib.ccr_shard_message_bytes.restype = sz
    lib.ccr_search_shard.argtypes = [vp, vp, i32, i32, vp, vp, sz, i32, vp]
    lib.ccr_shard_message_fill.argtypes = [vp, i32, i32, i32, vp, vp, i64, i64, vp]
    lib.ccr_merge_shard_messages.argtypes = [vp, i64, i32, i32, i32, vp, vp, vp]
    lib.ccr_merge_short_lists.argtypes = [vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is ctypes.c_int and name not in ("ccr_version", "ccr_index_dim", "ccr_index_dtype"):
            fn.restype = i32
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != CCR_OK:
        msg = load().ccr_last_error().decode("utf-8", "replace")
        if rc == CCR_ERR_BLOCK_ID:
            raise AssertionError("block id not found")
        raise CcrError(f"{what} failed ({rc}): {msg}")
