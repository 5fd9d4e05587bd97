"""The packed fine-tune step (library version 108) without a GPU: embed_grad_ref, the numpy restatement of ccr_embedding_grad's normative
summation order; the four new entry points in the header, the binding and the built library; MultipleNrlStep(one_pass=True)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

PACKED_EXPORTS = ["ccr_embed_layernorm_train_half", "ccr_embed_layernorm_bwd_half", "ccr_embedding_grad", "ccr_meanpool_bwd_packed"]


def order_case():
    """A run of 130 entries (two full chunks of 64 and one of 2) in four columns of 1e8, 1 and -1e8, whose fp32 sum depends on where the
    chunks are cut and on the order of the additions (fp32 spacing at 1e8 is 8: a 1 added to +-1e8 is lost, 63 added to 1e8 rounds to
    +64).  -> (rows [130, 4] float32, the sum under the normative rule, worked out by hand below)."""
    big = np.float32(1e8)
    k = np.arange(130)
    x = np.ones((130, 4), dtype=np.float32)
    x[:, 0] = np.array([1e8, 1, -1e8], dtype=np.float32)[k % 3]
    x[0, 1], x[128, 1] = big, -big
    x[64, 2], x[128, 2] = big, -big
    x[63, 3], x[64, 3] = big, -big
    # column 0: 1e8, 1, -1e8, 1e8, ..: every triple returns to 0 (the 1 is lost in 1e8 + 1).  Chunk 0 = 21 triples + 1e8 = 1e8; chunk 1
    #           starts at a 1: 1 - 1e8 = -1e8 (rounded), + 1e8 = 0, + 1 = 1, 21 times over = 1; chunk 2 = -1e8 + 1e8 = 0.
    #           (1e8 + 1) + 0 = 1e8.
    # column 1: chunk 0 = 1e8 + 63 ones, each lost = 1e8; chunk 1 = 64 ones = 64; chunk 2 = -1e8 + 1 = -1e8.  (1e8 + 64) - 1e8 = 64
    #           (a plain sequential sum loses all 127 ones before -1e8 and gives 1).
    # column 2: chunk 0 = 64; chunk 1 = 1e8 + 63 ones = 1e8; chunk 2 = -1e8.  (64 + 1e8) - 1e8 = 64 (back to front it is 2).
    # column 3: chunk 0 = 63 ones + 1e8 = 100000063 -> 100000064; chunk 1 = -1e8 + 63 ones = -1e8; chunk 2 = 2.
    #           (100000064 - 1e8) + 2 = 66 (chunks of 63 give 128, of 65 give 129).
    return x, np.array([1e8, 64, 64, 66], dtype=np.float32)


def test_the_restatement_matches_an_fp64_index_add_within_fp32_summation_error():
    """Random ids with runs from 0 to several chunks: |ref - fp64| <= (n - 1) * 2^-24 * sum |terms| per element, the first-order bound of any
    fp32 summation order over n terms (Higham 4.4: gamma_(n-1)), here with n the run length."""
    from ccrec_amd import embed_grad_ref
    rng = np.random.default_rng(0)
    T, dim, n_rows = 3000, 24, 40
    idx = np.where(rng.random(T) < 0.5, 3, rng.integers(0, n_rows, T))      # id 3 holds half the rows: a run of ~24 chunks
    idx[idx == 7] = 8                                                       # id 7 does not occur
    d_x = rng.standard_normal((T, dim)).astype(np.float32)
    got = embed_grad_ref.embedding_grad(idx, d_x, n_rows)
    assert got.dtype == np.float32 and got.shape == (n_rows, dim)
    ref = np.zeros((n_rows, dim))
    mag = np.zeros((n_rows, dim))
    np.add.at(ref, idx, d_x.astype(np.float64))
    np.add.at(mag, idx, np.abs(d_x).astype(np.float64))
    count = np.bincount(idx, minlength=n_rows)[:, None]
    bound = np.maximum(count - 1, 0) * 2.0 ** -24 * mag * 1.01 + np.abs(ref) * 2.0 ** -24      # + the final rounding of the comparison
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert (got[7] == 0).all() and not np.signbit(got[7]).any()             # an absent id: +0
    # ids outside the table land on the clamped row
    far = embed_grad_ref.embedding_grad(np.array([-5, 99, 1]), d_x[:3], 3)
    assert np.array_equal(far, np.stack([d_x[0], d_x[2], d_x[1]]))


def test_the_order_case_has_the_bits_worked_out_by_hand():
    from ccrec_amd import embed_grad_ref
    x, want = order_case()
    got = embed_grad_ref.run_sum(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # the same through the table interface, the run scattered between rows of other ids
    idx = np.full(200, 9)
    rows = np.sort(np.random.default_rng(1).choice(200, 130, replace=False))
    idx[rows] = 2
    d_x = np.full((200, 4), 0.5, dtype=np.float32)
    d_x[rows] = x
    grad = embed_grad_ref.embedding_grad(idx, d_x, 12)
    assert np.array_equal(grad[2].view(np.uint32), want.view(np.uint32)) and (grad[9] == 35.0).all()
    # every other cut or order this case was built against gives other bits somewhere
    others = {f"chunks of {c}": embed_grad_ref.run_sum(x, c) for c in (1, 2, 32, 63, 65, 128, 130)}
    others["back to front"] = embed_grad_ref.run_sum(x[::-1])
    others["numpy pairwise"] = x.sum(0)
    others["fp64 rounded once"] = x.astype(np.float64).sum(0).astype(np.float32)
    for name, other in others.items():
        assert not np.array_equal(other.view(np.uint32), want.view(np.uint32)), name
    assert embed_grad_ref.CHUNK == 64
    assert np.array_equal(embed_grad_ref.order([5, 0, 5, -3, 0], 4), [1, 3, 4, 0, 2])


def test_the_four_entry_points_are_declared_bound_and_exported():
    from ccrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    lib = _lib.load()
    for name in PACKED_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name      # one ctypes type per C parameter
        assert re.search(name + r" \((?:bbpr\.py:195-197|item_tower\.py:141-146)", header), name   # each cites the reference lines it serves
    assert re.search(r"^#define CCR_EMBED_GRAD_CHUNK 64$", header, flags=re.M)
    assert lib.ccr_version() >= _lib.ENCODER_PACKED_TRAIN_VERSION == 108 and _lib.MIN_VERSION == 101


def test_null_pointers_and_bad_shapes_are_refused_before_any_device_call():
    """(No device here: an entry point that got past its argument checks would fail differently or crash.)"""
    from ccrec_amd import _lib
    lib = _lib.load()
    assert lib.ccr_embedding_grad(None, None, None, 4, 256, None, 8, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_meanpool_bwd_packed(None, None, None, None, _lib.DTYPE_F32, 2, 256, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_embed_layernorm_bwd_half(None, 1, None, 1, None, 1, None, None, None, None, 1e-12, None, 1.0, None, None, None, None, 4, 256,
                                            None, 0, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_embed_layernorm_train_half(None, 1, None, 1, None, 1, None, None, None, None, None, 1e-12, None, 1.0, None, None, 4, 256,
                                              _lib.DTYPE_BF16, None) == _lib.CCR_ERR_INVALID
    assert b"null pointer" in lib.ccr_last_error()


def _table_step(one_pass, table, calls):
    from ccrec_amd.bbpr_loss import MultipleNrlStep

    def forward(ptr):
        calls.append(int(torch.as_tensor(ptr).numel()))
        return table[torch.as_tensor(ptr)]

    return MultipleNrlStep(forward, torch.tensor([0, 1, 2, 3]), torch.arange(12), {0: [8, 9], 1: [9, 10], 2: [10, 11], 3: [11, 8]},
                           n_negatives=2, one_pass=one_pass)


def test_one_pass_gives_the_three_pass_loss_and_gradients_bit_for_bit_over_a_table_lookup(monkeypatch):
    """forward = a pure table lookup: nothing depends on the row count of a call, so the split rows are the three calls' rows and the loss
    and the table's gradient agree bit for bit.  The loss itself runs on a kernel (ops.pool_ce): stood in for by torch here, the same
    stand-in for both steps."""
    from ccrec_amd import bbpr_loss, ops
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")

    def pool_ce(q, c, labels, inv_temperature, weights=None):
        return torch.nn.functional.cross_entropy(q @ c.T * inv_temperature, labels.long())

    monkeypatch.setattr(ops, "pool_ce", pool_ce)
    batch = torch.tensor([[0, 4, 1.0], [1, 5, 1.0], [2, 6, 1.0], [3, 7, 1.0]])
    results = []
    for one_pass in (False, True):
        table = torch.randn(12, 16, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
        calls = []
        loss = _table_step(one_pass, table, calls)(batch)
        loss.backward()
        results.append((loss.detach(), table.grad.clone(), calls))
    (l3, g3, c3), (l1, g1, c1) = results
    assert c3 == [4, 4, 8] and c1 == [16]                                   # one_pass calls forward exactly once, on all 16 pointers
    assert torch.equal(l3.view(torch.int32), l1.view(torch.int32)) and torch.equal(g3.view(torch.int32), g1.view(torch.int32))
    assert g1.abs().sum() > 0


def test_one_pass_is_off_by_default_and_reaches_bert_mt_step():
    from ccrec_amd.bbpr_loss import BertMTStep, MultipleNrlStep
    args = (lambda ptr: None, torch.arange(3), torch.arange(3), {})
    assert MultipleNrlStep(*args).one_pass is False and BertMTStep(*args).one_pass is False
    assert BertMTStep(*args, one_pass=True).one_pass is True
