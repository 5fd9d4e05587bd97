"""ccrec_amd/index_ref.py -- the CPU definition an fp16 (or bf16) index is checked against: its pack equals torch's conversion bit for
bit on the edge table, its bf16 search equals the oracle's, the CCREC_INDEX_DTYPE switch parses, and the claim the fp16 index rests
on holds: rounding embeddings to fp16 keeps more of the fp32 ranking than rounding them to bf16."""
import os

import numpy as np
import pytest
import torch

from ccrec_amd import index_ref
from oracle import oracle as orc

TORCH = {"fp16": torch.float16, "bf16": torch.bfloat16}


def edge_table():
    """fp32 values at every edge of the two 16-bit formats: signed zeros, fp16 subnormals (the smallest, 2^-24, and the tie 2^-25 below
    it, which rounds to even = 0), the largest fp16 value, the largest value that still rounds to it, the first that rounds to inf,
    NaN and the infinities -- and the same with the other sign."""
    pos = [0.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1.0, 1.0 + 2.0 ** -11,
           1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, 65504.0, 65519.996, 65520.0, 1e5, 3.0e38, 3.4e38]
    vals = np.array(pos + [-v for v in pos] + [np.nan, np.inf, -np.inf], np.float32)
    assert vals[13] < np.float32(65520.0) and vals[13] > np.float32(65519.99)
    return vals


def torch_bits(x, name):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TORCH[name]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_pack_equals_torch_on_the_edge_table_and_on_gaussians(name):
    x = edge_table()
    got, want = index_ref.pack(x, name), torch_bits(x, name)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan]), [(float(v), hex(a), hex(b)) for v, a, b in zip(x[~nan], got[~nan], want[~nan]) if a != b]
    assert np.all(np.isnan(index_ref.unpack(got[nan], name)))
    if name == "fp16":
        by_value = dict(zip(x.tolist()[:18], got.tolist()[:18]))
        assert by_value[2.0 ** -24] == 0x0001 and by_value[2.0 ** -25] == 0x0000 and by_value[1.5 * 2.0 ** -25] == 0x0001
        assert by_value[65504.0] == 0x7BFF and got[13] == 0x7BFF and by_value[65520.0] == 0x7C00
        assert index_ref.overflow_count(x) == 2 * 4          # 65 520, 1e5, 3.0e38, 3.4e38 and their negatives; not inf, not NaN
    g = (np.random.RandomState(3).randn(500, 96) * np.float32(96 ** -0.5)).astype(np.float32)
    assert np.array_equal(index_ref.pack(g, name), torch_bits(g, name))
    assert np.array_equal(index_ref.unpack(index_ref.pack(g, name), name), torch.from_numpy(g).to(TORCH[name]).float().numpy())


def test_bf16_search_equals_the_oracle_with_engineered_ties():
    rs = np.random.RandomState(11)
    n, d, nq, k = 300, 64, 9, 40
    D = rs.randint(-4, 5, size=(n, d)).astype(np.float32) / 4        # exact arithmetic: equal rows score equal
    D[50:90] = D[7]                                                   # 41 identical rows
    D[200:230, :32] = D[3, :32]
    Q = rs.randint(-4, 5, size=(nq, d)).astype(np.float32) / 4
    Q[0] = D[7]
    Q[1] = 0.0                                                        # every score equal: the order is the row order
    Db, Qb = index_ref.pack(D, "bf16"), index_ref.pack(Q, "bf16")
    assert np.array_equal(Db, orc.pack_bf16(D)) and np.array_equal(Qb, orc.pack_bf16(Q))
    assert np.array_equal(index_ref.canonical_scores(Qb, Db, "bf16").view(np.uint32), orc.canonical_scores(Qb, Db).view(np.uint32))
    for block in (None, [[], [0, 1, 299], list(range(45, 95))] + [[7]] * (nq - 3)):
        i0, s0 = orc.canonical_search(Qb, Db, k, block)
        i1, s1 = index_ref.canonical_search(Qb, Db, "bf16", k, block)
        assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert np.array_equal(index_ref.canonical_search(Qb, Db, "bf16", k)[0][1], np.arange(k))
    # the normalising pack and the norms, on rows of a width that is no multiple of 4 as well
    for width in (64, 41):
        X = (rs.randn(37, width) * 3).astype(np.float32)
        assert np.array_equal(index_ref.normalize_pack(X, "bf16"), orc.normalize_pack_bf16(X))
        assert np.array_equal(index_ref.row_norms(X).view(np.uint32), orc.row_norms(X).view(np.uint32))
    # the sparse prior form
    indptr = np.array([0, 0, 3] + [3] * (nq - 2), np.int64)
    idx, val = np.array([5, 60, 250], np.int64), np.array([0.5, -2.0, 1e-3])
    i0, s0 = orc.sparse_prior_search(Qb, Db, indptr, idx, val, k)
    i1, s1 = index_ref.sparse_prior_search(Qb, Db, "bf16", indptr, idx, val, k)
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64))
    with pytest.raises(AssertionError, match="block id not found"):
        index_ref.rank(np.zeros((1, 4), np.float32), 2, [[4]])


def test_index_dtype_switch_parses(monkeypatch):
    from ccrec_amd import ops
    monkeypatch.delenv("CCREC_INDEX_DTYPE", raising=False)
    assert ops.index_dtype() == torch.bfloat16                       # the default
    monkeypatch.setenv("CCREC_INDEX_DTYPE", "fp16")                   # read at call time
    assert ops.index_dtype() == torch.float16
    monkeypatch.setenv("CCREC_INDEX_DTYPE", "bf16")
    assert ops.index_dtype() == torch.bfloat16
    for bad in ("float16", "FP16", "", "fp32"):
        monkeypatch.setenv("CCREC_INDEX_DTYPE", bad)
        with pytest.raises(ValueError, match="CCREC_INDEX_DTYPE"):
            ops.index_dtype()
    # the overflow counter of a bf16 build holds nothing and never raises; the message of an fp16 one names both ways out
    ops.IndexOverflow(torch.bfloat16, "cpu").check()
    of = ops.IndexOverflow(torch.float16, "cpu")
    of.check()
    of.counter += 3
    with pytest.raises(OverflowError, match=r"3 embedding.*bf16.*CCREC_SIM_TYPE=cos"):
        of.check()
    with pytest.raises(ValueError):
        index_ref.pack(np.zeros(2, np.float32), "fp32")


def test_fp16_keeps_more_of_the_fp32_ranking_than_bf16():
    """Gaussian embeddings scaled by 1 / sqrt(768) (the benchmark's data: corpus seed 1234, query seed 4321), N = 20 000, Q = 16, top-100
    by fp64 scores of the fp32 rows against top-100 of the same rows rounded to each 16-bit type: the count of rank positions that hold
    the same row is strictly larger for fp16.  (1 518 against 1 143 of 1 600 when this was written.)"""
    n, nq, d, k = 20_000, 16, 768, 100
    D = (torch.randn(n, d, generator=torch.Generator().manual_seed(1234)) / d ** 0.5).numpy()
    Q = (torch.randn(nq, d, generator=torch.Generator().manual_seed(4321)) / d ** 0.5).numpy()

    def top(q, dd):
        s = q.astype(np.float64) @ dd.astype(np.float64).T
        return np.argsort(-s, axis=1, kind="stable")[:, :k]

    want = top(Q, D)
    same = {}
    for name in ("bf16", "fp16"):
        got = top(index_ref.unpack(index_ref.pack(Q, name), name), index_ref.unpack(index_ref.pack(D, name), name))
        same[name] = int((got == want).sum())
    print(same)
    assert same["fp16"] > same["bf16"], same
    assert same["fp16"] <= nq * k
