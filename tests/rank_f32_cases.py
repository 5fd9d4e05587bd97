"""Inputs shared by the fp32-ranking tests (tests/test_cpu_rank_f32_ref.py, tests/test_gpu_rank_f32.py)."""
import numpy as np

from ccrec_amd import index_ref


def near_duplicate_cluster():
    """(query [1, 64], corpus [600, 64]) fp32, seed 7.  v = a bf16-representable gaussian / sqrt(d); rows j < 100 are
    (float)(v (1 + (j + 1) 2^-17)): they differ below bf16's spacing, so the bf16 search returns them in corpus order while their
    fp32 scores rise with j; the other 500 rows are gaussian / sqrt(d) * 0.25, far below the cluster.  The query is v."""
    rs = np.random.RandomState(7)
    d, n = 64, 600
    v = index_ref.unpack(index_ref.pack((rs.randn(d) / np.sqrt(d)).astype(np.float32), "bf16"), "bf16")
    D = (rs.randn(n, d) / np.sqrt(d) * 0.25).astype(np.float32)
    j = np.arange(100)
    D[:100] = (v.astype(np.float64)[None, :] * (1.0 + (j[:, None] + 1) * 2.0 ** -17)).astype(np.float32)
    return v[None, :].copy(), D


def gaussian(n=20000, nq=16, d=768):
    """(queries [nq, d], corpus [n, d]) fp32 gaussian / sqrt(d): corpus seed 1234, query seed 4321 (the benchmark's data)."""
    D = (np.random.RandomState(1234).randn(n, d) / np.sqrt(d)).astype(np.float32)
    Q = (np.random.RandomState(4321).randn(nq, d) / np.sqrt(d)).astype(np.float32)
    return Q, D
