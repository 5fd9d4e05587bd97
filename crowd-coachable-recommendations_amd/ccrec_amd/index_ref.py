"""The pack and the search of an index restated on the CPU (numpy only, no GPU, no library) for either 16-bit element type: the
bit-exact definition that csrc/ccr_pack.hip and every search path obey.

    pack      fp32 -> bf16 / fp16 bits, round to nearest even (the bits of torch's .to(dtype); fp16 keeps subnormals and turns a finite
              value of magnitude >= 65 520 into +-inf -- count them with overflow_count)
    normalise y_i = pack((float)((double) x_i / max(sqrt(ss), 1e-12))), ss = the row's fp64 sum of squares in the library's order:
              64 lanes, lane l owns the elements of the 4-element chunks c with c % 64 == l in increasing index, then
              p[l] += p[l ^ off] for off = 32, 16, .., 1
    score     (float) sum over i ascending of (double) q_i * (double) d_i -- a loop over dim, each step ONE fp64 multiply-add over the
              whole [nq, nd] array (a product of two bf16 or two fp16 values is exact in fp64, so the step rounds once)
    rank      score descending, index ascending; blocked columns score -1e6 first (kept, not removed); with a sparse prior the
              final score is (double) score + prior, ranked the same way

For bf16 inputs every function here equals oracle/oracle.py's canonical_* bit for bit (tests/test_cpu_index_ref.py); the oracle knows
bf16 only, this module is what an fp16 index is checked against."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BF16, FP16 = "bf16", "fp16"


def _parallel(fn, items):
    """fn over independent pieces of the work on a few threads (numpy releases the GIL); the result does not depend on the split."""
    items = list(items)
    workers = min(8, os.cpu_count() or 1, len(items))
    if workers <= 1:
        return [fn(it) for it in items]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(fn, items))


def _kind(dtype):
    name = str(dtype).replace("torch.", "")
    if name in ("bf16", "bfloat16"):
        return BF16
    if name in ("fp16", "float16", "half"):
        return FP16
    raise ValueError(f"index_ref: dtype {dtype!r} (bf16 or fp16)")


def pack(x, dtype):
    """fp32 array -> uint16 bit patterns of `dtype`, round to nearest even.  A NaN stays a NaN (payload not specified)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if _kind(dtype) == FP16:
        with np.errstate(all="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def unpack(bits, dtype):
    """uint16 bit patterns of `dtype` -> their exact fp32 values."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if _kind(dtype) == FP16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def overflow_count(x):
    """Elements that are finite in fp32 and +-inf as fp16: what the fp16 pack adds to its overflow counter."""
    a = np.abs(np.asarray(x, dtype=np.float32))
    return int(np.count_nonzero((a >= np.float32(65520.0)) & np.isfinite(a)))


def row_sumsq(x):
    """[rows] fp64 sums of squares of fp32 rows of any width, in the library's order (module docstring)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, dim = x.shape
    p = np.zeros((rows, 64), np.float64)
    for i in range(dim):
        v = x[:, i].astype(np.float64)
        p[:, (i >> 2) & 63] += v * v
    lanes = np.arange(64)
    off = 32
    while off >= 1:
        p = p + p[:, lanes ^ off]
        off >>= 1
    return p[:, 0]


def row_norms(x):
    """[rows] fp32: the L2 norms the pack reports for fp32 rows (before normalisation)."""
    return np.sqrt(row_sumsq(x)).astype(np.float32)


def normalize_pack(x, dtype):
    """rows x / max(||x||, 1e-12) -> bits of `dtype` (the cos pack)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    den = np.maximum(np.sqrt(row_sumsq(x)), 1e-12)
    return pack((x.astype(np.float64) / den[:, None]).astype(np.float32), dtype)


def canonical_scores(q_bits, d_bits, dtype):
    """[nq, nd] fp32 canonical scores of two bit matrices of `dtype`."""
    q = unpack(q_bits, dtype).astype(np.float64)
    d = unpack(d_bits, dtype).astype(np.float64)
    assert q.ndim == d.ndim == 2 and q.shape[1] == d.shape[1]
    nq, nd = q.shape[0], d.shape[0]
    out = np.empty((nq, nd), np.float32)
    qt, dt = np.ascontiguousarray(q.T), np.ascontiguousarray(d.T)     # [dim, nq], [dim, nd]: a step reads two contiguous rows
    cols = max(64, (1 << 16) // max(nq, 1))                           # the array is walked in column blocks that stay in cache:
                                                                      # the same steps on the same elements, only sooner

    def block(lo):
        hi = min(nd, lo + cols)
        acc = np.zeros((nq, hi - lo), np.float64)
        prod = np.empty_like(acc)
        with np.errstate(all="ignore"):
            for i in range(q.shape[1]):
                np.multiply(qt[i][:, None], dt[i, lo:hi][None, :], out=prod)   # exact: the step rounds once, in the add
                acc += prod
            out[:, lo:hi] = acc

    _parallel(block, range(0, nd, cols))
    return out


def _order(scores):
    """Column order of one score row: score descending, index ascending (a stable sort keeps equal scores in index order)."""
    return np.argsort(-scores, kind="stable")


def rank(scores, k, block=None):
    """(ids [nq, k] int64, scores [nq, k]) of a score matrix by (score desc, index asc).  block: per query a list of blocked
    columns -- they score -1e6 and stay in the ranking.  AssertionError("block id not found") on a column outside the matrix."""
    scores = np.array(scores, copy=True)
    nq, nd = scores.shape
    assert 1 <= k <= nd
    ids = np.empty((nq, k), np.int64)
    out = np.empty((nq, k), scores.dtype)
    if block is not None:
        for r in range(nq):
            if len(block[r]):
                b = np.asarray(block[r], np.int64)
                assert b.min() >= 0 and b.max() < nd, "block id not found"
                scores[r, b] = -1e6

    def one(r):
        o = _order(scores[r])[:k]
        ids[r], out[r] = o, scores[r][o]

    _parallel(one, range(nq))
    return ids, out


def canonical_search(q_bits, d_bits, dtype, k, block=None):
    """Exhaustive canonical top-k: (ids [nq, k] int64, scores [nq, k] fp32)."""
    return rank(canonical_scores(q_bits, d_bits, dtype), k, block)


def sparse_prior_search(q_bits, d_bits, dtype, indptr, indices, data, k):
    """Top-k of (canonical score + sparse prior): final = (double) score + prior in fp64, order (final desc, column asc).
    CSR prior (indptr [nq + 1], indices, data).  -> (ids [nq, k] int64, finals [nq, k] float64)."""
    final = canonical_scores(q_bits, d_bits, dtype).astype(np.float64)
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.float64)
    for r in range(final.shape[0]):
        sl = slice(indptr[r], indptr[r + 1])
        np.add.at(final[r], indices[sl], data[sl])
    return rank(final + 0.0, k)
