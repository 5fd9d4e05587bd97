"""The ranking on the fp32 embeddings restated on the CPU (numpy only, no GPU, no library): the bit-exact definition that
csrc/ccr_rank_f32.hip and ops.ExactF32Index obey.  It extends index_ref, whose pack / unpack / row_sumsq / rank it uses.

    kept row    y = x zero-padded to padded_dim(dim); with normalize y_i = (float)((double) x_i / max(sqrt(ss), 1e-12)), ss =
                index_ref.row_sumsq(x): the value the pack rounds, so index_ref.pack(y, dtype) IS the packed row h
    score       s32(q, j) = (float) sum over i ascending of fma((double) y_q[i], (double) y_j[i], acc): index_ref's rule with fp32
                operands (a product of two fp32 values is exact in fp64, so each step rounds once)
    rank        s32 descending, row index ascending; a blocked row scores -1e6 and stays in the ranking
    residual    res_bounds[j] >= ||y_j - unpack(h_j)||_2: the fp64 norm, times (1 + 2^-20), rounded UP to fp32
    verified    of one query, given its first n_cand rows by the 16-bit search (cand_s16 in that search's rank order), k <= n_cand:
                tau = the k-th s32 among the candidates, cut = cand_s16[n_cand - 1], A >= ||y_q||_2, r = the query's own residual bound,
                Rmax / Nmax = the maxima of the corpus's res_bounds / norm_bounds, all in fp64:
                    E = A Rmax + r Nmax,   slack = 2^-21 (|cut| + |tau|) + 2^-40 A (Nmax + Rmax)
                    verified <=> n_cand == n_rows  or  cut == -1e6f  or  cut + E + slack < tau
                (the second case: a blocked row was fetched, so every unblocked row was)
    search      exact_search(): the rungs n1 = min(n_rows, max_candidates, 2 k + 32), doubled for the queries still unverified up to
                min(n_rows, max_candidates); then the dense path: the rows whose s16 + A res_bounds[j] + r norm_bounds[j] + slack_j
                reaches the last rung's tau are re-scored, and the k best of them are the result
"""
import numpy as np

from . import index_ref

BLOCKED = np.float32(-1e6)
MAX_K = 4096


def padded_dim(dim):
    return (int(dim) + 7) // 8 * 8


def round_up_f32(v):
    """fp64 array (>= 0) -> the smallest fp32 values that are not below it."""
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def kept_rows(x, normalize=False):
    """fp32 [rows, dim] -> the kept rows y, fp32 [rows, padded_dim(dim)] (module docstring)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, dim = x.shape
    y = np.zeros((rows, padded_dim(dim)), np.float32)
    if normalize:
        den = np.maximum(np.sqrt(index_ref.row_sumsq(x)), 1e-12)
        y[:, :dim] = (x.astype(np.float64) / den[:, None]).astype(np.float32)
    else:
        y[:, :dim] = x
    return y


def scores(yq, yd):
    """[nq, nd] fp32 canonical scores s32 of kept rows."""
    q = np.ascontiguousarray(yq, dtype=np.float32).astype(np.float64)
    d = np.ascontiguousarray(yd, dtype=np.float32).astype(np.float64)
    assert q.ndim == d.ndim == 2 and q.shape[1] == d.shape[1]
    nq, nd = q.shape[0], d.shape[0]
    out = np.empty((nq, nd), np.float32)
    qt, dt = np.ascontiguousarray(q.T), np.ascontiguousarray(d.T)
    cols = max(64, (1 << 16) // max(nq, 1))   # column blocks that stay in cache: the same steps on the same elements

    def block(lo):
        hi = min(nd, lo + cols)
        acc = np.zeros((nq, hi - lo), np.float64)
        prod = np.empty_like(acc)
        with np.errstate(all="ignore"):
            for i in range(q.shape[1]):
                np.multiply(qt[i][:, None], dt[i, lo:hi][None, :], out=prod)   # exact: the step rounds once, in the add
                acc += prod
            out[:, lo:hi] = acc

    index_ref._parallel(block, range(0, nd, cols))
    return out


def ranking(yq, yd, k, block=None):
    """The exhaustive fp32 ranking: (ids [nq, k] int64, scores [nq, k] fp32)."""
    return index_ref.rank(scores(yq, yd), k, block)


def residual_norms(y, h_bits, dtype):
    """[rows] fp64: ||y_j - unpack(h_j)||_2 (numpy's summation; the bounds below cover any order)."""
    with np.errstate(all="ignore"):
        diff = np.asarray(y, np.float32).astype(np.float64) - index_ref.unpack(h_bits, dtype).astype(np.float64)
        return np.sqrt(np.sum(diff * diff, axis=1))


def res_bounds(y, h_bits, dtype):
    """[rows] fp32 >= the residual norms: times (1 + 2^-20), rounded up."""
    return round_up_f32(residual_norms(y, h_bits, dtype) * (1.0 + 2.0 ** -20))


def norm_bounds(h_bits, dtype):
    """[rows] fp32 >= ||unpack(h_j)||_2, formed like res_bounds (the library's pack kernels write looser ones)."""
    h = index_ref.unpack(h_bits, dtype).astype(np.float64)
    return round_up_f32(np.sqrt(np.sum(h * h, axis=1)) * (1.0 + 2.0 ** -20))


def query_norm_bounds(nb, r):
    """A >= ||y_q||_2 from nb >= ||h_q||_2 and r >= ||y_q - h_q||_2 (triangle inequality): the fp32 sum, one step up."""
    s = np.asarray(nb, np.float32) + np.asarray(r, np.float32)
    return np.nextafter(s, np.float32(np.inf)).astype(np.float32)


def error_bound(A, r, Rmax, Nmax):
    """E = A Rmax + r Nmax in fp64 (both products of two fp32 values are exact)."""
    return np.float64(A) * np.float64(Rmax) + np.float64(r) * np.float64(Nmax)


def slack(a, tau, A, Rmax, Nmax):
    """2^-21 (|a| + |tau|) + 2^-40 A (Nmax + Rmax) in fp64, every step rounded on its own (a: cut, or a row's 16-bit score)."""
    first = 2.0 ** -21 * (np.abs(np.float64(a)) + np.abs(np.float64(tau)))
    second = 2.0 ** -40 * (np.float64(A) * (np.float64(Nmax) + np.float64(Rmax)))
    return first + second


def verified(n_cand, n_rows, cut, tau, A, r, Rmax, Nmax):
    """The verification rule of one query (module docstring)."""
    if n_cand == n_rows or np.float32(cut) == BLOCKED:
        return True
    return bool((np.float64(np.float32(cut)) + error_bound(A, r, Rmax, Nmax)) + slack(np.float32(cut), np.float32(tau), A, Rmax, Nmax)
                < np.float64(np.float32(tau)))


def candidate_scores(yq, yd_t, rows):
    """s32 of every query with ITS OWN candidate rows: yq [nq, pdim], yd_t [pdim, n_rows] (the kept corpus rows, transposed and
    contiguous), rows [nq, n_cand] -> [nq, n_cand] fp32.  The rule of scores(): one fp64 multiply-add per element, ascending."""
    q = np.asarray(yq, np.float32).astype(np.float64)
    acc = np.zeros(rows.shape, np.float64)
    with np.errstate(all="ignore"):
        for i in range(q.shape[1]):
            acc += q[:, i:i + 1] * yd_t[i][rows]            # fp64 x fp32: exact product, the add rounds once
        return acc.astype(np.float32)


def rescore(yq, yd, cand_ids, cand_s16, k, A, r, Rmax, Nmax, id_offset=0, yd_t=None):
    """What ccr_rescore_f32 writes: yq [nq, pdim], yd [n_rows, pdim] kept rows, cand_ids [nq, n_cand] global ids, cand_s16 their
    16-bit scores in rank order -> (scores [nq, k] fp32, ids [nq, k] int64, flags [nq] int32: 0 verified, 1 not).
    yd_t: np.ascontiguousarray(yd.T), for callers that re-score against one corpus many times."""
    yq, yd = np.asarray(yq, np.float32), np.asarray(yd, np.float32)
    cand_ids, cand_s16 = np.asarray(cand_ids, np.int64), np.asarray(cand_s16, np.float32)
    nq, n_cand = cand_ids.shape
    assert 1 <= k <= n_cand <= yd.shape[0]
    rows = cand_ids - id_offset
    s = candidate_scores(yq, np.ascontiguousarray(yd.T) if yd_t is None else yd_t, rows)
    s[cand_s16 == BLOCKED] = BLOCKED
    out_s = np.empty((nq, k), np.float32)
    out_i = np.empty((nq, k), np.int64)
    flags = np.empty(nq, np.int32)
    for q in range(nq):
        order = np.lexsort((rows[q], -s[q].astype(np.float64)))[:k]     # score descending, row ascending
        out_s[q], out_i[q] = s[q][order], cand_ids[q][order]
        flags[q] = 0 if verified(n_cand, yd.shape[0], cand_s16[q, -1], out_s[q, -1], A[q], r[q], Rmax, Nmax) else 1
    return out_s, out_i, flags


def rungs(n_rows, k, max_candidates=MAX_K):
    """The candidate counts of the search's rungs: 2 k + 32, doubled up to min(n_rows, max_candidates)."""
    top = min(n_rows, max_candidates)
    assert 1 <= k <= top
    n = min(top, 2 * k + 32)
    out = [n]
    while n < top:
        n = min(top, 2 * n)
        out.append(n)
    return out


def dense_filter(s16_row, tau, A, r, res_b, norm_b, Rmax, Nmax):
    """Rows of one query that may reach tau on the fp32 rows: s16 + A res_bounds[j] + r norm_bounds[j] + slack_j >= tau (fp64)."""
    s = np.asarray(s16_row, np.float32).astype(np.float64)
    up = (s + (np.float64(A) * np.asarray(res_b, np.float32).astype(np.float64)
               + np.float64(r) * np.asarray(norm_b, np.float32).astype(np.float64))) + slack(s, np.float32(tau), A, Rmax, Nmax)
    return np.nonzero(up >= np.float64(np.float32(tau)))[0]


def exact_search(xq, xd, dtype, k, normalize=False, max_candidates=MAX_K, block=None):
    """ExactF32Index.search on the CPU: fp32 queries xq [nq, dim] and corpus xd [n_rows, dim] -> (ids [nq, k] int64, scores [nq, k]
    fp32, stats).  stats = {"rungs": candidates per rung that ran, "flagged": queries unverified after each, "dense": queries that took
    the dense path, "dense_rows": rows its filter kept, per dense query}.  The result is ranking()'s whatever path a query takes."""
    yq, yd = kept_rows(xq, normalize), kept_rows(xd, normalize)
    hq, hd = index_ref.pack(yq, dtype), index_ref.pack(yd, dtype)
    nq, n_rows = yq.shape[0], yd.shape[0]
    rq, rd = res_bounds(yq, hq, dtype), res_bounds(yd, hd, dtype)
    nbq, nbd = norm_bounds(hq, dtype), norm_bounds(hd, dtype)
    A = query_norm_bounds(nbq, rq)
    Rmax, Nmax = rd.max(), nbd.max()
    if not np.all(np.isfinite([Rmax, Nmax])) or not (np.all(np.isfinite(A)) and np.all(np.isfinite(rq))):
        raise ValueError("non-finite embeddings: the fp32 ranking needs finite bounds")
    yd_t = np.ascontiguousarray(yd.T)
    s16 = index_ref.canonical_scores(hq, hd, dtype)
    if block is not None:
        for q in range(nq):
            if len(block[q]):
                s16[q, np.asarray(block[q], np.int64)] = BLOCKED
    order = [index_ref._order(s16[q]) for q in range(nq)]
    out_i = np.empty((nq, k), np.int64)
    out_s = np.empty((nq, k), np.float32)
    stats = {"rungs": [], "flagged": [], "dense": 0, "dense_rows": []}
    todo = np.arange(nq)
    for n_cand in rungs(n_rows, k, max_candidates):
        if todo.size == 0:
            break
        ids = np.stack([order[q][:n_cand] for q in todo])
        s, i, flags = rescore(yq[todo], yd, ids, np.take_along_axis(s16[todo], ids, 1), k, A[todo], rq[todo], Rmax, Nmax, yd_t=yd_t)
        out_s[todo], out_i[todo] = s, i
        todo = todo[flags != 0]
        stats["rungs"].append(n_cand)
        stats["flagged"].append(int(todo.size))
    for q in todo:
        keep = dense_filter(s16[q], out_s[q, -1], A[q], rq[q], rd, nbd, Rmax, Nmax)
        s, i, _ = rescore(yq[q:q + 1], yd, keep[None, :], s16[q][keep][None, :], k, A[q:q + 1], rq[q:q + 1], Rmax, Nmax, yd_t=yd_t)
        out_s[q], out_i[q] = s[0], i[0]
        stats["dense"] += 1
        stats["dense_rows"].append(int(keep.size))
    return out_i, out_s, stats
