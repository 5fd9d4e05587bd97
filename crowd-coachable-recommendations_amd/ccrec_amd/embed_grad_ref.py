"""numpy restatement of ccr_embedding_grad's summation (csrc/ccr_embed_train.hip, include/ccr_retrieval.h): the kernel's bit-exact
oracle, in the manner of optim_ref and dropout_ref.

grad[r] = the sum of d_x[row] over the token rows whose id, clamped to 0 .. n_rows - 1, is r.  The order of the additions is part of the
interface: the rows of one id, in ascending row order (its RUN), are cut into chunks of CHUNK = 64 consecutive entries; a chunk is summed
sequentially in fp32 starting from its first entry; the chunk sums are then added sequentially, in order.  Only fp32 additions, each
rounded to nearest even -- numpy's float32 `+` on arrays is exactly that, one column per element.  Rows of ids that do not occur are +0."""
import numpy as np

CHUNK = 64   # CCR_EMBED_GRAD_CHUNK


def order(idx, n_rows):
    """The permutation the kernel is handed: token rows sorted by (clamped id, row) ascending."""
    ids = np.clip(np.asarray(idx, dtype=np.int64), 0, int(n_rows) - 1)
    return np.argsort(ids, kind="stable").astype(np.int64)


def run_sum(rows, chunk=CHUNK):
    """The normative sum of one run: rows [n, dim] float32 in run order (n >= 1) -> [dim] float32."""
    rows = np.asarray(rows, dtype=np.float32)
    total = None
    for c0 in range(0, rows.shape[0], chunk):
        s = rows[c0].copy()
        for e in range(c0 + 1, min(c0 + chunk, rows.shape[0])):
            s = s + rows[e]
        total = s if total is None else total + s
    return total


def embedding_grad(idx, d_x, n_rows, chunk=CHUNK):
    """idx [T] integer, d_x [T, dim] float32 -> grad [n_rows, dim] float32 with the kernel's bits."""
    d_x = np.ascontiguousarray(d_x, dtype=np.float32)
    ids = np.clip(np.asarray(idx, dtype=np.int64), 0, int(n_rows) - 1)
    grad = np.zeros((int(n_rows), d_x.shape[1]), dtype=np.float32)
    perm = np.argsort(ids, kind="stable")
    sorted_ids = ids[perm]
    starts = np.flatnonzero(np.r_[True, sorted_ids[1:] != sorted_ids[:-1]]) if ids.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], ids.size]
    for lo, hi in zip(starts, ends):
        grad[sorted_ids[lo]] = run_sum(d_x[perm[lo:hi]], chunk)
    return grad
