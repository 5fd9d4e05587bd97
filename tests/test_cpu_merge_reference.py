"""The merge oracle checked on its own (no GPU): tests/test_gpu_merge.py compares the HIP merges with orc.merge_topk and
orc.merge_short_lists bit for bit, so these two are first held to the plainest statement of the same operation -- one np.lexsort of a
query's R k entries by (score desc, id asc) -- on the generator and at the (R, k) pairs the GPU test uses."""
import numpy as np
import pytest

from helpers import MERGE_CASES, MERGE_ID_SHIFT, canonical_order, synthetic_shard_lists
from oracle import oracle as orc


def _lexsort_merge(scores, ids, k_out):
    R, n_q, k = scores.shape
    os_, oi = np.empty((n_q, k_out), np.float32), np.empty((n_q, k_out), np.int64)
    for q in range(n_q):
        s, i = scores[:, q].reshape(-1), ids[:, q].reshape(-1)
        o = np.lexsort((i, -s.astype(np.float64)))[:k_out]
        os_[q], oi[q] = s[o], i[o]
    return os_, oi


@pytest.mark.parametrize("levels", [1, 2, 6, 0])
@pytest.mark.parametrize("R,k", MERGE_CASES)
def test_generator_gives_canonical_lists_of_distinct_ids(R, k, levels):
    scores, ids = synthetic_shard_lists(R, 2, k, levels, seed=R * 10007 + k)
    assert scores.dtype == np.float32 and ids.dtype == np.int64 and scores.shape == ids.shape == (R, 2, k)
    assert not np.isnan(scores).any()
    for q in range(2):
        assert len(set(ids[:, q].reshape(-1).tolist())) == R * k
        for r in range(R):
            assert np.array_equal(canonical_order(scores[r, q], ids[r, q]), np.arange(k))
    assert ids[R - 1].min() >= MERGE_ID_SHIFT and (R == 1 or ids[:R - 1].max() < 3 * R * k)
    if levels == 1:
        assert np.all(scores == -np.inf)
    if levels == 6 and R * k >= 600:
        assert np.isposinf(scores).any() and np.isneginf(scores).any()


@pytest.mark.parametrize("levels", [1, 2, 6, 0])
@pytest.mark.parametrize("R,k", MERGE_CASES)
def test_oracle_merge_topk_is_one_lexsort(R, k, levels):
    scores, ids = synthetic_shard_lists(R, 3, k, levels, seed=R * 10007 + k)
    os_, oi = orc.merge_topk(scores, ids)
    ref_s, ref_i = _lexsort_merge(scores, ids, k)
    assert np.array_equal(oi, ref_i)
    assert np.array_equal(os_.view(np.uint32), ref_s.view(np.uint32))


def test_oracle_merge_short_lists_flags_exactly_the_consumed_truncated_lists():
    """orc.merge_short_lists on hand-made lists: the kept entries are the lexsort's, padding slots (ids above 2^62) never count as real
    entries, and a query is flagged exactly when every real entry of a truncated list is kept."""
    pad = np.iinfo(np.int64).max
    inf = np.float32(-np.inf)
    # R = 3, kl = 3, k_out = 5.  shard 0: truncated, 3 real; shard 1: sent everything, 3 real; shard 2: sent everything, 1 real + 2 pads
    scores = np.array([[[9, 8, 1], [9, 8, 7]],
                       [[7, 6, 5], [6, 5, 4]],
                       [[7, inf, inf], [3, inf, inf]]], np.float32)
    ids = np.array([[[10, 11, 12], [10, 11, 12]],
                    [[20, 21, 22], [20, 21, 22]],
                    [[5, pad - 6, pad - 7], [5, pad - 6, pad - 7]]], np.int64)
    os_, oi, flags = orc.merge_short_lists(scores, ids, [True, False, False], 5)
    assert oi.tolist() == [[10, 11, 5, 20, 21], [10, 11, 12, 20, 21]]      # query 0: the 7.0 tie goes to the lower id (shard 2's 5)
    assert os_.tolist() == [[9, 8, 7, 7, 6], [9, 8, 7, 6, 5]]
    assert flags.tolist() == [0, 1]                                        # query 1 keeps all of truncated shard 0
    assert orc.merge_short_lists(scores, ids, [False, False, True], 5)[2].tolist() == [1, 0]   # shard 2's ONE real entry kept / not kept
    ref_s, ref_i = _lexsort_merge(scores, ids, 5)
    assert np.array_equal(oi, ref_i) and np.array_equal(os_, ref_s)
