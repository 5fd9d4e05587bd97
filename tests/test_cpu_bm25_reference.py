"""The BM25 reference and builders of tests/helpers.py, checked on the CPU: the numpy restatement against the oracle on golden g12 (which
test_bm25.py ties to the reference project's own output), the structured index's invariants, the exact probes' bits, and the restated
filter on hand-made rows.  tests/test_gpu_bm25_edges.py runs csrc/ccr_bm25.hip against all of it."""
import json
import os

import numpy as np
import pytest

from helpers import (BM25_MASK_EDGE_DOCS, BM25_PROBE_SHARED_DOC, BM25_ROUNDING_PROBES, BM25_SLICE_KINDS, bm25_mask_probe, bm25_mask_value,
                     bm25_order_probe, bm25_reference_filter, bm25_reference_rows, bm25_reference_topk, bm25_slice_lengths,
                     bm25_structured_layout, bm25_structured_postings, bm25_structured_queries)
from oracle import oracle as orc


def test_reference_equals_the_oracle_on_golden_g12(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "g12_bm25.json")))
    model = orc.bm25_fit(list(g["corpus"].values()), b=g["b"], k1=g["k1"])
    qtexts = list(g["queries"].values())
    queries = [orc.bm25_query_terms(model, t) for t in qtexts]
    rows = bm25_reference_rows(model["indptr"], model["doc_ids"], model["tf"], model["doc_k"], model["idf"], queries, model["k1"])
    dense = np.stack([orc.bm25_scores(model, t) for t in qtexts])
    assert np.array_equal(rows.view(np.uint32), dense.view(np.uint32))
    for k in (1, 7, model["n_docs"]):
        ref_i, ref_s = orc.bm25_ranking(model, qtexts, k)
        ids, sc = bm25_reference_topk(rows, k)
        assert np.array_equal(ids, ref_i) and np.array_equal(sc.view(np.uint32), ref_s.view(np.uint32))


@pytest.mark.parametrize("tile,step", [(512, 64), (512, 128), (512, 256), (1024, 64), (1024, 128), (1024, 256)])
@pytest.mark.parametrize("n_docs", [1023, 1024, 1025, 2049, 3073, 4096])
def test_structured_index_invariants(n_docs, tile, step):
    indptr, rows, counts, doc_k, idf = bm25_structured_postings(n_docs, tile, step, seed=n_docs)
    lay = bm25_structured_layout()
    assert len(indptr) == lay["n_terms"] + 1 == len(idf) + 1 and indptr[0] == 0 and indptr[-1] == len(rows) == len(counts)
    assert rows.min() == 0 and rows.max() == n_docs - 1 and len(doc_k) == n_docs
    for t in range(lay["n_terms"]):                                     # documents ascend strictly inside a term
        assert (np.diff(rows[indptr[t]:indptr[t + 1]].astype(np.int64)) > 0).all(), t
    for t in lay["empty"]:                                              # first, a consecutive pair in the middle, last
        assert indptr[t] == indptr[t + 1]
    assert lay["empty"][0] == 0 and lay["empty"][1] + 1 == lay["empty"][2] and lay["empty"][3] == lay["n_terms"] - 1
    assert 0 < indptr[lay["empty"][1]] < len(rows) and indptr[lay["empty"][3]] == len(rows)
    # every slice length of the set occurs (clipped to the documents a tile has)
    want = {0, 1, step - 1, step, step + 1, 2 * step, 2 * step + 1, tile}
    assert len(BM25_SLICE_KINDS) == 8
    n_tiles = (n_docs + tile - 1) // tile
    sizes = [min(n_docs, (i + 1) * tile) - i * tile for i in range(n_tiles)]
    seen = [set() for _ in range(n_tiles)]
    for t in lay["regular"]:
        for i, n in enumerate(bm25_slice_lengths(indptr, rows, t, n_docs, tile)):
            seen[i].add(int(n))
    for i in range(n_tiles):
        assert seen[i] == {min(w, sizes[i]) for w in want}, (i, seen[i])
    if n_docs == 4096:
        assert seen[0] == {w for w in want if w <= tile}
    # a posting exactly at every run boundary (multiples of 512: every CCR_BM25_RUN_TILES x tile used) and one just before it
    e = rows[indptr[lay["E"]]:indptr[lay["E"] + 1]]
    for b in range(512, n_docs, 512):
        assert b in e and b - 1 in e
    assert np.array_equal(rows[indptr[lay["A"]]:indptr[lay["A"] + 1]], np.arange(n_docs))
    last = rows[indptr[lay["L"]]:indptr[lay["L"] + 1]]                  # the index's last list: one full step inside one tile
    assert indptr[lay["L"] + 1] == len(rows) and len(last) == step and last[0] // tile == last[-1] // tile and last[-1] - last[0] == step - 1
    assert counts.max() == 2.0 ** 24 and counts.min() >= 1 and np.array_equal(counts, np.round(counts))
    assert doc_k.min() == 1e-3 and doc_k.max() == 1e3 and len(set(idf.tolist())) == len(idf) and idf.min() > 0
    # the query set: the counts of active terms per tile it promises
    queries = bm25_structured_queries(indptr, rows, n_docs, tile, seed=n_docs)
    active = [{n: 0 for n in (1, 4, 5, 8, 9)} for _ in range(n_tiles)]
    for q in queries:
        assert (np.diff(q) > 0).all()
        if 2 <= len(q) <= 11 and set(q.tolist()) <= set(lay["regular"]):
            per_tile = sum((bm25_slice_lengths(indptr, rows, t, n_docs, tile) > 0).astype(int) for t in q)
            for i, n in enumerate(per_tile):
                if n in active[i]:
                    active[i][int(n)] += 1
    assert all(c >= 2 for a in active for c in a.values()), active
    assert sum(len(q) == 64 for q in queries) == 1 and sum(len(q) == 0 for q in queries) == 1


def test_exact_probes_evaluate_to_the_stated_bits():
    indptr, rows, counts, doc_k, w = bm25_order_probe()
    for n_terms in (64, 256, 260):
        row = bm25_reference_rows(indptr, rows, counts, doc_k, w, [np.arange(n_terms)], 1.0)[0]
        for first, ws, doc, bits in BM25_ROUNDING_PROBES:
            if first + len(ws) <= n_terms:
                assert row[doc].view(np.uint32) == bits, (first, hex(row[doc].view(np.uint32)))
    # ... and the alternatives the probes are there to catch give other bits: fp32 accumulation, and the terms in the other order
    for first, ws, doc, bits in BM25_ROUNDING_PROBES:
        acc32 = np.float32(0)
        for x in ws:
            acc32 = np.float32(acc32 + np.float32(x))
        rev = np.float64(0)
        for x in ws[::-1]:
            rev = rev + np.float64(x)
        if len(ws) == 3:
            assert acc32.view(np.uint32) != bits or np.float32(rev).view(np.uint32) != bits, first
    assert [np.float32(np.float64(1) + 2.0 ** -24 + 2.0 ** -50).view(np.uint32), np.float32(np.float64(1) + 2.0 ** -24).view(np.uint32)] == [0x3F800001, 0x3F800000]
    # all 260 terms meet in one document; no filler term touches a probe document
    assert all(BM25_PROBE_SHARED_DOC in rows[indptr[t]:indptr[t + 1]] for t in range(260))
    for first, ws, doc, _ in BM25_ROUNDING_PROBES:
        holders = [t for t in range(260) if doc in rows[indptr[t]:indptr[t + 1]]]
        assert holders == list(range(first, first + len(ws)))
    # the presence mask: the score IS the subset's bitmask, for every document and block
    indptr, rows, counts, doc_k, w, member = bm25_mask_probe()
    ref = bm25_reference_rows(indptr, rows, counts, doc_k, w, [np.arange(64 * g, 64 * g + 64) for g in range(4)], 1.0)
    for g in range(4):
        for d in np.flatnonzero(member.any(1)):
            v = bm25_mask_value(member[d], g)
            assert ref[g, d] == v and float(v) * 2 ** 23 == int(float(v) * 2 ** 23) and v > 0
    assert all(member[d].any() for d in BM25_MASK_EDGE_DOCS)
    lanes = np.flatnonzero(member.any(0)) % 64
    assert {0, 1, 62, 63} <= set(lanes.tolist())


def test_reference_filter_on_hand_made_rows():
    n_docs, rank, k = 3000, 40, 10
    zeros = np.zeros(n_docs, np.float32)
    assert bm25_reference_filter(zeros, n_docs, rank, k) == (0.0, 0, False)             # zero fill finishes the row
    row = zeros.copy()                                                                  # fewer than `rank` positives in the sample
    row[:39] = 2.0
    row[2000:2005] = 1.0
    assert bm25_reference_filter(row, n_docs, rank, k) == (0.0, 44, False)
    assert bm25_reference_filter(row, n_docs, rank, 45) == (0.0, 44, False)             # 44 < k: sorted positives, then zeros
    row[39] = 3.0                                                                       # the 40th positive: tau = 2
    assert bm25_reference_filter(row, n_docs, rank, k) == (2.0, 40, False)              # ties at tau all pass
    assert bm25_reference_filter(row, n_docs, rank, 41) == (2.0, 40, True)              # tau > 0 and fewer than k reach it
    row[1500:2000] = 2.0                                                                # ties at tau outside the sample pass as well
    assert bm25_reference_filter(row, n_docs, rank, k) == (2.0, 540, False)
    neg = zeros.copy()                                                                  # a negative score: zeros rank above it
    neg[1024] = -1.0
    assert bm25_reference_filter(neg, n_docs, rank, k) == (0.0, 0, True)
    neg[1100:1110] = 1.0
    assert bm25_reference_filter(neg, n_docs, rank, k) == (0.0, 10, False)              # k positives: the negative cannot reach the top
    assert bm25_reference_filter(neg, n_docs, rank, 11) == (0.0, 10, True)
    neg[:1024] = -2.0                                                                   # tau < 0: still only positive scores pass
    assert bm25_reference_filter(neg, n_docs, rank, k) == (-2.0, 10, False)
    nan = zeros.copy()
    nan[2000] = np.nan
    assert bm25_reference_filter(nan, n_docs, rank, k)[1:] == (0, True)
    flood = np.ones(20_000, np.float32)
    flood[:1024] = 0.0
    assert bm25_reference_filter(flood, 20_000, rank, k) == (0.0, 18_976, True)         # more than the list holds
    flood[1024 + 16_384:] = 0.0
    assert bm25_reference_filter(flood, 20_000, rank, k) == (0.0, 16_384, False)
    two = np.zeros(66_561, np.float32)                                                  # a second piece of one real document and -inf
    two[65_536] = 5.0
    two[:38] = 1.0
    assert bm25_reference_filter(two, 66_561, rank, k) == (0.0, 39, False)
    two[38] = 1.0
    assert bm25_reference_filter(two, 66_561, rank, k) == (1.0, 40, False)
