"""csrc/ccr_bm25.hip against a plain numpy fp64 restatement (helpers.bm25_reference_rows / _topk / _filter), bit for bit -- ids equal and
score bits equal, no tolerance: the order (score descending, document ascending) is total -- on inputs written around the kernels' control
flow instead of random corpora: slices of exactly one cursor step, one more, lists that end at a step and at the index's last posting,
postings at and just before every run boundary, 4 / 5 / 8 / 9 active terms per tile, 64 | 65 ... 256 | 257 terms per query, exact probes
for the order of the adds and the single rounding, candidate lists of k - 1 ... 16 385 records, zero fill, negative / infinite / NaN
weights, several batches of the round kernels, and the contribution table's term lookup.  Every case asserts the path it ran.
The builders and their own checks: tests/helpers.py, tests/test_cpu_bm25_reference.py."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import (BM25_MASK_EDGE_DOCS, BM25_PROBE_DOCS, BM25_PROBE_SHARED_DOC, BM25_ROUNDING_PROBES, _random_postings, bm25_mask_probe,
                     bm25_mask_value, bm25_order_probe, bm25_postings_from_lists, bm25_reference_filter, bm25_reference_rows,
                     bm25_reference_topk, bm25_structured_layout, bm25_structured_postings, bm25_structured_queries)

pytestmark = pytest.mark.gpu

# CCR_BM25_TILE -> (documents per tile, postings per step); -1: the round kernels (the index of the default shape)
TILE_SHAPES = {-1: (1024, 128), 0: (1024, 128), 1: (1024, 64), 2: (512, 128), 3: (1024, 256), 4: (512, 256)}
KNOBS = ("CCR_BM25_TILE", "CCR_BM25_RUN_TILES", "CCR_BM25_REDO_ROWS", "CCR_BM25_TABLE", "CCR_BM25_DENSE_SELECT")
ROUNDS, STORED, FUSED = "rounds+stored_rows", "tile+stored_rows", "tile+fused_filter"


def _make(monkeypatch, index, k1, tile=None, run_tiles=None, redo_rows=None, table=True):
    """An index under exactly these knobs (the others deleted).  index = (indptr, rows, counts, doc_k, idf)."""
    from ccrec_amd.bm25 import BM25
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in (("CCR_BM25_TILE", tile), ("CCR_BM25_RUN_TILES", run_tiles), ("CCR_BM25_REDO_ROWS", redo_rows), ("CCR_BM25_TABLE", None if table else 0)):
        if v is not None:
            monkeypatch.setenv(name, str(v))
    model = BM25.from_postings(*index, k1=k1)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return model


def _search(monkeypatch, model, queries, k, dense, path, table):
    """-> (ids, scores, stats) on the host; the path and the table use are asserted."""
    if dense:
        monkeypatch.setenv("CCR_BM25_DENSE_SELECT", "1")
    else:
        monkeypatch.delenv("CCR_BM25_DENSE_SELECT", raising=False)
    s, i = model.transform_terms_topk(queries, k)
    st = model.last_stats()
    assert st["path"] == path and st["contribution_table"] == (table and path != ROUNDS), st
    return i.cpu().numpy(), s.cpu().numpy(), st


def _same(ids, sc, ref_ids, ref_sc, what):
    assert ids.shape == ref_ids.shape and sc.shape == ref_sc.shape, (what, ids.shape, ref_ids.shape)
    bad = (ids != ref_ids) | (sc.view(np.uint32) != ref_sc.view(np.uint32))
    if bad.any():
        r, c = np.argwhere(bad)[0]
        pytest.fail(f"{what}: {int(bad.any(1).sum())} rows differ, first query {r} rank {c}: document {ids[r, c]} score {sc[r, c]!r} "
                    f"(0x{sc[r, c].view(np.uint32):08X}), reference document {ref_ids[r, c]} score {ref_sc[r, c]!r} (0x{ref_sc[r, c].view(np.uint32):08X})")


def _redo_expected(ref_rows, rank, k):
    return sum(bm25_reference_filter(row, len(row), rank, k)[2] for row in ref_rows)


def _fused_vs_reference(monkeypatch, model, queries, k, ref_rows, table, what):
    ids, sc, st = _search(monkeypatch, model, queries, k, False, FUSED, table)
    _same(ids, sc, *bm25_reference_topk(ref_rows, k), what)
    assert st["rows_redone"] == _redo_expected(ref_rows, st["sample_rank"], k), (what, st)
    return st


_STRUCTURED = {}


def _structured(n_docs, cfg):
    """Index, queries and reference rows (under idf and under 1.25 idf) of one (corpus size, tile shape), built once."""
    tile, step = TILE_SHAPES[cfg]
    key = (n_docs, tile, step)
    if key not in _STRUCTURED:
        index = bm25_structured_postings(n_docs, tile, step, seed=n_docs)
        queries = bm25_structured_queries(index[0], index[1], n_docs, tile, seed=n_docs)
        ref = {scale: bm25_reference_rows(*index[:4], index[4] * scale, queries, 1.2) for scale in (1.0, 1.25)}
        _STRUCTURED[key] = (index, queries, ref)
    return _STRUCTURED[key]


def _variants(monkeypatch, index, k1, **knobs):
    """The three ways a query's weights reach the scorer: the contribution table, tf / K_d per posting with the index's idf
    (CCR_BM25_TABLE=0), and weights that are not the index's idf (the generic path) -> (name, model, weight scale, table used)."""
    yield "table", _make(monkeypatch, index, k1, **knobs), 1.0, True
    yield "no table", _make(monkeypatch, index, k1, table=False, **knobs), 1.0, False
    other = _make(monkeypatch, index, k1, **knobs)
    other.idf = index[4] * 1.25
    yield "generic", other, 1.25, False


# ------------------------------------------------------------------------------------------------ a. every document, stored rows
@pytest.mark.parametrize("n_docs", [1023, 1024, 1025, 2049, 3073, 4096])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
def test_every_document_of_every_tile_shape(cfg, n_docs, monkeypatch):
    """k = n_docs with the stored rows: the whole row comes back, so EVERY document's score is compared.  Runs of 1, 2 and 3 tiles put
    the run boundaries (binary search: the posting at run_base is taken, the one before it is not) on 512, 1024, 1536, 2048 and 3072."""
    index, queries, ref = _structured(n_docs, cfg)
    path = ROUNDS if cfg < 0 else STORED
    multi = next(j for j, q in enumerate(queries) if len(q) == 11)
    tops = {scale: bm25_reference_topk(rows, n_docs) for scale, rows in ref.items()}
    for run_tiles in ((None,) if cfg < 0 else (None, 1, 2, 3)):
        for name, model, scale, table in _variants(monkeypatch, index, 1.2, tile=cfg, run_tiles=run_tiles):
            what = f"tile cfg {cfg}, {n_docs} documents, run tiles {run_tiles}, {name}"
            ref_ids, ref_sc = tops[scale]
            ids, sc, _ = _search(monkeypatch, model, queries, n_docs, True, path, table)
            _same(ids, sc, ref_ids, ref_sc, what)
            for j in (multi, len(queries) - 3):                       # one query per call: every ticket is one tile
                ids, sc, _ = _search(monkeypatch, model, queries[j:j + 1], n_docs, True, path, table)
                _same(ids, sc, ref_ids[j:j + 1], ref_sc[j:j + 1], what + f", query {j} alone")


# ------------------------------------------------------------------------------------------------ b. the same through FILTER
@pytest.mark.parametrize("n_docs", [2049, 3073, 4096])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
def test_every_tile_shape_through_the_fused_filter(cfg, n_docs, monkeypatch):
    """k = 100 of 2 049 ... 4 096 documents takes the sampled filter.  The E term (a posting at every multiple of 512 and one before it:
    4 of them in the sample, fewer than k in all), the empty terms and the empty query give tau = 0 and fewer than k records: the row is the
    sorted positives followed by the zero fill, i.e. every positive score that FILTER computed is compared; the regular terms have
    hundreds of postings in the sample (tau > 0).  rows_redone is the restated filter's count, exactly."""
    index, queries, ref = _structured(n_docs, cfg)
    lay = bm25_structured_layout()
    k = 100
    for run_tiles in (None, 2):
        for name, model, scale, table in _variants(monkeypatch, index, 1.2, tile=cfg, run_tiles=run_tiles):
            what = f"fused, tile cfg {cfg}, {n_docs} documents, run tiles {run_tiles}, {name}"
            st = _fused_vs_reference(monkeypatch, model, queries, k, ref[scale], table, what)
            verdicts = [bm25_reference_filter(row, n_docs, st["sample_rank"], k) for row in ref[scale]]
            assert verdicts[lay["E"]][0] == 0 and 0 < verdicts[lay["E"]][1] < k and not verdicts[lay["E"]][2]      # tau = 0, zero fill
            assert sum(tau > 0 for tau, _, _ in verdicts) >= 20 and verdicts[-2][:2] == (0, 0)


# ------------------------------------------------------------------------------------------------ c + d. cursor groups, exact probes
_PROBE = {}


def _order_probe():
    if not _PROBE:
        index = bm25_order_probe()
        prefixes = [np.arange(n, dtype=np.int32) for n in (64, 65, 128, 129, 192, 193, 256)]
        one = [np.asarray([5], np.int32)]
        _PROBE["index"] = index
        _PROBE["batches"] = {"narrow": [prefixes[0]] + one, "wide": prefixes, "wide+one": prefixes + one,
                             "too long": prefixes + one + [np.arange(257, dtype=np.int32)]}
        _PROBE["ref"] = {n: bm25_reference_rows(*index, qs, 1.0) for n, qs in _PROBE["batches"].items()}
    return _PROBE


def _assert_probe_bits(ids, sc, queries, what):
    for r, q in enumerate(queries):
        for first, ws, doc, bits in BM25_ROUNDING_PROBES:
            if first + len(ws) <= len(q):
                at = np.flatnonzero(ids[r] == doc)
                assert len(at) == 1 and sc[r, at[0]].view(np.uint32) == bits, \
                    f"{what}: query of {len(q)} terms, document {doc} (terms {first}..): {[hex(x) for x in sc[r, at].view(np.uint32)]}, must be {bits:#x}"


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
def test_cursor_groups_term_order_and_one_rounding(cfg, monkeypatch):
    """Queries of the first 64, 65, 128, 129, 192, 193 and 256 terms of the order probe (all 260 terms have postings in tile [1024, 2048) and
    meet in one document), with and without a one-term row in the batch (the batch chooses G = 4: the short row runs through the wide
    kernel), and with a 257-term row (the whole call takes the round kernels).  Contributions are the weights themselves, so the probe
    documents must carry exactly 0x3F800000 / 0x3F800001: another order of the adds, an fp32 accumulation or a second rounding fails.
    Stored and fused, with the table and with weights passed per query."""
    P = _order_probe()
    indptr, rows, counts, doc_k, w = P["index"]
    n_docs = BM25_PROBE_DOCS
    table_model = _make(monkeypatch, P["index"], 1.0, tile=cfg)
    generic_model = _make(monkeypatch, (indptr, rows, counts, doc_k, w * 0.5), 1.0, tile=cfg)
    generic_model.idf = w                                             # the table holds w / 2, the queries ask for w
    plain_model = _make(monkeypatch, P["index"], 1.0, tile=cfg, table=False)
    for name, model, table in (("table", table_model, True), ("generic", generic_model, False), ("no table", plain_model, False)):
        for batch, queries in P["batches"].items():
            rounds = cfg < 0 or batch == "too long"
            what = f"tile cfg {cfg}, {name}, batch {batch}"
            ids, sc, _ = _search(monkeypatch, model, queries, n_docs, True, ROUNDS if rounds else STORED, table)
            _same(ids, sc, *bm25_reference_topk(P["ref"][batch], n_docs), what + ", stored")
            _assert_probe_bits(ids, sc, queries, what + ", stored")
            assert ids[0, 0] == BM25_PROBE_SHARED_DOC
            if not rounds:
                ids, sc, st = _search(monkeypatch, model, queries, 100, False, FUSED, table)
                _same(ids, sc, *bm25_reference_topk(P["ref"][batch], 100), what + ", fused")
                _assert_probe_bits(ids, sc, queries, what + ", fused")
                assert st["rows_redone"] == _redo_expected(P["ref"][batch], st["sample_rank"], 100), (what, st)


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])
def test_presence_mask(cfg, monkeypatch):
    """Term t weighs 2^-(t % 24) and contributes exactly that, so a document's score under the query of one block of 64 terms is the
    bitmask of the lists it is in: a dropped, doubled or misplaced posting names its bit.  Documents at every tile and run edge, terms
    in lanes 0, 1, 62 and 63; the 256-term query walks the same lists as cursor groups 64 + r, 128 + r, 192 + r."""
    indptr, rows, counts, doc_k, w, member = bm25_mask_probe()
    index = (indptr, rows, counts, doc_k, w)
    n_docs = BM25_PROBE_DOCS
    blocks = [np.arange(64 * g, 64 * g + 64, dtype=np.int32) for g in range(4)]
    whole = [np.arange(256, dtype=np.int32), np.asarray([0, 63, 64, 255], np.int32)]
    ref_whole = bm25_reference_rows(*index, whole, 1.0)
    expect = np.zeros((4, n_docs), np.float32)
    for g in range(4):
        for d in np.flatnonzero(member.any(1)):
            expect[g, d] = bm25_mask_value(member[d], g)
    path = ROUNDS if cfg < 0 else STORED
    for run_tiles in ((None,) if cfg < 0 else (None, 2, 3)):
        for table in (True, False):
            model = _make(monkeypatch, index, 1.0, tile=cfg, run_tiles=run_tiles, table=table)
            what = f"tile cfg {cfg}, run tiles {run_tiles}, table {table}"
            ids, sc, _ = _search(monkeypatch, model, blocks, n_docs, True, path, table)
            for g in range(4):
                got = np.zeros(n_docs, np.float32)
                got[ids[g]] = sc[g]
                assert len(set(ids[g].tolist())) == n_docs
                for d in np.flatnonzero(got != expect[g]):
                    wrong = int(round(abs(float(got[d]) - float(expect[g, d])) * 2 ** 23))
                    pytest.fail(f"{what}: block {g} document {d}{' (an edge)' if d in BM25_MASK_EDGE_DOCS else ''}: score {got[d]!r}, mask "
                                f"{expect[g, d]!r}; differing weight bits {wrong:#x} (bit 23 - j <-> terms with t % 24 == j)")
            _same(ids, sc, *bm25_reference_topk(expect, n_docs), what)
            ids, sc, _ = _search(monkeypatch, model, whole, n_docs, True, path, table)
            _same(ids, sc, *bm25_reference_topk(ref_whole, n_docs), what + ", 256 terms")
            if cfg >= 0:
                _fused_vs_reference(monkeypatch, model, blocks + whole, 100, np.concatenate([expect, ref_whole]), table, what + ", fused")


# ------------------------------------------------------------------------------------------------ e. list classes and zero fill
LIST_SIZES = [0, 9, 10, 11, 4095, 4096, 4097, 16383, 16384, 16385]
_LISTS = {}


def _list_index(equal):
    """20 000 documents.  Terms 0 .. 9: exactly LIST_SIZES[t] documents, all at ids >= 1024 (outside the sample: tau = 0 and exactly that
    many records); terms 10 .. 14: the zero-fill placements for k = 100.  equal: tf = 1 and doc_k = 1 everywhere, so a term's documents
    all score the same (mass ties, decided by the document id); else distinct doc_k."""
    if equal not in _LISTS:
        rs = np.random.RandomState(11)
        n_docs, k = 20_000, 100
        lists = [np.sort(rs.choice(np.arange(1024, n_docs), n, replace=False)) for n in LIST_SIZES]
        lists += [np.arange(30), np.arange(0, 78, 2), np.arange(k - 30, k), np.arange(n_docs - 50, n_docs),
                  np.concatenate([np.arange(0, 78, 2), 1024 + 3 * np.arange(60)])]            # 99 = k - 1 records around the one fill document
        indptr, rows, counts = bm25_postings_from_lists([(d, np.ones(len(d))) for d in lists])
        doc_k = np.ones(n_docs) if equal else rs.uniform(0.3, 3.0, n_docs)
        idf = rs.uniform(0.5, 4.0, len(lists))
        index = (indptr, rows, counts, doc_k, idf)
        queries = [np.asarray([t], np.int32) for t in range(len(lists))]
        _LISTS[equal] = (index, queries, bm25_reference_rows(*index, queries, 1.2))
    return _LISTS[equal]


@pytest.mark.parametrize("equal", [False, True], ids=["distinct", "equal"])
def test_list_classes_and_zero_fill(equal, monkeypatch):
    """Candidate lists of exactly 0, k - 1, k, k + 1, 4 095 / 4 096 / 4 097 (the two sort classes) and 16 383 / 16 384 / 16 385 (the capacity)
    records at k = 10: results against the reference, and rows_redone EXACTLY the restated filter's count -- only the 16 385 row.  At
    k = 100 the zero fill: listed documents {0 .. n-1}, {0, 2, 4, ..}, {k-n .. k-1}, the corpus's last n, and k - 1 of them around the
    single fill document."""
    index, queries, ref = _list_index(equal)
    model = _make(monkeypatch, index, 1.2)
    st = _fused_vs_reference(monkeypatch, model, queries, 10, ref, True, "k = 10")
    verdicts = [bm25_reference_filter(row, 20_000, st["sample_rank"], 10) for row in ref]
    assert [n for _, n, _ in verdicts[:10]] == LIST_SIZES and [redo for _, _, redo in verdicts[:10]] == [False] * 9 + [True]
    assert st["rows_redone"] == 1
    st = _fused_vs_reference(monkeypatch, model, queries, 100, ref, True, "k = 100")
    verdicts = [bm25_reference_filter(row, 20_000, st["sample_rank"], 100) for row in ref]
    assert all(tau == 0 and n < 100 and not redo for tau, n, redo in verdicts[10:]) and st["rows_redone"] == 1
    ids, _, _ = _search(monkeypatch, model, queries[10:], 100, False, FUSED, True)
    assert sorted(ids[0, :30].tolist()) == list(range(30)) and ids[0, 30:].tolist() == list(range(30, 100)) and ids[2, 30:].tolist() == list(range(70)) and ids[3, 50:].tolist() == list(range(50))
    assert ids[4, 99] == 1 and sorted(ids[1, 39:].tolist()) == ids[1, 39:].tolist() and ids[1, 39] == 1


def _search_abi(model, queries, k, canary):
    """ccr_bm25_search through the C ABI into outputs pre-filled with a canary."""
    lib, h = model._lib, model._h
    n_q = len(queries)
    q_ptr = np.zeros(n_q + 1, np.int64)
    q_ptr[1:] = np.cumsum([len(t) for t in queries])
    q_terms = np.concatenate(queries).astype(np.int32)
    q_idf = np.ascontiguousarray(model.idf[q_terms], np.float64)
    out_s = torch.full((n_q, k), float(canary), dtype=torch.float32, device="cuda")
    out_i = torch.full((n_q, k), int(canary), dtype=torch.int64, device="cuda")
    vp = ctypes.c_void_p
    ws = torch.empty(int(lib.ccr_bm25_search_workspace_bytes_k(h, n_q, max(len(t) for t in queries), k)), dtype=torch.uint8, device="cuda")
    rc = lib.ccr_bm25_search(h, q_ptr.ctypes.data_as(vp), q_terms.ctypes.data_as(vp), q_idf.ctypes.data_as(vp), n_q, k, out_s.data_ptr(),
                             out_i.data_ptr(), ws.data_ptr(), ws.numel(), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ccr_last_error().decode()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_s.cpu().numpy(), model.last_stats()


@pytest.mark.parametrize("k", [10, 100])
def test_redone_rows_land_in_their_own_output_rows(k, monkeypatch):
    """300 rows (the 15 list-class rows, 20 times) with CCR_BM25_REDO_ROWS = 2: the twenty 16 385-record rows are redone in ten chunks and
    must land at their own output rows, every other row as the filter left it; outputs pre-filled with a canary through the C ABI."""
    index, queries, ref = _list_index(False)
    model = _make(monkeypatch, index, 1.2, redo_rows=2)
    batch = queries * 20
    ref_ids, ref_sc = bm25_reference_topk(ref, k)
    ids, sc, st = _search_abi(model, batch, k, canary=-77)
    assert st["path"] == FUSED and st["contribution_table"] and st["rows_redone"] == 20 == 20 * _redo_expected(ref, st["sample_rank"], k), st
    _same(ids, sc, np.tile(ref_ids, (20, 1)), np.tile(ref_sc, (20, 1)), f"300 rows, k = {k}")


@pytest.mark.parametrize("k", [10, 1001])
def test_second_sample_piece_of_one_document(k, monkeypatch):
    """66 561 documents: the sample is [0, 1024) and [65 536, 66 560], a second piece that holds ONE real document and 1 023 fills of -inf."""
    rs = np.random.RandomState(66)
    n_docs = 66_561
    indptr, rows, counts, doc_k, idf = _random_postings(rs, n_docs, 200, dense_terms=3)
    extra = np.asarray([5, 40_000, n_docs - 1])
    indptr = np.concatenate([indptr, [indptr[-1] + len(extra)]])
    rows, counts, idf = np.concatenate([rows, extra]).astype(np.int32), np.concatenate([counts, [3, 1, 2]]).astype(np.float32), np.concatenate([idf, [9.0]])
    index = (indptr, rows, counts, doc_k, idf)
    queries = [np.sort(rs.choice(200, rs.randint(1, 7), replace=False)).astype(np.int32) for _ in range(9)]
    queries += [np.asarray([200], np.int32), np.asarray([0, 200], np.int32), np.asarray([150, 200], np.int32)]
    ref = bm25_reference_rows(*index[:4], idf, queries, 1.2)
    model = _make(monkeypatch, index, 1.2)
    _fused_vs_reference(monkeypatch, model, queries, k, ref, True, f"66 561 documents, k = {k}")
    ids, sc, _ = _search(monkeypatch, model, queries, k, True, STORED, True)
    _same(ids, sc, *bm25_reference_topk(ref, k), "stored")


# ------------------------------------------------------------------------------------------------ f. negative, zero, infinite, NaN weights
def _weights_index():
    rs = np.random.RandomState(23)
    n_docs = 20_000
    pool = rs.permutation(np.arange(1024, n_docs))
    # 0 NEG (30 documents, two of them in the sample)  1 FEW (5)  2 MANY (50)  3 ZERO (40)  4 INF (3)  5 NAN (7, none in the sample)
    lists = [np.sort(np.concatenate([[3, 700], pool[:28]])), np.sort(pool[30:35]), np.sort(pool[40:90]), np.sort(pool[100:140]),
             np.sort(pool[41:44]), np.sort(pool[300:307])]
    indptr, rows, counts = bm25_postings_from_lists([(d, rs.randint(1, 4, len(d))) for d in lists])
    doc_k = rs.uniform(0.3, 3.0, n_docs)
    weights = np.asarray([-1.5, 2.0, 1.0, 0.0, np.inf, np.nan])
    return (indptr, rows, counts, doc_k, np.ones(6)), weights


def test_negative_zero_and_infinite_weights(monkeypatch):
    """Weights set through model.idf (the generic path), k = 10.  Only negative matches: zeros rank above them, the filter lists nothing
    and the row must be redone (odd_cnt); positives and negatives with fewer than k positives: redone; with at least k: finished by
    the filter; a weight of 0 matches nothing; +inf scores sort first.  All against the reference, rows_redone exact."""
    index, weights = _weights_index()
    queries = [np.asarray(q, np.int32) for q in ([0], [0, 1], [0, 2], [3], [1, 4], [0, 4], [2, 3])]
    ref = bm25_reference_rows(*index[:4], weights, queries, 1.2)
    assert (ref[0] < 0).sum() == 30 and (ref[0] > 0).sum() == 0 and (ref[1] > 0).sum() == 5 and (ref[2] > 0).sum() == 50 and not ref[3].any()
    assert np.isinf(ref[4]).sum() == 3
    for cfg in (0, 4):
        model = _make(monkeypatch, index, 1.2, tile=cfg)
        model.idf = weights
        st = _fused_vs_reference(monkeypatch, model, queries, 10, ref, False, f"tile cfg {cfg}")
        assert st["rows_redone"] == 3, st                                       # NEG, NEG + FEW, NEG + INF (3 positives)
        ids, sc, _ = _search(monkeypatch, model, queries, 10, True, STORED, False)
        _same(ids, sc, *bm25_reference_topk(ref, 10), "stored")


def test_nan_weight(monkeypatch):
    """A NaN weight makes NaN scores.  The order every path must agree on is the dense selection's: a NaN sorts ABOVE +inf (its bit
    pattern is the largest), ties by document.  The fused, stored and round paths return identical bits for the NaN rows -- a row with
    at least k positive scores beside its NaNs among them: the filter's list holds k records and none of the NaN documents -- and the
    other rows of the batch still equal the reference."""
    index, weights = _weights_index()
    queries = [np.asarray(q, np.int32) for q in ([2], [5], [0, 1], [2, 5], [1, 5], [1, 2])]
    nan_rows, others = [1, 3, 4], [0, 2, 5]
    ref = bm25_reference_rows(*index[:4], weights, queries, 1.2)
    assert all(np.isnan(ref[r]).sum() == 7 for r in nan_rows) and (ref[3] > 0).sum() == 50
    results = {}
    for name, cfg, dense, path in (("fused", 0, False, FUSED), ("stored", 0, True, STORED), ("rounds", -1, True, ROUNDS)):
        model = _make(monkeypatch, index, 1.2, tile=cfg)
        model.idf = weights
        ids, sc, st = _search(monkeypatch, model, queries, 10, dense, path, False)
        _same(ids[others], sc[others], *bm25_reference_topk(ref[others], 10), name)
        results[name] = (ids, sc.view(np.uint32), st)
    for name in ("stored", "fused"):
        for r in nan_rows:
            assert np.array_equal(results[name][0][r], results["rounds"][0][r]) and np.array_equal(results[name][1][r], results["rounds"][1][r]), \
                f"{name} against rounds, query {queries[r].tolist()}: documents {results[name][0][r].tolist()} / {results['rounds'][0][r].tolist()}"
    ids, bits, st = results["fused"]
    nan_docs = np.flatnonzero(np.isnan(ref[1]))
    for r in nan_rows:                                                          # the NaN documents first, in document order
        assert ids[r, :7].tolist() == nan_docs.tolist() and np.isnan(bits[r, :7].view(np.float32)).all()
    assert st["rows_redone"] == 4, st                                           # the three NaN rows and NEG + FEW


# ------------------------------------------------------------------------------------------------ g. the round kernels alone
def test_round_kernels_three_batches_and_chunk_edges(monkeypatch):
    """CCR_BM25_TILE=-1, 5 000 documents, 600 queries = three batches of 256 rows on one fp64 accumulator (a cell that is not re-zeroed
    shows in batches 2 and 3); posting lists of 1, 2047, 2048, 2049, 4096 and 4097 postings (BM25_CHUNK = 2048 per block); rounds that
    pair the 4097-posting list with the 1-posting list in both row orders (the grid is sized by the longest pair of the round)."""
    rs = np.random.RandomState(31)
    n_docs = 5000
    sizes = [1, 2047, 2048, 2049, 4096, 4097]
    lists = [np.sort(rs.choice(n_docs, n, replace=False)) for n in sizes]
    lists += [np.sort(rs.choice(n_docs, rs.randint(1, 400), replace=False)) for _ in range(34)]
    indptr, rows, counts = bm25_postings_from_lists([(d, rs.randint(1, 6, len(d))) for d in lists])
    index = (indptr, rows, counts, rs.uniform(0.3, 3.0, n_docs), rs.uniform(0.2, 6.0, len(lists)))
    queries = [np.asarray([t], np.int32) for t in range(6)]
    # round 1 is rows 0 .. 5's single terms: the 1-posting list leads, the 4097-posting list follows; then the other order, and the same
    # pairing among the second terms
    queries += [np.asarray(q, np.int32) for q in ([5], [0], [1, 5], [4, 5], [0, 1], [3, 5])]
    queries += [np.sort(rs.choice(40, rs.randint(1, 7), replace=False)).astype(np.int32) for _ in range(588)]
    assert len(queries) == 600
    ref = bm25_reference_rows(*index, queries, 1.2)
    model = _make(monkeypatch, index, 1.2, tile=-1)
    ids, sc, st = _search(monkeypatch, model, queries, 50, False, ROUNDS, False)
    assert st["batches"] == 3, st
    _same(ids, sc, *bm25_reference_topk(ref, 50), "rounds, three batches")
    ids, sc, _ = _search(monkeypatch, model, queries[:12], 4096, False, ROUNDS, False)          # (nearly) the whole rows of the chunk-edge lists
    _same(ids, sc, *bm25_reference_topk(ref[:12], 4096), "rounds, whole rows")


# ------------------------------------------------------------------------------------------------ h. the contribution table's term lookup
def _table_indices():
    rs = np.random.RandomState(41)
    n_docs = 1500
    long_a, long_b = np.sort(rs.choice(n_docs, 900, replace=False)), np.sort(rs.choice(n_docs, 700, replace=False))
    none, one = np.zeros(0, np.int64), np.asarray([777])
    few = lambda n: np.sort(rs.choice(n_docs, n, replace=False))
    return {"one term": [long_a], "one posting": [one],
            "empties first, doubled, last": [none, none, few(3), none, none, few(300), none, few(2), none, none],
            "one posting between long lists": [long_a, one, long_b],
            "every other term empty": [none if t % 2 else few(1 + 37 * t) for t in range(9)]}


@pytest.mark.parametrize("name", list(_table_indices()))
def test_contribution_table_term_lookup(name, monkeypatch):
    """bm25_contrib_kernel finds a posting's term by a binary search of indptr: one term, empty terms in front, behind and doubled, a term
    of one posting between two long ones.  Single-term queries for EVERY term, the table against CCR_BM25_TABLE=0 against the
    reference: a wrong lookup shows as a neighbour's weight."""
    lists = _table_indices()[name]
    rs = np.random.RandomState(len(lists))
    n_docs = 1500
    indptr, rows, counts = bm25_postings_from_lists([(d, rs.randint(1, 6, len(d))) for d in lists])
    index = (indptr, rows, counts, rs.uniform(0.3, 3.0, n_docs), rs.uniform(0.2, 6.0, len(lists)) * 2.0 ** np.arange(len(lists)))
    queries = [np.asarray([t], np.int32) for t in range(len(lists))] + [np.arange(len(lists), dtype=np.int32)]
    ref = bm25_reference_rows(*index, queries, 1.2)
    for cfg in (0, 4):
        for table in (True, False):
            model = _make(monkeypatch, index, 1.2, tile=cfg, table=table)
            ids, sc, _ = _search(monkeypatch, model, queries, n_docs, True, STORED, table)
            _same(ids, sc, *bm25_reference_topk(ref, n_docs), f"{name}, tile cfg {cfg}, table {table}")
            _fused_vs_reference(monkeypatch, model, queries, 10, ref, table, f"{name}, fused, tile cfg {cfg}, table {table}")
