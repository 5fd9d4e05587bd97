"""The tile epilogue of the 256 x 384 main pass (gemm_topk16w_kernel, CCR_WIDE=1) keeps a lane's six sub-list counters in registers
for the length of a tile: several records per lane and query tile, a sub-list that runs past its capacity, the last valid row of a
one-row last tile, and every lane of every wave recording in the same tile.  A query's hits are exact copies of twice its own row
(a power of two: exact in bf16), which beat every random row.  Every case is compared with the oracle bit for bit, and its
n_candidates with the 256 x 256 kernel's on the same plan (CCR_WIDE=0 CCR_MFMA16=1: the same ranges, sub-lists and capacity)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FUSED = 2
OFFSET = 4321
NQ, K = 385, 10            # two query blocks, the second of one row
TILES, RANGES = 40, 8      # range r owns the tiles r, r + 8, ...


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()


_bits = {}


def _rand_bits(n, d, seed):
    """Seeded bf16 rows, made once per shape and left unchanged (the cases copy them)."""
    if (n, d, seed) not in _bits:
        g = torch.Generator().manual_seed(seed)
        _bits[(n, d, seed)] = orc.pack_bf16((torch.randn(n, d, generator=g) * d ** -0.5).numpy())
    return _bits[(n, d, seed)]


def _twice(row_bits):
    """2 x a bf16 row: one more in the exponent field (the rows are normal numbers far from overflow)."""
    return (row_bits + np.uint16(0x0080)).astype(np.uint16)


@contextmanager
def _knobs(**kv):
    """Environment knobs are read ONCE, when an index is created."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _search(Db, Qb, **kv):
    from ccrec_amd import ops
    with _knobs(CCR_NARROW=0, **kv):
        index = ops.CorpusIndex(_bf16(Db), global_row_offset=OFFSET)
    s, i = index.search(_bf16(Qb), K, FUSED)
    return s, i, index.last_stats()


def _check(Db, Qb, want_overflow=False):
    s, i, st = _search(Db, Qb, CCR_WIDE=1)
    print("wide", st)
    assert st["path"] == 1 and st["main_tile_queries"] == 384 and st["main_launches"] == 1 and st["ranges"] == RANGES, st
    ref_i, ref_s = orc.canonical_search(Qb, Db, K, None)
    got = i.cpu().numpy() - OFFSET
    assert np.array_equal(got, ref_i), f"ids differ in {np.sum(got != ref_i)} places"
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))
    s0, i0, st0 = _search(Db, Qb, CCR_WIDE=0, CCR_MFMA16=1)
    print("256 ", st0)
    assert st0["path"] == 1 and st0["main_tile_queries"] == 256 and (st0["ranges"], st0["sublists"], st0["cap"]) == (st["ranges"], st["sublists"], st["cap"])
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    assert st["n_candidates"] == st0["n_candidates"], (st["n_candidates"], st0["n_candidates"])
    if want_overflow:
        assert st["n_fallback"] > 0 and st["n_retried"] + st["n_dense"] > 0, st
    return st


@pytest.mark.parametrize("d", [32, 96], ids=["one K step", "three K steps"])
def test_several_records_per_lane_and_query_tile(d):
    """40 copies of the best row of query 5 in the rows 100 .. 139 of tile 3 (both halves of the tile's rows): five records per
    sub-list, all of one tile."""
    n = TILES * 256 - 34
    Db, Qb = _rand_bits(n, d, n + 3).copy(), _rand_bits(NQ, d, NQ + 5)
    Db[3 * 256 + 100:3 * 256 + 140] = _twice(Qb[5])
    st = _check(Db, Qb)
    assert st["n_fallback"] == 0, st


@pytest.mark.parametrize("d", [32, 96], ids=["one K step", "three K steps"])
def test_a_sub_list_past_its_capacity_flags_the_query(d):
    """300 copies: the rows 0 .. 99 of the tiles 3, 11 and 19 -- one range, 75 rows for each of its first four sub-lists of query 5,
    more than they hold.  The count keeps running past the capacity, the select flags the query and the retry or the dense path
    answers it exactly."""
    n = TILES * 256 - 34
    Db, Qb = _rand_bits(n, d, n + 3).copy(), _rand_bits(NQ, d, NQ + 5)
    for t in (3, 3 + RANGES, 3 + 2 * RANGES):
        Db[t * 256:t * 256 + 100] = _twice(Qb[5])
    st = _check(Db, Qb, want_overflow=True)
    assert st["cap"] < 75, st


@pytest.mark.parametrize("d", [32, 96], ids=["one K step", "three K steps"])
def test_the_last_valid_row_of_a_one_row_tile(d):
    """The last tile holds ONE row, the best of the only query of the partly filled last block (and of query 0): it is recorded, the
    255 copies of it that the tile's padding re-reads are not (their ids would lie beyond the corpus)."""
    n = TILES * 256 + 1
    Db, Qb = _rand_bits(n, d, n + 3).copy(), _rand_bits(NQ, d, NQ + 5).copy()
    Qb[0] = Qb[NQ - 1]
    Db[n - 1] = _twice(Qb[NQ - 1])
    Db[n - 2] = _twice(Qb[NQ - 1])     # and the last row of the last whole tile
    st = _check(Db, Qb)
    assert st["n_fallback"] == 0, st


@pytest.mark.parametrize("d", [32, 96], ids=["one K step", "three K steps"])
def test_every_lane_of_every_wave_records_in_the_same_tile(d):
    """All 385 queries are the same row, 40 copies of its best row lie in one tile: every cell of both blocks takes five records there."""
    n = TILES * 256 - 34
    Db = _rand_bits(n, d, n + 3).copy()
    Qb = np.repeat(_rand_bits(NQ, d, NQ + 5)[7:8], NQ, axis=0)
    Db[21 * 256 + 100:21 * 256 + 140] = _twice(Qb[0])
    st = _check(Db, Qb)
    assert st["n_fallback"] == 0, st
