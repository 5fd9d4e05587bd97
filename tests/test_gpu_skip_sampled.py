"""The main pass that leaves out the sampled tiles (CCR_SKIP_SAMPLED; single launch under estimated thresholds) and the select stage
that joins their rows from the sample pass's group maxima: exact against the oracle on each of the three main-pass kernels, bit-equal
to the search that scores every tile, exact when the whole top-k sits in sampled tiles, on ties between a sampled and an unsampled
row and with a whole sampled tile above everything else, and through the packed shard message of a 2-rank search.  Every case pins the
knobs and asserts the statistics of the path it means to take."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = 2
OFFSET = 4321
SKIP = {"CCR_SKIP_SAMPLED": 1, "CCR_OPTIMISTIC": 1, "CCR_NARROW": 0}


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()


def _rand_bits(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return orc.pack_bf16((torch.randn(n, d, generator=g) * d ** -0.5).numpy())


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


def _index(Db, **kv):
    from ccrec_amd import ops
    with _knobs(**kv):
        return ops.CorpusIndex(_bf16(Db), global_row_offset=OFFSET)


def _assert_skipped(st, **more):
    """The path the case means to take: fused, ONE launch under estimated thresholds, the sampled tiles left out."""
    assert st["path"] == 1 and st["opt_rank"] > 0 and st["main_launches"] == 1 and st["skipped_tiles"] > 0, st
    assert st["skipped_tiles"] == st["sample_tiles"], st
    for key, want in more.items():
        assert st[key] == want, (key, st)


def _assert_oracle(s, i, Qb, Db, k, offset=OFFSET):
    ref_i, ref_s = orc.canonical_search(Qb, Db, k, None)
    got_i = i.cpu().numpy() - offset
    assert np.array_equal(got_i, ref_i), f"ids differ in {np.sum(got_i != ref_i)} places (queries {np.unique(np.nonzero(got_i != ref_i)[0])[:10]})"
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("n,nq,d,k", [
    (20_001, 300, 64, 10),   # 79 tiles, ten sampled at stride 7: both branches of the tile map, the partial last tile in the second
    (20_001, 130, 32, 5),    # one K step per tile
])
def test_skip_sampled_equals_the_oracle(n, nq, d, k):
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    index = _index(Db, CCR_SAMPLE_DIV=8, **SKIP)
    s, i = index.search(_bf16(Qb), k, FUSED)
    st = index.last_stats()
    print(st)
    _assert_skipped(st, skipped_tiles=10)
    assert (n // 256) // st["sample_tiles"] == 7   # the sample stride: virtual tiles 0 .. 59 sit between sampled tiles, 60 .. 68 behind them
    _assert_oracle(s, i, Qb, Db, k)


_wide_case = {}


def _wide_case_data():
    """(40 000, 700, 768, 100): the corpus, the queries and the oracle's answer, computed once for the three kernels."""
    if not _wide_case:
        n, nq, d, k = 40_000, 700, 768, 100
        Db, Qb = _rand_bits(n, d, 40_003), _rand_bits(nq, d, 705)
        _wide_case.update(Db=Db, Qb=Qb, k=k, ref=orc.canonical_search(Qb, Db, k, None))
    return _wide_case


@pytest.mark.parametrize("kernel,knobs,tile_queries,sublists", [
    ("256 x 384, 16x16x32", {"CCR_WIDE": 1}, 384, 8),
    ("256 x 256, 16x16x32", {"CCR_WIDE": 0}, 256, 8),
    ("256 x 256, 32x32x16", {"CCR_WIDE": 0, "CCR_MFMA16": 0}, 256, 4),
])
def test_skip_sampled_on_each_main_pass_kernel(kernel, knobs, tile_queries, sublists):
    c = _wide_case_data()
    index = _index(c["Db"], CCR_SAMPLE_DIV=8, **SKIP, **knobs)
    s, i = index.search(_bf16(c["Qb"]), c["k"], FUSED)
    st = index.last_stats()
    print(kernel, st)
    _assert_skipped(st, main_tile_queries=tile_queries, sublists=sublists, skipped_tiles=20)
    ref_i, ref_s = c["ref"]
    assert np.array_equal(i.cpu().numpy() - OFFSET, ref_i)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. skip on against skip off
@pytest.mark.parametrize("defer", [False, True], ids=["sync", "deferred"])
@pytest.mark.parametrize("n,nq,d,k", [
    (300_000, 1100, 256, 1001),   # the 1 024-thread select, at the planner's own plan
    (250_003, 3452, 128, 100),    # nine query blocks
])
def test_skip_sampled_is_bit_equal_to_scoring_every_tile(n, nq, d, k, defer):
    Db, Qb = _rand_bits(n, d, n + 11), _rand_bits(nq, d, nq + 13)
    Q = _bf16(Qb)
    on = _index(Db, **SKIP)
    off = _index(Db, **dict(SKIP, CCR_SKIP_SAMPLED=0))
    s, i = on.search(Q, k, FUSED, defer=defer)
    if defer:
        on.finish()
    st = on.last_stats()
    print(st)
    _assert_skipped(st)
    s0, i0 = off.search(Q, k, FUSED, defer=defer)
    if defer:
        off.finish()
    st0 = off.last_stats()
    print(st0)
    assert st0["path"] == 1 and st0["opt_rank"] > 0 and st0["main_launches"] == 1 and st0["skipped_tiles"] == 0, st0
    assert st0["sample_tiles"] == st["sample_tiles"] and st0["main_tile_queries"] == st["main_tile_queries"]
    differ = torch.nonzero((i != i0).any(dim=1) | (s.view(torch.int32) != s0.view(torch.int32)).any(dim=1)).flatten()
    print("queries that differ:", differ.numel(), differ[:10].tolist())
    for q in differ[:3].tolist():
        only_off = sorted(set(i0[q].tolist()) - set(i[q].tolist()))
        print(" query", q, "rows only without the skip (row, tile, row in tile):", [(r - OFFSET, (r - OFFSET) // 256, (r - OFFSET) % 256) for r in only_off],
              "only with it:", sorted(r - OFFSET for r in set(i[q].tolist()) - set(i0[q].tolist())))
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 3. planted rows
def test_skip_sampled_with_planted_rows_in_the_sampled_tiles():
    """Queries 0-4: k + 5 scaled copies of the query in rows of SAMPLED tiles only -- the whole top-k comes from the join.  Queries 5-9:
    exact duplicates, one copy in a sampled and one in an unsampled tile, the k-th place falling inside a pair -- the tie order.  Query
    10: one whole sampled tile (256 rows) above everything else -- the collected rows hold it beside the regular ones (no flag)."""
    n, nq, d, k, div = 20_001, 300, 64, 10, 8
    g = torch.Generator().manual_seed(77)
    D = (torch.randn(n, d, generator=g) * d ** -0.5).numpy()
    Qf = (torch.randn(nq, d, generator=g) * d ** -0.5).numpy()
    # the sampled tiles, from the statistics of a search with the same knobs (the plan depends on the shape only)
    probe = _index(orc.pack_bf16(D), CCR_SAMPLE_DIV=div, **SKIP)
    probe.search(_bf16(orc.pack_bf16(Qf)), k, FUSED)
    st = probe.last_stats()
    _assert_skipped(st)
    stride = (n // 256) // st["sample_tiles"]
    sampled = [j * stride for j in range(st["sample_tiles"])]
    unsampled = [t for t in range(n // 256) if t not in sampled]
    assert stride >= 2 and len(sampled) >= 6
    hot = sampled[2]                                   # query 10's tile: nothing else is planted there
    pool = [t for t in sampled if t != hot]
    rs = np.random.RandomState(5)
    used = set()

    def free_row(tiles):
        while True:
            row = int(tiles[rs.randint(len(tiles))]) * 256 + int(rs.randint(256))
            if row not in used:
                used.add(row)
                return row

    edge_rows = [0, 255, 3, 4, 8, 27, 28, 127, 128, 131, 224, 251]   # first and last rows of the tile, of a 16-row group, of a wave's half
    for q in range(5):
        for c in range(k + 5):
            row = pool[(q + c) % len(pool)] * 256 + edge_rows[(3 * q + c) % len(edge_rows)]
            if row in used:
                row = free_row(pool)
            used.add(row)
            D[row] = Qf[q] * (2.0 + 0.125 * c)
    for q in range(5, 10):
        D[free_row(pool if q % 2 else unsampled)] = Qf[q] * 4.0           # one row on top
        for c in range(6):                                                  # pairs: places 2-3, 4-5, 6-7, 8-9, 10-11: the cut splits a pair
            a, b = free_row(pool), free_row(unsampled)
            D[a] = D[b] = Qf[q] * (3.5 - 0.25 * c)
    assert all(r // 256 != hot for r in used)
    D[hot * 256:(hot + 1) * 256] = 3.0 * Qf[10] + 0.3 * D[hot * 256:(hot + 1) * 256]
    Db, Qb = orc.pack_bf16(D), orc.pack_bf16(Qf)
    index = _index(Db, CCR_SAMPLE_DIV=div, **SKIP)
    s, i = index.search(_bf16(Qb), k, FUSED)
    st = index.last_stats()
    print("n_fallback", st["n_fallback"], st)
    _assert_skipped(st, skipped_tiles=len(sampled))
    _assert_oracle(s, i, Qb, Db, k)
    ids = i.cpu().numpy() - OFFSET
    tiles_of = ids // 256
    assert np.isin(tiles_of[:5], sampled).all()            # the whole top-k of queries 0-4 came from the join
    assert (tiles_of[10] == hot).all()
    both = np.isin(tiles_of[5:10], sampled)
    assert both.any() and not both.all()
    # the hot-tile query alone: nothing is flagged
    s1, i1 = index.search(_bf16(Qb[10:11]), k, FUSED)
    st1 = index.last_stats()
    print("hot tile alone: n_fallback", st1["n_fallback"], st1)
    _assert_skipped(st1, n_fallback=0)
    _assert_oracle(s1, i1, Qb[10:11], Db, k)


def test_skip_sampled_walks_the_column_when_the_short_list_overflows():
    """The threshold kernel hands the select a short list of the sampled groups that reach tau (2 * opt_rank + 30 entries at most).  One
    planted row for query 0 in each of 128 sampled groups, 123 of them equal, overflows it: the select walks the query's whole column of group maxima instead.
    Twelve stronger rows in unsampled tiles set L, five of the sampled rows are stronger still: they come from the join."""
    n, nq, d, k, div = 20_001, 300, 64, 10, 8
    g = torch.Generator().manual_seed(78)
    D = (torch.randn(n, d, generator=g) * d ** -0.5).numpy()
    Qf = (torch.randn(nq, d, generator=g) * d ** -0.5).numpy()
    stride, n_sampled = (n // 256) // 10, 10
    rows = [j * stride * 256 + 16 * grp + 5 for j in range(8) for grp in range(16)]   # row 5 of 128 different 16-row blocks = 128 groups
    for c, row in enumerate(rows):
        D[row] = Qf[0] * (5.0 + 0.125 * (c % 5) if c % 26 == 0 else 2.0)   # (the 123 equal rows tie at tau: all their groups reach it)
    unsampled = [t for t in range(n // 256) if t % stride or t // stride >= n_sampled]
    for c in range(12):
        D[unsampled[5 * c] * 256 + 17 * c] = Qf[0] * (3.0 + 0.0625 * c)
    Db, Qb = orc.pack_bf16(D), orc.pack_bf16(Qf)
    index = _index(Db, CCR_SAMPLE_DIV=div, **SKIP)
    s, i = index.search(_bf16(Qb), k, FUSED)
    st = index.last_stats()
    print("n_fallback", st["n_fallback"], st)
    _assert_skipped(st, skipped_tiles=n_sampled)
    assert 2 * st["opt_rank"] + 30 < 128              # the list cannot hold query 0's groups
    _assert_oracle(s, i, Qb, Db, k)
    top = (i.cpu().numpy()[0] - OFFSET)
    assert np.isin(top[:5], rows).all() and not np.isin(top[5:], rows).any()
    s1, i1 = index.search(_bf16(Qb[:1]), k, FUSED)    # alone (the small batch's threshold kernel writes the list): not flagged
    st1 = index.last_stats()
    print("alone: n_fallback", st1["n_fallback"])
    _assert_skipped(st1, n_fallback=0)
    _assert_oracle(s1, i1, Qb[:1], Db, k)


# ---------------------------------------------------------------------------------------------- 4. the packed shard message
def _shard_rank_worker(rank, world, port, out_dir):
    """Two processes on this GPU over gloo: each searches its shard with the sampled tiles left out and writes the packed shard
    message (ccr_search_shard); the merged lists equal the oracle's over the whole corpus."""
    import torch.distributed as dist
    sys.path[:0] = [ROOT, os.path.join(ROOT, "crowd-coachable-recommendations_amd")]
    from oracle import oracle as orc
    from ccrec_amd import ops
    from ccrec_amd.dist import shard_bounds, submit_sharded_search
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    n, d, k, nq = 40_002, 64, 10, 300
    Db, Qb = _rand_bits(n, d, 91), _rand_bits(nq, d, 92)
    lo, hi = shard_bounds(n, world, rank)
    os.environ.update({key: str(v) for key, v in dict(SKIP, CCR_SAMPLE_DIV=8).items()})
    index = ops.CorpusIndex(_bf16(Db[lo:hi]), global_row_offset=lo)
    ex = submit_sharded_search(index, _bf16(Qb), k)
    s, i = ex.result()
    st = index.last_stats()
    ref_i, ref_s = orc.canonical_search(Qb, Db, k, None)
    ok = np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))
    took = st["path"] == 1 and st["opt_rank"] > 0 and st["main_launches"] == 1 and st["skipped_tiles"] > 0
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if ok and took else f"MISMATCH ok={ok} took={took} {st}")
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def test_skip_sampled_through_the_shard_message_of_two_ranks(tmp_path):
    import torch.multiprocessing as mp
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    mp.spawn(_shard_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"
