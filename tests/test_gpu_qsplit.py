"""Unequal query groups of a single-launch main pass (CCR_QSPLIT; ccr::main_item): G = 2, 4 or 8 groups over the XCDs that do not
divide the count of query blocks -- each keeps its whole blocks, the left-over blocks are shared range by range.  Every case runs the
search with the split pinned (CCR_QSPLIT=1) and with equal groups (CCR_QSPLIT=0) on the same build and compares ids and score BITS,
asserts the groups the search reports (ccr_search_last_main_split), and at least one case per main-pass kernel is checked against the
oracle."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FUSED = 2
OFFSET = 4321
ONE_LAUNCH = {"CCR_PROGRESSIVE": 0, "CCR_NARROW": 0}


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()


_bits = {}


def _rand_bits(n, d, seed):
    """Seeded bf16 rows, made once per shape and left unchanged."""
    if (n, d, seed) not in _bits:
        g = torch.Generator().manual_seed(seed)
        _bits[(n, d, seed)] = orc.pack_bf16((torch.randn(n, d, generator=g) * d ** -0.5).numpy())
    return _bits[(n, d, seed)]


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


def _split_and_equal(Db, Qb, k, want_g, knobs, tile_queries):
    """The search with the split pinned and with equal groups: the same ids and score bits; returns the split search's results."""
    Q = _bf16(Qb)
    on = _index(Db, CCR_QSPLIT=1, **knobs)
    s, i = on.search(Q, k, FUSED)
    st = on.last_stats()
    print("split", on.last_main_split(), st)
    assert st["path"] == 1 and st["main_launches"] == 1 and st["main_tile_queries"] == tile_queries, st
    assert on.last_main_split() == want_g
    off = _index(Db, CCR_QSPLIT=0, **knobs)
    s0, i0 = off.search(Q, k, FUSED)
    st0 = off.last_stats()
    assert st0["path"] == 1 and st0["main_launches"] == 1 and st0["main_tile_queries"] == tile_queries and off.last_main_split() == 0, st0
    assert st0["ranges"] == st["ranges"] and st0["skipped_tiles"] == st["skipped_tiles"]
    differ = torch.nonzero((i != i0).any(dim=1) | (s.view(torch.int32) != s0.view(torch.int32)).any(dim=1)).flatten()
    print("queries that differ:", differ.numel(), differ[:10].tolist())
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    return s, i, st


def _assert_oracle(s, i, Qb, Db, k, sub=None):
    sub = np.arange(Qb.shape[0]) if sub is None else sub
    ref_i, ref_s = orc.canonical_search(Qb[sub], Db, k, None)
    got_i = i.cpu().numpy()[sub] - OFFSET
    assert np.array_equal(got_i, ref_i), f"ids differ in {np.sum(got_i != ref_i)} places"
    assert np.array_equal(s.cpu().numpy()[sub].view(np.uint32), ref_s.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the 256 x 384 kernel
@pytest.mark.parametrize("nq,g,n,d,k,oracle", [
    (1537, 2, 30_001, 64, 10, True),     # five blocks, the last of one row: base 2, rem 1
    (1537, 4, 30_001, 64, 100, False),   # base 1, rem 1
    (3077, 2, 20_001, 64, 10, False),    # nine blocks, the last holding five queries: base 4, rem 1
    (3077, 8, 20_001, 64, 10, False),    # base 1, rem 1
    (3841, 4, 20_001, 128, 10, False),   # eleven blocks: base 2, rem 3
    (1153, 8, 40_000, 128, 100, True),   # four blocks in eight groups: base 0, every block shared
])
def test_split_groups_on_the_wide_tile(nq, g, n, d, k, oracle):
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    s, i, st = _split_and_equal(Db, Qb, k, g, dict(ONE_LAUNCH, CCR_WIDE=1, CCR_QGROUPS=g), 384)
    if oracle:
        _assert_oracle(s, i, Qb, Db, k, np.r_[0:8, nq // 2:nq // 2 + 8, nq - 8:nq])


# ---------------------------------------------------------------------------------------------- the 256 x 256 kernels
@pytest.mark.parametrize("mfma16,sublists", [(1, 8), (0, 4)], ids=["16x16x32", "32x32x16"])
def test_split_groups_on_the_256_tile(mfma16, sublists):
    """1 025 queries = five blocks of 256, the last of one row; the pinned split's own choice is G = 2 (no CCR_QGROUPS)."""
    n, nq, d, k = 30_001, 1025, 64, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    s, i, st = _split_and_equal(Db, Qb, k, 2, dict(ONE_LAUNCH, CCR_WIDE=0, CCR_MFMA16=mfma16), 256)
    assert st["sublists"] == sublists
    _assert_oracle(s, i, Qb, Db, k, np.r_[0:8, 508:516, nq - 8:nq])


# ---------------------------------------------------------------------------------------------- tile counts and the skip
def test_split_groups_with_fewer_tiles_than_ranges():
    """Six corpus tiles (the last partial) in eight ranges: ranges without a tile, items with nothing to do."""
    n, nq, d, k = 1_400, 1537, 64, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    s, i, st = _split_and_equal(Db, Qb, k, 2, dict(ONE_LAUNCH, CCR_WIDE=1, CCR_QGROUPS=2), 384)
    assert st["ranges"] > (n + 255) // 256, st
    _assert_oracle(s, i, Qb, Db, k)


@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "every tile"])
def test_split_groups_with_and_without_the_skip_of_the_sampled_tiles(skip):
    """Estimated thresholds on a 1/8 sample: with the skip the launch walks the unsampled tiles only (the map's tile counts are those
    of the virtual tiles)."""
    n, nq, d, k = 40_000, 1537, 128, 100
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    knobs = dict(CCR_NARROW=0, CCR_WIDE=1, CCR_QGROUPS=4, CCR_OPTIMISTIC=1, CCR_SAMPLE_DIV=8, CCR_SKIP_SAMPLED=skip)
    s, i, st = _split_and_equal(Db, Qb, k, 4, knobs, 384)
    assert st["opt_rank"] > 0 and (st["skipped_tiles"] > 0) == bool(skip), st
    _assert_oracle(s, i, Qb, Db, k, np.r_[0:8, nq - 8:nq])


# ---------------------------------------------------------------------------------------------- the retry pass
def test_split_groups_when_flagged_queries_take_the_retry_pass():
    """Clustered rows in cluster order flood the sub-lists of the queries of their cluster: overflowing lists flag the query, the
    retry pass (equal groups, 256 x 256 tiles) and the dense path finish it -- exact, and the same as with equal groups."""
    g = torch.Generator().manual_seed(21)
    n, d, nq, k, nc = 60_000, 128, 1537, 100, 20
    centres = torch.randn(nc, d, generator=g)
    lab = torch.arange(n) * nc // n                      # rows sorted by cluster
    D = centres[lab] + 0.05 * torch.randn(n, d, generator=g)
    Q = centres[torch.arange(nq) % nc] + 0.05 * torch.randn(nq, d, generator=g)
    Db, Qb = orc.pack_bf16(D.numpy()), orc.pack_bf16(Q.numpy())
    s, i, st = _split_and_equal(Db, Qb, k, 2, dict(ONE_LAUNCH, CCR_WIDE=1, CCR_QGROUPS=2), 384)
    assert st["n_fallback"] > 0 and st["n_retried"] + st["n_dense"] > 0, st
    _assert_oracle(s, i, Qb, Db, k, np.r_[0:6, 700:706, nq - 6:nq])
