"""A single-launch main pass that leaves CUs to the caller's side work (CCR_SIDE_CUS; Plan::main_grid, the arrival counter and the gate
kernel behind ccr_search_stream_wait_main_pass).  A search leaves CUs free only when the call was made for the previous fused search on
the device (the hint), so every carved search here is the second of a pair with the call between them.  Parity: ids and score BITS with
8 / 24 / 40 CUs left free equal those on every CU, on each main-pass kernel and kind of plan, and the oracle.  Ordering: side work released
at the beginning of the main pass returns its own bits and leaves the search's unchanged."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DENSE, FUSED = 1, 2
OFFSET = 977
ONE_LAUNCH = {"CCR_PROGRESSIVE": 0, "CCR_NARROW": 0}
SIDES = (8, 24, 40)


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


def _index(D, **kv):
    from ccrec_amd import ops
    with _knobs(**kv):
        return ops.CorpusIndex(D, global_row_offset=OFFSET)


def _hinted_search(index, Q, k, side_stream, flags=FUSED):
    """The search after a search that was followed by the call: the one that may leave CUs free.  The call is made for it as well, so
    that the gate kernel runs against its arrival counter."""
    index.search(Q, k, flags)
    index.stream_wait_main_pass(side_stream)
    s, i = index.search(Q, k, flags)
    index.stream_wait_main_pass(side_stream)
    side_stream.synchronize()
    return s, i, index.last_stats()


def _parity(Db, Qb, k, knobs, check=None, oracle_rows=None):
    """Searches with 8, 24 and 40 CUs left free against the search on every CU (CCR_SIDE_CUS=0): the same ids and score bits; the
    latter against the oracle on `oracle_rows`.  check(stats, index) asserts what kind of plan ran."""
    D, Q = _bf16(Db), _bf16(Qb)
    side_stream = torch.cuda.Stream()
    off = _index(D, CCR_SIDE_CUS=0, **knobs)
    s0, i0, st0 = _hinted_search(off, Q, k, side_stream)
    print("every CU", st0)
    assert st0["path"] == 1 and st0["side_cus"] == 0 and st0["main_grid"] % 8 == 0 and st0["main_launches"] == 1, st0
    if check:
        check(st0, off)
    for side in SIDES:
        on = _index(D, CCR_SIDE_CUS=side, **knobs)
        s, i, st = _hinted_search(on, Q, k, side_stream)
        print("side", side, st)
        assert st["path"] == 1 and st["side_cus"] == side and st["main_grid"] == st0["main_grid"] - side and st["main_launches"] == 1, st
        if check:
            check(st, on)
        assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32)), f"side {side} differs from every CU"
    rows = np.arange(Qb.shape[0]) if oracle_rows is None else oracle_rows
    ref_i, ref_s = orc.canonical_search(Qb[rows], Db, k, None)
    assert np.array_equal(i0.cpu().numpy()[rows] - OFFSET, ref_i)
    assert np.array_equal(s0.cpu().numpy()[rows].view(np.uint32), ref_s.view(np.uint32))
    return st0


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("nq", [400, 1100])
def test_parity_on_the_wide_kernel(nq):
    """300 000 x 256, k = 100: two and three blocks of 384 queries (the last partial), the planner's own ranges at each grid."""
    n, d, k = 300_000, 256, 100
    Db, Qb = _rand_bits(n, d, 301), _rand_bits(nq, d, 300 + nq)
    _parity(Db, Qb, k, dict(ONE_LAUNCH, CCR_WIDE=1), lambda st, ix: st["main_tile_queries"] == 384 or pytest.fail(str(st)),
            np.r_[0:6, nq // 2:nq // 2 + 6, nq - 6:nq])


def test_parity_on_the_256_kernel_at_a_width_that_is_no_multiple_of_32():
    """600 queries (three blocks of 256, the last of 88 rows) at dim 40: the 16x16x32 kernel with a zero-filled last K sub-stage."""
    n, nq, d, k = 30_001, 600, 40, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    _parity(Db, Qb, k, dict(ONE_LAUNCH), lambda st, ix: (st["main_tile_queries"] == 256 and st["sublists"] == 8) or pytest.fail(str(st)),
            np.r_[0:8, 250:262, nq - 8:nq])


def test_parity_with_unequal_query_groups():
    n, nq, d, k = 30_001, 1537, 64, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    _parity(Db, Qb, k, dict(ONE_LAUNCH, CCR_WIDE=1, CCR_QSPLIT=1, CCR_QGROUPS=2), lambda st, ix: ix.last_main_split() == 2 or pytest.fail(str(st)),
            np.r_[0:8, nq - 8:nq])


def test_parity_when_the_sampled_tiles_are_left_out():
    n, nq, d, k = 40_000, 1537, 128, 100
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    _parity(Db, Qb, k, dict(CCR_NARROW=0, CCR_WIDE=1, CCR_OPTIMISTIC=1, CCR_SAMPLE_DIV=8, CCR_SKIP_SAMPLED=1),
            lambda st, ix: (st["opt_rank"] > 0 and st["skipped_tiles"] > 0) or pytest.fail(str(st)), np.r_[0:8, nq - 8:nq])


def test_parity_on_three_tiles_with_more_workgroups_than_items():
    """700 rows = three tiles (the last partial) in eight ranges of one query block: eight items, five of them empty, on 216 .. 256
    workgroups that all count themselves in."""
    n, nq, d, k = 700, 300, 64, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    st = _parity(Db, Qb, k, dict(ONE_LAUNCH), None)
    assert st["ranges"] * ((nq + st["main_tile_queries"] - 1) // st["main_tile_queries"]) < st["main_grid"] - max(SIDES), st


def test_parity_when_flagged_queries_take_the_retry_pass():
    """Clustered rows in cluster order flood the sub-lists of their cluster's queries: the retry pass (every CU, no arrival counter)
    and the dense path finish them -- exact, and the same with and without side CUs."""
    g = torch.Generator().manual_seed(21)
    n, d, nq, k, nc = 60_000, 128, 1537, 100, 20
    centres = torch.randn(nc, d, generator=g)
    lab = torch.arange(n) * nc // n
    D = centres[lab] + 0.05 * torch.randn(n, d, generator=g)
    Q = centres[torch.arange(nq) % nc] + 0.05 * torch.randn(nq, d, generator=g)
    Db, Qb = orc.pack_bf16(D.numpy()), orc.pack_bf16(Q.numpy())
    _parity(Db, Qb, k, dict(ONE_LAUNCH, CCR_WIDE=1, CCR_QGROUPS=2), lambda st, ix: (st["n_fallback"] > 0 and st["n_retried"] + st["n_dense"] > 0) or pytest.fail(str(st)),
            np.r_[0:6, 700:706, nq - 6:nq])


# ---------------------------------------------------------------------------------------------- ordering and the hint
def test_side_work_released_at_the_start_of_the_main_pass_keeps_both_results():
    """A deferred search that leaves 24 CUs free, the call, then a pack of ANOTHER buffer on the side stream (released behind the gate,
    beside the main pass): the pack's bits are those of a pack on the main stream, the search's those of a plain search.  After a
    dense-path search the call returns at once."""
    from ccrec_amd import ops
    n, nq, d, k = 300_000, 400, 256, 100
    Db, Qb = _rand_bits(n, d, 301), _rand_bits(nq, d, 300 + nq)
    D, Q = _bf16(Db), _bf16(Qb)
    index = _index(D, CCR_SIDE_CUS=24, CCR_WIDE=1, **ONE_LAUNCH)
    s0, i0 = index.search(Q, k, FUSED)
    x = torch.randn(200_000, d, device="cuda")
    want = ops.pack_bf16(x)
    side = torch.cuda.Stream()
    out = torch.empty_like(want)
    index.stream_wait_main_pass(side)      # the hint for the search below
    torch.cuda.synchronize()
    s, i = index.search(Q, k, FUSED, defer=True)
    index.stream_wait_main_pass(side)
    with torch.cuda.stream(side):
        ops.pack_bf16(x, out=out)
    torch.cuda.current_stream().wait_stream(side)
    index.finish()
    torch.cuda.synchronize()
    st = index.last_stats()
    assert st["path"] == 1 and st["side_cus"] == 24, st
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    index.search(Q[:3], k, DENSE)
    assert index.last_stats()["side_cus"] == 0
    index.stream_wait_main_pass(side)       # dense path: nothing recorded, returns at once
    side.synchronize()


def test_only_a_search_that_follows_the_call_leaves_cus_free():
    """The hint rule: side_cus is 0 for a first search and for a search not preceded by the call, 16 (pinned: the planner's own
    choice is for shapes whose main pass can hide a pack) for the search after a call."""
    n, nq, d, k = 30_001, 600, 64, 10
    Db, Qb = _rand_bits(n, d, n + 3), _rand_bits(nq, d, nq + 5)
    D, Q = _bf16(Db), _bf16(Qb)
    side = torch.cuda.Stream()
    index = _index(D, CCR_SIDE_CUS=16, **ONE_LAUNCH)
    index.search(Q[:2], k, DENSE)            # takes whatever hint an earlier test left on the device
    s0, i0 = index.search(Q, k, FUSED)
    assert index.last_stats()["path"] == 1 and index.last_stats()["side_cus"] == 0
    index.stream_wait_main_pass(side)
    s1, i1 = index.search(Q, k, FUSED)
    st = index.last_stats()
    assert st["side_cus"] == 16 and st["main_grid"] % 8 == 0, st
    s2, i2 = index.search(Q, k, FUSED)       # no call since: every CU again
    assert index.last_stats()["side_cus"] == 0
    side.synchronize()
    for s, i in ((s1, i1), (s2, i2)):
        assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
