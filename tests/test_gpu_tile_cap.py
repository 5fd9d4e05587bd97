"""The tile cap of estimated thresholds (csrc/ccr_threshold.hip, csrc/ccr_plan.hip: optimistic_rank): tau_q is the rank-th largest lower
bound among the sampled groups that are among the `cap` largest of their own sampled tile.

* The thresholds the three kernel forms write (small-batch, 16 and 64 group phases) are read back from the head of the search workspace
  (SearchWs in csrc/ccr_plan.h: qnorm, thr, cq -- nq_pad floats each) and compared BIT FOR BIT with a numpy selection over the score
  rows of ccr_scores, at caps 1, 4 and 16.  Integer-valued rows make every MFMA score exact, so the score rows ARE the sample pass's
  values; one sampled tile holds sixteen groups with EQUAL maxima for query 0 (a rule without the tie order would count all sixteen).
  A batch of 48 queries always takes the small-batch kernel (launch_threshold: at most 128 queries), so the two phase counts run on 144.
* A query whose whole cluster is one sampled tile: rank 13 without a cap is settled by that tile alone and the query fails the select's
  check; rank 17 under cap 4 flags nobody.  Both searches return the oracle's lists.
* Ids and score bits equal the exact dense path on gaussian, clustered and topically sorted rows, on both main-pass tiles."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DENSE, FUSED = 1, 2
DIM = 64
TILE = 256
# rows of group gi inside its 256-row tile (the sample pass's epilogue, csrc/ccr_select.hip: wave row, MFMA tile, lane half)
GROUP_ROWS = np.array([[(gi >> 3) * 128 + ((gi >> 1) & 3) * 32 + (gi & 1) * 4 + (e & 3) + 8 * (e >> 2) for e in range(16)] for gi in range(16)])
assert sorted(GROUP_ROWS.ravel().tolist()) == list(range(TILE))


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()


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


def _index(D, norm_bounds=None, **kv):
    from ccrec_amd import ops
    with _knobs(**kv):
        return ops.CorpusIndex(D, norm_bounds=norm_bounds)


# ------------------------------------------------------------------------------------------------ thresholds, bit for bit
N_THR, NQ_THR, K_THR = 16_640, 144, 10        # 65 full tiles; CCR_SAMPLE_DIV=4 under a forced fused search: 17 sampled tiles, stride 3
SAMPLE, STRIDE, RANK = 17, 3, 17
TIE_TILE = 2 * STRIDE                         # the third sampled tile
_thr = {}


def _thr_case():
    """Integer rows (every product and sum exact in fp32), made once: the corpus, 144 queries, the exact score rows, the row-norm
    bounds the index is given (so that the tile norms are known exactly) and the oracle's lists for both batch sizes."""
    if not _thr:
        rs = np.random.RandomState(20)
        D = rs.randint(-8, 9, size=(N_THR, DIM)).astype(np.float32)
        Q = rs.randint(-8, 9, size=(NQ_THR, DIM)).astype(np.float32)
        D[TIE_TILE * TILE + GROUP_ROWS[np.arange(16), np.arange(16)]] = Q[0]      # one row per group scores |q0|^2 for query 0: 16 equal maxima
        Db, Qb = orc.pack_bf16(D), orc.pack_bf16(Q)
        bounds = (np.sqrt((D.astype(np.float64) ** 2).sum(1)) * 1.0001).astype(np.float32)
        from ccrec_amd import ops
        index = ops.CorpusIndex(_bf16(Db))
        scores = index.scores(_bf16(Qb), "mfma").cpu().numpy()
        assert np.array_equal(scores, Q.astype(np.float64) @ D.astype(np.float64).T), "the premise: exact MFMA scores"
        g = scores[0].reshape(-1, TILE)[TIE_TILE][GROUP_ROWS].max(-1)
        assert np.all(g == g[0]) and g[0] == scores[0].max(), "the premise: sixteen equal group maxima on top for query 0"
        _thr.update(Db=Db, Qb=Qb, bounds=bounds, scores=scores,
                    tile_norm=bounds.reshape(-1, TILE).max(1)[np.arange(SAMPLE) * STRIDE],
                    ref={nq: orc.canonical_search(Qb[:nq], Db, K_THR, None) for nq in (48, NQ_THR)})
    return _thr


def _capped_tau(scores, tile_norm, c, rank, cap):
    """The reference: lower bounds fmaf(-c, tile norm, group maximum) of the sampled groups; inside a tile the larger value ranks first
    and on equal values the lower group index; the rank-th largest among the groups of in-tile rank < cap."""
    nq = scores.shape[0]
    tiles = scores.reshape(nq, -1, TILE)[:, np.arange(SAMPLE) * STRIDE]
    gmax = tiles[:, :, GROUP_ROWS].max(-1).astype(np.float64)                                    # [nq, sample, 16]
    low = (-c.astype(np.float64)[:, None, None] * tile_norm.astype(np.float64)[None, :, None] + gmax).astype(np.float32)   # (the product is exact in fp64)
    order = np.argsort(-low, axis=-1, kind="stable")
    kept = np.take_along_axis(low, order[..., :cap], -1).reshape(nq, -1)
    return -np.sort(-kept, axis=1)[:, rank - 1]


@pytest.mark.parametrize("cap", [1, 4, 16])
@pytest.mark.parametrize("form", ["small", 16, 64])
def test_thresholds_equal_the_capped_selection_bit_for_bit(form, cap):
    t = _thr_case()
    nq = 48 if form == "small" else NQ_THR
    knobs = dict(CCR_NARROW=0, CCR_WIDE=0, CCR_OPTIMISTIC=1, CCR_SAMPLE_DIV=4, CCR_SKIP_SAMPLED=0, CCR_OPT_RANK=RANK, CCR_TILE_CAP=cap)
    if form != "small":
        knobs["CCR_THR_PHASES"] = form
    index = _index(_bf16(t["Db"]), norm_bounds=torch.from_numpy(t["bounds"]).cuda(), **knobs)
    s, i = index.search(_bf16(t["Qb"][:nq]), K_THR, FUSED)
    st = index.last_stats()
    print(form, cap, st)
    assert st["path"] == 1 and st["main_launches"] == 1 and st["sample_tiles"] == SAMPLE and st["skipped_tiles"] == 0, st
    assert st["opt_rank"] == RANK and st["tile_cap"] == cap and st["n_fallback"] == 0, st
    assert index.last_threshold_phases() == (0 if form == "small" else form)
    head = index.workspace.view(torch.float32)[:3 * 256].cpu().numpy()        # nq_pad = 256: qnorm, thr, cq
    thr, cq = head[256:256 + nq], head[512:512 + nq]
    want = _capped_tau(t["scores"][:nq], t["tile_norm"], cq, RANK, cap)
    print("thr[:4]", thr[:4], "reference", want[:4], "differ in", int(np.sum(thr.view(np.uint32) != want.view(np.uint32))))
    assert np.array_equal(thr.view(np.uint32), want.view(np.uint32))
    assert st["n_candidates"] == int((t["scores"][:nq] >= want[:, None]).sum()), st       # what the main pass recorded under them
    ref_i, ref_s = t["ref"][nq]
    assert np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


def test_the_cap_changes_the_threshold_of_the_tied_tile():
    """The reference itself tells the caps apart on query 0 (sixteen equal group maxima on top): all sixteen count without a cap,
    four under cap 4, one under cap 1 -- so the bit-for-bit cases above cannot pass with the wrong number of them counted."""
    t = _thr_case()
    c = np.full(1, 1e-5, np.float32)
    taus = [float(_capped_tau(t["scores"][:1], t["tile_norm"], c, RANK, cap)[0]) for cap in (1, 4, 16)]
    assert taus[0] < taus[1] < taus[2], taus


# ------------------------------------------------------------------------------------------------ the adversarial sample
def test_a_cluster_inside_one_sampled_tile_fails_rank_13_uncapped_and_passes_rank_17_capped():
    n, dim, nq, k, div, sampled = 40 * TILE, 256, 144, 10, 4, 10          # every fourth of 40 tiles
    g = torch.Generator().manual_seed(31)
    D = torch.randn(n, dim, generator=g) * dim ** -0.5
    Q = torch.linalg.qr(torch.randn(dim, nq, generator=g))[0].T.contiguous()      # orthonormal query rows: query 0's cluster is noise for the others
    tile = 2 * 4                                     # a sampled tile: all of its rows are query 0's cluster, no other row is
    D[tile * TILE:(tile + 1) * TILE] = 3.0 * Q[0] + 0.05 * D[tile * TILE:(tile + 1) * TILE]
    Db, Qb = orc.pack_bf16(D.numpy()), orc.pack_bf16(Q.numpy())
    ref_i, ref_s = orc.canonical_search(Qb, Db, k, None)
    assert np.all(ref_i[0] // TILE == tile)
    # the main pass leaves out the sampled tiles: no recorded row of query 0 reaches a threshold that the cluster tile sets alone
    plan = dict(CCR_NARROW=0, CCR_OPTIMISTIC=1, CCR_SAMPLE_DIV=div, CCR_SKIP_SAMPLED=1)
    for rank, cap, flagged in ((13, 16, 1), (17, 4, 0)):
        index = _index(_bf16(Db), CCR_OPT_RANK=rank, CCR_TILE_CAP=cap, **plan)
        s, i = index.search(_bf16(Qb), k, FUSED)
        st = index.last_stats()
        print(rank, cap, st)
        assert st["path"] == 1 and st["main_launches"] == 1 and st["sample_tiles"] == sampled and st["skipped_tiles"] == sampled, st
        assert st["opt_rank"] == rank and st["tile_cap"] == cap, st
        assert st["n_fallback"] == flagged, st
        assert np.array_equal(i.cpu().numpy(), ref_i), f"ids differ in {np.sum(i.cpu().numpy() != ref_i)} places"
        assert np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


# ------------------------------------------------------------------------------------------------ search results against the dense path
_rows, _dense = {}, {}
NQ_SEARCH = 300


def _data(kind, n):
    """Seeded bf16 rows and queries of a kind, made once.  clustered / sorted: 64 centres, row = 0.8 centre + 0.6 noise; sorted: the
    corpus in topical order, cluster c owns rows [c n / 64, (c + 1) n / 64) -- about one tile per cluster at 16 640 rows."""
    if (kind, n) not in _rows:
        g = torch.Generator().manual_seed(n + len(kind))
        D = torch.randn(n, DIM, generator=g) * DIM ** -0.5
        Q = torch.randn(NQ_SEARCH, DIM, generator=g) * DIM ** -0.5
        if kind != "gaussian":
            centres = torch.randn(64, DIM, generator=g) * DIM ** -0.5
            cid = torch.randint(0, 64, (n,), generator=g) if kind == "clustered" else torch.arange(n) * 64 // n
            D = 0.8 * centres[cid] + 0.6 * D
            Q = 0.8 * centres[torch.randint(0, 64, (NQ_SEARCH,), generator=g)] + 0.6 * Q
        _rows[(kind, n)] = (_bf16(orc.pack_bf16(D.numpy())), _bf16(orc.pack_bf16(Q.numpy())))
    return _rows[(kind, n)]


def _dense_lists(kind, n, k):
    """The exact dense path's answer, computed once per (data, rows, k) and shared by both main-pass tiles."""
    if (kind, n, k) not in _dense:
        D, Q = _data(kind, n)
        s, i = _index(D).search(Q, k, DENSE)
        _dense[(kind, n, k)] = (s.cpu(), i.cpu())
    return _dense[(kind, n, k)]


@pytest.mark.parametrize("wide", [1, 0], ids=["256x384", "256x256"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("n", [16_640, 250_003])
@pytest.mark.parametrize("kind", ["gaussian", "clustered", "sorted"])
def test_capped_estimated_search_equals_the_dense_path(kind, n, k, wide):
    D, Q = _data(kind, n)
    want_s, want_i = _dense_lists(kind, n, k)
    # (65 tiles: the planner's own 1/32 sample is four tiles, too few to estimate from -- a quarter of the tiles is 17)
    pin = {"CCR_SAMPLE_DIV": 4} if n == 16_640 else {}
    index = _index(D, CCR_NARROW=0, CCR_OPTIMISTIC=1, CCR_WIDE=wide, **pin)
    s, i = index.search(Q, k, FUSED)
    st = index.last_stats()
    print(kind, n, k, wide, st)
    assert st["path"] == 1 and st["main_launches"] == 1 and st["opt_rank"] >= 17, st
    assert 4 <= st["tile_cap"] <= 16 and st["opt_rank"] > 4 * st["tile_cap"] and st["main_tile_queries"] == (384 if wide else 256), st
    assert torch.equal(i.cpu(), want_i), f"ids differ in {int((i.cpu() != want_i).sum())} places"
    assert torch.equal(s.cpu().view(torch.int32), want_s.view(torch.int32))


@pytest.mark.parametrize("wide", [1, 0], ids=["256x384", "256x256"])
@pytest.mark.parametrize("kind", ["gaussian", "clustered", "sorted"])
def test_the_planners_reduced_rank_on_a_large_sample_equals_the_dense_path(kind, wide):
    """The planner's OWN rank below 40 -- the flagship combination: the main pass leaves out the sampled tiles of a sample of forty tiles
    or more, the rank is the formula's (17 here), the capacities stay sized for rank 40.  250 003 rows = 976 full tiles with every 16th
    sampled: 62 tiles.  No rank and no cap is pinned."""
    n, k = 250_003, 10
    D, Q = _data(kind, n)
    want_s, want_i = _dense_lists(kind, n, k)
    index = _index(D, CCR_NARROW=0, CCR_OPTIMISTIC=1, CCR_WIDE=wide, CCR_SAMPLE_DIV=16, CCR_SKIP_SAMPLED=1)
    s, i = index.search(Q, k, FUSED)
    st = index.last_stats()
    print(kind, wide, st)
    assert st["path"] == 1 and st["main_launches"] == 1 and st["sample_tiles"] >= 40 and st["skipped_tiles"] == st["sample_tiles"], st
    assert 17 <= st["opt_rank"] < 40 and st["tile_cap"] == 4 and st["main_tile_queries"] == (384 if wide else 256), st
    assert torch.equal(i.cpu(), want_i), f"ids differ in {int((i.cpu() != want_i).sum())} places"
    assert torch.equal(s.cpu().view(torch.int32), want_s.view(torch.int32))
