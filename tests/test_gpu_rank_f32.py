"""The fp32 ranking on top of the 16-bit search (library version 111): ccr_keep_f32 and ccr_rescore_f32 against ccrec_amd/rank_f32_ref.py
bit for bit (ids and score bits), the verification flags against the restated rule, ops.ExactF32Index on every path it can take (first
rung, second rung, dense path, every row fetched, blocked rows), and the CCREC_RANK_PRECISION switch through the public ranking."""
import ctypes

import numpy as np
import pytest
import torch

from ccrec_amd import index_ref
from ccrec_amd import rank_f32_ref as R
from rank_f32_cases import gaussian, near_duplicate_cluster

pytestmark = pytest.mark.gpu

TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16}
OFFSET = 1000


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def half_bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def packed_and_kept(x, dt, normalize):
    """numpy fp32 rows -> (packed rows, their norm bounds, kept fp32 rows, residual bounds) on the device."""
    from ccrec_amd import ops
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    nb = torch.empty(xt.shape[0], device="cuda")
    h = ops.pack_half(xt, TORCH[dt], normalize=normalize, norm_bounds=nb)
    y, r = ops.keep_f32(xt, h, normalize)
    return h, nb, y, r


def exact_index(x, dt, normalize, **kw):
    from ccrec_amd import ops
    h, nb, y, r = packed_and_kept(x, dt, normalize)
    return ops.ExactF32Index(h, y, nb, r, **kw)


def search_np(ix, Q, k, normalize=False, **kw):
    s, i = ix.search(torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda(), k, normalize=normalize, **kw)
    assert s.shape == i.shape == (Q.shape[0], k) and s.dtype == torch.float32 and i.dtype == torch.int64
    return i.cpu().numpy() - ix.offset, s.cpu().numpy()


_TRUTH = {}


def truth(key, Q, D, k, normalize, block=None):
    """rank_f32_ref's exhaustive fp32 ranking, computed once per case and shared (never modified)."""
    if key not in _TRUTH:
        _TRUTH[key] = R.ranking(R.kept_rows(Q, normalize), R.kept_rows(D, normalize), k, block)
    return _TRUTH[key]


# ================================================================================================ 1. the keep kernel
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("normalize", [False, True], ids=["dot", "cos"])
def test_keep_f32_rows_bounds_and_padding(dt, normalize):
    rs = np.random.RandomState(31)
    for rows in (1, 63, 257):
        for dim in (8, 100, 768, 1032):
            x = (rs.randn(rows, dim) * (1.0 if normalize else dim ** -0.5)).astype(np.float32)
            if rows > 2:
                x[1] = index_ref.unpack(index_ref.pack(x[1], dt), dt)         # a row the pack keeps exactly: residual 0 (dot)
            h, _, y, r = packed_and_kept(x, dt, normalize)
            pdim = R.padded_dim(dim)
            y_np, r_np, h_np = y.cpu().numpy(), r.cpu().numpy(), half_bits(h)
            want = R.kept_rows(x, normalize)
            assert y_np.shape == (rows, pdim) and np.array_equal(bits(y_np), bits(want)), (rows, dim)
            assert not y_np[:, dim:].any() and not h_np[:, dim:].any()                        # the padding columns are zero
            assert np.array_equal(index_ref.pack(y_np, dt), h_np), (rows, dim)                # the kept row IS what the pack rounded
            exact = R.residual_norms(y_np, h_np, dt)
            assert np.all(r_np.astype(np.float64) >= exact), (rows, dim)
            assert np.all(r_np.astype(np.float64) <= exact * (1 + 2.0 ** -10)), (rows, dim, float((r_np / np.maximum(exact, 1e-300)).max()))
            if rows > 2 and not normalize:
                assert r_np[1] == 0.0


# ================================================================================================ 2. the re-score kernel
def _rescore_case(Q, D, dt, k, n_cand):
    """The 16-bit search's first n_cand rows re-scored by the kernel and by the reference, from the SAME bounds."""
    from ccrec_amd import ops
    hd, nbd, yd, rd = packed_and_kept(D, dt, False)
    hq, nbq, yq, rq = packed_and_kept(Q, dt, False)
    A = torch.nextafter(nbq + rq, torch.full_like(nbq, float("inf")))
    assert np.array_equal(A.cpu().numpy(), R.query_norm_bounds(nbq.cpu().numpy(), rq.cpu().numpy()))
    cmax = torch.stack([rd.max(), nbd.max()])
    index = ops.CorpusIndex(hd, global_row_offset=OFFSET, norm_bounds=nbd)
    yq_np, yd_np = yq.cpu().numpy(), yd.cpu().numpy()
    yd_t = np.ascontiguousarray(yd_np.T)                                                      # shared by every reference re-score of the case
    out = {}
    for n in n_cand:
        s16, i16 = index.search(hq, n)
        for kk in sorted({k, n} if n <= 64 else {k}):                                          # k = n_cand: the chunk mode
            s, i, flags, diag = ops.rescore_f32(yq, yd, i16, s16, kk, A, rq, cmax, OFFSET)
            ref_s, ref_i, ref_f = R.rescore(yq_np, yd_np, i16.cpu().numpy(), s16.cpu().numpy(), kk, A.cpu().numpy(), rq.cpu().numpy(),
                                            float(cmax[0]), float(cmax[1]), OFFSET, yd_t=yd_t)
            assert np.array_equal(i.cpu().numpy(), ref_i), (n, kk)
            assert np.array_equal(bits(s.cpu().numpy()), bits(ref_s)), (n, kk)
            assert np.array_equal(flags.cpu().numpy(), ref_f), (n, kk, flags.cpu().numpy(), ref_f)
            d = diag.cpu().numpy()
            assert np.array_equal(bits(d[:, 0]), bits(ref_s[:, -1])) and np.array_equal(bits(d[:, 1]), bits(s16[:, -1].cpu().numpy()))
            out[(n, kk)] = flags.cpu().numpy()
    return out


@pytest.mark.parametrize("dim", [8, 104, 768, 1032, 4096])
def test_rescore_equals_the_reference_at_every_list_length(dim):
    rs = np.random.RandomState(100 + dim)
    k = 10
    D = (rs.randn(5000, dim) * dim ** -0.5).astype(np.float32)
    Q = (rs.randn(8, dim) * dim ** -0.5).astype(np.float32)
    dt = "fp16" if dim in (104, 1032) else "bf16"
    flags = _rescore_case(Q, D[:3000], dt, k, (k, 52, 1000, 3000))                             # 3000 = N: every row fetched
    assert not flags[(3000, k)].any()
    _rescore_case(Q, D, dt, k, (4096,))                                                        # MAX_K of N = 5000: 16 chunks of rows


def test_rescore_orders_tied_scores_by_id():
    from ccrec_amd import ops
    rs = np.random.RandomState(77)
    D = rs.randint(-8, 9, size=(400, 40)).astype(np.float32) / 8                               # exact arithmetic: equal rows score equal
    D[100:160] = D[5]
    D[300:320, :20] = D[9, :20]
    Q = rs.randint(-8, 9, size=(5, 40)).astype(np.float32) / 8
    Q[0] = D[5]
    Q[1] = 0.0                                                                                 # every score equal: the order is the row order
    flags = _rescore_case(Q, D, "bf16", 30, (64, 200))
    assert flags[(64, 30)][1] == 1                                                             # a tie across the cut is never "verified"
    ix = exact_index(D, "bf16", False)
    want_i, want_s = truth("ties", Q, D, 30, False)
    got_i, got_s = search_np(ix, Q, 30)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    assert ix.last_stats()["dense"] == 0 and ix.last_stats()["rungs"][-1] == 400               # all-equal scores: every row is fetched


def test_rescore_bad_shapes_return_an_error_and_leave_the_outputs_alone():
    from ccrec_amd import _lib, ops
    lib = ops._require_rank_f32()
    rs = np.random.RandomState(3)
    D, Q = (rs.randn(50, 16) / 4).astype(np.float32), (rs.randn(2, 16) / 4).astype(np.float32)
    hd, nbd, yd, rd = packed_and_kept(D, "bf16", False)
    hq, nbq, yq, rq = packed_and_kept(Q, "bf16", False)
    cmax = torch.stack([rd.max(), nbd.max()])
    s16, i16 = ops.CorpusIndex(hd, norm_bounds=nbd).search(hq, 20)
    out_s = torch.full((2, 20), 7.5, device="cuda")
    out_i = torch.full((2, 20), -3, dtype=torch.int64, device="cuda")
    flags = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    ws = torch.full((64,), 2.5, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_cand=20, k=10, pdim=16, queries=yq, out=out_s):
        rc = lib.ccr_rescore_f32(p(queries) if queries is not None else None, p(yd), 50, pdim, p(i16), p(s16), 2, n_cand, k, 0, p(nbq), p(rq),
                                 p(cmax), p(out) if out is not None else None, p(out_i), p(flags), p(ws), ws.numel() * 4, None)
        torch.cuda.synchronize()
        return rc

    assert call(k=21) == _lib.CCR_ERR_INVALID                                                  # k > n_cand
    assert call(n_cand=ops.MAX_K + 1) == _lib.CCR_ERR_INVALID                                  # n_cand > MAX_K
    assert call(n_cand=51, k=10) == _lib.CCR_ERR_INVALID                                       # more candidates than rows
    assert call(pdim=12) == _lib.CCR_ERR_INVALID                                               # pdim % 8 != 0
    assert call(queries=None) == _lib.CCR_ERR_INVALID and call(out=None) == _lib.CCR_ERR_INVALID   # null pointers
    assert int(lib.ccr_rescore_f32_workspace_bytes(2, 20, 21, 16)) == 0 and int(lib.ccr_rescore_f32_workspace_bytes(2, 20, 10, 16)) == 32
    assert bool((out_s == 7.5).all()) and bool((out_i == -3).all()) and bool((flags == 9).all()) and bool((ws == 2.5).all())
    assert call() == _lib.CCR_OK and bool((flags != 9).all())                                  # the same buffers, a good shape
    with pytest.raises(_lib.CcrError):
        ops.rescore_f32(yq, yd, i16, s16, 21, nbq, rq, cmax)


# ================================================================================================ 3. the search
def test_near_duplicate_cluster_plain_search_is_wrong_exact_search_is_right():
    """Rows that differ below bf16's spacing: the 16-bit search returns them in corpus order whatever their fp32 scores say.
    FAILS without the feature: nothing else in the library can return rows 99..90 here."""
    from ccrec_amd import ops
    Q, D = near_duplicate_cluster()
    k = 10
    want_i, want_s = truth("cluster", Q, D, k, False)
    assert want_i[0].tolist() == list(range(99, 89, -1))
    h, nb, y, r = packed_and_kept(D, "bf16", False)
    plain = ops.CorpusIndex(h, norm_bounds=nb)
    _, ids = plain.search(ops.pack_bf16(torch.from_numpy(Q).cuda()), k)
    assert ids[0].tolist() == list(range(10))                                                  # the bf16 ranking: corpus order
    ix = ops.ExactF32Index(h, y, nb, r, max_candidates=64)
    got_i, got_s = search_np(ix, Q, k)
    assert got_i[0].tolist() == list(range(99, 89, -1)) and np.array_equal(bits(got_s), bits(want_s))
    st = ix.last_stats()
    assert st["rungs"] == [52, 64] and st["flagged"] == [1, 1] and st["dense"] == 1, st        # both rungs unverified, one dense query
    assert 10 <= st["dense_rows"][0] <= 100, st
    ix = ops.ExactF32Index(h, y, nb, r)                                                        # default: the second rung (104 rows) holds the cluster
    got_i, got_s = search_np(ix, Q, k)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    st = ix.last_stats()
    assert st["rungs"] == [52, 104] and st["flagged"] == [1, 0] and st["dense"] == 0, st


def test_dense_path_merges_chunks_beyond_max_k():
    """5 000 rows that round to the query in bf16, each with its own noise below bf16's spacing: their residual bounds are alike, so the
    dense filter keeps nearly all of them (4 806 with the reference's bounds) -- more than one re-score takes; the chunks are merged."""
    from ccrec_amd import ops
    rs = np.random.RandomState(12)
    d, n, k = 32, 6000, 20
    v = index_ref.unpack(index_ref.pack((rs.randn(d) / np.sqrt(d)).astype(np.float32), "bf16"), "bf16")
    D = (rs.randn(n, d) / np.sqrt(d) * 0.25).astype(np.float32)
    u = rs.uniform(-1, 1, size=(5000, d))
    D[:5000] = (v.astype(np.float64)[None, :] * (1.0 + u * 2.0 ** -10)).astype(np.float32)
    assert (index_ref.pack(D[:5000], "bf16") == index_ref.pack(v, "bf16")[None, :]).all()
    Q = v[None, :].copy()
    ix = exact_index(D, "bf16", False)
    want_i, want_s = truth("chunks", Q, D, k, False)
    got_i, got_s = search_np(ix, Q, k)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    st = ix.last_stats()
    assert st["rungs"][-1] == ops.MAX_K and st["flagged"][-1] == 1 and st["dense"] == 1 and st["dense_rows"][0] > ops.MAX_K, st


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("normalize", [False, True], ids=["dot", "cos"])
def test_gaussian_every_position_and_every_query_verified_on_the_first_rung(dt, normalize):
    Q, D = gaussian()
    k = 100
    want_i, want_s = truth(("gauss", normalize), Q, D, k, normalize)
    ix = exact_index(D, dt, normalize, global_row_offset=OFFSET)
    got_i, got_s = search_np(ix, Q, k, normalize)
    assert np.array_equal(got_i, want_i), f"{np.sum(got_i != want_i)} of 1600 positions differ"
    assert np.array_equal(bits(got_s), bits(want_s))
    st = ix.last_stats()
    assert st["rungs"] == [232] and st["flagged"] == [0] and st["dense"] == 0, st              # no second rung, no dense path


def test_every_row_fetched_tiny_corpus_and_no_queries():
    rs = np.random.RandomState(21)
    D, Q = (rs.randn(1500, 64) / 8).astype(np.float32), (rs.randn(4, 64) / 8).astype(np.float32)
    ix = exact_index(D, "bf16", False)
    want_i, want_s = truth("k1001", Q, D, 1001, False)
    got_i, got_s = search_np(ix, Q, 1001)                                                      # 2 k + 32 > N: all rows fetched, trivially verified
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    assert ix.last_stats() == {"rungs": [1500], "flagged": [0], "dense": 0, "dense_rows": []}
    D5 = D[:5, :13].copy()                                                                     # N = 5, a width that is padded
    ix5 = exact_index(D5, "fp16", True)
    for k in (1, 5):
        want_i, want_s = truth(("n5", k), Q[:, :13], D5, k, True)
        got_i, got_s = search_np(ix5, Q[:, :13], k, True)
        assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_s), bits(want_s))
    with pytest.raises(ValueError):
        search_np(ix5, Q[:, :13], 6, True)
    s, i = ix.search(torch.empty(0, 64, device="cuda"), 10)                                    # Q = 0
    assert s.shape == i.shape == (0, 10) and ix.last_stats()["rungs"] == []


# ================================================================================================ 4. blocked rows, through the public API
@pytest.fixture
def rank_env(monkeypatch):
    for name in ("CCREC_RANK_PRECISION", "CCREC_INDEX_DTYPE", "CCREC_SIM_TYPE"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _blocked_case():
    rs = np.random.RandomState(44)
    n, nq, d = 300, 7, 40
    Ed, Eq = (rs.randn(n, d) / 6).astype(np.float32), (rs.randn(nq, d) / 6).astype(np.float32)
    Ed[:nq] = Eq * 1.5                                                                         # row q is query q's best match, and is blocked
    block = [[q] for q in range(nq)]
    block[3] = sorted(set(range(n)) - {10, 20, 30, 40, 50})                                    # 295 rows: -1e6 entries enter every list
    return Eq, Ed, block


def _profile_arrays(prof, nq):
    ids = np.array([[int(p[1:]) for p in prof[f"q{i}"]] for i in range(nq)], np.int64)
    sc = np.array([list(prof[f"q{i}"].values()) for i in range(nq)], np.float32)
    return ids, sc


@pytest.mark.parametrize("sim", ["dot", "cos"])
def test_blocked_rows_through_retriever_and_ranking(rank_env, sim):
    from ccrec_amd.ms_marco_eval import Retriever, ranking
    Eq, Ed, block = _blocked_case()
    nq, n = Eq.shape[0], Ed.shape[0]
    normalize = sim == "cos"
    h, nb, y, r = packed_and_kept(Ed, "bf16", normalize)
    retriever = Retriever([f"p{j}" for j in range(n)], h, global_row_offset=OFFSET, norm_bounds=nb, corpus_f32=y, res_bounds=r, normalize=normalize)
    for k in (50, 300):
        want_i, want_s = truth(("blocked", sim, k), Eq, Ed, k, normalize, block)
        s, i = retriever.search(torch.from_numpy(Eq).cuda(), k, block)
        assert np.array_equal(i.cpu().numpy() - OFFSET, want_i) and np.array_equal(bits(s.cpu().numpy()), bits(want_s)), k
        assert want_s[3, 5] == np.float32(-1e6) and want_s[3, 4] > -1e6                        # 5 unblocked rows, then the blocked ones
    assert retriever.exact.last_stats()["dense"] == 0
    # ranking() under the switch, with block_dict: the fp32 ranking with the -1e6 rule (k = min(1001, N) = every row)
    rank_env.setenv("CCREC_RANK_PRECISION", "fp32")
    rank_env.setenv("CCREC_SIM_TYPE", sim)
    table = torch.cat([torch.from_numpy(Eq), torch.from_numpy(Ed)], 0)
    queries = {f"q{i}": i for i in range(nq)}
    corpus = {f"p{j}": nq + j for j in range(n)}
    block_dict = {f"q{i}": [f"p{j}" for j in block[i]] for i in range(nq)}
    prof = ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], 64, block_dict)
    ids, sc = _profile_arrays(prof, nq)
    want_i, want_s = truth(("blocked", sim, 300), Eq, Ed, 300, normalize, block)
    assert np.array_equal(ids, want_i) and np.array_equal(bits(sc), bits(want_s))
    rank_env.setenv("CCREC_INDEX_DTYPE", "fp16")                                               # both 16-bit index types work underneath
    ids, sc = _profile_arrays(ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], 64, block_dict), nq)
    assert np.array_equal(ids, want_i) and np.array_equal(bits(sc), bits(want_s))


# ================================================================================================ 5. the switch
def test_ranking_with_the_variable_unset_is_the_plain_retriever(rank_env):
    from ccrec_amd import ops
    from ccrec_amd.ms_marco_eval import Retriever, ranking
    Eq, Ed, block = _blocked_case()
    nq, n = Eq.shape[0], Ed.shape[0]
    rank_env.setenv("CCREC_SIM_TYPE", "dot")
    table = torch.cat([torch.from_numpy(Eq), torch.from_numpy(Ed)], 0)
    queries = {f"q{i}": i for i in range(nq)}
    corpus = {f"p{j}": nq + j for j in range(n)}
    block_dict = {f"q{i}": [f"p{j}" for j in block[i]] for i in range(nq)}
    prof = ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], 64, block_dict)
    nb = torch.empty(n, device="cuda")
    by_hand = Retriever(list(corpus), ops.pack_bf16(torch.from_numpy(Ed).cuda(), norm_bounds=nb), norm_bounds=nb)
    assert by_hand.exact is None
    want = by_hand.ranking_profile(list(queries), ops.pack_bf16(torch.from_numpy(Eq).cuda()), block_dict)
    assert list(prof) == list(want)
    for q in prof:
        assert list(prof[q].items()) == list(want[q].items())
    ids, sc = _profile_arrays(prof, nq)
    ref_i, ref_s = index_ref.canonical_search(index_ref.pack(Eq, "bf16"), index_ref.pack(Ed, "bf16"), "bf16", n, block)
    assert np.array_equal(ids, ref_i) and np.array_equal(bits(sc), bits(ref_s))


def test_out_of_scope_entry_points_raise_under_fp32(rank_env):
    from ccrec_amd import ops
    from ccrec_amd.bbpr_transform import LowRankScore, score_op
    from ccrec_amd.encode import ranking_sharded
    from ccrec_amd.rime_util import _assign_topk
    rs = np.random.RandomState(9)
    U_, V_ = torch.from_numpy(rs.randn(4, 16).astype(np.float32)).cuda(), torch.from_numpy(rs.randn(60, 16).astype(np.float32)).cuda()
    S = LowRankScore(ops.pack_bf16(U_), ops.pack_bf16(V_))
    index = ops.CorpusIndex(ops.pack_bf16(V_))
    ptr = np.zeros(5, np.int64)
    args = (ops.pack_bf16(U_), 3, ptr, np.zeros(0, np.int64), np.zeros(0))
    assert _assign_topk(S, 3).nnz == 12 and score_op(S, "max") == score_op(S, "max")           # unset: they run
    index.search_sparse_prior(*args)
    rank_env.setenv("CCREC_SIM_TYPE", "dot")
    rank_env.setenv("CCREC_RANK_PRECISION", "fp32")
    for call in (lambda: ranking_sharded({"p": "a"}, {"q": "b"}, None), lambda: index.search_sparse_prior(*args),
                 lambda: _assign_topk(S, 3), lambda: score_op(S, "max")):
        with pytest.raises(NotImplementedError, match="CCREC_RANK_PRECISION"):
            call()
    rank_env.setenv("CCREC_RANK_PRECISION", "exact")
    with pytest.raises(ValueError, match="CCREC_RANK_PRECISION"):
        _assign_topk(S, 3)


def test_a_corpus_holding_an_inf_raises_at_build(rank_env):
    from ccrec_amd.ms_marco_eval import ranking
    Eq, Ed, _ = _blocked_case()
    Ed = Ed.copy()
    Ed[17, 3] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        exact_index(Ed, "bf16", False)
    rank_env.setenv("CCREC_SIM_TYPE", "dot")
    rank_env.setenv("CCREC_RANK_PRECISION", "fp32")
    table = torch.cat([torch.from_numpy(Eq), torch.from_numpy(Ed)], 0)
    queries = {f"q{i}": i for i in range(Eq.shape[0])}
    corpus = {f"p{j}": Eq.shape[0] + j for j in range(Ed.shape[0])}
    with pytest.raises(ValueError, match="not finite"):
        ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], 64)
    rank_env.delenv("CCREC_RANK_PRECISION")                                                    # ... and stays on the 16-bit path
    assert len(ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], 64)) == Eq.shape[0]
