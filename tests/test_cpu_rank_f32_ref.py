"""ccrec_amd/rank_f32_ref.py -- the CPU definition the fp32 ranking is checked against: its score rule on exact arithmetic, the
CCREC_RANK_PRECISION switch, the soundness of the verification rule (whenever it says "verified", the candidates' top-k IS the
exhaustive fp32 ranking), and the path the search takes on the two constructions the GPU tests use."""
import numpy as np
import pytest

from ccrec_amd import index_ref, ops
from ccrec_amd import rank_f32_ref as R
from rank_f32_cases import gaussian, near_duplicate_cluster


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_score_rule_on_an_exact_arithmetic_table():
    rs = np.random.RandomState(5)
    D = rs.randint(-16, 17, size=(70, 40)).astype(np.float32) / 8          # multiples of 1/8: every summation order agrees
    Q = rs.randint(-16, 17, size=(6, 40)).astype(np.float32) / 8
    D[20:30] = D[4]                                                        # ties: the ids decide
    yq, yd = R.kept_rows(Q), R.kept_rows(D)
    assert yq.shape == (6, 40) and np.array_equal(bits(yq), bits(Q))
    s = R.scores(yq, yd)
    want = Q.astype(np.float64) @ D.astype(np.float64).T
    assert np.array_equal(s.astype(np.float64), want)
    assert np.array_equal(s, (Q[:, ::-1].astype(np.float64) @ D[:, ::-1].astype(np.float64).T).astype(np.float32))
    ids, sc = R.ranking(yq, yd, 25)
    for q in range(6):
        o = np.lexsort((np.arange(70), -want[q]))[:25]
        assert np.array_equal(ids[q], o) and np.array_equal(sc[q].astype(np.float64), want[q][o])
    blocked = [[int(ids[q, 0]), 3] for q in range(6)]                      # a blocked row scores -1e6 and stays in the ranking
    bi, bs = R.ranking(yq, yd, 70, blocked)
    assert np.all(bs[:, -2:] == np.float32(-1e6)) and all(set(bi[q, -2:].tolist()) == set(blocked[q]) for q in range(6))


def test_kept_rows_pad_and_round_to_the_packed_rows():
    rs = np.random.RandomState(6)
    for dim in (8, 13, 100):
        x = (rs.randn(9, dim) * 3).astype(np.float32)
        for normalize in (False, True):
            y = R.kept_rows(x, normalize)
            assert y.shape == (9, R.padded_dim(dim)) and not y[:, dim:].any()
            for dt in ("bf16", "fp16"):
                want = index_ref.normalize_pack(x, dt) if normalize else index_ref.pack(x, dt)
                assert np.array_equal(index_ref.pack(y, dt)[:, :dim], want)
                h = index_ref.pack(y, dt)
                b, exact = R.res_bounds(y, h, dt), R.residual_norms(y, h, dt)
                assert b.dtype == np.float32 and np.all(b.astype(np.float64) >= exact) and np.all(b <= exact * (1 + 2.0 ** -10) + 1e-45)
    assert np.array_equal(R.round_up_f32([1.0, 1.0 + 2.0 ** -40, 0.0]), np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), 0.0], np.float32))


def test_switch_parses_and_rejects(monkeypatch):
    monkeypatch.delenv("CCREC_RANK_PRECISION", raising=False)
    assert ops.rank_precision() == "index"
    ops.require_index_rank("anything")                                     # default: nothing is refused
    monkeypatch.setenv("CCREC_RANK_PRECISION", "fp32")                     # read at call time
    assert ops.rank_precision() == "fp32"
    with pytest.raises(NotImplementedError, match="CCREC_RANK_PRECISION"):
        ops.require_index_rank("encode.ranking_sharded")
    monkeypatch.setenv("CCREC_RANK_PRECISION", "index")
    assert ops.rank_precision() == "index"
    for bad in ("", "bf16", "fp64", "FP32", "exact"):
        monkeypatch.setenv("CCREC_RANK_PRECISION", bad)
        with pytest.raises(ValueError, match="CCREC_RANK_PRECISION"):
            ops.rank_precision()
    # CCREC_INDEX_DTYPE keeps its two values whatever the rank precision is
    monkeypatch.setenv("CCREC_RANK_PRECISION", "fp32")
    monkeypatch.delenv("CCREC_INDEX_DTYPE", raising=False)
    import torch
    assert ops.index_dtype() == torch.bfloat16
    monkeypatch.setenv("CCREC_INDEX_DTYPE", "fp16")
    assert ops.index_dtype() == torch.float16
    monkeypatch.setenv("CCREC_INDEX_DTYPE", "fp32")
    with pytest.raises(ValueError, match="CCREC_INDEX_DTYPE"):
        ops.index_dtype()


def test_binding_declares_the_entry_points():
    from ccrec_amd import _lib
    assert _lib.RANK_F32_VERSION == 111 and callable(ops._require_rank_f32)
    assert {"ccr_keep_f32", "ccr_rescore_f32", "ccr_rescore_f32_workspace_bytes"} <= set(_lib.EXPORTS)
    assert ops.MAX_K == R.MAX_K == 4096
    assert R.rungs(20000, 100) == [232, 464, 928, 1856, 3712, 4096] and R.rungs(600, 10, 64) == [52, 64] and R.rungs(5, 5) == [5]
    assert R.rungs(1500, 1001) == [1500]


def test_verification_rule_is_sound_on_200_random_problems():
    """Whenever the restated rule says "verified" for a candidate list, the candidates' top-k equals the exhaustive fp32 ranking.
    Data that makes the rule work for its living: rows drawn around a few centres (near-duplicates), norms spread, k and the list
    length drawn at random -- so both outcomes occur many times."""
    rs = np.random.RandomState(2024)
    said_yes = said_no = 0
    for trial in range(200):
        d = (8, 40, 768)[trial % 3]
        dt = ("bf16", "fp16")[(trial // 3) % 2]
        n = int(rs.randint(20, 401)) if d < 768 else int(rs.randint(20, 121))
        nq = 3
        centres = rs.randn(4, d)
        spread = 10.0 ** rs.uniform(-5, 0)
        X = centres[rs.randint(0, 4, size=n)] + spread * rs.randn(n, d)
        X = (X * np.exp(0.3 * rs.randn(n, 1)) / np.sqrt(d)).astype(np.float32)
        Qx = ((centres[rs.randint(0, 4, size=nq)] + spread * rs.randn(nq, d)) / np.sqrt(d)).astype(np.float32)
        normalize = bool(trial % 2)
        yq, yd = R.kept_rows(Qx, normalize), R.kept_rows(X, normalize)
        hq, hd = index_ref.pack(yq, dt), index_ref.pack(yd, dt)
        rq, rd = R.res_bounds(yq, hq, dt), R.res_bounds(yd, hd, dt)
        A = R.query_norm_bounds(R.norm_bounds(hq, dt), rq)
        Rmax, Nmax = rd.max(), R.norm_bounds(hd, dt).max()
        k = int(rs.randint(1, min(n, 30) + 1))
        n_cand = int(rs.randint(k, (n if trial % 4 == 0 else min(n, 2 * k + 8)) + 1))   # mostly short lists: both outcomes occur
        s16 = index_ref.canonical_scores(hq, hd, dt)
        ids16, sc16 = index_ref.rank(s16, n_cand)
        got_s, got_i, flags = R.rescore(yq, yd, ids16, sc16, k, A, rq, Rmax, Nmax)
        want_i, want_s = R.ranking(yq, yd, k)
        for q in range(nq):
            if flags[q] == 0:
                said_yes += 1
                assert np.array_equal(got_i[q], want_i[q]) and np.array_equal(bits(got_s[q]), bits(want_s[q])), (trial, q, d, dt, n, k, n_cand)
            else:
                said_no += 1
    assert said_yes >= 100 and said_no >= 100, (said_yes, said_no)


def test_near_duplicate_cluster_takes_the_stated_path():
    Q, D = near_duplicate_cluster()
    hb, qb = index_ref.pack(D, "bf16"), index_ref.pack(Q, "bf16")
    assert index_ref.canonical_search(qb, hb, "bf16", 10)[0][0].tolist() == list(range(10))          # bf16: corpus order
    truth_i, truth_s = R.ranking(R.kept_rows(Q), R.kept_rows(D), 10)
    assert truth_i[0].tolist() == list(range(99, 89, -1))                                            # fp32: rows 99..90
    ids, s, st = R.exact_search(Q, D, "bf16", 10, max_candidates=64)
    assert np.array_equal(ids, truth_i) and np.array_equal(bits(s), bits(truth_s))
    assert st["rungs"] == [52, 64] and st["flagged"] == [1, 1] and st["dense"] == 1                   # both rungs unverified, then dense
    assert 10 <= st["dense_rows"][0] <= 100                                                          # (46 of the cluster's 100 rows)
    ids, s, st = R.exact_search(Q, D, "bf16", 10)                                                    # default: the second rung holds the cluster
    assert np.array_equal(ids, truth_i) and np.array_equal(bits(s), bits(truth_s))
    assert st["rungs"] == [52, 104] and st["flagged"] == [1, 0] and st["dense"] == 0


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_gaussian_is_verified_on_the_first_rung(dt):
    Q, D = gaussian()
    ids, s, st = R.exact_search(Q, D, dt, 100)
    assert st["rungs"] == [232] and st["flagged"] == [0] and st["dense"] == 0
    want_i, want_s = R.ranking(R.kept_rows(Q), R.kept_rows(D), 100)
    assert np.array_equal(ids, want_i) and np.array_equal(bits(s), bits(want_s))


def test_non_finite_embeddings_are_refused():
    Q, D = near_duplicate_cluster()
    D = D.copy()
    D[17, 3] = np.inf
    with pytest.raises(ValueError):
        R.exact_search(Q, D, "bf16", 10)
