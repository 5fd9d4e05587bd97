"""The two exact paths every search ends on -- the fp64 dense path (dense_scores_kernel + dense_select_kernel, csrc/ccr_dense.hip) and the
margin path (MFMA score rows + margin_select_kernel + canonical re-score) -- and the primitives under them (block_radix_select,
radix_pick_digit, hist_add_aggregated, block_bitonic_sort_desc, csrc/ccr_topk_device.h), at every tile edge, tie and digit.  Most of the
suite uses these paths as its referee; here they face references that are not the library: oracle.canonical_* (bf16),
ccrec_amd.index_ref (fp16) and, for the exact-score probe of helpers.exact_probe_* (validated by tests/test_cpu_exact_probe.py), the order
computed in numpy from the integers the test chose.  Every comparison is bit for bit, ids and score patterns; no tolerance anywhere."""
import numpy as np
import pytest
import torch

from ccrec_amd import index_ref
from helpers import (EXACT_PROBE, EXACT_PROBE_FP16_WIDE_E, exact_probe_cat, exact_probe_draw, exact_probe_fixed, exact_probe_queries,
                     exact_probe_rows, exact_probe_scores, exact_probe_take, exact_probe_topk)
from oracle import oracle as orc
from test_gpu_index_fp16 import _f16
from test_gpu_wide import DENSE, FUSED, _bf16, _knobs

pytestmark = pytest.mark.gpu

OFFSET = 4321
KINDS = ["bf16", "fp16"]
SCALES = (1.0, -1.0, 8.0, -0.25)          # the probe query and three scaled copies: both directions of the order, other exponents


# ================================================================================================ plumbing
def _dev(bits, kind):
    return _bf16(bits) if kind == "bf16" else _f16(bits)


def _index(Db, kind, **knobs):
    from ccrec_amd import ops
    with _knobs(**knobs):
        return ops.CorpusIndex(_dev(Db, kind), global_row_offset=OFFSET)


def _pack(x, kind):
    x = np.ascontiguousarray(x, np.float32)
    return orc.pack_bf16(x) if kind == "bf16" else index_ref.pack(x, "fp16")


def _unpack(bits, kind):
    return index_ref.unpack(bits, kind)


def _rand(n, d, seed, kind):
    g = torch.Generator().manual_seed(seed)
    return _pack((torch.randn(n, d, generator=g) * d ** -0.5).numpy(), kind)


def _oracle_scores(Qb, Db, kind):
    return orc.canonical_scores(Qb, Db) if kind == "bf16" else index_ref.canonical_scores(Qb, Db, "fp16")


def _oracle_search(Qb, Db, kind, k):
    return orc.canonical_search(Qb, Db, k) if kind == "bf16" else index_ref.canonical_search(Qb, Db, "fp16", k)


def _search(index, Q, k, flags, **want):
    """(local ids, score bit patterns) of one search; `want`: what last_stats() must report about it."""
    s, i = index.search(Q, k, flags)
    st = index.last_stats()
    for name, v in want.items():
        assert st[name] == v, (name, v, st)
    return i.cpu().numpy() - index.offset, s.cpu().numpy().view(np.uint32)


def _same(got, ref_ids, ref_scores, what=""):
    ids, bits = got
    assert ids.shape == ref_ids.shape, (what, ids.shape, ref_ids.shape)
    assert np.array_equal(ids, ref_ids), f"{what}: ids differ in {np.sum(ids != ref_ids)} of {ids.size} places"
    assert np.array_equal(bits, np.ascontiguousarray(ref_scores, np.float32).view(np.uint32)), f"{what}: score bits differ"


def _probe_case(digits, kind, ks, scales=SCALES, e_range=None, flags=DENSE):
    """The probe corpus of `digits` searched on the fp64 path (stat: path == 0) at every k of `ks` against the numpy order."""
    index = _index(exact_probe_rows(digits, kind, e_range=e_range), kind)
    Q = _dev(exact_probe_queries(scales, kind), kind)
    for k in ks:
        ref_i, ref_s = exact_probe_topk(digits, kind, scales, k)
        _same(_search(index, Q, k, flags, path=0), ref_i, ref_s, f"{kind} n={len(digits[0])} k={k}")
    return index, Q


# ================================================================================================ 2. dense_select_kernel, radix primitives
_FLAT = {}


def _flat(kind, e_range=None):
    """20 011 rows with every digit uniform, drawn once per form."""
    key = (kind, e_range)
    if key not in _FLAT:
        _FLAT[key] = exact_probe_draw(20_011, 11, kind, e_range)
    return _FLAT[key]


@pytest.mark.parametrize("kind,e_range", [("bf16", None), ("fp16", None), ("fp16", EXACT_PROBE_FP16_WIDE_E)])
def test_flat_digit_distribution(kind, e_range):
    """dense_select_kernel<true> on score rows whose four radix digits are all spread out: 26 (bf16), 14 or 20 (fp16) top bytes, each wave
    of 64 rows holds more than three, so hist_add_aggregated runs its three aggregated rounds AND its fallback atomic in every pass;
    the three low digits take all 256 values, so radix_pick_digit's crossing lane walks its own four bins to a bin that is not its
    lowest, and a histogram pass that forgot the prefix of the digits above ((o & mask) == prefix) would pick another k-th key.  79 trips
    per thread, the last one partly filled.  Stat: path == 0 under the dense flag."""
    _probe_case(_flat(kind, e_range), kind, (1, 7, 256, 257, 1001, 4096), e_range=e_range)


@pytest.mark.parametrize("kind", KINDS)
def test_long_shared_prefixes(kind):
    """A run of 3 000 rows that share the three high bytes of the score pattern (they differ in c alone: about twelve rows per value, so
    the cut also falls into a tie) and a run of 3 000 that share two, among 2 000 flat rows, in shuffled row order: with the cut inside a
    run the radix passes of the shared digits see ONE bin hold thousands of the remaining rows (the aggregated rounds add whole waves at
    once), and the last one or two passes alone decide.  Stat: path == 0."""
    hi = EXACT_PROBE[kind]["e"][1]
    flat = exact_probe_draw(2000, 23, kind)
    rs = np.random.RandomState(24)
    run2 = list(exact_probe_fixed(3000, 1, hi - 1, 200, 0, 0))
    run2[3], run2[4] = rs.randint(0, 256, 3000), rs.randint(0, 256, 3000)
    run3 = list(exact_probe_fixed(3000, 1, hi - 2, 180, 99, 0))
    run3[4] = rs.randint(0, 256, 3000)
    digits = exact_probe_cat(flat, tuple(run2), tuple(run3))
    member = np.repeat([0, 2, 3], [2000, 3000, 3000])
    perm = rs.permutation(8000)
    digits, member = exact_probe_take(digits, perm), member[perm]
    score = exact_probe_scores(digits, kind)
    ks = []
    for run, depth in ((2, 1500), (3, 500)):
        k = int(np.sum(score > score[member == run].max())) + depth
        assert k <= 4096 and member[np.lexsort((np.arange(8000), -score))[k - 1]] == run      # the cut is inside the run
        ks.append(k)
    print(kind, "cuts at k =", ks)
    _probe_case(digits, kind, ks, scales=(1.0, 2.0))


TIED_ROWS = np.array([0, 250, 251, 252, 501, 502, 753, 1002])     # n = 1 003: seg = 251, the quarters begin at 0, 251, 502, 753


@pytest.mark.parametrize("kind", KINDS)
def test_ties_at_the_cut_across_all_four_wave_quarters(kind):
    """dense_select_kernel gives each of its four waves a contiguous quarter of the row (seg = 251 of 1 003 rows) and ranks the rows that
    equal the k-th key by (s_wave_eq prefix of the quarters before) + (ballot prefix inside the wave): the eight rows equal to T sit at
    the first and last row of quarters and on both sides of every border.  g = 248 rows are above T, k = g + r keeps the first r tied
    rows in row order (r = 8: k = 256 = its own power-of-two padding, every tied row is kept).  Stat: path == 0."""
    n, g = 1003, 248
    rs = np.random.RandomState(31)
    lo = EXACT_PROBE[kind]["e"][0]
    digits = list(exact_probe_draw(n, 32, kind))
    digits[0][:] = 1
    digits[1][:] = rs.randint(lo, 1, n)                     # below T: exponents up to 0
    others = np.setdiff1d(np.arange(n), TIED_ROWS)
    above = rs.choice(others, g, replace=False)
    digits[1][above] = 3                                    # above T
    for d, v in zip(digits, (1, 2, 200, 5, 9)):             # T
        d[TIED_ROWS] = v
    digits = tuple(digits)
    score = exact_probe_scores(digits, kind)
    assert np.sum(score > score[0]) == g and np.sum(score == score[0]) == 8
    index = _index(exact_probe_rows(digits, kind), kind)
    Q = _dev(exact_probe_queries((1.0,), kind), kind)
    for r in (1, 2, 3, 5, 8):
        ref_i, ref_s = exact_probe_topk(digits, kind, (1.0,), g + r)
        assert np.array_equal(ref_i[0, g:], TIED_ROWS[:r]) and set(ref_i[0, :g]) == set(above)
        _same(_search(index, Q, g + r, DENSE, path=0), ref_i, ref_s, f"{kind} r={r}")


@pytest.mark.parametrize("kind", KINDS)
def test_all_rows_equal(kind):
    """Every radix pass has ONE occupied bin (radix_pick_digit: the crossing lane's suffix count is the whole row), need_eq == k and
    cnt_gt == 0: the result is rows 0 .. k - 1, each wave contributing the head of its quarter.  Stat: path == 0."""
    digits = exact_probe_fixed(1003, 1, 0, 173, 41, 7)
    for scale in (1.0, -1.0):
        index, Q = _probe_case(digits, kind, (1, 500, 1003), scales=(scale,))
        ids, _ = _search(index, Q, 1003, DENSE, path=0)
        assert np.array_equal(ids[0], np.arange(1003))


@pytest.mark.parametrize("kind", KINDS)
def test_tiny_rows(kind):
    """Rows shorter than a wave, a block and a quarter (seg = 1 at n <= 4: waves past the row own nothing), and one row more or less than
    64 and 256; k = 1 and k = n.  An index creation that refuses a shape must say so.  Stat: path == 0."""
    from ccrec_amd import _lib
    Q = _dev(exact_probe_queries(SCALES, kind), kind)
    for n in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257):
        digits = exact_probe_draw(n, 40 + n, kind)
        for d in digits:
            d[: n // 2] = d[0]                               # the first half of the row is one tie
        try:
            index = _index(exact_probe_rows(digits, kind), kind)
        except _lib.CcrError as e:
            assert "ccr_index_create" in str(e) and "n_rows" in str(e), e
            continue
        for k in sorted({1, n}):
            ref_i, ref_s = exact_probe_topk(digits, kind, SCALES, k)
            _same(_search(index, Q, k, DENSE, path=0), ref_i, ref_s, f"{kind} n={n} k={k}")


@pytest.mark.parametrize("kind", KINDS)
def test_k_and_its_power_of_two_padding(kind):
    """The key array is padded to pow2_ceil(k) with zero keys that must sort behind every real key (negative scores included: their
    orderable keys are small but not zero), block_bitonic_sort_desc runs 1 .. 78 steps, from n = 256 on across waves; k = n = 4 096
    leaves no row out, n = 4 097 exactly one.  Stat: path == 0."""
    digits = exact_probe_draw(5000, 51, kind)
    _probe_case(digits, kind, (1, 2, 3, 255, 256, 257, 4095, 4096))
    _probe_case(exact_probe_take(digits, np.arange(4096)), kind, (4096,))
    _probe_case(exact_probe_take(digits, np.arange(4097)), kind, (4096,))


# ================================================================================================ 3. dense_scores_kernel
SCORE_ROWS, SCORE_NQ, SCORE_DIMS = (1, 63, 64, 65, 129), (1, 63, 64, 65, 130), (8, 16, 24, 32, 40, 776, 4096)


def _score_shapes(dim):
    return [(n, q) for n in SCORE_ROWS for q in SCORE_NQ] if dim in (24, 776) else [(129, 65)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", SCORE_DIMS)
def test_canonical_scores_at_every_tile_edge(kind, dim):
    """index.scores(q, "canonical") = dense_scores_kernel with q_begin = 0: 64 x 64 tiles that are one row or query short, full, or one
    over (a second tile of one row; clamped staging rows, guarded stores), and the 32-wide K stage: dims 8, 24 and 40 end in a stage
    where staging threads (schunk with k0 + 8 schunk >= dim) hold zeros instead of loading, 776 in a stage of 8, 4 096 runs 128 full
    stages.  Every (rows, queries) pair at dims 24 and 776, every dim at 129 x 65.  No search runs: there is no stat to read."""
    for n, nq in _score_shapes(dim):
        Db, Qb = _rand(n, dim, 1000 * n + dim, kind), _rand(nq, dim, 2000 * nq + dim, kind)
        got = _index(Db, kind).scores(_dev(Qb, kind), "canonical").cpu().numpy()
        ref = _oracle_scores(Qb, Db, kind)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, n, nq, dim)


@pytest.mark.parametrize("kind", KINDS)
def test_canonical_scores_of_integer_operands_are_not_transposed(kind):
    """Small integers, 129 rows x 70 queries x dim 40: every score is an exact integer, the matrix is far from symmetric, so rows taken
    for queries, a transposed 4 x 4 thread tile or a swapped store index cannot pass."""
    rs = np.random.RandomState(3)
    Db = _pack(rs.randint(-8, 9, size=(129, 40)), kind)
    Qb = _pack(rs.randint(-8, 9, size=(70, 40)), kind)
    got = _index(Db, kind).scores(_dev(Qb, kind), "canonical").cpu().numpy()
    want = (_unpack(Qb, kind).astype(np.int64) @ _unpack(Db, kind).astype(np.int64).T).astype(np.float32)
    assert np.array_equal(got, want) and np.array_equal(got.view(np.uint32), _oracle_scores(Qb, Db, kind).view(np.uint32))


# ================================================================================================ 4. the second chunk of the fp64 path
def test_second_query_chunk_of_the_fp64_path():
    """dense_for_list's loop with q_begin > 0.  140 001 rows: dense_chunk_rows = (2^30 / (140 001 x 4)) rounded down to 64s = 1 856, so
    of 2 000 queries the rows 1 856 .. 1 999 are a second launch pair: dense_scores_kernel reads query q_begin + qi into scratch row qi
    and dense_select_kernel writes output row q_begin + qi.  The first chunk's score area is 1 856 x 140 001 x 4 bytes = 0.97 GiB, past
    2^30 / 4 elements, so the 64-bit row offsets are exercised too.  Probe rows (a few of the best and worst rows doubled, far apart, so
    that the cut has ties); query i is the probe query times a signed power of two that changes from query to query, so a result
    written to another row, or computed from another query, differs.  Stat: path == 0; last_stats() has no chunk count: that the
    second chunk ran is shown by rows 1 856 .. 1 999 being right."""
    n, nq, k = 140_001, 2000, 10
    digits = exact_probe_draw(n, 61, "bf16")
    order = np.argsort(-exact_probe_scores(digits, "bf16"), kind="stable")
    for src, dst in ((order[0], 70_000), (order[2], 139_999), (order[5], 64), (order[-1], 99_999), (order[-4], 140_000), (order[-7], 1)):
        for d in digits:
            d[dst] = d[src]
    scales = np.array([(-1.0) ** (i // 3) * 2.0 ** ((i * 5) % 7 - 3) for i in range(nq)])
    assert scales[1855] != scales[1856] and len(set(scales)) == 14
    Db, Qb = exact_probe_rows(digits, "bf16"), exact_probe_queries(scales, "bf16")
    index = _index(Db, "bf16")
    got = _search(index, _bf16(Qb), k, DENSE, path=0, n_dense=0)
    print("fp64 path, 2 chunks: ms_total =", index.last_stats()["ms_total"])
    ref_i, ref_s = exact_probe_topk(digits, "bf16", scales, k)
    _same(got, ref_i, ref_s, "all 2000 queries against the numpy order")
    sub = np.r_[0:3, 1850:1862, 1997:2000]
    orc_i, orc_s = orc.canonical_search(Qb[sub], Db, k)
    _same((got[0][sub], got[1][sub]), orc_i, orc_s, "oracle")


# ================================================================================================ 5. margin_select_kernel
def _with_ties(n, dim, nq, seed, kind):
    """Gaussian rows with a block of identical rows that is the top of query 0 and lies across the first tile border where there is one."""
    Db, Qb = _rand(n, dim, seed, kind), _rand(nq, dim, seed + 1, kind)
    lo = max(0, min(240, n - 40))
    Db[lo:lo + 30] = Db[lo]
    Qb[0] = Db[lo]
    return Db, Qb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [8, 64, 776])
def test_margin_select_without_a_hint(kind, dim):
    """The default search of a corpus below 16 full tiles: search_dense -> margin_for_rows(hint = null) -> margin_select_kernel's
    `!done` branch: block_radix_select<true> over the lower bounds of the whole row, the collecting scan, canonical re-score, sort.
    255 / 256 / 257 rows: one tile short, full, one row over; 1 023 and 2 049 rows: the score rows' pitch (a multiple of 4) is not
    n_rows.  k = 1, 50 and n_rows (every row is collected and re-scored).  The scratch is the plan's dense area, sized for all seven
    queries: one chunk.  Stats: path == 0 and n_dense == 0 (no query was handed on to the fp64 path).  Against the oracle and against
    the fp64 path of the same index."""
    for n in (255, 256, 257, 1023, 2049):
        Db, Qb = _with_ties(n, dim, 7, 100 * n + dim, kind)
        index, Q = _index(Db, kind), _dev(Qb, kind)
        for k in (1, 50, n):
            got = _search(index, Q, k, 0, path=0, n_dense=0, n_fallback=0)
            ref_i, ref_s = _oracle_search(Qb, Db, kind, k)
            _same(got, ref_i, ref_s, f"margin {kind} n={n} dim={dim} k={k}")
            _same(_search(index, Q, k, DENSE, path=0), ref_i, ref_s, f"fp64 {kind} n={n} dim={dim} k={k}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tied,n_dense", [(8192, 0), (8193, 3)])
def test_margin_select_cap_boundary(kind, tied, n_dense):
    """`if (n > cap || n < k) give_up()` with cap = 8 192.  Rows 100 .. 100 + tied - 1 are one vector v, the 308 others are -s v with
    0.5 <= s <= 1; three queries are v, two are -v.  For a query v the tied rows share one MFMA score near |v|^2 and are all within the
    margin of each other; another row scores -s |v|^2, below the cut by (1 + s) |v|^2 >= 1.5 |v|^2 = 1.5 / gamma = 1.9e5 units of
    gamma |q| |d| (dim 64: gamma = 64 x 2^-23 x 1.02; |d| <= |q| = |v|), so exactly `tied` rows are collected.  8 192 rows fill the key
    array to the last slot and finish on the margin path (n_dense == 0); 8 193 send exactly the three v queries to the fp64 path
    (dense_for_list with the flag list, q_begin = 0, one chunk of the plan's dense area), the two -v queries finish on the margin path.
    k = 100 keeps the planner on path 0 (its sample would be 13 of 33 full tiles).  Stats: path == 0, n_dense, n_fallback."""
    dim, k = 64, 100
    g = torch.Generator().manual_seed(71)
    v = torch.randn(dim, generator=g).numpy() * dim ** -0.5
    rs = np.random.RandomState(72)
    n = 100 + tied + 208
    s = rs.uniform(0.5, 1.0, n)
    D = -s[:, None] * v[None, :]
    D[100:100 + tied] = v
    Q = np.stack([v, -v, v, -2 * v, v])
    Db, Qb = _pack(D, kind), _pack(Q, kind)
    index = _index(Db, kind)
    got = _search(index, _dev(Qb, kind), k, 0, path=0, n_dense=n_dense, n_fallback=n_dense)
    ref_i, ref_s = _oracle_search(Qb, Db, kind, k)
    assert np.array_equal(ref_i[0], np.arange(100, 100 + k))
    _same(got, ref_i, ref_s, f"{kind} {tied} tied rows")


def _orthogonal_to(Q, v):
    return Q - (Q @ v)[:, None] * v[None, :] / float(v @ v)


_FUSED_TIES = {}


def _fused_ties_case(kind):
    """The construction of test_margin_path_small_corpus_and_flagged_queries (c) at 60 000 rows: 3 000 rows, spread over the corpus, equal
    one vector, and so do queries 17 .. 22; the other queries are orthogonal to it (up to rounding), so the tied rows are nowhere near
    THEIR cut.  Built once per element type with the fp64 path's answer left to the tests."""
    if kind not in _FUSED_TIES:
        n, dim, nq = 60_000, 128, 600
        g = torch.Generator().manual_seed(81)
        D = (torch.randn(n, dim, generator=g) * dim ** -0.5).numpy()
        Q = (torch.randn(nq, dim, generator=g) * dim ** -0.5).numpy()
        tied = np.sort(np.random.RandomState(82).choice(n, 3000, replace=False))
        v = D[tied[0]].copy()
        D[tied] = v
        Q = _orthogonal_to(Q, v.astype(np.float64)).astype(np.float32)
        Q[17:23] = v
        _FUSED_TIES[kind] = (_pack(D, kind), _pack(Q, kind), tied)
    return _FUSED_TIES[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [100, 1001])
def test_margin_select_with_the_hint_of_a_fused_search(kind, k):
    """Six queries of a fused search tie with 3 000 rows at their cut: more than the select stage re-scores (256 rows at k = 100, 2 048
    at k = 1 001), so it flags them for the exact path and complete_dense gathers them (one gather: 6 <= nq_pad) and runs
    margin_for_rows with their thresholds as the hint: margin_select_kernel's one-scan branch (tau > -inf) collects the rows whose upper
    bound reaches tau -- the 3 000 and what else a threshold below the tie lets in --, selects L among them with
    block_radix_select<false> in LDS and rebuilds the list in place (more than the 8 192 of cap: the radix branch over the whole row
    instead, which ends with the 3 000 and their near neighbours).  The score rows lie in the candidate area when that is larger than
    the 16 reserved rows, else in those; six rows fit either: one chunk.  Stats: path == 1, n_fallback == 6 and n_dense == 6; n_dense counts the queries of
    the dense list whether the margin select or the fp64 path finished them -- last_stats() cannot tell which.  (A build whose
    dense_select_kernel ranks ties by the wave's own count alone passes every check against the oracle here and fails the closing
    comparison with the fp64 path only: the margin select is what finishes these six.  The test below fails at its first check on
    that build: there the fp64 path finishes.  DESIGN 4.4.)"""
    Db, Qb, tied = _fused_ties_case(kind)
    index, Q = _index(Db, kind), _dev(Qb, kind)
    got = _search(index, Q, k, FUSED, path=1, n_fallback=6, n_dense=6)
    assert np.array_equal(got[0][17:23], np.tile(tied[:k], (6, 1)))
    sub = np.r_[0:2, 15:25, 598:600]
    ref_i, ref_s = _oracle_search(Qb[sub], Db, kind, k)
    _same((got[0][sub], got[1][sub]), ref_i, ref_s, f"{kind} k={k}")
    ids, bits = _search(index, Q, k, DENSE, path=0)                    # (last: the fp64 path is not what this test is about)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], bits)


@pytest.mark.parametrize("kind", KINDS)
def test_more_than_256_flagged_queries_reach_the_fp64_path_in_chunks(kind):
    """300 of 320 queries equal a block of 8 300 identical rows (spread over 30 000): the fused search flags them, the margin select with
    the hint collects 8 300 > cap rows, falls through to its radix branch, collects 8 300 again and gives up for every one of them, and
    complete_dense hands the list of 300 to dense_for_list: n_dense (300) exceeds the 16 reserved rows, so the fp64 path scores in the
    candidate area when that holds 64 rows of 30 000 scores or more (chunk = min(rows that fit rounded down to 64s, 256): two or more
    chunks, the later ones with q_begin > 0 AND a query list, results scattered through out_rows), else in the reserved rows (19
    chunks of 16).  last_stats() does not say which; both walk the list in several chunks.  Stats: path == 1, n_fallback == 300,
    n_dense == 300."""
    n, dim, nq, k = 30_000, 64, 320, 10
    g = torch.Generator().manual_seed(91)
    D = (torch.randn(n, dim, generator=g) * dim ** -0.5).numpy()
    Q = (torch.randn(nq, dim, generator=g) * dim ** -0.5).numpy()
    tied = np.sort(np.random.RandomState(92).choice(n, 8300, replace=False))
    v = D[tied[0]].copy()
    D[tied] = v
    Q = _orthogonal_to(Q, v.astype(np.float64)).astype(np.float32)
    same = np.setdiff1d(np.arange(nq), np.arange(7, nq, 16))          # 300 queries; every 16th from 7 on stays an ordinary one
    assert len(same) == 300
    Q[same] = v
    Db, Qb = _pack(D, kind), _pack(Q, kind)
    index, Qd = _index(Db, kind), _dev(Qb, kind)
    got = _search(index, Qd, k, FUSED, path=1, n_fallback=300, n_dense=300)
    assert np.array_equal(got[0][same], np.tile(tied[:k], (300, 1)))
    sub = np.r_[0:9, 250:262, 316:320]
    ref_i, ref_s = _oracle_search(Qb[sub], Db, kind, k)
    _same((got[0][sub], got[1][sub]), ref_i, ref_s, kind)
    ids, bits = _search(index, Qd, k, DENSE, path=0)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], bits)


# ================================================================================================ 6. run to run
def test_three_runs_are_bit_equal():
    """block_bitonic_sort_desc waits for its LDS writes to complete before each step's barrier; without the wait single keys were out of
    place in some runs.  The flat-digit case at k = 4 096 (78 sort steps over 4 096 keys, 256 threads) and the margin select at
    k = n_rows = 2 049 (4 096 keys, 1 024 threads): three runs each, bit-equal, and equal to the reference."""
    digits = _flat("bf16")
    index = _index(exact_probe_rows(digits, "bf16"), "bf16")
    Q = _bf16(exact_probe_queries(SCALES, "bf16"))
    ref_i, ref_s = exact_probe_topk(digits, "bf16", SCALES, 4096)
    for run in range(3):
        _same(_search(index, Q, 4096, DENSE, path=0), ref_i, ref_s, f"fp64 path, run {run}")
    Db, Qb = _with_ties(2049, 64, 7, 77, "bf16")
    index, Q = _index(Db, "bf16"), _bf16(Qb)
    ref_i, ref_s = orc.canonical_search(Qb, Db, 2049)
    for run in range(3):
        _same(_search(index, Q, 2049, 0, path=0, n_dense=0), ref_i, ref_s, f"margin path, run {run}")
