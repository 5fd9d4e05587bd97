"""The exact-score probe of tests/test_gpu_exact_paths.py (helpers.exact_probe_*) says what it claims, without a GPU: for the scaled and
signed rows of either element type the oracle's canonical score IS sign 2^e (a + b / 256 + c / 65536) bit for bit, fp32 sums of the three
products in either order are that number too (what an MFMA score row holds), the oracle's search is the numpy order of the integers, and
the radix select's four digits see what the probe is for: at least 100 values in each of the three low bytes, many top bytes, and more
than three top bytes inside one wave's 64 rows (hist_add_aggregated aggregates three bins per wave and falls back to plain atomics for
the rest).

The issue's fp16 form draws e from [-6, 6]: thirteen exponents are seven values of (exponent >> 1), so with both signs its score rows
hold fourteen top bytes and no more; the form with e in [-12, 6] (EXACT_PROBE_FP16_WIDE_E, still exact and normal) reaches twenty."""
import numpy as np
import pytest

from ccrec_amd import index_ref
from helpers import (EXACT_PROBE, EXACT_PROBE_FP16_WIDE_E, exact_probe_draw, exact_probe_queries, exact_probe_rows, exact_probe_scores,
                     exact_probe_topk, f32_orderable)
from oracle import oracle as orc

N = 5000
SCALES = (1.0, -1.0, 8.0, -0.25)
FORMS = [("bf16", None, 20), ("fp16", None, 14), ("fp16", EXACT_PROBE_FP16_WIDE_E, 20)]


def _oracle_scores(Qb, Db, kind):
    return orc.canonical_scores(Qb, Db) if kind == "bf16" else index_ref.canonical_scores(Qb, Db, "fp16")


def _oracle_search(Qb, Db, kind, k):
    return orc.canonical_search(Qb, Db, k) if kind == "bf16" else index_ref.canonical_search(Qb, Db, "fp16", k)


def test_orderable_keys_order_like_the_values():
    x = np.array([-np.inf, -3.0, -2.0 ** -130, -0.0, 0.0, 2.0 ** -130, 1.0, 1.0000001, np.inf], np.float32)
    key = f32_orderable(x)
    assert np.all(np.diff(key.astype(np.int64)) > 0)


@pytest.mark.parametrize("kind,e_range,min_top", FORMS)
def test_probe_scores_are_the_chosen_digits(kind, e_range, min_top):
    digits = exact_probe_draw(N, 7, kind, e_range)
    sign, e, a, b, c = digits
    Db, Qb = exact_probe_rows(digits, kind, e_range=e_range), exact_probe_queries(SCALES, kind)
    want = exact_probe_scores(digits, kind)
    q0 = EXACT_PROBE[kind]["query"][0]
    assert np.array_equal(want.astype(np.float64), sign * np.exp2((e + q0).astype(np.float64)) * (a + b / 256.0 + c / 65536.0))
    got = _oracle_scores(Qb, Db, kind)
    for r, s in enumerate(SCALES):
        assert np.array_equal(got[r].view(np.uint32), (np.float32(s) * want).view(np.uint32)), (kind, s)
    # fp32 accumulation of the three exact products, ascending and descending: every partial sum is exact
    q, d = index_ref.unpack(Qb[:1], kind)[0], index_ref.unpack(Db, kind)
    prod = [(d[:, i] * q[i]).astype(np.float32) for i in range(3)]
    assert all(np.array_equal(p.astype(np.float64), d[:, i].astype(np.float64) * float(q[i])) for i, p in enumerate(prod))
    assert np.array_equal(((prod[0] + prod[1]) + prod[2]).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(((prod[2] + prod[1]) + prod[0]).view(np.uint32), want.view(np.uint32))
    # the bytes of the pattern are the digits
    u = want.view(np.uint32)
    assert np.array_equal(u & 0xFF, c) and np.array_equal((u >> 8) & 0xFF, b) and np.array_equal((u >> 16) & 0x7F, a & 0x7F)
    assert np.array_equal(u >> 31, (sign < 0).astype(np.uint32))
    # the search of the oracle is the numpy order of the integers
    k = 257
    ref_i, ref_s = _oracle_search(Qb, Db, kind, k)
    ids, sc = exact_probe_topk(digits, kind, SCALES, k)
    assert np.array_equal(ref_i, ids) and np.array_equal(ref_s.view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(ids[0], np.lexsort((np.arange(N), -want))[:k])


@pytest.mark.parametrize("kind,e_range,min_top", FORMS)
def test_probe_fills_every_digit_of_the_radix_select(kind, e_range, min_top):
    digits = exact_probe_draw(N, 7, kind, e_range)
    key = f32_orderable(exact_probe_scores(digits, kind))
    low = [len(np.unique((key >> np.uint32(shift)) & np.uint32(0xFF))) for shift in (16, 8, 0)]
    print(kind, e_range, "distinct values of the three low bytes:", low)
    assert min(low) >= 100
    assert low[0] >= 128 and low[1:] == [256, 256]
    top = (key >> np.uint32(24)).astype(np.int64)
    n_top = len(np.unique(top))
    lo, hi = e_range or EXACT_PROBE[kind]["e"]
    bias = 127 + 7 + EXACT_PROBE[kind]["query"][0]
    possible = 2 * len({(bias + x) >> 1 for x in range(lo, hi + 1)})
    print(kind, e_range, "top bytes:", n_top, "of", possible, "possible")
    assert n_top == possible >= min_top
    if e_range is None and kind == "fp16":
        assert possible == 14      # thirteen exponents cannot give more: see the module docstring
    per_wave = [len(np.unique(top[i:i + 64])) for i in range(0, N - 63, 64)]
    assert max(per_wave) > 3 and min(per_wave) > 3
