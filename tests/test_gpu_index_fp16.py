"""An index of fp16 rows (opt-in; bf16 stays the default): the pack equals torch's conversion bit for bit and counts what left the
type's range, EVERY search path returns the ids and score bits of ccrec_amd/index_ref.py, the operand type is exact (11-bit
significands, subnormals), the contract errors are raised, and the public ranking paths follow CCREC_INDEX_DTYPE.  Inputs are explicit
fp16 bit patterns (_f16), paths are pinned with the knobs of tests/test_gpu_wide.py and asserted from last_stats()."""
import os

import numpy as np
import pytest
import torch

from ccrec_amd import index_ref
from oracle import oracle as orc
from test_cpu_index_ref import edge_table, torch_bits
from test_gpu_wide import DENSE, FUSED, _bf16, _knobs

pytestmark = pytest.mark.gpu

OFFSET = 4321
U = 2.0 ** -11                       # unit roundoff of fp16


def _f16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.float16).cuda()


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _rand_f16(n, d, seed, scale=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g) * (scale if scale is not None else d ** -0.5)
    return index_ref.pack(x.numpy(), "fp16")


# the knobs that pin a main-pass kernel, and what last_stats() reports when it ran
WIDE = ({"CCR_WIDE": 1, "CCR_NARROW": 0}, FUSED, {"path": 1, "main_tile_queries": 384})
TILE256 = ({"CCR_WIDE": 0, "CCR_NARROW": 0}, FUSED, {"path": 1, "main_tile_queries": 256})
NARROW = ({"CCR_NARROW": 1}, FUSED, {"path": 1, "main_tile_queries": 0})
DENSE_PATH = ({}, DENSE, {"path": 0})
PLANNER = ({}, FUSED, {"path": 1})    # no kernel pinned: the planner's own tile (the flag only keeps it off the dense path, which has its own case)


def _index(Db, knobs, offset=OFFSET):
    from ccrec_amd import ops
    with _knobs(**knobs):
        return ops.CorpusIndex(_f16(Db), global_row_offset=offset)


_REF = {}


def _reference(key, Qb, Db, k):
    """index_ref's answer, computed once per case and shared (never modified)."""
    if key not in _REF:
        _REF[key] = index_ref.canonical_search(Qb, Db, "fp16", k)
    return _REF[key]


def _search_equals(index, how, Qb, ref, k):
    _, flags, want = how
    s, i = index.search(_f16(Qb), k, flags)
    st = index.last_stats()
    for name, v in want.items():
        assert st[name] == v, (name, st)
    ref_i, ref_s = ref
    got_i, got_s = i.cpu().numpy() - index.offset, s.cpu().numpy()
    assert np.array_equal(got_i, ref_i), f"ids differ in {np.sum(got_i != ref_i)} places"
    assert np.array_equal(got_s.view(np.uint32), ref_s.view(np.uint32))
    return st


# ================================================================================================ 1. pack
def test_pack_half_equals_torch_bit_for_bit():
    from ccrec_amd import ops
    tab = edge_table()
    x = np.zeros((8, 8), np.float32)                      # the table in rows of eight
    x.reshape(-1)[:tab.size] = tab
    for dtype, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        got = _bits(ops.pack_half(torch.from_numpy(x).cuda(), dtype))
        want, nan = torch_bits(x, name), np.isnan(x)
        assert np.array_equal(got[~nan], want[~nan]), name
        assert np.all(np.isnan(index_ref.unpack(got[nan], name)))
        assert np.array_equal(got[~nan], index_ref.pack(x, name)[~nan])
    g = (torch.randn(5000, 768, generator=torch.Generator().manual_seed(1)) / 768 ** 0.5)
    got = ops.pack_half(g.cuda(), torch.float16)
    assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16).cpu(), g.to(torch.float16).view(torch.int16))
    # the subnormals of that scale are there and kept
    sub = (got.float().abs() < 2.0 ** -14) & (got != 0)
    assert int(sub.sum()) > 1000
    # with row-norm bounds (another kernel): same bits, bounds >= the packed rows' norms
    nb = torch.empty(5000, device="cuda")
    got2 = ops.pack_half(g.cuda(), torch.float16, norm_bounds=nb)
    assert torch.equal(got2, got)
    true = got.double().norm(dim=1)
    assert torch.all(true <= nb.double()) and torch.all(nb.double() <= true * 1.001 + 1e-30)
    # old name, old result
    assert torch.equal(ops.pack_bf16(g.cuda()).view(torch.int16).cpu(), g.to(torch.bfloat16).view(torch.int16))


def test_pack_half_width_40_shard_slice_normalising_form_and_bounds():
    from ccrec_amd import ops
    rs = np.random.RandomState(2)
    x = (rs.randn(300, 40) * 0.2).astype(np.float32)
    x[5] = 0.0
    x[6] *= 2.0 ** -20                                                        # a row of subnormal results
    # width 40 is a multiple of 8; 37 is not: zero-padded to 40
    for width in (40, 37):
        xw = np.ascontiguousarray(x[:, :width])
        shard = torch.full((1000, 40), 7.0, dtype=torch.float16, device="cuda")
        nb = torch.full((1000,), -1.0, device="cuda")
        out, norms = ops.pack_half(torch.from_numpy(xw).cuda(), torch.float16, out=shard[100:400], return_norms=True, norm_bounds=nb[100:400])
        got = _bits(shard)
        want = np.zeros((300, 40), np.uint16)
        want[:, :width] = index_ref.pack(xw, "fp16")
        assert np.array_equal(got[100:400], want) and out.data_ptr() == shard[100:400].data_ptr()
        assert np.all(got[:100] == got[0, 0]) and np.all(got[400:] == got[0, 0]) and got[0, 0] == 0x4700     # the rest of the shard: untouched
        assert np.array_equal(norms.cpu().numpy().view(np.uint32), index_ref.row_norms(xw).view(np.uint32))
        true = np.sqrt((index_ref.unpack(want, "fp16").astype(np.float64) ** 2).sum(1))
        b = nb.cpu().numpy()
        assert np.all(true <= b[100:400]) and np.all(b[:100] == -1.0) and np.all(b[400:] == -1.0)
        # the normalising form against index_ref, bit for bit (the library's reduction order)
        nb2 = torch.empty(300, device="cuda")
        outn = ops.pack_half(torch.from_numpy(xw).cuda(), torch.float16, normalize=True, norm_bounds=nb2)
        wantn = np.zeros((300, 40), np.uint16)
        wantn[:, :width] = index_ref.normalize_pack(xw, "fp16")
        assert np.array_equal(_bits(outn), wantn)
        truen = np.sqrt((index_ref.unpack(wantn, "fp16").astype(np.float64) ** 2).sum(1))
        assert np.all(truen <= nb2.cpu().numpy()) and np.all(nb2.cpu().numpy() <= 1.01)


@pytest.mark.parametrize("form", ["plain", "bounds", "norms", "padded"])
def test_pack_half_counts_what_left_the_range(form):
    from ccrec_amd import ops
    rs = np.random.RandomState(4)
    width = 37 if form == "padded" else 64
    x = rs.randn(700, width).astype(np.float32)
    planted = [(0, 0, 65520.0), (3, 5, -1e5), (3, 6, 7e4), (699, width - 1, 3e38), (350, 17, -65520.0), (351, 1, 65519.996), (352, 2, np.inf),
               (353, 3, np.nan), (354, 4, -np.inf), (355, 5, 65504.0)]
    for r, c, v in planted:
        x[r, c] = v
    n_out = 5                                                                  # finite and beyond the range: the first five
    assert index_ref.overflow_count(x) == n_out
    xs = torch.from_numpy(x).cuda()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = {"bounds": {"norm_bounds": torch.empty(700, device="cuda")}, "norms": {"return_norms": True}}.get(form, {})
    out = ops.pack_half(xs, torch.float16, overflow=counter, **kw)
    out = out[0] if isinstance(out, tuple) else out
    assert int(counter.item()) == n_out
    got = out.float().cpu().numpy()
    assert np.isinf(got[0, 0]) and np.isinf(got[3, 5]) and got[3, 5] < 0 and got[351, 1] == 65504.0 and np.isnan(got[353, 3])
    if form == "bounds":                                                       # a row that holds an inf has an infinite bound
        b = kw["norm_bounds"].cpu().numpy()
        assert np.isinf(b[0]) and np.isinf(b[3]) and np.isinf(b[352]) and np.isfinite(b[1])
    ops.pack_half(xs, torch.float16, overflow=counter, **kw)                   # the counter accumulates over the packs of a build
    assert int(counter.item()) == 2 * n_out
    # the normalising form of the same (finite) rows: nothing leaves the range
    finite = np.where(np.isfinite(x), x, 1.0).astype(np.float32)
    counter.zero_()
    ops.pack_half(torch.from_numpy(finite).cuda(), torch.float16, normalize=True, overflow=counter)
    assert int(counter.item()) == 0
    # bf16 never touches the counter
    ops.pack_half(xs, torch.bfloat16, overflow=counter)
    assert int(counter.item()) == 0


def test_meanpool_pack_fp16_equals_pool_then_pack():
    from ccrec_amd import ops
    B, L, d = 3, 16, 768
    g = torch.Generator().manual_seed(6)
    hidden = (torch.randn(B, L, d, generator=g) * 0.3).cuda()
    hidden[1, 2, 7] = 9e5                                                       # pooled over 4 tokens: still beyond 65 504
    lens = torch.tensor([16, 4, 9])
    mask = (torch.arange(L)[None, :] < lens[:, None]).long().cuda()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    f32, h16 = ops.meanpool_pack(hidden, mask, dtype=torch.float16, overflow=counter)
    assert h16.dtype == torch.float16
    assert np.array_equal(f32.cpu().numpy().view(np.uint32), orc.meanpool(hidden.cpu().numpy(), mask.cpu().numpy()).view(np.uint32))
    want = ops.pack_half(f32, torch.float16)
    assert torch.equal(h16.view(torch.int16), want.view(torch.int16)) and int(counter.item()) == 1
    # the packed-token form: the same real tokens, no padding rows
    rows = torch.cat([hidden[b, :int(lens[b])] for b in range(B)]).contiguous()
    start = torch.tensor([0, 16, 20], dtype=torch.int32, device="cuda")
    out32 = torch.empty(B, d, device="cuda")
    nb = torch.empty(B, device="cuda")
    _, p16 = ops.meanpool_pack_packed(rows, start, lens.to(torch.int32).cuda(), out_f32=out32,
                                      out_bf16=torch.empty(B, d, dtype=torch.float16, device="cuda"), norm_bounds=nb, dtype=torch.float16,
                                      overflow=counter)
    assert torch.equal(p16.view(torch.int16), want.view(torch.int16)) and torch.equal(out32, f32) and int(counter.item()) == 2
    assert np.isinf(nb.cpu().numpy()[1]) and torch.all(p16[[0, 2]].double().norm(dim=1) <= nb[[0, 2]].double())
    # default dtype: today's bf16 result
    _, b16 = ops.meanpool_pack(hidden, mask)
    assert b16.dtype == torch.bfloat16 and torch.equal(b16.view(torch.int16), ops.pack_bf16(f32).view(torch.int16))


# ================================================================================================ 2. every search path
SEARCH_CASES = [
    ("wide", WIDE, (300, 200, 32, 10)), ("wide", WIDE, (513, 385, 64, 5)), ("wide", WIDE, (20_000, 300, 768, 100)),
    ("256", TILE256, (513, 385, 64, 5)), ("256", TILE256, (9000, 130, 32, 5)), ("256", TILE256, (4133, 70, 96, 17)),
    ("256", TILE256, (3000, 90, 40, 7)),
    ("narrow", NARROW, (4133, 1, 96, 17)), ("narrow", NARROW, (4133, 64, 96, 17)), ("narrow", NARROW, (70_000, 16, 768, 100)),
    ("dense", DENSE_PATH, (513, 385, 64, 5)),
    ("large-k", PLANNER, (40_000, 770, 128, 1001)),
]


def _case_data(n, nq, d):
    if d == 40:   # a width that needs the pack's zero padding: 37 -> 40
        from ccrec_amd import ops
        g = torch.Generator().manual_seed(n)
        D, Q = torch.randn(n, 37, generator=g) * 37 ** -0.5, torch.randn(nq, 37, generator=g) * 37 ** -0.5
        Db, Qb = _bits(ops.pack_half(D.cuda(), torch.float16)), _bits(ops.pack_half(Q.cuda(), torch.float16))
        assert Db.shape[1] == 40 and not Db[:, 37:].any()
        return Db, Qb
    return _rand_f16(n, d, n + 3), _rand_f16(nq, d, nq + 5)


@pytest.mark.parametrize("label,how,shape", SEARCH_CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[2]))}" for c in SEARCH_CASES])
def test_every_search_path_equals_index_ref(label, how, shape):
    n, nq, d, k = shape
    Db, Qb = _case_data(n, nq, d)
    ref = _reference((n, nq, d, k), Qb, Db, k)
    index = _index(Db, how[0])
    assert index.dtype == torch.float16
    st = _search_equals(index, how, Qb, ref, k)
    print(label, shape, st)


def _special_setup(n, nq, d, seed):
    Db, Qb = _rand_f16(n, d, seed), _rand_f16(nq, d, seed + 1)
    return Db, Qb, _index(Db, {}, offset=0)


def test_search_blocked_on_an_fp16_index():
    n, nq, d, k = 5000, 4, 64, 10
    Db, Qb, index = _special_setup(n, nq, d, 40)
    rs = np.random.RandomState(1)
    top = index_ref.canonical_search(Qb, Db, "fp16", 4200)[0]
    # lengths 0, 3 (inside the top-10), one longer than the over-fetch limit (k + len > 4096: the dense route), and 3 again
    block = [[], sorted(top[1][[0, 4, 9]].tolist()), sorted(top[2][:4100].tolist()), sorted(rs.choice(n, 3, replace=False).tolist())]
    ptr = np.cumsum([0] + [len(b) for b in block])
    idx = np.concatenate([np.asarray(b, np.int64) for b in block])
    s, i = index.search_blocked(_f16(Qb), k, ptr, idx)
    ref_i, ref_s = index_ref.canonical_search(Qb, Db, "fp16", k, block)
    assert np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))
    assert not set(ref_i[1].tolist()) & set(block[1])


def test_search_sparse_prior_on_an_fp16_index():
    n, nq, d, k = 6000, 3, 64, 10
    Db, Qb, index = _special_setup(n, nq, d, 50)
    rs = np.random.RandomState(2)
    cols = [np.sort(rs.choice(n, 4096, replace=False)), np.zeros(0, np.int64), np.sort(rs.choice(n, 5, replace=False))]   # 4 096 priors, none, a few
    vals = [rs.randn(len(c)) * 0.5 for c in cols]
    ptr = np.cumsum([0] + [len(c) for c in cols])
    idx, val = np.concatenate(cols).astype(np.int64), np.concatenate(vals)
    s, i = index.search_sparse_prior(_f16(Qb), k, ptr, idx, val)
    ref_i, ref_s = index_ref.sparse_prior_search(Qb, Db, "fp16", ptr, idx, val, k)
    assert np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(s.cpu().numpy().view(np.uint64), ref_s.view(np.uint64))


def test_two_fp16_shards_merge_to_the_single_index_search():
    from ccrec_amd import ops
    n, nq, d, k = 4133, 70, 96, 17
    Db, Qb = _case_data(n, nq, d)
    ref = _reference((n, nq, d, k), Qb, Db, k)
    Q = _f16(Qb)
    nbytes = ops.shard_message_bytes(nq, k)
    gathered = torch.zeros(2 * nbytes, dtype=torch.uint8, device="cuda")
    for r, (lo, hi) in enumerate(((0, 2000), (2000, 4133))):
        shard = ops.CorpusIndex(_f16(Db[lo:hi]), global_row_offset=lo)
        shard.search_shard(Q, k, gathered[r * nbytes:(r + 1) * nbytes])
    s, i = ops.merge_shard_messages(gathered, 2, nq, k)
    assert np.array_equal(i.cpu().numpy(), ref[0]) and np.array_equal(s.cpu().numpy().view(np.uint32), ref[1].view(np.uint32))
    # colsum follows the tensor it is given
    want = index_ref.unpack(Db, "fp16").astype(np.float64).sum(0)
    np.testing.assert_allclose(ops.colsum_bf16(_f16(Db)).cpu().numpy(), want, rtol=1e-12, atol=1e-12)


def _gamma(dim):
    return dim * 2.0 ** -23 * 1.02


@pytest.mark.parametrize("dim", [768, 4096])
def test_scores_canonical_bits_and_the_mfma_margin(dim):
    """scores() canonical = index_ref's bits; MFMA mode: max |mfma - canonical| / (||q|| ||d||) is measured and asserted against the
    filter margin's gamma = dim 2^-23 1.02 -- the bound nobody had measured on v_mfma_f32_*_f16.
    The measured ratios are recorded in DESIGN 4.3."""
    from ccrec_amd import ops
    Db, Qb = _rand_f16(700, dim, 1), _rand_f16(37, dim, 2)
    index = ops.CorpusIndex(_f16(Db))
    can = index.scores(_f16(Qb), "canonical").cpu().numpy()
    ref = index_ref.canonical_scores(Qb, Db, "fp16")
    assert np.array_equal(can.view(np.uint32), ref.view(np.uint32))
    mf = index.scores(_f16(Qb), "mfma").cpu().numpy().astype(np.float64)
    q, d = index_ref.unpack(Qb, "fp16").astype(np.float64), index_ref.unpack(Db, "fp16").astype(np.float64)
    exact = q @ d.T
    ratio = np.abs(mf - exact) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(d, axis=1)[None, :])
    print(f"dim {dim}: max |mfma - exact| / (|q||d|) = {ratio.max():.3e}, gamma = {_gamma(dim):.3e}, fraction = {ratio.max() / _gamma(dim):.3e}")
    assert ratio.max() <= _gamma(dim)
    # exact-integer operands (asymmetric): the f16 MFMA product must be exact -> catches any layout transposition
    rs = np.random.RandomState(3)
    Di = index_ref.pack(rs.randint(-8, 9, size=(515, 128)).astype(np.float32), "fp16")
    Qi = index_ref.pack(rs.randint(-8, 9, size=(261, 128)).astype(np.float32), "fp16")
    mf2 = ops.CorpusIndex(_f16(Di)).scores(_f16(Qi), "mfma").cpu().numpy()
    assert np.array_equal(mf2, index_ref.canonical_scores(Qi, Di, "fp16"))


# ================================================================================================ 3. exactness of the operand type
ALL_PATHS = [WIDE, TILE256, NARROW, DENSE_PATH]


def test_g5_exact_ties_on_every_path(golden_dir):
    from helpers import canonicalise
    g = np.load(os.path.join(golden_dir, "g5_ranking_exact_ties.npz"))     # multiples of 1/8: representable in both types
    Db, Qb = index_ref.pack(g["Ed"], "fp16"), index_ref.pack(g["Eq"], "fp16")
    assert np.array_equal(index_ref.unpack(Db, "fp16"), g["Ed"]) and np.array_equal(index_ref.unpack(Qb, "fp16"), g["Eq"])
    ri, rs = canonicalise(g["ids"], g["scores"])
    # the fused kernels take what one sampled tile can bound (400 rows = one full tile = 16 groups: k <= 16) -- a prefix of the canonical
    # list is the canonical shorter list --; the dense path takes the whole golden ranking
    for how in ALL_PATHS:
        k = ri.shape[1] if how is DENSE_PATH else 16
        _search_equals(_index(Db, how[0]), how, Qb, (ri[:, :k], rs[:, :k]), k)


def _one_column(values, dim, col):
    x = np.zeros((len(values), dim), np.float32)
    x[:, col] = values
    return x


@pytest.mark.parametrize("how", ALL_PATHS, ids=["wide", "256", "narrow", "dense"])
def test_eleven_bit_significands_are_not_truncated(how):
    """Rows 1 + j 2^-10, j = 0 .. 599 (600 > 512: values up to 1.585, all exact in fp16) in one column: any bf16 truncation anywhere
    collapses them into ties and the top-5 fails."""
    D = _one_column(1.0 + np.arange(600) * 2.0 ** -10, 64, 13)
    Q = _one_column([1.0], 64, 13)
    Db, Qb = index_ref.pack(D, "fp16"), index_ref.pack(Q, "fp16")
    assert np.array_equal(index_ref.unpack(Db, "fp16"), D)
    ref_i = np.arange(599, 594, -1)[None, :]
    ref_s = D[ref_i[0], 13][None, :].astype(np.float32)
    _search_equals(_index(Db, how[0]), how, Qb, (ref_i, ref_s), 5)


@pytest.mark.parametrize("how", [WIDE, TILE256, NARROW], ids=["wide", "256", "narrow"])
def test_fp16_subnormal_operands_are_not_flushed(how):
    """Row j holds (j + 1) 2^-24 -- a subnormal for j < 1023 -- and the query 1 024 in that column: the scores are (j + 1) 2^-14.  A
    kernel that flushed subnormal MFMA operands would score every row 0 and lose them (ties: rows 0 .. 4)."""
    D = _one_column((np.arange(600) + 1) * 2.0 ** -24, 64, 21)
    Q = _one_column([1024.0], 64, 21)
    Db, Qb = index_ref.pack(D, "fp16"), index_ref.pack(Q, "fp16")
    assert np.array_equal(Db[:, 21], np.arange(1, 601, dtype=np.uint16))        # the subnormal bit patterns themselves
    ref_i = np.arange(599, 594, -1)[None, :]
    ref_s = ((ref_i + 1) * 2.0 ** -14).astype(np.float32)
    index = _index(Db, how[0])
    _search_equals(index, how, Qb, (ref_i, ref_s), 5)
    mf = index.scores(_f16(Qb), "mfma").cpu().numpy()
    assert np.array_equal(mf[0], ((np.arange(600) + 1) * 2.0 ** -14).astype(np.float32))


def test_mass_ties_and_duplicates_fall_back_exactly_fp16():
    rs = np.random.RandomState(5)
    n, d = 12000, 128
    D = rs.randint(-4, 5, size=(n, d)).astype(np.float32) / 4
    D[2000:9000] = D[17]                    # 7001 identical rows
    Q = rs.randint(-4, 5, size=(5, d)).astype(np.float32) / 4
    Q[0] = D[17]                             # its top-k is inside the tie
    Db, Qb = index_ref.pack(D, "fp16"), index_ref.pack(Q, "fp16")
    ref = index_ref.canonical_search(Qb, Db, "fp16", 100)
    orc_i, orc_s = orc.canonical_search(orc.pack_bf16(Q), orc.pack_bf16(D), 100)     # exact in both types: the oracle's answer too
    assert np.array_equal(ref[0], orc_i) and np.array_equal(ref[1].view(np.uint32), orc_s.view(np.uint32))
    index = _index(Db, {})
    st = _search_equals(index, ({}, FUSED, {"path": 1}), Qb, ref, 100)
    assert st["n_fallback"] >= 1, st
    _search_equals(index, DENSE_PATH, Qb, ref, 100)


def test_non_finite_rows_do_not_fault_and_are_path_independent_fp16():
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(1)
    for n in (20000, 400):
        D = torch.randn(n, 128, generator=g) / 128 ** 0.5
        Q = torch.randn(6, 128, generator=g) / 128 ** 0.5
        D[5] = float("nan")
        D[7] = float("inf")
        D[9, 3] = float("-inf")
        D[11, 2] = 1e5                                   # finite in fp32, inf in fp16
        Q[2] = float("nan")
        index = ops.CorpusIndex(ops.pack_half(D.cuda(), torch.float16))
        Qh = ops.pack_half(Q.cuda(), torch.float16)
        s_f, i_f = index.search(Qh, 10, FUSED)
        st = index.last_stats()
        s_d, i_d = index.search(Qh, 10, DENSE)
        assert st["path"] == 1 and st["n_fallback"] == 6, st
        assert torch.equal(i_f, i_d) and torch.equal(s_f.view(torch.int32), s_d.view(torch.int32))
        finite = torch.isfinite(s_f[0])
        assert finite.sum() >= 6 and torch.all(s_f[0][finite][:-1] >= s_f[0][finite][1:])


# ================================================================================================ 4. contract and errors
def test_contract_and_errors():
    from ccrec_amd import ops, _lib
    Db = _rand_f16(100, 64, 1)
    index = ops.CorpusIndex(_f16(Db))
    assert index.dtype == torch.float16 and index.library_dtype() == torch.float16
    bf = ops.CorpusIndex(_bf16(orc.pack_bf16(np.ones((100, 64), np.float32))))
    assert bf.dtype == torch.bfloat16 and bf.library_dtype() == torch.bfloat16
    q_bf = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    q_h = torch.zeros(2, 64, dtype=torch.float16, device="cuda")
    for call in (lambda: index.search(q_bf, 5), lambda: index.scores(q_bf), lambda: index.search_blocked(q_bf, 5, [0, 0, 0], []),
                 lambda: index.search_shard(q_bf, 5, torch.zeros(ops.shard_message_bytes(2, 5), dtype=torch.uint8, device="cuda")),
                 lambda: bf.search(q_h, 5)):
        with pytest.raises(TypeError, match=r"(?s)float16.*bfloat16|bfloat16.*float16"):
            call()
    with pytest.raises(TypeError):
        ops.CorpusIndex(torch.zeros(4, 8, device="cuda"))                                     # fp32 rows
    with pytest.raises(_lib.CcrError):
        ops.CorpusIndex(torch.zeros(4, 12, dtype=torch.float16, device="cuda"))                # dim % 8 != 0
    with pytest.raises(_lib.CcrError):
        index.search(_f16(_rand_f16(2, 64, 2)), 101)                                           # k > n_rows
    lib = ops.require_gpu()
    h = __import__("ctypes").c_void_p()
    assert lib.ccr_index_create_half(ops._ptr(index.corpus), 100, 64, 0, 0, None, __import__("ctypes").byref(h)) == _lib.CCR_ERR_INVALID   # CCR_DTYPE_F32
    assert lib.ccr_version() >= 109 and lib.ccr_index_dtype(None) == -1
    s, i = index.search(torch.empty(0, 64, dtype=torch.float16, device="cuda"), 5)
    assert s.shape == (0, 5) and i.shape == (0, 5)


def test_old_style_bf16_index_returns_the_same_bits_as_before():
    from ccrec_amd import ops
    n, nq, d, k = 513, 385, 64, 5
    g = torch.Generator().manual_seed(n)
    Db = orc.pack_bf16((torch.randn(n, d, generator=g) * d ** -0.5).numpy())
    Qb = orc.pack_bf16((torch.randn(nq, d, generator=g) * d ** -0.5).numpy())
    ref_i, ref_s = orc.canonical_search(Qb, Db, k, None)
    for knobs, flags, want in (WIDE, TILE256, DENSE_PATH):
        with _knobs(**knobs):
            index = ops.CorpusIndex(_bf16(Db), global_row_offset=OFFSET)
        s, i = index.search(_bf16(Qb), k, flags)
        st = index.last_stats()
        assert all(st[name] == v for name, v in want.items()), st
        assert np.array_equal(i.cpu().numpy() - OFFSET, ref_i) and np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


# ================================================================================================ 5. through the public API
@pytest.fixture
def index_dtype_env():
    old = {k: os.environ.get(k) for k in ("CCREC_INDEX_DTYPE", "CCREC_SIM_TYPE")}
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _ranking(Eq, Ed, sim, batch_size):
    from ccrec_amd.ms_marco_eval import ranking
    os.environ["CCREC_SIM_TYPE"] = sim
    nq, nd = Eq.shape[0], Ed.shape[0]
    table = torch.cat([torch.from_numpy(Eq), torch.from_numpy(Ed)], 0)
    queries = {f"q{i}": i for i in range(nq)}
    corpus = {f"p{j}": nq + j for j in range(nd)}
    prof = ranking(corpus, queries, lambda rows: table[torch.as_tensor(rows, dtype=torch.long)], batch_size)
    ids = np.array([[int(p[1:]) for p in prof[f"q{i}"]] for i in range(nq)], np.int64)
    sc = np.array([list(prof[f"q{i}"].values()) for i in range(nq)], np.float32)
    return ids, sc


@pytest.mark.parametrize("name,sim", [("g1_ranking_dot.npz", "dot"), ("g2_ranking_cos.npz", "cos")])
def test_ranking_follows_the_index_dtype_switch(golden_dir, index_dtype_env, name, sim):
    g = np.load(os.path.join(golden_dir, name))
    Eq, Ed = g["Eq"], g["Ed"]
    os.environ["CCREC_INDEX_DTYPE"] = "fp16"
    ids, sc = _ranking(Eq, Ed, sim, int(g["batch_size"]))
    # bit for bit what index_ref says about the fp16 rows
    pk = index_ref.normalize_pack if sim == "cos" else index_ref.pack
    ref_i, ref_s = index_ref.canonical_search(pk(Eq, "fp16"), pk(Ed, "fp16"), "fp16", ids.shape[1])
    assert np.array_equal(ids, ref_i) and np.array_equal(sc.view(np.uint32), ref_s.view(np.uint32))
    # against the reference's fp32 scores: each operand rounded once (relative u) plus the absolute error 2^-24 of a subnormal result
    q, d = Eq.astype(np.float64), Ed.astype(np.float64)
    if sim == "cos":
        q, d = q / np.linalg.norm(q, axis=1, keepdims=True), d / np.linalg.norm(d, axis=1, keepdims=True)
    bound = ((2 * U + U * U) * np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(d, axis=1)[None, :]
             + 2.0 ** -24 * (np.abs(q).sum(1)[:, None] + np.abs(d).sum(1)[None, :]))            # [nq, nd], per pair
    gi, gs = g["ids"], g["scores"].astype(np.float64)
    worst, n_clear = 0.0, 0
    for r in range(ids.shape[0]):
        ours = np.empty(Ed.shape[0])
        ours[ids[r]] = sc[r]
        err = np.abs(ours[gi[r]] - gs[r])
        worst = max(worst, float((err / bound[r, gi[r]]).max()))
        assert np.all(err <= bound[r, gi[r]]), (r, float((err / bound[r, gi[r]]).max()))
        b = bound[r].max()
        gap_prev, gap_next = np.r_[np.inf, gs[r][:-1] - gs[r][1:]], np.r_[gs[r][:-1] - gs[r][1:], np.inf]
        clear = (gap_prev > 2 * b) & (gap_next > 2 * b)
        n_clear += int(clear.sum())
        assert np.array_equal(ids[r][clear], gi[r][clear])
    print(name, "worst |fp16 score - golden| / bound =", worst, " ranks pinned by their gaps:", n_clear)
    # the variable unset: today's bf16 result
    del os.environ["CCREC_INDEX_DTYPE"]
    ids_b, sc_b = _ranking(Eq, Ed, sim, int(g["batch_size"]))
    orc_i, orc_s = orc.canonical_ranking(Eq, Ed, sim)
    assert np.array_equal(ids_b, orc_i) and np.array_equal(sc_b.view(np.uint32), orc_s.view(np.uint32))


def test_ranking_raises_on_fp16_overflow_under_dot_and_ranks_under_cos(index_dtype_env):
    rs = np.random.RandomState(8)
    Eq, Ed = rs.randn(3, 64).astype(np.float32), rs.randn(40, 64).astype(np.float32)
    Ed[7, 5] = 1e5
    Ed[30, 0] = -1e5
    os.environ["CCREC_INDEX_DTYPE"] = "fp16"
    with pytest.raises(OverflowError, match=r"2 embedding.*bf16.*CCREC_SIM_TYPE=cos"):
        _ranking(Eq, Ed, "dot", 16)
    ids, sc = _ranking(Eq, Ed, "cos", 16)
    ref_i, ref_s = index_ref.canonical_search(index_ref.normalize_pack(Eq, "fp16"), index_ref.normalize_pack(Ed, "fp16"), "fp16", 40)
    assert np.array_equal(ids, ref_i) and np.array_equal(sc.view(np.uint32), ref_s.view(np.uint32))
    os.environ["CCREC_INDEX_DTYPE"] = "bf16"
    ids, sc = _ranking(Eq, Ed, "dot", 16)                 # bf16 has fp32's range
    assert np.all(np.isfinite(sc))
    os.environ["CCREC_INDEX_DTYPE"] = "half"
    with pytest.raises(ValueError, match="CCREC_INDEX_DTYPE"):
        _ranking(Eq, Ed, "dot", 16)


def test_length_sorted_encoder_and_retriever_under_fp16(index_dtype_env):
    from ccrec_amd.encode import LengthSortedEncoder
    from ccrec_amd.ms_marco_eval import Retriever
    from test_gpu_encode import ToyTokenizer, _texts, _tower
    tower, tok = _tower(), ToyTokenizer()
    texts, qtexts = _texts(333, 1), _texts(9, 2)
    os.environ["CCREC_INDEX_DTYPE"] = "fp16"
    enc = LengthSortedEncoder(tower, tok, max_length=32, max_tokens=1024, max_batch=64)
    try:
        d32 = torch.zeros(len(texts), 64, device="cuda")
        q32 = torch.zeros(len(qtexts), 64, device="cuda")
        nb = torch.empty(len(texts), device="cuda")
        from ccrec_amd import ops
        overflow = ops.IndexOverflow(torch.float16, "cuda")
        shard = enc.encode(texts, sim="dot", out_f32=d32, norm_bounds=nb, overflow=overflow)
        q16 = enc.encode(qtexts, sim="dot", out_f32=q32, overflow=overflow)
        overflow.check()
    finally:
        enc.close()
    assert shard.dtype == torch.float16 and q16.dtype == torch.float16
    Db, Qb = index_ref.pack(d32.cpu().numpy(), "fp16"), index_ref.pack(q32.cpu().numpy(), "fp16")
    assert np.array_equal(_bits(shard), Db) and np.array_equal(_bits(q16), Qb)
    assert torch.all(shard.double().norm(dim=1) <= nb.double())
    cids, qids = [f"p{j}" for j in range(len(texts))], [f"q{i}" for i in range(len(qtexts))]
    retriever = Retriever(cids, shard, norm_bounds=nb)
    assert retriever.index.dtype == torch.float16
    prof = retriever.ranking_profile(qids, q16, keep=50)
    ref_i, ref_s = index_ref.canonical_search(Qb, Db, "fp16", 50)
    ids = np.array([[int(p[1:]) for p in prof[q]] for q in qids], np.int64)
    sc = np.array([list(prof[q].values()) for q in qids], np.float32)
    assert np.array_equal(ids, ref_i) and np.array_equal(sc.view(np.uint32), ref_s.view(np.uint32))


def test_assign_topk_on_factors_packed_to_fp16():
    from ccrec_amd import ops
    from ccrec_amd.bbpr_transform import LowRankScore, score_op
    from ccrec_amd.rime_util import _assign_topk
    rs = np.random.RandomState(9)
    U_, V_ = rs.randn(9, 40).astype(np.float32), rs.randn(500, 40).astype(np.float32)
    S = LowRankScore(ops.pack_half(torch.from_numpy(U_).cuda(), torch.float16), ops.pack_half(torch.from_numpy(V_).cuda(), torch.float16))
    k = 7
    got = _assign_topk(S, k)
    Ub, Vb = index_ref.pack(U_, "fp16"), index_ref.pack(V_, "fp16")
    ref_i, _ = index_ref.canonical_search(Ub, Vb, "fp16", k)
    assert got.shape == (9, 500) and got.nnz == 9 * k
    for r in range(9):
        assert sorted(got[r].indices.tolist()) == sorted(ref_i[r].tolist())
    sc, ids = S.topk(k)
    assert np.array_equal(ids.cpu().numpy(), ref_i)
    full = index_ref.canonical_scores(Ub, Vb, "fp16")
    assert np.array_equal(S.as_tensor().cpu().numpy().view(np.uint32), full.view(np.uint32))
    assert score_op(S, "max") == float(full.max()) and score_op(S, "min") == float(full.min())
    want_sum = float(index_ref.unpack(Ub, "fp16").astype(np.float64).sum(0) @ index_ref.unpack(Vb, "fp16").astype(np.float64).sum(0))
    assert abs(score_op(S, "sum") - want_sum) <= 1e-9 * max(1.0, abs(want_sum))
    with pytest.raises(AssertionError):
        LowRankScore(S.user, ops.pack_bf16(torch.from_numpy(V_).cuda()))
