"""The row kernels -- LayerNorm and GELU of csrc/ccr_encoder.hip, the pack and mean-pool kernels of csrc/ccr_pack.hip, the small
per-row reductions beside them -- at every width class, launch shape and edge the dispatch code distinguishes.

Each kernel is held to a plain restatement of the same operation: fp64 LayerNorm on the operands the kernel sees, the oracle's
bit-exact pooling and pack, one IEEE division for the pooling backward, torch's own GELU on all 65 536 inputs of each 16-bit type.
Tolerances that are not zero are derived where they are used; two of them are measured on torch's fp32 kernels (never on the kernel
under test) and the figures are written beside them."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HALVES = [torch.bfloat16, torch.float16]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _name(dtype):
    return str(dtype).split(".")[-1]


# ----------------------------------------------------------------------------------------- LayerNorm
# Tolerance of |kernel - fp64 LayerNorm|, both taken on the same fp32 rows v: max(2e-5 + 2e-5 |ref|, 2 E), E = the largest error of
# torch.nn.functional.layer_norm in fp32 on the same rows against the same fp64 reference.  Both are fp32 two-pass reductions that
# differ in summation order only, so the kernel may be as far from the truth as torch is, times two; the floor is the tolerance the
# older tests hold the kernel to against torch.  Measured on an MI355X, worst over every C, row count and 16-bit type below
# (add + LayerNorm / embedding + LayerNorm):
#   rows "randn"              torch E = 7.8e-7 / 8.1e-7, kernel 8.3e-7 / 7.5e-7: the floor decides
#   rows "offset"             torch E = 1.9e-5 / 1.4e-5, kernel 4.7e-6 / 3.9e-6 (1.6e-5 / 1.3e-5 before the kernels corrected their mean)
#   rows "const", eps 1e-5    torch E = 9.0e-4 / 4.5e-4, kernel 0 (4.5e-4 / 2.3e-4 before)
#   rows "const", eps 1e-12   torch E = 2.9 / 1.4, kernel 0 (1.0 / 0.65 before: an ulp of the mean times 1e6; at C = 5 and 8 torch's own
#                             mean happened to be exact, and the bound taken from it, 0, caught the kernels' 0.18 and 0.35)
LN_KINDS = ["randn", "offset", "const"]


def _ln_fp64(v32, gamma, beta, eps):
    v = v32.double()
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def _check_layernorm(tag, got, v32, gamma, beta, eps, kind):
    """got: the kernel's fp32 rows; v32: the fp32 rows it normalised."""
    dim = v32.shape[-1]
    assert torch.isfinite(got).all()
    ref = _ln_fp64(v32, gamma, beta, eps)
    tch, tch_mean, _ = torch.native_layer_norm(v32, (dim,), gamma, beta, eps)
    e_torch = float((tch.double() - ref).abs().max())
    e_kernel = float((got.double() - ref).abs().max())
    if kind == "const" and eps < 1e-8:
        # zero variance under a vanishing eps: 1 / sqrt(var + eps) reaches 1e6 and amplifies whatever an fp32 mean leaves of v - mean.
        # That amplification belongs to the definition, not to a kernel: only finiteness and the reference's own bound are asserted.
        bound = gamma.abs().double() * (v32.double() - tch_mean.double()).abs() * 1e6
        worst = float(((got.double() - beta.double()).abs() - bound).max())
        assert worst <= 0.0, f"{tag}: |y - beta| exceeds |gamma| |v - mean|_fp32 1e6 by {worst:.3e}"
        return
    allowed = torch.maximum(2e-5 + 2e-5 * ref.abs(), torch.full_like(ref, 2 * e_torch))
    excess = float(((got.double() - ref).abs() - allowed).max())
    assert excess <= 0.0, f"{tag} {kind}: kernel error {e_kernel:.3e}, torch fp32 error {e_torch:.3e}, over the tolerance by {excess:.3e}"


def _affine(dim, g):
    return (torch.rand(dim, generator=g) + 0.5).cuda(), torch.randn(dim, generator=g).cuda()


@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("C", range(1, 9))
@pytest.mark.parametrize("half", HALVES, ids=_name)
def test_add_layernorm_every_width(half, C, kind):
    """dim = 256 C for every instantiated C; rows 1, 5, 6: a last block of 1, 1 and 2 live waves; with and without the residual, with
    and without the fp32 output."""
    from ccrec_amd import ops
    dim = 256 * C
    g = torch.Generator().manual_seed(1000 * C + len(kind))
    gamma, beta = _affine(dim, g)
    for rows in (1, 5, 6):
        if kind == "const":      # every element of a row's sum equal: zero variance
            x = (torch.randn(rows, 1, generator=g) * 2).to(half).expand(rows, dim).contiguous().cuda()
            res = (torch.randn(rows, 1, generator=g) * 3 + 0.5).expand(rows, dim).contiguous().cuda()
        else:
            x = torch.randn(rows, dim, generator=g).to(half).cuda()
            res = (torch.randn(rows, dim, generator=g) + 100.0 if kind == "offset" else torch.randn(rows, dim, generator=g) * 3 + 0.5).cuda()
        for eps in ((1e-12, 1e-5) if kind == "const" else (1e-12,)):
            for residual in (res, None):
                v32 = x.float() + residual if residual is not None else x.float()
                tag = f"add {_name(half)} C={C} rows={rows} res={residual is not None}"
                f32, b16 = ops.add_layernorm(x, residual, gamma, beta, eps)
                _check_layernorm(tag, f32, v32, gamma, beta, eps, kind)
                assert b16.dtype == half and torch.equal(b16, f32.to(half))          # the 16-bit copy is the rounded fp32 row
                none, only = ops.add_layernorm(x, residual, gamma, beta, eps, want_f32=False)
                assert none is None and torch.equal(only, b16)


@pytest.mark.parametrize("kind", LN_KINDS)
@pytest.mark.parametrize("C", range(1, 9))
@pytest.mark.parametrize("half", HALVES, ids=_name)
def test_embed_layernorm_every_width(half, C, kind):
    """Small fp32 tables made here (vocab 50, 40 positions, 2 types), 9 tokens (a last block of one live wave), with and without token
    types.  The reference is the plain fp32 sum (word[id] + type[t]) + position[p] -- the kernel's order, so the same bits -- then
    LayerNorm in fp64."""
    from ccrec_amd import ops
    dim, T = 256 * C, 9
    g = torch.Generator().manual_seed(2000 * C + len(kind))
    gamma, beta = _affine(dim, g)

    def table(n, offset=0.0):
        if kind == "const":
            return (torch.randn(n, 1, generator=g) * 2 + offset).expand(n, dim).contiguous().cuda()
        return (torch.randn(n, dim, generator=g) + offset).cuda()

    word, pos_tab, type_tab = table(50), table(40, 100.0 if kind == "offset" else 0.0), table(2)
    ids = torch.randint(0, 50, (T,), generator=g).cuda()
    pos = torch.randint(0, 40, (T,), generator=g).cuda()
    types = torch.randint(0, 2, (T,), generator=g).cuda()
    for eps in ((1e-12, 1e-5) if kind == "const" else (1e-12,)):
        for tt in (types, None):
            v32 = (word[ids] + type_tab[tt if tt is not None else torch.zeros_like(ids)]) + pos_tab[pos]
            f32, b16 = ops.embed_layernorm(word, pos_tab, type_tab, ids, pos, tt, gamma, beta, eps, dtype=half)
            _check_layernorm(f"embed {_name(half)} C={C} types={tt is not None}", f32, v32, gamma, beta, eps, kind)
            assert b16.dtype == half and torch.equal(b16, f32.to(half))


@pytest.mark.parametrize("dim", [128, 2304, 300])
def test_layernorm_refuses_other_widths(dim):
    from ccrec_amd import ops, _lib
    gamma, beta = torch.ones(dim, device="cuda"), torch.zeros(dim, device="cuda")
    for half in HALVES:
        with pytest.raises(_lib.CcrError):
            ops.add_layernorm(torch.zeros(2, dim, dtype=half, device="cuda"), None, gamma, beta, 1e-5)
        tab = torch.zeros(4, dim, device="cuda")
        idx = torch.zeros(2, dtype=torch.int64, device="cuda")
        with pytest.raises(_lib.CcrError):
            ops.embed_layernorm(tab, tab, tab, idx, idx, None, gamma, beta, 1e-5, dtype=half)


# ----------------------------------------------------------------------------------------- mean pooling, forward
POOL_DIMS = [4, 8, 252, 260, 1024, 1028, 2052, 3076, 4096]     # 1 .. 4 chunks per thread, partly idle last waves, 64-thread blocks
POOL_B = 5


def _pool_masks(L, g):
    """Prefixes of every length 1 .. L; (L >= 2) a mask with holes whose FIRST token is masked; one live token at the last position."""
    rows = [(torch.arange(L) < n).long() for n in range(1, L + 1)]
    if L >= 2:
        holes = (torch.rand(L, generator=g) < 0.6).long()
        holes[0] = 0
        holes[1 + int(torch.randint(0, L - 1, (1,), generator=g))] = 1
        rows.append(holes)
    last = torch.zeros(L, dtype=torch.int64)
    last[L - 1] = 1
    rows.append(last)
    return torch.stack(rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("L", [1, 7, 8, 9, 37])                 # the token loop is unrolled by 8 with a clamped tail
@pytest.mark.parametrize("dim", POOL_DIMS)
def test_meanpool_pack_equals_the_oracle(dim, L, dtype):
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(dim * 100 + L)
    hidden = torch.randn(POOL_B, L, dim, generator=g).to(dtype)
    masks = _pool_masks(L, g)
    hidden_d, hidden_np = hidden.cuda(), hidden.float().numpy()
    for lo in range(0, masks.shape[0], POOL_B):
        mask = masks[[(lo + j) % masks.shape[0] for j in range(POOL_B)]]          # batches of B = 5, the last one wrapping round
        f32, b16 = ops.meanpool_pack(hidden_d, mask.cuda())
        ref = orc.meanpool(hidden_np, mask.numpy())
        assert np.array_equal(f32.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(_bits(b16), orc.pack_bf16(ref))
        _, b16n = ops.meanpool_pack(hidden_d, mask.cuda(), normalize=True, want_f32=False)
        refn = ref / np.maximum(np.linalg.norm(ref.astype(np.float64), axis=1, keepdims=True), 1e-12)
        np.testing.assert_allclose(b16n.float().cpu().numpy(), refn, atol=4e-3, rtol=8e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_name)
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dim", [1028, 4096])
def test_packed_pooling_gives_the_padded_pooling_bits_when_threads_own_several_chunks(dim, normalize, dtype):
    """ccr_meanpool_pack_bf16_packed == the padded form, bit for bit (fp32 rows, bf16 rows, norm bounds), at widths where a thread owns
    two and four chunks, with the destination rows a permutation."""
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(dim)
    lens = [5, 1, 9, 8, 7]
    B, L = len(lens), 9
    padded = torch.zeros(B, L, dim, dtype=dtype)
    mask = torch.zeros(B, L, dtype=torch.int64)
    pieces = []
    for b, n in enumerate(lens):
        x = (torch.randn(n, dim, generator=g) * 0.4).to(dtype)
        padded[b, :n] = x
        mask[b, :n] = 1
        pieces.append(x)
    packed = torch.cat(pieces).contiguous().cuda()
    seq_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    seq_start = (torch.cumsum(seq_len, 0, dtype=torch.int32) - seq_len).contiguous()
    rows = torch.tensor([3, 0, 4, 1, 2], device="cuda")
    outs = []
    for form in ("padded", "packed"):
        b16 = torch.zeros(B, dim, dtype=torch.bfloat16, device="cuda")
        f32 = torch.zeros(B, dim, dtype=torch.float32, device="cuda")
        nb = torch.zeros(B, dtype=torch.float32, device="cuda")
        if form == "padded":
            ops.meanpool_pack(padded.cuda(), mask.cuda(), normalize=normalize, out_bf16=b16, out_f32=f32, dst_rows=rows, norm_bounds=nb)
        else:
            ops.meanpool_pack_packed(packed, seq_start, seq_len, normalize=normalize, out_bf16=b16, out_f32=f32, dst_rows=rows, norm_bounds=nb)
        outs.append((b16, f32, nb))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    ref = orc.meanpool(padded.float().numpy(), mask.numpy())
    assert np.array_equal(outs[1][1].cpu().numpy()[rows.cpu().numpy()], ref)         # and both are the oracle's rows, scattered


@pytest.mark.parametrize("dim", [4100, 6])
def test_meanpool_pack_refuses_other_widths(dim):
    from ccrec_amd import ops, _lib
    hidden = torch.zeros(2, 3, dim, device="cuda")
    mask = torch.ones(2, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.CcrError):
        ops.meanpool_pack(hidden, mask)
    lens = torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.CcrError):
        ops.meanpool_pack_packed(hidden.view(6, dim), torch.tensor([0, 3], dtype=torch.int32, device="cuda"), lens)


# ----------------------------------------------------------------------------------------- mean pooling, backward
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("L", [1, 9, 37, 300])                  # 300: more tokens than the block has threads, in the count loop
@pytest.mark.parametrize("dim", POOL_DIMS + [96])
def test_meanpool_backward_is_one_division_and_one_rounding(dim, L, dtype):
    """d hidden[b][l] = mask[b][l] ? grad[b] / count_b : 0 -- exactly one IEEE fp32 division and one conversion to the hidden states'
    type, which the CPU does bit for bit alike."""
    from ccrec_amd import ops
    B = 3
    g = torch.Generator().manual_seed(dim * 1000 + L)
    mask = (torch.rand(B, L, generator=g) < 0.6).long()                       # holes anywhere, the first token included
    mask[torch.arange(B), torch.randint(0, L, (B,), generator=g)] = 1         # at least one live token per row
    h = torch.randn(B, L, dim, generator=g).to(dtype).cuda().requires_grad_(True)
    grad = torch.randn(B, dim, generator=g) * torch.tensor([1e-3, 1.0, 1e3])[:, None]
    out = ops.meanpool(h, mask.cuda())
    out.backward(grad.cuda())
    count = mask.sum(1)
    ref = torch.where(mask[..., None].bool(), (grad / count.float()[:, None])[:, None, :], torch.zeros(())).to(dtype)
    got = h.grad.cpu()
    assert got.dtype == dtype and got.shape == ref.shape
    int_view = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(int_view), ref.view(int_view)), int((got.view(int_view) != ref.view(int_view)).sum())


# ----------------------------------------------------------------------------------------- pack kernels: grid wrap
def _wrap_windows(rows, cap_blocks):
    """The first 64 rows, the last 64 and 64 around the row at which a grid capped at cap_blocks blocks of four waves wraps."""
    wrap = 4 * cap_blocks
    assert rows > wrap
    return np.r_[0:64, wrap - 32:min(rows, wrap + 32), rows - 64:rows]


def _n64(bits):
    return np.sqrt((orc.unpack_bf16(bits).astype(np.float64) ** 2).sum(1))


@pytest.mark.parametrize("dim", [8, 5])                          # pack_rows_kernel / pack_rows_padded_kernel, 65 536 blocks each
def test_normalising_pack_wraps_its_grid(dim):
    from ccrec_amd import ops
    rows = 262_149                                               # 4 x 65 536 + 5
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(rows, dim, generator=g) * (torch.rand(rows, 1, generator=g) * 5 + 0.01)
    xd = x.cuda()
    nb = torch.empty(rows, device="cuda")
    out, norms = ops.pack_bf16(xd, normalize=True, return_norms=True, norm_bounds=nb)
    plain = ops.pack_bf16(xd)
    w = _wrap_windows(rows, 65_536)
    xs = x.numpy()[w]
    assert np.array_equal(_bits(out)[w][:, :dim], orc.normalize_pack_bf16(xs)) and not _bits(out)[:, dim:].any()
    assert np.array_equal(norms.cpu().numpy()[w], orc.row_norms(xs))
    assert np.array_equal(_bits(plain)[w][:, :dim], orc.pack_bf16(xs))
    # every row, on the device: the plain pack is torch's conversion; the normalised rows are F.normalize up to bf16 rounding, the norms
    # torch's up to fp32 rounding, the bounds 1.004 (no row here is zero)
    assert torch.equal(plain[:, :dim].view(torch.int16), xd.to(torch.bfloat16).view(torch.int16))
    torch.testing.assert_close(out[:, :dim].float(), torch.nn.functional.normalize(xd, p=2, dim=1), atol=4e-3, rtol=8e-3)
    torch.testing.assert_close(norms, xd.double().norm(dim=1).float(), atol=0, rtol=1e-6)
    assert torch.equal(nb, torch.full_like(nb, 1.004))


def test_bounded_pack_wraps_its_grid():
    """pack_rows_bound_kernel: 131 072 blocks of four waves, then r += nwaves."""
    from ccrec_amd import ops
    rows, dim = 524_291, 8                                       # 4 x 131 072 + 3
    g = torch.Generator().manual_seed(3)
    xd = (torch.randn(rows, dim, generator=g) * (torch.rand(rows, 1, generator=g) * 5 + 0.01)).cuda()
    nb = torch.full((rows,), float("nan"), device="cuda")
    out = ops.pack_bf16(xd, norm_bounds=nb)
    assert torch.equal(out.view(torch.int16), xd.to(torch.bfloat16).view(torch.int16))
    w = _wrap_windows(rows, 131_072)
    assert np.array_equal(_bits(out)[w], orc.pack_bf16(xd.cpu().numpy()[w]))
    n64 = out.double().norm(dim=1)                               # every row
    assert bool((n64 <= nb.double()).all()) and bool((nb.double() <= 1.01 * n64).all())
    true = orc.row_norms_bf16(_bits(out)[w]).astype(np.float64)
    got = nb.cpu().numpy().astype(np.float64)[w]
    assert np.all(true <= got) and np.all(got <= 1.01 * true)


# ----------------------------------------------------------------------------------------- the norm bounds
# bounds[r] >= ||packed row r|| is what the fused filter's margins rest on (the lower side); the cap follows from the code: the
# loosest kernel writes 1.004 x the fp32 row's norm, bf16 rounding moves a norm by at most 2^-9 relative either way, and
# 1.004 (1 + 2^-9) / (1 - 2^-9) < 1.008.  Magnitudes stay in bf16's normal range (or exactly 0): the 2^-9 argument needs it.
def _scaled_rows(rows, dim, g):
    x = torch.randn(rows, dim, generator=g) * torch.logspace(-6, 6, rows)[:, None]
    x[rows // 2] = 0
    tiny = (x != 0) & (x.abs() < 1e-30)
    assert not tiny.any()
    return x


def _assert_bounds(bounds, packed_bits, zero_row):
    got = bounds.cpu().numpy().astype(np.float64)
    for n64 in (_n64(packed_bits), orc.row_norms_bf16(packed_bits).astype(np.float64)):
        assert np.all(n64 <= got), f"bound below the norm at rows {np.nonzero(n64 > got)[0][:5]}"
        assert np.all(got <= 1.01 * n64), f"bound above 1.01 x the norm at rows {np.nonzero(got > 1.01 * n64)[0][:5]}"
    assert got[zero_row] == 0.0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dim", [8, 64, 2048, 4096, 5, 301, 772])     # multiples of 8: pack_rows_bound / pack_rows; the rest: padded
def test_pack_norm_bounds_hold_at_every_scale(dim, normalize):
    from ccrec_amd import ops
    rows = 25
    x = _scaled_rows(rows, dim, torch.Generator().manual_seed(dim))
    nb = torch.full((rows,), float("nan"), device="cuda")
    out = ops.pack_bf16(x.cuda(), normalize=normalize, norm_bounds=nb)
    assert np.array_equal(_bits(out)[:, :dim], orc.normalize_pack_bf16(x.numpy()) if normalize else orc.pack_bf16(x.numpy()))
    _assert_bounds(nb, _bits(out), rows // 2)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dim", [8, 64, 772, 2048, 4096])
def test_meanpool_norm_bounds_hold_at_every_scale(dim, normalize):
    from ccrec_amd import ops
    rows, L = 25, 9
    g = torch.Generator().manual_seed(dim + 1)
    hidden = torch.randn(rows, L, dim, generator=g) * torch.logspace(-6, 6, rows)[:, None, None]
    hidden[rows // 2] = 0
    mask = (torch.arange(L)[None, :] < torch.randint(1, L + 1, (rows, 1), generator=g)).long()
    nb = torch.full((rows,), float("nan"), device="cuda")
    f32, b16 = ops.meanpool_pack(hidden.cuda(), mask.cuda(), normalize=normalize, norm_bounds=nb)
    assert np.array_equal(f32.cpu().numpy(), orc.meanpool(hidden.numpy(), mask.numpy()))
    _assert_bounds(nb, _bits(b16), rows // 2)


# ----------------------------------------------------------------------------------------- GELU, the whole domain
# |kernel - round16(fp64 GELU)| <= ulp16(ref) + GELU_FACTOR 2^-24 |x|: one unit of the 16-bit type for the final rounding (the fp64
# value is rounded through fp32), and the fp32 error of 1 + erf(x / sqrt 2) -- its rounding plus erff's own few ulps -- times |x| / 2,
# which decides in the negative tail where the formula cancels.  The factor is calibrated on torch's GPU GELU over all 65 536 inputs of
# each type, not on the kernel: torch needs a factor of 0.232 (bf16) and 0.210 (fp16) on an MI355X, so 4 is not widened.
GELU_FACTOR = 4.0
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}    # mantissa bits, smallest normal exponent


def _all_patterns(half):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(half)


_TORCH_GELU = {}


def _torch_gelu_table(half):
    """torch's GPU GELU of all 65 536 inputs of the type, entry 32768 + (the input's bits as int16), computed once."""
    if half not in _TORCH_GELU:
        _TORCH_GELU[half] = torch.nn.functional.gelu(_all_patterns(half).cuda())
    return _TORCH_GELU[half]


def _ulp16(ref, half):
    mant, emin = _FMT[half]
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(ref), e - mant)


def _gelu_factor_needed(y, x, half):
    """The factor f at which |y - ref| <= ulp16(ref) + f 2^-24 |x| just holds over the finite part of the domain."""
    xd = x.double()
    ref = (0.5 * xd * (1.0 + torch.special.erf(xd / math.sqrt(2.0)))).to(half).double()
    finite = torch.isfinite(ref) & torch.isfinite(xd)
    nan, inf = torch.isnan(ref), torch.isinf(ref)                 # x = NaN and -inf (0 x inf) give NaN, x = +inf gives +inf
    assert torch.equal(torch.isnan(y), nan) and torch.equal(y.double()[inf], ref[inf])
    over = ((y.double() - ref).abs() - _ulp16(ref, half))[finite] / (2.0 ** -24 * xd.abs()[finite]).clamp_min(1e-300)
    return float(over.clamp_min(0).max())


@pytest.mark.parametrize("half", HALVES, ids=_name)
def test_gelu_on_every_input_of_the_type(half):
    from ccrec_amd import ops
    x = _all_patterns(half).cuda()
    ref = _torch_gelu_table(half)
    got = ops.gelu_(x.clone())
    same = (got.view(torch.int16) == ref.view(torch.int16)) | (torch.isnan(got) & torch.isnan(ref))
    assert same.all(), f"{int((~same).sum())} inputs differ from torch, first {x[~same][:5].tolist()}"
    f_torch, f_kernel = _gelu_factor_needed(ref.cpu(), x.cpu(), half), _gelu_factor_needed(got.cpu(), x.cpu(), half)
    assert f_kernel <= max(GELU_FACTOR, 1.5 * f_torch)


@pytest.mark.parametrize("n", [8, 2040, 2056])                   # one vector; just below and just above one block of 256 vectors
@pytest.mark.parametrize("half", HALVES, ids=_name)
def test_gelu_tails(half, n):
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(n)
    buf = torch.full((n + 16,), 7.0, dtype=half, device="cuda")
    x = (torch.randn(n, generator=g) * 3).to(half).cuda()
    buf[8:8 + n] = x
    ops.gelu_(buf[8:8 + n])
    # torch's GELU of the same values, read from its run over the whole domain: on a short array torch's own result is not always
    # that one (measured on an MI355X: at n = 2040 in fp16 torch's direct result differed from its whole-domain one at 62 values, at the
    # other five (type, n) pairs at none), and the kernel computes one value per input whatever the length
    ref = _torch_gelu_table(half)[x.view(torch.int16).long() + 32768]
    assert torch.equal(buf[8:8 + n].view(torch.int16), ref.view(torch.int16))
    assert bool((buf[:8] == 7).all()) and bool((buf[8 + n:] == 7).all())      # nothing written beside the array


def test_gelu_refuses_a_length_that_is_no_multiple_of_8():
    from ccrec_amd import ops, _lib
    lib = ops.require_gpu()
    x = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.CcrError):
        _lib.check(lib.ccr_gelu_half(ops._ptr(x), ops._ptr(x), 12, _lib.DTYPE_BF16, ops._stream(x)), "ccr_gelu_half")
    with pytest.raises(AssertionError):
        ops.gelu_(x[:12])


# ----------------------------------------------------------------------------------------- rank metrics, column sums
def test_rank_metrics_over_several_blocks():
    """One thread per query: 1 000 queries are four blocks.  k = 50 with a cut-off above it (100); queries without qrels; queries with
    several relevant ids in the list (hits above 1)."""
    from ccrec_amd.evaluation import rank_metrics
    rs = np.random.RandomState(11)
    nq, k, n = 1000, 50, 3000
    ids = np.stack([rs.permutation(n)[:k] for _ in range(nq)]).astype(np.int64)
    qrels = []
    for q in range(nq):
        rel = set(rs.randint(0, n, size=rs.randint(0, 4)).tolist())
        if q % 4 == 1:
            rel |= set(ids[q, rs.choice(k, 3, replace=False)].tolist())      # several hits
        elif q % 4 == 2:
            rel = set()                                                      # no qrels at all
        qrels.append(rel)
    k_values = (1, 10, 50, 100)
    got = rank_metrics(torch.from_numpy(ids).cuda(), qrels, k_values)
    assert max(len(set(ids[q].tolist()) & qrels[q]) for q in range(nq)) >= 3 and any(not r for r in qrels)
    for kk in k_values:
        assert got[f"MRR@{kk}"] == orc.mrr(ids, qrels, kk)
        rec = [len(set(ids[q, :kk].tolist()) & qrels[q]) / len(qrels[q]) for q in range(nq) if qrels[q]]
        assert abs(got[f"Recall@{kk}"] - round(float(np.mean(rec)), 5)) < 2e-5
    assert got["MRR@100"] == got["MRR@50"] and got["Recall@100"] == got["Recall@50"]


@pytest.mark.parametrize("rows,dim", [(1, 8), (31, 8), (33, 72), (5003, 4096)])
def test_colsum_bf16_shapes(rows, dim):
    """One row, one short of and one more than the 32 row lanes, a second block of columns that is partly idle, and a wide matrix."""
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(rows + dim)
    bits = orc.pack_bf16(torch.randn(rows, dim, generator=g).numpy())
    got = ops.colsum_bf16(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()).cpu().numpy()
    ref = orc.unpack_bf16(bits).astype(np.float64).sum(0)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-9)
