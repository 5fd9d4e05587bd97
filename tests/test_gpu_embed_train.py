"""The fine-tune step in one packed pass (library version 108) on the GPU: the embedding block with a backward
(ops.embed_layernorm_train over ccr_embed_layernorm_train_half / ccr_embed_layernorm_bwd_half / ccr_embedding_grad), mean pooling of a
packed token array with a backward (ops.meanpool_packed), and the whole stack under CCREC_FUSED_ENCODER_TRAIN_PACKED=1 with
MultipleNrlStep(one_pass=True).

Bars.  Forward, table gradient and pooling are compared bit for bit with what they restate (ops.embed_layernorm + ops.dropout_apply,
embed_grad_ref, ops.meanpool on the zero-padded form).  The LayerNorm backward carries test_gpu_encoder_train.py's LayerNorm bar (no
further from fp64 than 2 x torch's fp32 path, floor 1e-6 max |ref|); the whole stack carries that file's fine-tune bars, measured against
the fp32 module.  Measured ratios are printed (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, PKG  # noqa: F401
from helpers import DTYPES, LN_EPS, spacing as _spacing
from test_cpu_embed_grad import order_case
from test_gpu_encoder_train import _KEY_BIAS, _stack_batch, _tiny_model

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ the embedding block
_BLOCKS = {}


def _block(rows, dim, seed=0, no_types=False):
    """Tables, index vectors (a few ids outside their table: the kernels clamp), gamma, beta, keep bits (p = 0.25) and d_y of one case,
    built once and shared (never modified)."""
    key = (rows, dim, seed, no_types)
    if key not in _BLOCKS:
        from ccrec_amd import dropout_ref, ops
        g = torch.Generator().manual_seed(1000 * seed + rows + dim)
        vocab, n_pos, n_types = 50, 40, 1 if no_types else 2
        c = {"word": torch.randn(vocab, dim, generator=g).cuda(), "pos": 0.5 * torch.randn(n_pos, dim, generator=g).cuda(),
             "types": torch.zeros(1, dim).cuda() if no_types else 0.5 * torch.randn(n_types, dim, generator=g).cuda(),
             "ids": torch.randint(0, vocab, (rows,), generator=g).cuda(), "positions": torch.randint(0, n_pos, (rows,), generator=g).cuda(),
             "tt": None if no_types else torch.randint(0, n_types, (rows,), generator=g).cuda(),
             "gamma": (0.6 + 0.8 * torch.rand(dim, generator=g)).cuda(), "beta": 0.1 * torch.randn(dim, generator=g).cuda(),
             "d_y": torch.randn(rows, dim, generator=g).cuda(), "sizes": (vocab, n_pos, n_types)}
        if rows >= 3:
            c["ids"][0], c["ids"][2], c["positions"][1] = vocab + 9, -4, n_pos
        c["bits"] = ops.dropout_bits_rows(rows, dim, 77 + seed, 5, 0.25)
        c["inv_keep"] = dropout_ref.inv_keep(0.25)
        _BLOCKS[key] = c
    return _BLOCKS[key]


def _fwd_args(c):
    return c["word"], c["pos"], c["types"], c["ids"], c["positions"], c["tt"], c["gamma"], c["beta"], LN_EPS


def _keep_mask(bits, dim):
    """bits int32 [rows, dim / 32] -> bool [rows, dim] (bit i of word w <-> column 32 w + i)."""
    shifts = torch.arange(32, device=bits.device, dtype=torch.int64)
    return ((bits.long()[:, :, None] >> shifts) & 1).bool().reshape(bits.shape[0], dim)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", range(1, 9))
def test_forward_has_the_bits_of_embed_layernorm_then_dropout_apply(C, dtype):
    """Every width 256 .. 2048: without bits, and with all-ones bits and inv_keep = 1, both outputs are ops.embed_layernorm's; with random
    bits they are ops.dropout_apply(ops.embed_layernorm(...))'s.  And through the autograd op."""
    from ccrec_amd import ops
    c = _block(11, 256 * C)
    f32, b16 = ops.embed_layernorm(*_fwd_args(c), dtype=dtype)
    ones = torch.full((11, 8 * C), -1, dtype=torch.int32, device="cuda")
    for got in (ops.embed_layernorm(*_fwd_args(c), dtype=dtype), ops.embed_layernorm(*_fwd_args(c), keep_bits=ones, inv_keep=1.0, dtype=dtype)):
        assert _same(got[0], f32) and _same(got[1], b16)
    want = ops.dropout_apply(f32, c["bits"], c["inv_keep"], dtype)
    got = ops.embed_layernorm(*_fwd_args(c), keep_bits=c["bits"], inv_keep=c["inv_keep"], dtype=dtype)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert (got[0] == 0).any() and (got[0] != 0).any()
    got = ops.embed_layernorm_train(*_fwd_args(c), keep_bits=c["bits"], inv_keep=c["inv_keep"], dtype=dtype)
    assert _same(got[0], want[0]) and _same(got[1], want[1])


def test_forward_of_the_no_type_form():
    """DistilBERT's embeddings: a one-row all-zero type table and no token types."""
    from ccrec_amd import ops
    c = _block(9, 768, no_types=True)
    f32, b16 = ops.embed_layernorm(*_fwd_args(c))
    want = ops.dropout_apply(f32, c["bits"], c["inv_keep"])
    got = ops.embed_layernorm_train(*_fwd_args(c), keep_bits=c["bits"], inv_keep=c["inv_keep"])
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    plain = ops.embed_layernorm_train(*_fwd_args(c))
    assert _same(plain[0], f32) and _same(plain[1], b16)


def _clamped(c):
    vocab, n_pos, n_types = c["sizes"]
    tt = torch.zeros_like(c["ids"]) if c["tt"] is None else c["tt"].clamp(0, n_types - 1)
    return c["ids"].clamp(0, vocab - 1), c["positions"].clamp(0, n_pos - 1), tt


def _autograd(c, dt, drop):
    """Gradients of sum(d_y * dropout(LayerNorm((word[i] + type[t]) + pos[p]))) in precision dt by torch autograd ->
    {v (the gathered sum), word, pos, types, gamma, beta}."""
    ids, positions, tt = _clamped(c)
    leaves = {n: c[n].to(dt).detach().requires_grad_(True) for n in ("word", "pos", "types", "gamma", "beta")}
    v = (leaves["word"][ids] + leaves["types"][tt]) + leaves["pos"][positions]
    v.retain_grad()
    y = F.layer_norm(v, (v.shape[1],), leaves["gamma"], leaves["beta"], LN_EPS)
    if drop:
        y = y * (_keep_mask(c["bits"], v.shape[1]).to(dt) * torch.tensor(c["inv_keep"], dtype=torch.float32).to(dt).item())
    (y * c["d_y"].to(dt)).sum().backward()
    out = {n: t.grad for n, t in leaves.items()}
    out["v"] = v.grad
    return out


BWD_SHAPES = [(rows, 256) for rows in (1, 3, 4, 5, 2047, 2049)] + [(7, 256 * C) for C in range(1, 9)]


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("rows,dim", sorted(set(BWD_SHAPES)))
def test_backward_against_fp64_autograd(rows, dim, drop):
    """d_x, d gamma, d beta of the kernel and the three table gradients of the autograd op vs fp64 autograd over dropout(LayerNorm(word[i]
    + type[t] + pos[p])): at most 2 x the error of torch's fp32 autograd (max and mean; floor 1e-6 max |ref|) -- the LayerNorm bar of
    test_gpu_encoder_train.py.  Rows 2047 / 2049: the 512-workgroup limit of the partial sums; 2049 rows over 2 types: runs that the
    long-run kernel of ccr_embedding_grad sums."""
    from ccrec_amd import ops
    c = _block(rows, dim, seed=1)
    ref, yard = _autograd(c, torch.float64, drop), _autograd(c, torch.float32, drop)
    bits, inv_keep = (c["bits"], c["inv_keep"]) if drop else (None, 1.0)
    d_x, d_gamma, d_beta = ops.embed_layernorm_bwd(c["word"], c["pos"], c["types"], c["ids"], c["positions"], c["tt"], c["gamma"], LN_EPS,
                                                   c["d_y"], bits, inv_keep)
    leaves = [c[n].clone().requires_grad_(True) for n in ("word", "pos", "types", "gamma", "beta")]
    f32, b16 = ops.embed_layernorm_train(leaves[0], leaves[1], leaves[2], c["ids"], c["positions"], c["tt"], leaves[3], leaves[4], LN_EPS,
                                         keep_bits=bits, inv_keep=inv_keep)
    (f32 * c["d_y"]).sum().backward()
    assert _same(leaves[3].grad, d_gamma) and _same(leaves[4].grad, d_beta)
    mine = {"v": d_x, "gamma": d_gamma, "beta": d_beta, "word": leaves[0].grad, "pos": leaves[1].grad, "types": leaves[2].grad}
    for label, got in mine.items():
        r, y = ref[label], yard[label]
        assert got.dtype == torch.float32 and got.shape == r.shape and torch.isfinite(got).all()
        e_k, e_y = (got.double() - r).abs(), (y.double() - r).abs()
        floor = 1e-6 * r.abs().max().item()
        print(f"embed_bwd {rows}x{dim} {'drop' if drop else 'plain'} {label}: max err kernel {e_k.max().item():.3e} torch {e_y.max().item():.3e}; "
              f"mean err kernel {e_k.mean().item():.3e} torch {e_y.mean().item():.3e}; max |ref| {r.abs().max().item():.3e}")
        assert e_k.max().item() <= 2 * e_y.max().item() + floor, (label, e_k.max().item(), e_y.max().item(), floor)
        assert e_k.mean().item() <= 2 * e_y.mean().item() + floor, (label, e_k.mean().item(), e_y.mean().item(), floor)
    # the table gradients are ccr_embedding_grad of the kernel's d_x: the restatement's bits
    from ccrec_amd import embed_grad_ref
    ids, positions, tt = _clamped(c)
    for got, idx in ((mine["word"], ids), (mine["pos"], positions), (mine["types"], tt)):
        want = embed_grad_ref.embedding_grad(idx.cpu().numpy(), d_x.cpu().numpy(), got.shape[0])
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_backward_honours_needs_input_grad_and_sums_both_outputs():
    from ccrec_amd import ops
    c = _block(37, 512, seed=2)
    g16 = torch.randn(37, 512, device="cuda").to(torch.bfloat16)
    word, gamma = c["word"].clone().requires_grad_(True), c["gamma"].clone().requires_grad_(True)
    calls = []
    real = ops.embedding_grad
    ops.embedding_grad = lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1]
    try:
        f32, b16 = ops.embed_layernorm_train(word, c["pos"], c["types"], c["ids"], c["positions"], c["tt"], gamma, c["beta"], LN_EPS,
                                             keep_bits=c["bits"], inv_keep=c["inv_keep"])
        ((f32 * c["d_y"]).sum() + (b16.float() * g16.float()).sum()).backward()
    finally:
        ops.embedding_grad = real
    assert calls == [50]                                    # only the word table asked for a gradient
    d_x, d_gamma, _ = ops.embed_layernorm_bwd(c["word"], c["pos"], c["types"], c["ids"], c["positions"], c["tt"], c["gamma"], LN_EPS,
                                              c["d_y"] + g16.float(), c["bits"], c["inv_keep"])
    assert _same(gamma.grad, d_gamma) and _same(word.grad, ops.embedding_grad(c["ids"], d_x, 50))


def test_d_beta_of_integer_gradients_is_the_exact_column_sum_and_the_workspace_is_exactly_sized():
    """d_y of small integers, inv_keep = 2: every partial sum of d beta is an integer below 2^24, exact in any order.  The workspace is
    min(ceil(rows / 4), 512) * 2 * dim * 4 bytes as the header says: the kernel runs with exactly that, a canary behind it survives."""
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    rows, dim = 2051, 256
    c = _block(rows, dim, seed=3)
    d_y = torch.randint(-8, 9, (rows, dim), generator=torch.Generator().manual_seed(4)).float().cuda()
    bits = ops.dropout_bits_rows(rows, dim, 5, 6, 0.5)
    _, _, d_beta = ops.embed_layernorm_bwd(c["word"], c["pos"], c["types"], c["ids"], c["positions"], c["tt"], c["gamma"], LN_EPS, d_y, bits, 2.0)
    want = (d_y.double() * _keep_mask(bits, dim) * 2).sum(0)
    assert torch.equal(d_beta.double(), want)
    need = 512 * 2 * dim * 4
    buf = torch.full((need // 4 + 64,), 7.0, device="cuda")
    d_x, d_gamma, d_beta2 = torch.empty(rows, dim, device="cuda"), torch.empty(dim, device="cuda"), torch.empty(dim, device="cuda")
    p = ops._ptr
    rc = lib.ccr_embed_layernorm_bwd_half(p(c["word"]), 50, p(c["pos"]), 40, p(c["types"]), 2, p(c["ids"]), p(c["positions"]), p(c["tt"]),
                                          p(c["gamma"]), LN_EPS, p(bits), 2.0, p(d_y), p(d_x), p(d_gamma), p(d_beta2), rows, dim, p(buf), need,
                                          ops._stream(buf))
    assert rc == _lib.CCR_OK
    assert _same(d_beta2, d_beta) and (buf[need // 4:] == 7).all()


# ------------------------------------------------------------------------------------------------------------------- the table gradient
def _runs(lengths, rng):
    """idx with one run of each length (ids 2, 4, 6, ..: odd ids and id 0 stay absent), rows shuffled."""
    idx = np.concatenate([np.full(n, 2 * (k + 1)) for k, n in enumerate(lengths)])
    return rng.permutation(idx), 2 * len(lengths) + 3


def _grad_cases():
    rng = np.random.default_rng(5)
    cases = {"run_edges": _runs([1, 63, 64, 65, 128, 129], rng),
             "kernel_threshold": _runs([255, 256, 257, 320, 513], rng),          # up to 256 entries: a wave; above: the long-run kernel
             "consecutive_long": (np.repeat([0, 1, 2, 3, 4, 5], [100, 257, 300, 5, 600, 256]), 6),    # owners at sorted positions 256, 512, 768
             "all_equal_4100": (np.full(4100, 1), 3),
             "all_distinct": (rng.permutation(300), 300),
             "first_and_last_id": (rng.permutation(np.repeat([0, 9], [70, 3])), 10),
             "out_of_range": (np.array([-7, 2, 15, 4, 10 ** 12, -1, 4]), 5),
             "one_row_table": (np.full(70, 0), 1),
             "empty": (np.zeros(0, dtype=np.int64), 4)}
    return cases


GRAD_CASES = _grad_cases()


@pytest.mark.parametrize("dim", [40, 260])
@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_embedding_grad_has_the_bits_of_the_restatement(name, dim):
    """dim 40: 2.5 column groups of the long-run kernel, a partly idle wave in the other; dim 260: 65 four-column pieces, the wave's second
    trip.  Every case: embed_grad_ref's bits, +0 on absent rows, a canary behind grad survives, a second run repeats the bits."""
    from ccrec_amd import embed_grad_ref, ops
    idx_np, n_rows = GRAD_CASES[name]
    idx_np = np.asarray(idx_np, dtype=np.int64)
    T = idx_np.size
    d_x_np = np.random.default_rng(T + dim).standard_normal((T, dim)).astype(np.float32)
    want = embed_grad_ref.embedding_grad(idx_np, d_x_np, n_rows)
    idx, d_x = torch.from_numpy(idx_np).cuda(), torch.from_numpy(d_x_np).cuda()
    buf = torch.full((n_rows * dim + 64,), 7.0, device="cuda")
    out = buf[:n_rows * dim].view(n_rows, dim)
    got = ops.embedding_grad(idx, d_x, n_rows, out=out)
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (buf[n_rows * dim:] == 7).all()
    absent = np.setdiff1d(np.arange(n_rows), np.clip(idx_np, 0, n_rows - 1))
    assert (got.cpu().numpy().view(np.uint32)[absent] == 0).all()                       # +0, not -0
    order = ops.embedding_order(idx, n_rows)
    assert np.array_equal(order.cpu().numpy(), embed_grad_ref.order(idx_np, n_rows))
    again = ops.embedding_grad(idx, d_x, n_rows, order=order)
    assert _same(again, got)


def test_embedding_grad_order_case_on_the_device():
    """The hand-worked run of tests/test_cpu_embed_grad.py (130 entries of 1e8, 1, -1e8 in four columns), alone and as a run of 130 + 256
    entries that the long-run kernel sums (the chunks after the case hold zeros)."""
    from ccrec_amd import ops
    x, want = order_case()
    got = ops.embedding_grad(torch.zeros(130, dtype=torch.int64, device="cuda"), torch.from_numpy(x).cuda(), 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32)[0], want.view(np.uint32)), (got, want)
    long = np.concatenate([x, np.zeros((256, 4), dtype=np.float32)])
    got = ops.embedding_grad(torch.zeros(386, dtype=torch.int64, device="cuda"), torch.from_numpy(long).cuda(), 1)
    assert np.array_equal(got.cpu().numpy().view(np.uint32)[0], want.view(np.uint32)), (got, want)


# ------------------------------------------------------------------------------------------------------------------------ packed pooling
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_meanpool_packed_has_the_bits_of_meanpool_on_the_padded_form(dtype):
    """Lengths 1, 7, 8, 9, 512 and an empty sequence in one launch, two unowned rows between the sequences: forward and d_hidden equal
    ops.meanpool's on the zero-padded [B, 512, dim] form of the same rows bit for bit; the gap rows keep a canary (kernel) / get no gradient
    (autograd op)."""
    from ccrec_amd import ops
    lens, dim, L = [1, 7, 8, 9, 512, 0], 264, 512
    g = torch.Generator().manual_seed(9)
    starts, at = [], 2
    for n in lens:
        starts.append(at)
        at += n + 2
    T = at
    hidden = torch.randn(T, dim, generator=g).to(dtype).cuda()
    seq_start, seq_len = torch.tensor(starts, dtype=torch.int32).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    padded = torch.zeros(len(lens), L, dim, dtype=dtype, device="cuda")
    mask = torch.zeros(len(lens), L, dtype=torch.int64, device="cuda")
    owned = torch.zeros(T, dtype=torch.bool, device="cuda")
    for b, (s, n) in enumerate(zip(starts, lens)):
        padded[b, :n], mask[b, :n], owned[s:s + n] = hidden[s:s + n], 1, True
    grad = torch.randn(len(lens), dim, generator=g).cuda()
    hp, hk = padded.clone().requires_grad_(True), hidden.clone().requires_grad_(True)
    want = ops.meanpool(hp, mask)
    got = ops.meanpool_packed(hk, seq_start, seq_len)
    assert _same(got.detach(), want.detach()) and torch.isfinite(got[:5]).all()
    want.backward(grad)
    got.backward(grad)
    assert hk.grad.dtype == dtype and (hk.grad[~owned] == 0).all()
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert _same(hk.grad[s:s + n], hp.grad[b, :n]), b
    canary = torch.full((T, dim), 7.0, dtype=dtype, device="cuda")
    ops.meanpool_bwd_packed(grad, seq_start, seq_len, canary)
    assert (canary[~owned] == 7).all() and _same(canary[owned], hk.grad[owned])


# --------------------------------------------------------------------------------------------------------------------- the whole stack
def _step(tower, ids, mask, autocast_dtype, one_pass):
    """One MultipleNrlStep over the nine texts of test_gpu_encoder_train.py's stack batch: loss.backward() -> (loss, gradients)."""
    import contextlib
    from ccrec_amd.bbpr_loss import MultipleNrlStep

    def forward(ptr):
        ptr = torch.as_tensor(ptr, device=ids.device)
        return tower(input_ids=ids[ptr], attention_mask=mask[ptr], input_step="inputs", output_step="mean_pooling")

    step = MultipleNrlStep(forward, torch.tensor([0, 1, 2]), torch.arange(9), {0: [6, 7], 1: [7, 8], 2: [8, 6]}, one_pass=one_pass)
    batch = torch.tensor([[0, 3, 1.0], [1, 4, 1.0], [2, 5, 1.0]])
    tower.zero_grad(set_to_none=True)
    with contextlib.nullcontext() if autocast_dtype is None else torch.autocast("cuda", dtype=autocast_dtype):
        loss = step(batch)
    loss.backward()
    return loss.item(), {n: p.grad.detach().clone() for n, p in tower.cls_model.named_parameters() if p.grad is not None}


def _count(monkeypatch, module, name):
    calls, real = [], getattr(module, name)
    monkeypatch.setattr(module, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _tower(kind, monkeypatch, dropout=0.0):
    from ccrec_amd.item_tower import NaiveItemTower
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    for name in ("CCREC_FUSED_ENCODER_TRAIN", "CCREC_FUSED_ENCODER_TRAIN_PACKED", "CCREC_FUSED_ENCODER_TRAIN_DROPOUT"):
        monkeypatch.delenv(name, raising=False)
    return NaiveItemTower(_tiny_model(kind, dropout=dropout), torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_one_pass_fine_tune_step_on_the_packed_path(kind, dtype, monkeypatch):
    """Both opt-ins and one_pass=True vs the fp32 module's three-pass step, under test_fine_tune_step_through_the_layer_kernels' own bars
    with the autocast module as the yardstick: per parameter relative L2 error <= 1.5 x the module's (floor 2^-8 bf16 / 2^-11 fp16), cosine
    >= the module's - 1e-3, the key-bias rule, the loss within 1.5 x the module's deviation (floor one spacing).  One encoder forward: two
    attention calls, not six; the word table's gradient is exactly +0 on the rows of tokens that are not in the batch."""
    from ccrec_amd import ops
    tower = _tower(kind, monkeypatch)
    ids, mask = _stack_batch()
    attention, embed, pooled = (_count(monkeypatch, ops, n) for n in ("attention_train", "embed_layernorm_train", "meanpool_packed"))
    loss32, g32 = _step(tower, ids, mask, None, False)
    loss_m, g_m = _step(tower, ids, mask, dtype, False)
    assert not attention and not embed and not pooled
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_PACKED", "1")
    loss_k, g_k = _step(tower, ids, mask, dtype, True)
    assert len(attention) == 2 and len(embed) == 1 and len(pooled) == 1
    pooler = {n for n in g32 if n.startswith("pooler.")}
    assert set(g_k) == set(g32) - pooler and set(g_m) - pooler == set(g_k)
    floor = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    worst = (0.0, None)
    for name in sorted(g_k):
        ref = g32[name].double()
        assert torch.isfinite(g_k[name]).all() and g_k[name].dtype == torch.float32
        if name.endswith(_KEY_BIAS):      # identically zero: only its size is checked (test_gpu_encoder_train.py says why)
            scale = g32[name.replace("key.bias", "query.bias").replace("k_lin.bias", "q_lin.bias")].double().norm().item()
            assert g_k[name].double().norm().item() <= max(1.5 * g_m[name].double().norm().item(), floor * scale), (name, g_k[name].norm().item(), scale)
            continue
        rel_k = ((g_k[name].double() - ref).norm() / ref.norm()).item()
        rel_m = ((g_m[name].double() - ref).norm() / ref.norm()).item()
        cos_k = F.cosine_similarity(g_k[name].double().flatten(), ref.flatten(), dim=0).item()
        cos_m = F.cosine_similarity(g_m[name].double().flatten(), ref.flatten(), dim=0).item()
        worst = max(worst, (rel_k / max(rel_m, floor), name))
        assert rel_k <= max(1.5 * rel_m, floor), (name, rel_k, rel_m)
        assert cos_k >= cos_m - 1e-3, (name, cos_k, cos_m)
    print(f"one-pass step {kind} {str(dtype)[6:]}: loss fp32 {loss32:.6f} module {loss_m:.6f} kernels {loss_k:.6f}; "
          f"worst relative-L2 ratio kernel / max(module, floor) {worst[0]:.2f} ({worst[1]})")
    assert abs(loss_k - loss32) <= max(1.5 * abs(loss_m - loss32), _spacing(loss32, dtype)), (loss_k, loss_m, loss32)
    word = next(g for n, g in g_k.items() if n.endswith("word_embeddings.weight"))
    unused = torch.ones(word.shape[0], dtype=torch.bool, device="cuda")
    unused[ids[mask.bool()]] = False
    assert unused.any() and (_bits(word[unused]) == 0).all() and (word[~unused] != 0).any()


def test_one_pass_step_with_dropout_repeats_under_a_seed(monkeypatch):
    """Dropout 0.1 with the dropout opt-in on top: the same torch.manual_seed repeats the loss and every gradient bit for bit (no atomics
    anywhere, the keep bits are a function of the seed); another seed moves the loss."""
    tower = _tower("bert", monkeypatch, dropout=0.1)
    ids, mask = _stack_batch()
    for name in ("CCREC_FUSED_ENCODER_TRAIN", "CCREC_FUSED_ENCODER_TRAIN_PACKED", "CCREC_FUSED_ENCODER_TRAIN_DROPOUT"):
        monkeypatch.setenv(name, "1")
    runs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        runs.append(_step(tower, ids, mask, torch.bfloat16, True))
    (l_a, g_a), (l_b, g_b), (l_c, _) = runs
    assert l_a == l_b and set(g_a) == set(g_b) and all(_same(g_a[n], g_b[n]) for n in g_a)
    assert l_c != l_a


def test_the_packed_path_is_opt_in(monkeypatch):
    """Without CCREC_FUSED_ENCODER_TRAIN_PACKED=1 -- and with it but without CCREC_FUSED_ENCODER_TRAIN=1 -- _embed_train and the tower take
    today's path: no call of the new ops, the padded pooling runs."""
    from ccrec_amd import ops
    tower = _tower("bert", monkeypatch).eval()
    ids, mask = _stack_batch()
    attention, embed, pooled, padded = (_count(monkeypatch, ops, n) for n in ("attention_train", "embed_layernorm_train", "meanpool_packed", "meanpool"))
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    _step(tower, ids, mask, torch.bfloat16, False)
    assert len(attention) == 6 and len(padded) == 3 and not embed and not pooled
    monkeypatch.delenv("CCREC_FUSED_ENCODER_TRAIN")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN_PACKED", "1")
    _step(tower, ids, mask, torch.bfloat16, False)
    assert len(attention) == 6 and len(padded) == 6 and not embed and not pooled      # the module ran
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    _step(tower, ids, mask, torch.bfloat16, False)                                     # both: three packed passes
    assert len(attention) == 12 and len(padded) == 6 and len(embed) == 3 and len(pooled) == 3


# ----------------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_return_an_error_code_and_launch_nothing():
    """A null pointer, a dim that is not a multiple of 256 and a short workspace: an error code, the outputs keep their bytes."""
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    c = _block(8, 256, seed=6)
    p, st, code = ops._ptr, ops._stream(c["word"]), _lib.DTYPE_BF16
    f32, b16 = torch.full((8, 256), 7.0, device="cuda"), torch.full((8, 256), 7.0, dtype=torch.bfloat16, device="cuda")

    def fwd(word=c["word"], dim=256, inv_keep=c["inv_keep"]):
        return lib.ccr_embed_layernorm_train_half(p(word), 50, p(c["pos"]), 40, p(c["types"]), 2, p(c["ids"]), p(c["positions"]), p(c["tt"]),
                                                  p(c["gamma"]), p(c["beta"]), LN_EPS, p(c["bits"]), inv_keep, p(f32), p(b16), 8, dim, code, st)

    assert fwd(word=None) == _lib.CCR_ERR_INVALID and fwd(dim=320) == _lib.CCR_ERR_INVALID and fwd(inv_keep=0.5) == _lib.CCR_ERR_INVALID
    d_x, d_gamma = torch.full((8, 256), 7.0, device="cuda"), torch.full((256,), 7.0, device="cuda")
    ws = torch.empty(2 * 2 * 256 * 4, dtype=torch.uint8, device="cuda")

    def bwd(d_y=c["d_y"], dim=256, ws=ws, ws_bytes=2 * 2 * 256 * 4):
        return lib.ccr_embed_layernorm_bwd_half(p(c["word"]), 50, p(c["pos"]), 40, p(c["types"]), 2, p(c["ids"]), p(c["positions"]), p(c["tt"]),
                                                p(c["gamma"]), LN_EPS, None, 1.0, p(d_y), p(d_x), p(d_gamma), None, 8, dim, p(ws), ws_bytes, st)

    assert bwd(d_y=None) == _lib.CCR_ERR_INVALID and bwd(dim=320) == _lib.CCR_ERR_INVALID
    assert bwd(ws_bytes=2 * 2 * 256 * 4 - 1) == _lib.CCR_ERR_WORKSPACE and b"workspace" in lib.ccr_last_error()
    assert bwd(ws=None, ws_bytes=0) == _lib.CCR_ERR_WORKSPACE
    grad = torch.full((50, 256), 7.0, device="cuda")
    order = torch.arange(8, device="cuda")
    assert lib.ccr_embedding_grad(p(c["ids"]), None, p(c["d_y"]), 8, 256, p(grad), 50, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_embedding_grad(p(c["ids"]), p(order), p(c["d_y"]), 8, 254, p(grad), 50, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_embedding_grad(p(c["ids"]), p(order), p(c["d_y"]), 8, 256, None, 50, st) == _lib.CCR_ERR_INVALID
    seq = torch.tensor([0, 4], dtype=torch.int32, device="cuda")
    assert lib.ccr_meanpool_bwd_packed(p(c["d_y"]), p(seq), None, p(d_x), _lib.DTYPE_F32, 2, 256, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_meanpool_bwd_packed(p(c["d_y"]), p(seq), p(seq), p(d_x), _lib.DTYPE_F32, 2, 254, st) == _lib.CCR_ERR_INVALID
    assert lib.ccr_meanpool_bwd_packed(p(c["d_y"]), p(seq), p(seq), p(d_x), 9, 2, 256, st) == _lib.CCR_ERR_INVALID
    torch.cuda.synchronize()
    assert (f32 == 7).all() and (b16 == 7).all() and (d_x == 7).all() and (d_gamma == 7).all() and (grad == 7).all()
