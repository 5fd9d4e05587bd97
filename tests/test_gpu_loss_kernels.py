"""The training-side GEMM kernels (csrc/ccr_inbatch.hip, csrc/ccr_poolce.hip) at every tile edge, width class, split count and part:
loss and gradients against fp64 on the same bf16-rounded operands, at the bounds of test_gpu_inbatch.py / test_gpu_pool_ce.py (loss 2e-5,
gradients rtol 2e-4 + atol 3e-4 of the largest); logits of several hundred; and the part probe, whose bound tells three bf16 parts of
the logit gradient from two (helpers.loss_probe_errors; tests/test_cpu_loss_probe.py shows on the CPU that it can fail)."""
import numpy as np
import pytest
import torch

from helpers import INBATCH_PROBE_SHAPES, LOSS_PROBE_INV_T, POOL_PROBE_SHAPES, bf16_round, loss_probe_case, loss_probe_errors, probe_error
from oracle import oracle as orc
from test_gpu_pool_ce import check_grad, check_loss, problem, restate

pytestmark = pytest.mark.gpu

INV_T = 20.0


def _blocks(B, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).float() for _ in range(3)]


def _run_inbatch(q, p, n, inv_t, grad_out=1.0):
    """-> (loss fp32 scalar, [dq, dp, dn], lse [B]) on the device."""
    from ccrec_amd import ops
    a, b, c = (t.cuda().requires_grad_(True) for t in (q, p, n))
    loss = ops.inbatch_ce(a, b, c, inv_t)
    saved = loss.grad_fn.saved_tensors
    lse = saved[0][-4 * q.shape[0]:].view(torch.float32).clone() if len(saved) == 1 and saved[0].dtype == torch.uint8 else None
    (loss * grad_out).backward()
    return loss.detach(), [a.grad, b.grad, c.grad], lse


def _check_inbatch(q, p, n, inv_t, grad_out=1.0):
    loss, grads, _ = _run_inbatch(q, p, n, inv_t, grad_out)
    ref, dQ, dP, dN = orc.inbatch_ce(q.numpy(), p.numpy(), n.numpy(), inv_t, "dot")
    check_loss(float(loss), ref)
    for got, want, what in zip(grads, (dQ, dP, dN), ("dQ", "dP", "dN")):
        assert got.shape == q.shape and got.dtype == torch.float32
        check_grad(got, want, grad_out, what)
    return loss, grads


# ---------------------------------------------------------------------------------------------- A1: width classes of the forward's K loop
@pytest.mark.parametrize("dim", [16, 48, 112, 128, 144, 256, 384, 400, 640])
def test_inbatch_width_classes(dim):
    """dim / 128 full chunks through the two-set prefetch (0, 1, 2, 3: odd, its last half-iteration skipped; 5) and a 16-wide tail of 0,
    1, 3 or 7 steps behind 0, 1 or 3 chunks.  B = 40: the row-major forward, two query tiles (the second partly filled), three key tiles."""
    _check_inbatch(*_blocks(40, dim, 1000 + dim), INV_T)


# ---------------------------------------------------------------------------------------------- A2: fragment-major = row-major = fp64
@pytest.mark.parametrize("B", [32, 64, 96])
@pytest.mark.parametrize("dim", [128, 384, 640])
def test_inbatch_fragment_major_against_row_major_and_fp64(monkeypatch, B, dim):
    q, p, n = _blocks(B, dim, 2000 + B + dim)
    loss_f, grads_f = _check_inbatch(q, p, n, INV_T, 0.5)
    monkeypatch.setenv("CCR_INBATCH_ROWMAJOR", "1")
    loss_r, grads_r = _check_inbatch(q, p, n, INV_T, 0.5)
    assert torch.equal(loss_f.view(torch.int32), loss_r.view(torch.int32))
    assert torch.equal(torch.stack(grads_f).view(torch.int32), torch.stack(grads_r).view(torch.int32))


# ---------------------------------------------------------------------------------------------- A3: B edges
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 97, 160, 161])
def test_inbatch_batch_edges(B):
    """Around one key tile (2B = 32), one and two query tiles, and ldq / 64 chunks that the four waves of inbatch_gemm3_kernel do not
    share evenly (B = 161: 6 chunks, 2 per wave, none for the last).  dim = 144: one chunk + a tail; grad_out = 3."""
    _check_inbatch(*_blocks(B, 144, 3000 + B), INV_T, 3.0)


# ---------------------------------------------------------------------------------------------- A4: split counts of the forward
def _pick_splits(B):
    """pick_splits of csrc/ccr_inbatch.hip, restated: a change of policy fails here instead of moving the cases off their paths."""
    qtiles, ktiles = (B + 31) // 32, (2 * B + 31) // 32
    return max(1, min(2048 // qtiles, ktiles, 64))


@pytest.mark.parametrize("B,qtiles,ktiles,splits", [(272, 9, 17, 17), (1056, 33, 66, 62), (2080, 65, 130, 31)])
def test_inbatch_split_counts(B, qtiles, ktiles, splits):
    """17 splits: one entry in the combine loop's second round of 16; 62: uneven key ranges (66 tiles over 62 splits) and a partial
    fourth round; 31 over 130 tiles: fewer splits than key tiles, 4 or 5 tiles each."""
    assert ((B + 31) // 32, (2 * B + 31) // 32, _pick_splits(B)) == (qtiles, ktiles, splits)
    _check_inbatch(*_blocks(B, 64, 4000 + B), INV_T)


# ---------------------------------------------------------------------------------------------- A5: pool CE tile edges
@pytest.mark.parametrize("n_q,n_c,dim", [(63, 65, 72), (64, 64, 8), (65, 63, 200), (127, 129, 24), (128, 128, 136), (129, 127, 72), (5, 2, 8),
                                         (5, 3, 8), (3, 5, 16), (9, 1023, 72), (9, 1027, 72), (5, 2500, 72), (2500, 70, 72)])
def test_pool_tile_edges(n_q, n_c, dim):
    """The 64-row gradient tile and the 128-row logits tile at 63 .. 65 and 127 .. 129; n_c % 4 = 3 and n_c < 4 through pool_lse_kernel's
    tail; widths 8 x odd (the partly filled last chunk); (5, 2500): dQ in 32 splits over 40 chunks, (2500, 70): dC likewise."""
    from ccrec_amd import ops
    q, c, labels, w = problem(n_q, n_c, dim)
    assert (w == 0).any() and (w > 0).any()
    ref, dQ, dC = restate(q, c, labels, w, INV_T)
    out = []
    for _ in range(2):
        a, b = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
        loss = ops.pool_ce(a, b, labels.cuda(), INV_T, weights=w.cuda())
        (loss * 3.0).backward()
        out.append((loss.detach(), a.grad, b.grad))
    loss, ga, gb = out[0]
    check_loss(float(loss), ref)
    check_grad(ga, dQ, 3.0, "dQ")
    check_grad(gb, dC, 3.0, "dC")
    assert (ga[(w == 0).cuda()] == 0).all()                # a query without weight pulls on nothing: exactly zero
    for x, y in zip(out[0], out[1]):                       # the same bits on a second run
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------------------------- A6: large logits
def _large_logit_problem(n_q, n_c, dim, labels, others, seed):
    """Unit rows times sqrt(450 / inv_T), so <x, x> inv_T = 450 and <x, y> inv_T stays below about 260 for random rows.  Query i, by
    i % 5: 0 -- its label's candidate is the query itself (the label is the maximum by about 200: ce = 0 in fp32, every g underflows);
    1 -- the label is MINUS the query and candidate others[i] the query (-450 against +450: ce = 900); 2 -- the label is minus the query
    (ce about 650); 3, 4 -- random.  Query 3's maximum is the LAST candidate (= query 3)."""
    rs = np.random.RandomState(seed)
    Q, C = rs.standard_normal((n_q, dim)), rs.standard_normal((n_c, dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    for i in range(n_q):
        if i % 5 == 0:
            C[labels[i]] = Q[i]
        elif i % 5 <= 2:
            C[labels[i]] = -Q[i]
            if i % 5 == 1:
                C[others[i]] = Q[i]
    C[n_c - 1] = Q[3]
    gamma = (450.0 / INV_T) ** 0.5
    q, c = (torch.from_numpy(bf16_round((gamma * x).astype(np.float32))) for x in (Q, C))
    s = q.double() @ c.double().T * INV_T
    assert 440 < float(s.abs().max()) < 512                # (fp32 spacing of a logit below 512: 3e-5, inside rtol 2e-4)
    ce = torch.logsumexp(s, 1) - s[torch.arange(n_q), torch.from_numpy(np.asarray(labels))]
    assert float(ce[0::5].max()) < 1e-30 and float(ce[1::5].min()) > 850 and float(ce[2::5].min()) > 500
    assert int(s[3].argmax()) == n_c - 1 and float((s.max(1).values - s.min(1).values).max()) > 850
    return q, c, s


@pytest.mark.parametrize("B", [24, 200])
def test_inbatch_large_logits(B):
    """B = 24: one query tile, two key splits; B = 200: 13 splits, so a row's maximum comes from another split than most of its sum."""
    q, c, s = _large_logit_problem(B, 2 * B, 64, np.arange(B), B + np.arange(B), 5000 + B)
    loss, grads, lse = _run_inbatch(q, c[:B], c[B:], INV_T)
    ref, dQ, dP, dN = orc.inbatch_ce(q.numpy(), c[:B].numpy(), c[B:].numpy(), INV_T, "dot")
    assert np.isfinite(float(loss)) and ref > 100
    check_loss(float(loss), ref)
    lse = lse.cpu().double()
    assert torch.isfinite(lse).all()
    np.testing.assert_allclose(lse.numpy(), torch.logsumexp(s, 1).numpy(), rtol=2e-6, atol=0)    # (fp32: 2^-24, and the logit's own rounding)
    for got, want, what in zip(grads, (dQ, dP, dN), ("dQ", "dP", "dN")):
        assert torch.isfinite(got).all()
        check_grad(got, want, 1.0, what)


@pytest.mark.parametrize("n_q,n_c", [(24, 60), (40, 3000)])
def test_pool_large_logits(n_q, n_c):
    """(24, 60): one tile of everything; (40, 3000): 24 logits tiles per query, dQ over 32 K splits."""
    from ccrec_amd import ops
    rs = np.random.RandomState(n_c)
    perm = rs.permutation(n_c - 1)                          # (the last candidate is query 3's maximum)
    labels, others = perm[:n_q], perm[n_q:2 * n_q]
    q, c, s = _large_logit_problem(n_q, n_c, 64, labels, others, 6000 + n_c)
    w = torch.from_numpy((rs.rand(n_q) + 0.1).astype(np.float32))
    w[4::10] = 0.0
    lab = torch.from_numpy(labels)
    ref, dQ, dC = restate(q, c, lab, w, INV_T)
    a, b = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    out3, state = ops.pool_ce_forward(a.detach(), b.detach(), lab.cuda(), INV_T, w.cuda())
    lse = state[0][-4 * n_q:].view(torch.float32).cpu().double()
    loss = ops.pool_ce(a, b, lab.cuda(), INV_T, weights=w.cuda())
    loss.backward()
    assert np.isfinite(float(loss)) and ref > 100 and float(out3[0]) == float(loss)
    check_loss(float(loss), ref)
    assert torch.isfinite(lse).all()
    np.testing.assert_allclose(lse.numpy(), torch.logsumexp(s, 1).numpy(), rtol=2e-6, atol=0)
    assert torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    check_grad(a.grad, dQ, 1.0, "dQ")
    check_grad(b.grad, dC, 1.0, "dC")


# ---------------------------------------------------------------------------------------------- A7: the part probe
def _probe_verdict(kind, side, got, q, c, labels, w, grad_out, loss):
    ref, ref_loss, e3, e2 = loss_probe_errors(side, q, c, labels, w, grad_out, kind)
    check_loss(float(loss), ref_loss)
    err = probe_error(got.detach().cpu().numpy(), ref)
    print(f"{kind} {side} {tuple(q.shape)} x {tuple(c.shape)}: kernel {err:.3e}  three-part emulation {e3:.3e}  E2 {e2:.3e}  bound E2 / 3 {e2 / 3:.3e}")
    assert err < e2 / 3


@pytest.mark.parametrize("side", ["dq", "dc"])
@pytest.mark.parametrize("B,dim", INBATCH_PROBE_SHAPES)
def test_inbatch_part_probe(B, dim, side):
    """One operand one-hot: every element of dQ (side dq: the keys are one-hot) or of dP | dN (side dc: the queries are) is ONE product
    g * amplitude, so its relative error is the error of g -- lse, exp, the scale, and the THREE bf16 parts: a third of what two parts give."""
    q, c, labels, w, grad_out = loss_probe_case("inbatch", side, B, 2 * B, dim)
    loss, grads, _ = _run_inbatch(*(torch.from_numpy(x) for x in (q, c[:B], c[B:])), LOSS_PROBE_INV_T, grad_out)
    got = grads[0] if side == "dq" else torch.cat(grads[1:])
    _probe_verdict("inbatch", side, got, q, c, labels, w, grad_out, loss)


@pytest.mark.parametrize("side,n_q,n_c,dim", POOL_PROBE_SHAPES)
def test_pool_part_probe(side, n_q, n_c, dim):
    from ccrec_amd import ops
    q, c, labels, w, grad_out = loss_probe_case("pool", side, n_q, n_c, dim)
    a, b = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (q, c))
    loss = ops.pool_ce(a, b, torch.from_numpy(labels).cuda(), LOSS_PROBE_INV_T, weights=torch.from_numpy(w).cuda())
    (loss * grad_out).backward()
    _probe_verdict("pool", side, a.grad if side == "dq" else b.grad, q, c, labels, w, grad_out, loss.detach())


# ---------------------------------------------------------------------------------------------- C: any width through ops.inbatch_ce
@pytest.mark.parametrize("dim", [72, 300, 50, 8])
def test_inbatch_takes_any_width(dim):
    """Widths the square kernels refuse (no multiple of 16) are the same loss in the pool form, zero-padded: ops.inbatch_ce,
    multiple_nrl_loss and MultipleNrlStep's loss at widths 72, 300, 50 and 8 against fp64; gradients in the inputs' shapes and dtypes."""
    from ccrec_amd.bbpr_loss import multiple_nrl_loss
    B = 40
    q, p, n = _blocks(B, dim, 7000 + dim)
    p = torch.where(p.abs() < 2.0 ** -13, torch.zeros_like(p), p)       # (so that every bf16 value of p is an fp16 value too)
    _check_inbatch(q, p, n, INV_T, 3.0)
    ref, dQ, dP, dN = orc.inbatch_ce(q.numpy(), p.numpy(), n.numpy(), INV_T, "dot")
    a, b, c = q.cuda().requires_grad_(True), p.cuda().half().requires_grad_(True), n.cuda().requires_grad_(True)
    assert torch.equal(b.detach().float().cpu(), p)
    loss = multiple_nrl_loss(a, b, c, inv_temperature=INV_T, sim_type="dot")
    loss.backward()
    check_loss(float(loss), ref)
    assert a.grad.shape == b.grad.shape == c.grad.shape == (B, dim)
    assert a.grad.dtype == torch.float32 and b.grad.dtype == torch.float16 and c.grad.dtype == torch.float32
    check_grad(a.grad, dQ, 1.0, "dQ")
    check_grad(c.grad, dN, 1.0, "dN")
    assert torch.allclose(b.grad.float().cpu(), torch.from_numpy(dP).float(), rtol=1e-2, atol=1e-6)       # (an fp16 gradient: test_gpu_inbatch.py's bound)


def test_training_step_at_a_width_the_square_kernels_refuse(monkeypatch):
    """MultipleNrlStep (one negative per user, no weights: the square loss) over a table of width 50."""
    from ccrec_amd.bbpr_loss import MultipleNrlStep
    monkeypatch.setenv("CCREC_SIM_TYPE", "dot")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    B, dim = 16, 50
    g = torch.Generator().manual_seed(9000)
    table = (torch.randn(3 * B, dim, generator=g) / 6).to(torch.bfloat16).float()
    E = table.cuda().requires_grad_(True)
    step = MultipleNrlStep(lambda ptr: E[ptr], torch.arange(0, B), torch.arange(B, 3 * B), {u: [B + u] for u in range(B)})
    loss = step.training_and_validation_step(torch.stack([torch.arange(B), torch.arange(B), torch.ones(B, dtype=torch.long)], 1), 0)
    loss.backward()
    ref, dQ, dP, dN = orc.inbatch_ce(table[:B].numpy(), table[B:2 * B].numpy(), table[2 * B:].numpy(), INV_T, "dot")
    check_loss(float(loss), ref)
    assert E.grad.shape == (3 * B, dim)
    check_grad(E.grad, np.concatenate([dQ, dP, dN]), 1.0, "dE")


def test_inbatch_multiples_of_16_keep_their_bits():
    """The routing is by width alone: at a multiple of 16 ops.inbatch_ce is still the square kernels' autograd function, bit for bit."""
    from ccrec_amd import ops
    q, p, n = (t.cuda() for t in _blocks(40, 48, 8000))
    out = []
    for fn in (ops.inbatch_ce, ops._InBatchCE.apply):
        a, b, c = (t.clone().requires_grad_(True) for t in (q, p, n))
        loss = fn(a, b, c, INV_T)
        loss.backward()
        out.append(torch.cat([loss.detach().reshape(1), a.grad.flatten(), b.grad.flatten(), c.grad.flatten()]))
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
