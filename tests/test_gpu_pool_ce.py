"""GPU parity of the pool contrastive loss (ccr_pool_ce_*, ops.pool_ce, dist.gathered_pool_ce) against a torch fp64 restatement on
the CPU, against the square kernels it generalises and against the reference's own golden loss and gradients."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from test_cpu_pool_ce import _run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def restate(q, c, labels, weights, inv_t):
    """loss = sum w ce / sum w and its gradients (grad_out = 1) in torch fp64 on the CPU."""
    Q = q.detach().cpu().double().requires_grad_(True)
    C = c.detach().cpu().double().requires_grad_(True)
    s = Q @ C.T * inv_t
    ce = torch.logsumexp(s, 1) - s.gather(1, labels.cpu().long()[:, None])[:, 0]
    w = weights.detach().cpu().double() if weights is not None else torch.ones_like(ce)
    loss = (w * ce).sum() / w.sum()
    loss.backward()
    return float(loss), Q.grad.numpy(), C.grad.numpy()


def check_loss(got, ref):
    print(f"loss {got!r} ref {ref!r} err {abs(got - ref):.3e}")
    assert abs(got - ref) < 2e-5 * max(1.0, abs(ref))


def check_grad(got, ref, scale=1.0, what=""):
    """test_fwd_bwd_vs_oracle's bounds: rtol 2e-4 plus atol 3e-6 * max(1e-6, max |ref|) * 100, ref at grad_out = 1."""
    got = got.detach().float().cpu().numpy()
    print(f"{what} max |got - ref| {np.abs(got - scale * ref).max():.3e} of max |ref| {np.abs(scale * ref).max():.3e}")
    np.testing.assert_allclose(got, scale * ref, rtol=2e-4, atol=3e-6 * max(1e-6, np.abs(ref).max()) * 100)


def problem(n_q, n_c, dim, seed=None):
    g = torch.Generator().manual_seed(n_q * 31 + n_c if seed is None else seed)
    q = (torch.randn(n_q, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).float()
    c = (torch.randn(n_c, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).float()
    labels = torch.randint(0, n_c, (n_q,), generator=g)
    w = torch.rand(n_q, generator=g) + 0.1
    w[::5] = 0.0
    return q, c, labels, w


@pytest.mark.parametrize("n_q,n_c,dim", [(1024, 8192, 768), (1024, 16384, 768), (100, 400, 64), (33, 66, 1024), (30, 150, 768), (1, 1, 16),
                                         (7, 4096, 136)])
def test_fwd_bwd_vs_fp64_restatement(n_q, n_c, dim):
    from ccrec_amd import ops
    q, c, labels, w = problem(n_q, n_c, dim)
    if n_q == 1:
        w[0] = 0.7      # (the only query must carry weight: sum w = 0 is its own test)
    inv_t = 20.0
    qc, cc = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    loss = ops.pool_ce(qc, cc, labels.cuda(), inv_t, weights=w.cuda())
    (loss * 3.0).backward()
    ref, dQ, dC = restate(q, c, labels, w, inv_t)
    check_loss(float(loss), ref)
    check_grad(qc.grad, dQ, 3.0, "dQ")
    check_grad(cc.grad, dC, 3.0, "dC")
    zero = (w == 0).nonzero()[:, 0]
    assert (qc.grad[zero.cuda()] == 0).all()          # a query without weight pulls on nothing: exactly zero
    # deterministic: the same bits from a second forward and backward
    q2, c2 = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    loss2 = ops.pool_ce(q2, c2, labels.cuda(), inv_t, weights=w.cuda())
    (loss2 * 3.0).backward()
    assert torch.equal(loss2.detach().view(torch.int32), loss.detach().view(torch.int32))
    assert torch.equal(q2.grad.view(torch.int32), qc.grad.view(torch.int32)) and torch.equal(c2.grad.view(torch.int32), cc.grad.view(torch.int32))


@pytest.mark.parametrize("B,dim", [(32, 256), (1024, 768)])
def test_agrees_with_the_square_kernels(B, dim):
    """C = [P ; N], labels arange(B), no weights: the loss ops.inbatch_ce computes."""
    from ccrec_amd import ops
    g = torch.Generator().manual_seed(B)
    q, p, n = ((torch.randn(B, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).float().cuda() for _ in range(3))
    a, b, c = (t.clone().requires_grad_(True) for t in (q, p, n))
    sq = ops.inbatch_ce(a, b, c, 20.0)
    sq.backward()
    q2, pool = q.clone().requires_grad_(True), torch.cat([p, n]).requires_grad_(True)
    loss = ops.pool_ce(q2, pool, torch.arange(B, device="cuda"), 20.0)
    loss.backward()
    check_loss(float(loss), float(sq))
    check_grad(q2.grad, a.grad.cpu().numpy(), 1.0, "dQ")
    check_grad(pool.grad, torch.cat([b.grad, c.grad]).cpu().numpy(), 1.0, "dP ; dN")


@pytest.mark.parametrize("tag,B,sim", [("b8_dot", 8, "dot"), ("b32_dot", 32, "dot"), ("b8_cos", 8, "cos"), ("b32_cos", 32, "cos")])
def test_loss_and_grads_vs_reference_golden(golden_dir, tag, B, sim):
    """Fixture g7 (the reference's own loss and gradients, fp32): the bounds test_gpu_inbatch.py uses, 1e-3 and 1e-2."""
    from ccrec_amd import ops
    g = np.load(os.path.join(golden_dir, "g7_contrastive.npz"))
    E = torch.from_numpy(g[f"{tag}_E"]).cuda().requires_grad_(True)
    X = torch.nn.functional.normalize(E, p=2, dim=1) if sim == "cos" else E
    loss = ops.pool_ce(X[:B], X[B:], torch.arange(B, device="cuda"), 20.0)
    loss.backward()
    assert abs(float(loss) - float(g[f"{tag}_loss"])) < 1e-3 * max(1.0, abs(float(g[f"{tag}_loss"])))
    ref = g[f"{tag}_grad"]
    assert np.abs(E.grad.cpu().numpy() - ref).max() < 1e-2 * np.abs(ref).max()


def test_multiple_nrl_loss_defaults_are_the_square_kernels_bit_for_bit():
    from ccrec_amd import ops
    from ccrec_amd.bbpr_loss import multiple_nrl_loss
    g = torch.Generator().manual_seed(3)
    q, p, n = (torch.randn(96, 128, generator=g).cuda() * 128 ** -0.5 for _ in range(3))
    a, b, c = (t.clone().requires_grad_(True) for t in (q, p, n))
    ops.inbatch_ce(a, b, c, 20.0).backward()
    a2, b2, c2 = (t.clone().requires_grad_(True) for t in (q, p, n))
    loss = multiple_nrl_loss(a2, b2, c2, inv_temperature=20.0, sim_type="dot")
    loss.backward()
    assert torch.equal(loss.detach().view(torch.int32), ops.inbatch_ce(q, p, n, 20.0).view(torch.int32))
    for x, y in ((a, a2), (b, b2), (c, c2)):
        assert torch.equal(x.grad.view(torch.int32), y.grad.view(torch.int32))


def test_several_negatives_and_weights_through_multiple_nrl_loss():
    from ccrec_amd.bbpr_loss import multiple_nrl_loss
    B, dim = 48, 64
    g = torch.Generator().manual_seed(4)
    q, p = ((torch.randn(B, dim, generator=g) / 8).to(torch.bfloat16).float() for _ in range(2))
    n = (torch.randn(3 * B, dim, generator=g) / 8).to(torch.bfloat16).float()
    w = torch.rand(B, generator=g) + 0.1
    labels = torch.arange(B)
    # 3 B negatives, no weights
    a, b, c = (t.cuda().requires_grad_(True) for t in (q, p, n))
    loss = multiple_nrl_loss(a, b, c, inv_temperature=20.0, sim_type="dot")
    loss.backward()
    ref, dQ, dC = restate(q, torch.cat([p, n]), labels, None, 20.0)
    check_loss(float(loss), ref)
    check_grad(a.grad, dQ, 1.0, "dQ")
    check_grad(torch.cat([b.grad, c.grad]), dC, 1.0, "dP ; dN")
    # weights of all ones = the unweighted call
    a1, b1, c1 = (t.cuda().requires_grad_(True) for t in (q, p, n))
    ones = multiple_nrl_loss(a1, b1, c1, inv_temperature=20.0, sim_type="dot", weights=torch.ones(B).cuda())
    ones.backward()
    check_loss(float(ones), float(loss))
    check_grad(a1.grad, a.grad.cpu().numpy(), 1.0, "dQ, w = 1")
    check_grad(c1.grad, c.grad.cpu().numpy(), 1.0, "dN, w = 1")
    # B negatives WITH weights leave the square path; cos normalises in torch first
    a2, b2, c2 = (t.cuda().requires_grad_(True) for t in (q, p, n[:B]))
    wl = multiple_nrl_loss(a2, b2, c2, inv_temperature=20.0, sim_type="cos", weights=w.cuda())
    wl.backward()
    # fp64 restatement of the same call, the normalisation included (the kernel rounds the normalised rows to bf16, the restatement
    # does not: the golden bounds of test_gpu_inbatch.py, 1e-3 on the loss and 1e-2 of the largest gradient)
    q64, p64, n64 = (t.double().requires_grad_(True) for t in (q, p, n[:B]))
    qn, pn, nn = (torch.nn.functional.normalize(t, p=2, dim=1) for t in (q64, p64, n64))
    s = qn @ torch.cat([pn, nn]).T * 20.0
    ce = torch.logsumexp(s, 1) - s.diagonal()
    ref_loss = (w.double() * ce).sum() / w.double().sum()
    ref_loss.backward()
    ref_cos = float(ref_loss)
    print(f"cos + weights: loss {float(wl)!r} ref {ref_cos!r}")
    assert abs(float(wl) - ref_cos) < 1e-3 * max(1.0, abs(ref_cos))
    for got, ref in ((a2.grad, q64.grad), (b2.grad, p64.grad), (c2.grad, n64.grad)):
        err, top = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"cos + weights: max |got - ref| {err:.3e} of max |ref| {top:.3e}")
        assert top > 0 and err < 1e-2 * top
    with pytest.raises(ValueError):
        multiple_nrl_loss(a, b, c[:B + 1], inv_temperature=20.0, sim_type="dot")


def test_training_step_with_three_negatives_and_weights():
    """MultipleNrlStep(n_negatives=3, use_weights=True): three round-robin pops per user, the batch's third column as weights."""
    from ccrec_amd.bbpr_loss import MultipleNrlStep
    os.environ["CCREC_SIM_TYPE"] = "dot"
    os.environ["CCREC_BBPR_INV_TEMPERATURE"] = "20"
    B, dim = 16, 32
    g = torch.Generator().manual_seed(6)
    table = (torch.randn(3 * B, dim, generator=g) / 6).to(torch.bfloat16).float()
    E = table.cuda().requires_grad_(True)
    negs = {u: [(u + 1 + k) % B for k in range(1 + u % 4)] for u in range(B)}   # lists of length 1 .. 4: some cycle
    expect = {u: list(v) for u, v in negs.items()}
    w = torch.rand(B, generator=g) + 0.1
    batch = torch.stack([torch.arange(B).double(), ((torch.arange(B) * 5) % B).double(), w.double()], 1)
    step = MultipleNrlStep(lambda ptr: E[ptr], torch.arange(0, B), torch.arange(B, 2 * B), negs, n_negatives=3, use_weights=True)
    loss = step(batch)
    loss.backward()
    nj = []
    for _ in range(3):
        for u in range(B):
            v = expect[u].pop(0)
            nj.append(v)
            expect[u].append(v)
    assert negs == expect
    pos = B + (torch.arange(B) * 5) % B
    ref, dQ, dC = restate(table[:B], torch.cat([table[pos], table[B + torch.tensor(nj)]]), torch.arange(B), w, 20.0)
    check_loss(float(loss), ref)
    dE = np.zeros((3 * B, dim))
    dE[:B] += dQ
    np.add.at(dE, torch.cat([pos, B + torch.tensor(nj)]).numpy(), dC)      # duplicates count twice, as they would in torch
    check_grad(E.grad, dE, 1.0, "dE")


def test_copy_path_other_dtypes_strides_and_widths():
    """Widths that are no multiple of 8 are zero-padded; fp16 and transposed inputs go through torch copies; gradients come back in
    the inputs' dtypes and shapes; labels and weights receive none."""
    from ccrec_amd import ops
    q, c, labels, w = problem(20, 50, 20, seed=9)
    ref, dQ, dC = restate(q, c, labels, w, 20.0)
    a, b = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    wt = w.cuda().requires_grad_(True)
    loss = ops.pool_ce(a, b, labels.cuda(), 20.0, weights=wt)
    loss.backward()
    check_loss(float(loss), ref)
    assert a.grad.shape == (20, 20) and b.grad.shape == (50, 20) and wt.grad is None
    check_grad(a.grad, dQ, 1.0, "dQ")
    check_grad(b.grad, dC, 1.0, "dC")
    q, c, labels, w = problem(24, 40, 32, seed=10)
    ref, dQ, dC = restate(q.half().to(torch.bfloat16).float(), c, labels, w, 20.0)      # (fp16 -> bf16 rounds again: compare on what the kernel sees)
    a = q.half().cuda().requires_grad_(True)
    b = c.cuda().t().contiguous().t().requires_grad_(True)
    assert not b.is_contiguous()
    loss = ops.pool_ce(a, b, labels.cuda(), 20.0, weights=w.cuda())
    loss.backward()
    check_loss(float(loss), ref)
    assert a.grad.dtype == torch.float16 and b.grad.dtype == torch.float32
    assert torch.allclose(a.grad.float().cpu(), torch.from_numpy(dQ).float(), rtol=1e-2, atol=1e-5)
    check_grad(b.grad, dC, 1.0, "dC")


def test_bad_labels_and_zero_weight_sum_are_loud():
    from ccrec_amd import ops
    q, c, labels, w = problem(40, 130, 64, seed=11)
    for bad in (130, -1, 2 ** 31 - 1):
        lab = labels.clone()
        lab[17] = bad
        a, b = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
        wz = w.clone()
        wz[17] = 0.0                                       # even a query without weight: its label is still wrong
        loss = ops.pool_ce(a, b, lab.cuda(), 20.0, weights=wz.cuda())
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isnan(loss).item() and torch.isnan(a.grad).all() and torch.isnan(b.grad).all()
    a, b = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    loss = ops.pool_ce(a, b, labels.cuda(), 20.0, weights=torch.zeros(40).cuda())
    assert torch.isnan(loss).item()                        # 0 / 0, as the expression gives
    # and a good call right after works: nothing was left broken
    loss = ops.pool_ce(a, b, labels.cuda(), 20.0, weights=w.cuda())
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()


def test_backward_rejects_a_workspace_that_is_not_its_forwards_and_sizes_beyond_the_range():
    from ccrec_amd import _lib, ops
    lib = ops.require_gpu()
    n_q, n_c, dim = 64, 200, 32
    g = torch.Generator().manual_seed(2)
    qb = torch.randn(n_q, dim, generator=g).cuda().to(torch.bfloat16)
    cb = torch.randn(n_c, dim, generator=g).cuda().to(torch.bfloat16)
    cb2 = torch.randn(n_c + 64, dim, generator=g).cuda().to(torch.bfloat16)
    lab = torch.randint(0, n_c, (n_q,), generator=g).to(torch.int32).cuda()
    out3, lse, one = torch.empty(3, device="cuda"), torch.empty(n_q, device="cuda"), torch.ones(1, device="cuda")
    need, need2 = int(lib.ccr_pool_ce_workspace_bytes(n_q, n_c, dim)), int(lib.ccr_pool_ce_workspace_bytes(n_q, n_c + 64, dim))
    assert 0 < need <= need2
    ws, scratch, other = (torch.zeros(need2, dtype=torch.uint8, device="cuda") for _ in range(3))
    scratch.fill_(0x5A)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grads = torch.empty(n_q + n_c, dim, device="cuda")

    def bwd(w, inv_t):
        grads.zero_()
        _lib.check(lib.ccr_pool_ce_bwd_dev(vp(qb), vp(cb), vp(lab), None, vp(lse), n_q, n_c, dim, inv_t, vp(one), None, vp(grads), vp(grads[n_q:]),
                                           vp(w), need2, stream), "bwd")
        torch.cuda.synchronize()
        return grads.clone()

    _lib.check(lib.ccr_pool_ce_fwd(vp(qb), vp(cb), vp(lab), None, n_q, n_c, dim, 20.0, vp(out3), vp(lse), vp(ws), need2, stream), "fwd")
    lse_good = lse.clone()
    good = bwd(ws, 20.0)
    assert torch.isfinite(good).all() and good.abs().max() > 0
    assert torch.isnan(bwd(scratch, 20.0)).all()           # never written by a forward
    assert torch.isnan(bwd(ws, 10.0)).all()                # another temperature's logits
    lse2 = torch.empty(n_q, device="cuda")
    _lib.check(lib.ccr_pool_ce_fwd(vp(qb), vp(cb2), vp(lab), None, n_q, n_c + 64, dim, 20.0, vp(out3), vp(lse2), vp(other), need2, stream), "fwd")
    assert torch.isnan(bwd(other, 20.0)).all()             # another shape's forward
    lse.copy_(lse_good)
    again = bwd(ws, 20.0)
    assert torch.equal(again.view(torch.int32), good.view(torch.int32))
    # sizes beyond the supported range: an error code and a text, nothing launched
    rc = lib.ccr_pool_ce_fwd(vp(qb), vp(cb), vp(lab), None, n_q, (1 << 20) + 1, dim, 20.0, vp(out3), vp(lse), vp(ws), need2, stream)
    assert rc == _lib.CCR_ERR_INVALID and b"beyond the supported range" in lib.ccr_last_error()
    with pytest.raises(_lib.CcrError, match="beyond the supported range"):
        _lib.check(rc, "ccr_pool_ce_fwd")
    rc = lib.ccr_pool_ce_fwd(vp(qb), vp(cb), vp(lab), None, n_q, n_c, dim, 20.0, vp(out3), vp(lse), vp(ws), 1024, stream)
    assert rc == _lib.CCR_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------- cross-rank, real kernels, one GPU
def _rank_main(rank, world, port, case, out_dir):
    sys.path[:0] = [ROOT, PKG]
    import torch.distributed as dist
    from ccrec_amd import ops
    from ccrec_amd.dist import gathered_pool_ce
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    n_q, n_c, dim, inv_t = 96, 200, 128, 20.0
    q, c, labels, w = problem(world * n_q, world * n_c, dim, seed=50 + world)
    labels = labels % n_c                                  # local to each rank's block
    glob = labels + torch.arange(world).repeat_interleave(n_q) * n_c
    Qa, Ca = q.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    whole = ops.pool_ce(Qa, Ca, glob.cuda(), inv_t, weights=w.cuda())
    (whole * 3.0).backward()
    qs, cs = slice(rank * n_q, (rank + 1) * n_q), slice(rank * n_c, (rank + 1) * n_c)
    ql, cl = q[qs].cuda().requires_grad_(True), c[cs].cuda().requires_grad_(True)
    loss = gathered_pool_ce(ql, cl, labels[qs].cuda(), inv_t, weights=w[qs].cuda())
    (loss * 3.0).backward()
    try:
        check_loss(float(loss), float(whole))
        check_grad(ql.grad, Qa.grad[qs].cpu().numpy() / 3.0, 3.0, "dQ")
        check_grad(cl.grad, Ca.grad[cs].cpu().numpy() / 3.0, 3.0, "dC")
        verdict = "ok"
    except AssertionError as e:
        verdict = f"MISMATCH {e}"
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write(verdict)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gathered_loss_with_real_kernels_on_one_gpu(tmp_path, world):
    """`world` processes on this GPU over gloo: every rank's loss and gradients equal the single-process ops.pool_ce over all
    queries and the whole pool.  Every rank runs under a time limit."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert _run_ranks(tmp_path, world, "real", limit=240, script=os.path.abspath(__file__)) == ["ok"] * world


if __name__ == "__main__":
    sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
