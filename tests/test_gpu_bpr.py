"""GPU parity of the bpr objective (ccr_bpr_*, ops.bpr_*, bbpr_loss.BprStep): the sampler against a numpy fp64 restatement of
softmax(f(prior) + log proposal) drawn by inverse CDF, the fused frozen-tower loss and its gradients against a torch fp64
restatement of bbpr.py:144-147, 180-185 on the CPU, and the step end to end."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import (LAST_U, check_draws, check_grad, check_loss, dense_weights, frozen_problem, make_prior, restate_frozen, run_frozen,
                     run_sampler)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- sampler
def test_sampler_rows_of_0_to_40_entries():
    n_users, n_items, B, n_neg = 300, 3001, 257, 10
    prior = make_prior(n_users, n_items, lambda u: u % 41, lambda rng, m: rng.normal(size=m) * 2, seed=1)
    rng = np.random.default_rng(2)
    users = rng.integers(0, n_users, B)
    users[0], users[1], users[2], users[3] = 0, 41, 40, 40      # two empty rows, and one user twice
    got, proposal, cdf, uniforms = run_sampler(users, n_neg, n_items, prior, 0.0)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    assert not np.array_equal(got[:, 2], got[:, 3])             # the same user, other uniforms


def test_sampler_one_row_one_draw():
    prior = make_prior(1, 5, lambda u: 2, lambda rng, m: rng.normal(size=m), seed=3)
    got, proposal, cdf, uniforms = run_sampler([0], 1, 5, prior, 0.0)
    check_draws(got, [0], prior, 0.0, proposal, cdf, uniforms)


def test_sampler_row_of_4096_entries_and_refusal_of_4097():
    from ccrec_amd import _lib
    prior = make_prior(8, 5000, lambda u: 4096 if u == 5 else u, lambda rng, m: rng.normal(size=m), seed=4)
    users = np.arange(8)
    got, proposal, cdf, uniforms = run_sampler(users, 4, 5000, prior, 0.0)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    longer = make_prior(2, 5000, lambda u: 4097 if u == 1 else 3, lambda rng, m: rng.normal(size=m), seed=5)
    with pytest.raises(_lib.CcrError, match=r"\(-1\).*4096"):   # CCR_ERR_INVALID
        run_sampler([0, 1], 4, 5000, longer, 0.0)


def test_sampler_without_a_prior():
    users = np.zeros(100, dtype=np.int64)
    got, proposal, cdf, uniforms = run_sampler(users, 7, 1234, None, 0.0)
    check_draws(got, users, None, 0.0, proposal, cdf, uniforms)


def test_sampler_reranking_prior_1e5_draws_only_those_entries():
    n_users, n_items = 20, 2000
    prior = make_prior(n_users, n_items, lambda u: 3 + u, lambda rng, m: np.where(np.arange(m) % 3 == 1, 1e5, 1.0), seed=6)
    users = np.arange(n_users)
    got, proposal, cdf, uniforms = run_sampler(users, 10, n_items, prior, 0.0)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    ptr, idx, t = prior
    for b, u in enumerate(users):
        assert set(got[:, b]) <= set(idx[ptr[u]:ptr[u + 1]][t[ptr[u]:ptr[u + 1]] == 1e5])


def test_sampler_entries_below_t0_give_negative_corrections():
    n_users, n_items = 50, 777
    prior = make_prior(n_users, n_items, lambda u: 5 + u % 30, lambda rng, m: 3.0 + rng.uniform(-4, 2, size=m), seed=7)
    assert (prior[2] < 3).any() and (prior[2] > 3).any()
    users = np.arange(n_users)
    got, proposal, cdf, uniforms = run_sampler(users, 10, n_items, prior, 3.0)
    check_draws(got, users, prior, 3.0, proposal, cdf, uniforms)


@pytest.mark.parametrize("case", ["plain", "1e5", "below_t0", "no_prior"])
def test_sampler_edge_uniforms(case):
    """u = 0 draws the first item of non-zero weight, u = 1 - 2^-53 the last one."""
    n_users, n_items, t0 = 12, 500, 0.0
    if case == "plain":
        prior = make_prior(n_users, n_items, lambda u: 3 * u, lambda rng, m: rng.normal(size=m) * 2, seed=8)
    elif case == "1e5":
        prior = make_prior(n_users, n_items, lambda u: 2 + u, lambda rng, m: np.where(np.arange(m) % 2 == 1, 1e5, 1.0), seed=9)
    elif case == "below_t0":
        prior, t0 = make_prior(n_users, n_items, lambda u: 2 + 5 * u, lambda rng, m: 3.0 + rng.uniform(-4, 2, size=m), seed=10), 3.0
    else:
        prior = None
    users = np.arange(n_users)
    uniforms = np.stack([np.zeros(n_users), np.full(n_users, LAST_U)])
    got, proposal, cdf, _ = run_sampler(users, 2, n_items, prior, t0, uniforms=uniforms)
    for b, u in enumerate(users):
        nz = np.nonzero(dense_weights(u, prior, t0, proposal))[0]
        assert got[0, b] == nz[0] and got[1, b] == nz[-1], (case, b, got[:, b], nz[0], nz[-1])
        if case == "1e5":
            assert nz[0] > 0 or nz[-1] < n_items - 1   # (the zero-weight head or tail is really there)


def test_sampler_marks_a_user_outside_the_prior():
    prior = make_prior(4, 50, lambda u: 2, lambda rng, m: rng.normal(size=m), seed=11)
    got, *_ = run_sampler([1, 4, -1, 3], 3, 50, prior, 0.0)
    assert (got[:, [1, 2]] == -1).all() and (got[:, [0, 3]] >= 0).all() and (got[:, [0, 3]] < 50).all()


# ---------------------------------------------------------------------------------------------- frozen loss
@pytest.mark.parametrize("B,n_neg,dim,n_rows,gamma_scale", [(1, 1, 64, 3, 0.05), (33, 10, 768, 500, 0.05), (257, 3, 256, 1000, 0.05),
                                                          (64, 10, 2048, 100, 0.05), (33, 10, 768, 500, 1.0)])
def test_frozen_loss_and_gradients_vs_fp64_restatement(B, n_neg, dim, n_rows, gamma_scale):
    eps = 1e-5
    prob = frozen_problem(B, n_neg, dim, n_rows, gamma_scale)
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = prob
    ref, dg, db, D = restate_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w)
    print(f"max |D| {float(D.abs().max()):.3f}")
    if gamma_scale == 1.0:
        assert float(D.abs().max()) > 100      # the saturated case: exp(|D|) would overflow fp32
    loss, gg, gb = run_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w)
    assert math.isfinite(float(loss))
    check_loss(float(loss), ref)
    check_grad(gg, dg, 3.0, "dgamma")
    check_grad(gb, db, 3.0, "dbeta")
    # the same bits from a second run, and grad_out scales the unit gradient exactly
    loss2, gg2, gb2 = run_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(gg2.view(torch.int32), gg.view(torch.int32)) and torch.equal(gb2.view(torch.int32), gb.view(torch.int32))
    _, gg1, gb1 = run_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    assert torch.equal(gg, 3.0 * gg1) and torch.equal(gb, 3.0 * gb1)


def test_frozen_duplicate_pointer_gives_a_difference_of_exactly_zero():
    """ptr_nj == ptr_j: loss = softplus(0) = ln 2 whatever the rows hold (gamma = 1: the two products are in the hundreds)."""
    from ccrec_amd import ops
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = frozen_problem(16, 1, 768, 50, 1.0, seed=5)
    w = torch.ones(16)
    loss = ops.bpr_frozen_loss(table.cuda(), gamma.cuda(), beta.cuda(), 1e-5, ptr_i.cuda(), ptr_j.cuda(), ptr_j[None].cuda(), w.cuda())
    assert abs(float(loss) - math.log(2.0)) <= 6e-8


def test_frozen_all_zero_weights_and_a_pointer_outside_the_table_give_nan():
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = frozen_problem(20, 3, 128, 40)
    loss, gg, gb = run_frozen(table, gamma, beta, 1e-5, ptr_i, ptr_j, ptr_nj, torch.zeros(20))
    assert math.isnan(float(loss)) and torch.isnan(gg).all() and torch.isnan(gb).all()
    for where, value in (("i", 40), ("j", -1), ("nj", 1 << 40)):
        pi, pj, pnj = ptr_i.clone(), ptr_j.clone(), ptr_nj.clone()
        {"i": pi, "j": pj, "nj": pnj[2]}[where][7] = value
        loss, gg, gb = run_frozen(table, gamma, beta, 1e-5, pi, pj, pnj, w)
        assert math.isnan(float(loss)) and torch.isnan(gg).all() and torch.isnan(gb).all(), where


def test_frozen_without_affine_runs_forward_only_and_odd_widths_are_refused():
    from ccrec_amd import _lib, ops
    table, _, _, ptr_i, ptr_j, ptr_nj, w = frozen_problem(20, 3, 128, 40, 1.0)
    ref, _, _, _ = restate_frozen(table, None, None, 1e-5, ptr_i, ptr_j, ptr_nj, w)
    tc, pi, pj, pnj, wc = table.cuda(), ptr_i.cuda(), ptr_j.cuda(), ptr_nj.cuda(), w.cuda()
    loss = ops.bpr_frozen_loss(tc, None, None, 1e-5, pi, pj, pnj, wc)
    check_loss(float(loss), ref)
    lib = _lib.load()
    ws = torch.empty(int(lib.ccr_bpr_frozen_workspace_bytes(20, 3, 128)), dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, 128, device="cuda")
    one = torch.ones(1, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.ccr_bpr_frozen_bwd_dev(p(tc), 40, 128, None, None, 1e-5, p(pi), p(pj), p(pnj), p(wc), 20, 3, p(one), p(one), p(out[0]), p(out[1]),
                                    p(ws), ws.numel(), None)
    assert rc == _lib.CCR_ERR_INVALID and b"gamma" in lib.ccr_last_error()
    # dim = 72: CCR_ERR_INVALID from the entry point (and no workspace size)
    t72 = torch.randn(40, 72, device="cuda")
    out3 = torch.zeros(3, device="cuda")
    rc = lib.ccr_bpr_frozen_fwd(p(t72), 40, 72, None, None, 1e-5, p(pi), p(pj), p(pnj), p(wc), 20, 3, p(out3), p(ws), ws.numel(), None)
    assert rc == _lib.CCR_ERR_INVALID and b"dim" in lib.ccr_last_error()
    assert lib.ccr_bpr_frozen_workspace_bytes(20, 3, 72) == 0


# ---------------------------------------------------------------------------------------------- BprStep end to end
def step_problem(dim, seed=0):
    g = torch.Generator().manual_seed(seed)
    n_users, n_items, B = 40, 300, 64
    n_rows = n_users + n_items
    table = torch.randn(n_rows, dim, generator=g)
    perm = torch.randperm(n_rows, generator=g)
    i_to_ptr, j_to_ptr = perm[:n_users].clone(), perm[n_users:].clone()
    item_freq = torch.randint(0, 30, (n_items,), generator=g).numpy()
    nnz = 400
    idx = torch.stack([torch.randint(0, n_users, (nnz,), generator=g), torch.randint(0, n_items, (nnz,), generator=g)])
    prior = torch.sparse_coo_tensor(idx, torch.rand(nnz, generator=g) * 3, (n_users, n_items))
    batch = torch.stack([torch.randint(0, n_users, (B,), generator=g).float(), torch.randint(0, n_items, (B,), generator=g).float(),
                         torch.rand(B, generator=g) + 0.1], 1)
    batch[::5, 2] = 0.0
    ln = torch.nn.LayerNorm(dim)
    with torch.no_grad():
        ln.weight.copy_(0.1 * (1.0 + 0.2 * torch.randn(dim, generator=g)))
        ln.bias.copy_(0.02 * torch.randn(dim, generator=g))
    return table, i_to_ptr, j_to_ptr, item_freq, prior, batch, ln


def restate_step(table, ln, i_to_ptr, j_to_ptr, batch, nj):
    """bbpr.py:153-185 in torch fp64 on the CPU, fed the step's own negatives."""
    i, j, w = batch.cpu().T
    i, j = i.to(int), j.to(int)
    return restate_frozen(table, ln.weight, ln.bias, ln.eps, i_to_ptr[i], j_to_ptr[j], j_to_ptr[nj.cpu()], w)[:3]


@pytest.mark.parametrize("dim", [128, 72])
def test_step_fused_and_torch_paths_vs_fp64_restatement(dim):
    """dim 128: all_cls takes the fused kernel; dim 72: the step falls back to its torch formulation.  Both match the restatement, and
    a step built on `forward` (the unfrozen path) draws the same negatives from the same generator and gives the same loss."""
    import copy
    from ccrec_amd import BprStep
    table, i_to_ptr, j_to_ptr, item_freq, prior, batch, ln = step_problem(dim)
    tc, bc = table.cuda(), batch.cuda()
    fcn = lambda x: 2 * x
    ln_a, ln_b = copy.deepcopy(ln).cuda(), copy.deepcopy(ln).cuda()
    fused = BprStep(None, i_to_ptr, j_to_ptr, item_freq, tr_prior_score=prior, training_prior_fcn=fcn, all_cls=tc, layer_norm=ln_a,
                    valid_n_negatives=3, generator=torch.Generator(device="cuda").manual_seed(11))
    plain = BprStep(lambda ptr: ln_b(tc[ptr]), i_to_ptr, j_to_ptr, item_freq, tr_prior_score=prior, training_prior_fcn=fcn,
                    generator=torch.Generator(device="cuda").manual_seed(11))
    assert fused.n_negatives == 10 and fused.training
    loss_a = fused(bc)
    loss_a.backward()
    nj = fused.last_negatives
    assert nj.shape == (10, 64) and int(nj.min()) >= 0 and int(nj.max()) < 300
    ref, dg, db = restate_step(table, ln, i_to_ptr, j_to_ptr, batch, nj)
    check_loss(float(loss_a.detach()), ref)
    check_grad(ln_a.weight.grad, dg, what="dgamma")
    check_grad(ln_a.bias.grad, db, what="dbeta")
    loss_b = plain(bc)
    loss_b.backward()
    assert torch.equal(plain.last_negatives, nj)
    check_loss(float(loss_b.detach()), ref)
    check_loss(float(loss_b.detach()), float(loss_a.detach()))
    check_grad(ln_b.weight.grad, dg, what="dgamma (torch path)")
    # evaluation mode draws valid_n_negatives
    fused.eval()
    loss_v = fused(bc)
    assert fused.last_negatives.shape == (3, 64)
    check_loss(float(loss_v.detach()), restate_step(table, ln, i_to_ptr, j_to_ptr, batch, fused.last_negatives)[0])


def test_step_negatives_follow_the_prior():
    """A prior of 1e5 on one item per user (training_prior_fcn = identity): every negative is that item."""
    from ccrec_amd import BprStep
    table, i_to_ptr, j_to_ptr, item_freq, _, batch, ln = step_problem(128, seed=1)
    users = torch.arange(40)
    prior = torch.sparse_coo_tensor(torch.stack([users, (users * 7) % 300]), torch.full((40,), 1e5), (40, 300))
    step = BprStep(None, i_to_ptr, j_to_ptr, item_freq, tr_prior_score=prior, all_cls=table.cuda(), layer_norm=ln.cuda(), n_negatives=4)
    step(batch.cuda())
    i = batch[:, 0].to(int)
    assert torch.equal(step.last_negatives.cpu(), ((i * 7) % 300).expand(4, -1))
