"""The bpr kernels (csrc/ccr_bpr.hip) where tests/test_gpu_bpr.py does not reach: the backward's row loop past its 512-workgroup cap
(B = 2049 .. 10 000) with ONE live row among zero-weight rows, which must equal the one-row problem exactly; differences D that are exact
integers, so that softplus and sigmoid are read off against fp64 by relative error; every width template and the widths whose last
slot is partly inside the row; n_neg = 4096; the refusals of the C entry points; and the sampler's draw loop, scan carry, overlong
rows, row corners, zero proposals, excluding priors and B in the thousands.  tests/test_cpu_bpr_probe.py checks the probes themselves."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import (BPR_PROBE_KS, LAST_U, bpr_integer_probe, bpr_probe_reference, bpr_relative_error, check_draws, check_grad, check_loss,
                     dense_weights, frozen_problem, make_prior, restate_frozen, run_frozen, run_sampler)

pytestmark = pytest.mark.gpu

EPS = 1e-5
_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def same_floats(a, b):
    """Equal as fp32 values (+0 == -0: a sum of zeros may carry either sign), and finite."""
    return bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- A. one live row among many
def big_problem(B, dim):
    return cached(("big", B, dim), lambda: frozen_problem(B, 2, dim, 500))


def live_row_positions():
    cases = []
    for B in (5, 2048, 2049, 2052, 4100, 10000):
        rows = [0, 3, 2047, 2048, 4097, B - 1] + ([5000, 5001, 5002, 5003] if B == 10000 else [])      # (10 000: one row per wave of a workgroup)
        cases += [(B, 64, b) for b in sorted(set(rows)) if b < B]
    return cases + [(4100, 768, 4097)]


def assert_live_row_identity(prob, b_live):
    """w = 0.7 on row b_live and 0 elsewhere: loss, dgamma and dbeta equal those of the B = 1 problem of that row as fp32 values."""
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, _ = prob
    w = torch.zeros(ptr_i.numel())
    w[b_live] = 0.7
    s = slice(b_live, b_live + 1)
    many = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    one = run_frozen(table, gamma, beta, EPS, ptr_i[s], ptr_j[s], ptr_nj[:, s].contiguous(), w[s], scale=1.0)
    for name, a, b in zip(("loss", "dgamma", "dbeta"), many, one):
        assert same_floats(a, b), f"{name} of row {b_live} among {ptr_i.numel()} differs from the row alone: max |diff| {float((a - b).abs().max()):.3e}"
    assert float(one[0]) > 0 and bool((one[1] != 0).any()) and bool((one[2] != 0).any())


@pytest.mark.parametrize("B,dim,b_live", live_row_positions())
def test_one_live_row_among_zero_weight_rows_equals_the_row_alone(B, dim, b_live):
    prob = big_problem(B, dim)
    if b_live % 3 == 0:      # frozen_problem makes every third row's first negative its positive (D = 0 exactly): keep that in some cases only
        assert int(prob[5][0, b_live]) == int(prob[4][b_live])
    assert_live_row_identity(prob, b_live)


@pytest.mark.parametrize("B", [4100, 10000])
def test_all_rows_live_at_the_training_batch(B):
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, _ = big_problem(B, 64)
    g = torch.Generator().manual_seed(B)
    w = torch.rand(B, generator=g) + 0.1
    ref, dg, db, _ = restate_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w)
    loss, gg, gb = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    check_loss(float(loss), ref)
    check_grad(gg, dg, what="dgamma")
    check_grad(gb, db, what="dbeta")
    loss2, gg2, gb2 = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(gg2.view(torch.int32), gg.view(torch.int32)) and torch.equal(gb2.view(torch.int32), gb.view(torch.int32))
    perm = torch.randperm(B, generator=g)                      # the batch rows in another order: other sums, the same bounds
    loss3, gg3, gb3 = run_frozen(table, gamma, beta, EPS, ptr_i[perm], ptr_j[perm], ptr_nj[:, perm].contiguous(), w[perm], scale=1.0)
    check_loss(float(loss3), ref)
    check_grad(gg3, dg, what="dgamma (permuted)")
    check_grad(gb3, db, what="dbeta (permuted)")


def test_a_bad_pointer_in_a_waves_second_trip_reaches_every_output():
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, _ = big_problem(4100, 64)
    w = torch.full((4100,), 0.5)
    for where in ("i", "nj"):
        pi, pnj = ptr_i.clone(), ptr_nj.clone()
        {"i": pi, "nj": pnj[1]}[where][2050] = table.shape[0]      # row 2050 = 2048 + 2: the second trip of wave 2 of workgroup 0
        loss, gg, gb = run_frozen(table, gamma, beta, EPS, pi, ptr_j, pnj, w, scale=1.0)
        assert math.isnan(float(loss)) and bool(torch.isnan(gg).all()) and bool(torch.isnan(gb).all()), where


# ---------------------------------------------------------------------------------------------- B. integer differences
def run_probes(dim, gamma, variants):
    return cached(("probes", dim, gamma, variants), lambda: _run_probes(dim, gamma, variants))


def _run_probes(dim, gamma, variants):
    """Every k of BPR_PROBE_KS as one B = 1, n_neg = 1, w = 1 call -> per probe (D, loss, dgamma, dbeta, reference tuple)."""
    from ccrec_amd import ops
    probes = [bpr_integer_probe(dim, k, v) for k in BPR_PROBE_KS for v in variants]
    table = torch.from_numpy(np.concatenate([np.stack(p[:3]) for p in probes])).cuda()
    one = torch.ones(1).cuda()
    out = []
    for n, (xi, xj, xn, flipped) in enumerate(probes):
        gc, bc = torch.full((dim,), gamma).cuda().requires_grad_(True), torch.zeros(dim).cuda().requires_grad_(True)
        ptr = torch.tensor([3 * n, 3 * n + 1, 3 * n + 2]).cuda()
        loss = ops.bpr_frozen_loss(table, gc, bc, 0.0, ptr[0:1], ptr[1:2], ptr[2:3].view(1, 1), one)
        loss.backward()
        out.append((float(loss.detach()), gc.grad.cpu().numpy(), bc.grad.cpu().numpy(), flipped, bpr_probe_reference(xi, xj, xn, gamma)))
    return out


def torch_yardstick():
    """The largest relative error of torch's own fp32 softplus(-D) and sigmoid(-D) on the device at the probes' D, against the same fp64
    values, and the bound the kernel is held to: twice the worse of the two plus 2^-22.  Torch is measured where the fp64 value is a
    normal fp32 number: its sigmoid is 1 / (1 + exp(D)), whose exp overflows from D = 92 on, so it returns 0 for values of 1e-40 .. 4e-44
    (measured over the whole range: relative error 1.0, softplus 6.6e-8), and a bound of 2.0 would pass any softplus.  The kernel is held to
    the bound at EVERY D, one subnormal step forgiven below 2^-126: stricter than measuring torch over the whole range."""
    def build():
        Ds = sorted(set([4.0 * k for k in BPR_PROBE_KS] + [float(k) for k in BPR_PROBE_KS]))
        d = torch.tensor(Ds, dtype=torch.float32).cuda()
        sp = torch.nn.functional.softplus(-d).cpu().numpy()
        sg = torch.sigmoid(-d).cpu().numpy()
        ref_sp = np.array([max(-D, 0.0) + math.log1p(math.exp(-abs(D))) for D in Ds])
        ref_sg = np.array([math.exp(-D) / (1 + math.exp(-D)) if D >= 0 else 1 / (1 + math.exp(D)) for D in Ds])
        whole = bpr_relative_error(sp, ref_sp), bpr_relative_error(sg, ref_sg)
        normal_sp, normal_sg = ref_sp >= 2.0 ** -126, ref_sg >= 2.0 ** -126
        assert normal_sp.sum() > 100 and normal_sg.sum() > 100
        e_sp, e_sg = bpr_relative_error(sp[normal_sp], ref_sp[normal_sp]), bpr_relative_error(sg[normal_sg], ref_sg[normal_sg])
        bound = 2 * max(e_sp, e_sg) + 2.0 ** -22
        print(f"torch fp32 on the device, results in the normal range: softplus {e_sp:.3e} sigmoid {e_sg:.3e} -> bound {bound:.3e}; "
              f"over the whole range: softplus {whole[0]:.3e} sigmoid {whole[1]:.3e}")
        return e_sp, e_sg, bound
    return cached("yardstick", build)


@pytest.mark.parametrize("dim,gamma,variants", [(64, 1.0, (0, 1)), (64, 0.5, (0, 1)), (2048, 1.0, (1,))])
def test_integer_differences_read_softplus_and_sigmoid_off_exactly(dim, gamma, variants):
    e_sp, e_sg, bound = torch_yardstick()
    worst = {"loss": 0.0, "dgamma": 0.0, "dbeta": 0.0}
    seen = set()
    for loss, dg, db, flipped, (D, ref_loss, ref_dg, ref_db) in run_probes(dim, gamma, variants):
        seen.add(D)
        rest = np.ones(dim, bool)
        rest[flipped] = False
        assert not dg[rest].any() and not db[rest].any(), f"D = {D}: a gradient outside the flipped columns"
        assert not ref_dg[rest].any() and ref_dg[flipped].all() and ref_db[flipped].all()
        # the gradients are sigmoid(-D) times an exact power of two (dgamma -+4 gamma, dbeta -+2 gamma): divided out, so that the subnormal
        # step is forgiven on the sigmoid itself and not on four times it
        for name, got, ref in (("loss", loss, ref_loss), ("dgamma", dg[flipped].astype(np.float64) / (4 * gamma), ref_dg[flipped] / (4 * gamma)),
                               ("dbeta", db[flipped].astype(np.float64) / (2 * gamma), ref_db[flipped] / (2 * gamma))):
            err = bpr_relative_error(got, ref)
            worst[name] = max(worst[name], err)
            assert err <= bound, f"D = {D}: {name} relative error {err:.3e} > {bound:.3e}"
    step = 4 if gamma == 1.0 else 1
    assert seen == set(float(d) for d in range(-32 * step, 32 * step + 1, step))
    print(f"dim {dim} gamma {gamma}: kernel loss {worst['loss']:.3e} dgamma {worst['dgamma']:.3e} dbeta {worst['dbeta']:.3e}; "
          f"torch softplus {e_sp:.3e} sigmoid {e_sg:.3e}; bound {bound:.3e}")


def test_negative_equal_to_the_positive_gives_ln2_and_no_gradient_at_2048():
    from ccrec_amd import ops
    xi, xj, _, _ = bpr_integer_probe(2048, 5, 1)
    table = torch.from_numpy(np.stack([xi, xj])).cuda()
    gc, bc = torch.ones(2048).cuda().requires_grad_(True), torch.zeros(2048).cuda().requires_grad_(True)
    ptr = torch.tensor([0, 1]).cuda()
    loss = ops.bpr_frozen_loss(table, gc, bc, 0.0, ptr[0:1], ptr[1:2], ptr[1:2].view(1, 1), torch.ones(1).cuda())
    loss.backward()
    loss = loss.detach()
    print(f"loss {float(loss)!r} ln 2 {math.log(2.0)!r}")
    assert float(loss) == float(np.float32(math.log(2.0)))          # fp32 ln 2, bit for bit
    assert not bool(gc.grad.any()) and not bool(bc.grad.any())      # R = G xh_j - G xh_j: exactly 0
    # ... and the same bits as a difference of 0 built from one agreeing and one disagreeing flip
    zero = [p for p in run_probes(64, 1.0, (0,)) if p[4][0] == 0.0]
    assert len(zero) == 1 and zero[0][0] == float(loss)


# ---------------------------------------------------------------------------------------------- C. widths and limits
WIDTHS = [192, 320, 512, 1024, 1088, 1280, 1536, 1792, 1984]      # NV = 1 .. 8; the last slot partly inside the row at 192, 320, 1088, 1984


@pytest.mark.parametrize("dim", WIDTHS)
def test_every_width_template_vs_fp64_restatement(dim):
    prob = cached(("width", dim), lambda: frozen_problem(9, 3, dim, 40))
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = prob
    ref, dg, db, _ = restate_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w)
    loss, gg, gb = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    check_loss(float(loss), ref)
    check_grad(gg, dg, what="dgamma")
    check_grad(gb, db, what="dbeta")
    assert_live_row_identity(prob, 8)


@pytest.mark.parametrize("dim", WIDTHS)
def test_rows_that_differ_in_their_last_64_columns_only(dim):
    """The gradients of the last column block, compared on their own: a dropped tail cannot hide behind a larger element elsewhere."""
    g = torch.Generator().manual_seed(dim)
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = frozen_problem(9, 3, dim, 40)
    table = table[:1].repeat(40, 1)
    table[:, -64:] = torch.randn(40, 64, generator=g) * 2
    ref, dg, db, _ = restate_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w)
    loss, gg, gb = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
    check_loss(float(loss), ref)
    for name, got, want in (("dgamma", gg, dg), ("dbeta", gb, db)):
        got, want = got.cpu().numpy()[-64:].astype(np.float64), want[-64:]
        assert np.abs(want).min() > 0 and np.abs(got).min() > 0, name
        err, top = np.abs(got - want).max(), np.abs(want).max()
        print(f"{name}[-64:] max |got - ref| {err:.3e} of the block's max |ref| {top:.3e}")
        assert err <= 3e-4 * top, name


def test_two_negatives_and_the_most_negatives():
    for B, n_neg, n_rows in ((9, 2, 40), (2, 4096, 300)):
        table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = frozen_problem(B, n_neg, 64, n_rows)
        ref, dg, db, _ = restate_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w)
        loss, gg, gb = run_frozen(table, gamma, beta, EPS, ptr_i, ptr_j, ptr_nj, w, scale=1.0)
        check_loss(float(loss), ref)
        check_grad(gg, dg, what=f"dgamma n_neg {n_neg}")
        check_grad(gb, db, what=f"dbeta n_neg {n_neg}")


class Abi:
    """The C entry points as tests/test_gpu_bpr.py's refusal test calls them, on a small valid problem, with canaries in the outputs."""
    CANARY = -7.25

    def __init__(self, B=20, n_neg=3, dim=128, n_rows=40):
        from ccrec_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        table, gamma, beta, ptr_i, ptr_j, ptr_nj, w = frozen_problem(B, n_neg, dim, n_rows)
        self.B, self.n_neg, self.dim, self.n_rows = B, n_neg, dim, n_rows
        self.big = torch.zeros(n_rows * dim + 4, device="cuda")                  # the table also as a view that starts at element 1
        self.big[1:1 + n_rows * dim] = table.reshape(-1).cuda()
        self.table = table.cuda()
        self.gb = torch.stack([gamma, beta]).cuda()
        self.pi, self.pj, self.pnj, self.w = ptr_i.cuda(), ptr_j.cuda(), ptr_nj.cuda(), w.cuda()
        self.ws_bytes = int(self.lib.ccr_bpr_frozen_workspace_bytes(B, n_neg, dim))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.one = torch.ones(1, device="cuda")
        self.out3 = torch.full((3,), self.CANARY, device="cuda")
        self.grads = torch.full((2 * dim + 4,), self.CANARY, device="cuda")

    @staticmethod
    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def fwd(self, table=None, B=None, n_neg=None, dim=None, n_rows=None, ws="own", ws_bytes=None):
        p = self.p
        return self.lib.ccr_bpr_frozen_fwd(p(self.table if table is None else table), self.n_rows if n_rows is None else n_rows,
                                           self.dim if dim is None else dim, p(self.gb[0]), p(self.gb[1]), EPS, p(self.pi), p(self.pj), p(self.pnj),
                                           p(self.w), self.B if B is None else B, self.n_neg if n_neg is None else n_neg, p(self.out3),
                                           p(self.ws) if ws == "own" else ws, self.ws_bytes if ws_bytes is None else ws_bytes, None)

    def bwd(self, table=None, B=None, n_neg=None, dim=None, n_rows=None, ws="own", ws_bytes=None, grad_offset=0):
        p = self.p
        dgamma = self.grads[grad_offset:grad_offset + self.dim]
        dbeta = self.grads[self.dim:2 * self.dim]
        return self.lib.ccr_bpr_frozen_bwd_dev(p(self.table if table is None else table), self.n_rows if n_rows is None else n_rows,
                                               self.dim if dim is None else dim, p(self.gb[0]), p(self.gb[1]), EPS, p(self.pi), p(self.pj),
                                               p(self.pnj), p(self.w), self.B if B is None else B, self.n_neg if n_neg is None else n_neg,
                                               p(self.one), p(self.one), p(dgamma), p(dbeta), p(self.ws) if ws == "own" else ws,
                                               self.ws_bytes if ws_bytes is None else ws_bytes, None)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out3 == self.CANARY).all()) and bool((self.grads == self.CANARY).all())

    def error(self):
        return self.lib.ccr_last_error()


def test_refusals_through_the_c_abi_leave_the_outputs_untouched():
    a = Abi()
    L = a._lib
    view = a.big[1:1 + a.n_rows * a.dim]
    assert view.data_ptr() % 16 == 4
    refusals = [
        ("workspace one byte short", L.CCR_ERR_WORKSPACE, b"workspace", dict(ws_bytes=a.ws_bytes - 1)),
        ("null workspace", L.CCR_ERR_WORKSPACE, b"workspace", dict(ws=None)),
        ("table offset by 4 bytes", L.CCR_ERR_INVALID, b"aligned", dict(table=view)),
        ("B = 0", L.CCR_ERR_INVALID, b"B=0", dict(B=0)),
        ("n_rows = 0", L.CCR_ERR_INVALID, b"empty table", dict(n_rows=0)),
        ("dim 2112", L.CCR_ERR_INVALID, b"dim=2112", dict(dim=2112)),
        ("n_neg 4097", L.CCR_ERR_INVALID, b"n_neg=4097", dict(n_neg=4097)),
    ]
    for what, code, word, kw in refusals:
        for name, call in (("fwd", a.fwd), ("bwd", a.bwd)):
            rc = call(**kw)
            assert rc == code and word in a.error(), (what, name, rc, a.error())
            assert a.untouched(), (what, name)
    rc = a.bwd(grad_offset=1)                                                     # dgamma offset by 4 bytes
    assert rc == L.CCR_ERR_INVALID and b"aligned" in a.error() and a.untouched()
    assert a.lib.ccr_bpr_frozen_workspace_bytes(a.B, 4097, a.dim) == 0 and a.lib.ccr_bpr_frozen_workspace_bytes(a.B, 4096, a.dim) > 0
    assert a.lib.ccr_bpr_frozen_workspace_bytes(a.B, a.n_neg, 2112) == 0 and a.lib.ccr_bpr_frozen_workspace_bytes(0, a.n_neg, a.dim) == 0
    # the same arguments without the fault are accepted and write the outputs
    assert a.fwd() == L.CCR_OK and a.bwd() == L.CCR_OK
    torch.cuda.synchronize()
    assert bool((a.out3 != a.CANARY).all()) and bool((a.grads[:2 * a.dim] != a.CANARY).all()) and bool((a.grads[2 * a.dim:] == a.CANARY).all())


def test_more_than_4096_negatives_are_refused_by_the_op():
    from ccrec_amd import _lib, ops
    table, gamma, beta, ptr_i, ptr_j, _, w = frozen_problem(2, 1, 64, 10)
    with pytest.raises(_lib.CcrError, match="4096"):
        ops.bpr_frozen_loss(table.cuda(), gamma.cuda(), beta.cuda(), EPS, ptr_i.cuda(), ptr_j.cuda(), torch.zeros(4097, 2, dtype=torch.int64).cuda(), w.cuda())


# ---------------------------------------------------------------------------------------------- D. sampler
def prior_from_rows(rows):
    """rows: one (columns, values) per user -> (ptr, idx, t) as make_prior returns them."""
    ptr = np.cumsum([0] + [len(c) for c, _ in rows]).astype(np.int64)
    idx = np.concatenate([np.asarray(c, np.int64) for c, _ in rows]) if rows else np.zeros(0, np.int64)
    t = np.concatenate([np.asarray(v, np.float32) for _, v in rows]) if rows else np.zeros(0, np.float32)
    return ptr, idx, t


def integer_proposal(n_items, seed, zeros=()):
    """sqrt(integer + 0.1) in fp32 (every partial sum of a few thousand of them is exact in fp64), exact zeros on the given slices."""
    rng = np.random.default_rng(seed)
    proposal = ((rng.integers(0, 50, n_items) + 0.1) ** 0.5).astype(np.float32)
    for s in zeros:
        proposal[s] = 0.0
    return proposal


@pytest.mark.parametrize("n_neg", [64, 65, 200, 4096])
def test_sampler_many_draws_per_row(n_neg):
    n_items = 3000
    prior = make_prior(3, n_items, lambda u: (0, 5, 100)[u], lambda rng, m: rng.normal(size=m) * 2, seed=20)
    users = np.arange(3)
    got, proposal, cdf, uniforms = run_sampler(users, n_neg, n_items, prior, 0.0, seed=n_neg)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    assert n_neg == 64 or len(np.unique(got[64:])) > 1               # (the draws beyond a lane's first are draws, not a fill)


def test_sampler_scan_group_edges():
    lens = [63, 64, 65, 100, 127, 128, 129, 4095]
    prior = make_prior(len(lens), 5000, lambda u: lens[u], lambda rng, m: rng.normal(size=m) * 2, seed=21)
    users = np.arange(len(lens))
    got, proposal, cdf, uniforms = run_sampler(users, 8, 5000, prior, 0.0, seed=21)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)


def test_sampler_marks_a_row_longer_than_the_caller_said():
    from ccrec_amd import ops
    n_items, n_neg = 500, 6
    prior = make_prior(3, n_items, lambda u: (3, 70, 5)[u], lambda rng, m: rng.normal(size=m) * 2, seed=22)
    users = np.array([0, 1, 2, 1, 0])
    rng = np.random.default_rng(22)
    proposal = integer_proposal(n_items, 22)
    uniforms = rng.random((n_neg, len(users)))
    prop = torch.from_numpy(proposal).cuda()
    cdf = ops.bpr_proposal_cdf(prop)
    dev_prior = tuple(torch.from_numpy(a).cuda() for a in prior) + (64,)              # max_row_nnz = 64 < 70
    got = ops.bpr_sample_negatives(torch.from_numpy(users).cuda(), n_neg, prop, cdf, prior=dev_prior, t0=0.0,
                                   uniforms=torch.from_numpy(uniforms).cuda()).cpu().numpy()
    assert (got[:, [1, 3]] == -1).all()
    keep = [0, 2, 4]                                                                  # the user before and the user after: the reference's draws
    check_draws(got[:, keep], users[keep], prior, 0.0, proposal, cdf.cpu().numpy(), uniforms[:, keep])


def test_sampler_row_corner_cases():
    n_items = 300
    rng = np.random.default_rng(23)
    val = lambda m: rng.normal(size=m) * 2
    rows = [([0, n_items - 1], val(2)),                                               # the first and the last column
            ([0], val(1)), ([n_items - 1], val(1)),
            (list(range(10, 20)) + list(range(100, 103)) + [298, 299], val(15)),       # runs of adjacent columns
            (list(range(n_items)), val(n_items)),                                      # every item stored
            (list(range(n_items)), np.full(n_items, 1.5))]                             # ... all with one value: the proposal again
    prior = prior_from_rows(rows)
    users = np.arange(len(rows))
    got, proposal, cdf, uniforms = run_sampler(users, 40, n_items, prior, 0.0, seed=23)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    edges = np.stack([np.zeros(len(rows)), np.full(len(rows), LAST_U)])
    got, proposal, cdf, _ = run_sampler(users, 2, n_items, prior, 0.0, uniforms=edges, seed=23)
    assert (got[0] == 0).all() and (got[1] == n_items - 1).all()


@pytest.mark.parametrize("with_prior", [False, True])
def test_sampler_one_item(with_prior):
    prior = prior_from_rows([([0], [1.5]), ([], []), ([0], [-3.0])]) if with_prior else None
    users = np.array([0, 1, 2, 0])
    got, proposal, cdf, uniforms = run_sampler(users, 5, 1, prior, 0.0, seed=24)
    assert (got == 0).all()
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    edges = np.stack([np.zeros(4), np.full(4, LAST_U)])
    got, *_ = run_sampler(users, 2, 1, prior, 0.0, uniforms=edges, seed=24)
    assert (got == 0).all()


@pytest.mark.parametrize("case", ["no_prior", "prior"])
def test_sampler_zeros_in_the_proposal(case):
    """Runs of exact zeros at the head, in the middle and at the tail: no draw names an item of weight 0 (check_draws refuses one)."""
    n_items, n_users = 400, 6
    zeros = (slice(0, 7), slice(150, 190), slice(391, 400))
    proposal = integer_proposal(n_items, 25, zeros)
    prior = None
    if case == "prior":                                            # entries partly on the zero items: 0 .. 9, 140 .. 159, 385 .. 399, and elsewhere
        rng = np.random.default_rng(25)
        rows = []
        for u in range(n_users):
            cols = np.unique(np.concatenate([np.arange(0, 10, 1 + u % 2), np.arange(140, 160), np.arange(385, 400, 1 + u % 3), rng.choice(n_items, 10 * u)]))
            rows.append((cols, rng.normal(size=len(cols)) * 2))
        prior = prior_from_rows(rows)
    users = np.arange(n_users)
    got, prop, cdf, uniforms = run_sampler(users, 50, n_items, prior, 0.0, seed=25, proposal=proposal)
    assert np.array_equal(prop, proposal)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    assert (proposal[got] > 0).all()
    edges = np.stack([np.zeros(n_users), np.full(n_users, LAST_U)])
    got, _, cdf, _ = run_sampler(users, 2, n_items, prior, 0.0, uniforms=edges, seed=25, proposal=proposal)
    assert (got[0] == 7).all() and (got[1] == 390).all()      # the first and the last item of non-zero weight
    check_draws(got, users, prior, 0.0, proposal, cdf, edges)


def excluding_rows(n_items, pure):
    """Stored entries of t = -1e5 (weight exactly 0 while t0 = 0 keeps e0 = 1) in a block at the head, one in the middle and one at the tail.
    pure: nothing else is stored, so every sum of the kernel is exact; otherwise ordinary entries (t <= 0: e0 stays 1) lie among them."""
    rng = np.random.default_rng(26 + pure)
    rows = []
    for u in range(6):
        head, mid, tail = np.arange(0, 3 + 20 * u), np.arange(1000, 1040 + 7 * u), np.arange(n_items - 5 - 30 * u, n_items)
        blocks = [b for b, on in zip((head, mid, tail), ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1))[u]) if on]
        cols = np.concatenate(blocks)
        t = np.full(len(cols), -1e5)
        if not pure:
            free = np.setdiff1d(np.arange(n_items), cols)
            more = rng.choice(free, 25 + 10 * u, replace=False)
            cols, t = np.concatenate([cols, more]), np.concatenate([t, -np.abs(rng.normal(size=len(more))) * 2])
            order = np.argsort(cols)
            cols, t = cols[order], t[order]
        rows.append((cols, t))
    return prior_from_rows(rows)


@pytest.mark.parametrize("pure", [True, False])
def test_sampler_excluding_prior(pure):
    """Random uniforms and both edge uniforms.  Among ordinary entries the kernel's prefix sums are rounded and F of an excluded entry may
    come out a spacing above the last live item's: the draw must still be the live item (the kernel steps off an item of weight 0)."""
    n_items, n_users = 3000, 6
    proposal = integer_proposal(n_items, 27)
    prior = excluding_rows(n_items, pure)
    users = np.arange(n_users)
    got, _, cdf, uniforms = run_sampler(users, 100, n_items, prior, 0.0, seed=27, proposal=proposal)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    ptr, idx, t = prior
    for b, u in enumerate(users):
        assert not np.isin(got[:, b], idx[ptr[u]:ptr[u + 1]][t[ptr[u]:ptr[u + 1]] == -1e5]).any()
    edges = np.stack([np.zeros(n_users), np.full(n_users, LAST_U)])
    got, _, cdf, _ = run_sampler(users, 2, n_items, prior, 0.0, uniforms=edges, seed=27, proposal=proposal)
    check_draws(got, users, prior, 0.0, proposal, cdf, edges)
    live = [np.nonzero(dense_weights(u, prior, 0.0, proposal))[0] for u in users]
    assert np.array_equal(got[0], [nz[0] for nz in live]) and got[0, 0] == 3 and got[0, 2] == 0
    last = np.array([nz[-1] for nz in live])
    assert last[0] == n_items - 6 and last[1] == n_items - 1
    assert np.array_equal(got[1], last)


def test_sampler_t0_of_3_over_empty_rows():
    n_items = 700
    prior = make_prior(6, n_items, lambda u: 0 if u % 2 else 9, lambda rng, m: rng.normal(size=m), seed=28)
    users = np.array([1, 3, 5, 3])
    got, proposal, cdf, uniforms = run_sampler(users, 30, n_items, prior, 3.0, seed=28)
    check_draws(got, users, prior, 3.0, proposal, cdf, uniforms)
    check_draws(got, users, None, 0.0, proposal, cdf, uniforms)      # ... which are the draws from the proposal alone


@pytest.mark.parametrize("B,n_neg", [(4100, 1), (10000, 2)])
@pytest.mark.parametrize("with_prior", [False, True])
def test_sampler_batches_in_the_thousands(B, n_neg, with_prior):
    n_users, n_items = 37, 257
    prior = make_prior(n_users, n_items, lambda u: (u * 5) % 70, lambda rng, m: rng.normal(size=m) * 2, seed=29) if with_prior else None
    users = np.random.default_rng(B).integers(0, n_users, B)
    got, proposal, cdf, uniforms = run_sampler(users, n_neg, n_items, prior, 0.0, seed=B)
    check_draws(got, users, prior, 0.0, proposal, cdf, uniforms)
    for u in (0, 1, 36):                                          # a user that appears a hundred times and more: other uniforms, other draws
        mine = got[:, users == u]
        assert mine.shape[1] > 50 and len(np.unique(mine)) > 20


def test_sampler_out_of_range_columns_and_a_nan_uniform():
    n_items, n_neg = 200, 20
    prior = make_prior(4, n_items, lambda u: 6, lambda rng, m: rng.normal(size=m), seed=30)
    ptr, idx, t = prior
    broken = idx.copy()
    broken[ptr[1]] = -5                                           # the kernel clamps a stored column for addressing
    broken[ptr[2 + 1] - 1] = n_items + 10
    users = np.arange(4)
    got, proposal, cdf, uniforms = run_sampler(users, n_neg, n_items, (ptr, broken, t), 0.0, seed=30)
    assert (got >= 0).all() and (got < n_items).all()
    check_draws(got[:, [0, 3]], users[[0, 3]], prior, 0.0, proposal, cdf, uniforms[:, [0, 3]])
    uniforms = uniforms.copy()
    uniforms[3, 0] = uniforms[5, 3] = float("nan")
    got2, *_ = run_sampler(users, n_neg, n_items, prior, 0.0, uniforms=uniforms, seed=30)
    assert (got2 >= 0).all() and (got2 < n_items).all()
    ok = ~np.isnan(uniforms)
    assert np.array_equal(got2[:, [0, 3]][ok[:, [0, 3]]], got[:, [0, 3]][ok[:, [0, 3]]])
